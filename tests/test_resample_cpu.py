"""CPU tests of the resampler (wavthruvec_pytorch_amd/audio.py, csrc/v2w_resample.hip): the filter table against the independent restatement
of tests/resample_ref.py and against the issue's figures, resampled_length, the C ABI surface, the plan, what the entry points refuse (through
the dry-run stream), what the name sink reports, synthesize's --out-rate and the Python errors.  No GPU needed: nothing is launched."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

from tests import resample_ref as RR
from wavthruvec_pytorch_amd import _hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('v2w_resample_plan', 'v2w_resample', 'v2w_peak_scale')
FAKE = 0x7f0000100000       # aligned "device" pointers: the plan, the dry run and the name sink never dereference them
DRY = C.c_void_p(-1)


# ---------------------------------------------------------------------------------------------------------------
# the filter
@pytest.mark.parametrize('rate', sorted(RR.TABLE), ids=RR.rid)
def test_table_matches_the_restatement_and_the_listed_figures(rate):
    from wavthruvec_pytorch_amd import audio, resample_table
    assert audio.resample_table is resample_table
    t = resample_table(*rate)
    M, L, NT, kmin, kmax = RR.TABLE[rate]
    assert (t['M'], t['L'], t['NT']) == (M, L, NT) == (*RR.ratio(*rate), RR.nt_closed(M, L))
    k0, h = t['k0'], t['h']
    assert h.dtype == np.float64 and h.shape == (L, NT) and k0.shape == (L,)
    if kmin is not None:
        assert (int(k0.min()), int(k0.max()) + NT - 1) == (kmin, kmax)
    assert [int(v) for v in k0] == [RR.k0_closed(p, M, L) for p in range(L)]
    assert (np.diff(k0) >= 0).all() and k0[-1] - k0[0] <= M                   # what the kernel's window relies on
    k = k0[:, None] + np.arange(NT)[None, :]
    want = RR.coeff(np.arange(L)[:, None], k, M, L)
    assert np.abs(h - want).max() <= 1e-12
    # nothing outside the run: the restatement's coefficients one reach to either side of it are exactly 0
    R = RR.reach(M, L)
    for side in (k0[:, None] - 1 - np.arange(R)[None, :], k0[:, None] + NT + np.arange(R)[None, :]):
        assert not RR.coeff(np.arange(L)[:, None], side, M, L).any()
    sums = h.sum(axis=1)
    assert 1.00003 <= sums.min() and sums.max() <= 1.0009, (sums.min(), sums.max())


def test_table_applied_equals_the_per_sample_restatement():
    """The (k0, h) form against the restatement that has no table, on random input: the issue's 1.4e-15 agreement, held to 1e-13."""
    from wavthruvec_pytorch_amd import resample_table
    for rate, n in (((44100, 16000), 3000), ((16000, 44100), 700), ((8, 3), 200), ((5, 7), 100), ((16000, 48000), 50)):
        t = resample_table(*rate)
        x = np.random.default_rng(3).standard_normal(n)
        a, _ = RR.apply_table(x, t['h'], t['k0'], t['M'], t['L'])
        b, _ = RR.resample(x, *rate)
        assert a.shape == b.shape == (RR.length(n, *rate),) and np.abs(a - b).max() <= 1e-13, rate


def test_resampled_length():
    from wavthruvec_pytorch_amd import resampled_length
    for orig, new in sorted(RR.TABLE):
        M, L = RR.ratio(orig, new)
        for n in (1, 2, 3, 159, 160, 161, 440, 441, 442, 81920, 2 ** 31 - 1, 2 ** 31 // max(L, 1) + 1, 10 ** 12 + 7):
            want = (n * L + M - 1) // M
            assert resampled_length(n, orig, new) == want == RR.length(n, orig, new), (orig, new, n)
            assert (want - 1) * M < n * L <= want * M                        # ceil, in integers
    assert resampled_length(1, 44100, 16000) == 1 and resampled_length(1, 16000, 48000) == 3
    assert resampled_length(13_000_000, 16000, 44100) == math.ceil(13_000_000 * 441 / 160)           # n * L = 5.7e9 > 2^31
    for bad in ((0, 1), (1, 0), (1.5, 2), (-3, 3)):
        with pytest.raises(ValueError):
            resampled_length(10, *bad)


# ---------------------------------------------------------------------------------------------------------------
# the C ABI
def test_entry_points_are_declared_bound_and_additive():
    hdr = open(os.path.join(ROOT, 'include', 'vec2wav_hip.h')).read()
    assert int(re.search(r'#define V2W_ABI_VERSION (\d+)', hdr).group(1)) == _hip.ABI_VERSION == 35 == _hip.load().v2w_abi_version()
    args = {n: re.search(r'\bint\s+%s\s*\(([^)]*)\)\s*;' % n, hdr).group(1).split(',') for n in NAMES}
    ctype = {'int': C.c_int, 'float': C.c_float}
    for name in NAMES:
        res, sig = _hip.SIGNATURES[name]
        assert res is C.c_int and len(sig) == len(args[name]), name
        for a, s in zip(args[name], sig):
            a = a.strip()
            if 'v2w_resample_grids*' in a:
                assert s is C.POINTER(_hip.ResampleGrids), (name, a)
            elif '*' in a:
                assert s is C.c_void_p, (name, a)
            else:
                assert s is ctype[a.split()[0]], (name, a)
        assert (name in _hip.LAUNCHERS) == (name != 'v2w_resample_plan'), name
    body = hdr[:hdr.index('} v2w_resample_grids;')]
    body = re.sub(r'/\*.*?\*/', '', body[body.rindex('typedef struct {'):], flags=re.S)
    assert re.findall(r'\b(\w+)\s*[;,]', body) == [n for n, _ in _hip.ResampleGrids._fields_]
    assert C.sizeof(_hip.ResampleGrids) == 16
    from wavthruvec_pytorch_amd import build
    assert 'v2w_resample.hip' in build.SOURCES


def _plan(lib, M, L, NT, B=1, Lout=100000):
    g = _hip.ResampleGrids()
    return lib.v2w_resample_plan(M, L, NT, B, Lout, C.byref(g)), g


def _lds_restated(M, L, NT, T):
    return 4 * (L * (NT | 1) + L + ((T - 1) // L + 2) * M + NT + 4)


@pytest.mark.parametrize('rate', sorted(RR.TABLE), ids=RR.rid)
def test_plan_matches_the_headers_statement(rate):
    lib = _hip.load()
    M, L, NT = RR.TABLE[rate][:3]
    for B, Lout in ((1, 1), (3, 4095), (3, 4096), (32, 160000), (2, 2 ** 31 - 1)):
        rc, g = _plan(lib, M, L, NT, B, Lout)
        assert rc == 0
        fits = [T for T in (4096, 2048, 1024, 512, 256) if _lds_restated(M, L, NT, T) <= 65536]
        assert g.tile == fits[0] and g.lds_bytes == _lds_restated(M, L, NT, g.tile) <= 65536
        assert g.tiles == -(-Lout // g.tile) and g.grid == B * g.tiles
    assert _plan(lib, 441, 160, 34)[1].tile == 2048 and _plan(lib, 160, 441, 13)[1].tile == 4096


def test_plan_rejects_what_does_not_fit():
    from wavthruvec_pytorch_amd import resample_table
    lib = _hip.load()
    E_ARG, E_SHAPE = _hip.E_ARG, _hip.E_SHAPE
    M, L = RR.ratio(16000, 44101)                                           # coprime rates: 44101 phases of 13 taps
    assert (M, L) == (16000, 44101) and _plan(lib, M, L, 13)[0] == E_SHAPE
    assert _plan(lib, 44101, 16000, 34)[0] == E_SHAPE
    # the header's limit at the smallest tile, from both sides
    for M, L, NT in ((441, 160, 34), (7000, 1, 13), (1, 1000, 13), (3, 400, 37)):
        ok = L * ((NT | 1) + 1) + (255 // L + 2) * M + NT + 4 <= 16384
        assert (_plan(lib, M, L, NT)[0] == 0) == ok, (M, L, NT)
    most = max(L for L in range(1000, 1300) if L * 14 + 2 + 13 + 4 <= 16384)       # M = 1, NT = 13: the last L that fits
    assert _plan(lib, 1, most, 13)[0] == 0 and _plan(lib, 1, most + 1, 13)[0] == E_SHAPE
    assert _plan(lib, 1, 3, 13, B=2 ** 20, Lout=2 ** 31 - 1)[0] == E_SHAPE      # B * tiles past 2^31 - 1
    for bad in ((0, 3, 13, 1, 10), (1, 0, 13, 1, 10), (1, 3, 0, 1, 10), (1, 3, 13, 0, 10), (1, 3, 13, 1, 0), (-1, 3, 13, 1, 10)):
        g = _hip.ResampleGrids()
        assert lib.v2w_resample_plan(*bad, C.byref(g)) == E_ARG, bad
    assert lib.v2w_resample_plan(1, 3, 13, 1, 10, None) == E_ARG
    t = resample_table(48000, 44100)
    assert _plan(lib, t['M'], t['L'], t['NT'])[0] == 0                       # 160 : 147 fits


def _rs(lib, stream=DRY, **kw):
    a = dict(x=FAKE, in_i16=0, y=FAKE + 0x10000000, B=3, Lin=1000, Lout=363, h=FAKE + 0x20000000, k0=FAKE + 0x30000000, M=441, L=160, NT=34,
             len=FAKE + 0x40000000, peak_part=FAKE + 0x50000000)
    a.update(kw)
    return lib.v2w_resample(a['x'], a['in_i16'], a['y'], a['B'], a['Lin'], a['Lout'], a['h'], a['k0'], a['M'], a['L'], a['NT'], a['len'],
                            a['peak_part'], stream)


def _ps(lib, stream=DRY, **kw):
    a = dict(y=FAKE, B=3, Lout=363, peak_part=FAKE + 0x1000, parts=1, peak=0.95)
    a.update(kw)
    return lib.v2w_peak_scale(a['y'], a['B'], a['Lout'], a['peak_part'], a['parts'], a['peak'], stream)


def test_entry_points_refuse_bad_arguments_through_the_dry_run():
    lib = _hip.load()
    E_ARG, E_SHAPE = _hip.E_ARG, _hip.E_SHAPE
    assert _rs(lib) == 0 and _rs(lib, len=None, peak_part=None) == 0 and _rs(lib, in_i16=1) == 0
    assert -(-1000 * 160 // 441) == 363
    assert _rs(lib, Lout=362) == E_ARG and _rs(lib, Lout=364) == 0          # Lout < ceil(L * Lin / M)
    for null in ('x', 'y', 'h', 'k0'):
        assert _rs(lib, **{null: None}) == E_ARG, null
    for size in ('B', 'Lin', 'Lout', 'M', 'L', 'NT'):
        assert _rs(lib, **{size: 0}) == E_ARG and _rs(lib, **{size: -1}) == E_ARG, size
    for ptr in ('x', 'y', 'h', 'k0', 'len', 'peak_part'):
        assert _rs(lib, **{ptr: FAKE + 0x100002}) == E_ARG, ptr             # 2 bytes off a float / an int32
    assert _rs(lib, x=FAKE + 2, in_i16=1) == 0 and _rs(lib, x=FAKE + 1, in_i16=1) == E_ARG
    assert _rs(lib, M=16000, L=44101, NT=13, Lin=10, Lout=28) == E_SHAPE
    assert _rs(lib, Lin=2 ** 31 - 1, Lout=2 ** 31 - 1, B=4096) == E_SHAPE    # B * tiles
    need = -(-(2 ** 31 - 1) * 160 // 441)                                   # L * Lin passes 2^31: the check is made in 64 bits
    assert _rs(lib, Lin=2 ** 31 - 1, Lout=need - 1) == E_ARG and _rs(lib, Lin=2 ** 31 - 1, Lout=need) == 0
    assert _ps(lib) == 0
    for null in ('y', 'peak_part'):
        assert _ps(lib, **{null: None}) == E_ARG and _ps(lib, **{null: FAKE + 2}) == E_ARG, null
    for size in ('B', 'Lout', 'parts'):
        assert _ps(lib, **{size: 0}) == E_ARG and _ps(lib, **{size: -2}) == E_ARG, size
    for peak in (0.0, -0.95, float('inf'), float('nan')):
        assert _ps(lib, peak=peak) == E_ARG, peak
    assert _ps(lib, B=2 ** 20, Lout=2 ** 31 - 1) == E_SHAPE


def test_name_sink_lists_the_kernels():
    lib = _hip.load()
    a = (FAKE, 0, FAKE, 3, 1000, 363, FAKE, FAKE, 441, 160, 34, FAKE, FAKE)
    rc, names = _hip.kernel_names(lib.v2w_resample, *a)
    assert rc in (0, 100) and names == ['resample_kernel'], names
    rc, names = _hip.kernel_names(lib.v2w_peak_scale, FAKE, 3, 363, FAKE, 1, 0.95)
    assert rc in (0, 100) and names == ['peak_scale_kernel'], names
    assert _hip.kernel_names(lib.v2w_resample, *a[:5], 362, *a[6:]) == (-1, [])
    assert _hip.kernel_names(lib.v2w_peak_scale, FAKE, 3, 363, FAKE, 0, 0.95) == (-1, [])


# ---------------------------------------------------------------------------------------------------------------
# Python
def test_synthesize_takes_out_rate(capsys):
    from wavthruvec_pytorch_amd import synthesize as S
    base = ['--checkpoint', 'c', '--feat', 'a.npy', '--spk-emb', 's.pth', '--out', 'o.wav']
    a = S.parse_args(base)
    assert a.out_rate is None and a.sampling_rate == 16000
    a = S.parse_args(base + ['--out-rate', '48000'])
    assert a.out_rate == 48000 and a.sampling_rate == 16000
    with pytest.raises(SystemExit):
        S.parse_args(base + ['--out-rate', '0'])
    assert "--sampling-rate` is the MODEL's rate" in S.__doc__
    with pytest.raises(SystemExit):
        S.parse_args(['--help'])
    text = ' '.join(capsys.readouterr().out.split())
    assert "the MODEL's sampling rate" in text and '--out-rate' in text


def test_python_errors():
    import wavthruvec_pytorch_amd as W
    from wavthruvec_pytorch_amd import audio
    for name in ('resample', 'resample_table', 'resampled_length', 'peak_normalize'):
        assert getattr(W, name) is getattr(audio, name) and name in W.__all__
    x = torch.zeros(3, 1000)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        audio.resample(x, 44100, 16000)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        audio.resample(x.to(torch.int16), 16000, 48000, lengths=[1000, 1, 500], peak=0.95)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        audio.peak_normalize(x[0])
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        audio.resample(x, 16000, 16000)
    with pytest.raises(NotImplementedError, match='forward only'):
        audio.resample(x.clone().requires_grad_(True), 44100, 16000)
    with torch.no_grad(), pytest.raises(RuntimeError, match='no CPU fallback'):                # (not a gradient question without grad mode)
        audio.resample(x.clone().requires_grad_(True), 44100, 16000)
    for lengths in ([1000, 1], [1000, 0, 500], [1001, 1, 500], torch.tensor([1.0, 2.0, 3.0]), torch.tensor([[1, 2, 3]])):
        with pytest.raises(ValueError, match='lengths'):
            audio.resample(x, 44100, 16000, lengths=lengths)
    for bad in (torch.zeros(2, 3, 4), torch.zeros(3, 10, dtype=torch.float64), torch.zeros(3, 10, dtype=torch.int32), torch.zeros(0, 10),
                torch.zeros(3, 0), np.zeros((3, 10), np.float32)):
        with pytest.raises(ValueError, match='resample: '):
            audio.resample(bad, 44100, 16000)
    for rates in ((0, 16000), (16000, -1), (44100.5, 16000)):
        with pytest.raises(ValueError, match='positive integers'):
            audio.resample(x, *rates)
    for peak in (0.0, -1.0, float('nan'), float('inf')):
        with pytest.raises(ValueError, match='peak'):
            audio.resample(x, 44100, 16000, peak=peak)
    with pytest.raises(ValueError, match='lowpass_filter_width'):
        audio.resample_table(44100, 16000, lowpass_filter_width=0)
    with pytest.raises(ValueError, match='rolloff'):
        audio.resample_table(44100, 16000, rolloff=1.5)
