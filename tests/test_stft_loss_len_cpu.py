"""CPU tests of the STFT loss with per-item lengths (csrc/v2w_stft_loss.hip: v2w_stft_loss_multi_len, _len_bwd; stft_loss.py: lengths=,
len_mul=): the C ABI surface, what the entry points refuse (through the dry-run stream) and what the name sink reports, the work split
(the dense call's), the references of tests/stft_loss_len_ref.py against tests/stft_loss_ref.py and against autograd, and the Python errors.
No GPU needed: nothing is launched.  Every test that touches the new symbols or the `lengths` keyword fails without the feature."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from tests import stft_loss_len_ref as LR
from tests import stft_loss_ref as SL
from tests import stft_ref as S
from tests.test_stft_loss_cpu import DRY, FAKE, PLANS, _items, _plan_restated
from wavthruvec_pytorch_amd import _hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('v2w_stft_loss_multi_len', 'v2w_stft_loss_multi_len_bwd')
LEN = FAKE + 0x2000


def _ints(vals):
    return (C.c_int32 * len(vals))(*vals)


def _fwd(lib, arr, n, hop, n_fft, stream=DRY, **kw):
    a = dict(len=LEN, len_mul=1, sc=FAKE, mag=FAKE + 0x100, total=FAKE + 0x200, sums=FAKE + 0x300, scratch=FAKE + 0x1000)
    a.update(kw)
    return lib.v2w_stft_loss_multi_len(arr, n, hop, n_fft, a['len'], a['len_mul'], a['sc'], a['mag'], a['total'], a['sums'], a['scratch'], stream)


def _bwd(lib, arr, n, hop, n_fft, stream=DRY, **kw):
    a = dict(len=LEN, len_mul=1, sums=FAKE, g=(FAKE, FAKE, None, None))
    a.update(kw)
    return lib.v2w_stft_loss_multi_len_bwd(arr, n, hop, n_fft, a['len'], a['len_mul'], a['sums'], *a['g'], stream)


def test_entry_points_are_declared_bound_and_additive():
    hdr = open(os.path.join(ROOT, 'include', 'vec2wav_hip.h')).read()
    lib = _hip.load()
    assert int(re.search(r'#define V2W_ABI_VERSION (\d+)', hdr).group(1)) == _hip.ABI_VERSION == 35 == lib.v2w_abi_version()
    c_types = {'const v2w_stft_loss_item*': C.POINTER(_hip.StftLossItem), 'int': C.c_int, 'const int32_t*': None, 'void*': C.c_void_p,
               'float*': C.c_void_p, 'double*': C.c_void_p, 'const float*': C.c_void_p, 'const double*': C.c_void_p}
    for name in NAMES:
        assert name in _hip.SIGNATURES and name in _hip.LAUNCHERS and hasattr(lib, name), name
        m = re.search(r'\bint\s+%s\s*\((.*?)\);' % name, hdr, flags=re.S)
        assert m, name
        params = [re.sub(r'\s+', ' ', p).strip() for p in m.group(1).split(',')]
        types = [p.rsplit(' ', 1)[0] for p in params]
        names = [p.rsplit(' ', 1)[1] for p in params]
        res, args = _hip.SIGNATURES[name]
        assert res is C.c_int and len(args) == len(types), name
        for t, pn, a in zip(types, names, args):
            want = c_types[t]
            if want is None:                               # hop, n_fft: HOST arrays; len: DEVICE memory
                want = C.c_void_p if pn == 'len' else C.POINTER(C.c_int32)
            assert a is want, (name, pn, t)
        assert names[:6] == ['items', 'n', 'hop', 'n_fft', 'len', 'len_mul'] and names[-1] == 'stream', name
    # the descriptor and the dense entry points are what they were
    assert C.sizeof(_hip.StftLossItem) == 48
    assert _hip.SIGNATURES['v2w_stft_loss_multi'][1] == [C.POINTER(_hip.StftLossItem), C.c_int] + [C.c_void_p] * 6
    assert _hip.SIGNATURES['v2w_stft_loss_multi_bwd'][1] == [C.POINTER(_hip.StftLossItem), C.c_int] + [C.c_void_p] * 6


def _geo_of(shapes):
    """A valid (hop, n_fft) per descriptor."""
    return _ints([4 + i for i in range(len(shapes))]), _ints([8 + 3 * i for i in range(len(shapes))])


@pytest.mark.parametrize('case', sorted(PLANS))
def test_the_split_and_the_scratch_are_the_dense_calls(case):
    """The grids depend on the shapes only: the length-aware calls take the plan and the scratch of v2w_stft_loss_plan / _scratch_bytes (24
    bytes per workgroup of the restated split), whatever the geometry, and the dry run takes what the plan takes."""
    lib = _hip.load()
    shapes = PLANS[case]
    n = len(shapes)
    starts = (C.c_int32 * (n + 1))()
    nwg = lib.v2w_stft_loss_plan(_items(shapes), n, starts)
    assert list(starts) == _plan_restated(shapes) and nwg == starts[-1]
    assert lib.v2w_stft_loss_scratch_bytes(_items(shapes), n) == 24 * nwg
    hop, n_fft = _geo_of(shapes)
    if max(s[4] for s in shapes) <= 65535:
        assert _fwd(lib, _items(shapes), n, hop, n_fft) == 0 and _bwd(lib, _items(shapes), n, hop, n_fft) == 0


def test_entry_points_refuse_what_the_dense_calls_refuse_and_their_own():
    lib = _hip.load()
    ok = SL.SHAPES['tail3']
    nb, F, FP, Cs, B = ok
    E_ARG, E_SHAPE = _hip.E_ARG, _hip.E_SHAPE
    h1, f1 = _ints([4]), _ints([8])

    def both(shapes, n=None, hop=None, n_fft=None, off=0, **kw):
        arr = _items(shapes, off=off)
        n = len(shapes) if n is None else n
        hop = _ints([4] * 9) if hop is None else hop
        n_fft = _ints([8] * 9) if n_fft is None else n_fft
        r = {_fwd(lib, arr, n, hop, n_fft, **kw), _bwd(lib, arr, n, hop, n_fft, **kw)}
        assert len(r) == 1, r
        return r.pop()

    # the dense calls' refusals, with their codes
    assert both([ok] * 8) == 0
    assert both([ok] * 8, n=9) == E_ARG and both([ok], n=0) == E_ARG
    assert _fwd(lib, None, 1, h1, f1) == E_ARG and _bwd(lib, None, 1, h1, f1) == E_ARG
    for bad in ((0, F, FP, Cs, B), (nb, 0, FP, Cs, B), (nb, F, FP, Cs, 0), (nb, F, FP, Cs, -1)):
        assert both([bad]) == E_ARG, bad
    assert both([(nb, 9, 8, Cs, B)]) == E_ARG                       # FP < F
    assert both([(nb, F, FP, 2 * nb - 1, B)]) == E_ARG              # Cs < 2 nb
    assert both([(nb, F, FP, 2 * nb, B)]) == 0
    assert both([(nb, F, 10, Cs, B)]) == E_ARG                      # FP % 4
    assert both([ok], off=4) == E_ARG                               # rows off the 16-byte lines
    assert both([(nb, 1 << 21, 1 << 21, 2 * nb + 1000, 1)]) == E_SHAPE                       # Cs * FP past 2^31 - 1
    assert both([(1025, 1000, 1000, 2112, 1017)]) == E_SHAPE and both([(1025, 1000, 1000, 2112, 1016)]) == 0     # B * Cs * FP
    arr = _items([ok])
    for null in ('spec_x', 'spec_y'):
        a = _items([ok])
        setattr(a[0], null, None)
        assert _fwd(lib, a, 1, h1, f1) == E_ARG and _bwd(lib, a, 1, h1, f1) == E_ARG, null
    a = _items([ok])
    a[0].dspec_x = None
    assert _fwd(lib, a, 1, h1, f1) == 0 and _bwd(lib, a, 1, h1, f1) == E_ARG
    assert _fwd(lib, arr, 1, h1, f1, scratch=None) == E_ARG and _fwd(lib, arr, 1, h1, f1, scratch=FAKE + 4) == E_ARG
    assert _fwd(lib, arr, 1, h1, f1, sc=None, mag=None, total=None, sums=None) == E_ARG
    assert _fwd(lib, arr, 1, h1, f1, sc=None, mag=None, total=None) == 0 and _fwd(lib, arr, 1, h1, f1, sums=FAKE + 4) == E_ARG
    assert _bwd(lib, arr, 1, h1, f1, sums=None) == E_ARG and _bwd(lib, arr, 1, h1, f1, g=(None, None, None, None)) == E_ARG
    assert _bwd(lib, arr, 1, h1, f1, g=(None, None, FAKE, None)) == 0 and _bwd(lib, arr, 1, h1, f1, g=(FAKE + 2, None, None, None)) == E_ARG
    # their own: V2W_E_ARG
    assert both([ok], len=None) == E_ARG
    assert both([ok], len_mul=0) == E_ARG and both([ok], len_mul=-3) == E_ARG and both([ok], len_mul=320) == 0
    assert _fwd(lib, arr, 1, None, f1) == E_ARG and _bwd(lib, arr, 1, None, f1) == E_ARG
    assert _fwd(lib, arr, 1, h1, None) == E_ARG and _bwd(lib, arr, 1, h1, None) == E_ARG
    assert both([ok], hop=_ints([0])) == E_ARG and both([ok], hop=_ints([-1])) == E_ARG
    assert both([ok], hop=_ints([9])) == E_ARG and both([ok], hop=_ints([8])) == 0                      # n_fft < hop; n_fft == hop
    assert both([ok, ok], hop=_ints([4, 9])) == E_ARG                                                   # every resolution is looked at
    # V2W_E_SHAPE: B > 65535, F * hop + n_fft past 2^31 - 1
    assert both([(1, 4, 4, 2, 65536)]) == E_SHAPE and both([(1, 4, 4, 2, 65535)]) == 0
    big = (1, 1 << 20, 1 << 20, 2, 1)
    assert both([big], hop=_ints([2047]), n_fft=_ints([2048])) == 0                                      # 2^20 * 2047 + 2048 = 2^31 - 2^20 + 2048
    assert both([big], hop=_ints([2048]), n_fft=_ints([2048])) == E_SHAPE
    assert both([ok, big], hop=_ints([4, 2048]), n_fft=_ints([8, 2048])) == E_SHAPE
    # an argument error of the dense call comes before a shape error of the lengths
    assert both([(nb, F, 10, Cs, 65536)]) == E_ARG


def test_name_sink_lists_the_length_aware_kernels():
    lib = _hip.load()
    shapes = [SL.SHAPES[s] for s in SL.KERNEL_CASES['mixed']]
    arr = _items(shapes)
    hop, n_fft = _geo_of(shapes)
    rc, names = _hip.kernel_names(lib.v2w_stft_loss_multi_len, arr, 3, hop, n_fft, LEN, 2, FAKE, FAKE, FAKE, FAKE, FAKE)
    assert rc in (0, 100) and names == ['stft_loss_sums_len_kernel', 'stft_loss_finish_len_kernel'], names
    rc, names = _hip.kernel_names(lib.v2w_stft_loss_multi_len_bwd, arr, 3, hop, n_fft, LEN, 2, FAKE, FAKE, FAKE, None, None)
    assert rc in (0, 100) and names == ['stft_loss_bwd_len_kernel'], names
    assert _hip.kernel_names(lib.v2w_stft_loss_multi_len, arr, 3, hop, n_fft, None, 2, FAKE, FAKE, FAKE, FAKE, FAKE) == (-1, [])
    # the dense calls launch what they launched
    rc, names = _hip.kernel_names(lib.v2w_stft_loss_multi, arr, 3, FAKE, FAKE, FAKE, FAKE, FAKE)
    assert names == ['stft_loss_sums_kernel', 'stft_loss_finish_kernel'], names


# ---------------------------------------------------------------------------------------------------------------
# the references
WANT_FB = dict(one_frame=[[0, 1, 1]], tail2=[[6, 2, 0]], tail3=[[3, 7, 1, 5]], nb1025=[[9, 0, 6]], odd=[[1, 5, 3]],
               mixed=[[5, 1, 7], [9, 3, 9], [1, 0, 1]], full=[[7, 7, 7], [9, 9, 9], [1, 1, 1]], none=[[0, 0, 0], [0, 0, 0]])


def test_frame_counts_of_the_kernel_cases_and_the_host_formula():
    """The cases hold the counts the issue lists - 0, 1, F_b % 4 in {1, 2, 3}, F itself, a count clamped from above F - and `frames` is
    mel.mel_frames."""
    from wavthruvec_pytorch_amd import mel
    assert set(WANT_FB) == set(LR.CASES)
    seen = set()
    for name, c in LR.CASES.items():
        got = []
        for s, (hop, n_fft) in zip(c['shapes'], c['geo']):
            F = LR.SHAPES[s][1]
            fb = LR.item_frames(c['lens'], c['len_mul'], hop, n_fft, F)
            got.append(fb)
            for n, f in zip(c['lens'], fb):
                raw = LR.frames(max(n * c['len_mul'], 0), hop, n_fft)
                assert f == min(raw, F)
                seen |= {'zero'} if f == 0 else set()
                seen |= {'one'} if f == 1 and F > 1 else set()
                seen |= {'mod%d' % (f % 4)} if 0 < f < F else set()
                seen |= {'F'} if f == raw == F else set()
                seen |= {'clamped'} if raw > F else set()
        assert got == WANT_FB[name], (name, got)
    assert seen >= {'zero', 'one', 'mod1', 'mod2', 'mod3', 'F', 'clamped'}, seen
    for n_fft, hop in ((8, 4), (8, 2), (6, 3), (16, 8), (128, 25), (2048, 240), (128, 128)):
        for n in list(range(0, 40)) + [127, 128, 129, 1000, 5000]:
            assert LR.frames(n, hop, n_fft) == mel.mel_frames(n, n_fft, hop), (n_fft, hop, n)


@pytest.mark.parametrize('case', sorted(LR.CASES))
def test_the_masked_statement_is_autograd_through_the_oracles_formulas(case):
    """Reference (a) with lengths against stft_loss_ref.loss_of_spectra in fp64 on the valid entries joined along the frame axis; both
    gradient inputs at once; zero value and zero bound at every masked entry.  case_specs itself asserts the cap on unsigned entries."""
    specs = LR.case_specs(case)
    n = len(specs)
    g_sc, g_mag = SL.g_of(0.75, 0.5, n), SL.g_of(-1.25, None, n)
    for (nb, F, FP, Cs, B), _geo, Fb, sx, sy in specs:
        v, b = LR.sums(sx, sy, F, nb, Fb)
        dre, dim, bre, bim, unsure = LR.dspec(sx, sy, F, nb, Fb, v['Sd'], v['Sy'], v['N'], g_sc, g_mag)
        keep = LR.keep_of(Fb, nb, F)
        assert v['N'] == nb * sum(Fb)
        assert all(np.isfinite(a).all() for a in (dre, dim, bre, bim))
        assert not dre[~keep].any() and not bre[~keep].any() and not dim[~keep].any() and not bim[~keep].any() and not unsure[~keep].any()
        if not v['N']:
            assert not any(v.values()) and not any(b.values()) and not dre.any() and not dim.any()
            continue
        assert all(0 < b[k] < 1e-4 * v[k] for k in ('Sd', 'Sy', 'Sl', 'sc', 'mag'))
        cols = [(i, f) for i, f in enumerate(Fb) if f]
        t = [torch.from_numpy(np.concatenate([np.asarray(a[i:i + 1, r0:r0 + nb, :f], dtype=np.float64) for i, f in cols], axis=2))
             for a, r0 in ((sx, 0), (sx, nb), (sy, 0), (sy, nb))]
        t[0].requires_grad_(True)
        t[1].requires_grad_(True)
        sc, mag = SL.loss_of_spectra(*t)
        assert abs(sc.item() - v['sc']) <= 1e-12 * v['sc'] and abs(mag.item() - v['mag']) <= 1e-12 * v['mag']
        (g_sc * sc + g_mag * mag).backward()
        scale = np.abs(dre).max()
        o = 0
        for i, f in cols:
            assert np.abs(dre[i, :, :f] - t[0].grad.numpy()[0, :, o:o + f]).max() <= 1e-12 * scale
            assert np.abs(dim[i, :, :f] - t[1].grad.numpy()[0, :, o:o + f]).max() <= 1e-12 * scale
            o += f
        assert bre.max() < 1e-4 * scale


def test_full_counts_give_the_dense_statement():
    """Every F_b == F: the masked statement is stft_loss_ref's, values and bounds."""
    for (nb, F, FP, Cs, B), _geo, Fb, sx, sy in LR.case_specs('full'):
        assert Fb == [F] * B
        with np.errstate(all='ignore'):
            v0, b0 = SL.sums(sx, sy, F, nb)
            d0 = SL.dspec(sx, sy, F, nb, v0['Sd'], v0['Sy'], 0.75, -1.25)
        v, b = LR.sums(sx, sy, F, nb, Fb)
        d = LR.dspec(sx, sy, F, nb, Fb, v0['Sd'], v0['Sy'], v['N'], 0.75, -1.25)
        assert v['N'] == B * nb * F
        for k in v0:
            assert abs(v[k] - v0[k]) <= 1e-13 * abs(v0[k]) and abs(b[k] - b0[k]) <= 1e-9 * b0[k], k
        for p, q in zip(d, d0):
            assert np.allclose(p, q, rtol=1e-12, atol=0)


def test_the_ragged_oracle_with_full_lengths_is_the_dense_oracle():
    x, y = SL.signals(2, 700)
    res = ((128, 32, 96), (128, 25, 100))
    for dtype, tol in ((torch.float64, 1e-12), (torch.float32, 2e-5)):
        s0, m0, d0 = SL.oracle(x, y, res, dtype, 1.0, 2.0)
        s1, m1, d1 = LR.ragged_oracle(x, y, [700, 700], res, dtype, 1.0, 2.0)
        assert abs(s1 - s0) <= tol * s0 and abs(m1 - m0) <= tol * m0 and np.abs(d1 - d0).max() <= tol * np.abs(d0).max()


def test_the_ragged_oracle_of_one_item_is_the_dense_oracle_of_the_trimmed_signals():
    """The definition the docstrings state: with lengths a B = 1 batch equals the dense loss of y_hat[:, :n], y[:, :n]; and what lies past n_b
    has no effect on the oracle and gets no gradient."""
    x, y = SL.signals(1, 700)
    res = ((128, 48, 128),)
    s0, m0, d0 = SL.oracle(x[:, :411], y[:, :411], res, torch.float64)
    xp, yp = x.copy(), y.copy()
    xp[:, 411:], yp[:, 411:] = np.nan, np.nan
    s1, m1, d1 = LR.ragged_oracle(xp, yp, [411], res, torch.float64)
    close = lambda p, q: abs(p - q) <= 1e-12 * abs(q)  # noqa: E731  (fp64 sums in another order: a few 2^-53 relative)
    assert close(s1, s0) and close(m1, m0) and np.abs(d1[:, :411] - d0).max() <= 1e-12 * np.abs(d0).max() and not d1[:, 411:].any()
    # an item without a frame counts nothing; a resolution without any item contributes 0 to the means
    x3, y3 = SL.signals(3, 700)
    s2, m2, d2 = LR.ragged_oracle(x3, y3, [700, 40, 700], res, torch.float64)
    s3, m3, d3 = LR.ragged_oracle(x3[[0, 2]], y3[[0, 2]], [700, 700], res, torch.float64)
    assert close(s2, s3) and close(m2, m3) and np.abs(d2[[0, 2]] - d3).max() <= 1e-12 * np.abs(d3).max() and not d2[1].any()
    s4, m4, d4 = LR.ragged_oracle(x3, y3, [40, 30, 20], res, torch.float64)
    assert s4 == 0 and m4 == 0 and not d4.any()


def test_end_to_end_case_list():
    """The device test's cases: B = 3 at every stft_ref.SMALL geometry with an item at full L, one without a frame, and each of the other
    listed lengths; the multi-resolution case."""
    from wavthruvec_pytorch_amd import mel
    cases = LR.small_cases()
    assert {c[0][0] for c in cases} == set(S.SMALL)
    for (geo,), L, lens, len_mul, _w in cases:
        g = mel.stft_geometry(*geo)
        Ls = S.lengths_of(geo[0], geo[1], g['pad'])
        assert len(lens) == 3 and L == Ls[-1] and L in lens and set(lens) - {L} - set(Ls) <= {max(g['pad'], 1)} and len_mul == 1
        fb = [S.frames(n, g) for n in lens]
        assert 0 in fb and max(fb) == S.frames(L, g) > 0
    seen = {(c[0][0], n) for c in cases for n in c[2]}
    for geo in S.SMALL:
        g = mel.stft_geometry(*geo)
        assert all((geo, n) in seen for n in S.lengths_of(geo[0], geo[1], g['pad']))
    res, L, lens, len_mul, w_mag = LR.large_case()
    assert res == tuple(S.LARGE) and LR.samples_of(lens, len_mul, L) == [8192, 5000] and w_mag == 2.0


# ---------------------------------------------------------------------------------------------------------------
# the Python surface
def test_python_errors_with_lengths():
    from wavthruvec_pytorch_amd import MultiResolutionSTFTLoss, mel, stft_loss
    a, b = torch.zeros(2, 4096), torch.zeros(2, 4096)
    m = MultiResolutionSTFTLoss()
    bad = [([4096], 1), ([4096, 4096, 4096], 1), (torch.tensor([4096.0, 100.0]), 1), (torch.tensor([True, False]), 1), ([4096, 0], 1),
           (torch.tensor([4096, 0]), 1), ([4097, 5], 1), ([13, 12], 320), ([4096, 4096], 0), (torch.tensor([[4096, 4096]]), 1)]
    for lengths, mul in bad:
        with pytest.raises(ValueError) as e0:
            mel.check_lengths(lengths, 2, 4096, mul)
        with pytest.raises(ValueError) as e1:
            stft_loss.stft_loss(a, b, 512, 50, 240, lengths=lengths, len_mul=mul)
        with pytest.raises(ValueError) as e2:
            m(a.unsqueeze(1), b, lengths=lengths, len_mul=mul)
        with pytest.raises(ValueError) as e3:
            m(a, b, lengths, mul)                          # (positional in the module's forward)
        assert str(e0.value) == str(e1.value) == str(e2.value) == str(e3.value), (lengths, mul)
    # valid lengths reach the device check; the other errors come as before
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        stft_loss.stft_loss(a, b, 512, 50, 240, lengths=[4096, 100])
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        m(a, b, lengths=torch.tensor([12, 1], dtype=torch.int32), len_mul=320)
    with pytest.raises(ValueError, match='one shape'):
        stft_loss.stft_loss(a, torch.zeros(3, 4096), 512, 50, 240, lengths=[4096, 100])
    with pytest.raises(ValueError, match='must not require grad'):
        stft_loss.stft_loss(a, b.clone().requires_grad_(True), 512, 50, 240, lengths=[4096, 100])
    with pytest.raises(TypeError):
        stft_loss.stft_loss(a, b, 512, 50, 240, [4096, 100])                          # keyword-only in the function
    for doc in (stft_loss.stft_loss.__doc__, MultiResolutionSTFTLoss.__doc__):
        assert 'valid entries' in doc and 'B = 1' in doc and 'lengths' in doc
