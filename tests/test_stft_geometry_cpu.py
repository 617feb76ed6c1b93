"""CPU tests of mel_spectrogram's frame geometry (win_size <= n_fft, any 1 <= hop_size <= n_fft): the host-only geometry / weight function of
wavthruvec_pytorch_amd/mel.py against torch.stft in fp64 (oracle/mel_oracle.py's statement), the frame counts, the refusals, the C ABI surface
of the v2w_mel_*_geo entry points (header <-> ctypes, the kernels the name sink reports, what they refuse), and the numpy statements of
tests/stft_ref.py against the ones of tests/mel_ref.py where the two geometries meet.  Nothing is launched.

The bar of the weights: max |S - torch.stft| <= 1e-12 * max |torch.stft| per geometry (both fp64; a frame's sum has at most 2048 terms)."""
import os
import re

import numpy as np
import pytest
import torch

from wavthruvec_pytorch_amd import _hip, mel

from tests import mel_ref as R
from tests import stft_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEO = ('v2w_mel_phases_geo', 'v2w_mel_phases_geo_len', 'v2w_mel_phases_geo_bwd', 'v2w_mel_finish_geo', 'v2w_mel_finish_geo_len',
       'v2w_mel_finish_geo_bwd', 'v2w_l1_masked_geo')
FAKE = 0x7f0000100000
EXTRA = [(1024, 256, 1024), (400, 160, 400), (2048, 300, 1200), (1024, 320, 1024), (64, 1, 64), (64, 64, 1), (7, 3, 5)]


@pytest.mark.parametrize('geo', S.SMALL + S.LARGE + EXTRA, ids=S.gid)
def test_weights_contract_to_torch_stft(geo):
    n_fft, hop, win = geo
    g, w = mel.dft_conv_weights(n_fft, hop, win)
    assert w.dtype == np.float64 and w.shape == (g['k'], g['cp'], g['cs'])
    assert g['pad'] == int((n_fft - hop) / 2) and g['left'] == (n_fft - win) // 2 and g['k'] == -(-win // hop) and g['nb'] == n_fft // 2 + 1
    assert g['cp'] % 32 == 0 and hop <= g['cp'] < hop + 32 and g['cs'] % 64 == 0 and 2 * g['nb'] <= g['cs'] < 2 * g['nb'] + 64
    # zeros on the padding channels, the padding rows and the taps past the window
    assert not w[:, hop:, :].any() and not w[:, :, 2 * g['nb']:].any()
    assert not w.reshape(g['k'], g['cp'], -1)[:, :hop].transpose(2, 0, 1).reshape(g['cs'], -1)[:, win:].any()
    L = max(g['pad'] + 1, n_fft) + 3 * hop + 1
    y = torch.from_numpy(np.random.default_rng(n_fft + hop + win).uniform(-0.5, 0.5, (2, L)))
    yp = torch.nn.functional.pad(y.unsqueeze(1), (g['pad'], g['pad']), mode='reflect').squeeze(1)
    want = torch.stft(yp, n_fft, hop_length=hop, win_length=win, window=torch.hann_window(win, dtype=torch.float64), center=False,
                      return_complex=True)
    got = S.contract(w, g, yp.numpy())
    F = mel.mel_frames(L, n_fft, hop)
    assert got.shape == (2, 2 * g['nb'], F) and want.shape == (2, g['nb'], F) and F == S.frames(L, g) >= 3
    ref = np.concatenate([want.real.numpy(), want.imag.numpy()], 1)
    rel = np.abs(got - ref).max() / np.abs(ref).max()
    print('[stft weights] %s: k %d, %d channels, max |S - torch.stft| = %.2e of max |torch.stft|' % (S.gid(geo), g['k'], g['cp'], rel))
    assert rel <= 1e-12


def test_the_geometries_the_first_entry_points_serve_keep_their_weights():
    """1024 / 256 / 1024 and its like: the rows as they were built before (n_fft / hop taps of hop channels, no `left`), value for value."""
    for n_fft, hop in ((1024, 256), (128, 32), (2048, 512)):
        g, w = mel.dft_conv_weights(n_fft, hop, n_fft)
        assert g['old'] and g['cp'] == hop and g['k'] == n_fft // hop and g['left'] == 0
        nb, cs = g['nb'], g['cs']
        t = np.arange(n_fft, dtype=np.float64)
        win = 0.5 - 0.5 * np.cos(2.0 * np.pi * t / n_fft)
        ang = 2.0 * np.pi * np.outer(np.arange(nb, dtype=np.float64), t) / n_fft
        wd = np.zeros((cs, n_fft), dtype=np.float64)
        wd[:nb] = np.cos(ang) * win
        wd[nb:2 * nb] = -np.sin(ang) * win
        assert np.array_equal(w, wd.reshape(cs, n_fft // hop, hop).transpose(1, 2, 0))
    assert not mel.stft_geometry(1024, 320, 1024)['old'] and not mel.stft_geometry(128, 32, 96)['old'] and not mel.stft_geometry(128, 16, 128)['old']


@pytest.mark.parametrize('geo', S.SMALL + S.LARGE, ids=S.gid)
def test_frame_counts_and_the_listed_lengths(geo):
    n_fft, hop, win = geo
    g = mel.stft_geometry(n_fft, hop, win)
    pad = g['pad']
    lens = S.lengths_of(n_fft, hop, pad)
    assert lens[0] == pad + 1 and {(n + 2 * pad - n_fft) % hop for n in lens if n + 2 * pad >= n_fft} >= {0, hop - 1}
    if n_fft - 2 * pad + hop - 1 > pad:                          # (odd n_fft - hop at 128 / 25 / 100: pad + 1 samples are two frames already)
        assert 1 in [mel.mel_frames(n, n_fft, hop) for n in lens]
    for n in lens + [pad, 1]:
        F = mel.mel_frames(n, n_fft, hop)
        assert F == S.frames(n, g)
        if n <= pad:
            assert F == 0
            continue
        yp = torch.nn.functional.pad(torch.zeros(1, 1, n), (pad, pad), mode='reflect').squeeze(1)
        if n + 2 * pad < n_fft:
            assert F == 0
            continue
        assert F == torch.stft(yp, n_fft, hop_length=hop, win_length=win, window=torch.hann_window(win), center=False,
                               return_complex=True).shape[-1] >= 1


def test_refusals():
    y = torch.zeros(2, 4100)
    for n_fft, hop, win in ((128, 129, 128), (128, 0, 128), (128, 32, 129), (128, 32, 0), (4096, 256, 1024), (2049, 256, 1024), (0, 0, 0)):
        with pytest.raises(ValueError, match='n_fft'):
            mel.stft_geometry(n_fft, hop, win)
        with pytest.raises(ValueError, match='n_fft'):
            mel.mel_spectrogram(y, n_fft, 8, 16000, hop, win, 0, None)
    with pytest.raises(ValueError, match='hop_size'):
        mel.stft_geometry(128, 200, 128)
    with pytest.raises(ValueError, match='win_size'):
        mel.stft_geometry(128, 32, 200)
    with pytest.raises(NotImplementedError):
        mel.mel_spectrogram(y, 128, 8, 16000, 25, 100, 0, None, center=True)
    with pytest.raises(ValueError):
        mel.mel_l1(torch.zeros(2, 8, 16), torch.zeros(2, 8, 16), [100, 50], n_fft=128, hop_size=129)
    # a geometry that is served gets as far as the device check
    with pytest.raises(RuntimeError, match='HIP path only'):
        mel.mel_spectrogram(y, 128, 8, 16000, 25, 100, 0, None)
    with pytest.raises(RuntimeError, match='HIP path only'):
        mel.mel_l1(torch.zeros(2, 8, 16), torch.zeros(2, 8, 16), [100, 50], n_fft=128, hop_size=25)


def test_oracle_alone_excludes_no_entry():
    """Seeded uniform noise of amplitude 0.5: no fp64 filterbank sum of the oracle lies within mel_ref.GAP of the clamp, at any listed geometry
    and length of tests/test_stft_geometry_gpu.py (an empty filter sums to 0, far below it)."""
    for geo in S.SMALL:
        g = mel.stft_geometry(*geo)
        for L in S.lengths_of(geo[0], geo[1], g['pad']):
            if S.frames(L, g):
                assert not S.near_clamp(S.signal(2, L, L), S.cfg_of(geo, S.SMALL_MELS)).any(), (geo, L)
    for geo in S.LARGE:
        assert not S.near_clamp(S.signal(S.LARGE_B, S.LARGE_L, geo[0]), S.cfg_of(geo, S.LARGE_MELS)).any(), geo


# ---------------------------------------------------------------------------------------------------------------
# the C ABI surface
def test_entry_points_are_declared_bound_and_additive():
    hdr = open(os.path.join(ROOT, 'include', 'vec2wav_hip.h')).read()
    lib = _hip.load()
    text = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    for name in GEO:
        assert name in _hip.SIGNATURES and name in _hip.LAUNCHERS and re.search(r'\b%s\s*\(' % name, hdr) and hasattr(lib, name) and name in text, name
    assert _hip.SIGNATURES['v2w_mel_finish_geo'] == _hip.SIGNATURES['v2w_mel_finish']
    assert _hip.SIGNATURES['v2w_mel_finish_geo_len'] == _hip.SIGNATURES['v2w_mel_finish_len']
    assert _hip.SIGNATURES['v2w_mel_finish_geo_bwd'] == _hip.SIGNATURES['v2w_mel_finish_bwd']
    assert _hip.SIGNATURES['v2w_l1_masked_geo'] == _hip.SIGNATURES['v2w_l1_masked']
    assert _hip.ABI_VERSION == lib.v2w_abi_version()             # new symbols only: the version stays


def _names(fn, *args):
    rc, names = _hip.kernel_names(fn, *args)
    return (0 if rc == 100 else rc), names                     # (100 = hipErrorNoDevice from a GPU-less process: nothing was launched)


def test_name_sink_reports_the_kernels_and_the_entry_points_refuse_bad_arguments():
    lib = _hip.load()
    A, Bp, Cp, Dp, Ep = (FAKE + (i << 28) for i in range(5))
    # B, L, n_fft, win, hop, CP, pad, left, k, FP
    geo = dict(B=3, L=400, n_fft=128, win=100, hop=25, CP=32, pad=51, left=14, k=4, FP=20)
    ok = tuple(geo.values())
    assert _names(lib.v2w_mel_phases_geo, A, Bp, *ok) == (0, ['mel_phase_kernel'])
    assert _names(lib.v2w_mel_phases_geo_len, A, Bp, *ok, Cp, 1) == (0, ['mel_phase_len_kernel'])
    assert _names(lib.v2w_mel_phases_geo_bwd, A, Bp, *ok) == (0, ['mel_phase_bwd_kernel'])
    bad = [dict(B=0), dict(L=1), dict(hop=0), dict(hop=129), dict(win=0), dict(win=129), dict(CP=24), dict(pad=-1), dict(pad=400), dict(left=-1),
           dict(left=29), dict(k=0), dict(k=3), dict(FP=0)]
    for d in bad:
        args = tuple(dict(geo, **d).values())
        for fn, tail in ((lib.v2w_mel_phases_geo, ()), (lib.v2w_mel_phases_geo_len, (Cp, 1)), (lib.v2w_mel_phases_geo_bwd, ())):
            assert _names(fn, A, Bp, *args, *tail) == (_hip.E_ARG, []), d
    assert _names(lib.v2w_mel_phases_geo, None, Bp, *ok) == (_hip.E_ARG, []) and _names(lib.v2w_mel_phases_geo_bwd, A, None, *ok) == (_hip.E_ARG, [])
    assert _names(lib.v2w_mel_phases_geo_len, A, Bp, *ok, None, 1) == (_hip.E_ARG, [])
    assert _names(lib.v2w_mel_phases_geo_len, A, Bp, *ok, Cp, 0) == (_hip.E_ARG, [])
    # the kernels' int arithmetic: CP * FP = 2^31, hop * FP + left = 2^31, L + 2 pad = 2^31; one below each is taken
    for d, rc in ((dict(hop=1 << 16, CP=1 << 16, n_fft=1 << 16, win=1 << 16, left=0, k=1, FP=1 << 15), _hip.E_SHAPE),
                  (dict(hop=32, CP=64, n_fft=128, FP=1 << 25), _hip.E_SHAPE), (dict(hop=32, CP=32, n_fft=128, left=0, win=128, FP=(1 << 26) - 1), 0),
                  (dict(hop=32, CP=32, n_fft=128, left=1, win=127, FP=1 << 26), _hip.E_SHAPE),
                  (dict(L=(1 << 30) + 2, pad=(1 << 29) - 1), _hip.E_SHAPE), (dict(L=(1 << 30) + 1, pad=(1 << 29) - 1), 0), (dict(B=65536), _hip.E_SHAPE)):
        assert _names(lib.v2w_mel_phases_geo, A, Bp, *dict(geo, **d).values())[0] == rc, d
        assert _names(lib.v2w_mel_phases_geo_bwd, A, Bp, *dict(geo, **d).values())[0] == rc, d
    # finish: the first kernels wherever they fit their LDS block, the 8-frame ones above, nothing past those
    fin = lambda nb, m: (A, Bp, Cp, 2, 2 * nb + 6, 20, 17, nb, m)  # noqa: E731
    for nb, m, fwd, bwd in ((513, 80, 'mel_finish_kernel', 'mel_finish_bwd_kernel'), (1024, 80, 'mel_finish_kernel', 'mel_finish8_bwd_kernel'),
                            (1025, 80, 'mel_finish8_kernel<false>', 'mel_finish8_bwd_kernel'), (2048, 1, 'mel_finish8_kernel<false>', None),
                            (2049, 1, None, None)):
        assert _names(lib.v2w_mel_finish_geo, *fin(nb, m)) == ((0, [fwd]) if fwd else (_hip.E_SHAPE, [])), nb
        flen = fwd and fwd.replace('mel_finish_kernel', 'mel_finish_len_kernel').replace('<false>', '<true>')
        assert _names(lib.v2w_mel_finish_geo_len, *fin(nb, m), Dp, 1, 25, 128) == ((0, [flen]) if fwd else (_hip.E_SHAPE, [])), nb
        s, b, o = fin(nb, m)[:3]
        assert _names(lib.v2w_mel_finish_geo_bwd, s, b, Dp, Ep, o, *fin(nb, m)[3:]) == ((0, [bwd]) if bwd else (_hip.E_SHAPE, [])), nb
    assert _names(lib.v2w_mel_finish_geo, None, *fin(1025, 80)[1:]) == (_hip.E_ARG, [])
    assert _names(lib.v2w_mel_finish_geo_len, *fin(1025, 80), None, 1, 25, 128) == (_hip.E_ARG, [])
    assert _names(lib.v2w_mel_finish_geo_len, *fin(1025, 80), Dp, 1, 129, 128) == (_hip.E_ARG, [])
    assert _names(lib.v2w_mel_finish_geo_len, *fin(1025, 80), Dp, 0, 25, 128) == (_hip.E_ARG, [])
    # the conditions that v2w_mel_finish_len and v2w_l1_masked keep are what their siblings drop
    assert _names(lib.v2w_mel_finish_len, *fin(513, 80), Dp, 1, 25, 128) == (_hip.E_ARG, [])
    tail = (Dp, 1, 25, 128, Ep, Ep + 4096, Ep + 8192)
    assert _names(lib.v2w_l1_masked, A, Bp, 5, 80, 16, *tail) == (_hip.E_ARG, [])
    assert _names(lib.v2w_l1_masked_geo, A, Bp, 5, 80, 16, *tail) == (0, ['l1_masked_kernel<true>', 'l1_masked_finish_kernel'])
    assert _names(lib.v2w_l1_masked_geo, A, Bp, 5, 80, 16, Dp, 1, 129, 128, *tail[4:]) == (_hip.E_ARG, [])
    assert _names(lib.v2w_l1_masked_geo, A, Bp, 5, 80, 16, None, *tail[1:]) == (_hip.E_ARG, [])


# ---------------------------------------------------------------------------------------------------------------
# tests/stft_ref.py where it meets tests/mel_ref.py: left = 0, cp = hop is the first entry points' statement
@pytest.mark.parametrize('L,hop,pad', [(100, 32, 48), (49, 32, 48), (37, 3, 5), (64, 32, 0)])
def test_the_numpy_statements_agree_where_the_geometries_meet(L, hop, pad):
    g = dict(n_fft=2 * pad + hop, hop=hop, cp=hop, pad=pad, left=0, k=(2 * pad + hop) // hop)
    rng = np.random.default_rng(L)
    y = rng.standard_normal((3, L)).astype(np.float32)
    FP = S.columns(L, g) + 4
    assert np.array_equal(S.phases(y, g, FP), R.phases(y, hop, pad, FP)[0])
    dxp = rng.standard_normal((3, hop, FP)).astype(np.float32)
    assert np.array_equal(S.phases_bwd(dxp, L, g), R.phases_bwd(dxp, L, hop, pad)[0])
    lens = (L, pad + 1, (L + pad) // 2, 1)
    y4 = rng.standard_normal((4, L)).astype(np.float32)
    assert np.array_equal(S.phases_len(y4, g, FP, lens), R.phases_len(y4, hop, pad, FP, lens, 1)[0])


def test_the_numpy_adjoint_is_the_transpose_of_the_gather():
    """<phases(y), d> == <y, phases_bwd(d)> in fp64-exact integers, at a geometry with left > 0, padding channels and an odd n_fft - hop."""
    g = mel.stft_geometry(128, 25, 100)
    rng = np.random.default_rng(5)
    for L in (52, 150, 203):
        FP = S.columns(L, g)
        y = rng.integers(-8, 9, (2, L)).astype(np.float32)
        d = rng.integers(-8, 9, (2, g['cp'], FP)).astype(np.float32)
        assert (S.phases(y, g, FP).astype(np.float64) * d).sum() == (y.astype(np.float64) * S.phases_bwd(d, L, g)).sum()
