"""CPU tests of the fused mel L1 training loss (`mel.mel_loss`): the fp64 reference of tests/mel_loss_ref.py against F.l1_loss, the
conditions on the inputs that the GPU tests' bounds rest on, the C ABI surface of the new entry points and their host argument checks,
and the refusals that need no GPU.  Nothing is launched."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from tests import mel_loss_ref as ML
from tests import stft_ref as S
from wavthruvec_pytorch_amd import _hip, mel, mel_loss

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('v2w_mel_loss_fwd', 'v2w_mel_loss_bwd', 'v2w_mel_phases_len_bwd', 'v2w_mel_phases_geo_len_bwd')
FAKE = 0x7f0000100000          # 16-byte aligned "device" pointers: the name sink never dereferences them
CFG = (1024, 80, 16000, 256, 1024, 0, None)
BY_NAME = {c['name']: c for c in ML.CASES}


def P(i):
    return FAKE + (i << 28)


# ---- the reference
def test_reference_without_lengths_is_l1_loss_of_the_trimmed_and_permuted_pair():
    from oracle import mel_oracle as M
    c = BY_NAME['128_32_96']
    B, L, cfg = 2, c['L'], c['cfg']
    y = S.signal(B, L, 3)
    F = mel.mel_frames(L, c['geo'][0], c['geo'][1])
    tgt = np.random.default_rng(4).standard_normal((B, F + 2, c['mels'])).astype(np.float32)
    got, per, dy = ML.loss_torch(y, tgt, cfg, [L] * B, [F] * B, 45.0)
    yt = torch.from_numpy(y).double().requires_grad_(True)
    want = 45.0 * torch.nn.functional.l1_loss(torch.from_numpy(tgt).double()[:, :F], M.mel_spectrogram(yt, *cfg, dtype=torch.float64).permute(0, 2, 1))
    want.backward()
    assert abs(got - want.item()) <= 1e-12 * abs(want.item())
    assert np.abs(dy - yt.grad.numpy()).max() <= 1e-12 * np.abs(dy).max()
    assert abs(np.mean(per) * 45.0 - got) <= 1e-12 * got          # equal frame counts: the mean of the per-item means


def test_reference_with_lengths_is_the_frame_weighted_mean_of_the_trimmed_losses():
    from oracle import mel_oracle as M
    c = BY_NAME['128_32_75']
    y, tgt, _m = ML.make_inputs(c)
    ns = ML.samples_of(c)
    F, Ft, Fb = ML.frames_of(c)
    assert Fb[0] == F and 0 < Fb[1] < Fb[2] < F and Ft == F + 2
    got, per, dy = ML.loss_torch(y, tgt, c['cfg'], ns, Fb, 1.0)
    each = [float(torch.nn.functional.l1_loss(torch.from_numpy(tgt[b, :f]).double(),
                                              M.mel_spectrogram(torch.from_numpy(y[b:b + 1, :n]), *c['cfg'], dtype=torch.float64)[0].t()))
            for b, (n, f) in enumerate(zip(ns, Fb))]
    assert np.allclose(per, each, rtol=1e-12, atol=0)
    assert abs(got - sum(e * f for e, f in zip(each, Fb)) / sum(Fb)) <= 1e-12 * got
    for b, n in enumerate(ns):
        assert not dy[b, n:].any() and dy[b, :n].any()
    # what lies past an item's end has no effect
    y2, t2 = y.copy(), tgt.copy()
    for b, (n, f) in enumerate(zip(ns, Fb)):
        y2[b, n:], t2[b, f:] = 1e30, np.nan
    assert ML.loss_torch(y2, t2, c['cfg'], ns, Fb, 1.0)[0] == got


@pytest.mark.parametrize('c', ML.CASES, ids=ML.IDS)
def test_conditions_on_the_inputs(c):
    """No entry of a trimmed item within mel_ref.GAP of the clamp; |m64 - t| >= 0.05 on every valid entry; zeros past F_b."""
    y, tgt, m64 = ML.make_inputs(c)
    F, Ft, Fb = ML.frames_of(c)
    assert tgt.shape == (len(c['lens']), F + 2, c['mels']) and max(Fb) == F
    for b, (n, f) in enumerate(zip(ML.samples_of(c), Fb)):
        if not f:                                    # (pad + 1 samples that are no frame)
            assert m64[b] is None and not tgt[b].any()
            continue
        assert m64[b].shape == (c['mels'], f), (b, n, f)
        assert not S.near_clamp(y[b:b + 1, :n], c['cfg']).any(), b
        assert (np.abs(m64[b] - tgt[b, :f].T.astype(np.float64)) >= ML.MARGIN).all(), b
        assert not tgt[b, f:].any()


def test_the_cases_are_the_listed_ones():
    assert [c['name'] for c in ML.CASES] == ['samples', 'frames'] + [S.gid(g) for g in S.SMALL] + ['1024_120_600', '2048_240_1200']
    assert (BY_NAME['samples']['L'], BY_NAME['samples']['lens']) == (4100, [4100, 385, 640, 1023, 2049, 4099])
    assert (BY_NAME['frames']['L'], BY_NAME['frames']['len_mul'], BY_NAME['frames']['lens']) == (3840, 320, [12, 2, 5, 11])
    for g in S.SMALL:
        c, geo = BY_NAME[S.gid(g)], mel.stft_geometry(*g)
        L = c['L']
        assert L == S.lengths_of(g[0], g[1], geo['pad'])[-1] and c['lens'] == [L, geo['pad'] + 1, (L + geo['pad'] + 1) // 2]
    for name in ('1024_120_600', '2048_240_1200'):
        assert BY_NAME[name]['L'] == 4096 and BY_NAME[name]['mels'] == 80
    assert mel.stft_geometry(2048, 240, 1200)['nb'] == 1025


# ---- the C ABI
def test_entry_points_are_declared_bound_and_additive():
    hdr = open(os.path.join(ROOT, 'include', 'vec2wav_hip.h')).read()
    lib = _hip.load()
    assert int(re.search(r'#define V2W_ABI_VERSION (\d+)', hdr).group(1)) == _hip.ABI_VERSION == 35 == lib.v2w_abi_version()
    text = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    for name in NAMES + ('v2w_mel_loss_plan',):
        assert name in _hip.SIGNATURES and re.search(r'\b%s\s*\(' % name, hdr) and hasattr(lib, name) and name in text, name
    assert set(NAMES) <= _hip.LAUNCHERS and 'v2w_mel_loss_plan' not in _hip.LAUNCHERS
    assert _hip.SIGNATURES['v2w_mel_phases_len_bwd'] == _hip.SIGNATURES['v2w_mel_phases_len']
    assert _hip.SIGNATURES['v2w_mel_phases_geo_len_bwd'] == _hip.SIGNATURES['v2w_mel_phases_geo_len']
    assert len(_hip.SIGNATURES['v2w_mel_loss_fwd'][1]) == 22 and len(_hip.SIGNATURES['v2w_mel_loss_bwd'][1]) == 21
    assert _hip.SIGNATURES['v2w_mel_loss_fwd'][1][16] is C.c_float


def test_plan_is_host_only_and_follows_the_finish_kernels_choice():
    lib = _hip.load()
    n = C.c_longlong(-1)
    assert lib.v2w_mel_loss_plan(6, 17, 513, 80, C.byref(n)) == 2 and n.value == 6 * 2 * 8          # 16 frames per workgroup
    assert lib.v2w_mel_loss_plan(6, 17, 1024, 80, C.byref(n)) == 2
    assert lib.v2w_mel_loss_plan(6, 17, 1025, 80, C.byref(n)) == 3 and n.value == 6 * 3 * 8         # 8 frames per workgroup
    assert lib.v2w_mel_loss_plan(6, 16, 1025, 80, None) == 2
    assert lib.v2w_mel_loss_plan(6, 17, 2049, 80, None) == _hip.E_SHAPE and lib.v2w_mel_loss_plan(65536, 17, 513, 80, None) == _hip.E_SHAPE
    for bad in ((0, 17, 513, 80), (6, 0, 513, 80), (6, 17, 0, 80), (6, 17, 513, 0)):
        assert lib.v2w_mel_loss_plan(*bad, None) == _hip.E_ARG, bad


def _fwd_args(**kw):
    a = dict(spec=P(0), basis=P(1), tgt=P(2), ts_f=80, ts_m=1, B=6, Cs=1088, FP=20, F=17, Ft=19, nb=513, n_mels=80, len=P(3), len_mul=1,
             hop=256, n_fft=1024, scale=1.0, per_item=P(4), total=P(5), coef=P(6), ws=P(7))
    a.update(kw)
    return tuple(a.values())


def _bwd_args(**kw):
    a = dict(spec=P(0), basis=P(1), basisT=P(2), tgt=P(3), ts_f=80, ts_m=1, gout=P(4), coef=P(5), dspec=P(6), B=6, Cs=1088, FP=20, F=17, Ft=19,
             nb=513, n_mels=80, len=P(7), len_mul=1, hop=256, n_fft=1024)
    a.update(kw)
    return tuple(a.values())


def test_name_sink_reports_the_kernels_of_every_branch():
    lib = _hip.load()
    for kw, kern in ((dict(), 'mel_loss_fwd_kernel<16, true>'), (dict(len=None), 'mel_loss_fwd_kernel<16, false>'),
                     (dict(nb=1025, Cs=2112), 'mel_loss_fwd_kernel<8, true>'), (dict(nb=1025, Cs=2112, len=None), 'mel_loss_fwd_kernel<8, false>'),
                     (dict(ts_f=1, ts_m=19), 'mel_loss_fwd_kernel<16, true>')):
        rc, names = _hip.kernel_names(lib.v2w_mel_loss_fwd, *_fwd_args(**kw))
        assert rc in (0, 100) and names == [kern, 'mel_loss_finish_kernel'], (kw, names)
    for kw, kern in ((dict(), 'mel_loss_bwd_kernel<16, true>'), (dict(len=None), 'mel_loss_bwd_kernel<16, false>'),
                     (dict(nb=1025, Cs=2112), 'mel_loss_bwd_kernel<8, true>'), (dict(nb=1025, Cs=2112, len=None), 'mel_loss_bwd_kernel<8, false>'),
                     (dict(nb=1000, Cs=2048), 'mel_loss_bwd_kernel<8, true>')):           # 1000 bins + 80 mels: 16 frames pass 64 KiB
        rc, names = _hip.kernel_names(lib.v2w_mel_loss_bwd, *_bwd_args(**kw))
        assert rc in (0, 100) and names == [kern], (kw, names)
    ph = (P(0), P(1), 6, 4100, 256, 384, 20)
    rc, names = _hip.kernel_names(lib.v2w_mel_phases_len_bwd, *ph, P(2), 1)
    assert rc in (0, 100) and names == ['mel_phase_len_bwd_kernel'], names
    geo = (P(0), P(1), 3, 4096, 1024, 600, 120, 128, 452, 212, 5, 36)
    rc, names = _hip.kernel_names(lib.v2w_mel_phases_geo_len_bwd, *geo, P(2), 1)
    assert rc in (0, 100) and names == ['mel_phase_len_bwd_kernel'], names


def test_host_argument_checks_return_their_code_and_launch_nothing():
    lib = _hip.load()
    E_ARG, E_SHAPE = (_hip.E_ARG, []), (_hip.E_SHAPE, [])
    fwd = lambda **kw: _hip.kernel_names(lib.v2w_mel_loss_fwd, *_fwd_args(**kw))  # noqa: E731
    for kw in (dict(spec=None), dict(basis=None), dict(tgt=None), dict(ws=None), dict(ws=P(7) + 4), dict(per_item=None, total=None, coef=None),
               dict(B=0), dict(F=0), dict(FP=16), dict(nb=0), dict(Cs=1025), dict(n_mels=0), dict(Ft=0), dict(scale=float('nan')),
               dict(ts_f=79), dict(ts_f=1, ts_m=17), dict(ts_f=0, ts_m=0), dict(ts_f=-80, ts_m=1),
               dict(len_mul=0), dict(hop=0), dict(n_fft=255), dict(len=None, Ft=16)):
        assert fwd(**kw) == E_ARG, kw
    for kw in (dict(B=65536), dict(nb=2049, Cs=4098), dict(n_mels=1 << 28, ts_f=1 << 28), dict(hop=1 << 27, n_fft=1 << 27), dict(Ft=1 << 25)):
        assert fwd(**kw) == E_SHAPE, kw
    assert fwd(len=None, Ft=17)[0] in (0, 100) and fwd(Ft=1)[0] in (0, 100) and fwd(per_item=None, total=None)[0] in (0, 100)
    bwd = lambda **kw: _hip.kernel_names(lib.v2w_mel_loss_bwd, *_bwd_args(**kw))  # noqa: E731
    for kw in (dict(spec=None), dict(basis=None), dict(basisT=None), dict(tgt=None), dict(gout=None), dict(coef=None), dict(dspec=None),
               dict(B=0), dict(F=0), dict(FP=16), dict(nb=0), dict(Cs=1025), dict(n_mels=0), dict(Ft=0), dict(ts_f=79), dict(ts_f=1, ts_m=17),
               dict(len_mul=0), dict(hop=0), dict(n_fft=255), dict(len=None, Ft=16)):
        assert bwd(**kw) == E_ARG, kw
    for kw in (dict(B=65536), dict(nb=2000, Cs=4000), dict(hop=1 << 27, n_fft=1 << 27)):
        assert bwd(**kw) == E_SHAPE, kw
    ph = lambda *a: _hip.kernel_names(lib.v2w_mel_phases_len_bwd, *a)  # noqa: E731
    good = (P(0), P(1), 6, 4100, 256, 384, 20, P(2), 1)
    assert ph(*good)[0] in (0, 100)
    for i, v in ((0, None), (1, None), (2, 0), (3, 1), (4, 0), (5, -1), (5, 4100), (6, 0), (7, None), (8, 0), (5, 100)):      # (100: 2 pad % hop != 0)
        assert ph(*good[:i], v, *good[i + 1:]) == E_ARG, (i, v)
    assert ph(*good[:2], 65536, *good[3:]) == E_SHAPE and ph(*good[:6], 1 << 24, *good[7:]) == E_SHAPE
    gl = lambda *a: _hip.kernel_names(lib.v2w_mel_phases_geo_len_bwd, *a)  # noqa: E731
    good = (P(0), P(1), 3, 4096, 1024, 600, 120, 128, 452, 212, 5, 36, P(2), 1)
    assert gl(*good)[0] in (0, 100)
    for i, v in ((0, None), (1, None), (2, 0), (3, 1), (4, 100), (5, 0), (5, 1025), (6, 0), (7, 100), (8, -1), (8, 4096), (9, -1), (9, 425), (10, 0),
                 (10, 4), (11, 0), (12, None), (13, 0)):
        assert gl(*good[:i], v, *good[i + 1:]) == E_ARG, (i, v)
    assert gl(*good[:2], 65536, *good[3:]) == E_SHAPE and gl(*good[:11], 1 << 25, *good[12:]) == E_SHAPE


# ---- the public function, as far as a machine without a GPU goes
def test_mel_loss_is_exported_and_refuses_what_it_does_not_serve():
    import wavthruvec_pytorch_amd as W
    assert W.mel_loss is mel.mel_loss and 'mel_loss' in W.__all__
    y, t = torch.zeros(2, 4100), torch.zeros(2, 18, 80)
    with pytest.raises(RuntimeError, match='HIP path only'):
        mel_loss(y, t, *CFG)
    with pytest.raises(RuntimeError, match='HIP path only'):
        mel_loss(y[:, None], t, *CFG, lengths=[4100, 400])
    with pytest.raises(NotImplementedError):
        mel_loss(y, t.clone().requires_grad_(), *CFG)
    with torch.no_grad(), pytest.raises(RuntimeError, match='HIP path only'):       # no-grad: such a target is taken (and then needs a GPU)
        mel_loss(y, t.clone().requires_grad_(), *CFG)
    with pytest.raises(ValueError, match='15 frames'):
        mel_loss(y, t[:, :15], *CFG)                                                # F_t < F = 16 without lengths
    with pytest.raises(RuntimeError, match='HIP path only'):
        mel_loss(y, t[:, :15], *CFG, lengths=[4100, 400])                           # with lengths F_b is clamped to F_t
    for bad in (dict(lengths=[4100, 0]), dict(lengths=[4101, 5]), dict(lengths=[5]), dict(lengths=[13, 2], len_mul=320), dict(lengths=[1, 1], len_mul=0)):
        with pytest.raises(ValueError):
            mel_loss(y, t, *CFG, **bad)
    for geo in ((1024, 0, 1024), (1024, 256, 1025), (4096, 256, 1024)):             # mel_spectrogram's geometry errors
        with pytest.raises(ValueError):
            mel_loss(y, t, geo[0], 80, 16000, geo[1], geo[2], 0, None)
    with pytest.raises(ValueError):
        mel_loss(y, t.permute(0, 2, 1), *CFG)                                       # mels first needs frames_first=False
    with pytest.raises(RuntimeError, match='HIP path only'):
        mel_loss(y, t.permute(0, 2, 1), *CFG, frames_first=False)
    with pytest.raises(ValueError):
        mel_loss(torch.zeros(2, 2, 4100), t, *CFG)
    with pytest.raises(TypeError):
        mel_loss(y, t, *CFG, [4100, 400])                                           # lengths is keyword-only; center is not offered
    with pytest.raises(TypeError):
        mel_loss(y, t, *CFG, center=True)


def test_mel_spectrogram_with_lengths_still_refuses_under_grad_mode():
    with pytest.raises(NotImplementedError):
        mel.mel_spectrogram(torch.zeros(2, 4100).requires_grad_(), *CFG, lengths=[4100, 400])
