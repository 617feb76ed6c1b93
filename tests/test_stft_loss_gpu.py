"""The multi-resolution STFT loss on the device: the three kernels of csrc/v2w_stft_loss.hip behind v2w_stft_loss_multi and
v2w_stft_loss_multi_bwd against the fp64 statements of tests/stft_loss_ref.py (a), then stft_loss.py end to end against the torch.stft
oracle (b).  tests/test_stft_loss_cpu.py holds the host-only half.

  1. kernel level, on guarded buffers: random float32 specs with NaN in the rows >= 2 nb and +-3e38 in the columns >= F.  The sums, sc, mag and
     the totals within the header's roundings (error / bound <= 1); d spec per entry, the entries with |X / Y - 1| < mel_ref.GAP left out (at
     most 0.5 % of a case); the pad rows and columns of d spec exactly +0.0; the backward is handed the device's own sums, so the chain is
     cut there; every call twice from restored buffers, the same bits; a resolution inside a three-descriptor call has the bits of its own
     call; x == y gives sc == 0, mag == 0 and d spec == 0 without a NaN.
  2. end to end: stft_ref.SMALL at stft_ref.lengths_of lengths with B = 1 and 2, the three LARGE resolutions at B = 2, L = 8192 singly and as
     the module.  d x: max |error| <= 4 x the oracle's own float32-against-float64 max gap on that input.  sc / mag: relative error <= 4 x the
     LARGEST relative float32-against-float64 gap of the oracle over the whole case list (computed here, per quantity).  The module case
     back-propagates sc + 2 mag, the others sc + mag.
Every test here fails without the feature (no wavthruvec_pytorch_amd.stft_loss, no v2w_stft_loss_* symbol).  DESIGN.md 3d'''' records the
measured ratios.

Measured on an MI355X.  Kernel level (error / bound): the sums 0.0002 - 0.036, sc 0.013 - 0.049, mag 0.0008 - 0.034, d spec 0.13 - 0.34.  End
to end: scalar bars 1.60e-6 (sc) and 1.58e-6 (mag), errors at most 0.055 and 0.091 of them; d x error / the oracle's float32 gap (bar 4):
the 128-point geometries 0.33 - 1.85, 512 / 50 / 240 0.71, 1024 / 120 / 600 2.33 (1.056e-7 against a gap of 4.533e-8), 2048 / 240 / 1200 1.52,
the module 1.42.  With the forward DFT conv in one launch (one chain of k * cp fp32 terms per spec entry) the last three were 5.77, 2.41 and
3.56, and 1024 / 120 / 600 missed the bar: the whole of that error was the forward conv's (the device's spec with everything after it in
fp64: 5.76), which the log term's gradient carries as d / X^2 at the entries of small X.  stft_loss.py adds the input channels 64 at a time
since (stft_loss._dft_conv_fwd)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import mel_ref as R
from tests import stft_loss_ref as SL
from tests import stft_ref as S
from tests.test_cbn_kernels_gpu import _addr, _inp, _kept, _out, _twice
from tests.test_disc_kernels_gpu import _report, env  # noqa: F401  (env: the module-scoped fixture)
from tests.test_mel_kernels_gpu import _bits_equal
from tests.test_tile_kernels_gpu import _sync_or_stop

pytestmark = pytest.mark.gpu
OK = 0
G_OUT, GT_SC, GT_MAG = (0.75, -1.25), (0.5, -0.25, 1.5), (0.125, 2.0, -0.5)      # (g_sc, g_mag) and the per-resolution terms


# ---------------------------------------------------------------------------------------------------------------
# 1. kernel level
def _call(env, specs, gterm):
    """Forward, then backward on the device's own sums, twice from restored buffers -> the buffers."""
    dev, _hip, lib, st = env
    n = len(specs)
    arr = (_hip.StftLossItem * n)()
    A = dict(sx=[_inp(dev, sx) for _s, sx, _y in specs], sy=[_inp(dev, sy) for _s, _x, sy in specs],
             dx=[_out(dev, *sx.shape) for _s, sx, _y in specs], sc=_out(dev, n), mag=_out(dev, n), total=_out(dev, 2),
             sums=_out(dev, 3 * n, dtype=torch.float64), g=_inp(dev, np.asarray(G_OUT, dtype=np.float32)),
             gt_sc=_inp(dev, np.asarray(GT_SC[:n], dtype=np.float32)), gt_mag=_inp(dev, np.asarray(GT_MAG[:n], dtype=np.float32)))
    t = _addr(A)
    for i, (d, ((nb, F, FP, Cs, B), _x, _y)) in enumerate(zip(arr, specs)):
        d.spec_x, d.spec_y, d.dspec_x = t['sx'][i], t['sy'][i], t['dx'][i]
        d.B, d.Cs, d.FP, d.F, d.nb = B, Cs, FP, F, nb
    nbytes = lib.v2w_stft_loss_scratch_bytes(arr, n)
    assert nbytes > 0 and nbytes % 24 == 0
    A['scratch'] = _out(dev, nbytes // 8, dtype=torch.float64)
    t = _addr(A)
    gt = (t['gt_sc'], t['gt_mag']) if gterm else (None, None)
    assert _twice(A, 'stft_loss', lambda: (
        lib.v2w_stft_loss_multi(arr, n, t['sc'], t['mag'], t['total'], t['sums'], t['scratch'], st),
        lib.v2w_stft_loss_multi_bwd(arr, n, t['sums'], t['g'], t['g'] + 4, *gt, st))) == (OK, OK)
    _kept(A, {'dx', 'sc', 'mag', 'total', 'sums', 'scratch'}, 'stft_loss')
    return A


def _check_case(env, name, gterm):
    specs = SL.case_specs(name)
    n = len(specs)
    A = _call(env, specs, gterm)
    sums, sc, mag, total = A['sums'].get(), A['sc'].get(), A['mag'].get(), A['total'].get()
    vals, bounds, ratios = [], [], {}
    for i, ((nb, F, FP, Cs, B), sx, sy) in enumerate(specs):
        v, b = SL.sums(sx, sy, F, nb)
        vals.append(v)
        bounds.append(b)
        for j, k in enumerate(('Sd', 'Sy', 'Sl')):
            ratios['%s[%d]' % (k, i)] = R.worst_ratio(sums[3 * i + j], v[k], b[k])
        ratios['sc[%d]' % i] = R.worst_ratio(sc[i], v['sc'], b['sc'])
        ratios['mag[%d]' % i] = R.worst_ratio(mag[i], v['mag'], b['mag'])
        g_sc = SL.g_of(G_OUT[0], GT_SC[i] if gterm else None, n)
        g_mag = SL.g_of(G_OUT[1], GT_MAG[i] if gterm else None, n)
        dre, dim, bre, bim, unsure = SL.dspec(sx, sy, F, nb, float(sums[3 * i]), float(sums[3 * i + 1]), g_sc, g_mag)
        assert unsure.mean() <= SL.MAX_UNSURE, (name, i, unsure.mean())
        got = A['dx'][i].get()
        assert np.isfinite(got).all()
        keep = ~unsure
        ratios['dRe[%d]' % i] = R.worst_ratio(got[:, :nb, :F][keep], dre[keep], bre[keep])
        ratios['dIm[%d]' % i] = R.worst_ratio(got[:, nb:2 * nb, :F][keep], dim[keep], bim[keep])
        assert _bits_equal(got[:, 2 * nb:, :], np.zeros((B, Cs - 2 * nb, FP))), (name, i, 'pad rows of dspec are not +0.0')
        assert _bits_equal(got[:, :, F:], np.zeros((B, Cs, FP - F))), (name, i, 'columns >= F of dspec are not +0.0')
    tot = SL.totals(vals, bounds)
    ratios['total_sc'] = R.worst_ratio(total[0], *tot['sc'])
    ratios['total_mag'] = R.worst_ratio(total[1], *tot['mag'])
    _report('stft_loss %s' % name, **ratios)
    return A


@pytest.mark.parametrize('name', [k for k in SL.KERNEL_CASES if k != 'mixed'])
def test_one_resolution(env, name):
    _check_case(env, name, gterm=name in ('tail3', 'odd'))


def test_three_resolutions_in_one_call(env):
    """The mixed call within its bounds, and each of its resolutions the bits of the call that holds it alone."""
    A = _check_case(env, 'mixed', gterm=True)
    sums, sc, mag = A['sums'].get(), A['sc'].get(), A['mag'].get()
    for i, s in enumerate(SL.KERNEL_CASES['mixed']):
        own = _call(env, SL.case_specs(s), gterm=False)
        assert np.array_equal(own['sums'].get().view(np.int64), sums[3 * i:3 * i + 3].view(np.int64)), s
        assert _bits_equal(own['sc'].get(), sc[i:i + 1]) and _bits_equal(own['mag'].get(), mag[i:i + 1]), s


def test_equal_signals(env):
    specs = SL.case_specs('tail3', same=True) + SL.case_specs('nb1025', same=True)
    A = _call(env, specs, gterm=True)
    assert not A['sc'].get().any() and not A['mag'].get().any() and not A['total'].get().any()
    sums = A['sums'].get()
    assert sums[0] == 0 and sums[2] == 0 and sums[3] == 0 and sums[5] == 0 and sums[1] > 0 and sums[4] > 0
    for a in A['dx']:
        got = a.get()
        assert np.isfinite(got).all() and not got.any()


# ---------------------------------------------------------------------------------------------------------------
# 2. end to end against the oracle
def _small_cases():
    from wavthruvec_pytorch_amd import mel
    out = []
    for geo in S.SMALL:
        g = mel.stft_geometry(*geo)
        for L in S.lengths_of(geo[0], geo[1], g['pad']):
            if S.frames(L, g) and L > 1:
                out += [((geo,), B, L, 1.0) for B in (1, 2)]
    return out


def _large_cases():
    return [((geo,), S.LARGE_B, S.LARGE_L, 1.0) for geo in S.LARGE] + [(tuple(S.LARGE), S.LARGE_B, S.LARGE_L, 2.0)]


@functools.lru_cache(maxsize=None)
def _oracle(case):
    """The oracle's fp64 results and its own float32 gaps on one case (CPU, once)."""
    res, B, L, w_mag = case
    x, y = SL.signals(B, L)
    return SL.oracle_gaps(x, y, res, 1.0, w_mag)


@functools.lru_cache(maxsize=None)
def _scalar_bars():
    """4 x the largest relative float32-against-float64 gap of the oracle over the whole case list, per quantity."""
    o = [_oracle(c) for c in _small_cases() + _large_cases()]
    return 4 * max(g['rel_sc'] for g in o), 4 * max(g['rel_mag'] for g in o)


def _end_to_end(dev, case):
    """-> the figures of one case: (relative errors of sc and mag, their bars, max |d x - oracle|, its bar)."""
    from wavthruvec_pytorch_amd import MultiResolutionSTFTLoss, stft_loss
    res, B, L, w_mag = case
    o = _oracle(case)
    x, y = SL.signals(B, L)
    xd = torch.from_numpy(x).to(dev).requires_grad_(True)
    yd = torch.from_numpy(y).to(dev)
    if len(res) == 1:
        sc, mag = stft_loss.stft_loss(xd.unsqueeze(1) if B == 1 else xd, yd, *res[0])          # ((B, 1, L) is taken too)
    else:
        sc, mag = MultiResolutionSTFTLoss(res)(xd, yd)
    assert sc.dim() == 0 and mag.dim() == 0 and sc.is_cuda and mag.is_cuda
    (sc + w_mag * mag).backward()
    _sync_or_stop('stft_loss %s B=%d L=%d' % ('+'.join(S.gid(g) for g in res), B, L))
    dx = xd.grad.cpu().numpy()
    assert np.isfinite(dx).all() and dx.shape == (B, L)
    e_sc, e_mag = abs(sc.item() - o['sc']) / abs(o['sc']), abs(mag.item() - o['mag']) / abs(o['mag'])
    e_dx = float(np.abs(dx - o['dx']).max())
    bar_sc, bar_mag = _scalar_bars()
    print('[stft loss] %s B=%d L=%d: sc %.6f mag %.6f; oracle f32 - f64 rel gaps sc %.3e mag %.3e dx %.3e (max |dx| %.3e); HIP - f64 rel sc %.3e '
          'mag %.3e dx %.3e; ratios to the bars sc %.3f mag %.3f (bars %.3e %.3e), dx / gap %.3f (bar 4)'
          % ('+'.join(S.gid(g) for g in res), B, L, o['sc'], o['mag'], o['rel_sc'], o['rel_mag'], o['gap_dx'], np.abs(o['dx']).max(), e_sc, e_mag,
             e_dx, e_sc / bar_sc, e_mag / bar_mag, bar_sc, bar_mag, e_dx / o['gap_dx']))
    return e_sc, bar_sc, e_mag, bar_mag, e_dx, 4 * o['gap_dx']


def _assert_figures(case, fig):
    e_sc, bar_sc, e_mag, bar_mag, e_dx, bar_dx = fig
    assert e_sc <= bar_sc and e_mag <= bar_mag and e_dx <= bar_dx, (case, fig)


@pytest.mark.parametrize('geo', S.SMALL, ids=S.gid)
def test_end_to_end_at_the_listed_lengths(env, geo):
    cases = [c for c in _small_cases() if c[0] == (geo,)]
    assert cases
    figures = [_end_to_end(env[0], c) for c in cases]
    for c, f in zip(cases, figures):
        _assert_figures(c, f)


@pytest.mark.parametrize('case', _large_cases(), ids=lambda c: '+'.join(S.gid(g) for g in c[0]))
def test_end_to_end_at_the_multi_resolution_settings(env, case):
    _assert_figures(case, _end_to_end(env[0], case))


def test_no_grad_and_the_length_conditions(env):
    from wavthruvec_pytorch_amd import MultiResolutionSTFTLoss, stft_loss
    dev = env[0]
    x, y = (torch.from_numpy(a).to(dev) for a in SL.signals(2, 600))
    m = MultiResolutionSTFTLoss([(128, 32, 96), (128, 25, 100)])
    a = m(x.clone().requires_grad_(True), y)
    b = m(x, y)
    with torch.no_grad():
        c = m(x.clone().requires_grad_(True), y)
    _sync_or_stop('stft_loss no_grad')
    assert a[0].requires_grad and not b[0].requires_grad and not c[0].requires_grad
    for u, v in zip(a + a, b + c):
        assert _bits_equal(u.detach().cpu().numpy(), v.cpu().numpy())
    with pytest.raises(RuntimeError, match='reflect padding'):
        stft_loss.stft_loss(x[:, :48], y[:, :48], 128, 32, 128)
    with pytest.raises(RuntimeError, match='shorter than one frame'):
        stft_loss.stft_loss(x[:, :20], y[:, :20], 128, 128, 128)
