"""The STFT loss with per-item lengths on the device: v2w_stft_loss_multi_len / _len_bwd against the fp64 statements of
tests/stft_loss_len_ref.py (a), then stft_loss.py's `lengths=` end to end against that module's ragged torch.stft oracle (b).
tests/test_stft_loss_len_cpu.py holds the host-only half.

  1. kernel level, on guarded buffers: stft_loss_ref.random_specs operands with NaN and +-3e38 in EVERY column at or past F_b of item b (and
     NaN in the rows >= 2 nb); frame counts 0, 1, F_b % 4 in {1, 2, 3}, F and counts clamped from above F; a three-resolution call.  The four
     sums, sc, mag, the totals and every d spec entry within the reference's bounds (error / bound <= 1; N exactly), the entries with
     |X / Y - 1| < mel_ref.GAP left out (at most 0.5 % of a resolution's valid entries, asserted on the fp64 reference when the cases are
     built); the columns [F_b, FP) and the pad rows of d spec bitwise +0.0; every call twice from restored buffers, the same bits.
  2. every F_b == F: the bits of v2w_stft_loss_multi / _multi_bwd, and MultiResolutionSTFTLoss(lengths=[L // m] * B, len_mul=m) the bits of
     the call without lengths, values and gradient.
  3. NaN written over y_hat[b, n_b:] and y[b, n_b:] changes no bit of sc, mag or the gradient; the gradient past n_b is bitwise +0.0.
  4. every item too short: sc == mag == 0, the gradient all zero and finite (kernel level: case 'none').
  5. end to end at stft_ref.SMALL, B = 3 (lengths from stft_ref.lengths_of, one item at L, one without a frame) and the three LARGE
     resolutions as one module at B = 2, L = 8192, lengths (8192, 5000), sc + 2 mag.  sc / mag: relative error <= 4 x the LARGEST relative
     float32-against-float64 gap of the ragged oracle over this file's case list; d x: max |error| <= 4 x the oracle's own float32-against-
     float64 max gap on that case.
  6. no_grad, and y_hat without requires_grad: the same bits, no graph.
Every test here fails without the feature (no `lengths` keyword, no v2w_stft_loss_multi_len symbol).

Measured on an MI355X.  Kernel level (error / bound): the sums 0.0001 - 0.025, sc 0.004 - 0.049, mag 0.005 - 0.035, d spec 0.15 - 0.36.  End to
end: scalar bars 6.31e-7 (sc) and 8.08e-7 (mag), errors at most 0.08 and 0.18 of them; d x error / the oracle's float32 gap (bar 4): 0.21 -
1.81 at the 128-point geometries but for 128 / 128 / 128 at lengths (1, 511, 384), 3.50 (2.22e-7 against a gap of 6.36e-8); the module 1.45.
DESIGN.md 3d'''' has the list."""
import functools

import numpy as np
import pytest
import torch

from tests import mel_ref as R
from tests import stft_loss_len_ref as LR
from tests import stft_loss_ref as SL
from tests import stft_ref as S
from tests.test_cbn_kernels_gpu import _addr, _inp, _kept, _out, _twice
from tests.test_disc_kernels_gpu import _report, env  # noqa: F401  (env: the module-scoped fixture)
from tests.test_mel_kernels_gpu import _bits_equal
from tests.test_stft_loss_gpu import G_OUT, GT_MAG, GT_SC
from tests.test_stft_loss_gpu import _call as _dense_call
from tests.test_tile_kernels_gpu import _sync_or_stop

pytestmark = pytest.mark.gpu
OK = 0


def _positive_zero(a):
    a = np.ascontiguousarray(a, dtype=np.float32)
    return not a.view(np.int32).any()


# ---------------------------------------------------------------------------------------------------------------
# 1. kernel level
def _call(env, name, gterm):
    """Forward, then backward on the device's own four sums, twice from restored buffers -> (the buffers, the case's specs)."""
    import ctypes as C
    dev, _hip, lib, st = env
    c = LR.CASES[name]
    specs = LR.case_specs(name)
    n = len(specs)
    arr = (_hip.StftLossItem * n)()
    A = dict(sx=[_inp(dev, s[3]) for s in specs], sy=[_inp(dev, s[4]) for s in specs], dx=[_out(dev, *s[3].shape) for s in specs],
             sc=_out(dev, n), mag=_out(dev, n), total=_out(dev, 2), sums=_out(dev, 4 * n, dtype=torch.float64),
             g=_inp(dev, np.asarray(G_OUT, dtype=np.float32)), gt_sc=_inp(dev, np.asarray(GT_SC[:n], dtype=np.float32)),
             gt_mag=_inp(dev, np.asarray(GT_MAG[:n], dtype=np.float32)))
    ld = torch.tensor(c['lens'], dtype=torch.int32, device=dev)               # (B int32: the kernels read len[b] for b < B alone)
    t = _addr(A)
    for i, (d, ((nb, F, FP, Cs, B), *_r)) in enumerate(zip(arr, specs)):
        d.spec_x, d.spec_y, d.dspec_x = t['sx'][i], t['sy'][i], t['dx'][i]
        d.B, d.Cs, d.FP, d.F, d.nb = B, Cs, FP, F, nb
    nbytes = lib.v2w_stft_loss_scratch_bytes(arr, n)
    assert nbytes > 0 and nbytes % 24 == 0
    A['scratch'] = _out(dev, nbytes // 8, dtype=torch.float64)
    t = _addr(A)
    hop, n_fft = (C.c_int32 * n)(*[g[0] for g in c['geo']]), (C.c_int32 * n)(*[g[1] for g in c['geo']])
    gt = (t['gt_sc'], t['gt_mag']) if gterm else (None, None)
    assert _twice(A, 'stft_loss_len ' + name, lambda: (
        lib.v2w_stft_loss_multi_len(arr, n, hop, n_fft, ld.data_ptr(), c['len_mul'], t['sc'], t['mag'], t['total'], t['sums'], t['scratch'], st),
        lib.v2w_stft_loss_multi_len_bwd(arr, n, hop, n_fft, ld.data_ptr(), c['len_mul'], t['sums'], t['g'], t['g'] + 4, *gt, st))) == (OK, OK)
    _kept(A, {'dx', 'sc', 'mag', 'total', 'sums', 'scratch'}, 'stft_loss_len ' + name)
    assert ld.cpu().tolist() == list(c['lens'])
    return A, specs


def _check_case(env, name, gterm):
    A, specs = _call(env, name, gterm)
    n = len(specs)
    sums, sc, mag, total = A['sums'].get(), A['sc'].get(), A['mag'].get(), A['total'].get()
    assert np.isfinite(sums).all() and np.isfinite(sc).all() and np.isfinite(mag).all() and np.isfinite(total).all()
    vals, bounds, ratios = [], [], {}
    for i, ((nb, F, FP, Cs, B), _geo, Fb, sx, sy) in enumerate(specs):
        v, b = LR.sums(sx, sy, F, nb, Fb)
        vals.append(v)
        bounds.append(b)
        for j, k in enumerate(('Sd', 'Sy', 'Sl')):
            ratios['%s[%d]' % (k, i)] = R.worst_ratio(sums[4 * i + j], v[k], b[k])
        assert sums[4 * i + 3] == v['N'] == nb * sum(Fb), (name, i, sums[4 * i + 3])
        ratios['sc[%d]' % i] = R.worst_ratio(sc[i], v['sc'], b['sc'])
        ratios['mag[%d]' % i] = R.worst_ratio(mag[i], v['mag'], b['mag'])
        g_sc = SL.g_of(G_OUT[0], GT_SC[i] if gterm else None, n)
        g_mag = SL.g_of(G_OUT[1], GT_MAG[i] if gterm else None, n)
        dre, dim, bre, bim, unsure = LR.dspec(sx, sy, F, nb, Fb, float(sums[4 * i]), float(sums[4 * i + 1]), float(sums[4 * i + 3]), g_sc, g_mag)
        assert unsure.sum() <= SL.MAX_UNSURE * max(v['N'], 1), (name, i, int(unsure.sum()))
        got = A['dx'][i].get()
        assert np.isfinite(got).all()
        keep = ~unsure
        ratios['dRe[%d]' % i] = R.worst_ratio(got[:, :nb, :F][keep], dre[keep], bre[keep])
        ratios['dIm[%d]' % i] = R.worst_ratio(got[:, nb:2 * nb, :F][keep], dim[keep], bim[keep])
        assert _positive_zero(got[:, 2 * nb:, :]), (name, i, 'pad rows of dspec are not +0.0')
        for b_, f in enumerate(Fb):
            assert _positive_zero(got[b_, :, f:]), (name, i, b_, 'columns >= F_b of dspec are not +0.0')
        if not v['N']:
            assert _positive_zero(sc[i:i + 1]) and _positive_zero(mag[i:i + 1]) and not sums[4 * i:4 * i + 4].any()
    tot = SL.totals(vals, bounds)
    ratios['total_sc'] = R.worst_ratio(total[0], *tot['sc'])
    ratios['total_mag'] = R.worst_ratio(total[1], *tot['mag'])
    _report('stft_loss_len %s' % name, **ratios)
    return A


@pytest.mark.parametrize('name', ['one_frame', 'tail2', 'tail3', 'nb1025', 'odd'])
def test_one_resolution_with_lengths(env, name):
    _check_case(env, name, gterm=name in ('tail3', 'odd'))


def test_three_resolutions_with_lengths_in_one_call(env):
    _check_case(env, 'mixed', gterm=True)


def test_no_valid_entry_at_the_kernel_level(env):
    """Every F_b == 0 in both resolutions: sc == mag == total == 0 (+0.0), the four sums 0, d spec all +0.0 - and nothing was loaded: the
    whole spec is junk past F_b = 0."""
    A = _check_case(env, 'none', gterm=True)
    assert _positive_zero(A['total'].get()) and _positive_zero(A['sc'].get()) and _positive_zero(A['mag'].get())
    for a in A['dx']:
        assert _positive_zero(a.get())


# ---------------------------------------------------------------------------------------------------------------
# 2. full lengths
def test_full_counts_give_the_bits_of_the_dense_entry_points(env):
    A = _check_case(env, 'full', gterm=True)
    specs = LR.case_specs('full')
    D = _dense_call(env, [(s[0], s[3], s[4]) for s in specs], gterm=True)
    sums = A['sums'].get().reshape(-1, 4)
    assert np.array_equal(sums[:, :3].reshape(-1).view(np.int64), D['sums'].get().view(np.int64))
    for k in ('sc', 'mag', 'total'):
        assert _bits_equal(A[k].get(), D[k].get()), k
    for a, d in zip(A['dx'], D['dx']):
        assert _bits_equal(a.get(), d.get())


def _module_run(dev, res, x, y, w_mag=1.0, **kw):
    from wavthruvec_pytorch_amd import MultiResolutionSTFTLoss
    xd = torch.from_numpy(x).to(dev).requires_grad_(True)
    sc, mag = MultiResolutionSTFTLoss(res)(xd, torch.from_numpy(y).to(dev), **kw)
    assert sc.dim() == 0 and mag.dim() == 0 and sc.is_cuda and mag.is_cuda and sc.requires_grad
    (sc + w_mag * mag).backward()
    _sync_or_stop('stft_loss lengths=%r' % (kw.get('lengths'),))
    return sc.detach().cpu().numpy(), mag.detach().cpu().numpy(), xd.grad.cpu().numpy()


def test_full_lengths_give_the_bits_of_the_call_without_lengths(env):
    dev = env[0]
    res = [(128, 32, 96), (128, 25, 100), (512, 50, 240)]
    B, L, m = 3, 1280, 4
    x, y = SL.signals(B, L)
    plain = _module_run(dev, res, x, y)
    for lens in ([L // m] * B, torch.full((B,), L // m, dtype=torch.int64, device=dev)):
        for a, b in zip(plain, _module_run(dev, res, x, y, lengths=lens, len_mul=m)):
            assert _bits_equal(a, b)


# ---------------------------------------------------------------------------------------------------------------
# 3. padding is inert
def test_padding_is_inert_and_gets_no_gradient(env):
    dev = env[0]
    res = [(128, 32, 96), (128, 48, 128), (512, 50, 240)]
    L, lens, m = 1536, [384, 201, 30, 9], 4                       # 1536, 804, 120 (no frame at 512 / 50 / 240: pad 231), 36 (no frame anywhere)
    x, y = SL.signals(len(lens), L)
    clean = _module_run(dev, res, x, y, lengths=lens, len_mul=m)
    assert all(np.isfinite(a).all() for a in clean)
    xn, yn = x.copy(), y.copy()
    for b, n in enumerate(LR.samples_of(lens, m, L)):
        xn[b, n:], yn[b, n:] = np.nan, np.nan
    for a, b in zip(clean, _module_run(dev, res, xn, yn, lengths=torch.tensor(lens, device=dev), len_mul=m)):
        assert _bits_equal(a, b), 'NaN past n_b changed the bits'
    dx = clean[2]
    for b, n in enumerate(LR.samples_of(lens, m, L)):
        assert _positive_zero(dx[b, n:]), b
    assert dx[0].any() and dx[1].any() and dx[2].any() and _positive_zero(dx[3])


# ---------------------------------------------------------------------------------------------------------------
# 4. no valid entry
def test_no_valid_entry_gives_zero_loss_and_zero_gradient(env):
    dev = env[0]
    x = np.full((3, 600), np.nan, dtype=np.float32)
    for lens in ([40, 1, 20], torch.tensor([40, 1, -5], device=dev)):                      # pad = 48 and 40: no reflection, no frame
        sc, mag, dx = _module_run(dev, [(128, 32, 128), (128, 48, 128)], x, x.copy(), lengths=lens)
        assert _positive_zero(sc) and _positive_zero(mag) and np.isfinite(dx).all() and not dx.any()


# ---------------------------------------------------------------------------------------------------------------
# 5. end to end against the ragged oracle
def _cases():
    return LR.small_cases() + [LR.large_case()]


@functools.lru_cache(maxsize=None)
def _scalar_bars():
    """4 x the largest relative float32-against-float64 gap of the ragged oracle over this file's case list, per quantity."""
    o = [LR.case_oracle(c) for c in _cases()]
    return 4 * max(g['rel_sc'] for g in o), 4 * max(g['rel_mag'] for g in o)


def _end_to_end(dev, case):
    from wavthruvec_pytorch_amd import stft_loss
    res, L, lens, len_mul, w_mag = case
    o = LR.case_oracle(case)
    x, y = SL.signals(len(lens), L)
    if len(res) == 1:
        xd = torch.from_numpy(x).to(dev).requires_grad_(True)
        sc, mag = stft_loss.stft_loss(xd, torch.from_numpy(y).to(dev).unsqueeze(1), *res[0], lengths=list(lens), len_mul=len_mul)
        (sc + w_mag * mag).backward()
        _sync_or_stop('stft_loss %s lengths=%r' % (S.gid(res[0]), lens))
        sc, mag, dx = sc.item(), mag.item(), xd.grad.cpu().numpy()
    else:
        sc, mag, dx = _module_run(dev, res, x, y, w_mag, lengths=list(lens), len_mul=len_mul)
        sc, mag = float(sc), float(mag)
    assert np.isfinite(dx).all() and dx.shape == x.shape
    for b, n in enumerate(LR.samples_of(lens, len_mul, L)):
        assert _positive_zero(dx[b, n:]), (case, b)
    e_sc, e_mag = abs(sc - o['sc']) / abs(o['sc']), abs(mag - o['mag']) / abs(o['mag'])
    e_dx = float(np.abs(dx - o['dx']).max())
    bar_sc, bar_mag = _scalar_bars()
    print('[stft loss, lengths] %s L=%d lens=%r x %d: sc %.6f mag %.6f; oracle f32 - f64 rel gaps sc %.3e mag %.3e dx %.3e (max |dx| %.3e); HIP - '
          'f64 rel sc %.3e mag %.3e dx %.3e; ratios to the bars sc %.3f mag %.3f (bars %.3e %.3e), dx / gap %.3f (bar 4)'
          % ('+'.join(S.gid(g) for g in res), L, tuple(lens), len_mul, o['sc'], o['mag'], o['rel_sc'], o['rel_mag'], o['gap_dx'],
             np.abs(o['dx']).max(), e_sc, e_mag, e_dx, e_sc / bar_sc, e_mag / bar_mag, bar_sc, bar_mag, e_dx / o['gap_dx']))
    return e_sc, bar_sc, e_mag, bar_mag, e_dx, 4 * o['gap_dx']


def _assert_figures(case, fig):
    e_sc, bar_sc, e_mag, bar_mag, e_dx, bar_dx = fig
    assert e_sc <= bar_sc and e_mag <= bar_mag and e_dx <= bar_dx, (case, fig)


@pytest.mark.parametrize('geo', S.SMALL, ids=S.gid)
def test_end_to_end_with_lengths_at_the_listed_lengths(env, geo):
    cases = [c for c in LR.small_cases() if c[0] == (geo,)]
    assert cases
    figures = [_end_to_end(env[0], c) for c in cases]
    for c, f in zip(cases, figures):
        _assert_figures(c, f)


def test_end_to_end_with_lengths_at_the_multi_resolution_setting(env):
    case = LR.large_case()
    _assert_figures(case, _end_to_end(env[0], case))


# ---------------------------------------------------------------------------------------------------------------
# 6. under autograd
def test_no_grad_and_no_requires_grad_give_the_same_bits_and_no_graph(env):
    from wavthruvec_pytorch_amd import MultiResolutionSTFTLoss
    dev = env[0]
    x, y = (torch.from_numpy(a).to(dev) for a in SL.signals(3, 600))
    m = MultiResolutionSTFTLoss([(128, 32, 96), (128, 25, 100)])
    kw = dict(lengths=[150, 97, 12], len_mul=4)
    a = m(x.clone().requires_grad_(True), y, **kw)
    b = m(x, y, **kw)
    with torch.no_grad():
        c = m(x.clone().requires_grad_(True), y, **kw)
    _sync_or_stop('stft_loss lengths no_grad')
    assert a[0].requires_grad and a[1].requires_grad
    assert not b[0].requires_grad and not c[0].requires_grad and b[0].grad_fn is None and c[1].grad_fn is None
    for u, v in zip(a + a, b + c):
        assert _bits_equal(u.detach().cpu().numpy(), v.cpu().numpy())
    dense = m(x, y)
    _sync_or_stop('stft_loss dense')
    assert not _bits_equal(dense[1].cpu().numpy(), b[1].cpu().numpy())                    # (the lengths were not ignored)
