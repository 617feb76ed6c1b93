"""GPU tests of the fused mel L1 training loss: the new entry points of csrc/v2w_mel.hip one by one, then `mel.mel_loss` end to end against
tests/mel_loss_ref.py (oracle/mel_oracle.py and torch autograd in fp64, item by item on the TRIMMED signals).  The cases, signals and targets
are tests/mel_loss_ref.py's (tests/test_mel_loss_cpu.py asserts the conditions the bounds rest on).

  1. v2w_mel_phases_len_bwd / _geo_len_bwd: bit for bit the B = 1 plain call on a dense copy of dxp[b, :, :FP_b]; +0.0 past n_b; NaN in the
     columns from FP_b on reaches nothing.
  2. v2w_mel_loss_fwd against fp64 on the same float32 spec.  Bound, from the operation counts (u = 2^-24, e = 2^-53): an entry's v is within
     tests/mel_ref.py's finish bound b_e of its fp64 value v64; fl(v - t) = (v - t)(1 + d), |d| <= u, |.| exact, so an entry's term is within
     b_e + u (|v64 - t| + b_e) of |v64 - t|.  Every sum is fp64 on non-negative terms: at most ceil(n_mels FT / 256) additions in a thread's
     chain, [6 + 4] in the workgroup's reduction, [tiles] over the item's partials, [1] the quotient; then [1] fp32 for the stored value:
         |per_item - want| <= (mean_e(b_e + u (|v64 - t| + b_e)) + want (u + n64 e)) (1 + 2 u),     n64 = ceil(n_mels FT / 256) + tiles + 12
     and for total the same over all valid entries with scale, n64 + ceil(B / 256) + 12 (the items' sums, the product with scale, the
     second quotient).  coef is the correctly rounded float32 of scale / (n_mels sum F_b), held bit for bit.  NaN / 1e30 in the target past
     F_b and in the spec frames past F_b reach nothing: the same bits as with clean padding.
  3. v2w_mel_loss_bwd against tests/mel_ref.py's fp64 finish backward with gout = coef * sign(v64 - t) under that module's own bound (the
     kernel's gout[0] * coef[0] is exact for gout = 1, and +-that / acc is the plain kernel's quotient).  dspec frames >= F_b stay 0.
  4. end to end: |loss - want| <= scale * 4 * max_b gap_out_b + 1e-6 |want| (an L1 of entries each within 4 gap_out of the oracle's, times
     scale / count summed over count entries; the fp64 sums add 1e-7 relative); d y_hat[b, :n_b] within 4 gap_dy_b of fp64 autograd; exact
     zeros past n_b; poisoned and clean padding, two runs: identical bits; permuting the items permutes per_item bit for bit.
     (With mel_spectrogram's one-launch input-gradient conv the 1024 / 256 / 1024 items stood at 2.7 - 9.5 gaps; mel_loss splits it by rows.)
  5. lengths = [L] * B gives the bits of lengths=None, loss and gradient; both target layouts give identical bits.
  6. every n_b <= pad: loss 0.0, gradient all +0.0.
  7. mel_spectrogram(lengths=...) under grad mode still raises NotImplementedError.
Measured on an MI355X (error / bound, bar 1; end to end error / the oracle's own float32 gap, bar 4): DESIGN.md 3d-loss.
Every test here fails without the feature: there is no mel.mel_loss and none of the new symbols."""
import math

import numpy as np
import pytest
import torch

from tests import mel_loss_ref as ML
from tests import mel_ref as R
from tests.test_disc_kernels_gpu import env  # noqa: F401  (the module-scoped fixture)
from tests.test_mel_kernels_gpu import _bits_equal
from tests.test_tile_kernels_gpu import _sync_or_stop

pytestmark = pytest.mark.gpu
OK = 0
U24, U53 = 2.0 ** -24, 2.0 ** -53
cases = pytest.mark.parametrize('c', ML.CASES, ids=ML.IDS)


def _geo(c):
    from wavthruvec_pytorch_amd import mel
    return mel.stft_geometry(*c['geo'])


def _poison(c, r, val_y, val_t):
    """y with val_y past every n_b, the target with val_t past every F_b."""
    y, t = r['y'].copy(), r['tgt'].copy()
    for b, (n, f) in enumerate(zip(r['ns'], r['Fb'])):
        y[b, n:], t[b, f:] = val_y, val_t
    return y, t


def _positive_zero(a):
    a = np.ascontiguousarray(a, dtype=np.float32)
    return not a.view(np.int32).any()


# ---------------------------------------------------------------------------------------------------------------
# 1. the phase backward with lengths
@cases
def test_phase_backward_with_lengths_is_the_trimmed_call_bit_for_bit(env, c):
    dev, _hip, lib, st = env
    g = _geo(c)
    B, L, mul = len(c['lens']), c['L'], c['len_mul']
    ns = ML.samples_of(c)
    F, _Ft, Fb = ML.frames_of(c)
    hop, cp, pad, k = g['hop'], g['cp'], g['pad'], g['k']
    FP = R.roundup4(F + k - 1)
    FPb = [R.roundup4(f + k - 1) if f else 0 for f in Fb]
    dxp = np.random.default_rng(c['seed']).standard_normal((B, cp, FP)).astype(np.float32)
    for b, fp in enumerate(FPb):
        dxp[b, :, fp:] = np.nan
    xd = torch.from_numpy(dxp).to(dev)
    ld = torch.tensor(c['lens'], dtype=torch.int32, device=dev)
    dy = torch.full((B, L), 7.0, device=dev)
    ints = lambda B_, L_, FP_: (B_, L_, g['n_fft'], g['win'], hop, cp, pad, g['left'], k, FP_)  # noqa: E731
    if g['old']:
        assert lib.v2w_mel_phases_len_bwd(xd.data_ptr(), dy.data_ptr(), B, L, hop, pad, FP, ld.data_ptr(), mul, st) == OK
    else:
        assert lib.v2w_mel_phases_geo_len_bwd(xd.data_ptr(), dy.data_ptr(), *ints(B, L, FP), ld.data_ptr(), mul, st) == OK
    _sync_or_stop('phase backward with lengths ' + c['name'])
    got = dy.cpu().numpy()
    assert np.isfinite(got).all()
    for b, (n, fp) in enumerate(zip(ns, FPb)):
        assert _positive_zero(got[b, n:]), (b, 'dy past n_b is not +0.0')
        if not fp:
            assert _positive_zero(got[b]), b
            continue
        own = torch.from_numpy(np.ascontiguousarray(dxp[b:b + 1, :, :fp])).to(dev)
        ref = torch.full((1, n), 7.0, device=dev)
        if g['old']:
            assert lib.v2w_mel_phases_bwd(own.data_ptr(), ref.data_ptr(), 1, n, hop, pad, fp, st) == OK
        else:
            assert lib.v2w_mel_phases_geo_bwd(own.data_ptr(), ref.data_ptr(), *ints(1, n, fp), st) == OK
        _sync_or_stop('the B = 1 phase backward ' + c['name'])
        assert _bits_equal(got[b, :n], ref.cpu().numpy()[0]), (b, n)


# ---------------------------------------------------------------------------------------------------------------
# 2. and 3. the fused entries on mel.py's own spec
def _spec_of(dev, c, r):
    from wavthruvec_pytorch_amd import mel
    ld = torch.tensor(c['lens'], dtype=torch.int32, device=dev)
    with torch.no_grad():
        spec, k, geom = mel._spectrum(torch.from_numpy(r['y']).to(dev), c['cfg'], ld, c['len_mul'])
    _sync_or_stop('spectrum ' + c['name'])
    return spec, k, geom, ld


def _fp64_entries(spec, basis, r, nb):
    """(v64, b_e, keep) on the float32 spec: tests/mel_ref.py's finish statement and bound over the frames f < F_b."""
    F = r['F']
    keep = np.arange(F)[None, :] < np.asarray(r['Fb'])[:, None]
    value, bound = R._finish(R._parts(spec, basis, F, nb, keep))
    return value, bound, keep


@cases
def test_fused_forward_entry_against_fp64_on_the_same_spec(env, c):
    from wavthruvec_pytorch_amd import mel
    dev = env[0]
    r = ML.reference(c)
    spec, k, geom, ld = _spec_of(dev, c, r)
    B, mels, F, Fb, scale, nb = len(c['lens']), c['mels'], r['F'], r['Fb'], c['scale'], k['nb']
    outs = []
    for val_s, val_t in ((None, 0.0), (float('nan'), 1e30), (1e30, float('nan'))):
        sp = spec.clone()
        if val_s is not None:
            for b, f in enumerate(Fb):
                sp[b, :, f:] = val_s
        tgt = torch.from_numpy(_poison(c, r, 0.0, val_t)[1]).to(dev)
        outs.append(mel._loss_launch(sp, k, geom, tgt, True, mels, ld, c['len_mul'], scale))
        _sync_or_stop('mel loss forward ' + c['name'])
    for o in outs[1:]:
        assert all(torch.equal(a, b) for a, b in zip(outs[0], o)), 'poisoned padding changed the bits'
    total, per, coef = (t.cpu().numpy() for t in outs[0])
    assert np.isfinite(total).all() and np.isfinite(per).all()
    assert _bits_equal(coef, np.float32(scale / (mels * sum(Fb))).reshape(1))
    v64, be, keep = _fp64_entries(spec.cpu().numpy(), k['basis'].cpu().numpy(), r, nb)
    d64 = np.abs(v64 - r['tgt'][:, :F].transpose(0, 2, 1).astype(np.float64))
    term = np.where(keep[:, None, :], be + U24 * (d64 + be), 0.0)
    d64 = np.where(keep[:, None, :], d64, 0.0)
    ft = 16 if nb * 64 <= 65536 else 8
    n64 = -(-mels * ft // 256) + -(-F // ft) + 12
    ratios = []
    for b, f in enumerate(Fb):
        if not f:
            assert per[b] == 0.0 and not np.signbit(per[b])
            continue
        want = d64[b].sum() / (mels * f)
        bound = (term[b].sum() / (mels * f) + want * (U24 + n64 * U53)) * (1 + 2 * U24)
        ratios.append(abs(float(per[b]) - want) / bound)
    n64 += -(-B // 256) + 12
    want = scale * d64.sum() / (mels * sum(Fb))
    bound = (scale * term.sum() / (mels * sum(Fb)) + want * (U24 + n64 * U53)) * (1 + 2 * U24)
    print('[mel loss] %s forward entry: per_item error / bound %.3f (worst of %d), total %.3f' % (c['name'], max(ratios), len(ratios),
                                                                                                   abs(float(total[0]) - want) / bound))
    assert max(ratios) <= 1 and abs(float(total[0]) - want) <= bound


@cases
def test_fused_backward_entry_against_the_fp64_finish_backward(env, c):
    from wavthruvec_pytorch_amd import mel
    dev, _hip, lib, st = env
    r = ML.reference(c)
    spec, k, geom, ld = _spec_of(dev, c, r)
    k = mel._bwd_constants(k)
    B, mels, F, Ft, Fb, scale, nb = len(c['lens']), c['mels'], r['F'], r['Ft'], r['Fb'], c['scale'], k['nb']
    FP = geom[4]
    sp = spec.clone()
    for b, f in enumerate(Fb):
        sp[b, :, f:] = float('nan')
    tgt = torch.from_numpy(_poison(c, r, 0.0, float('nan'))[1]).to(dev)
    coef = torch.tensor([scale / (mels * sum(Fb))], dtype=torch.float32, device=dev)
    gout = torch.ones(1, device=dev)
    dspec = torch.zeros_like(spec)
    assert lib.v2w_mel_loss_bwd(sp.data_ptr(), k['basis'].data_ptr(), k['basisT'].data_ptr(), tgt.data_ptr(), mels, 1, gout.data_ptr(),
                                coef.data_ptr(), dspec.data_ptr(), B, k['cs'], FP, F, Ft, nb, mels, ld.data_ptr(), c['len_mul'], k['hop'],
                                k['n_fft'], st) == OK
    _sync_or_stop('mel loss backward ' + c['name'])
    got = dspec.cpu().numpy()
    own = np.zeros(got.shape, dtype=bool)
    for b, f in enumerate(Fb):
        own[b, :2 * nb, :f] = True
    assert _positive_zero(got[~own]), 'dspec was written outside rows < 2 nb of the frames < F_b'
    spec0, basis = spec.cpu().numpy(), k['basis'].cpu().numpy()
    v64, _be, keep = _fp64_entries(spec0, basis, r, nb)
    sign = np.sign(v64 - r['tgt'][:, :F].transpose(0, 2, 1).astype(np.float64))
    G = np.where(keep[:, None, :], np.float32(coef.item()) * sign, 0.0).astype(np.float32)
    value, bound = R.finish_bwd(spec0, basis, G, F, nb)
    ratio = R.worst_ratio(got[:, :2 * nb, :F], value, bound)
    print('[mel loss] %s backward entry: error / bound %.3f' % (c['name'], ratio))
    assert ratio <= 1


# ---------------------------------------------------------------------------------------------------------------
# 4. end to end
def _run(dev, c, y, tgt, lens, **kw):
    from wavthruvec_pytorch_amd import mel_loss
    yd = torch.from_numpy(y).to(dev).requires_grad_(True)
    loss, per = mel_loss(yd, torch.from_numpy(tgt).to(dev), *c['cfg'], lengths=lens, len_mul=c['len_mul'], scale=c['scale'], per_item=True, **kw)
    assert loss.dim() == 0 and loss.requires_grad and per.shape == (y.shape[0],) and not per.requires_grad
    loss.backward()
    _sync_or_stop('mel_loss ' + c['name'])
    return loss.detach().cpu().numpy(), per.cpu().numpy(), yd.grad.cpu().numpy()


@cases
def test_end_to_end_against_the_fp64_reference(env, c):
    dev = env[0]
    r = ML.reference(c)
    B, ns, Fb, scale = len(c['lens']), r['ns'], r['Fb'], c['scale']
    clean = _run(dev, c, r['y'], r['tgt'], c['lens'])
    loss, per, dy = clean
    assert np.isfinite(loss) and np.isfinite(per).all() and np.isfinite(dy).all()
    for val_y, val_t in ((float('nan'), 1e30), (1e30, float('nan'))):
        y, t = _poison(c, r, val_y, val_t)
        for a, b in zip(clean, _run(dev, c, y, t, torch.tensor(c['lens'], device=dev))):         # (device lengths: the same bits too)
            assert _bits_equal(a, b), 'poisoned padding or a second run changed the bits'
    bar = scale * 4 * max(r['gap_out']) + 1e-6 * abs(r['want'])
    e_dy = [float(np.abs(dy[b, :n] - r['dy'][b, :n]).max()) if f else 0.0 for b, (n, f) in enumerate(zip(ns, Fb))]
    with np.errstate(divide='ignore', invalid='ignore'):
        ratios = [e / g if g else 0.0 for e, g in zip(e_dy, r['gap_dy'])]
    print('[mel loss] %s end to end: loss %.7f want %.7f, |d| %.3e bar %.3e; d y error / oracle f32 - f64 gap per item %s (bar 4)'
          % (c['name'], loss, r['want'], abs(loss - r['want']), bar, ' '.join('%.2f' % x for x in ratios)))
    assert abs(float(loss) - r['want']) <= bar
    for b, (n, f) in enumerate(zip(ns, Fb)):
        assert _positive_zero(dy[b, n:]), (b, 'd y_hat past n_b is not +0.0')
        if f:
            assert e_dy[b] <= 4 * r['gap_dy'][b], (b, e_dy[b], r['gap_dy'][b])
            assert abs(float(per[b]) - r['per'][b]) <= 4 * r['gap_out'][b] + 1e-6 * r['per'][b], b
        else:
            assert _positive_zero(dy[b]) and _positive_zero(per[b:b + 1]), b
    # an item's bits do not depend on its neighbours
    perm = list(range(B))[::-1]
    _l, per2, _d = _run(dev, c, r['y'][perm], r['tgt'][perm], [c['lens'][i] for i in perm])
    assert _bits_equal(per2, per[perm])


# ---------------------------------------------------------------------------------------------------------------
# 5. full lengths, the two layouts
@pytest.mark.parametrize('name', ['samples', '128_25_100', '2048_240_1200'])
def test_full_lengths_and_both_layouts_give_the_bits_of_no_lengths(env, name):
    from wavthruvec_pytorch_amd import mel_loss
    dev = env[0]
    c = next(x for x in ML.CASES if x['name'] == name)
    B, L = len(c['lens']), c['L']
    r = ML.reference(c)
    y = r['y']
    tgt = np.random.default_rng(L).standard_normal(r['tgt'].shape).astype(np.float32) * 2 - 5
    plain = _run(dev, c, y, tgt, None)
    for lens in ([L] * B, torch.full((B,), L, dtype=torch.int32, device=dev)):
        for a, b in zip(plain, _run(dev, c, y, tgt, lens)):
            assert _bits_equal(a, b)
    tm = np.ascontiguousarray(tgt.transpose(0, 2, 1))
    for lens in (None, c['lens']):
        a, b = _run(dev, c, y, tgt, lens), _run(dev, c, y, tm, lens, frames_first=False)
        assert all(_bits_equal(p, q) for p, q in zip(a, b)), 'the two target layouts differ'
    # (B, 1, L), no grad, no per_item: the same loss bits
    with torch.no_grad():
        l3 = mel_loss(torch.from_numpy(y).to(dev)[:, None], torch.from_numpy(tgt).to(dev), *c['cfg'], scale=c['scale'])
    _sync_or_stop('mel_loss no grad')
    assert l3.dim() == 0 and not l3.requires_grad and _bits_equal(l3.cpu().numpy(), plain[0])
    # against torch on the device's own mel: F.l1_loss reduces N elements in fp32, within N u relative of the exact mean
    from wavthruvec_pytorch_amd.mel import mel_spectrogram
    F = r['F']
    with torch.no_grad():
        m = mel_spectrogram(torch.from_numpy(y).to(dev), *c['cfg']).permute(0, 2, 1).double()
        want = c['scale'] * torch.nn.functional.l1_loss(torch.from_numpy(tgt).to(dev)[:, :F].double(), m).item()
    assert abs(float(plain[0]) - want) <= 4 * U24 * want


# ---------------------------------------------------------------------------------------------------------------
# 6. nothing valid
def test_no_valid_entry_gives_zero_loss_and_zero_gradient(env):
    from wavthruvec_pytorch_amd import mel_loss
    dev = env[0]
    c = ML.CASES[0]
    y = np.full((3, 4100), np.nan, dtype=np.float32)
    tgt = np.full((3, 18, 80), np.nan, dtype=np.float32)
    for lens in ([384, 1, 100], torch.tensor([384, 1, -5], device=dev)):                  # pad = 384: no reflection, no frame
        yd = torch.from_numpy(y).to(dev).requires_grad_(True)
        loss, per = mel_loss(yd, torch.from_numpy(tgt).to(dev), *c['cfg'], lengths=lens, scale=45.0, per_item=True)
        loss.backward()
        _sync_or_stop('mel_loss without a valid entry')
        assert _positive_zero(loss.detach().cpu().numpy()) and _positive_zero(per.cpu().numpy()) and _positive_zero(yd.grad.cpu().numpy())


# ---------------------------------------------------------------------------------------------------------------
# 7. nothing changed
def test_mel_spectrogram_with_lengths_still_refuses_under_grad_mode(env):
    from wavthruvec_pytorch_amd.mel import mel_spectrogram
    y = torch.zeros(2, 4100, device=env[0]).requires_grad_(True)
    with pytest.raises(NotImplementedError):
        mel_spectrogram(y, *ML.CASES[0]['cfg'], lengths=[4100, 400])
    assert math.isfinite(mel_spectrogram(y, *ML.CASES[0]['cfg']).sum().item())
