"""The parameter-space backward kernels of csrc/v2w_backward.hip - `cbn_backward`, `cond_backward`, `wn_backward` - each against the fp64
autograd reference of its own operation (tests/backward_ref.py), per entry, at the shapes of the training step and at the edges of
their loops.  Every tolerance is a forward-error bound computed from the reference's data (backward_ref.*_bounds); each test prints the
worst error / bound ratio it saw (`-s` shows them), and a ratio above 1 fails.

Worst ratios measured on an MI355X when these tests were written (the 128 u allowance for fp32 chains is what makes the sums look easy):
  cbn_backward   dxr 0.061 train / 0.49 eval, dgamma 7.2e-3, dbeta 1.2e-3, sum dxr 4.8e-3, sum dxr (xr - mean) 0.045; sync hook dxr 0.057
  cond_backward  d weight_orig 0.10, d bias 0.27, d fc_w 0.086, d fc_b 0.073
  wn_backward    dv 0.25, dg 0.50 (one rounding of an fp64 value against 4u / 2u); against the fold kernel's central difference 0.028 of 1e-3
One-line mutants of v2w_backward.hip these tests fail on: `- mean * S1` dropped from dgamma (every cbn case), `Cc[row % C]` read as `Cc[0]`
(the train-mode cbn cases), `u[r] * v[j]` dropped from phase 3 of cond_bwd_kernel (every cond case), the transposed index order of
wn_bwd_kernel's dw_at swapped (every transposed wn case)."""
import numpy as np
import pytest
import torch

from oracle import vec2wav_oracle as O
from tests import backward_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a MI355X'
    from wavthruvec_pytorch_amd import _hip
    _hip.load()
    return torch.device('cuda:0')


def _f32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))


def _report(name, **ratios):
    print(f'[ratio] {name}: ' + '  '.join(f'{k}={v:.3g}' for k, v in ratios.items()))
    for k, v in ratios.items():
        assert v <= 1.0, f'{name}: {k} misses its bound, error / bound = {v:.3g}'


# ---------------------------------------------------------------------------------------------------------------
# cbn_backward
CBN_GENERATOR = [(4, 256, 1280), (4, 128, 5120), (3, 64, 20480), (2, 32, 40960), (2, 16, 81920),     # the five stages at T = 256, B reduced
                 (32, 256, 1280)]                                                                   # the training step's 8 192 rows
CBN_EDGES = [(2, 16, 1), (3, 24, 255), (2, 70, 257),     # C not a multiple of the 64-thread block, L around the 256-thread stride
             (5, 8, 16385)]                               # one element past 256 chains of 64 terms
CBN_CASES = [(s, t) for s in CBN_GENERATOR + CBN_EDGES for t in (True, False)] + [((1, 16, 1), False)]
OFFSET_OVER_SCALE = (0.0, 10.0, 100.0)                    # per channel, cycling: |mean| / std of the normalised input


def _cbn_inputs(B, C, L, seed, constant_channel=None):
    r = np.random.default_rng(seed)
    scale = 0.5 + r.random(C)
    offset = scale * np.array([OFFSET_OVER_SCALE[c % 3] for c in range(C)])
    xr = _f32(offset[None, :, None] + scale[None, :, None] * r.standard_normal((B, C, L)))
    if constant_channel is not None:
        xr[:, constant_channel, :] = 0.5
    dx = _f32(r.standard_normal((B, C, L)))
    gb = _f32(np.concatenate((1 + 0.2 * r.standard_normal((B, C)), 0.3 * r.standard_normal((B, C))), axis=1))
    rmean = _f32(offset + 0.1 * scale * r.standard_normal(C))          # eval mode: running statistics near, not at, the batch's
    rvar = _f32(scale ** 2 * (0.5 + r.random(C)))
    x64 = xr.double()
    stats = torch.cat((x64.sum(dim=(0, 2)), x64.pow(2).sum(dim=(0, 2)), torch.tensor([float(B * L)], dtype=torch.float64)))
    return dx, xr, gb, stats, rmean, rvar


def _cbn_gpu(dev, dx, xr, gb, stats, rmean, rvar, training, sync=None):
    from wavthruvec_pytorch_amd import hipops
    dxr, dgb = hipops.cbn_backward(dx.to(dev), xr.to(dev), gb.to(dev), stats.to(dev) if training else None, rmean.to(dev), rvar.to(dev),
                                   training=training, eps=O.BN_EPS, sync=sync)
    torch.cuda.synchronize()
    return dxr.cpu(), dgb.cpu()


def _cbn_identity_ratios(dxr, dx, xr, gb, terms):
    """Train mode, per channel, on the kernel's own output: sum dxr = 0 and sum dxr (xr - mean) = eps rstd^3 sum gamma dx (xr - mean)
    (backward_ref.cbn_centered_moment_ref), each a sum of the products |a dx| + |bc xr| + |cc| under the reduction bound."""
    xc = (xr.double() - xr.double().mean(dim=(0, 2), keepdim=True)).abs()
    zero = torch.zeros(dx.shape[1], dtype=torch.float64)
    m0 = R.worst_ratio(dxr.double().sum(dim=(0, 2)), zero, R.sum_bound(terms.sum(dim=(0, 2)), zero))
    want = R.cbn_centered_moment_ref(dx, xr, gb)
    m1 = R.worst_ratio(R.cbn_centered_moment(dxr, xr), want, R.sum_bound((terms * xc).sum(dim=(0, 2)), want))
    return m0, m1


@pytest.mark.parametrize('shape,training', CBN_CASES, ids=lambda v: 'x'.join(map(str, v)) if isinstance(v, tuple) else ('train' if v else 'eval'))
def test_cbn_backward_matches_fp64(dev, shape, training):
    """dxr per element and dgb per (item, channel) entry; in train mode the two moment identities of dxr as well."""
    B, C, L = shape
    dx, xr, gb, stats, rmean, rvar = _cbn_inputs(B, C, L, seed=100 + C + L % 97)
    want_dxr, want_dgb = R.cbn_ref(dx, xr, gb, training, rmean, rvar)
    bnd = R.cbn_bounds(dx, xr, gb, training, rmean, rvar)
    dxr, dgb = _cbn_gpu(dev, dx, xr, gb, stats, rmean, rvar, training)
    ratios = dict(dxr=R.worst_ratio(dxr, want_dxr, bnd.dxr), dgamma=R.worst_ratio(dgb[:, :C], want_dgb[:, :C], bnd.dgb[:, :C]),
                  dbeta=R.worst_ratio(dgb[:, C:], want_dgb[:, C:], bnd.dgb[:, C:]))
    if training:
        ratios['sum_dxr'], ratios['sum_dxr_xc'] = _cbn_identity_ratios(dxr, dx, xr, gb, bnd.terms)
    _report(f'cbn {shape} {"train" if training else "eval"}', **ratios)


def test_cbn_backward_constant_channel(dev):
    """A channel that is 0.5 everywhere has batch variance 0: rstd = eps^-1/2, and kernel and reference agree on finite values."""
    B, C, L, cst = 3, 24, 255, 5
    dx, xr, gb, stats, rmean, rvar = _cbn_inputs(B, C, L, seed=7, constant_channel=cst)
    assert stats[C + cst].item() / stats[2 * C].item() - (stats[cst].item() / stats[2 * C].item()) ** 2 == 0.0
    want_dxr, want_dgb = R.cbn_ref(dx, xr, gb, True, rmean, rvar)
    assert torch.isfinite(want_dxr).all() and torch.isfinite(want_dgb).all()
    assert want_dgb[:, cst].abs().max().item() == 0.0                    # xhat = 0 on that channel
    bnd = R.cbn_bounds(dx, xr, gb, True, rmean, rvar)
    dxr, dgb = _cbn_gpu(dev, dx, xr, gb, stats, rmean, rvar, True)
    assert torch.isfinite(dxr).all() and torch.isfinite(dgb).all()
    m0, m1 = _cbn_identity_ratios(dxr, dx, xr, gb, bnd.terms)
    _report('cbn constant channel', dxr=R.worst_ratio(dxr, want_dxr, bnd.dxr), dgb=R.worst_ratio(dgb, want_dgb, bnd.dgb),
            dxr_cst=R.worst_ratio(dxr[:, cst], want_dxr[:, cst], bnd.dxr[:, cst]), sum_dxr=m0, sum_dxr_xc=m1)


@pytest.mark.parametrize('shape', [(3, 24, 255), (2, 64, 5120)], ids=lambda v: 'x'.join(map(str, v)))
def test_cbn_backward_sync_hook_is_two_identical_ranks(dev, shape):
    """`sync` doubling the per-channel sums, with the statistics doubled too, is a data-parallel run of two ranks holding the same batch:
    the result is the first half of the reference on cat([x, x])."""
    B, C, L = shape
    dx, xr, gb, stats, rmean, rvar = _cbn_inputs(B, C, L, seed=11)
    dx2, xr2, gb2 = (torch.cat((t, t), dim=0) for t in (dx, xr, gb))
    want_dxr, want_dgb = R.cbn_ref(dx2, xr2, gb2, True, rmean, rvar)
    bnd = R.cbn_bounds(dx2, xr2, gb2, True, rmean, rvar)
    calls = []

    def sync(csum):
        calls.append(tuple(csum.shape))
        csum.mul_(2)

    dxr, dgb = _cbn_gpu(dev, dx, xr, gb, 2 * stats, rmean, rvar, True, sync=sync)
    assert calls == [(2 * C,)]
    _report(f'cbn sync {shape}', dxr=R.worst_ratio(dxr, want_dxr[:B], bnd.dxr[:B]), dgb=R.worst_ratio(dgb, want_dgb[:B], bnd.dgb[:B]))
    # and the hook is what made it so: without it the local sums are divided by the doubled count
    plain, _ = _cbn_gpu(dev, dx, xr, gb, 2 * stats, rmean, rvar, True)
    assert R.worst_ratio(plain, want_dxr[:B], bnd.dxr[:B]) > 1.0


# ---------------------------------------------------------------------------------------------------------------
# cond_backward
def _cond_inputs(B, C, spk_dim, noise_dim, seed):
    r = np.random.default_rng(seed)
    Rr, D = 2 * C, spk_dim + noise_dim
    W = _f32(0.5 + 0.5 * r.standard_normal((Rr, 128)))
    b = _f32(0.1 * r.standard_normal(Rr))
    # one power iteration from a random start, as the train-mode forward does; then constants
    u0 = torch.from_numpy(r.standard_normal(Rr))
    v = torch.nn.functional.normalize(W.double().t() @ u0, dim=0)
    u = torch.nn.functional.normalize(W.double() @ v, dim=0).float()
    v = v.float()
    sigma = torch.dot(u, torch.mv(W, v)).reshape(1)                       # fp32, as the forward computes it
    fc_w = _f32((2 * r.random((128, D)) - 1) / np.sqrt(D))
    fc_b = _f32(0.05 * r.standard_normal(128))
    spk, noise = _f32(r.standard_normal((B, spk_dim))), _f32(r.standard_normal((B, noise_dim)))
    dgb = _f32(r.standard_normal((B, Rr)))
    z = (torch.cat((spk, noise), 1).double() @ fc_w.double().t() + fc_b.double()).float()
    return dict(dgb=dgb, W=W, b=b, u=u, v=v, fc_w=fc_w, fc_b=fc_b, spk=spk, noise=noise), z, sigma


def _cond_ratios(got, p, sigma):
    want = R.cond_ref(**p)
    bnd = R.cond_bounds(**p, sigma_used=sigma.item())
    for g, w in zip(got, want):
        assert g.shape == w.shape
    return dict(zip(('d_weight_orig', 'd_bias', 'd_fc_w', 'd_fc_b'), (R.worst_ratio(g, w, b) for g, w, b in zip(got, want, bnd))))


@pytest.mark.parametrize('spk_dim,noise_dim', [(192, 192), (192, 10), (64, 1)])
@pytest.mark.parametrize('B,C', [(1, 16), (2, 256), (32, 64), (64, 128), (5, 24)])
def test_cond_backward_matches_fp64(dev, B, C, spk_dim, noise_dim):
    """All four outputs per entry.  D = 384 is three full passes of the 128-thread loop over the fc inputs; 202 and 65 end mid-pass."""
    from wavthruvec_pytorch_amd import hipops
    p, z, sigma = _cond_inputs(B, C, spk_dim, noise_dim, seed=B + C + noise_dim)
    got = hipops.cond_backward(p['dgb'].to(dev), z.to(dev), p['W'].to(dev), p['u'].to(dev), p['v'].to(dev), sigma.to(dev),
                               p['spk'].to(dev), p['noise'].to(dev))
    torch.cuda.synchronize()
    _report(f'cond B={B} C={C} D={spk_dim}+{noise_dim}', **_cond_ratios([g.cpu() for g in got], p, sigma))


def test_cond_backward_reads_nothing_stale_from_its_workspace(dev):
    """Phase 1 writes dz into the workspace and phase 2 the scalar at word B * 128; phases 3 and 4 read them back.  Two problems of different
    B run back to back through ONE oversized workspace that starts as NaN: every word either problem reads, it has written itself."""
    from wavthruvec_pytorch_amd import _hip
    lib = _hip.load()
    ws = torch.full((64 * 128 + 1 + 4096,), float('nan'), device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    for B, C, spk_dim, noise_dim in [(5, 24, 64, 1), (2, 16, 192, 10), (5, 24, 64, 1)]:
        p, z, sigma = _cond_inputs(B, C, spk_dim, noise_dim, seed=31 + B)
        d = {k: t.to(dev) for k, t in p.items()}
        zd, sd = z.to(dev), sigma.to(dev)
        outs = [torch.full(s, float('nan'), device=dev) for s in ((2 * C, 128), (2 * C,), (128, spk_dim + noise_dim), (128,))]
        _hip.check(lib.v2w_cond_bwd(d['dgb'].data_ptr(), zd.data_ptr(), d['W'].data_ptr(), d['u'].data_ptr(), d['v'].data_ptr(), sd.data_ptr(),
                                    d['spk'].data_ptr(), d['noise'].data_ptr(), *(o.data_ptr() for o in outs), ws.data_ptr(),
                                    B, C, spk_dim, noise_dim, st), 'v2w_cond_bwd')
        torch.cuda.synchronize()
        _report(f'cond shared workspace B={B} C={C}', **_cond_ratios([o.cpu() for o in outs], p, sigma))
        assert torch.isfinite(ws[:B * 128 + 1]).all() and torch.isnan(ws[64 * 128 + 1:]).all()


# ---------------------------------------------------------------------------------------------------------------
# wn_backward
WN_CONV = [(512, 768, 7), (256, 256, 11), (16, 16, 3), (1, 16, 7), (24, 40, 5)]            # (C_out, C_in, k): test_wn_fold_conv's shapes
WN_CONVT = [(512, 256, 11), (32, 16, 4), (512, 256, 16), (20, 12, 6)]                       # (C_in, C_out, k): test_wn_fold_convt's shapes
WN_CASES = [(s, False) for s in WN_CONV] + [(s, True) for s in WN_CONVT]


def _wn_inputs(shape, transposed, seed):
    """Rows of weight_v with ||v|| spread over 1e-3 ... 1e3, weight_g of either sign."""
    r = np.random.default_rng(seed)
    d0, d1, k = shape
    ci, co = (d0, d1) if transposed else (d1, d0)
    norms = 10.0 ** np.linspace(-3, 3, d0) if d0 > 1 else np.array([1e-3])
    r.shuffle(norms)
    v = r.standard_normal((d0, d1, k))
    v = _f32(v / np.sqrt((v ** 2).sum(axis=(1, 2), keepdims=True)) * norms[:, None, None])
    g = _f32((1 + 0.1 * r.standard_normal((d0, 1, 1))) * np.where(r.random((d0, 1, 1)) < 0.5, -1.0, 1.0))
    dwf = _f32(r.standard_normal((k, ci, co)))
    return dwf, v, g


@pytest.mark.parametrize('shape,transposed', WN_CASES, ids=lambda v: 'x'.join(map(str, v)) if isinstance(v, tuple) else ('convt' if v else 'conv'))
def test_wn_backward_matches_fp64(dev, shape, transposed):
    from wavthruvec_pytorch_amd import hipops
    dwf, v, g = _wn_inputs(shape, transposed, seed=5)
    want_dv, want_dg = R.wn_ref(dwf, v, g, transposed)
    b_dv, b_dg = R.wn_bounds(dwf, v, g, transposed)
    dv, dg = hipops.wn_backward(dwf.to(dev), v.to(dev), g.to(dev), transposed)
    assert dv.shape == v.shape and dg.shape == g.shape
    _report(f'wn {shape} {"convt" if transposed else "conv"}', dv=R.worst_ratio(dv.cpu(), want_dv, b_dv), dg=R.worst_ratio(dg.cpu(), want_dg, b_dg))
    # weight norm removed: the parameter is the weight, its gradient the relayout - bit for bit
    plain, none = hipops.wn_backward(dwf.to(dev), v.to(dev), None, transposed)
    assert none is None and torch.equal(plain.cpu(), R.wn_ref(dwf, v, None, transposed)[0])


@pytest.mark.parametrize('shape,transposed', WN_CASES, ids=lambda v: 'x'.join(map(str, v)) if isinstance(v, tuple) else ('convt' if v else 'conv'))
def test_wn_backward_differentiates_the_fold_kernel(dev, shape, transposed):
    """<dv, dv_dir> + <dg, dg_dir> against the central difference of <dwf, fold(v, g)> along (dv_dir, dg_dir), with fold the forward's own
    kernel (its fp32 outputs cast to fp64): the backward differentiates what the forward computes, the [k][C_in][C_out] layout included.
    The step h = 2^-8 of a direction as large as (v, g) leaves a truncation error of order h^2 and a rounding error of order u / h, both
    near 1e-5 of the terms: 1e-3 of the two inner products' magnitudes is the (loose) tolerance."""
    from wavthruvec_pytorch_amd import hipops
    dwf, v, g = _wn_inputs(shape, transposed, seed=6)
    r = np.random.default_rng(8)
    row_norm = v.double().pow(2).sum(dim=(1, 2), keepdim=True).sqrt()
    dv_dir = torch.from_numpy(r.standard_normal(tuple(v.shape))) * row_norm / np.sqrt(v[0].numel())
    dg_dir = torch.from_numpy(r.standard_normal(tuple(g.shape)))
    h = 2.0 ** -8
    fold = hipops.fold_convt_weight if transposed else hipops.fold_conv_weight
    vp, vm = (v.double() + h * dv_dir).float(), (v.double() - h * dv_dir).float()
    gp, gm = (g.double() + h * dg_dir).float(), (g.double() - h * dg_dir).float()
    dv_dir, dg_dir = (vp.double() - vm.double()) / (2 * h), (gp.double() - gm.double()) / (2 * h)     # the step really taken, after rounding
    f_p = (fold(vp.to(dev), gp.to(dev)).cpu().double() * dwf.double()).sum().item()
    f_m = (fold(vm.to(dev), gm.to(dev)).cpu().double() * dwf.double()).sum().item()
    fd = (f_p - f_m) / (2 * h)
    dv, dg = hipops.wn_backward(dwf.to(dev), v.to(dev), g.to(dev), transposed)
    a_v, a_g = (dv.cpu().double() * dv_dir).sum().item(), (dg.cpu().double() * dg_dir).sum().item()
    err, scale = abs(a_v + a_g - fd), abs(a_v) + abs(a_g)
    print(f'[ratio] wn vs fold {shape}: <dv,.>={a_v:.6g} <dg,.>={a_g:.6g} fd={fd:.6g} err/(1e-3 scale)={err / (1e-3 * scale):.3g}')
    assert err <= 1e-3 * scale
