"""The fp64 references of tests/backward_ref.py are themselves checked here, without a GPU: each against a central finite difference of
the forward it differentiates (written out again below, without autograd), and all three chained through one stage of the synthetic
generator against the whole-model oracle gradients."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import vec2wav_oracle as O
from tests import backward_ref as R


def _rand(r, *shape):
    return torch.from_numpy(r.standard_normal(shape))


def _directional(f, params, grads, r, h=1e-6):
    """(central difference of f along a random direction, <grads, direction>)."""
    deltas = [_rand(r, *p.shape) for p in params]
    with torch.no_grad():
        fp = f(*[p + h * d for p, d in zip(params, deltas)])
        fm = f(*[p - h * d for p, d in zip(params, deltas)])
    fd = (fp - fm).item() / (2 * h)
    an = sum((g * d).sum().item() for g, d in zip(grads, deltas))
    return fd, an


@pytest.mark.parametrize('training', [True, False])
def test_cbn_ref_matches_finite_differences(training):
    r = np.random.default_rng(1)
    B, C, L = 3, 4, 5
    xr, dx = 2.0 + 1.5 * _rand(r, B, C, L), _rand(r, B, C, L)
    gb = torch.cat((1 + 0.2 * _rand(r, B, C), 0.3 * _rand(r, B, C)), dim=1)
    rm, rv = 0.1 * _rand(r, C), 0.5 + torch.from_numpy(r.random(C))

    def f(xr_, gb_):
        if training:
            mean = xr_.mean(dim=(0, 2), keepdim=True)
            var = ((xr_ - mean) ** 2).mean(dim=(0, 2), keepdim=True)
        else:
            mean, var = rm[None, :, None], rv[None, :, None]
        x = gb_[:, :C, None] * (xr_ - mean) / torch.sqrt(var + 1e-5) + gb_[:, C:, None]
        return (x * dx).sum()

    dxr, dgb = R.cbn_ref(dx, xr, gb, training, rm, rv)
    assert dxr.dtype == torch.float64 and dxr.shape == xr.shape and dgb.shape == gb.shape
    for _ in range(3):
        fd, an = _directional(f, (xr, gb), (dxr, dgb), r)
        assert abs(fd - an) <= 1e-7 * max(1.0, abs(an)), (fd, an)
    if training:    # the identities of the batch statistics (the first is why d(ups.*.bias) = 0 in train mode)
        assert dxr.sum(dim=(0, 2)).abs().max().item() <= 1e-12
        got, want = R.cbn_centered_moment(dxr, xr), R.cbn_centered_moment_ref(dx, xr, gb)
        assert (got - want).abs().max().item() <= 1e-12 and want.abs().min().item() > 1e-7      # eps keeps it away from 0


def test_cond_ref_matches_finite_differences():
    r = np.random.default_rng(2)
    B, C, ds, dn = 3, 4, 5, 2
    W, b = 1 + 0.3 * _rand(r, 2 * C, 128), _rand(r, 2 * C)
    u, v = F.normalize(_rand(r, 2 * C), dim=0), F.normalize(_rand(r, 128), dim=0)
    fc_w, fc_b = _rand(r, 128, ds + dn) / 3, _rand(r, 128)
    spk, noise, dgb = _rand(r, B, ds), _rand(r, B, dn), _rand(r, B, 2 * C)

    def f(W_, b_, fw_, fb_):
        z = torch.cat((spk, noise), 1) @ fw_.t() + fb_
        sigma = (u[:, None] * W_ * v[None, :]).sum()
        return ((z @ W_.t() / sigma + b_) * dgb).sum()

    grads = R.cond_ref(dgb, W, b, u, v, fc_w, fc_b, spk, noise)
    assert [g.shape for g in grads] == [W.shape, b.shape, fc_w.shape, fc_b.shape]
    for _ in range(3):
        fd, an = _directional(f, (W, b, fc_w, fc_b), grads, r)
        assert abs(fd - an) <= 1e-7 * max(1.0, abs(an)), (fd, an)


@pytest.mark.parametrize('transposed', [False, True])
def test_wn_ref_matches_finite_differences(transposed):
    r = np.random.default_rng(3)
    d0, d1, k = 3, 5, 4                                   # (C_out, C_in, k) of a conv, (C_in, C_out, k) of a transposed conv
    ci, co = (d0, d1) if transposed else (d1, d0)
    v, g, dwf = _rand(r, d0, d1, k), _rand(r, d0, 1, 1), _rand(r, k, ci, co)

    def f(v_, g_):
        w = torch.empty_like(v_)
        for row in range(d0):
            w[row] = g_[row, 0, 0] * v_[row] / torch.sqrt((v_[row] ** 2).sum())
        tot = 0.0
        for t in range(k):                               # the [k][C_in][C_out] layout, index by index
            for a in range(ci):
                for o in range(co):
                    tot = tot + dwf[t, a, o] * (w[a, o, t] if transposed else w[o, a, t])
        return tot

    dv, dg = R.wn_ref(dwf, v, g, transposed)
    assert dv.shape == v.shape and dg.shape == g.shape
    for _ in range(3):
        fd, an = _directional(f, (v, g), (dv, dg), r)
        assert abs(fd - an) <= 1e-7 * max(1.0, abs(an)), (fd, an)
    plain, none = R.wn_ref(dwf, v, None, transposed)
    assert none is None and plain.is_contiguous()
    assert torch.equal(R.param_to_wf_layout(plain, transposed), dwf)
    t, a, o = 2, 1, 2
    assert plain[(a, o, t) if transposed else (o, a, t)] == dwf[t, a, o]


def test_chained_refs_match_whole_model_oracle_gradients():
    """Stage 0 of the synthetic B = 2, T = 8 generator in fp64: the cotangent at the CondBN output goes through cbn_ref, cond_ref and
    (via the transposed convolution's weight gradient) wn_ref, and lands on the oracle's gradients of cbns.0 / fcs.0 / ups.0."""
    from wavthruvec_pytorch_amd import synthetic
    dt = torch.float64
    h = synthetic.make_hparams(num_wv_feat=768)
    sd = synthetic.make_state_dict(h, seed=5)
    x, spk, nz = synthetic.make_inputs(h, 2, 8, seed=9)
    dy = torch.from_numpy(np.random.default_rng(4).standard_normal((2, 1, 8 * synthetic.total_upsample(h))))
    _, want, nb = O.generator_gradients(sd, h, x, spk, nz, dy, training=True, dtype=dt)

    # the same graph once more, to read the cotangent at the CondBN output off it
    probes = {}
    y, _ = O.generator_forward_impl({k: (v.to(dt).requires_grad_(True) if v.is_floating_point() else v) for k, v in sd.items()},
                                    h, x, spk, nz, True, dt, probes)
    dx, = torch.autograd.grad((y * dy).sum(), probes['cbns.0'])
    xr, pre = probes['ups.0'].detach(), probes['conv_pre'].detach()

    p = 'cbns.0'
    W, b = sd[p + '.layer.weight_orig'].to(dt), sd[p + '.layer.bias'].to(dt)
    u, v = nb[p + '.layer.weight_u'].to(dt), nb[p + '.layer.weight_v'].to(dt)     # the vectors after the forward's power iteration
    fc_w, fc_b = sd['fcs.0.weight'].to(dt), sd['fcs.0.bias'].to(dt)
    z = torch.cat((spk, nz), 1).to(dt) @ fc_w.t() + fc_b
    gb = z @ (W / torch.dot(u, W @ v)).t() + b

    def close(got, key):
        w = want[key]
        assert got.shape == w.shape, key
        assert (got - w).abs().max().item() <= 1e-10 * w.abs().max().item(), key

    dxr, dgb = R.cbn_ref(dx, xr, gb, True, sd[p + '.batch_nrom.running_mean'], sd[p + '.batch_nrom.running_var'])
    d_w, d_b, d_fw, d_fb = R.cond_ref(dgb, W, b, u, v, fc_w, fc_b, spk, nz)
    close(d_w, p + '.layer.weight_orig'); close(d_b, p + '.layer.bias')
    close(d_fw, 'fcs.0.weight'); close(d_fb, 'fcs.0.bias')

    vv, gg = sd['ups.0.weight_v'].to(dt), sd['ups.0.weight_g'].to(dt)
    w = O.fold_weight_norm(gg, vv).requires_grad_(True)
    up = F.conv_transpose1d(F.leaky_relu(pre, O.LRELU_SLOPE), w, None, stride=h.upsample_rates[0],
                            padding=(h.upsample_kernel_sizes[0] - h.upsample_rates[0]) // 2)
    dw, = torch.autograd.grad(up, w, dxr)
    dv, dg = R.wn_ref(R.param_to_wf_layout(dw, True), vv, gg, True)
    close(dv, 'ups.0.weight_v'); close(dg, 'ups.0.weight_g')


def test_bounds_are_positive_and_scale_with_the_data():
    """The bound helpers return one finite, non-negative number per compared entry, and scale linearly with the cotangent."""
    r = np.random.default_rng(5)
    B, C, L = 2, 3, 40
    xr, dx = (5.0 + _rand(r, B, C, L)).float(), _rand(r, B, C, L).float()
    gb = torch.cat((1 + 0.2 * _rand(r, B, C), 0.3 * _rand(r, B, C)), dim=1).float()
    rm, rv = torch.zeros(C), torch.ones(C)
    for training in (True, False):
        b1 = R.cbn_bounds(dx, xr, gb, training, rm, rv)
        b2 = R.cbn_bounds(2 * dx, xr, gb, training, rm, rv)
        for a, b, shape in zip((b1.dxr, b1.dgb, b1.terms), (b2.dxr, b2.dgb, b2.terms), ((B, C, L), (B, 2 * C), (B, C, L))):
            assert a.shape == shape and torch.isfinite(a).all() and (a > 0).all()
            assert torch.allclose(b, 2 * a, rtol=1e-12)
    want = torch.tensor([1.0, 2.0, 0.0], dtype=torch.float64)
    assert R.worst_ratio(torch.tensor([1.5, 2.0, 0.0]), want, torch.tensor([1.0, 0.0, 0.0], dtype=torch.float64)) == 0.5
    assert R.worst_ratio(torch.tensor([1.0, 2.5, 0.0]), want, torch.tensor([1.0, 0.0, 0.0], dtype=torch.float64)) == float('inf')
    assert R.worst_ratio(torch.tensor([float('nan'), 2.0, 0.0]), want, torch.ones(3, dtype=torch.float64)) == float('inf')
