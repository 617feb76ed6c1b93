"""tests/disc_ref.py pinned against independent statements of the same operations (torch's strided / 2-d convolutions, avg_pool1d, reflect
pad + unfold, autograd, the discriminator oracle), the dispatch table of the discriminator kernel tests (tests/disc_cases.py through the name
sink: which kernel every GPU case launches), and the exhaustive check of phase_split_rows_kernel's fp32 division.  No GPU needed."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import disc_cases as K
from tests import disc_ref as R
from wavthruvec_pytorch_amd import _hip


def _rnd(seed, *shape):
    return torch.from_numpy(np.random.default_rng(seed).standard_normal(shape))


def _close(a, b, tol=1e-12):
    assert a.shape == b.shape, (a.shape, b.shape)
    assert (a - b).abs().max().item() <= tol * max(1.0, b.abs().max().item())


def _stacked_weights(w, s, P, Cg):
    """(C_out, C_in, k) of a stride-s conv with padding P -> wf' [kp][s*C_in][C_out] and Q for the stride-1 conv over the stacked phases:
    tap j = s*q + r + P of channel c sits at tap q + Q of stacked channel (c // Cg)*s*Cg + r*Cg + c % Cg."""
    co, ci, k = w.shape
    Q = -(-P // s)
    kp = Q + (k - 1 - P) // s + 1
    wf = torch.zeros(kp, s * ci, co, dtype=w.dtype)
    for j in range(k):
        q, r = divmod(j - P, s)
        for c in range(ci):
            wf[q + Q, (c // Cg) * s * Cg + r * Cg + c % Cg] = w[:, c, j]
    return wf, Q


@pytest.mark.parametrize('L', [20, 21, 22])
def test_phase_split_then_stride1_conv_is_the_strided_conv(L):
    B, C, co, k, s, P = 2, 3, 4, 5, 3, 2
    x, w, b = _rnd(1, B, C, L), _rnd(2, co, C, k), _rnd(3, co)
    want = F.conv1d(x, w, b, stride=s, padding=P)
    wf, Q = _stacked_weights(w, s, P, C)
    xs = R.phase_split(x.unsqueeze(-1), C, s)
    got, S = R.conv(xs.squeeze(-1), wf, b, 1, Q)
    assert wf.shape[0] == 2 and Q == 1
    _close(got[:, :, :want.shape[2]], want)
    assert (S >= got.abs() - 1e-12).all()
    _close(R.phase_merge(xs, C, s, L), x.unsqueeze(-1), 0.0)


@pytest.mark.parametrize('p', [13, 19])
def test_period_forms_are_the_conv2d_with_a_k_by_1_kernel(p):
    """Stride (3, 1): phase split with inner = p, then a two-tap conv of dilation p.  Stride 1: a five-tap conv of dilation p, pad_left 2 p."""
    B, C, co, H, k, P = 2, 4, 6, 11, 5, 2
    x, w, b = _rnd(4, B, C, H, p), _rnd(5, co, C, k, 1), _rnd(6, co)
    want = F.conv2d(x, w, b, stride=(1, 1), padding=(P, 0))
    got, _ = R.conv(x.reshape(B, C, H * p), w[..., 0].permute(2, 1, 0), b, p, P)
    _close(got.reshape(B, co, H, p), want)
    want3 = F.conv2d(x, w, b, stride=(3, 1), padding=(P, 0))
    wf, Q = _stacked_weights(w[..., 0], 3, P, 2)                      # two groups of two channels: the stacking is per group
    xs = R.phase_split(x, 2, 3)
    got3, _ = R.conv(xs.reshape(B, 3 * C, -1), wf, b, p, Q)
    _close(got3.reshape(B, co, -1, p)[:, :, :want3.shape[2]], want3)
    lr = R.conv(x.reshape(B, C, H * p), w[..., 0].permute(2, 1, 0), b, p, P, out_slope=0.1)[0]
    _close(lr.reshape(B, co, H, p), F.leaky_relu(want, float(np.float32(0.1))))


def test_grouped_conv_and_its_gradients_are_torch_autograd():
    B, G, cig, cog, L, k, dil, tap0 = 2, 3, 4, 5, 17, 4, 2, 1
    x = _rnd(7, B, G * cig, L).requires_grad_(True)
    w = _rnd(8, G * cog, cig, k).requires_grad_(True)
    b, dy = _rnd(9, G * cog), _rnd(10, B, G * cog, L)
    y = F.conv1d(F.pad(x, (tap0 * dil, (k - 1 - tap0) * dil)), w, b, dilation=dil, groups=G)
    y.backward(dy)
    wf4 = w.detach().view(G, cog, cig, k).permute(0, 3, 2, 1)
    got, _ = R.conv_groups(x.detach(), wf4, b, dil, tap0)
    _close(got, y.detach())
    for g in range(G):
        xg, dyg = x.detach()[:, g * cig:(g + 1) * cig], dy[:, g * cog:(g + 1) * cog]
        dx, Sx, dwf, Sw = R.conv_grads(xg, wf4[g], dyg, dil, tap0)
        _close(dx, x.grad[:, g * cig:(g + 1) * cig])
        _close(dwf, w.grad.view(G, cog, cig, k)[g].permute(2, 1, 0))
        assert (Sx >= dx.abs() - 1e-12).all() and (Sw >= dwf.abs() - 1e-12).all()
        # the input gradient is the forward conv of dy with the transposed, tap-flipped weights at tap0' = k - 1 - tap0
        _close(R.conv(dyg, R.transpose_flip(wf4[g]), None, dil, k - 1 - tap0)[0], dx)


@pytest.mark.parametrize('L', [1, 2, 3, 10, 11])
def test_avgpool4_is_avg_pool1d(L):
    x = _rnd(11, 3, 1, L).requires_grad_(True)
    want = F.avg_pool1d(x, 4, 2, padding=2)
    g = _rnd(12, *want.shape)
    want.backward(g)
    got, S = R.avgpool4(x.detach()[:, 0])
    _close(got, want.detach()[:, 0])
    dx, Sd = R.avgpool4_bwd(g[:, 0], L)
    _close(dx, x.grad[:, 0])
    assert (S >= got.abs() - 1e-12).all() and (Sd >= dx.abs() - 1e-12).all()


def _unfold1_torch(x, H, inner, s, k, pad):
    B, T = x.shape
    xp = F.pad(x.unsqueeze(1), (0, H * inner - T), 'reflect').squeeze(1) if H * inner > T else x
    x2 = F.pad(xp.view(B, 1, H, inner), (0, 0, pad, pad))
    return F.unfold(x2, kernel_size=(k, 1), stride=(s, 1))            # (B, k, U * inner)


@pytest.mark.parametrize('c', K.UNFOLD1, ids=K.ids(K.UNFOLD1))
def test_unfold1_and_fold1_are_reflect_pad_and_unfold(c):
    B, T, H, inner, s, k, pad, rows = (c[n] for n in ('B', 'T', 'H', 'inner', 's', 'k', 'pad', 'rows'))
    x = _rnd(13, B, T).requires_grad_(True)
    want = _unfold1_torch(x, H, inner, s, k, pad)
    got = R.unfold1(x.detach(), H, inner, s, k, pad, rows)
    Uq = K.unfold1_geom(c)[0]
    assert got.shape == (B, rows, Uq, inner)
    _close(got[:, :k].reshape(B, k, -1), want.detach(), 0.0)
    assert got[:, k:].abs().max().item() == 0.0
    dxu = _rnd(14, B, rows, Uq, inner)
    want.backward(dxu[:, :k].reshape(B, k, -1))
    dx, S = R.fold1(dxu, T, H, inner, s, k, pad)
    _close(dx, x.grad)
    assert (S >= dx.abs() - 1e-12).all()


@pytest.mark.parametrize('c', K.UNFOLD_TAPS, ids=K.ids(K.UNFOLD_TAPS))
def test_unfold_taps_is_unfold(c):
    B, Cc, L, inner, s, k, pad = (c[n] for n in ('B', 'C', 'L', 'inner', 's', 'k', 'pad'))
    x = _rnd(15, B, Cc, L, inner)
    un = F.unfold(F.pad(x, (0, 0, pad, pad)), kernel_size=(k, 1), stride=(s, 1))      # (B, C * k, U * inner), channel c * k + j
    want = un.view(B, Cc, k, -1, inner).transpose(1, 2).reshape(B, k * Cc, -1, inner)
    got = R.unfold_taps(x, s, k, pad)
    _close(got, want, 0.0)
    assert got.shape[2] == 3 and s * (got.shape[2] - 1) + k - 1 - pad >= L           # the last row reads past L


def test_dz_is_the_leaky_relu_backward_and_its_fp32_form():
    z, g, d = _rnd(16, 5, 40), _rnd(17, 5, 40), _rnd(18, 5, 40)
    z[0, :3] = torch.tensor([0.0, -0.0, 1e-300])
    zz = z.clone().requires_grad_(True)
    f = F.leaky_relu(zz, float(np.float32(0.1)))
    f.backward(g + d)
    _close(R.dz(f.detach(), g, d, 0.1), zz.grad)
    _close(R.dz(f.detach(), None, d, 0.1), zz.grad - R.dz(f.detach(), g, None, 0.1))
    _close(R.dz(f.detach(), g, d, 1.0), g + d)
    f32, g32, d32 = (t.detach().float().numpy() for t in (f, g, d))
    for gg, dd in ((g32, d32), (g32, None), (None, d32), (None, None)):
        for slope in (0.1, 1.0):
            want = R.dz(f32, gg, dd, slope)
            got = torch.from_numpy(R.dz_f32(f32, gg, dd, slope)).double()
            assert ((got - want).abs() <= 2 * R.U * want.abs()).all()
    # the rule is !(f > 0) -> slope: +0, -0 take the slope
    assert R.dz_f32(np.float32([0.0, -0.0, 1e-45, -1e-45]), np.float32([1, 1, 1, 1]), None, 0.5).tolist() == [0.5, 0.5, 1.0, 0.5]


def test_rowsum_reduce_is_the_sum_over_the_batch():
    rs = np.random.default_rng(19).standard_normal((33, 65)).astype(np.float32)
    got = R.rowsum_reduce_f32(rs)
    assert got.dtype == np.float32 and np.abs(got - rs.astype(np.float64).sum(0)).max() <= 2 * R.U * np.abs(rs).sum(0).max()
    tot, S = R.rowsum(torch.from_numpy(rs))
    assert tot.shape == (33,) and (S >= tot.abs()).all()


def test_chain_through_the_oracles_first_two_mpd_layers():
    """unfold1 -> one-tap conv over the 16 rows -> leaky_relu is DiscriminatorP's first layer, phase split -> two-tap conv of dilation p ->
    leaky_relu its second, on the oracle's own weights.  (disc_ref applies the slope the kernels get, float32(0.1); the oracle the double 0.1:
    1.5e-9 apart, relative, per layer - hence 1e-7.)"""
    from oracle import disc_oracle as D
    from wavthruvec_pytorch_amd import synthetic
    p, B, T = 13, 2, 13 * 40 - 5
    sd = {n: t.double() for n, t in synthetic.make_disc_state_dict(synthetic.mpd_state_dict_spec([p]), seed=3).items()}
    x = _rnd(20, B, 1, T)
    _, fmap = D.disc_p(x, sd, 'discriminators.0', p)
    H = -(-T // p)
    w0, b0 = D.wn_weight(sd, 'discriminators.0.convs.0')[..., 0], sd['discriminators.0.convs.0.bias']      # (32, 1, 5)
    xu = R.unfold1(x[:, 0], H, p, 3, 5, 2, 16)
    wf0 = torch.zeros(1, 16, 32, dtype=torch.float64)
    wf0[0, :5] = w0[:, 0, :].t()
    f0, _ = R.conv(xu.reshape(B, 16, -1), wf0, b0, 1, 0, out_slope=0.1)
    U0 = xu.shape[2]
    _close(f0.reshape(B, 32, U0, p), fmap[0], 1e-7)
    w1, b1 = D.wn_weight(sd, 'discriminators.0.convs.1')[..., 0], sd['discriminators.0.convs.1.bias']      # (128, 32, 5)
    wf1, Q = _stacked_weights(w1, 3, 2, 32)
    xs = R.phase_split(f0.reshape(B, 32, U0, p), 32, 3)
    f1, _ = R.conv(xs.reshape(B, 96, -1), wf1, b1, p, Q, out_slope=0.1)
    _close(f1.reshape(B, 128, -1, p)[:, :, :fmap[1].shape[2]], fmap[1], 1e-7)
    # the same second layer through unfold_taps: one tap over 5 * 32 channels
    xt = R.unfold_taps(f0.reshape(B, 32, U0, p), 3, 5, 2)
    wt = w1.permute(2, 1, 0).reshape(1, 5 * 32, 128)
    _close(R.conv(xt.reshape(B, 160, -1), wt, b1, 1, 0, out_slope=0.1)[0].reshape(B, 128, -1, p), fmap[1], 1e-7)


# ---------------------------------------------------------------------------------------------------------------
# the dispatch table: one row per GPU case
ROWS = [(e, c) for e, cases in K.TABLE.items() for c in cases]


@pytest.mark.parametrize('entry,c', ROWS, ids=['%s-%s' % (e, c['id']) for e, c in ROWS])
def test_dispatch_of_every_gpu_case(entry, c):
    rc, names = K.dispatch(entry, c)
    print(entry, c['id'], rc, names)
    assert (rc, names) == (c['rc'], c['kernels']), (rc, names)


@pytest.mark.parametrize('c', K.CONV, ids=K.ids(K.CONV))
def test_dispatch_of_the_conv_forms(c):
    fwd, dgrad = K.dispatch_conv(c), K.dispatch_conv(c, dgrad=True)
    print(c['id'], fwd, dgrad)
    assert fwd == (K.OK, c['kernels']) and dgrad == (K.OK, c['dgrad']), (fwd, dgrad)


@pytest.mark.parametrize('c', K.SPLIT, ids=K.ids(K.SPLIT))
def test_dispatch_of_the_split_f16_forms(c):
    fwd, dgrad = K.dispatch_conv(c, algo=_hip.ALGO_SPLIT), K.dispatch_conv(c, dgrad=True, algo=_hip.ALGO_SPLIT)
    print(c['id'], fwd, dgrad)
    assert fwd == (K.OK, c['kernels']) and dgrad == (c['dgrad_rc'], c['dgrad']), (fwd, dgrad)


def test_the_table_reaches_every_branch():
    seen = {n for cases in K.TABLE.values() for c in cases for n in c['kernels']}
    seen |= {n for c in K.CONV for n in c['kernels'] + c['dgrad']}
    need = ['phase_split_vec_kernel<2>', 'phase_split_vec_kernel<4>', 'phase_split_vec_kernel<5>', 'phase_split_vec_kernel<8>',
            'phase_split_rows_kernel', 'phase_split_kernel', 'disc_dz_rows_kernel<false>', 'disc_dz_rows_kernel<true>',
            'wgrad_pipe_kernel<16, 1, 1, 1, 1, false>', 'wgrad_pipe_kernel<32, 1, 1, 2, 1, false>', 'wgrad_pipe_kernel<32, 2, 2, 5, 1, true>',
            'wgrad_pipe_kernel<32, 2, 2, 5, 1, false>', 'wgrad_kernel<32>',
            'conv_tile_kernel<32, 1, 2, 2, 2, 2, 32, 4, 4, 2, true>', 'conv_tile_kernel<32, 1, 1, 2, 2, 2, 32, 4, 4, 2, true>',
            'conv_tile_kernel<32, 1, 2, 2, 2, 2, 32, 4, 4, 0, true>', 'conv_tile_kernel<32, 1, 1, 2, 2, 2, 32, 4, 4, 0, true>']
    assert [n for n in need if n not in seen] == []
    # both layouts of the dz kernel (a wave per row up to a pitch of 256, a block per row past it), in both forms
    for cases in (K.DZ, K.DZ_MERGE):
        assert {c['pitch'] > 256 for c in cases} == {True, False}
    # the launcher's own conditions, for what the names cannot show: gridDim.y of the rows kernel, the grid-stride loop of zero_tail
    assert all((K.split_pitches(c)[2] // 4 + 255) // 256 >= 2 for c in K.PHASE_SPLIT if c['id'].startswith('rows_inner'))
    assert any(c['rows'] * (c['pitch'] - c['valid']) > 1024 * 256 for c in K.ZERO_TAIL)
    assert max(K.split_pitches(c)[2] for c in K.PHASE_SPLIT) == (1 << 22) - 4


# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('inner', [1, 2, 3, 5, 7, 11, 13, 17, 19])
def test_rows_kernel_division_is_exact_below_2p22(inner):
    """phase_split_rows_kernel divides by `inner` with an fp32 reciprocal and one correction step; the launcher uses it for opitch < 2^22.
    Every rem below that, in the same float32 arithmetic."""
    rem = np.arange(1 << 22, dtype=np.int64)
    got = R.rows_kernel_quotient(rem, inner)
    bad = np.nonzero(got != rem // inner)[0]
    assert bad.size == 0, (inner, bad[:5], got[bad[:5]])
