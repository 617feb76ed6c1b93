"""Every entry point of the discriminator path (csrc/v2w_disc.hip, v2w_wgrad_slice / v2w_wgrad_groups) and the conv forms only that path
feeds to v2w_conv1d_fwd, each against the fp64 definition of its own operation (tests/disc_ref.py), per entry.

The cases are the records of tests/disc_cases.py; tests/test_disc_ref_cpu.py asserts which kernel each of them launches.  Movement kernels
and dz must be bit-equal to the definition; sums are held to n * 2^-24 * S per entry (n: the length of the reduction or of the fp32 chain
named with the case, S: the summed magnitudes of the entry's terms, from the reference's data).  Outputs start as NaN, buffers a kernel must
leave partly alone as a sentinel, input pitch tails as a sentinel no output may show.  Each test prints its worst error / bound ratio
(`-s` shows them; DESIGN.md 3e' records them).

Worst ratios on an MI355X when these tests were written: conv forms 0.020 (two-tap), 0.0079 / 0.0053 (halo-48), 0.020 (grouped); wgrad 0.036 at
Lq = 20 and below 0.005 from Lq = 128; dz row sums 0.10; fold1 0.10; cout1_wgrad 0.041 at L = 700, 0.13 at 256 and 0.94 at L = 40 with k = 3,
dilation 19: n = ceil(L / 256) = 1 there and an entry is a sum of six products, so the one rounding of the fp64 total to fp32, which n does
not count, nearly fills the bound by itself.
One-line mutants of v2w_disc.hip these tests fail on: `!(fr[t] > 0.f)` read as `fr[t] < 0.f` (every dz and dz_merge case: the seeded +0 / -0),
`v[S + r]` and `v[2 * S + r]` swapped in phase_split_vec_kernel (its 16 cases), the reflected term `at(m)` dropped from fold1_kernel (the four
cases with a reflect pad)."""
import numpy as np
import pytest
import torch

from tests import disc_cases as K
from tests import disc_ref as R
from wavthruvec_pytorch_amd import hipops

pytestmark = pytest.mark.gpu

NAN, SENT = float('nan'), 777.0


@pytest.fixture(scope='module')
def env():
    assert torch.cuda.is_available(), 'GPU tests need a MI355X'
    from wavthruvec_pytorch_amd import _hip
    dev = torch.device('cuda:0')
    return dev, _hip, _hip.load(), torch.cuda.current_stream(dev).cuda_stream       # (lib, stream: the entry points hipops does not wrap)


def _f32(seed, *shape):
    return torch.from_numpy(np.random.default_rng(seed).standard_normal(shape, dtype=np.float32))


def _nan(dev, *shape):
    return torch.full(shape, NAN, device=dev)


def _report(name, **ratios):
    print(f'[ratio] {name}: ' + '  '.join(f'{k}={v:.3g}' for k, v in ratios.items()))
    for k, v in ratios.items():
        assert v <= 1.0, f'{name}: {k} misses its bound, error / bound = {v:.3g}'


def _cases(cases):
    return pytest.mark.parametrize('c', cases, ids=K.ids(cases))


# ---------------------------------------------------------------------------------------------------------------
# movement kernels: bit-equal
@_cases(K.PHASE_SPLIT)
def test_phase_split(env, c):
    dev, _hip, lib, st = env
    B, Cc, Cg, L, inner, s, off = (c[n] for n in ('B', 'C', 'Cg', 'L', 'inner', 's', 'out_off'))
    Uq, ip, op = K.split_pitches(c)
    x = _f32(1, B, Cc, L, inner)
    xd = R.pitched(x, ip, SENT).to(dev)
    n = B * s * Cc * op
    buf = _nan(dev, off + n + 4)
    hipops.phase_split(xd, L=L, inner=inner, s=s, cg=Cg, out=buf[off:off + n].view(B, s * Cc, op))     # the pitches: those of xd and of the view
    got = buf.cpu()
    assert torch.equal(got[off:off + n].view(B, s * Cc, op), R.pitched(R.phase_split(x, Cg, s), op))
    assert torch.isnan(got[:off]).all() and torch.isnan(got[off + n:]).all()


@_cases(K.PHASE_MERGE)
def test_phase_merge(env, c):
    dev, _hip, lib, st = env
    B, Cc, Cg, L, inner, s, ip, op = (c[n] for n in ('B', 'C', 'Cg', 'L', 'inner', 's', 'ipitch', 'opitch'))
    Uq = R.ceil_div(L, s)
    xs = _f32(2, B, s * Cc, Uq, inner)
    xsd = R.pitched(xs, ip, SENT).to(dev)
    out = torch.full((B, Cc, op), SENT, device=dev)
    _hip.check(lib.v2w_phase_merge(xsd.data_ptr(), out.data_ptr(), B, Cc, Cg, L, inner, s, ip, op, st), 'v2w_phase_merge')
    want = R.phase_merge(xs, Cg, s, L)
    assert torch.equal(out.cpu(), R.pitched(want, op, SENT))            # the pitch tail keeps its sentinel
    # and it inverts v2w_phase_split on the valid part: split(merge(xs)) is xs with the positions past L zeroed
    back = _nan(dev, B, s * Cc, ip)
    hipops.phase_split(out, L=L, inner=inner, s=s, cg=Cg, out=back)
    assert torch.equal(back.cpu(), R.pitched(R.phase_split(want, Cg, s), ip))
    assert torch.equal(R.phase_merge(R.unpitched(back.cpu(), Uq, inner), Cg, s, L), want)


@_cases(K.UNFOLD1)
def test_unfold1(env, c):
    dev, _hip, lib, st = env
    B, T, H, inner, s, k, pad, rows = (c[n] for n in ('B', 'T', 'H', 'inner', 's', 'k', 'pad', 'rows'))
    Uq, P = K.unfold1_geom(c)
    x = _f32(3, B, T)
    xd = x.to(dev)
    out = _nan(dev, B, rows, P)
    hipops.unfold1(xd, H=H, inner=inner, s=s, k=k, pad=pad, rows=rows, out=out)
    got = out.cpu()
    assert torch.equal(got, R.pitched(R.unfold1(x, H, inner, s, k, pad, rows), P))
    assert torch.equal(got[:, k:], torch.zeros(B, rows - k, P))


@_cases(K.FOLD1)
def test_fold1(env, c):
    """Each dx entry sums at most k taps of its own position and k of the position that reflects onto it: 2k terms."""
    dev, _hip, lib, st = env
    B, T, H, inner, s, k, pad, rows = (c[n] for n in ('B', 'T', 'H', 'inner', 's', 'k', 'pad', 'rows'))
    Uq, P = K.unfold1_geom(c)
    dxu = _f32(4, B, rows, Uq, inner)                                   # rows k .. 15 are not the kernel's to read
    dxud = R.pitched(dxu, P, SENT).to(dev)
    dx = _nan(dev, B, T)
    hipops.fold1(dxud, T=T, H=H, inner=inner, s=s, k=k, pad=pad, out=dx)
    want, S = R.fold1(dxu, T, H, inner, s, k, pad)
    _report('fold1 ' + c['id'], dx=R.worst_ratio(dx.cpu(), want, R.sum_bound(2 * k, S)))
    if H * inner > T:                                                   # the samples the pad reflects carry more than their own taps
        _, S0 = R.fold1(dxu, H * inner, H, inner, s, k, pad)
        assert (S[:, :T] - S0[:, :T]).abs().max().item() > 0


@_cases(K.UNFOLD_TAPS)
def test_unfold_taps(env, c):
    dev, _hip, lib, st = env
    B, Cc, L, inner, s, k, pad, ip, op = (c[n] for n in ('B', 'C', 'L', 'inner', 's', 'k', 'pad', 'ipitch', 'opitch'))
    x = _f32(5, B, Cc, L, inner)
    xd = R.pitched(x, ip, SENT).to(dev)
    out = _nan(dev, B, k * Cc, op)
    hipops.unfold_taps(xd, L=L, inner=inner, s=s, k=k, pad=pad, out=out)
    assert torch.equal(out.cpu(), R.pitched(R.unfold_taps(x, s, k, pad), op))


@_cases(K.ZERO_TAIL)
def test_zero_tail(env, c):
    dev, _hip, lib, st = env
    rows, pitch, valid = c['rows'], c['pitch'], c['valid']
    x = _f32(6, rows + 1, pitch)                                        # one row more than the call owns
    xd = x.to(dev)
    hipops.zero_tail(xd[:rows], valid=valid)
    want = torch.cat((R.zero_tail(x[:rows], valid), x[rows:]))
    assert torch.equal(xd.cpu(), want)


@_cases(K.AVGPOOL)
def test_avgpool4_and_backward(env, c):
    dev, _hip, lib, st = env
    B, L = c['B'], c['L']
    Lo = L // 2 + 1
    x, g = _f32(7, B, L), _f32(8, B, Lo)
    xd, gd = x.to(dev), g.to(dev)
    out, dx = _nan(dev, B, Lo), _nan(dev, B, L)
    hipops.avgpool4(xd, out=out)
    hipops.avgpool4_bwd(gd, L=L, out=dx)
    want, _ = R.avgpool4(x)
    wdx, _ = R.avgpool4_bwd(g, L)
    e, eb = (out.cpu().double() - want).abs().max().item(), (dx.cpu().double() - wdx).abs().max().item()
    print(f'[err] avgpool4 L={L}: fwd {e:.3g} bwd {eb:.3g}')
    assert e <= 1e-6 and eb <= 1e-6                                      # (NaN fails both)


# ---------------------------------------------------------------------------------------------------------------
# dz, its row sums, their batch reduce
def _seed_f(f):
    """Exact +0, -0 and denormals of either sign where the rule !(f > 0) -> slope decides."""
    flat = f.view(-1)
    vals = torch.tensor([0.0, -0.0, 1e-40, -1e-40], dtype=torch.float32)
    n = min(4, flat.numel())
    flat[:n] = vals[:n]
    return f


def _check_dz(env, name, c, rows, pitch, valid, f, g, d_buf, d_valid, call):
    dev, _hip, lib, st = env
    dz = _nan(dev, rows, pitch)
    rs = _nan(dev, rows + 4) if c.get('rowsum', True) else None
    call(dz, rs)
    got = dz.cpu()
    want = R.dz_f32(f[:, :valid].numpy(), None if g is None else g.numpy(), None if d_valid is None else d_valid.numpy(), c['slope'])
    assert torch.equal(got[:, :valid], torch.from_numpy(want)), name
    assert torch.equal(got[:, valid:], torch.zeros(rows, pitch - valid)), name          # the pitch tail is exactly 0
    if rs is not None:
        tot, S = R.rowsum(torch.from_numpy(want))
        r = rs.cpu()
        assert torch.isnan(r[rows:]).all()                                               # the row < rows guard
        _report(name, rowsum=R.worst_ratio(r[:rows], tot, R.sum_bound(c['chain'], S)))
    return got


@_cases(K.DZ)
def test_disc_dz(env, c):
    dev, _hip, lib, st = env
    rows, pitch, valid, ops = c['rows'], c['pitch'], c['valid'], c['ops']
    f = _seed_f(_f32(9, rows, pitch))
    g = _f32(10, rows, valid) if 'g' in ops else None
    d = R.pitched(_f32(11, rows, valid), pitch, SENT) if 'd' in ops else None
    fd, gd, dd = f.to(dev), None if g is None else g.to(dev), None if d is None else d.to(dev)

    def call(dz, rs):
        hipops.disc_dz(fd, gd, dd, valid=valid, slope=c['slope'], out=dz, rowsum=rs)

    _check_dz(env, 'dz ' + c['id'], c, rows, pitch, valid, f, g, d, None if d is None else d[:, :valid], call)


@_cases(K.DZ_MERGE)
def test_disc_dz_merge(env, c):
    dev, _hip, lib, st = env
    B, Cc, Cg, L, inner, s, pitch, dpitch = (c[n] for n in ('B', 'C', 'Cg', 'L', 'inner', 's', 'pitch', 'dpitch'))
    rows, valid, Uq = B * Cc, L * inner, R.ceil_div(L, s)
    f = _seed_f(_f32(12, rows, pitch))
    g = _f32(13, rows, valid) if c['g'] else None
    dxs = _f32(14, B, s * Cc, Uq, inner)
    dxsd = R.pitched(dxs, dpitch, SENT).to(dev)
    fd, gd = f.to(dev), None if g is None else g.to(dev)
    d_valid = R.dz_merge_d(dxs, Cg, s, L).reshape(rows, valid)

    def call(dz, rs):
        hipops.disc_dz_merge(fd, gd, dxsd, cg=Cg, L=L, inner=inner, s=s, slope=c['slope'], out=dz, rowsum=rs)

    _check_dz(env, 'dz_merge ' + c['id'], c, rows, pitch, valid, f, g, None, d_valid, call)


@_cases(K.ROWSUM_REDUCE)
def test_rowsum_reduce(env, c):
    dev, _hip, lib, st = env
    B, Cc = c['B'], c['C']
    rs = _f32(15, B, Cc) * 100
    rsd = rs.to(dev)
    db = _nan(dev, Cc + 4)
    hipops.rowsum_reduce(rsd, out=db[:Cc])
    got = db.cpu()
    assert torch.equal(got[:Cc], torch.from_numpy(R.rowsum_reduce_f32(rs.numpy()))) and torch.isnan(got[Cc:]).all()


@_cases(K.COUT1)
def test_cout1_wgrad(env, c):
    dev, _hip, lib, st = env
    B, Cc, L, k, dil, tap0 = (c[n] for n in ('B', 'C', 'L', 'k', 'dil', 'tap0'))
    x, dz = _f32(16, B, Cc, L), _f32(17, B, 1, L)
    xd, dzd = x.to(dev), dz.to(dev)
    dwf = _nan(dev, k, Cc, 1)
    hipops.cout1_wgrad(xd, dzd, k=k, dil=dil, tap0=tap0, out=dwf)
    _, _, want, S = R.conv_grads(x, torch.zeros(k, Cc, 1), dz, dil, tap0)
    _report('cout1_wgrad ' + c['id'], dwf=R.worst_ratio(dwf.cpu(), want, R.sum_bound(c['chain'], S)))


# ---------------------------------------------------------------------------------------------------------------
# conv forms: forward and input gradient on the f32 MFMA tile kernel, the split-f16 kernel against it
def _conv_data(c, seed):
    B, G, cig, cog, L, k = (c[n] for n in ('B', 'G', 'cig', 'cog', 'L', 'k'))
    x = _f32(seed, B, G * cig, L)
    w4 = _f32(seed + 1, G, k, cig, cog) / float(np.sqrt(cig * k))          # [G][k][cig][cog]
    if c.get('zero_last_tap'):
        w4[:, -1] = 0
    return x, w4, _f32(seed + 2, G * cog), _f32(seed + 3, B, G * cog, L)


def _run_conv(x, w4, bias, out, c, tap0, out_slope, algo, packs):
    """The launches discriminators.py makes for a conv (hipops.conv1d_groups); x (B, G*ci, L), w4 [G][k][ci][co] on the GPU."""
    hipops.conv1d_groups(x, w4, bias, out, packs, dil=c['dil'], pad_left=tap0 * c['dil'], out_slope=out_slope, algo=algo)
    torch.cuda.synchronize()
    return out


def _ref_device(c, dev):
    """The fp64 reference of the one case of 64 x 256 x 1064 runs as torch's fp64 matrix products on the GPU (22 G multiply-adds)."""
    return dev if c['B'] * c['G'] * c['cig'] * c['cog'] * c['L'] * c['k'] > 1 << 32 else torch.device('cpu')


@_cases(K.CONV)
def test_conv_forms_f32_mfma(env, c):
    dev = env[0]
    B, G, cig, cog, L, k, dil, tap0 = (c[n] for n in ('B', 'G', 'cig', 'cog', 'L', 'k', 'dil', 'tap0'))
    x, w4, bias, dy = _conv_data(c, 20)
    xd, w4d, bd, dyd = x.to(dev), w4.to(dev), bias.to(dev), dy.to(dev)
    out = _run_conv(xd, w4d, bd, _nan(dev, B, G * cog, L), c, tap0, c['out_slope'], hipops.ALGO_MFMA, hipops.pack_mfma_batch(w4d))
    wT4d = w4d.flip(1).transpose(2, 3).contiguous()                       # [G][k][cog][cig], taps reversed
    dx = _run_conv(dyd, wT4d, None, _nan(dev, B, G * cig, L), c, k - 1 - tap0, 0.0, hipops.ALGO_MFMA, hipops.pack_mfma_batch(wT4d))
    rd = _ref_device(c, dev)
    want, S = R.conv_groups(x.to(rd), w4.to(rd), bias.to(rd), dil, tap0, c['out_slope'])
    r_out = R.worst_ratio(out.to(rd), want, R.sum_bound(k * cig, S))
    r_dx = 0.0
    for g in range(G):
        wdx, Sx, _, _ = R.conv_grads(x[:, g * cig:(g + 1) * cig].to(rd), w4[g].to(rd), dy[:, g * cog:(g + 1) * cog].to(rd), dil, tap0)
        r_dx = max(r_dx, R.worst_ratio(dx[:, g * cig:(g + 1) * cig].to(rd), wdx, R.sum_bound(k * cog, Sx)))
    _report('conv ' + c['id'], out=r_out, dx=r_dx)


@_cases(K.SPLIT)
def test_conv_forms_split_f16(env, c):
    """The project's bar for the split-f16 products (test_conv1d_split_f16): no worse than twice the f32 kernel's error plus 1e-6, both
    against fp64.  A shape the split kernel has no tile for is declined with V2W_E_SHAPE."""
    dev, _hip = env[0], env[1]
    B, G, cig, cog, L, k, dil, tap0 = (c[n] for n in ('B', 'G', 'cig', 'cog', 'L', 'k', 'dil', 'tap0'))
    x, w4, bias, dy = _conv_data(c, 30)
    xd, w4d, bd, dyd = x.to(dev), w4.to(dev), bias.to(dev), dy.to(dev)

    def both(xin, w, b, co, t0, slope):
        o_f32 = _run_conv(xin, w, b, _nan(dev, B, G * co, L), c, t0, slope, hipops.ALGO_MFMA, hipops.pack_mfma_batch(w))
        o_split = _run_conv(xin, w, b, _nan(dev, B, G * co, L), c, t0, slope, hipops.ALGO_SPLIT, [hipops.pack_split(w[g].contiguous()) for g in range(G)])
        return o_f32.cpu().double(), o_split.cpu().double()

    want, _ = R.conv_groups(x, w4, bias, dil, tap0, c['out_slope'])
    o_f32, o_split = both(xd, w4d, bd, cog, tap0, c['out_slope'])
    e_f32, e_split = (o_f32 - want).abs().max().item(), (o_split - want).abs().max().item()
    print(f'[err] split {c["id"]}: forward split {e_split:.3g} f32 {e_f32:.3g}')
    assert e_split <= 2 * e_f32 + 1e-6
    wT4d = w4d.flip(1).transpose(2, 3).contiguous()
    if c['dgrad_rc'] != K.OK:
        with pytest.raises(_hip.HipLibraryError) as ei:
            _run_conv(dyd, wT4d, None, _nan(dev, B, G * cig, L), c, k - 1 - tap0, 0.0, hipops.ALGO_SPLIT,
                      [(torch.empty(8, device=dev, dtype=torch.float16), torch.empty(4, device=dev))] * G)
        assert ei.value.code == c['dgrad_rc']
        return
    wdx = torch.cat([R.conv_grads(x[:, g * cig:(g + 1) * cig], w4[g], dy[:, g * cog:(g + 1) * cog], dil, tap0)[0] for g in range(G)], 1)
    d_f32, d_split = both(dyd, wT4d, None, cig, k - 1 - tap0, 0.0)
    e_f32, e_split = (d_f32 - wdx).abs().max().item(), (d_split - wdx).abs().max().item()
    print(f'[err] split {c["id"]}: dgrad split {e_split:.3g} f32 {e_f32:.3g}')
    assert e_split <= 2 * e_f32 + 1e-6


# ---------------------------------------------------------------------------------------------------------------
# weight gradients: n = B * Lq terms per entry
@_cases(K.WGRAD)
def test_wgrad_slice(env, c):
    dev, _hip, lib, st = env
    B, ci, co, Lq, k, dil, tap0 = (c[n] for n in ('B', 'c_in', 'c_out', 'Lq', 'k', 'dil', 'tap0'))
    x_ct, dy_ct, grp = c.get('x_ct', 0), c.get('dy_ct', 0), c.get('grp', 0)
    x, dy = _f32(40, B, x_ct or ci, Lq), _f32(41, B, dy_ct or co, Lq)
    xd, dyd = x.to(dev), dy.to(dev)
    ns = lib.v2w_wgrad_slabs(B, ci, co, Lq)
    assert ns > 0
    got = []
    for _ in range(2):
        slab, dwf = _nan(dev, ns * k * ci * co), _nan(dev, k, ci, co)
        _hip.check(lib.v2w_wgrad_slice(xd.data_ptr() + 4 * grp * ci * Lq, dyd.data_ptr() + 4 * grp * co * Lq, dwf.data_ptr(), slab.data_ptr(),
                                       B, ci, co, Lq, k, dil, tap0, x_ct, dy_ct, st), 'v2w_wgrad_slice')
        got.append(dwf.cpu())
    assert torch.equal(got[0], got[1])                                   # deterministic
    _, _, want, S = R.conv_grads(x[:, grp * ci:(grp + 1) * ci], torch.zeros(k, ci, co), dy[:, grp * co:(grp + 1) * co], dil, tap0)
    _report('wgrad_slice ' + c['id'], dwf=R.worst_ratio(got[0], want, R.sum_bound(B * Lq, S)))


@_cases(K.WGRAD_GROUPS)
def test_wgrad_groups(env, c):
    dev, _hip, lib, st = env
    B, ci, co, Lq, k, dil, tap0, G = (c[n] for n in ('B', 'c_in', 'c_out', 'Lq', 'k', 'dil', 'tap0', 'G'))
    x, dy = _f32(42, B, G * ci, Lq), _f32(43, B, G * co, Lq)
    xd, dyd = x.to(dev), dy.to(dev)
    ns = lib.v2w_wgrad_group_slabs(B, ci, co, Lq, G)
    assert 0 < ns <= lib.v2w_wgrad_slabs(B, ci, co, Lq)
    got = []
    for _ in range(2):
        slab, dw = _nan(dev, G * ns * k * ci * co), _nan(dev, G, k, ci, co)
        hipops.wgrad_groups(xd, dyd, groups=G, k=k, dil=dil, tap0=tap0, out=dw, slab=slab)
        got.append(dw.cpu())
    assert torch.equal(got[0], got[1])
    ratios = {}
    for g in range(G):
        _, _, want, S = R.conv_grads(x[:, g * ci:(g + 1) * ci], torch.zeros(k, ci, co), dy[:, g * co:(g + 1) * co], dil, tap0)
        ratios['group%d' % g] = R.worst_ratio(got[0][g], want, R.sum_bound(B * Lq, S))
    _report('wgrad_groups ' + c['id'], **ratios)
