"""GPU tests of the summed Winograd launch (hipops.conv1d_wino_sum -> v2w_conv1d_wino_sum_fwd, csrc/v2w_conv_wino.hip): the second convs of a
ResBlock2 stage's branches on one accumulator, against the fp64 statement tests/wino_sum_ref.py.  Bar: tests/test_stage_wino_gpu.py's,
|out - ref| <= 4e-5 * max|ref|.  Shapes: L = 132 at dilation 3 is 66 pairs = 2 tiles of 64, the second with one dead column-wave."""
import numpy as np
import pytest
import torch

from tests import wino_sum_ref

pytestmark = pytest.mark.gpu

SLOPE, DIL = 0.1, 3
SENT = -777.0


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a MI355X'
    from wavthruvec_pytorch_amd import _hip
    _hip.load()
    return torch.device('cuda:0')


def _rand(r, shape, scale=1.0):
    return torch.from_numpy((scale * r.standard_normal(shape)).astype(np.float32))


def _problem(dev, B, C, L, ks, seed):
    from wavthruvec_pytorch_amd import hipops
    rng = np.random.default_rng(seed)
    xs = [_rand(rng, (B, C, L)) for _ in ks]
    wfs = [_rand(rng, (k, C, C), 1 / np.sqrt(C * k)) for k in ks]
    bs = [_rand(rng, (C,)) for _ in ks]
    xd = [x.to(dev) for x in xs]
    wpw = [hipops.pack_wino(w.to(dev)) for w in wfs]
    bd = [b.to(dev) for b in bs]
    return xs, wfs, bs, xd, wpw, bd


def _run(dev, xd, wpw, bd, ks, out_div=3.0, **kw):
    from wavthruvec_pytorch_amd import hipops
    out = torch.full_like(xd[0], SENT)
    assert hipops.conv1d_wino_sum([(x, w, b, k) for x, w, b, k in zip(xd, wpw, bd, ks)], out, dil=DIL, slope=SLOPE, out_div=out_div, **kw)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize('C,L,ks', [(64, 132, (3, 7, 11)), (64, 134, (3, 7, 11)), (128, 132, (3, 7, 11)), (64, 132, (3, 7))],
                         ids=['three_sources', 'scalar_staging_L134', 'two_m_tiles_C128', 'two_sources'])
def test_wino_sum_matches_fp64(dev, C, L, ks):
    xs, wfs, bs, xd, wpw, bd = _problem(dev, 2, C, L, ks, seed=11)
    ref = wino_sum_ref.wino_sum(xs, wfs, bs, dil=DIL, slope=SLOPE, out_div=float(len(ks)))
    got = _run(dev, xd, wpw, bd, ks, out_div=float(len(ks))).cpu().double()
    err, scale = (got - ref).abs().max().item(), ref.abs().max().item()
    print(f'C={C} L={L} ks={ks}: |out-ref|={err:.3e} bar={4e-5 * scale:.3e}')
    assert err <= 4e-5 * scale


def test_one_source_is_bitwise_the_winograd_conv(dev):
    """nsrc == 1 against conv1d_wino_multi on the same problem (res = x): 65 x 2 workgroups, past the 128 below which that call leaves the kernel."""
    from wavthruvec_pytorch_amd import hipops, _hip
    B, C, L, k = 65, 64, 132, 7
    xs, wfs, bs, xd, wpw, bd = _problem(dev, B, C, L, (k,), seed=12)
    got = _run(dev, xd, wpw, bd, (k,), out_div=3.0)
    want = torch.full_like(got, SENT)
    kw = dict(k=k, dil=DIL, slope=SLOPE, res=xd[0], out_div=3.0, algo=hipops.ALGO_AUTO, wp=hipops.pack_mfma(wfs[0].to(dev)), wpw=wpw[0])
    arr = (_hip.Conv1dArgs * 1)()
    hipops._conv1d_args(arr[0], xd[0], None, bd[0], want, **{**{q: v for q, v in kw.items() if q != 'wpw'}, 'algo': hipops.ALGO_WINO, 'wp': wpw[0]})
    assert _hip.kernel_names(_hip.load().v2w_conv1d_fwd_multi, arr, 1)[1] == ['conv_wino_kernel<1, 2, 3, true>']
    hipops.conv1d_wino_multi([(xd[0], None, bd[0], want, kw)])
    torch.cuda.synchronize()
    assert torch.equal(got, want)


def test_full_lengths_are_bitwise_the_plain_launch(dev):
    B, C, L, ks = 3, 64, 132, (3, 7, 11)
    xs, wfs, bs, xd, wpw, bd = _problem(dev, B, C, L, ks, seed=13)
    plain = _run(dev, xd, wpw, bd, ks)
    lens = torch.full((B,), L, dtype=torch.int32, device=dev)
    assert torch.equal(_run(dev, xd, wpw, bd, ks, lengths=lens, len_mul=1), plain)


def test_lengths_kept_outputs_and_poison(dev):
    """len = (L, L - 37, 5): the kept outputs are the fp64 statement's with the inputs past the end counted as zero, whatever they hold (1e30)."""
    B, C, L, ks = 3, 64, 132, (3, 7, 11)
    ends = [L, L - 37, 5]
    xs, wfs, bs, xd, wpw, bd = _problem(dev, B, C, L, ks, seed=14)
    lens = torch.tensor(ends, dtype=torch.int32, device=dev)
    ref = wino_sum_ref.wino_sum(xs, wfs, bs, dil=DIL, slope=SLOPE, out_div=3.0, lengths=ends)
    clean = _run(dev, xd, wpw, bd, ks, lengths=lens, len_mul=1)
    xp = [x.clone() for x in xd]
    for x in xp:
        for b, e in enumerate(ends):
            x[b, :, e:] = 1e30
    poisoned = _run(dev, xp, wpw, bd, ks, lengths=lens, len_mul=1)
    for b, e in enumerate(ends):
        assert torch.equal(clean[b, :, :e], poisoned[b, :, :e]), b
        err, scale = (clean[b, :, :e].cpu().double() - ref[b, :, :e]).abs().max().item(), ref[b, :, :e].abs().max().item()
        print(f'item {b} end {e}: |out-ref|={err:.3e} bar={4e-5 * scale:.3e}')
        assert err <= 4e-5 * scale, b


def test_lengths_leave_what_the_two_launch_winograd_path_leaves(dev):
    """Past an item's end the outputs are unspecified; WHICH of them a launch leaves untouched is the Winograd LEN kernel's rule (tiles and
    column-waves whose first output lies at or past the end store nothing).  Same rule, same set: against the LEN form of the two-launch path
    (k = 7, 11 with their own outputs, then k = 3 adding them) on the Winograd kernel - 66 items, past the 128 workgroups it needs."""
    from wavthruvec_pytorch_amd import hipops
    B, C, L, ks = 66, 64, 132, (3, 7, 11)
    ends = [L, L - 37, 5] * 22
    xs, wfs, bs, xd, wpw, bd = _problem(dev, B, C, L, ks, seed=15)
    lens = torch.tensor(ends, dtype=torch.int32, device=dev)
    got = _run(dev, xd, wpw, bd, ks, lengths=lens, len_mul=1)
    outs = [torch.full_like(got, SENT) for _ in ks]
    kw = [dict(k=k, dil=DIL, slope=SLOPE, res=x, algo=hipops.ALGO_AUTO, wp=hipops.pack_mfma(w.to(dev)), wpw=s, lengths=lens, len_mul=1)
          for k, x, w, s in zip(ks, xd, wfs, wpw)]
    hipops.conv1d_wino_multi([(xd[j], None, bd[j], outs[j], kw[j]) for j in (2, 1)])
    hipops.conv1d_wino_multi([(xd[0], None, bd[0], outs[0], dict(kw[0], add=[outs[1], outs[2]], out_div=3.0))])
    torch.cuda.synchronize()
    assert torch.equal(got == SENT, outs[0] == SENT)
    keep = torch.arange(L, device=dev)[None, None, :] < lens[:, None, None]
    d = torch.where(keep, got - outs[0], torch.zeros_like(got)).abs().max().item()
    scale = torch.where(keep, outs[0], torch.zeros_like(got)).abs().max().item()
    print(f'|sum - two launches| over kept outputs = {d:.3e}, max|out| = {scale:.3e}')
    assert d <= 2 * 4e-5 * scale        # (each within the bar of the exact value)


def test_declines(dev):
    """in_a with nsrc > 1, mixed dilations and an even k: V2W_E_SHAPE, nothing launched (the output keeps its fill)."""
    from wavthruvec_pytorch_amd import hipops, _hip
    B, C, L, ks = 2, 64, 132, (3, 7, 11)
    xs, wfs, bs, xd, wpw, bd = _problem(dev, B, C, L, ks, seed=16)
    out = torch.full_like(xd[0], SENT)
    aff = (torch.ones(B, C, device=dev), torch.zeros(B, C, device=dev))
    src = [(x, w, b, k) for x, w, b, k in zip(xd, wpw, bd, ks)]
    assert hipops.conv1d_wino_sum(src, out, dil=DIL, slope=SLOPE, out_div=3.0, in_affine=aff) is False
    assert hipops.conv1d_wino_sum([(xd[0], wpw[0], bd[0], 3), (xd[1], wpw[1], bd[1], 4)], out, dil=DIL, slope=SLOPE, out_div=3.0) is False
    arr = (_hip.Conv1dArgs * 3)()
    for a, (x, w, b, k), d in zip(arr, src, (3, 3, 1)):
        hipops._conv1d_args(a, x, None, b, out, k=k, dil=d, slope=SLOPE, out_div=3.0, algo=hipops.ALGO_WINO, wp=w)
    assert _hip.load().v2w_conv1d_wino_sum_fwd(arr, 3, None, 1, hipops._stream(out)) == -2
    torch.cuda.synchronize()
    assert bool((out == SENT).all())
