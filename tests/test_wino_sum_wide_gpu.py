"""GPU tests of the summed Winograd launch at the channel counts of stages 0 and 1 (C = 256 / 128, dilation 3; hipops.conv1d_wino_sum ->
v2w_conv1d_wino_sum_fwd[_order], csrc/v2w_conv_wino.hip): every tile-geometry case against the fp64 statement tests/wino_sum_ref.py, the walk
orders, and one generator forward with the shipped `Generator.wino_sum` / `wino_sum_wide`.  Bar: tests/test_wino_sum_gpu.py's, |out - ref| <= 4e-5 * max|ref|.
Lengths at dilation 3 (tiles of 64 output pairs): L = 70 is 36 pairs - one partial tile; L = 384 is 192 pairs - three full tiles, no tail;
L = 386 is 195 pairs - a fourth tile with ONE live pair (and scalar staging: L % 4 != 0); L = 200 with per-item lengths - the `_len_` kernel."""
import numpy as np
import pytest
import torch

from oracle import vec2wav_oracle as O
from tests import wino_sum_ref

pytestmark = pytest.mark.gpu

SLOPE, DIL, B = 0.1, 3, 2
SENT = -777.0
BAR = 4e-5
ORDERS = [(0, 1, 2), (1, 2, 0), (2, 1, 0)]
ENDS = [200, 37]


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a MI355X'
    from wavthruvec_pytorch_amd import _hip
    _hip.load()
    return torch.device('cuda:0')


def _rand(r, shape, scale=1.0):
    return torch.from_numpy((scale * r.standard_normal(shape)).astype(np.float32))


_cache = {}


def _problem(dev, C, L, ks, nb=B, lengths=None):
    """Operands on the host and on the device and the fp64 reference: computed once per shape, shared, never written."""
    key = (C, L, ks, nb, None if lengths is None else tuple(lengths))
    if key not in _cache:
        from wavthruvec_pytorch_amd import hipops
        rng = np.random.default_rng(1000 * C + L + len(ks))
        xs = [_rand(rng, (nb, C, L)) for _ in ks]
        wfs = [_rand(rng, (k, C, C), 1 / np.sqrt(C * k)) for k in ks]
        bs = [_rand(rng, (C,)) for _ in ks]
        ref = wino_sum_ref.wino_sum(xs, wfs, bs, dil=DIL, slope=SLOPE, out_div=float(len(ks)), lengths=lengths)
        _cache[key] = ([x.to(dev) for x in xs], [hipops.pack_wino(w.to(dev)) for w in wfs], [b.to(dev) for b in bs], ref)
    return _cache[key]


def _run(xd, wpw, bd, ks, **kw):
    from wavthruvec_pytorch_amd import hipops
    out = torch.full_like(xd[0], SENT)
    assert hipops.conv1d_wino_sum([(x, w, b, k) for x, w, b, k in zip(xd, wpw, bd, ks)], out, dil=DIL, slope=SLOPE, out_div=float(len(ks)), **kw)
    torch.cuda.synchronize()
    return out


def _check(got, ref, what):
    err, scale = (got.cpu().double() - ref).abs().max().item(), ref.abs().max().item()
    print(f'{what}: |out-ref|={err:.3e} bar={BAR * scale:.3e}')
    assert err <= BAR * scale


@pytest.mark.parametrize('ks', [(3, 7, 11), (3, 7)], ids=['k3_7_11', 'k3_7'])
@pytest.mark.parametrize('L', [70, 384, 386])
@pytest.mark.parametrize('C', [128, 256])
def test_wide_sum_matches_fp64(dev, C, L, ks):
    xd, wpw, bd, ref = _problem(dev, C, L, ks)
    _check(_run(xd, wpw, bd, ks), ref, f'C={C} L={L} ks={ks}')


@pytest.mark.parametrize('ks', [(3, 7, 11), (3, 7)], ids=['k3_7_11', 'k3_7'])
@pytest.mark.parametrize('C', [128, 256])
def test_wide_sum_with_lengths_matches_fp64(dev, C, ks):
    """L = 200 with len = (200, 37): conv_wino_sum_len_kernel; an item's kept outputs are the statement's with the inputs past its end counted as zero."""
    xd, wpw, bd, ref = _problem(dev, C, 200, ks, lengths=ENDS)
    got = _run(xd, wpw, bd, ks, lengths=torch.tensor(ENDS, dtype=torch.int32, device=dev), len_mul=1)
    for b, e in enumerate(ENDS):
        _check(got[b, :, :e], ref[b, :, :e], f'C={C} ks={ks} item {b} end {e}')


def test_four_m_tiles_and_an_odd_tile_count(dev):
    """C = 256 is four row tiles of 64 channels; B = 3 x one tile per item is an odd number of position tiles."""
    ks = (3, 7, 11)
    xd, wpw, bd, ref = _problem(dev, 256, 70, ks, nb=3)
    _check(_run(xd, wpw, bd, ks), ref, 'C=256 B=3 L=70')


@pytest.mark.parametrize('C,L', [(128, 386), (256, 384)])
def test_walk_orders_are_within_the_bound(dev, C, L):
    ks = (3, 7, 11)
    xd, wpw, bd, ref = _problem(dev, C, L, ks)
    for order in ORDERS:
        _check(_run(xd, wpw, bd, ks, order=order), ref, f'C={C} L={L} order={order}')


def test_library_order_is_one_of_the_explicit_ones(dev):
    """order = None is the walk v2w_wino_sum_order reports: the same bits as that order given explicitly."""
    from wavthruvec_pytorch_amd import hipops
    ks = (3, 7, 11)
    xd, wpw, bd, _ = _problem(dev, 128, 386, ks)
    assert torch.equal(_run(xd, wpw, bd, ks), _run(xd, wpw, bd, ks, order=hipops.wino_sum_order(ks)))


def test_bias_and_residual_sums_do_not_depend_on_the_walk_order(dev):
    """Zero weights: the output is exactly ((b0 + b1) + b2 + ((t1_0 + t1_1) + t1_2)) / 3 in fp32, by branch index, for every walk order."""
    from wavthruvec_pytorch_amd import hipops
    ks, C, L = (3, 7, 11), 128, 386
    xd, _, bd, _ = _problem(dev, C, L, ks)
    zero = [hipops.pack_wino(torch.zeros((k, C, C), device=dev)) for k in ks]
    bc, xc = [b.cpu() for b in bd], [x.cpu() for x in xd]
    want = (((bc[0] + bc[1]) + bc[2])[None, :, None] + ((xc[0] + xc[1]) + xc[2])) / 3.0
    for order in ORDERS + [None]:
        assert torch.equal(_run(xd, zero, bd, ks, order=order).cpu(), want), order


def test_a_bad_order_is_an_argument_error(dev):
    from wavthruvec_pytorch_amd import hipops, _hip
    ks = (3, 7, 11)
    xd, wpw, bd, _ = _problem(dev, 128, 70, ks)
    out = torch.full_like(xd[0], SENT)
    for order in [(0, 0, 1), (0, 1, 3), (-1, 0, 1)]:
        with pytest.raises(_hip.HipLibraryError):
            hipops.conv1d_wino_sum([(x, w, b, k) for x, w, b, k in zip(xd, wpw, bd, ks)], out, dil=DIL, slope=SLOPE, out_div=3.0, order=order)
    torch.cuda.synchronize()
    assert bool((out == SENT).all())


def test_generator_with_the_shipped_wino_sum(dev):
    """One small forward (B = 2, T = 8, default hparams) with the shipped `wino_sum` against the oracle at the generator tests' bar, 1e-4;
    `lengths` all equal to T is bit-identical to none."""
    from wavthruvec_pytorch_amd import Generator, synthetic
    h = synthetic.make_hparams(num_wv_feat=768)
    sd = synthetic.make_state_dict(h, seed=5)
    inp = synthetic.make_inputs(h, 2, 8, seed=9)
    O.calibrate_running_stats(sd, h, *inp)      # eval mode (`lengths` needs it) on running statistics of these inputs
    want, _ = O.generator_forward({k: v.clone() for k, v in sd.items()}, h, *inp, training=False)
    g = Generator(h)
    g.load_state_dict(sd)
    g = g.to(dev).eval()
    with torch.no_grad():
        y0 = g(*(t.to(dev) for t in inp))
        y1 = g(*(t.to(dev) for t in inp), lengths=torch.full((2,), 8, dtype=torch.int64, device=dev))
    d = (y0.cpu() - want).abs().max().item()
    print(f'wino_sum={g.wino_sum} wino_sum_wide={g.wino_sum_wide}: max|dy| = {d:.3e}')
    assert torch.isfinite(y0).all() and d <= 1e-4
    assert torch.equal(y0, y1)
    # the fold wrote no stream twice: the wide stages' second convs have theirs from `wino`, only the 64-channel stage's are `wpw_sum`'s
    nk = g.num_kernels
    wpw, wpw_sum = g._fold_key['wpw'], g._fold_key['wpw_sum']
    assert not set(wpw) & set(wpw_sum)
    assert set(wpw_sum) == {f'resblocks.{i * nk + j}.convs.1' for i, up in enumerate(g.ups) if up.out_channels == 64 for j in range(nk)}
    assert all(f'resblocks.{i * nk + j}.convs.1' in wpw for i, up in enumerate(g.ups) if up.out_channels in g.wino_sum_wide for j in range(nk))
