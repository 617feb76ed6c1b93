"""GPU tests of the upsampler form of the Winograd kernel (hipops.convt1d_wino, v2w_convt1d_wino_fwd, csrc/v2w_conv_wino.hip): the stream the
batched fold writes against tests/wino_up_ref.py bit for bit; every output entry against the fp64 transposed conv with the per-entry
bound n * 2^-24 * S over the operands as the kernel rounds them (wino_up_ref), never looser than the one-conv Winograd kernel's bar
(tests/test_wino_gpu.py: 2e-5 max(1, max |ref|)); the direct conv_tile_kernel on the same records against its own bound (tests/tile_ref.py);
the per-tile statistics rows; canaries around the output and the statistics rows; and the Generator switch.

Statistics bound.  A slot is an fp32 chain over the stored values v_i of one tile and channel: 2 u values per lane, 5 shuffle levels, 2
waves, i.e. m = 2 u + 7 additions (sumsq: one more rounding, the fma's).  With e_i the per-entry bound of v_i, the sum over the tiles (fp64
here) is within sum e_i + m 2^-24 sum |v_i| of the exact sum, the sum of squares within sum (2 |v_i| e_i + e_i^2) + (m + 1) 2^-24 sum v_i^2."""
import numpy as np
import pytest
import torch

from tests import tile_ref, wino_up_ref as R
from tests.disc_ref import f64

pytestmark = pytest.mark.gpu

SHAPES = [(64, 32, 4, 2), (128, 64, 8, 4), (256, 128, 8, 4)]       # (C_in, C_out, k, u): ups.3, ups.2, ups.1
LENGTHS = [1, 2, 63, 64, 65, 127, 129]      # a lone single, tile edges on both sides (64 pairs = 128 positions t = 0 .. L), odd and even counts
SENT = -7.25
MARGIN = 64
# (staging affine + leaky_relu, bias, stats_part)
COMBOS = [(True, True, True), (False, False, False), (True, False, True), (False, True, False)]


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a MI355X'
    from wavthruvec_pytorch_amd import _hip
    _hip.load()
    return torch.device('cuda:0')


def _rand(r, shape, scale=1.0):
    return torch.from_numpy((scale * r.standard_normal(shape)).astype(np.float32))


@pytest.fixture(scope='module')
def layers(dev):
    """Per shape: the plain weight w [C_in][C_out][k] (CPU), and on the device what ONE batched fold wrote for it: wf, wp (direct tile), wpw."""
    from wavthruvec_pytorch_amd import hipops
    r = np.random.default_rng(16)
    out, batch = {}, []
    for ci, co, k, u in SHAPES:
        w = _rand(r, (ci, co, k), 1 / np.sqrt(2 * ci))
        wp = torch.empty(k * ci * co, device=dev)
        wf = torch.empty((k, ci, co), device=dev)
        wpw = torch.full((3 * u * co * ci + MARGIN,), SENT, device=dev)
        batch.append((w.to(dev), None, wp, ci, co, k, u, True, wf, None, wpw))
        out[(ci, co, k, u)] = dict(w=w, wp=wp, wf=wf, wpw=wpw)
    hipops.FoldPlan(batch, dev).run()
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize('shape', SHAPES)
def test_fold_writes_the_stream_bitwise(layers, shape):
    ci, co, k, u = shape
    rec = layers[shape]
    got = rec['wpw'].cpu()
    assert torch.equal(got[:-MARGIN], R.stream_ref(rec['w'], u)) and bool((got[-MARGIN:] == SENT).all())
    assert torch.equal(rec['wf'].cpu(), rec['w'].permute(2, 0, 1).contiguous())


def _guarded(dev, shape):
    flat = torch.full((int(np.prod(shape)) + 2 * MARGIN,), SENT, device=dev)
    return flat, flat[MARGIN:-MARGIN].view(shape)


def _worst(err, bound):
    ok = bound > 0
    return float((err[ok] / bound[ok]).max()) if bool(ok.any()) else 0.0


@pytest.mark.parametrize('L', LENGTHS)
@pytest.mark.parametrize('B', [1, 3])
@pytest.mark.parametrize('shape', SHAPES)
def test_kernel_per_entry_against_fp64(dev, layers, shape, B, L):
    from wavthruvec_pytorch_amd import hipops
    ci, co, k, u = shape
    rec = layers[shape]
    r = np.random.default_rng(1000 * ci + 10 * L + B)
    x = _rand(r, (B, ci, L))
    ia, is_ = 1 + 0.2 * _rand(r, (B, ci)), 0.3 * _rand(r, (B, ci))
    bias = _rand(r, (co,))
    xd, iad, isd, biasd = x.to(dev), ia.to(dev), is_.to(dev), bias.to(dev)
    tiles, wgs = hipops.convt_wino_tiles(B, ci, co, L, k, u)
    assert tiles == B * (-(-((L + 2) // 2) // 64)) and wgs == tiles * (u * co // 64)
    T64 = R.terms(f64(rec['w']), u)
    for aff, use_bias, use_stats in COMBOS:
        slope = 0.1 if aff else 1.0
        act = R.activate(x, slope, ia if aff else None, is_ if aff else None)
        want, S = R.convt_from_terms(T64, act, u, bias if use_bias else None)
        e = R.n_ops(ci) * R.U24 * S
        bar = torch.minimum(e, torch.full_like(e, 2e-5 * max(1.0, want.abs().max().item())))
        flat, out = _guarded(dev, (B, co, u * L))
        sflat, part = _guarded(dev, (tiles, co, 2))
        assert hipops.convt1d_wino(xd, rec['wpw'][:-MARGIN], biasd if use_bias else None, out, k=k, u=u, slope=slope,
                                   in_affine=(iad, isd) if aff else None, stats_part=part if use_stats else None) is True
        # the direct tile on the same record (it has no staging affine: the affine is applied in fp32 in front of it)
        xa = torch.addcmul(isd[:, :, None], iad[:, :, None], xd) if aff else xd
        od = torch.empty((B, co, u * L), device=dev)
        hipops.convt1d(xa, rec['wf'], biasd if use_bias else None, od, k=k, u=u, slope=slope, algo=hipops.ALGO_MFMA, wp=rec['wp'])
        torch.cuda.synchronize()
        got, fl = f64(out.cpu()), flat.cpu()
        assert bool((fl[:MARGIN] == SENT).all()) and bool((fl[-MARGIN:] == SENT).all()), 'wrote outside the output'
        err = (got - want).abs()
        wd, Sd = tile_ref.convt1d(xa.cpu() if aff else x, rec['w'].permute(2, 0, 1), u, slope=slope, bias=bias if use_bias else None)
        errd, ed = (f64(od.cpu()) - wd).abs(), (2 * ci + 2) * R.U24 * Sd
        print(f'[wino_up] {shape} B={B} L={L} aff={aff} bias={use_bias} stats={use_stats}: max err {err.max().item():.3e}  worst err / bound '
              f'{_worst(err, e):.3f} (direct tile: {_worst(errd, ed):.3f})  entries over the bar {int((~(err <= bar)).sum())}')
        assert bool((err <= bar).all()), (err.max().item(), _worst(err, bar))
        assert bool((errd <= ed).all())
        sf = sflat.cpu()
        assert bool((sf[:MARGIN] == SENT).all()) and bool((sf[-MARGIN:] == SENT).all()), 'wrote outside the statistics rows'
        if not use_stats:
            assert bool((sf == SENT).all())
            continue
        st = f64(part.cpu()).sum(0)                              # (C_out, 2): the tiles added in fp64
        m = 2 * u + 7
        s1, s2, sa = want.sum((0, 2)), (want * want).sum((0, 2)), want.abs().sum((0, 2))
        b1 = e.sum((0, 2)) + m * R.U24 * sa
        b2 = (2 * want.abs() * e + e * e).sum((0, 2)) + (m + 1) * R.U24 * s2
        print(f'          stats: worst sum ratio {_worst((st[:, 0] - s1).abs(), b1):.3f}  sumsq ratio {_worst((st[:, 1] - s2).abs(), b2):.3f}')
        assert bool(((st[:, 0] - s1).abs() <= b1).all()) and bool(((st[:, 1] - s2).abs() <= b2).all())


def test_vector_staging_unaligned_output_and_determinism(dev, layers):
    """L % 4 == 0 on an aligned input takes the float4 staging (the generator's case); an output 4 bytes off takes the scalar stores: the
    same bits; two runs are bit-identical."""
    from wavthruvec_pytorch_amd import hipops
    for shape, B, L in (((128, 64, 8, 4), 2, 256), ((64, 32, 4, 2), 2, 132)):
        ci, co, k, u = shape
        rec = layers[shape]
        r = np.random.default_rng(L)
        x, bias = _rand(r, (B, ci, L)).to(dev), _rand(r, (co,)).to(dev)
        outs = []
        for off in (0, 0, 1):
            flat = torch.full((B * co * u * L + 2 * MARGIN,), SENT, device=dev)
            out = flat[MARGIN + off:MARGIN + off + B * co * u * L].view(B, co, u * L)
            assert hipops.convt1d_wino(x, rec['wpw'][:-MARGIN], bias, out, k=k, u=u, slope=0.1) is True
            torch.cuda.synchronize()
            fl = flat.cpu()
            assert bool((fl[:MARGIN + off] == SENT).all()) and bool((fl[MARGIN + off + B * co * u * L:] == SENT).all())
            outs.append(out.clone())
        assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
        x1 = x[:, :, :L - 1].contiguous()                        # ragged L: the scalar staging, the same values where both are defined
        o1 = torch.empty((B, co, u * (L - 1)), device=dev)
        assert hipops.convt1d_wino(x1, rec['wpw'][:-MARGIN], bias, o1, k=k, u=u, slope=0.1) is True
        want, S = R.convt_from_terms(R.terms(f64(rec['w']), u), R.activate(x.cpu(), 0.1), u, bias.cpu())
        assert bool(((f64(outs[0].cpu()) - want).abs() <= R.n_ops(ci) * R.U24 * S).all())
        assert torch.equal(o1[:, :, :u * (L - 2)], outs[0][:, :, :u * (L - 2)])


def _forward(dev, wino_up, B, T, *, mode='plain', lengths=None):
    from wavthruvec_pytorch_amd import Generator, synthetic
    h = synthetic.make_hparams(num_wv_feat=768)
    g = Generator(h)
    g.load_state_dict(synthetic.make_state_dict(h, seed=5))
    g = g.to(dev).train(mode != 'lengths')
    g.wino_up = wino_up
    inp = tuple(t.to(dev) for t in synthetic.make_inputs(h, B, T, seed=9))
    if mode == 'save':
        y = g(*inp)
        assert y.requires_grad
        return y.detach(), g, inp
    with torch.no_grad():
        y = g(*inp, lengths=lengths) if mode == 'lengths' else g(*inp)
    return y, g, inp


def test_generator_switch_small_forward(dev):
    """B = 2, T = 8, train mode: `wino_up = (1, 2, 3)` against `()` within the bar of the other Winograd switches (tests/test_wino_gpu.py:
    1e-6).  At this size every upsampler launch is below the planner's size rule, so today's launches run."""
    y1, _g, _i = _forward(dev, (1, 2, 3), 2, 8)
    y0, _g, _i = _forward(dev, (), 2, 8)
    assert (y1 - y0).abs().max().item() <= 1e-6


def test_generator_switch_with_the_launches_taken(dev):
    """B = 8, T = 64: ups.1 / ups.2 / ups.3 pass the size rule (192 / 352 / 328 workgroups), conv_wino_up_kernel runs behind the unchanged
    tags `ups.i`, the fold built the three streams, and the output stays within the same 1e-6 of the switch-off forward."""
    y1, g, inp = _forward(dev, (1, 2, 3), 8, 64)
    y0, g0, _i = _forward(dev, (), 8, 64)
    assert sorted(g._fold_key['wpw_up']) == ['ups.1', 'ups.2', 'ups.3'] and not g0._fold_key.get('wpw_up')
    d = (y1 - y0).abs().max().item()
    print(f'[wino_up] generator B=8 T=64: max |dy| = {d:.3e} at max |y| = {y0.abs().max().item():.3f}')
    assert d <= 1e-6
    g.eval()
    names = g.profile_kernel_names(*inp)
    assert names['ups.1'] == ['conv_wino_up_kernel<4, 1, 2, 3, true>'] and names['ups.2'] == ['conv_wino_up_kernel<4, 1, 2, 3, true>']
    assert names['ups.3'] == ['conv_wino_up_kernel<2, 1, 2, 3, true>']
    assert not any('conv_wino_up_kernel' in n for tag, ns in names.items() if tag not in ('ups.1', 'ups.2', 'ups.3') for n in ns)


@pytest.mark.parametrize('mode', ['lengths', 'save'])
def test_lengths_and_saved_forwards_keep_todays_bits(dev, mode):
    kw = dict(lengths=[64, 64, 64, 64, 64, 64, 64, 64]) if mode == 'lengths' else {}
    y1, g, _i = _forward(dev, (1, 2, 3), 8, 64, mode=mode, **kw)
    y0, _g, _i = _forward(dev, (), 8, 64, mode=mode, **kw)
    assert torch.equal(y1, y0)
    if mode == 'save':
        assert not g._fold_key.get('wpw_up')
