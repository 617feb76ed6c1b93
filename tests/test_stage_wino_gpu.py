"""GPU tests of the Winograd F(2,3) form of the fused 32-channel stage kernel (hipops.resblock2_stage_wino, csrc/v2w_resblock_fused.hip):
the entry point against the direct-form stage kernel and an fp64 statement of the section, at the tile seams of both window sizes, run to
run, and the Generator switch `wino_stage`."""
import numpy as np
import pytest
import torch

from tests import tile_ref

pytestmark = pytest.mark.gpu

KS, D1, D2 = [3, 7, 11], [1, 1, 1], [3, 3, 3]
SLOPE = 0.1
BIG_B, BIG_TILES = 2, 113          # 226 windows of 256 positions: past the 224 below which the launch takes windows of 128


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a MI355X'
    from wavthruvec_pytorch_amd import _hip
    _hip.load()
    return torch.device('cuda:0')


def _rand(r, shape, scale=1.0):
    return torch.from_numpy((scale * r.standard_normal(shape)).astype(np.float32))


def _section_ref(x, ia, ws, bs):
    """The section in float64: out = (sum_j [t1_j + conv2_j(lrelu(t1_j)) + b2_j]) / nk, t1_j = x + conv1_j(lrelu(x)) + b1_j, x = a * in + s."""
    xa = tile_ref.f64(ia[0])[:, :, None] * tile_ref.f64(x) + tile_ref.f64(ia[1])[:, :, None]
    total = None
    for (w1, w2), (b1, b2), k, d1, d2 in zip(ws, bs, KS, D1, D2):
        t1 = xa + tile_ref.taps_sum(tile_ref.lrelu(xa, SLOPE), w1, d1, d1 * (k - 1) // 2)[0] + tile_ref.f64(b1)[None, :, None]
        r = t1 + tile_ref.taps_sum(tile_ref.lrelu(t1, SLOPE), w2, d2, d2 * (k - 1) // 2)[0] + tile_ref.f64(b2)[None, :, None]
        total = r if total is None else total + r
    return total / len(KS)


def _problem(dev, B, L, seed):
    from wavthruvec_pytorch_amd import hipops
    rng = np.random.default_rng(seed)
    x = _rand(rng, (B, 32, L))
    ia = (1 + 0.2 * _rand(rng, (B, 32)), 0.3 * _rand(rng, (B, 32)))
    ws = [(_rand(rng, (k, 32, 32), 1 / np.sqrt(32 * k)), _rand(rng, (k, 32, 32), 1 / np.sqrt(32 * k))) for k in KS]
    bs = [(_rand(rng, (32,)), _rand(rng, (32,))) for _ in KS]
    ref = _section_ref(x, ia, ws, bs)
    xd, iad = x.to(dev), tuple(t.to(dev) for t in ia)
    direct = [dict(wp1=hipops.pack_mfma(w1.to(dev)), wp2=hipops.pack_mfma(w2.to(dev)), b1=b1.to(dev), b2=b2.to(dev), k=k, dil1=d1, dil2=d2)
              for (w1, w2), (b1, b2), k, d1, d2 in zip(ws, bs, KS, D1, D2)]
    wino = [dict(wpw1=hipops.pack_wino(w1.to(dev)), wpw2=hipops.pack_wino(w2.to(dev)), b1=br['b1'], b2=br['b2'], k=br['k'], dil1=br['dil1'],
                 dil2=br['dil2']) for (w1, w2), br in zip(ws, direct)]
    return xd, iad, direct, wino, ref


def _nadv(B, L):
    from wavthruvec_pytorch_amd import hipops
    n = hipops.resblock2_stage_wino_tile(B, 32, L, KS, D1, D2)
    assert n > 0 and n % 4 == 0, n
    return n


def _cases():
    """(id, B, L as a function of the kept outputs per tile): shorter than every halo, one partial tile, an exact tile, a seam and a 4-wide
    last tile, two seams, L % 4 != 0 (scalar staging and stores) - on the windows of 128 positions small launches take - and the same seams
    at the far end of a launch large enough for the windows of 256 (every tile start in between is a seam too)."""
    out = []
    for B in (1, 2):
        for name, fn in (('L4', lambda n: 4), ('L60', lambda n: 60), ('tile', lambda n: n), ('seam4', lambda n: n + 4),
                         ('seams', lambda n: 2 * n + 4), ('odd', lambda n: n + 7)):
            out.append((f'w128-B{B}-{name}', B, fn, False))
    for name, fn in (('tile', lambda n: BIG_TILES * n), ('seam4', lambda n: (BIG_TILES - 1) * n + 4), ('odd', lambda n: (BIG_TILES - 1) * n + 7)):
        out.append((f'w256-{name}', BIG_B, fn, True))
    return out


CASES = _cases()


@pytest.mark.parametrize('case', CASES, ids=[c[0] for c in CASES])
def test_stage_wino_matches_the_direct_stage_kernel(dev, case):
    """The Winograd form against the direct-form stage kernel on the same inputs: within 2 x 2e-5 x max(1, max|ref|) - the project's bar for
    ONE Winograd conv against direct form (test_wino_matches_direct), twice because the section chains two convs (weights scaled
    1 / sqrt(C k)).  Both kernels' errors against the fp64 section are printed, not asserted; so is the position of the worst difference
    (a seam or an edge bug sits at a tile start or at the ends, rounding anywhere).  Two launches are bit-identical.  The entry point is
    called directly: a launch it declined would return False here - nothing falls back.
    Measured on MI355X: max |wino - direct| = 3.5e-6 over all cases (w256-seam4, max|ref| = 10.7, bar 4.3e-4: under a hundredth of it; the
    worst positions sit mid-tile, pos % nadv = 89 .. 104); against fp64 the Winograd form 1.5e-6, the direct form 3.4e-6."""
    from wavthruvec_pytorch_amd import hipops
    _id, B, fn, big = case
    nadv = _nadv(B, 60) if not big else _nadv(BIG_B, 224 * BIG_TILES)
    L = fn(nadv)
    assert _nadv(B, L) == nadv, 'the case must run on the window size it names'
    assert nadv == (224 if big else 96)
    x, ia, direct, wino, ref = _problem(dev, B, L, seed=17 * L + B)
    o_w, o_w2, o_d = (torch.full((B, 32, L), float('nan'), device=dev) for _ in range(3))
    for o in (o_w, o_w2):
        assert hipops.resblock2_stage_wino(x, ia, wino, o, slope=SLOPE, out_div=3.0), 'the Winograd stage kernel declined the launch'
    assert hipops.resblock2_stage(x, ia, direct, o_d, slope=SLOPE, out_div=3.0)
    torch.cuda.synchronize()
    assert torch.equal(o_w, o_w2), 'not run-to-run deterministic'
    assert torch.isfinite(o_w).all()
    scale = max(1.0, ref.abs().max().item())
    diff = (o_w - o_d).abs()
    err = diff.max().item()
    b, c, pos = np.unravel_index(int(diff.argmax().item()), diff.shape)
    e_w = (o_w.double().cpu() - ref).abs().max().item()
    e_d = (o_d.double().cpu() - ref).abs().max().item()
    print(f'{_id}: L={L} nadv={nadv} |wino-direct|={err:.3e} at (b={b}, c={c}, pos={pos}, pos%nadv={pos % nadv}) bar={4e-5 * scale:.3e} '
          f'|wino-fp64|={e_w:.3e} |direct-fp64|={e_d:.3e} max|ref|={scale:.3f}')
    assert err <= 2 * 2e-5 * scale, (err, (b, c, pos))


@pytest.mark.parametrize('B,L,lens', [(2, 200, [200, 200]), (2, 200, [77, 200]), (2, 200, [3, 130]), (BIG_B, 112 * 224 + 4, [112 * 224 + 4, 9001])],
                         ids=['w128-full', 'w128-short', 'w128-seam', 'w256'])
def test_stage_wino_per_item_lengths(dev, B, L, lens):
    """v2w_resblock2_stage_wino_fwd_len: with every length L bit-identical to the call without lengths; else every item's valid part is
    bit-identical to that item run alone at its own length, whatever the input holds past it (NaN here), as the direct kernel's LEN form."""
    from wavthruvec_pytorch_amd import hipops
    x, ia, _direct, wino, _ref = _problem(dev, B, L, seed=5 * L + lens[-1])
    full = torch.empty((B, 32, L), device=dev)
    assert hipops.resblock2_stage_wino(x, ia, wino, full, slope=SLOPE, out_div=3.0)
    xp = x.clone()
    for b, n in enumerate(lens):
        xp[b, :, n:] = float('nan')
    out = torch.zeros((B, 32, L), device=dev)
    lt = torch.tensor(lens, dtype=torch.int32, device=dev)
    assert hipops.resblock2_stage_wino(xp, ia, wino, out, slope=SLOPE, out_div=3.0, lengths=lt, len_mul=1)
    torch.cuda.synchronize()
    for b, n in enumerate(lens):
        if n == L:
            assert torch.equal(out[b], full[b])
            continue
        xb = x[b:b + 1, :, :n].contiguous()
        alone = torch.empty((1, 32, n), device=dev)
        assert hipops.resblock2_stage_wino(xb, (ia[0][b:b + 1].contiguous(), ia[1][b:b + 1].contiguous()), wino, alone, slope=SLOPE, out_div=3.0)
        got = out[b:b + 1, :, :n]
        assert torch.isfinite(got).all()
        if hipops.resblock2_stage_wino_tile(1, 32, n, KS, D1, D2) == hipops.resblock2_stage_wino_tile(B, 32, L, KS, D1, D2):
            assert torch.equal(got, alone), (b, n)          # (the same window size: the same sums in the same order)
        else:
            assert (got - alone).abs().max().item() <= 4e-5 * max(1.0, alone.abs().max().item()), (b, n)


def test_stage_wino_declines_what_it_does_not_serve(dev):
    """16 channels, a first dilation other than 1, an even kernel size: False (V2W_E_SHAPE), nothing written."""
    from wavthruvec_pytorch_amd import hipops
    x, ia, _direct, wino, _ref = _problem(dev, 1, 60, seed=3)
    out = torch.full((1, 32, 60), 7.0, device=dev)
    bad = [dict(br, dil1=3) for br in wino]
    assert hipops.resblock2_stage_wino(x, ia, bad, out, slope=SLOPE, out_div=3.0) is False
    bad = [dict(br, k=4) for br in wino]
    assert hipops.resblock2_stage_wino(x, ia, bad, out, slope=SLOPE, out_div=3.0) is False
    x16, out16 = x[:, :16].contiguous(), out[:, :16].contiguous()
    assert hipops.resblock2_stage_wino(x16, (ia[0][:, :16].contiguous(), ia[1][:, :16].contiguous()), wino, out16, slope=SLOPE, out_div=3.0) is False
    torch.cuda.synchronize()
    assert (out == 7.0).all() and (out16 == 7.0).all()
    assert hipops.resblock2_stage_wino_tile(1, 16, 60, KS, D1, D2) == 0


@pytest.mark.parametrize('training', [True, False])
def test_generator_wino_stage_on_vs_off(dev, training):
    """Generator.wino_stage on vs off (two modules from one state dict, as test_generator_switch_on_vs_off): six streams under
    _fold_key['wpw_stage'] when on and none when off, _fold_key['wpw'] the same either way, the flag flipped on one module re-plans, an
    eval-mode replay is bit-identical, and the outputs agree within the existing switch test's bar, 1e-6 (eval mode on statistics calibrated
    by a train-mode pass; train mode on batch statistics).  Measured on MI355X: |dy| = 7.6e-8 in train mode at max|y| = 0.15."""
    from wavthruvec_pytorch_amd import Generator, synthetic
    h = synthetic.make_hparams(num_wv_feat=768)
    sd = synthetic.make_state_dict(h, seed=5)
    inp = tuple(t.to(dev) for t in synthetic.make_inputs(h, 2, 8, seed=9))
    ys, names = {}, {}
    for on in (True, False):
        g = Generator(h)
        g.load_state_dict(sd)
        g = g.to(dev)
        if not training:
            for m in g.modules():
                if isinstance(m, torch.nn.BatchNorm1d):
                    m.momentum = None
                    m.reset_running_stats()
            with torch.no_grad():
                g(*inp)
        g.train(training)
        g.wino_stage = on
        with torch.no_grad():
            ys[on] = g(*inp)
            assert len(g._fold_key.get('wpw_stage', {})) == (6 if on else 0)
            names[on] = sorted(g._fold_key.get('wpw', {}))
            if not training:
                assert torch.equal(ys[on], g(*inp))
                ntapes = len(g._tapes)
                assert torch.equal(ys[on], g(*inp)) and len(g._tapes) == ntapes      # (a replay of the recorded plan)
                g.wino_stage = not on
                y_flip = g(*inp)
                # planned again: only a planned forward runs _fold_weights, which alone rewrites this table (a replay never does)
                assert len(g._fold_key.get('wpw_stage', {})) == (0 if on else 6)
                assert sorted(g._fold_key.get('wpw', {})) == names[on]
                d_flip = (y_flip - ys[on]).abs().max().item()
                print(f'eval: flipped on one module |dy|={d_flip:.3e}')
                assert d_flip <= 1e-6, d_flip
    assert names[True] == names[False]
    d = (ys[True] - ys[False]).abs().max().item()
    print(f'training={training}: wino_stage on vs off |dy|={d:.3e} max|y|={ys[False].abs().max().item():.3f}')
    assert d <= 1e-6, d
