"""GPU tests of the Winograd F(2,3) Conv1d kernel (hipops.ALGO_WINO, csrc/v2w_conv_wino.hip): its weight stream (v2w_pack_wino and the
batched fold) against the torch reference bit for bit, the kernel against the direct kernel with every epilogue operand, multi-problem
launches, run-to-run determinism, and the Generator switch."""
import numpy as np
import pytest
import torch

from tests import wino_ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a MI355X'
    from wavthruvec_pytorch_amd import _hip
    _hip.load()
    return torch.device('cuda:0')


def _rand(r, shape, scale=1.0):
    return torch.from_numpy((scale * r.standard_normal(shape)).astype(np.float32))


@pytest.mark.parametrize('k,ci,co', [(3, 64, 64), (7, 768, 512), (11, 256, 256), (5, 128, 96)])
def test_pack_wino_matches_the_reference_bitwise(dev, k, ci, co):
    from wavthruvec_pytorch_amd import hipops
    wf = _rand(np.random.default_rng(k), (k, ci, co))
    got = hipops.pack_wino(wf.to(dev))
    assert got is not None and torch.equal(got.cpu(), wino_ref.pack_ref(wf))


def test_batched_fold_writes_the_winograd_stream(dev):
    """v2w_fold_desc::wpw: the same stream as v2w_pack_wino of the folded weights the same pass writes in the plain layout."""
    from wavthruvec_pytorch_amd import hipops
    r = np.random.default_rng(3)
    layers, outs = [], []
    for k, ci, co in ((11, 256, 256), (7, 768, 512), (3, 64, 64)):
        v, g = _rand(r, (co, ci, k)).to(dev), (1 + 0.1 * _rand(r, (co, 1, 1))).to(dev)
        wp = torch.empty(k * ci * co, device=dev)
        wf = torch.empty((k, ci, co), device=dev)
        wpw = torch.full((hipops.wino_terms(k) * ci * co,), float('nan'), device=dev)
        layers.append((v, g, wp, ci, co, k, 1, False, wf, None, wpw))
        outs.append((wf, wpw))
    hipops.FoldPlan(layers, dev).run()
    for wf, wpw in outs:
        assert torch.equal(wpw, hipops.pack_wino(wf))


# (C, B, L0): sizes at which the kernel takes the launch (more than 128 workgroups); L = L0 + r covers every L mod 6
SIZES = [(256, 2, 2100), (128, 32, 300), (64, 32, 600), (256, 1, 4200)]


@pytest.mark.parametrize('dil', [1, 3])
@pytest.mark.parametrize('k', [3, 7, 11])
@pytest.mark.parametrize('r', range(6))
@pytest.mark.parametrize('C,B,L0', SIZES)
def test_wino_matches_direct(dev, C, B, L0, r, k, dil):
    """Against ALGO_DIRECT with the CondBN affine + leaky_relu on the input, the residual affine, addends (even r) or the running sum
    (odd r), and out_div; the Winograd kernel really ran (a declined launch would raise: no wp of the direct form is handed over)."""
    from wavthruvec_pytorch_amd import hipops
    L = L0 + r
    rng = np.random.default_rng(1000 * k + 10 * r + dil)
    x = _rand(rng, (B, C, L)).to(dev)
    wf = _rand(rng, (k, C, C), 1 / np.sqrt(C * k)).to(dev)
    bias = _rand(rng, (C,)).to(dev)
    ia = ((1 + 0.2 * _rand(rng, (B, C))).to(dev), (0.3 * _rand(rng, (B, C))).to(dev))
    res = _rand(rng, (B, C, L)).to(dev)
    ra = ((1 + 0.2 * _rand(rng, (B, C))).to(dev), (0.3 * _rand(rng, (B, C))).to(dev))
    prev = _rand(rng, (B, C, L)).to(dev)
    adds = [_rand(rng, (B, C, L)).to(dev) for _ in range(2)]
    kw = dict(k=k, dil=dil, slope=0.1, in_affine=ia, res=res, res_affine=ra, out_div=3.0)
    kw.update(dict(add=adds) if r % 2 == 0 else dict(accumulate=True))
    wpw = hipops.pack_wino(wf)
    o_w, o_w2, o_d = prev.clone(), prev.clone(), prev.clone()
    import ctypes as C_
    from wavthruvec_pytorch_amd import _hip
    for o in (o_w, o_w2):
        a = _hip.Conv1dArgs()
        hipops._conv1d_args(a, x, None, bias, o, algo=hipops.ALGO_WINO, wp=wpw, **kw)
        _hip.check(_hip.load().v2w_conv1d_fwd(C_.byref(a), hipops._stream(x)), 'v2w_conv1d_fwd')
    hipops.conv1d(x, wf, bias, o_d, algo=hipops.ALGO_DIRECT, **kw)
    torch.cuda.synchronize()
    assert torch.equal(o_w, o_w2), 'not run-to-run deterministic'
    err = (o_w - o_d).abs().max().item()
    assert err <= 2e-5 * max(1.0, o_d.abs().max().item()), err


def test_wino_multi_problem_launch(dev):
    """The three branches of a stage (k = 11, 7, 3, heaviest first) in ONE launch through conv1d_wino_multi: each equals its own launch
    bit for bit and the direct kernel to 2e-5; a launch the kernel declines (B = 1) runs on the f32 MFMA fallback."""
    from wavthruvec_pytorch_amd import hipops
    rng = np.random.default_rng(5)
    B, C, L = 8, 128, 1280
    x = _rand(rng, (B, C, L)).to(dev)
    ia = ((1 + 0.2 * _rand(rng, (B, C))).to(dev), (0.3 * _rand(rng, (B, C))).to(dev))
    probs, singles, directs = [], [], []
    for k, dil in ((11, 3), (7, 1), (3, 3)):
        wf = _rand(rng, (k, C, C), 1 / np.sqrt(C * k)).to(dev)
        bias = _rand(rng, (C,)).to(dev)
        kw = dict(k=k, dil=dil, slope=0.1, in_affine=ia, res=x, res_affine=ia)
        o, o1, od = (torch.empty((B, C, L), device=dev) for _ in range(3))
        probs.append((x, None, bias, o, dict(kw, wp=hipops.pack_mfma(wf), wpw=hipops.pack_wino(wf))))
        hipops.conv1d(x, None, bias, o1, wp=hipops.pack_mfma(wf), wpw=hipops.pack_wino(wf), **kw)
        hipops.conv1d(x, wf, bias, od, algo=hipops.ALGO_DIRECT, **kw)
        singles.append(o1); directs.append(od)
    hipops.conv1d_multi(probs)
    torch.cuda.synchronize()
    for (_x, _w, _b, o, _kw), o1, od in zip(probs, singles, directs):
        assert torch.equal(o, o1)
        assert (o - od).abs().max().item() <= 2e-5 * max(1.0, od.abs().max().item())
    # declined (40 workgroups): the fallback stream serves it
    x1 = x[:1].contiguous()
    wf = _rand(rng, (7, C, C), 1 / np.sqrt(C * 7)).to(dev)
    o, od = torch.empty((1, C, L), device=dev), torch.empty((1, C, L), device=dev)
    hipops.conv1d(x1, None, None, o, k=7, dil=1, slope=0.1, wp=hipops.pack_mfma(wf), wpw=hipops.pack_wino(wf))
    hipops.conv1d(x1, wf, None, od, k=7, dil=1, slope=0.1, algo=hipops.ALGO_DIRECT)
    assert (o - od).abs().max().item() <= 2e-5 * max(1.0, od.abs().max().item())


@pytest.mark.parametrize('training', [True, False])
def test_generator_switch_on_vs_off(dev, training):
    """Generator.wino on vs off at a size where the kernel takes the residual convs of stages 0-2: within 1e-6 (two modules from one state
    dict - a train-mode forward advances the spectral-norm vectors); a replayed eval-mode forward is bit-identical; the switch flipped on one
    module re-plans.  Eval mode runs on running statistics calibrated by a train-mode pass: with the synthetic state dict's own ones the
    output is 99 % saturated and any two summation orders (direct vs f32 MFMA kernel as much as these two) differ by ~1e-2."""
    from wavthruvec_pytorch_amd import Generator, synthetic
    h = synthetic.make_hparams(num_wv_feat=768)
    sd = synthetic.make_state_dict(h, seed=5)
    inp = tuple(t.to(dev) for t in synthetic.make_inputs(h, 8, 128, seed=9))
    ys = {}
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
        g.wino = on
        with torch.no_grad():
            ys[on] = g(*inp)
            assert len(g._fold_key.get('wpw', {})) == (16 if on else 0)     # conv_pre + the residual convs of stages 0-2 but the 64-channel dilation-3 ones
            if not training:
                assert torch.equal(ys[on], g(*inp))
                g.wino = not on
                y_flip = g(*inp)
                assert len(g._fold_key.get('wpw', {})) == (0 if on else 16)
                assert (y_flip - ys[on]).abs().max().item() <= 1e-6
    d = (ys[True] - ys[False]).abs().max().item()
    assert d <= 1e-6, d
