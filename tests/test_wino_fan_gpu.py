"""GPU tests of the fan-out Winograd launch (hipops.conv1d_wino_fan -> v2w_conv1d_wino_fan_fwd, csrc/v2w_conv_wino.hip): the first convs of a
ResBlock2 stage's branches over one staged input.  Every output is compared BIT FOR BIT with the one-conv kernel's (conv_wino_kernel through
v2w_conv1d_fwd, V2W_ALGO_WINO - a declined launch raises) and with the fp64 statement tests/wino_ref.py at the bar of tests/test_wino_tail_gpu.py,
2e-5 max(1, max |ref|) on every entry.  C = 64, dilation 1, slope 0.1, seeded normal inputs.

The one-conv kernel declines launches of 128 workgroups or fewer, and the cases below are a handful of tiles.  A workgroup computes one tile of
one batch item from that item's rows alone, so the reference launch runs on the case's items repeated to REF_B items and its first B items
are compared: the same kernel on the same problems."""
import ctypes as C_

import numpy as np
import pytest
import torch

from tests import wino_ref

pytestmark = pytest.mark.gpu

C, DIL, SLOPE = 64, 1, 0.1
REF_B = 136         # items of the one-conv reference launches (more than 128 workgroups at one tile per item)
SENT = -7.0e30
GUARD = 4096


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a MI355X'
    from wavthruvec_pytorch_amd import _hip
    _hip.load()
    return torch.device('cuda:0')


def _rand(r, shape, scale=1.0):
    return torch.from_numpy((scale * r.standard_normal(shape)).astype(np.float32))


def _guarded(shape, dev):
    n = int(np.prod(shape))
    flat = torch.full((n + 2 * GUARD,), SENT, device=dev)
    return flat, flat[GUARD:GUARD + n].view(shape)


def _guards_intact(flat, shape):
    n = int(np.prod(shape))
    return bool((flat[:GUARD] == SENT).all()) and bool((flat[GUARD + n:] == SENT).all())


_CASES = {}


def _case(dev, B, L, affine=True):
    """Inputs of a case and, per kernel size, the one-conv kernel's output and the fp64 statement - computed once, shared, never written."""
    key = (B, L, affine)
    if key in _CASES:
        return _CASES[key]
    from wavthruvec_pytorch_amd import _hip, hipops
    rng = np.random.default_rng(7000 + 10 * L + B + (0 if affine else 5))
    x = _rand(rng, (B, C, L))
    ia = (1 + 0.2 * _rand(rng, (B, C)), 0.3 * _rand(rng, (B, C))) if affine else None
    rep = (REF_B + B - 1) // B
    xb = x.repeat(rep, 1, 1)[:REF_B].contiguous().to(dev)
    iab = tuple(t.repeat(rep, 1)[:REF_B].contiguous().to(dev) for t in ia) if affine else None
    xa = x.double() if not affine else ia[0].double()[:, :, None] * x.double() + ia[1].double()[:, :, None]
    per_k = {}
    for k in (3, 7, 11):
        wf = _rand(rng, (k, C, C), 1 / np.sqrt(C * k))
        bias = _rand(rng, (C,))
        wpw = hipops.pack_wino(wf.to(dev))
        o = torch.empty((REF_B, C, L), device=dev)
        a = _hip.Conv1dArgs()
        hipops._conv1d_args(a, xb, None, bias.to(dev), o, algo=hipops.ALGO_WINO, wp=wpw, k=k, dil=DIL, slope=SLOPE, in_affine=iab, res=xb, res_affine=iab)
        _hip.check(_hip.load().v2w_conv1d_fwd(C_.byref(a), hipops._stream(xb)), 'v2w_conv1d_fwd')
        torch.cuda.synchronize()
        ref = wino_ref.conv1d(torch.nn.functional.leaky_relu(xa, SLOPE), wf.permute(2, 1, 0).double(), bias.double(), dilation=DIL) + xa
        per_k[k] = dict(wpw=wpw, bias=bias.to(dev), single=o[:B].clone(), ref=ref)
    _CASES[key] = dict(x=x.to(dev), ia=tuple(t.to(dev) for t in ia) if affine else None, k=per_k)
    return _CASES[key]


def _fan(dev, case, ks, B, L):
    from wavthruvec_pytorch_amd import hipops
    outs = [_guarded((B, C, L), dev) for _ in ks]
    assert hipops.conv1d_wino_fan(case['x'], [(case['k'][k]['wpw'], case['k'][k]['bias'], o, k) for k, (_f, o) in zip(ks, outs)],
                                  dil=DIL, slope=SLOPE, in_affine=case['ia'], res=case['x'], res_affine=case['ia'])
    torch.cuda.synchronize()
    return outs


def _check(case, ks, outs, B, L):
    for k, (flat, o) in zip(ks, outs):
        want, ref = case['k'][k]['single'], case['k'][k]['ref']
        err = (o.cpu().double() - ref).abs().max().item()
        bound = 2e-5 * max(1.0, ref.abs().max().item())
        print(f'B={B} L={L} k={k}: bitwise {bool(torch.equal(o, want))}  max|fan - fp64| = {err:.3e}  bound {bound:.3e}')
        assert torch.equal(o, want), f'k={k}: not the one-conv kernel\'s bits ({int((o != want).sum())} entries differ)'
        assert err <= bound, (k, err, bound)
        assert _guards_intact(flat, (B, C, L)), f'k={k}: stored outside the output tensor'


# B = 2, L = 128: one full tile per item.  L = 132: a second tile with one live and one dead column-wave, the tail tiles last.
# B = 1, L = 130: L % 4 != 0, the scalar staging instantiation.  L = 131: a short last pair (its second output, position L, is not stored).
@pytest.mark.parametrize('B,L', [(2, 128), (2, 132), (1, 130), (2, 131)])
def test_fan_is_the_one_conv_kernel_bit_for_bit(dev, B, L):
    case = _case(dev, B, L)
    _check(case, (3, 7, 11), _fan(dev, case, (3, 7, 11), B, L), B, L)


def test_fan_without_the_input_affine(dev):
    case = _case(dev, 2, 256, affine=False)
    _check(case, (3, 7, 11), _fan(dev, case, (3, 7, 11), 2, 256), 2, 256)


@pytest.mark.parametrize('ks', [(3, 7), (11,), (11, 3, 7)])
def test_fan_source_lists_and_orders(dev, ks):
    """The outputs are independent: any list, any order, the same bits per conv."""
    case = _case(dev, 2, 132)
    _check(case, ks, _fan(dev, case, ks, 2, 132), 2, 132)


def test_short_last_pair_leaves_the_bytes_past_L(dev):
    """L = 131: pair 65 is (130, 131) and 131 is past the end.  The buffers start out poisoned; every row's last entry is the one-conv
    kernel's, the entry behind the tensor's last row keeps the poison (a store at position L of a row would land there or on the next row)."""
    B, L = 2, 131
    case = _case(dev, B, L)
    for k, (flat, o) in zip((3, 7, 11), _fan(dev, case, (3, 7, 11), B, L)):
        assert torch.equal(o, case['k'][k]['single']) and not bool((o == SENT).any())
        assert bool((flat[GUARD + B * C * L:] == SENT).all()) and bool((flat[:GUARD] == SENT).all())


def test_refusals(dev):
    from wavthruvec_pytorch_amd import _hip, hipops
    rng = np.random.default_rng(11)
    B, L = 2, 128

    def problem(Cc, n=3):
        x = _rand(rng, (B, Cc, L)).to(dev)
        outs = [torch.full((B, Cc, L), SENT, device=dev) for _ in range(n)]
        wpws = [hipops.pack_wino(_rand(rng, (k, Cc, Cc)).to(dev)) for k in (3, 7, 11)[:n]]
        return x, outs, [(w, None, o, k) for w, o, k in zip(wpws, outs, (3, 7, 11))]

    # C = 128: four chunks, declined without a launch
    x, outs, br = problem(128)
    assert hipops.conv1d_wino_fan(x, br, dil=1, slope=SLOPE) is False
    # per-item lengths: not served
    x, outs2, br = problem(64)
    assert hipops.conv1d_wino_fan(x, br, dil=1, slope=SLOPE, lengths=torch.full((B,), 100, dtype=torch.int32, device=dev), len_mul=1) is False
    torch.cuda.synchronize()
    assert all(bool((o == SENT).all()) for o in outs + outs2)
    # problems that do not share `in` / the dilation: an argument error
    x2 = x.clone()
    for other in (dict(x=x2, dil=1), dict(x=x, dil=3)):
        arr = (_hip.Conv1dArgs * 2)()
        hipops._conv1d_args(arr[0], x, None, None, outs2[0], k=3, dil=1, slope=SLOPE, algo=hipops.ALGO_WINO, wp=br[0][0])
        hipops._conv1d_args(arr[1], other['x'], None, None, outs2[1], k=7, dil=other['dil'], slope=SLOPE, algo=hipops.ALGO_WINO, wp=br[1][0])
        assert _hip.load().v2w_conv1d_wino_fan_fwd(arr, 2, hipops._stream(x)) == -1
    torch.cuda.synchronize()
    assert all(bool((o == SENT).all()) for o in outs2)


def test_generator_forward_is_bitwise_the_same_with_and_without_the_fan(dev):
    """B = 2, T = 8, train mode, two modules from one state dict: `wino_fan = (64,)` against `()`.  The planner tags the merged launch once;
    at this size the one-conv Winograd launch is below the library's size rule, so the fan declines as well and both run today's launches."""
    from wavthruvec_pytorch_amd import Generator, synthetic
    h = synthetic.make_hparams(num_wv_feat=768)
    sd = synthetic.make_state_dict(h, seed=5)
    inp = tuple(t.to(dev) for t in synthetic.make_inputs(h, 2, 8, seed=9))
    ys, tags = {}, {}
    for fan in ((64,), ()):
        g = Generator(h)
        g.load_state_dict(sd)
        g = g.to(dev).train()
        g.wino_fan = fan
        g._profile = []
        with torch.no_grad():
            ys[fan] = g(*inp)
        torch.cuda.synchronize()
        tags[fan] = [t for t, _e0, _e1 in g._profile]
        g._profile = None
    nk = 3
    i64 = [i for i, up in enumerate(Generator(h).ups) if up.out_channels == 64][0]
    merged = 'bconv0:' + '+'.join(f'resblocks.{i64 * nk + j}.0' for j in range(nk))
    assert merged == 'bconv0:resblocks.6.0+resblocks.7.0+resblocks.8.0'
    assert tags[(64,)].count(merged) == 1 and merged not in tags[()]
    assert torch.equal(ys[(64,)], ys[()])


def test_generator_forward_with_the_fan_launch_taken(dev):
    """B = 8, T = 32: the 64-channel stage's first convs pass the size rule (3 x 8 x 20 workgroups), the fan launch runs
    (conv_wino_fan_kernel behind the merged tag) and the forward is bit-identical to the one with `wino_fan = ()`."""
    from wavthruvec_pytorch_amd import Generator, synthetic
    h = synthetic.make_hparams(num_wv_feat=768)
    sd = synthetic.make_state_dict(h, seed=5)
    inp = tuple(t.to(dev) for t in synthetic.make_inputs(h, 8, 32, seed=9))
    ys = {}
    for fan in ((64,), ()):
        g = Generator(h)
        g.load_state_dict(sd)
        g = g.to(dev).train()
        g.wino_fan = fan
        with torch.no_grad():
            ys[fan] = g(*inp)
        if fan:
            g.eval()        # (the name probe runs one more forward: keep the module's statistics out of it)
            names = g.profile_kernel_names(*inp)
            assert names['bconv0:resblocks.6.0+resblocks.7.0+resblocks.8.0'] == ['conv_wino_fan_kernel<1, 2, 3, true>'], names
    assert torch.equal(ys[(64,)], ys[()])
