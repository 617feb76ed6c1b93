"""GPU tests of the Winograd F(2,3) Conv1d kernel (csrc/v2w_conv_wino.hip) at the partial last tile of a row: a column-wave (32 output pairs)
whose first output position lies at or past the end of the sequence runs no matrix work and stores nothing, and the partial tail tiles of a
problem take its last workgroups.  Dilation 3 at C_in = 64 -> C_out = 128, B = 8 (more than 128 workgroups, or the kernel declines the
launch), every k of the generator with the epilogues its second convs use, against ALGO_DIRECT with the bound of tests/test_wino_gpu.py
applied to every entry; the per-item-length entry point (v2w_conv1d_fwd_len) with item ends inside, on and behind a wave boundary."""
import ctypes as C_

import numpy as np
import pytest
import torch

from tests import wino_ref

pytestmark = pytest.mark.gpu

B, CI, CO = 8, 64, 128
NTP = 64          # output pairs of a tile; a column-wave owns 32 of them
SENTINEL = -7.0e30


def tpos(P, d):
    """First output position of pair P (wino_tpos): the pair is (t, t + d)."""
    return 2 * d * (P // d) + P % d


def npairs(L, d):
    return d * ((L + 2 * d - 1) // (2 * d))


def tail_live_pairs(L, d):
    """Pairs of the row's last tile with a first output below L (0: the row's pairs fill their tiles)."""
    n = npairs(L, d)
    if n % NTP == 0:
        return 0
    return sum(1 for P in range(n // NTP * NTP, n) if tpos(P, d) < L)


def workgroups(L, d, co=CO, b=B):
    return b * ((npairs(L, d) + NTP - 1) // NTP) * (co // 64)


# (L, dilation, live pairs of the tail tile).  1280: pair 640 alone, a single (1279 + 3 >= L; pair 641 starts at L).  1284: pairs 640 and 641 whole.
# 1341 / 1344: exactly 32 - the second column-wave is dead with the first one full (1341: scalar staging, the last pairs singles); at
# 1344 = 21 * 64 the 672 pairs are 10.5 tiles.  1345: 33 - the second wave is live with ONE column; 1348: with three, float4 staging.
# 1152 (dilation 3) and 1280 (dilation 1): the pairs fill their tiles - the item-major tile map.
TAIL_CASES = [(1280, 3, 1), (1284, 3, 2), (1341, 3, 32), (1344, 3, 32), (1345, 3, 33), (1348, 3, 35), (1152, 3, 0), (1280, 1, 0)]

# the epilogues of the generator's second convs (forward_plan.residual...): every branch adds its input back (res); the last of nk branches
# adds the other branches' outputs and divides by nk
EPILOGUES = {3: 'res', 7: 'res+add0+div', 11: 'res+add0+add1+div'}


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a MI355X'
    from wavthruvec_pytorch_amd import _hip
    _hip.load()
    return torch.device('cuda:0')


def _rand(r, shape, scale=1.0):
    return torch.from_numpy((scale * r.standard_normal(shape)).astype(np.float32))


def _guarded(shape, dev, guard=4096):
    """A sentinel-filled flat buffer and the (B, C, L) view in its middle: whatever the kernel leaves alone keeps the sentinel."""
    n = int(np.prod(shape))
    flat = torch.full((n + 2 * guard,), SENTINEL, device=dev)
    return flat, flat[guard:guard + n].view(shape)


def _guards_intact(flat, shape, guard=4096):
    n = int(np.prod(shape))
    return bool((flat[:guard] == SENTINEL).all()) and bool((flat[guard + n:] == SENTINEL).all())


def _problem(rng, dev, L, k, epilogue):
    x = _rand(rng, (B, CI, L)).to(dev)
    wf = _rand(rng, (k, CI, CO), 1 / np.sqrt(CI * k)).to(dev)
    bias = _rand(rng, (CO,)).to(dev)
    kw = dict(k=k, slope=0.1, res=_rand(rng, (B, CO, L)).to(dev))
    nadd = epilogue.count('add')
    if nadd:
        kw.update(add=[_rand(rng, (B, CO, L)).to(dev) for _ in range(nadd)], out_div=float(nadd + 1))
    return x, wf, bias, kw


def _run_wino(x, bias, out, wpw, lengths=None, **kw):
    """The Winograd kernel itself: a declined launch raises (no weights of the direct form are handed over)."""
    from wavthruvec_pytorch_amd import _hip, hipops
    a = _hip.Conv1dArgs()
    hipops._conv1d_args(a, x, None, bias, out, algo=hipops.ALGO_WINO, wp=wpw, **kw)
    if lengths is None:
        _hip.check(_hip.load().v2w_conv1d_fwd(C_.byref(a), hipops._stream(x)), 'v2w_conv1d_fwd')
    else:
        _hip.check(_hip.load().v2w_conv1d_fwd_len(C_.byref(a), 1, hipops._len_ptr(lengths, 1), 1, hipops._stream(x)), 'v2w_conv1d_fwd_len')


def _assert_entries(got, want, what):
    """test_wino_gpu's bound, 2e-5 max(1, max |direct|), on every entry (an entry left at the sentinel or NaN fails it)."""
    bound = 2e-5 * max(1.0, want.abs().max().item())
    err = (got - want).abs()
    bad = ~(err <= bound)
    print(f'{what}: max err {err[~bad].max().item() if (~bad).any() else float("nan"):.3e}  bound {bound:.3e}  entries over {int(bad.sum())}')
    assert not bad.any(), (what, int(bad.sum()), bad.nonzero()[:4].tolist())


@pytest.mark.parametrize('k', [3, 7, 11])
@pytest.mark.parametrize('L,dil,live', TAIL_CASES)
def test_tail_tile_matches_direct(dev, L, dil, live, k):
    from wavthruvec_pytorch_amd import hipops
    assert workgroups(L, dil) > 128
    rng = np.random.default_rng(100 * L + 10 * k + dil)
    x, wf, bias, kw = _problem(rng, dev, L, k, EPILOGUES[k])
    kw['dil'] = dil
    flat, o_w = _guarded((B, CO, L), dev)
    o_d = torch.empty((B, CO, L), device=dev)
    _run_wino(x, bias, o_w, hipops.pack_wino(wf), **kw)
    hipops.conv1d(x, wf, bias, o_d, algo=hipops.ALGO_DIRECT, **kw)
    torch.cuda.synchronize()
    _assert_entries(o_w, o_d, f'L={L} dil={dil} k={k} {EPILOGUES[k]}')
    assert _guards_intact(flat, (B, CO, L)), 'stored outside the output tensor'


def test_tail_tiles_of_a_multi_problem_launch(dev):
    """k = 7 and k = 3 in one launch, as the generator launches a stage's dilation-3 convs: either problem's tail tiles close ITS block range."""
    from wavthruvec_pytorch_amd import _hip, hipops
    L, dil = 1280, 3
    rng = np.random.default_rng(77)
    x = _rand(rng, (B, CI, L)).to(dev)
    arr = (_hip.Conv1dArgs * 2)()
    keep, outs = [], []
    for a, k in zip(arr, (7, 3)):
        _x, wf, bias, kw = _problem(rng, dev, L, k, 'res')
        kw['dil'] = dil
        flat, o_w = _guarded((B, CO, L), dev)
        o_d = torch.empty((B, CO, L), device=dev)
        wpw = hipops.pack_wino(wf)
        hipops._conv1d_args(a, x, None, bias, o_w, algo=hipops.ALGO_WINO, wp=wpw, **kw)
        hipops.conv1d(x, wf, bias, o_d, algo=hipops.ALGO_DIRECT, **kw)
        keep.append((wf, bias, kw, wpw))
        outs.append((k, flat, o_w, o_d))
    _hip.check(_hip.load().v2w_conv1d_fwd_multi(arr, 2, hipops._stream(x)), 'v2w_conv1d_fwd_multi')
    torch.cuda.synchronize()
    for k, flat, o_w, o_d in outs:
        _assert_entries(o_w, o_d, f'multi k={k}')
        assert _guards_intact(flat, (B, CO, L))


# Item ends (dilation 3, tile 5 = pairs 320..383 starts at position 638, its second column-wave at pair 352 = position 703):
# 660 inside the first wave; 703 on the wave boundary (pair 351 = position 702 is the last live first output: the second wave is dead);
# 704 one live column in the second wave; 720 inside it; 638 the tile starts at the end (it returns); 639 one live column in the tile;
# 1280 the whole row, with the row's own tail tile; 2000 clamped to L.
LEN_ENDS = [660, 703, 704, 720, 638, 639, 1280, 2000]


@pytest.mark.parametrize('k', [3, 7, 11])
def test_len_entry_point_item_ends_at_the_wave_boundary(dev, k):
    from wavthruvec_pytorch_amd import hipops
    L, dil = 1280, 3
    assert tpos(5 * NTP, dil) == 638 and tpos(5 * NTP + 32, dil) == 703 and tpos(5 * NTP + 31, dil) == 702 and len(LEN_ENDS) == B
    rng = np.random.default_rng(900 + k)
    x, wf, bias, kw = _problem(rng, dev, L, k, EPILOGUES[k])
    kw['dil'] = dil
    ends = [min(e, L) for e in LEN_ENDS]
    x_nan, x_zero = x.clone(), x.clone()
    for b, e in enumerate(ends):
        x_nan[b, :, e:] = float('nan')
        x_zero[b, :, e:] = 0.0            # (no input affine: leaky_relu(0) = 0, the zero the kernel selects past the end)
    flat, o_w = _guarded((B, CO, L), dev)
    o_d = torch.empty((B, CO, L), device=dev)
    _run_wino(x_nan, bias, o_w, hipops.pack_wino(wf), lengths=torch.tensor(LEN_ENDS, dtype=torch.int32, device=dev), **kw)
    hipops.conv1d(x_zero, wf, bias, o_d, algo=hipops.ALGO_DIRECT, **kw)
    torch.cuda.synchronize()
    for b, e in enumerate(ends):          # outputs at and past an item's end are unspecified: take the reference's there
        o_w[b, :, e:] = o_d[b, :, e:]
    _assert_entries(o_w, o_d, f'len k={k}')
    assert _guards_intact(flat, (B, CO, L))


def test_wino_ref_agrees_at_the_tail(dev):
    """tests/wino_ref.py's Winograd scheme in fp64 against the kernel on one tail-tile row (L = 1280, k = 11, no epilogue operands):
    the same per-entry bound."""
    from wavthruvec_pytorch_amd import hipops
    L, k, dil = 1280, 11, 3
    rng = np.random.default_rng(5)
    x = _rand(rng, (B, CI, L))
    wf = _rand(rng, (k, CI, CO), 1 / np.sqrt(CI * k))
    bias = _rand(rng, (CO,))
    want = wino_ref.conv1d(torch.nn.functional.leaky_relu(x, 0.1).double(), wf.permute(2, 1, 0).double(), bias.double(), dilation=dil)
    flat, o_w = _guarded((B, CO, L), dev)
    _run_wino(x.to(dev), bias.to(dev), o_w, hipops.pack_wino(wf.to(dev)), k=k, dil=dil, slope=0.1)
    torch.cuda.synchronize()
    _assert_entries(o_w.cpu().double(), want, 'wino_ref fp64')
    assert _guards_intact(flat, (B, CO, L))
