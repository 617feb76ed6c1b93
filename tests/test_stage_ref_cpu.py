"""tests/stage_ref.py pinned against independent statements of the same operations (F.conv1d and autograd in float64, trimmed single items),
the Winograd magnitude sum against the direct one, and the dispatch table of the fused narrow-stage kernel tests (tests/stage_cases.py through
the name sink: which kernel every GPU record launches, and its return code).  No GPU needed."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import disc_ref as D
from tests import stage_cases as K
from tests import stage_ref as R
from tests import tile_ref
from tests.test_disc_ref_cpu import _close, _rnd

SLOPE = float(np.float32(0.1))


def _lr(v, slope=SLOPE):
    return F.leaky_relu(v, float(np.float32(slope)))


def _conv(x, wf, b, d):
    return F.conv1d(x, D.wf_to_w(wf), b, padding=d * (wf.shape[0] - 1) // 2, dilation=d)


def _branches(seed, Cc, brs, bias=True):
    out = []
    for j, (k, d1, d2) in enumerate(brs):
        s = seed + 10 * j
        out.append(dict(w1=_rnd(s, k, Cc, Cc) / np.sqrt(Cc * k), w2=_rnd(s + 1, k, Cc, Cc) / np.sqrt(Cc * k),
                        b1=_rnd(s + 2, Cc) if bias else None, b2=_rnd(s + 3, Cc) if bias else None, d1=d1, d2=d2))
    return out


def _section(x, brs, div):
    tot = None
    for br in brs:
        t1 = x + _conv(_lr(x), br['w1'], br['b1'], br['d1'])
        r = t1 + _conv(_lr(t1), br['w2'], br['b2'], br['d2'])
        tot = r if tot is None else tot + r
    return tot / div if div else tot


BRS = ((3, 1, 3), (7, 2, 3), (11, 1, 1))


@pytest.mark.parametrize('wino', [False, True])
@pytest.mark.parametrize('div', [0.0, 3.0])
def test_section_is_f_conv1d_through_the_branches(wino, div):
    B, Cc, L = 2, 4, 70
    x_in, a, s = _rnd(1, B, Cc, L), _rnd(2, B, Cc), _rnd(3, B, Cc)
    brs = _branches(100, Cc, BRS)
    n = [40] * 3
    got, E = R.section(x_in, brs, n, n, slope=0.1, in_a=a, in_s=s, out_div=div, wino=wino)
    _close(got, _section(a[:, :, None] * x_in + s[:, :, None], brs, div))
    assert (E > 0).all() and E.shape == got.shape
    # without the affine and the biases; one branch
    one = _branches(200, Cc, BRS[:1], bias=False)
    _close(R.section(x_in, one, n, n, slope=0.1, wino=wino)[0], _section(x_in, one, 0.0))


def test_the_bound_is_the_two_phase_propagation():
    """One branch, hand-made: E(r) = E1 + taps_sum(E1, |w2|) + n2 eps S2 with E1 = n1 eps S1, then the division."""
    B, Cc, L, k, d1, d2 = 1, 3, 30, 3, 1, 2
    x = _rnd(4, B, Cc, L)
    br = _branches(300, Cc, ((k, d1, d2),))[0]
    n1, n2 = 17, 23
    _, E = R.section(x, [br], [n1], [n2], slope=0.1, out_div=3.0)
    ax = _lr(x)
    S1 = x.abs() + _conv(ax.abs(), br['w1'].abs(), br['b1'].abs(), d1)
    t1 = x + _conv(ax, br['w1'], br['b1'], d1)
    E1 = n1 * D.U * S1
    S2 = t1.abs() + _conv(_lr(t1).abs(), br['w2'].abs(), br['b2'].abs(), d2)
    r = t1 + _conv(_lr(t1), br['w2'], br['b2'], d2)
    Er = E1 + _conv(E1, br['w2'].abs(), None, d2) + n2 * D.U * S2
    _close(E, Er / 3.0 + D.U * (r / 3.0).abs(), 1e-9)


@pytest.mark.parametrize('mode', [0, 1])
def test_pair_is_two_chained_convs_with_the_addends(mode):
    B, Cc, L, k, d1, d2 = 2, 4, 50, 7, 1, 3
    x_in, a, s, a0, a1 = _rnd(5, B, Cc, L), _rnd(6, B, Cc), _rnd(7, B, Cc), _rnd(8, B, Cc, L), _rnd(9, B, Cc, L)
    br = _branches(400, Cc, ((k, d1, d2),))[0]
    x = a[:, :, None] * x_in + s[:, :, None]
    c1 = _conv(_lr(x), br['w1'], br['b1'], d1)
    t1 = x + c1 if mode == 0 else c1
    r = (t1 if mode == 0 else x) + _conv(_lr(t1), br['w2'], br['b2'], d2)
    got, E = R.pair(x_in, br, 30, 30, 2, slope=0.1, res_mode=mode, in_a=a, in_s=s, add0=a0, add1=a1, out_div=3.0)
    _close(got, ((a0 + a1) + r) / 3.0)
    assert (E > 0).all()
    _close(R.pair(x_in, br, 30, 30, 1, slope=0.1, res_mode=mode, add0=a0)[0], a0 + _pair_plain(x_in, br, mode))
    _close(R.pair(x_in, br, 30, 30, 0, slope=0.1, res_mode=mode)[0], _pair_plain(x_in, br, mode))


def _pair_plain(x, br, mode):
    c1 = _conv(_lr(x), br['w1'], br['b1'], br['d1'])
    t1 = x + c1 if mode == 0 else c1
    return (t1 if mode == 0 else x) + _conv(_lr(t1), br['w2'], br['b2'], br['d2'])


@pytest.mark.parametrize('post_k,bias', [(1, True), (3, False), (7, True), (9, True)])
def test_tail_is_tanh_of_conv_post(post_k, bias):
    B, Cc, L = 2, 4, 40
    out, E_out = _rnd(10, B, Cc, L), _rnd(11, B, Cc, L).abs() * 1e-6
    pw, pb = _rnd(12, post_k, Cc, 1), (_rnd(13, 1) if bias else None)
    got, E, arg = R.tail(out, E_out, pw, pb, 33, post_slope=0.01)
    want = torch.tanh(F.conv1d(_lr(out, 0.01), D.wf_to_w(pw), pb, padding=(post_k - 1) // 2))
    assert got.shape == (B, 1, L)
    _close(got, want)
    _close(arg, torch.atanh(want), 1e-9)
    mag = F.conv1d(_lr(out, 0.01).abs(), D.wf_to_w(pw).abs(), None if pb is None else pb.abs(), padding=(post_k - 1) // 2)
    _close(E, F.conv1d(E_out, D.wf_to_w(pw).abs(), padding=(post_k - 1) // 2) + 33 * D.U * mag + R.TANH_C * D.U, 1e-9)
    # with lengths: the operand is zero at and past the item's end, and so is the result
    ends = [13, L]
    nan_out = tile_ref.unspecified_past(out, ends)
    gl, El, _ = R.tail(nan_out, tile_ref.unspecified_past(E_out, ends), pw, pb, 33, post_slope=0.01, ends=ends)
    assert (gl[0, :, 13:] == 0).all() and (El[0, :, 13:] == 0).all()
    _close(gl[0:1, :, :13], R.tail(out[0:1, :, :13].contiguous(), E_out[0:1, :, :13].contiguous(), pw, pb, 33, post_slope=0.01)[0])
    _close(gl[1], got[1], 0.0)


@pytest.mark.parametrize('aff', [True, False])
def test_gradient_form_is_autograd_through_the_section(aff):
    """The forward section in float64 with autograd; the gradient form fed with the transposed, tap-reversed weights of conv2_j / conv1_j and
    the swapped dilations, bwd_mask1[j] = t1_j, bwd_mask2 = xr (x = a xr + s), in = dL/d(out), in_a = 1 / nk."""
    B, Cc, L, nk = 2, 4, 60, 3
    xr, a, s, dout = _rnd(14, B, Cc, L), _rnd(15, B, Cc), _rnd(16, B, Cc), _rnd(17, B, Cc, L)
    if not aff:
        a, s = torch.ones_like(a), torch.zeros_like(s)
    brs = _branches(500, Cc, BRS, bias=False)
    x = (a[:, :, None] * xr + s[:, :, None]).requires_grad_(True)
    t1s, tot = [], None
    for br in brs:
        t1 = x + _conv(_lr(x), br['w1'], None, br['d1'])
        t1.retain_grad()
        r = t1 + _conv(_lr(t1), br['w2'], None, br['d2'])
        tot = r if tot is None else tot + r
        t1s.append(t1)
    (tot / nk).backward(dout)
    gbr = [dict(w1=D.transpose_flip(br['w2']), d1=br['d2'], w2=D.transpose_flip(br['w1']), d2=br['d1']) for br in brs]
    inv, zero = torch.full((B, Cc), 1.0 / nk, dtype=torch.float64), torch.zeros(B, Cc, dtype=torch.float64)
    n = [20] * nk
    got, E, mids = R.section_bwd(dout, gbr, [t.detach() for t in t1s], n, n, mask2=xr, mask2_a=a if aff else None, mask2_s=s if aff else None,
                                 bwd_slope=0.1, in_a=inv, in_s=zero)
    _close(got, x.grad, 1e-10)
    for (t1g, E1), t1 in zip(mids, t1s):
        _close(t1g, t1.grad, 1e-10)
        assert (E1 > 0).all()
    assert (E > 0).all()


def test_lengths_are_each_items_own_unpadded_call():
    B, Cc, L = 3, 4, 50
    x_in, a, s = _rnd(18, B, Cc, L), _rnd(19, B, Cc), _rnd(20, B, Cc)
    brs = _branches(600, Cc, BRS)
    ends = [0, 17, 50]
    xn = x_in.clone()
    for b, e in enumerate(ends):
        xn[b, :, e:] = float('nan')                                   # whatever the tensor holds there
    n = [40] * 3
    for wino in (False, True):
        got, E = R.section(xn, brs, n, n, slope=0.1, in_a=a, in_s=s, out_div=3.0, ends=ends, wino=wino)
        for b, e in enumerate(ends):
            assert torch.isnan(got[b, :, e:]).all() and torch.isnan(E[b, :, e:]).all()
            if e:
                alone, Ea = R.section(x_in[b:b + 1, :, :e].contiguous(), brs, n, n, slope=0.1, in_a=a[b:b + 1], in_s=s[b:b + 1], out_div=3.0, wino=wino)
                _close(got[b:b + 1, :, :e], alone)
                _close(E[b:b + 1, :, :e], Ea, 1e-9)


@pytest.mark.parametrize('k,dil', [(3, 1), (3, 3), (7, 1), (7, 3), (11, 1), (11, 3), (5, 2)])
def test_the_winograd_magnitude_sum_covers_the_direct_one_and_the_value(k, dil):
    B, Cc, L = 2, 5, 45
    act, wf = _rnd(21, B, Cc, L), _rnd(22, k, Cc, Cc)
    z, S = tile_ref.taps_sum(act, wf, dil, dil * (k - 1) // 2)
    Sw = R.wino_mag(act, wf, dil)
    assert (Sw >= S * (1 - 1e-12)).all() and (Sw >= z.abs()).all() and (Sw <= 4 * S + 1e-12).any()
    # the value of the Winograd form itself (tests/wino_ref.py) is the direct conv
    from tests import wino_ref
    _close(wino_ref.conv1d(act, D.wf_to_w(wf), None, dilation=dil), z, 1e-10)
    assert R.phase(act, wf, dil, wino=True)[1] is not None and torch.equal(R.phase(act, wf, dil)[1], S)


def test_the_mask_redraw_ends():
    """_draw_mask of the GPU tests (|a m + s| >= 2^-10, offenders redrawn on the CPU) on the largest gradient-form record: it ends, and no
    entry is left to exclude."""
    from tests.test_tile_kernels_gpu import MASK_MIN, _draw_mask, _f32
    rng = np.random.default_rng(3)
    B, Cc, L = 112, 32, 228
    a, s = _f32(rng, B, Cc, scale=0.5) + 1.0, _f32(rng, B, Cc, scale=0.5)
    m = _draw_mask(rng, B, Cc, L, a, s)
    assert ((D.f64(a)[:, :, None] * D.f64(m) + D.f64(s)[:, :, None]).abs() >= MASK_MIN).all()
    m0 = _draw_mask(rng, 2, 16, 100, None, None)
    assert (m0 == 0).sum() >= 6 and torch.signbit(m0.view(-1)[1])


# ---------------------------------------------------------------------------------------------------------------
# the dispatch table: one row per GPU record
ROWS = [(g, c) for g, cases in K.TABLE.items() for c in cases]


@pytest.mark.parametrize('group,c', ROWS, ids=['%s-%s' % (g, c['id']) for g, c in ROWS])
def test_dispatch_of_every_gpu_record(group, c):
    rc, names = K.dispatch(c)
    print(group, c['id'], rc, names)
    assert (rc, names) == (c['rc'], c['kernels']), (rc, names)


def test_the_table_reaches_every_instantiation():
    seen = {n for c in K.EVERY for n in c['kernels']}
    assert [n for n in K.INSTANTIATIONS if n not in seen] == []


def test_the_table_reaches_every_branch():
    # what the names cannot show: the window rule at its threshold, the seams, the scalar paths, the chain lengths
    std = K.geometry('direct', 1, 100, K.STD)
    assert (std['nto'], K.geometry('direct', 112, 228, K.STD)['nto']) == (96, 224)
    assert (K.geometry('direct', 1, 100, K.STD, 7)['nadv'], K.geometry('direct', 112, 228, K.STD, 7)['nadv']) == (88, 216)
    for c in K.LENGTHS:
        if c['id'].endswith('takes_256'):
            assert c['B'] * D.ceil_div(c['L'], 224) == 224 and c['W'] == 256
        if c['id'].endswith('stays_on_128'):
            assert c['B'] * D.ceil_div(c['L'], 224) == 222 and c['W'] == 128
    for v, _ in K.VARIANTS:
        for W in (128, 256):
            Ls = sorted(c['L'] for c in K.LENGTHS if c['id'].startswith('%s_w%d_L' % (v, W)))
            step = next(c for c in K.LENGTHS if c['id'].startswith('%s_w%d_L' % (v, W)))['geom']['nadv']
            assert Ls == sorted((1, 4, 5, step - 1, step, step + 1, step + 4, 2 * step + 4, step + 7)), (v, W)
    for c in K.ALIGN:
        assert len(c['offs']) == 1 and c['L'] % 4 == 0
    for c in K.LENS:
        ends = [e * c['len_mul'] for e in c['lens']]
        step = c['geom']['nadv']
        assert 0 in ends and 1 in c['lens'] and any(e > c['L'] for e in ends) and c['L'] in ends, c['id']
        assert any(0 < e < c['L'] and e % step == 0 for e in ends) and any(0 < e < c['L'] and e % step for e in ends), c['id']
    assert {K.halos(c['br'])[0] for c in K.BRANCHES} >= {32} and {(c['W'], K.halos(c['br'])[1]) for c in K.BRANCHES} >= {(128, 32), (256, 64)}
    assert {len(c['br']) for c in K.BRANCHES} >= {1, 3, 4} and {c['post_k'] for c in K.BRANCHES} >= {1, 3, 7, 9}
    assert {(c['bwd']['aff'], c['bwd']['rowsum']) for c in K.GRAD} == {(a, r) for a in (True, False) for r in (True, False)}
    assert {(c['res_mode'], len(c['ks']), c['adds']) for c in K.PAIR} >= {(m, n, a) for m in (0, 1) for n, a in ((1, 2), (4, 1), (1, 0))}
    for c in K.EVERY:
        Cc = c['C']
        ks = c['ks'] if c['op'] == 'pair' else [k for k, _, _ in c['br']]
        prods = [(len(K.segments(k)) * Cc + 5) if c['form'] == 'wino' else k * Cc for k in ks]
        assert c['n1'] == tuple(p + c['ops'][0] for p in prods) and c['n2'] == tuple(p + c['ops'][1] for p in prods), c['id']
    codes = {c['id']: c['rc'] for c in K.REFUSALS}
    assert all(rc in (K.E_ARG, K.E_SHAPE) for rc in codes.values())
    assert [i for i, rc in codes.items() if rc == K.E_ARG] == ['grad_with_bias', 'grad_with_slope', 'grad_with_lens', 'grad_with_tail', 'len_mul0']


def test_bwd_rows_is_four_rows_per_tile():
    for c in K.GRAD:
        assert K.bwd_rows(c) == c['B'] * c['geom']['ntl'] * 4, c['id']
