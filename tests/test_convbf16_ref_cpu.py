"""tests/convbf16_ref.py pinned against independent statements (F.conv1d / F.conv_transpose1d in fp64 on the rounded operands, the packer
decoded back to the transposed conv), the dispatch table of tests/convbf16_cases.py (configuration query and name sink: which
conv_bf16_kernel instantiation every GPU record launches, and its return code), the coverage of every template tuple the dispatchers can
return, the termination of the operand redraw, and three wrong kernels stated in fp64 that every record they apply to must see (at least
one entry past its bound, and a stated fraction where the arithmetic allows one).  No GPU needed.

The reference does not depend on the batch, so the value checks run on at most eight items of a record (evenly spread: a short-chain
record keeps eight different live channels)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import convbf16_cases as K
from tests import convbf16_ref as R
from tests import disc_ref as D
from tests import split_ref
from tests import tile_ref
from tests.test_disc_ref_cpu import _close

RUN = [c for c in K.CONV_ALL if c['rc'] == K.OK and c['inst'] is not None]
TILES = K.TILES


def _items(c, o, i=0):
    """(x, wf, keyword arguments) of problem i on at most eight items of the batch."""
    sel = torch.arange(0, c['B'], max(1, c['B'] // 8))[:8]
    kw = {q: (v[sel] if isinstance(v, torch.Tensor) and v.dim() >= 2 and v.shape[0] == c['B'] else v) for q, v in K.ref_kwargs(c, o).items()}
    return o['t']['x'][sel], o['t']['wf'], kw


def _independent(c, x, wf, kw):
    """The call's value from F.conv1d on the rounded operands and the header's formula, in fp64."""
    k, dil = wf.shape[0], kw['dil']
    left = kw['pad_left'] if kw['pad_left'] >= 0 else dil * (k - 1) // 2
    t = x.float()
    if 'in_a' in kw:
        t = (kw['in_a'].double()[:, :, None] * t.double() + kw['in_s'].double()[:, :, None]).float()
    if kw['slope'] != 1.0:
        t = torch.where(t > 0, t, t * float(np.float32(kw['slope'])))
    act = t.bfloat16().double()
    z = F.conv1d(F.pad(act, (left, (k - 1) * dil - left)), D.wf_to_w(wf.bfloat16().double()), dilation=dil)
    if 'mask_src' in kw:
        arg = kw['mask_src'].double()
        if 'mask_a' in kw:
            arg = kw['mask_a'].double()[:, :, None] * arg + kw['mask_s'].double()[:, :, None]
        z = torch.where(arg > 0, z, z * float(np.float32(kw['mask_slope'])))
    if 'bias' in kw:
        z = z + kw['bias'].double()[None, :, None]
    if 'res' in kw:
        r = kw['res'].double()
        z = z + (r if 'res_a' not in kw else kw['res_a'].double()[:, :, None] * r + kw['res_s'].double()[:, :, None])
    if 'add0' in kw:
        z = (kw['add0'].double() + (kw['add1'].double() if 'add1' in kw else 0.0)) + z
    if 'old' in kw:
        z = kw['old'].double() + z
    return z / float(np.float32(kw['out_div'])) if kw['out_div'] else z


@pytest.mark.parametrize('c', RUN, ids=K.ids(RUN))
def test_the_reference_is_f_conv1d_on_the_rounded_operands_and_the_redraw_terminates(c):
    for i in range(len(c['ks'])):
        o = K.operands(c, i)                                     # (asserts that no ambiguous element is left after at most 64 rounds)
        x, io = o['t']['x'], c['io']
        if 'in_aff' in c['flags']:
            assert not R.ambiguous(x, c['slope'], o['ref']['in_a'], o['ref']['in_s']).any() and o['rounds'] <= 64
            print('[redraw] %s: %d rounds' % (c['id'], o['rounds']))
        if io & 1:
            assert torch.equal(x, R.rne_bf16(x))
        if io & 2:
            assert all(torch.equal(o['ref'][q], R.rne_bf16(o['ref'][q])) for q in ('res', 'add0', 'add1', 'old') if q in o['ref'])
        if c['short']:
            live = (x != 0).any(2)
            assert (live.sum(1) == 1).all() and len({int(v) for v in live.float().argmax(1)}) == min(c['B'], c['ci'])
            if c['ci'] > c['B']:
                ch = {K.live_channel(c, b) for b in range(c['B'])}
                assert {v % 64 for v in ch} == set(range(64)) and {v // 64 for v in ch} == set(range(c['ci'] // 64))
        xs, wf, kw = _items(c, o, i)
        want, bound = R.conv1d(xs, wf, c['n'][i], **kw)
        _close(want, _independent(c, xs, wf, kw), 1e-12)
        assert torch.isfinite(bound).all() and (bound >= 0).all()


def test_the_redraw_sees_and_removes_an_element_on_a_rounding_boundary():
    a, s = torch.full((1, 1), 1.0), torch.full((1, 1), 2.0 ** -30)
    x = torch.tensor([[[1.00390625, 0.7]]])                      # 1 + 2^-8: halfway between two bf16 numbers; + 2^-30 moves the fma across
    assert R.ambiguous(x, 1.0, a, s).tolist() == [[[True, False]]]
    y, rounds = R.redraw(x, 1.0, a, s, lambda n: torch.full((n,), 0.3))
    assert rounds == 1 and y.tolist() == [[[pytest.approx(0.3), pytest.approx(0.7)]]]
    with pytest.raises(AssertionError):
        R.redraw(x, 1.0, a, s, lambda n: torch.full((n,), 1.00390625))


def test_the_store_interval():
    want = torch.tensor([1.0, 1.00390625, 1.0039, -3.0, 2.0], dtype=torch.float64)
    lo, hi = R.store_interval(want, torch.full_like(want, 1e-6))
    assert lo.tolist() == [1.0, 1.0, 1.0, -3.0, 2.0] and hi.tolist() == [1.0, 1.0078125, 1.0, -3.0, 2.0]
    r = R.check_store(torch.tensor([1.0, 1.0078125, 1.0, -3.0, 2.0]), want, torch.full_like(want, 1e-6))
    assert r['outside'] == 0 and r['ratio'] <= 1 and (r['single'], r['lower'], r['upper']) == (4, 0, 1)
    r = R.check_store(torch.tensor([1.0078125, 1.0, 1.0078125, -3.015625, 2.0]), want, torch.full_like(want, 1e-6))
    assert r['outside'] == 3 and r['ratio'] > 1
    lo, hi = R.bf16_cell(torch.tensor([1.0, -1.0, 0.0]))
    assert lo.tolist() == [1 - 2.0 ** -9, -1 - 2.0 ** -8, -2.0 ** -134] and hi.tolist() == [1 + 2.0 ** -8, -1 + 2.0 ** -9, 2.0 ** -134]


# ---------------------------------------------------------------------------------------------------------------
# three wrong kernels, in fp64
def _seen(name, c, diff, bound, where, need):
    d = diff.abs()
    live = where & (d > 0)
    seen = live & (d > bound)
    print('[power] %s %s: exceeds the bound on %d of %d affected entries, worst %.3g bounds'
          % (name, c['id'], int(seen.sum()), int(live.sum()), float((d / bound)[live].max()) if bool(live.any()) else 0.0))
    assert int(live.sum()) > 0 and int(seen.sum()) >= max(1, need * int(live.sum())), (name, c['id'])


@pytest.mark.parametrize('c', TILES, ids=K.ids(TILES))
def test_the_records_see_three_wrong_kernels(c):
    o = K.operands(c)
    x, wf, kw = _items(c, o)
    n, k, dil = c['n'][0], c['ks'][0], c['dil']
    want, bound = R.conv1d(x, wf, n, **kw)
    every = torch.ones_like(want, dtype=torch.bool)
    # (a) the operand truncated to bf16, not rounded to nearest even.  Every record, dense ones included, must have an entry past its bound
    # (one such entry fails a GPU record); nine in ten of the live entries of a short-chain record; half of the entries of a dense record
    # with k <= 3, or with an fp32-stored input and k C_in <= 1024.  Beyond that the bound n 2^-24 S grows faster than the truncation's
    # drift, and a bf16-stored input is exact where it is positive (only the negative half, a tenth as large after the slope, is
    # rounded at all): fewer entries show it - 0.6 % at C_in = 512, k = 11 - but some always do
    _seen('truncated', c, R.conv1d(x, wf, n, rnd=R.trunc_bf16, **kw)[0] - want, bound, every,
          0.9 if c['short'] else 0.5 if (k <= 3 or (k * c['ci'] <= 1024 and not c['io'] & 1)) else 0.0)
    # (b) the last tap dropped at a tile's first position (the position a tile-edge mistake in the staged rows would hit): short and dense
    a, w = D.f64(R.operand(x, c['slope'])), D.f64(R.rne_bf16(wf))
    left = split_ref._left(k, dil, c['pad_left'])
    one = torch.zeros_like(w)
    one[k - 1] = w[k - 1]
    first = torch.zeros_like(every)
    first[:, :, ::K.nt_of(c['inst'])] = True
    _seen('tap dropped', c, tile_ref.taps_sum(a, one, dil, left)[0], bound, first, 0.9)
    # (c) channels j and j ^ 1 swapped inside a k-step: the short-chain records (a dense sum hides nothing either, but only these are asserted)
    if c['short']:
        swap = torch.arange(c['ci']) ^ 1
        _seen('channels swapped', c, R.conv1d(x[:, swap], wf, n, **kw)[0] - want, bound, every, 0.9)


# ---------------------------------------------------------------------------------------------------------------
# dispatch
@pytest.mark.parametrize('c', K.ALL, ids=K.ids(K.ALL))
def test_dispatch_of_every_gpu_record(c):
    if c['op'] == 'conv':
        rc, names, cfg = K.dispatch(c)
    else:
        rc, names, cfg, tiles = K.convt_dispatch(c)
        if c['rc'] == K.OK:                                      # the rows of stats_part: one per batch item and tile width of positions
            assert tiles == c['B'] * D.ceil_div(c['L'], 32 * c['tile'][1] * c['tile'][3])
        else:
            assert tiles == c['rc']
    print(c['id'], rc, names, cfg)
    assert (rc, names) == (c['rc'], c['kernels']), (rc, names)
    if c['cfg'] is not None:
        assert cfg == c['cfg'], cfg


def test_the_records_reach_every_template_tuple_the_dispatchers_can_return():
    seen = {}
    for c in K.ALL:
        if c['cfg'] is not None:
            seen.setdefault(c['cfg'], []).append(c)
    assert set(seen) == K.REACHABLE
    conv_insts = {t[:6] for t in K.REACHABLE if t[6] != 2}
    for inst in conv_insts:
        # full tiles through the chunk loop (ONE64 is one chunk by construction); dense and short-chain at every (k, dil)
        assert any(c['inst'] == inst and c['L'] >= K.nt_of(inst) and (c['ci'] // inst[4] >= 2 or inst == K.ONE64) for c in K.TILES + K.FULL), inst
        for k, d in K.KD:
            for short in (False, True):
                assert any(c['inst'] == inst and c['ks'] == (k,) and c['dil'] == d and c['short'] == short for c in K.TILES), (inst, k, d, short)
    for c in K.CONV_ALL:
        assert c['n'] == tuple(k * (1 if c['short'] else c['ci']) + c['ops'] for k in c['ks'])
        assert not c['short'] or c['B'] >= c['ci'] or (c['ci'] % c['B'] == 0 and c['ci'] == 512)
    # the mask epilogue on the 64 x 128, 64 x 256 and 128 x 256 tiles; every storage form where the dispatcher allows it
    assert all(t + (1, False, False) in seen for t in (K.T64, K.T256, K.T128))
    for inst, ios in K.IOS.items():
        assert {c['io'] for c in K.TILES if c['inst'] == inst} == set(ios)
    # the transposed conv: every generator (k, u) on every tile, with and without statistics
    for k, u in K.KU:
        for t in (K.CT2, K.CT1, K.CT0):
            assert any(c['tile'] == t and (c['k'], c['u']) == (k, u) and c['rc'] == K.OK for c in K.CONVT), (k, u, t)
        assert {c['stats'] for c in K.CONVT if (c['k'], c['u']) == (k, u) and c['io'] == 0} == {True, False}


# ---------------------------------------------------------------------------------------------------------------
# transposed conv and its packer
CT = [c for c in K.CONVT if c['B'] <= 2 and c['L'] <= 260]


@pytest.mark.parametrize('c', CT, ids=K.ids(CT))
def test_the_transposed_reference_is_f_conv_transpose1d_on_the_rounded_operands(c):
    x, wf, bias = K.convt_operands(c)
    k, u = c['k'], c['u']
    want, bound = R.convt1d(x, wf, u, c['n'], slope=c['slope'], bias=bias)
    act = F.leaky_relu(x, float(np.float32(c['slope']))).bfloat16().double()
    ind = F.conv_transpose1d(act, wf.bfloat16().double().permute(1, 2, 0).contiguous(), bias.double(), stride=u, padding=(k - u) // 2)
    _close(want, ind, 1e-12)
    assert torch.isfinite(bound).all() and (bound > 0).all()


@pytest.mark.parametrize('k,u,ci,co', K.PACKS)
def test_the_packer_statement_is_the_transposed_conv_as_a_conv_over_virtual_rows(k, u, ci, co):
    """Wv of convbf16_ref.virtual_weights, applied as a KV-tap Conv1d with hl taps on the left, gives row co * UP + r = output phase r of
    channel co of the transposed conv; and the fragment arrays have the size v2w_pack_bf16_convt_bytes reports."""
    from wavthruvec_pytorch_amd import _hip
    rng = np.random.default_rng(k * 100 + u)
    wf = (rng.standard_normal((k, ci, co)) / np.sqrt(k * ci)).astype(np.float32)
    UP, hl, hr, KV = R.convt_geom(k, u)
    x = torch.from_numpy(rng.standard_normal((2, ci, 24)))
    want = F.conv_transpose1d(x, torch.from_numpy(wf).double().permute(1, 2, 0).contiguous(), stride=u, padding=(k - u) // 2)
    for rows_per in (UP, u):
        wv = torch.from_numpy(R.virtual_weights(wf, u, rows_per)).double()
        z = tile_ref.taps_sum(x, wv, 1, hl)[0].reshape(2, co, rows_per, 24)
        _close(z[:, :, :u].permute(0, 1, 3, 2).reshape(2, co, 24 * u), want, 1e-12)
        assert not z[:, :, u:].any()
    frags = R.pack_bf16_convt(wf, u)
    assert len(frags) == 1 + R.exact_region(co, u)
    assert sum(f.size for f in frags) * 2 * 2 == R.pack_bf16_convt_bytes(k, ci, co, u) == _hip.load().v2w_pack_bf16_convt_bytes(k, ci, co, u)
