"""tests/bf16res_ref.py pinned against independent statements (F.conv1d / F.conv_transpose1d in fp64 on the rounded operands, the residual
and the statistics rows written out by hand), the dispatch table of tests/bf16res_cases.py (name sink and configuration query: which
conv_bf16_res_kernel / convt_bf16_res_kernel instantiation every GPU record launches, and its return code; the fall-backs land on
conv_bf16_kernel), the coverage of the 4 + 9 instantiations, the termination of the operand redraw, and the visibility of one lost tap at
the short-chain records.  No GPU needed.

The reference does not depend on the batch beyond the per-item affine, so the value checks run on the first two items of a record."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import bf16res_cases as K
from tests import bf16res_ref as Q
from tests import convbf16_cases as KC
from tests import convbf16_ref as R
from tests import disc_ref as D
from tests.test_disc_ref_cpu import _close

RUN = [c for c in K.BRANCH_ALL if c['rc'] == K.OK]
SEL = slice(0, 2)


def _independent_branch(c, x, wf, dil, bias, in_a, in_s):
    """bias + residual + conv of one branch from F.conv1d on the rounded operands, in fp64."""
    k, slope = wf.shape[0], float(np.float32(c['slope']))
    t = x.float()
    if in_a is not None:
        t = (in_a.double()[:, :, None] * t.double() + in_s.double()[:, :, None]).float()
    act = (t if c['slope'] == 1.0 else torch.where(t > 0, t, t * slope)).bfloat16().double()
    inv = float(np.float32(1.0) / np.float32(c['slope']))
    z = F.conv1d(act, D.wf_to_w(wf.bfloat16().double()), dilation=dil, padding=dil * (k - 1) // 2)
    z = z + torch.where(act > 0, act, act * inv)
    return z if bias is None else z + bias.double()[None, :, None]


@pytest.mark.parametrize('c', RUN, ids=K.ids(RUN))
def test_the_reference_is_f_conv1d_on_the_rounded_operands_and_the_redraw_terminates(c):
    o = K.branch_operands(c)                                     # (asserts that no ambiguous element is left after at most 64 rounds)
    for x in o['xs']:
        assert torch.equal(x, R.rne_bf16(x))
    if c['aff']:
        assert not R.ambiguous(o['xs'][0], c['slope'], o['in_a'], o['in_s']).any() and o['rounds'] <= 64
        print('[redraw] %s: %d rounds' % (c['id'], o['rounds']))
    if c['short']:
        for x in o['xs']:
            live = (x != 0).any(2)
            assert (live.sum(1) == 1).all() and len({int(v) for v in live.float().argmax(1)}) == c['B']
    if c['data'] == 'neg':
        assert all(bool((x < 0).all()) for x in o['xs'])
    if c['data'] == 'zeros':
        for x in o['xs']:
            bits = x.view(torch.int32)
            assert bool((bits == 0).any()) and bool((bits == -(1 << 31)).any())
    got = K.branch_reference(c, o, SEL)
    aff = (o['in_a'][SEL], o['in_s'][SEL]) if c['aff'] else (None, None)
    ind = [_independent_branch(c, o['xs'][0 if c['mode'] == 0 else j][SEL], o['wfs'][j], d, o['biases'][j], *aff)
           for j, (_, d) in enumerate(c['kd'])]
    if c['mode'] == 1:
        tot = sum(ind)
        ind = [tot / float(np.float32(c['out_div'])) if c['out_div'] else tot]
    assert len(got) == len(ind)
    for (want, bound), w2 in zip(got, ind):
        _close(want, w2, 1e-12)
        assert torch.isfinite(bound).all() and (bound >= 0).all()
    assert c['n'] == (tuple(k * (1 if c['short'] else c['C']) + 3 for k, _ in c['kd']) if c['mode'] == 0 else
                      (sum(k * (1 if c['short'] else c['C']) + 3 for k, _ in c['kd']) + (c['out_div'] != 0),))


def test_the_residual_is_the_kernels():
    xs = torch.tensor([2.0, -0.5, 0.0, -0.0, -3.0])
    r = Q.residual(xs, 0.3)
    inv = float(np.float32(1.0) / np.float32(0.3))                # (the fp32 reciprocal of the fp32 slope, not 1 / 0.3)
    assert inv != 1.0 / 0.3 and r.tolist() == [2.0, -0.5 * inv, 0.0, -0.0, -3.0 * inv]
    assert (r.view(torch.int64)[2:4] == torch.tensor([0, -(1 << 63)])).all()
    assert Q.residual(xs, 1.0).tolist() == xs.double().tolist()


@pytest.mark.parametrize('c', K.SHORT, ids=K.ids(K.SHORT))
def test_a_short_chain_record_sees_one_lost_tap(c):
    """At a short-chain record the last tap of the last branch, lost, moves `want` by more than b at more than half of the entries (of
    that branch's output in mode 0, of the one output in mode 1)."""
    o = K.branch_operands(c)
    want, bound = K.branch_reference(c, o)[-1]
    lost = dict(o, wfs=[w.clone() for w in o['wfs']])
    lost['wfs'][-1][-1] = 0.0
    moved = (K.branch_reference(c, lost)[-1][0] - want).abs()
    seen = float((moved > bound).double().mean())
    print('[power] %s: one lost tap exceeds the bound at %.3g of the entries, median %.3g bounds' % (c['id'], seen, float((moved / bound).median())))
    assert seen > 0.5


# ---------------------------------------------------------------------------------------------------------------
# dispatch
@pytest.mark.parametrize('c', K.BRANCH_ALL, ids=K.ids(K.BRANCH_ALL))
def test_dispatch_of_every_branch_record(c):
    rc, names = K.branch_dispatch(c)
    print(c['id'], rc, names)
    assert (rc, names) == (c['rc'], c['kernels']), (rc, names)


@pytest.mark.parametrize('c', K.CONVT_ALL, ids=K.ids(K.CONVT_ALL))
def test_dispatch_of_every_transposed_record(c):
    rc, names, cfg, tiles = KC.convt_dispatch(c)
    print(c['id'], rc, names, cfg)
    assert (rc, names, cfg) == (c['rc'], c['kernels'], c['cfg']), (rc, names, cfg)
    q = (C.c_int32 * 10)()
    assert K._hip.load().v2w_convt1d_bf16_config(C.byref(KC.convt_struct(c, KC.CT_FAKE)), q) == 0
    if c['inst'] is not None:                                    # the resident kernel: cfg[5] == 102, (MI, NI, WM, WN, UP, .., U)
        assert q[5] == 102 and tuple(q[:5]) + (q[9],) == c['inst']
        assert tiles == c['B'] * D.ceil_div(c['L'], K.ct_nt(c['inst']))
    else:
        assert q[5] == 2 and names[0].startswith('conv_bf16_kernel<')


def test_the_records_reach_every_instantiation():
    seen = {c['inst'] for c in K.BRANCH_ALL if c['inst'] is not None}
    assert seen == K.REACHABLE and len(seen) == 4
    ct = {c['inst'] for c in K.CONVT if c['inst'] is not None}
    assert ct == set(K.RES_CT) and len(ct) == 9
    for inst in K.REACHABLE:
        mine = [c for c in RUN if c['inst'] == inst]
        assert {c['L'] for c in mine} >= {4, 20, 252, 256, 260, 516}
        assert {len(c['kd']) for c in mine} == {1, 2, 3}
        assert {k for c in mine for k, _ in c['kd']} >= {1, 3, 5, 7, 11}
        assert {c['h'] for c in mine if len(c['kd']) == 1} >= {0, 1, 3, 5, 9, 15, 16, 24}
        assert {(-c['h']) % 4 for c in mine if len(c['kd']) == 1} == {0, 1, 2, 3}
        assert {c['slope'] for c in mine} >= {0.1, 0.25, 1.0}
        assert {c['data'] for c in mine} == {None, 'zeros', 'neg'}
        assert any(not any(c['bias']) for c in mine) and any(any(c['bias']) and not all(c['bias']) for c in mine)
        assert any(c['short'] for c in mine)
        if inst[4] == 0:
            assert {c['aff'] for c in mine} == {True, False}
        else:
            assert {c['out_div'] for c in mine} >= {0.0, 2.0, 3.0}
    for inst in K.RES_CT:
        mine = [c for c in K.CONVT if c['inst'] == inst]
        nt = K.ct_nt(inst)
        assert {c['L'] for c in mine} >= ({64, 128, 192} if inst[5] == 5 else {4, nt - 4, nt, nt + 4, 2 * nt + 4})
        assert {c['ci'] for c in mine} >= {32, 64} and {c['bias'] for c in mine} == {True, False}
        assert {c['stats'] for c in mine} == {True, False} and {c['slope'] for c in mine} == {0.1, 1.0}


# ---------------------------------------------------------------------------------------------------------------
# transposed conv
CT = [c for c in K.CONVT if c['L'] <= 260 and c['co'] <= 32]


@pytest.mark.parametrize('c', CT, ids=K.ids(CT))
def test_the_transposed_reference_and_its_rows(c):
    x, wf, bias = KC.convt_operands(c)
    x, k, u = x[:2], c['k'], c['u']
    bias = bias if c['bias'] else None
    assert torch.equal(x, R.rne_bf16(x))
    want, bound = R.convt1d(x, wf, u, c['n'], slope=c['slope'], bias=bias)
    act = F.leaky_relu(x, float(np.float32(c['slope']))).bfloat16().double()
    ind = F.conv_transpose1d(act, wf.bfloat16().double().permute(1, 2, 0).contiguous(), None if bias is None else bias.double(),
                             stride=u, padding=(k - u) // 2)
    _close(want, ind, 1e-12)
    assert torch.isfinite(bound).all() and (bound > 0).all()
    # the rows, by hand: tile t of item b covers the outputs [t NT u, min((t + 1) NT, L) u)
    NT = K.ct_nt(c['inst'])
    s1, b1, s2, b2 = Q.convt_rows(want, bound, NT, u)
    ntl = D.ceil_div(c['L'], NT)
    assert s1.shape == (2 * ntl, c['co'])
    for b in range(2):
        for t in range(ntl):
            w, e = want[b, :, t * NT * u:(t + 1) * NT * u], bound[b, :, t * NT * u:(t + 1) * NT * u]
            N = w.shape[1]
            assert N == min(NT, c['L'] - t * NT) * u
            _close(s1[b * ntl + t], w.sum(1), 1e-12)
            _close(s2[b * ntl + t], (w * w).sum(1), 1e-12)
            _close(b1[b * ntl + t], e.sum(1) + N * 2.0 ** -24 * w.abs().sum(1), 1e-12)
            _close(b2[b * ntl + t], (2 * w.abs() * e + e * e).sum(1) + N * 2.0 ** -24 * (w * w).sum(1), 1e-12)
