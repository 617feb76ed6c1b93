"""Every record of tests/bf16res_cases.py on the device: conv_bf16_res_kernel (csrc/v2w_conv_bf16_res.hip) in its four instantiations and
convt_bf16_res_kernel (csrc/v2w_convt_bf16_res.hip) in its nine, against the fp64 statement of the call on the operands as the kernel
rounds them and its derived bound (tests/bf16res_ref.py), per entry.  tests/test_bf16res_ref_cpu.py asserts which instantiation each record
launches.

What fails a record: a stored bf16 entry outside the one or two bf16 numbers that rne_bf16 can make of an fp32 value within n 2^-24 S of
`want` (the printed ratio is the distance from `want` to the nearest real that rounds to the stored value, over the bound; `single / lower /
upper / wider` count where the stored values landed); a statistics row of the transposed conv further from the sums of `want` than
bf16res_ref.convt_rows allows; any changed bit outside the region a call may write - outputs and statistics rows are NaN-filled between NaN
guards, inputs, affines and biases sit between NaN guards no output may show, and inputs, affines, biases and weights keep every bit; a
refusal that returns another code or touches a buffer; two runs of the same call that differ in a bit.

Worst ratios on an MI355X when these tests were written (all bf16 stores): branch convs lengths 0.0044, one branch per halo 0.0098
(C = 128, k = 1, mode 1), branches of different halos 0.0069, switches 0.0052, short-chain 0.11 (C = 128, (3,1) / (7,3) / (11,1), mode 0),
thresholds 0.0022; resident transposed conv 0.013 (the exact five phases, C_in = 32), its statistics rows 0.0067 (sums) and 0.0068
(squares); the fall-backs to conv_bf16_kernel 0.0023.  Of the 23.6 M stored entries 76.6 % have a one-member interval (|got - want| / b
there up to 1.6e4: the bf16 rounding itself, which is why it is not the criterion), 8.2 % landed on the lower and 8.2 % on the upper of
two, 7.0 % have a wider interval.  The file takes 5.1 s for its 250 tests, the slowest record 0.43 s (c128_L4_m0: the first launch of the
session), every other at most 0.05 s.

Defects: the records found none in the kernels.  Reading found two in v2w_branch_convs_bf16_fwd, fixed with this file and held by the
refusal records in_s_null_* / in_a_null_* and m1_in1_null: half an input affine was passed on (a set in_a with a NULL in_s is read by the
kernel; an in_s alone was dropped) and is now V2W_E_ARG in both modes, ahead of the launch; a NULL in[j], j >= 1, in mode 1 returned
V2W_E_SHAPE, which hipops.branch_convs_bf16 takes for "shape not served", and is now V2W_E_ARG like in[0].  Neither call was run on a
device before the check stood.

Value-only one-line mutants (no global address or launch geometry changes; (e) and (f) move a read inside the staged LDS tile), one run
each of this file on a library of its own, records that fail of 250:
(a) inv_slope taken as 1 in residual4 - 138: every branch record that runs but the four slope-1 records (the factor is 1 there);
(b) in_s read as 0 - 56: every mode-0 record with the affine, none without;
(c) mode 1's bias sum skips the last branch - 44: every mode-1 record of two or three branches whose last bias is set;
(d) out_div ignored - 44: every mode-1 record with out_div != 0;
(e) r0 computed with hla in place of hl - 122: every branch record that runs with a branch whose halo is no multiple of 4; the 20
    whose only halos are 0, 16, 24 or 32 pass (hla == hl there: the same row);
(f) the swizzle term dropped from residual4 - 142: every branch record that runs;
(g) bias[0] for both channels of a UP = 2 quad - 12: the records with a bias on the two UP = 2 tiles (the two without a bias pass);
(h) the `!ok` zeroing removed in front of the statistics - 35: the records with statistics rows and a partial last tile on the seven
    U == UP tiles (NaN-free but the rows count positions past L);
(i) the squares row fed from s1 - 42: every record with statistics rows on the seven U == UP tiles (the stride-5 forms sum elsewhere).
"""
import ctypes as C

import pytest
import torch

from tests import bf16res_cases as K
from tests import bf16res_ref as Q
from tests import convbf16_cases as KC
from tests import convbf16_ref as R
from tests import disc_ref as D
from tests.test_convbf16_kernels_gpu import Buf16
from tests.test_disc_kernels_gpu import _cases, _report, env  # noqa: F401  (env: the module-scoped fixture)
from tests.test_tile_kernels_gpu import GUARD, Buf, _nan_payload, _sync_or_stop  # noqa: F401  (GUARD: the guards' size)
from wavthruvec_pytorch_amd import hipops

pytestmark = pytest.mark.gpu


def _bits(b):
    return b.flat.view(torch.int16 if b.flat.dtype == torch.bfloat16 else torch.int32).clone()


def _kept(b):
    return b.untouched_outside(torch.zeros(b.shape, dtype=torch.bool))


def _store(cid, name, got, want, bound, ratios):
    r = R.check_store(got.float(), want, bound)
    print('[store] %s %s: single=%d (|got - want| / b up to %.3g) lower=%d upper=%d wider=%d'
          % (cid, name, r['single'], r['single_err'], r['lower'], r['upper'], r['wider']))
    assert r['outside'] == 0, '%s %s: %d entries outside their bf16 interval, worst ratio %.3g' % (cid, name, r['outside'], r['ratio'])
    ratios[name] = r['ratio']


def run_branch(env, c):
    dev, _hip, lib, st = env
    o = K.branch_operands(c)
    B, Cc, L, nb, ok = c['B'], c['C'], c['alloc_L'], len(c['kd']), c['rc'] == K.OK
    ins = [Buf16(dev, x, c['in_offb'] // 2) for x in o['xs']]
    outs = [Buf16(dev, _nan_payload(B, Cc, L), c['out_offb'] // 2) for _ in range(nb if c['mode'] == 0 else 1)]
    small = {q: Buf(dev, o[q]) for q in ('in_a', 'in_s') if o[q] is not None}
    biases = [None if b is None else Buf(dev, b) for b in o['biases']]
    if ok:
        wps = [hipops.pack_split(wf.to(dev).contiguous(), bf16=True)[0] for wf in o['wfs']]
    else:
        wps = [torch.zeros(2048, dtype=torch.float16, device=dev) for _ in range(nb)]
    wps0 = [w.clone() for w in wps]
    a = K.branch_struct(c, dict(in_=[b.base for b in ins], out=[b.base for b in outs], wps=[w.data_ptr() for w in wps],
                                bias=[0 if b is None else b.base for b in biases],
                                in_a=small['in_a'].base if 'in_a' in small else 0, in_s=small['in_s'].base if 'in_s' in small else 0))
    torch.cuda.synchronize()
    rc = lib.v2w_branch_convs_bf16_fwd(C.byref(a), st)
    _sync_or_stop(c['id'])
    assert rc == c['rc'], (c['id'], rc)
    if ok:                                                   # the same call once more, from the same buffers: the same bits
        first = [_bits(b) for b in outs]
        for b in outs:
            b.flat.copy_(b.before)
        assert lib.v2w_branch_convs_bf16_fwd(C.byref(a), st) == K.OK
        _sync_or_stop(c['id'] + ' (second run)')
        assert all(torch.equal(_bits(b), f) for b, f in zip(outs, first)), c['id'] + ': two runs differ'
    for b in outs:
        assert b.untouched_outside(torch.full(b.shape, ok, dtype=torch.bool)), c['id'] + ': stored outside its region'
    for b in ins + list(small.values()) + [b for b in biases if b is not None]:
        assert _kept(b), c['id'] + ': an input changed'
    assert all(torch.equal(w.view(torch.int16), w0.view(torch.int16)) for w, w0 in zip(wps, wps0)), c['id'] + ': the weights changed'
    if not ok:
        return
    ratios = {}
    for j, (want, bound) in enumerate(K.branch_reference(c, o)):
        _store(c['id'], 'out%d' % j, outs[j].payload().cpu(), want, bound, ratios)
    _report('bf16res ' + c['id'] + ' n=' + '/'.join(map(str, c['n'])), **ratios)


@_cases(K.LENGTHS)
def test_branch_convs_lengths(env, c):
    run_branch(env, c)


@_cases(K.HALOS)
def test_branch_convs_one_branch_per_halo(env, c):
    run_branch(env, c)


@_cases(K.MIXED)
def test_branch_convs_branches_of_different_halos(env, c):
    run_branch(env, c)


@_cases(K.SWITCHES)
def test_branch_convs_switches(env, c):
    run_branch(env, c)


@_cases(K.SHORT)
def test_branch_convs_short_chain(env, c):
    run_branch(env, c)


@_cases(K.THRESHOLDS)
def test_branch_convs_thresholds(env, c):
    run_branch(env, c)


@_cases(K.REFUSALS)
def test_branch_convs_refusals(env, c):
    run_branch(env, c)


# ---------------------------------------------------------------------------------------------------------------
# transposed conv
@_cases(K.CONVT_ALL)
def test_transposed_conv(env, c):
    dev, _hip, lib, st = env
    B, ci, co, L, u = (c[q] for q in ('B', 'ci', 'co', 'L', 'u'))
    x, wf, bias = KC.convt_operands(c)
    xb, out = Buf16(dev, x, c['in_offb'] // 2), Buf16(dev, _nan_payload(B, co, L * u))
    bd = Buf(dev, bias)
    wp = hipops.pack_bf16_convt(wf.to(dev).contiguous(), u)
    assert wp is not None
    wp0 = wp.clone()
    addr = dict(in_=xb.base, wp=wp.data_ptr(), bias=bd.base if c['bias'] else 0, out=out.base)
    stats = None
    if c['stats']:
        a0 = KC.convt_struct(c, dict(addr, stats_part=0))
        a0.stats_part = None
        rows = lib.v2w_convt1d_bf16_tiles(C.byref(a0))
        assert rows == B * D.ceil_div(L, K.ct_nt(c['inst']))
        stats = Buf(dev, _nan_payload(rows, co, 2))                         # exactly the rows the library reports, between guards
        addr['stats_part'] = stats.base
    a = KC.convt_struct(c, addr)
    if not c['bias']:
        a.bias = None
    torch.cuda.synchronize()
    rc = lib.v2w_convt1d_bf16_fwd(C.byref(a), st)
    _sync_or_stop(c['id'])
    assert rc == K.OK, (c['id'], rc)
    first = (_bits(out), None if stats is None else _bits(stats))
    out.flat.copy_(out.before)
    if stats is not None:
        stats.flat.copy_(stats.before)
    assert lib.v2w_convt1d_bf16_fwd(C.byref(a), st) == K.OK
    _sync_or_stop(c['id'] + ' (second run)')
    assert torch.equal(_bits(out), first[0]) and (stats is None or torch.equal(_bits(stats), first[1])), c['id'] + ': two runs differ'
    assert out.untouched_outside(torch.ones(out.shape, dtype=torch.bool)), c['id'] + ': stored outside its region'
    assert _kept(xb) and _kept(bd) and torch.equal(wp.view(torch.int16), wp0.view(torch.int16)), c['id'] + ': an input changed'
    if stats is not None:
        assert stats.untouched_outside(torch.ones(stats.shape, dtype=torch.bool)), c['id'] + ': statistics rows'
    want, bound = R.convt1d(x, wf, u, c['n'], slope=c['slope'], bias=bias if c['bias'] else None)
    ratios = {}
    _store(c['id'], 'out', out.payload().cpu(), want, bound, ratios)
    if stats is not None:
        s1, b1, s2, b2 = Q.convt_rows(want, bound, K.ct_nt(c['inst']), u)
        got = stats.payload().cpu()
        ratios.update(rowsum=D.worst_ratio(got[..., 0], s1, b1), sumsq=D.worst_ratio(got[..., 1], s2, b2))
    _report('bf16res ' + c['id'] + ' n=%d' % c['n'], **ratios)
