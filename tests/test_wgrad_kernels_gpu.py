"""Every record of tests/wgrad_cases.py on the device: v2w_wgrad (the pipelined Conv1d and ConvTranspose1d instantiations, the generic kernel
by each of its routes, both slab reduces) and v2w_wgrad_bf16 (both wave arrangements, fp32- and bf16-stored operands) against the fp64
weight gradient of the layer (tests/wgrad_ref.py), per entry.  tests/test_wgrad_ref_cpu.py asserts which kernels each record launches.

A record fails when any entry's |got - want| / (n * 2^-24 * S) exceeds 1 (n: B * Lq terms, one more for the affine and one for the slope;
S: the summed magnitudes of the entry's terms, from the reference's data; no entry is excluded).  The slab workspace holds exactly the slabs
the library asks for and, like dwf, starts as NaN; behind each lies a guard of one slab's size that must keep its sentinel; x and dy lie between
NaN guards, which no entry may show.  Every call runs twice and must give the same bits.  A refused call must leave every buffer as it was.
Each test prints its worst error / bound ratio (`-s` shows them; DESIGN.md 3e'-w records them).

Worst ratios on an MI355X when these tests were written (measurements for the record; the pass condition is the bound): v2w_wgrad, u = 1:
pipelined 0.045 at Lq = 20 and 0.0073 from Lq = 128 (WIDE 0.0016), generic 0.0018 (padded 0.00063), S < items 0.00020, the reduce records
0.000075; u > 1: 0.25 at Lq = 4 (n = 12 .. 14, so the roundings of the products and of the slab sum, which n counts once, weigh most), 0.028
at Lq = 28 .. 52 and 0.014 above; v2w_wgrad_bf16: 0.10 at Lq = 8, 0.0037 from Lq = 120, S < items 0.00012.  No record found a defect and no
kernel changed.  The file takes 5 to 9 s, its slowest record 0.2 s behind the first one's start-up.

One-line mutants of csrc/v2w_wgrad.hip and csrc/v2w_wgrad_bf16.hip, each built into a library of its own and run once; records that fail:
`pad` taken as `(k - u + 1) / 2` in wgrad_impl: the 4 `u2_k5_*` records (every other record has an even k - u, where the two agree);
`c - m` as `c + m` in the u > 1 offset: all 66 transposed records;  `x_s` read at `[0]` in wgrad_pipe_kernel: the 74 `_aff` records on a
pipelined kernel; the same in wgrad_kernel's scalar staging: the 20 `_aff` records on the generic kernel;  `p.hla` not rounded up to 4: the
first record (`c3222_k3_d1_L20_aff`; run with -x, the mutant loads float4s off their alignment);  wgrad_reduce16_kernel's tail loop stepping
4: the 2 `reduce16_nslab160_*` records (at 128 slabs the tail loop does not run);  `nt = 3` as 2 for k > 4 in v2w_wgrad_bf16: the 64 tap-sharing
records with k = 9 and 11 (taps 8 .. 10 stay NaN; k = 5 and 7 give the same bits with two taps per wave, and the CPU test sees the name)."""
import numpy as np
import pytest
import torch

from tests import wgrad_cases as K
from tests import wgrad_ref as R
from tests.test_disc_kernels_gpu import NAN, SENT, _cases, _report, env  # noqa: F401  (env: the module-scoped fixture)
from tests.test_tile_kernels_gpu import GUARD, _f32, _rng, _sync_or_stop

pytestmark = pytest.mark.gpu


class In:
    """An operand between NaN guards: [GUARD | lead | payload | GUARD] elements; `ptr` is the payload's address, `lead` bytes past a 16-byte boundary."""

    def __init__(self, dev, payload, lead=0):
        es = payload.element_size()
        assert lead % es == 0
        n, le = payload.numel(), lead // es
        flat = torch.full((2 * GUARD + le + n,), NAN, dtype=payload.dtype)
        flat[GUARD + le:GUARD + le + n] = payload.reshape(-1)
        self.flat = flat.to(dev)
        assert self.flat.data_ptr() % 16 == 0 and (GUARD * es) % 16 == 0
        self.ptr = self.flat.data_ptr() + (GUARD + le) * es


class Out:
    """n NaN floats the call may write, then `guard` floats holding the sentinel."""

    def __init__(self, dev, n, guard):
        flat = torch.full((n + guard,), NAN)
        flat[n:] = SENT
        self.flat, self.n = flat.to(dev), n
        self.ptr = self.flat.data_ptr()
        assert self.ptr % 16 == 0

    def guard_intact(self):
        return bool((self.flat[self.n:] == SENT).all())

    def all_nan(self):
        return bool(torch.isnan(self.flat[:self.n]).all())


def _operands(c, dev):
    """(device operands, (want, S) or None for a refused record)."""
    rng = _rng(c)
    bf = K.is_bf16(c)
    B, Lq, k, dil, u = c['B'], c['Lq'], c['k'], c['dil'], c.get('u', 1)
    ci, co = (c['C'], c['C']) if bf else (c['c_in'], c['c_out'])
    a = s = None
    if bf:
        x, ga, gs = R.draw_exact(rng, B, ci, Lq)
        if c['affine']:
            a, s = ga, gs
    else:
        x = _f32(rng, B, ci, Lq)
        if c['affine']:
            a, s = 1.0 + _f32(rng, B, ci, scale=0.2), _f32(rng, B, ci, scale=0.3)
    dy = _f32(rng, B, co, u * Lq)
    if bf and c['stored'] == 'bf16':
        x, dy = x.bfloat16(), dy.bfloat16()
    ops = dict(x=In(dev, x, c.get('x_off', 0)), dy=In(dev, dy), a=None if a is None else In(dev, a),
               s=None if s is None or c.get('no_xs') else In(dev, s))
    if c['rc'] != K.OK:
        return ops, None
    ref = R.wgrad_bf16(x, a, s, dy, k, dil, c['slope']) if bf else R.wgrad(x, a, s, dy, k, dil, u, c['slope'])
    return ops, ref


def _run(env, c, name):
    dev, _hip, lib, st = env
    ops, ref = _operands(c, dev)
    bf = K.is_bf16(c)
    ci, co = (c['C'], c['C']) if bf else (c['c_in'], c['c_out'])
    nw = c['k'] * ci * co
    ns = K.slabs(c)
    ptr = {n: (None if o is None else o.ptr) for n, o in ops.items()}
    before = {n: o.flat.clone() for n, o in ops.items() if o is not None}
    got = []
    for _ in range(2):
        slab, dwf = Out(dev, max(ns, 1) * nw, max(nw, GUARD)), Out(dev, nw, max(nw, GUARD))
        rc = K.call(c, ptr['x'], ptr['a'], ptr['s'], ptr['dy'], dwf.ptr, slab.ptr, stream=st)
        _sync_or_stop(name)
        assert rc == c['rc'], rc
        assert slab.guard_intact() and dwf.guard_intact()
        for n, o in ops.items():
            assert o is None or torch.equal(o.flat.view(torch.int16 if o.flat.element_size() == 2 else torch.int32),
                                            before[n].view(torch.int16 if o.flat.element_size() == 2 else torch.int32)), n
        if rc != K.OK:
            assert slab.all_nan() and dwf.all_nan()               # a refused call stores nothing
            continue
        got.append(dwf.flat[:nw].cpu().view(c['k'], ci, co))
    if ref is None:
        return
    assert ns > 0
    assert torch.equal(got[0].view(torch.int32), got[1].view(torch.int32))                 # deterministic: the same bits
    want, S = ref
    _report(name, dwf=R.worst_ratio(got[0], want, R.sum_bound(c['n'], S)))


@_cases(K.WGRAD)
def test_wgrad_conv(env, c):
    _run(env, c, 'wgrad ' + c['id'])


@_cases(K.WGRAD_T)
def test_wgrad_conv_transpose(env, c):
    _run(env, c, 'wgrad_t ' + c['id'])


@_cases(K.WGRAD_REJECT)
def test_wgrad_refusals(env, c):
    _run(env, c, 'wgrad_reject ' + c['id'])


@_cases(K.WGRAD_BF16)
def test_wgrad_bf16(env, c):
    _run(env, c, 'wgrad_bf16 ' + c['id'])


@_cases(K.WGRAD_BF16_REJECT)
def test_wgrad_bf16_refusals(env, c):
    _run(env, c, 'wgrad_bf16_reject ' + c['id'])
