"""Every record of tests/convbf16_cases.py on the device: conv_bf16_kernel (csrc/v2w_conv_bf16.hip) in every instantiation its two
dispatchers can return - eight Conv1d tile forms with fp32 / bf16 storage and the mask epilogue, three transposed-conv forms with vector
and element-wise staging - and pack_bf16_convt_kernel, against the fp64 statement of the call on the operands as the kernel rounds them and
its derived bound (tests/convbf16_ref.py), per entry.  tests/test_convbf16_ref_cpu.py asserts which instantiation each record launches.

What fails a record: an fp32-stored entry with |got - want| / (n * 2^-24 * S) above 1; a bf16-stored entry outside the one or two bf16
numbers that rne_bf16 can make of an fp32 value within that bound (the printed ratio is the distance from `want` to the nearest real that
rounds to the stored value, over the bound; `single / lower / upper` count where the stored values landed); a statistics row of the
transposed conv further than n * 2^-24 * sum |v| (sum v^2) from the sums of the values the launch itself stored; any changed bit outside
the region a call may write - every such buffer is NaN-filled between guards of tests/test_tile_kernels_gpu.GUARD floats (the same byte
count of bf16 NaN for bf16 tensors, so a read or store at 2-byte granularity next to the payload shows), inputs sit between NaN guards no
output may show; a refusal that returns another code or touches a buffer; two runs of the same call that differ in a bit.  The packer is
compared bit for bit (int16 view) over both regions on a pattern-filled buffer whose other bytes must keep the pattern.

Worst ratios on an MI355X when these tests were written (fp32 store / bf16 store): tiles dense 0.037 (128 x 256, k = 1) / 0.0066,
short-chain 0.64 (64 x 128, k = 2 with n = 3) / 0.12; full tiles 0.017 / 0.0032; threshold records 0.027 / 0.0020; lengths and offsets
0.0077 / 0.0023; prologue / epilogue switches 0.029 (four problems, element-wise epilogue) / 0.0089; fallback to the split kernel 0.013;
transposed conv 0.036 / 0.0030, its statistics rows 0.0062 (sums) and 0.0060 (squares).  Of the bf16-stored entries 78 % have a one-member interval
(|got - want| / b there up to 3e4: the bf16 rounding itself, which is why it is not the criterion), 6.3 % landed on the lower and 6.3 % on
the upper of two, 9 % have a wider interval (a small value under the bound of a long chain).
The file takes 10.8 s for its 418 tests, the slowest records 0.5 s (t128_io3_all_add_L168: 11 M entries; c32_io0_k3_d1_short: the
first launch of the session).

Defect these records found: t128_io3_all_add and t128_io3_all_acc (128 x 256 tile, bf16 tensors, addends, L = 40) had half of their
entries outside the interval - the pipelined epilogue's request for the next row block's residual / addend rows was skipped together with a
column pass wholly past L, so the second row block added the first block's rows.  Fixed in the kernel (DESIGN.md 3e''''').  The two
records at L = 168 put the same edge into the second wave column; all four fail on the kernel as it was and pass on the fixed one.

Value-only one-line mutants of csrc/v2w_conv_bf16.hip (no address changes), one run each of this file, records that fail:
`res_s` read as 0 - 50, every switch record with a residual affine on every path; `out_div` applied before the residual / addends - 44,
every record with out_div and another term (res_aff_div, all_add, all_acc, n4_all, mask_all); `add1` ignored - 35 (add01, all_add, n4_all,
mask_all on every path, the three unaligned-addend records); mask compare as `>=` - 6: the records without a mask affine, whose source
holds the exact +0 / -0 (t64, t64_escal, scal, wide t256 / t128 / c32); slope applied after the bf16 rounding - 291: every record with an
fp32 input and a slope, none with a bf16-stored input (rounding a bf16 number changes nothing: same kernel values); one tap's fragment
zeroed in pack_bf16_convt_kernel - 80: all eight packer cases and 72 transposed-conv records; the transposed conv's s2 taken as s1 - 69:
every transposed-conv record with statistics rows.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import convbf16_cases as K
from tests import convbf16_ref as R
from tests import disc_ref as D
from tests import split_ref
from tests.test_disc_kernels_gpu import NAN, _cases, _report, env  # noqa: F401  (env: the module-scoped fixture)
from tests.test_tile_kernels_gpu import GUARD, Buf, _addr, _nan_payload, _sum_rows_ok, _sync_or_stop
from wavthruvec_pytorch_amd import hipops

pytestmark = pytest.mark.gpu

WIDE = ('res', 'add0', 'add1', 'mask_src')
PATTERN = 0x5a5b


class Buf16(Buf):
    """tests/test_tile_kernels_gpu.Buf for a bf16 tensor: [guard | lead | payload | guard] in 2-byte elements, the guards GUARD floats' worth
    of bytes of bf16 NaN; `lead` in elements; `base` 16-byte aligned."""

    def __init__(self, dev, payload, lead=0):
        n, g = payload.numel(), 2 * GUARD
        flat = torch.full((2 * g + lead + n,), NAN, dtype=torch.bfloat16)
        flat[g + lead:g + lead + n] = payload.reshape(-1).bfloat16()
        self.flat, self.lo, self.n, self.shape = flat.to(dev), g + lead, n, tuple(payload.shape)
        self.before = self.flat.clone()
        assert self.flat.data_ptr() % 16 == 0
        self.base = self.flat.data_ptr() + 2 * g

    def untouched_outside(self, written):
        w = torch.zeros(self.flat.numel(), dtype=torch.bool, device=self.flat.device)
        w[self.lo:self.lo + self.n] = written.reshape(-1).to(self.flat.device)
        return bool(((self.flat.view(torch.int16) == self.before.view(torch.int16)) | w).all())


def _buf(dev, payload, esize, offb=0):
    assert offb % esize == 0
    return (Buf16 if esize == 2 else Buf)(dev, payload, offb // esize)


def _bits(b):
    return b.flat.view(torch.int16 if b.flat.dtype == torch.bfloat16 else torch.int32).clone()


def _problem(c, i, dev):
    o = K.operands(c, i)
    t, ref = o['t'], o['ref']
    bufs = {'in_': _buf(dev, t['x'], K.esize(c, 'in_', i), c['in_offb'])}
    if c['rc'] == K.OK:
        bufs['wps'], bufs['winv'] = hipops.pack_split(t['wf'].to(dev).contiguous(), bf16=True)
    else:
        bufs['wps'], bufs['winv'] = torch.zeros(2048, dtype=torch.float16, device=dev), torch.ones(4, device=dev)
    for name, v in t.items():
        if name in WIDE:
            bufs[name] = _buf(dev, v, K.esize(c, name, i), c['e_offb'])
        elif name not in ('x', 'wf'):
            bufs[name] = v.to(dev)
    out = _nan_payload(c['B'], c['out_ct'] or c['co'], K.S.problem_L(c, i))
    if 'old' in ref:
        out[:] = ref['old']
    bufs['out'] = _buf(dev, out, K.esize(c, 'out', i), c['out_offb'])
    return bufs, o


def _check(name, got, want, bound, out_bf, ratios, lands):
    if not out_bf:
        ratios[name] = D.worst_ratio(got, want, bound)
        return
    r = R.check_store(got.float(), want, bound)
    assert r['outside'] == 0, '%s: %d entries outside their bf16 interval, worst ratio %.3g' % (name, r['outside'], r['ratio'])
    ratios[name] = r['ratio']
    lands.append('%s: single=%d (|got - want| / b up to %.3g) lower=%d upper=%d wider=%d'
                 % (name, r['single'], r['single_err'], r['lower'], r['upper'], r['wider']))


def run_conv(env, c):
    dev, _hip, lib, st = env
    n = len(c['ks'])
    probs = [_problem(c, i, dev) for i in range(n)]
    per = [{name: _addr(b) for name, b in bufs.items()} for bufs, _ in probs]
    torch.cuda.synchronize()
    rc, _ = K.call(c, per, st)
    _sync_or_stop(c['id'])
    assert rc == c['rc'], (c['id'], rc)
    first = [_bits(bufs['out']) for bufs, _ in probs]
    if rc == K.OK:                                           # the same call once more, from the same buffers: the same bits
        for bufs, _ in probs:
            bufs['out'].flat.copy_(bufs['out'].before)
        rc2, _ = K.call(c, per, st)
        _sync_or_stop(c['id'] + ' (second run)')
        assert rc2 == K.OK
        for (bufs, _), f in zip(probs, first):
            assert torch.equal(_bits(bufs['out']), f), c['id'] + ': two runs differ'
    rd = dev if c['big'] else torch.device('cpu')
    ratios, lands = {}, []
    for i, (bufs, o) in enumerate(probs):
        out = bufs['out']
        assert out.untouched_outside(torch.full(out.shape, rc == K.OK, dtype=torch.bool)), c['id'] + ': stored outside its region'
        for name in ('in_',) + WIDE:
            if name in bufs:
                assert bufs[name].untouched_outside(torch.zeros(bufs[name].shape, dtype=torch.bool)), name
        if rc != K.OK:
            continue
        kw = {q: (v.to(rd) if isinstance(v, torch.Tensor) else v) for q, v in K.ref_kwargs(c, o).items()}
        x, wf = o['t']['x'].to(rd), o['t']['wf'].to(rd)
        if c['inst'] is None:                                # the split kernel's bf16 form took the call
            want, bound = split_ref.conv1d_bf16(x[:, :, c['in_phase']::c['in_stride']], wf, c['n'][i], **kw)
        else:
            want, bound = R.conv1d(x, wf, c['n'][i], **kw)
        _check('out%d' % i, out.payload().to(rd), want, bound, K.esize(c, 'out', i) == 2, ratios, lands)
    for line in lands:
        print('[store] %s %s' % (c['id'], line))
    _report('convbf16 ' + c['id'] + ' n=' + '/'.join(map(str, c['n'])), **ratios)


@_cases(K.TILES)
def test_tiles_dense_and_short_chain(env, c):
    run_conv(env, c)


@_cases(K.FULL)
def test_full_tiles_through_the_chunk_loop(env, c):
    run_conv(env, c)


@_cases(K.THRESHOLDS)
def test_dispatch_thresholds(env, c):
    run_conv(env, c)


@_cases(K.LENGTHS)
def test_lengths_and_alignment(env, c):
    run_conv(env, c)


@_cases(K.EPILOGUES)
def test_prologue_and_epilogue_switches(env, c):
    run_conv(env, c)


@_cases(K.FALLBACK)
def test_fallback_to_the_split_kernel(env, c):
    run_conv(env, c)


@_cases(K.REFUSALS)
def test_refusals(env, c):
    run_conv(env, c)


# ---------------------------------------------------------------------------------------------------------------
# transposed conv
@_cases(K.CONVT_ALL)
def test_transposed_conv(env, c):
    dev, _hip, lib, st = env
    B, ci, co, L, k, u, io = (c[q] for q in ('B', 'ci', 'co', 'L', 'k', 'u', 'io'))
    x, wf, bias = K.convt_operands(c)
    es = 2 if io == 3 else 4
    xb, out = _buf(dev, x, es, c['in_offb']), _buf(dev, _nan_payload(B, co, L * u), es, c['out_offb'])
    bd = bias.to(dev)
    wp = hipops.pack_bf16_convt(wf.to(dev).contiguous(), u) if c['rc'] == K.OK else torch.zeros(4096, dtype=torch.bfloat16, device=dev)
    assert wp is not None
    addr = dict(in_=xb.base, wp=wp.data_ptr(), bias=bd.data_ptr(), out=out.base)
    stats = None
    if c['stats']:
        a0 = K.convt_struct(c, dict(addr, stats_part=0))
        a0.stats_part = None
        rows = lib.v2w_convt1d_bf16_tiles(C.byref(a0))
        assert rows == B * D.ceil_div(L, 32 * c['tile'][1] * c['tile'][3]) if c['rc'] == K.OK else rows == c['rc']
        stats = Buf(dev, _nan_payload(max(rows, 1), co, 2))                 # exactly the rows the library reports, between guards
        addr['stats_part'] = stats.base
    a = K.convt_struct(c, addr)
    torch.cuda.synchronize()
    rc = lib.v2w_convt1d_bf16_fwd(C.byref(a), st)
    _sync_or_stop(c['id'])
    assert rc == c['rc'], (c['id'], rc)
    ok = rc == K.OK
    if ok:
        first = (_bits(out), None if stats is None else _bits(stats))
        out.flat.copy_(out.before)
        if stats is not None:
            stats.flat.copy_(stats.before)
        assert lib.v2w_convt1d_bf16_fwd(C.byref(a), st) == K.OK
        _sync_or_stop(c['id'] + ' (second run)')
        assert torch.equal(_bits(out), first[0]) and (stats is None or torch.equal(_bits(stats), first[1])), c['id'] + ': two runs differ'
    assert out.untouched_outside(torch.full(out.shape, ok, dtype=torch.bool)), c['id'] + ': stored outside its region'
    assert xb.untouched_outside(torch.zeros(xb.shape, dtype=torch.bool))
    if stats is not None:
        assert stats.untouched_outside(torch.full(stats.shape, ok, dtype=torch.bool)), c['id'] + ': statistics rows'
    if not ok:
        return
    rd = dev if c['big'] else torch.device('cpu')
    want, bound = R.convt1d(x.to(rd), wf.to(rd), u, c['n'], slope=c['slope'], bias=bias.to(rd))
    ratios, lands = {}, []
    got = out.payload().to(rd)
    _check('out', got, want, bound, io == 3, ratios, lands)
    if stats is not None:
        NT = 32 * c['tile'][1] * c['tile'][3]
        ratios.update(_sum_rows_ok(c['id'], stats.payload().to(rd), got, NT * u, NT * u, True))
    for line in lands:
        print('[store] %s %s' % (c['id'], line))
    _report('convbf16 ' + c['id'] + ' n=%d' % c['n'], **ratios)


# ---------------------------------------------------------------------------------------------------------------
# the packer, bit for bit
@pytest.mark.parametrize('k,u,ci,co', K.PACKS)
def test_pack_bf16_convt_is_the_documented_layout_bit_for_bit(env, k, u, ci, co):
    dev, _hip, lib, st = env
    wf = (np.random.default_rng(k * 100 + u).standard_normal((k, ci, co)) / np.sqrt(k * ci)).astype(np.float32)
    nbytes = lib.v2w_pack_bf16_convt_bytes(k, ci, co, u)
    assert nbytes == R.pack_bf16_convt_bytes(k, ci, co, u) > 0
    buf = torch.full((nbytes // 2 + 1024,), PATTERN, dtype=torch.int16, device=dev)
    wfd = torch.from_numpy(wf).to(dev)
    assert lib.v2w_pack_bf16_convt(wfd.data_ptr(), buf.data_ptr(), k, ci, co, u, st) == 0
    _sync_or_stop('pack_bf16_convt')
    got = buf.cpu().numpy()
    assert (got[nbytes // 2:] == PATTERN).all()
    units = got[:nbytes // 2].reshape(-1, 2, 64, 8)          # units of (hi, lo) x 64 lanes x 8 bf16
    want = np.concatenate([f.reshape(-1, 64, 8) for f in R.pack_bf16_convt(wf, u)])
    assert np.array_equal(units[:, 0], want)
    assert (units[:, 1] == PATTERN).all()
