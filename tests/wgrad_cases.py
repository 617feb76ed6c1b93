"""The cases of tests/test_wgrad_kernels_gpu.py, one record per call of v2w_wgrad / v2w_wgrad_bf16, with the kernels each launches, its
return code and the length `n` of its summation chain.

tests/test_wgrad_ref_cpu.py drives every record through the name sink (`dispatch`, host-only, made-up pointers with the record's
alignment) and asserts `kernels` and `rc`; the GPU tests run the same records on real tensors.  The names were filled in by reading
try_pipe, v2w_wgrad_plan, wgrad_impl and wgb_plan (csrc/v2w_wgrad.hip, csrc/v2w_wgrad_bf16.hip); the comments carry the arithmetic.
The shapes are the smallest that land on each branch, not the workload's.

v2w_wgrad_plan: mf = 32 when both channel counts are multiples of 32, else 16 when both are multiples of 16, else 16 `padded`.  u = 1: the
waves sit 2 x 2 over (C_out, C_in) when both are multiples of 2 mf, else 1 x 1 with 4 position lanes (wp = 4 / (wco wci)).  u > 1: wco = 2
when C_out is a multiple of 2 mf, wci = 2 when C_in is.  tiles = ceil(C_out / (wco mf)) ceil(C_in / (wci mf)), items = B ceil(Lq / 128),
S = min(ceil(512 / tiles), items), nslab = S wp; nslab >= 128 takes wgrad_reduce16_kernel.
wgrad_impl: ceil(k / 7) balanced tap groups (11 -> 6 + 5, 8 -> 4 + 4); per group hl = -min(0, offsets), hr = max(0, offsets),
hla = roundup4(hl), xc4 = (hla + ptq + hr + 3) / 4, ptq = 128, 128, 48, 32 for u = 1, 2, 4, 5.  The pipelined kernel needs Lq % 4 == 0,
x and dy 16-byte aligned, channel counts that are multiples of 16, xc4 <= 40 (u = 1) or (ptq + 16) / 4, and an instantiation (try_pipe);
anything else runs the generic kernel, once per dy phase and tap group."""
from wavthruvec_pytorch_amd import _hip

from tests.disc_cases import AUX, AUX2, OK, OUT, SLAB, X, _case, _names, ids  # noqa: F401  (ids: for the two test files)

E_ARG, E_SHAPE = _hip.E_ARG, _hip.E_SHAPE
SLOPE = 0.1


def _pipe(mf, wco, wci, nt, u=1, wide=False):
    return 'wgrad_pipe_kernel<%d, %d, %d, %d, %d, %s>' % (mf, wco, wci, nt, u, 'true' if wide else 'false')


GEN32, GEN16 = 'wgrad_kernel<32>', 'wgrad_kernel<16>'
RED, RED16 = 'wgrad_reduce_kernel', 'wgrad_reduce16_kernel'


def _both(id, kernels, B=3, **kw):
    """A call with the input affine and slope 0.1, and the same call with x_a = x_s = NULL and slope 1.  n = B Lq terms per entry, one more
    for the affine's fma and one for the slope's multiply."""
    n = B * kw['Lq']
    return [_case(id + '_aff', kernels, B=B, affine=True, slope=SLOPE, n=n + 2, **kw),
            _case(id + '_plain', kernels, B=B, affine=False, slope=1.0, n=n, **kw)]


# ---------------------------------------------------------------------------------------------------------------
# v2w_wgrad, u = 1
WGRAD = []
# cfg 3222 (64, 64): one tile, S = items <= 9, wp = 1 -> wgrad_reduce_kernel.  xc4 per group:
#   (3, 1): offsets -1 .. 1, hla 4, hr 1 -> 34;  (7, 3): -9 .. 9, hla 12 -> 38;  (7, 5): -15 .. 15, hla 16 -> (16 + 128 + 15 + 3) / 4 = 40 exactly;
#   (11, 3): taps 0 .. 5 at -15 .. 0 (hla 16, hr 0 -> 36), taps 6 .. 10 at 3 .. 15 (hla 0, hr 15 -> 36);  (11, 5): -25 .. 0 (hla 28 -> 39), 5 .. 25 (39).
#   The five-tap groups stay at xc4 <= 40, so none takes the WIDE instantiation (that needs 40 < xc4 <= 56).
for _k, _dil, _nts in ((3, 1, (3,)), (7, 3, (7,)), (11, 3, (6, 5)), (11, 5, (6, 5)), (7, 5, (7,))):
    for _Lq in (20, 128, 300):        # shorter than the halo, exactly one chunk, a ragged third chunk
        WGRAD += _both('c3222_k%d_d%d_L%d' % (_k, _dil, _Lq), [_pipe(32, 2, 2, nt) for nt in _nts] + [RED],
                       c_in=64, c_out=64, Lq=_Lq, k=_k, dil=_dil, u=1)
# cfg 3211: C_in = 32 is no multiple of 64 -> 1 x 1 waves, 4 position lanes.  k = 4: centre (4 - 1) / 2 = 1, offsets -1, 0, 1, 2 (hla 4, hr 2 -> 34)
for _ci, _co in ((32, 64), (32, 32)):
    for _Lq in (20, 300):
        WGRAD += _both('c3211_%dx%d_k7_d3_L%d' % (_ci, _co, _Lq), [_pipe(32, 1, 1, 7), RED], c_in=_ci, c_out=_co, Lq=_Lq, k=7, dil=3, u=1)
        WGRAD += _both('c3211_%dx%d_k4_L%d' % (_ci, _co, _Lq), [_pipe(32, 1, 1, 4), RED], c_in=_ci, c_out=_co, Lq=_Lq, k=4, dil=1, u=1)
# cfg 1611: (16, 32) has C_in no multiple of 32 -> mf 16.  k = 11: offsets -5 .. 0 (hla 8 -> 34) and 1 .. 5 (34)
for _ci, _co in ((16, 16), (16, 32)):
    for _Lq in (20, 300):
        WGRAD += _both('c1611_%dx%d_k11_L%d' % (_ci, _co, _Lq), [_pipe(16, 1, 1, 6), _pipe(16, 1, 1, 5), RED],
                       c_in=_ci, c_out=_co, Lq=_Lq, k=11, dil=1, u=1)
# every tap count of launch_pipe_nt on the three arrangements (k = 1 .. 7 at dilation 1 is one group of k taps, xc4 <= 34), and the WIDE
# instantiation: (64, 64), k = 5, dil = 9 -> offsets -18 .. 18, hla 20, hr 18, xc4 = (20 + 128 + 18 + 3) / 4 = 42 in (40, 56] with ntap 5
for _C, _mf, _w in ((64, 32, 2), (32, 32, 1), (16, 16, 1)):
    for _k in range(1, 8):
        WGRAD += _both('nt_c%d_k%d' % (_C, _k), [_pipe(_mf, _w, _w, _k), RED], c_in=_C, c_out=_C, Lq=132, k=_k, dil=1, u=1)
WGRAD += _both('wide_k5_d9', [_pipe(32, 2, 2, 5, 1, True), RED], c_in=64, c_out=64, Lq=300, k=5, dil=9, u=1)
# the generic kernel by each of its four routes
WGRAD += _both('gen_L301_c64_k11', [GEN32, GEN32, RED], c_in=64, c_out=64, Lq=301, k=11, dil=3, u=1)      # Lq % 4 != 0; 6 + 5 taps
WGRAD += _both('gen_L301_c16_k3', [GEN16, RED], c_in=16, c_out=16, Lq=301, k=3, dil=1, u=1)
WGRAD += _both('gen_x_plus4', [GEN32, RED], c_in=64, c_out=64, Lq=300, k=7, dil=3, u=1, x_off=4)          # x 4 bytes past a 16-byte boundary
WGRAD += _both('gen_halo_k7_d7', [GEN32, RED], c_in=64, c_out=64, Lq=300, k=7, dil=7, u=1)                # -21 .. 21: hla 24, xc4 44 > 40, ntap 7 != 5
WGRAD += _both('gen_pad_8x8_k11_d3', [GEN16, GEN16, RED], c_in=8, c_out=8, Lq=300, k=11, dil=3, u=1)      # padded: 16-row tiles, rows 8 .. 15 staged as 0
WGRAD += _both('gen_pad_16x8_k3', [GEN16, RED], c_in=16, c_out=8, Lq=300, k=3, dil=1, u=1)
# 6 x 6 = 36 weights per tap is a multiple of 4: the plan takes it as a padded shape (the reduce sums float4s of the k C_in C_out weights)
WGRAD += _both('gen_pad_6x6_k3', [GEN16, RED], c_in=6, c_out=6, Lq=300, k=3, dil=1, u=1)
# S < items: 16 tiles, S = 512 / 16 = 32, 36 items -> two per slab, slabs 18 .. 31 get none and hold zeros.  With 12 chunks per batch item no
# pair straddles two batch entries; at Lq = 1408 (11 chunks, 33 items) the pair (10, 11) does: item 10 is the end of b = 0, item 11 the start of b = 1.
# (That second record is an addition: the first lands on S < items but walks no slab across a batch boundary.)
WGRAD += _both('S_below_items_L1536', [_pipe(32, 2, 2, 3), RED], c_in=256, c_out=256, Lq=1536, k=3, dil=1, u=1)
WGRAD += _both('S_below_items_L1408', [_pipe(32, 2, 2, 3), RED], c_in=256, c_out=256, Lq=1408, k=3, dil=1, u=1)
# wgrad_reduce16_kernel from nslab = 128: one tile, wp = 4, S = items.  B = 2, Lq = 2048: 32 items, 128 slabs (two rounds of the 64-slab loop,
# no tail); B = 2, Lq = 2560: 40 items, 160 slabs (the tail loop runs for every lane); B = 1, Lq = 3848: 31 items, 124 slabs, the 4-lane reduce.
WGRAD += _both('reduce16_nslab128', [_pipe(16, 1, 1, 3), RED16], B=2, c_in=16, c_out=16, Lq=2048, k=3, dil=1, u=1)
WGRAD += _both('reduce16_nslab160', [_pipe(16, 1, 1, 3), RED16], B=2, c_in=16, c_out=16, Lq=2560, k=3, dil=1, u=1)
WGRAD += _both('reduce_nslab124', [_pipe(16, 1, 1, 3), RED], B=1, c_in=16, c_out=16, Lq=3848, k=3, dil=1, u=1)

# ---------------------------------------------------------------------------------------------------------------
# v2w_wgrad, u > 1 (ConvTranspose1d, pad = (k - u) / 2; dy is (B, C_out, u Lq)).  Every offset is -1, 0 or 1: hla <= 4, hr <= 1.
PTQ = {2: 128, 4: 48, 5: 32, 8: 128}          # (u = 8 has no pipelined form: the generic kernel's chunk is 128 positions)


def _lqs(u):
    p = PTQ[u]
    return (4, p - 4, p, p + 4, 2 * p + 8)


WGRAD_T = []
for _u, _k, _ci, _co, _kern, _tag in (
        (5, 11, 64, 64, [_pipe(32, 2, 2, 6, 5), _pipe(32, 2, 2, 5, 5)], 'u5_k11_64x64'),      # 3222; 11 taps -> 6 + 5
        (4, 8, 64, 64, [_pipe(32, 2, 2, 4, 4)] * 2, 'u4_k8_64x64'),                           # 3222; 8 taps -> 4 + 4
        (2, 4, 64, 32, [_pipe(32, 1, 2, 4, 2)], 'u2_k4_64x32'),                               # C_out = 32: wco 1, C_in = 64: wci 2 -> 3212
        (2, 4, 32, 16, [_pipe(16, 1, 2, 4, 2)], 'u2_k4_32x16'),                               # mf 16, wci 2 -> 1612
        (8, 16, 64, 64, [GEN32] * 8, 'u8_k16_64x64'),                                         # v2w_wg_ptq(8) == 0: one launch per phase, two taps each
        (2, 4, 16, 8, [GEN16] * 2, 'u2_k4_pad_16x8')):                                        # padded: generic, one launch per phase
    for _Lq in _lqs(_u):
        WGRAD_T += _both('%s_L%d' % (_tag, _Lq), _kern + [RED], c_in=_ci, c_out=_co, Lq=_Lq, k=_k, dil=1, u=_u)
WGRAD_T += _both('u4_k8_64x64_L50', [GEN32] * 4 + [RED], c_in=64, c_out=64, Lq=50, k=8, dil=1, u=4)       # Lq % 4 != 0: generic, four phases
# an odd k - u, which no layer of the generator has and every record above avoids: the only shapes at which pad = (k - u) / 2 rounds (down).
# u = 2, k = 5: pad 1, taps 1 and 3 on phase 0, taps 0, 2, 4 on phase 1; five taps have no u = 2 instantiation -> generic, one launch per phase.
# The layer's output has 2 Lq + 1 positions; dy holds the first 2 Lq.
for _Lq in (4, 132):
    WGRAD_T += _both('u2_k5_64x32_L%d' % _Lq, [GEN32] * 2 + [RED], c_in=64, c_out=32, Lq=_Lq, k=5, dil=1, u=2)

# ---------------------------------------------------------------------------------------------------------------
# v2w_wgrad, refusals (nothing launched).  `plan_ok`: v2w_wgrad_slabs, which sees neither k nor the pointers, still reports slabs.
WGRAD_REJECT = [
    _case('xa_without_xs', [], rc=E_ARG, B=3, c_in=64, c_out=64, Lq=128, k=3, dil=1, u=1, affine=True, no_xs=True, slope=SLOPE, n=0, plan_ok=True),
    # 7 x 7 = 49 weights per tap, no multiple of 4: no plan, 0 slabs.  (6 x 6 = 36 IS one: `gen_pad_6x6_k3` above.)
    _case('c7x7', [], rc=E_SHAPE, B=3, c_in=7, c_out=7, Lq=128, k=3, dil=1, u=1, affine=False, slope=1.0, n=0),
    _case('k65', [], rc=E_SHAPE, B=3, c_in=64, c_out=64, Lq=128, k=65, dil=1, u=1, affine=False, slope=1.0, n=0, plan_ok=True),
]

# ---------------------------------------------------------------------------------------------------------------
# v2w_wgrad_bf16 (wgb_plan: C_in == C_out, Lq % 8 == 0, odd k <= 11; C % 64 == 0 -> 64 x 64 tiles on 2 x 2 waves, every wave all taps of the
# launch, ceil(k / 7) balanced launches; C = 32 / 16 -> the waves share the taps, nt = 1 per wave for k <= 4, else 3; S = min(1024 or 512 / tiles, items)).
def _bf(mf, wco, wci, nt, stored):
    return 'wgrad_bf16_kernel<%d, %d, %d, %d, %s>' % (mf, wco, wci, nt, 'true' if stored == 'bf16' else 'false')


BRED = 'wgrad_bf16_reduce_kernel'


def _bf_all(id, kern, B=3, **kw):
    """fp32-stored and bf16-stored operands, each with and without the affine.  n = B Lq: the operands are rounded before the products."""
    out = []
    for stored in ('f32', 'bf16'):
        for aff in (True, False):
            out.append(_case('%s_%s_%s' % (id, stored, 'aff' if aff else 'plain'), [_bf(*a, stored) for a in kern] + [BRED], B=B, stored=stored,
                             affine=aff, slope=SLOPE, n=B * kw['Lq'], **kw))
    return out


WGRAD_BF16 = []
for _Lq in (8, 120, 128, 136):        # below one item, 8 short of one, one, one and 8
    for _C, _mf in ((16, 16), (32, 32)):
        # tap sharing: wave w takes taps 3 w .. 3 w + 2.  k = 5: wave 1 two taps, waves 2 and 3 none; k = 7: wave 2 one; k = 11: wave 3 two
        for _k, _dil in ((1, 1), (3, 1), (5, 1), (7, 1), (9, 1), (11, 1), (7, 2)):
            WGRAD_BF16 += _bf_all('ts%d_k%d_d%d_L%d' % (_C, _k, _dil, _Lq), [(_mf, 1, 1, 1 if _k <= 4 else 3)], C=_C, Lq=_Lq, k=_k, dil=_dil)
    # 2 x 2: hl = 9 (k 7, dil 3) and 15 (k 11, dil 3) -> hla 16, xc8 = (16 + 128 + hl + 7) / 8 = 20 <= 24
    for _k, _dil, _nts in ((1, 1, (1,)), (3, 1, (3,)), (5, 1, (5,)), (7, 3, (7,)), (9, 1, (5, 4)), (11, 3, (6, 5))):
        WGRAD_BF16 += _bf_all('c64_k%d_d%d_L%d' % (_k, _dil, _Lq), [(32, 2, 2, nt) for nt in _nts], C=64, Lq=_Lq, k=_k, dil=_dil)
    WGRAD_BF16 += _bf_all('c128_k3_L%d' % _Lq, [(32, 2, 2, 3)], C=128, Lq=_Lq, k=3, dil=1)            # 4 tiles
# S < items: C = 256 -> 16 tiles, S = 512 / 16 = 32; B = 3, Lq = 1408: 33 items, two per slab, the pair (10, 11) straddles b = 0 and b = 1
WGRAD_BF16 += _bf_all('S_below_items_c256', [(32, 2, 2, 3)], C=256, Lq=1408, k=3, dil=1)

WGRAD_BF16_REJECT = [
    _case('c48', [], rc=E_SHAPE, B=2, C=48, Lq=256, k=3, dil=1, stored='f32', affine=False, slope=SLOPE, n=0),
    _case('Lq_252', [], rc=E_SHAPE, B=2, C=32, Lq=252, k=3, dil=1, stored='f32', affine=False, slope=SLOPE, n=0),
    _case('k4', [], rc=E_SHAPE, B=2, C=32, Lq=256, k=4, dil=1, stored='f32', affine=False, slope=SLOPE, n=0),
    # hl = 35, hla = 40, xc8 = (40 + 128 + 35 + 7) / 8 = 26 > 24: wgb_plan (which sees no dilation) has a split count, the call declines
    _case('k11_d7', [], rc=E_SHAPE, B=2, C=32, Lq=256, k=11, dil=7, stored='f32', affine=False, slope=SLOPE, n=0, plan_ok=True),
    _case('x_plus4', [], rc=E_ARG, B=2, C=32, Lq=256, k=3, dil=1, stored='f32', affine=False, slope=SLOPE, n=0, x_off=4, plan_ok=True),
]

TABLE = dict(wgrad=WGRAD, wgrad_t=WGRAD_T, wgrad_reject=WGRAD_REJECT, wgrad_bf16=WGRAD_BF16, wgrad_bf16_reject=WGRAD_BF16_REJECT)


def is_bf16(c):
    return 'stored' in c


def slabs(c):
    """What the library asks for: partial slabs of k C_in C_out floats (0: no plan for the shape)."""
    lib = _hip.load()
    if is_bf16(c):
        return lib.v2w_wgrad_bf16_slabs(c['B'], c['C'], c['C'], c['Lq'], c['k'])
    return lib.v2w_wgrad_slabs(c['B'], c['c_in'], c['c_out'], c['Lq'])


def call(c, x, x_a, x_s, dy, dwf, slab, stream=None, sink=False):
    """One record's call on the given addresses: through the name sink (-> (rc, names)) or on `stream` (-> rc)."""
    lib = _hip.load()
    if is_bf16(c):
        fn, args = lib.v2w_wgrad_bf16, (x, x_a, x_s, dy, dwf, slab, c['B'], c['C'], c['C'], c['Lq'], c['k'], c['dil'], c['slope'],
                                        3 if c['stored'] == 'bf16' else 0)
    else:
        fn, args = lib.v2w_wgrad, (x, x_a, x_s, dy, dwf, slab, c['B'], c['c_in'], c['c_out'], c['Lq'], c['k'], c['dil'], c['u'], c['slope'])
    return _names(fn, *args) if sink else fn(*args, stream)


def dispatch(c):
    """Host-only dispatch of one record: (return code, kernel names).  The made-up pointers carry the record's alignment."""
    return call(c, X + c.get('x_off', 0), AUX2 if c['affine'] else None, AUX2 + 0x1000 if c['affine'] and not c.get('no_xs') else None,
                AUX, OUT, SLAB, sink=True)
