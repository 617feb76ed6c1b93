"""The cases of tests/test_bf16res_kernels_gpu.py: one record per call of v2w_branch_convs_bf16_fwd (conv_bf16_res_kernel,
csrc/v2w_conv_bf16_res.hip) and of v2w_convt1d_bf16_fwd with io_bf16 == 3 that lands on convt_bf16_res_kernel
(csrc/v2w_convt_bf16_res.hip), with the instantiation the call must launch, its return code and its chain lengths n.
tests/test_bf16res_ref_cpu.py drives every record through the name sink (and the transposed conv's configuration query) - host-only,
made-up pointers of the record's alignment - and asserts both; the GPU tests run the same records on real tensors.

Branch convs: conv_bf16_res_kernel<MI, NI, WM, WN, MODE>.  Read off launch_res: C % 128 == 0 takes (2, 4, 2, 2) (128 rows), every other
C % 64 == 0 (1, 4, 2, 2) (64 rows); both tiles are NT = 256 positions; the image of ALL C channels, (roundup4(h) + 256 + h rounded up to
4) rows of 64 bytes per 32-channel plane, plus (3 MT + 2 C) floats must fit 80 KiB (two workgroups per CU), h the largest halo
dil (k - 1) / 2 of the launch, h <= 32.  That serves C = 64 (h <= 32) and C = 128 (h <= 24) and nothing wider: four instantiations.

Transposed conv: convt_bf16_res_kernel<MI, NI, WM, WN, UP, U>, nine instantiations (RES_CT below) by the stride and C_out * UP; the two
stride-5 forms serve whole tiles of 64 positions only.

n: mode 0 k_j C + 3 per branch, mode 1 sum_j k_j C + 3 nbr + (out_div != 0) (short-chain: k_j for k_j C); transposed conv
ceil(k / u) C_in + 2 (tests/bf16res_ref.py)."""
import ctypes as C

import numpy as np
import torch

from wavthruvec_pytorch_amd import _hip

from tests import convbf16_cases as K
from tests import convbf16_ref as R
from tests import split_cases as S
from tests.disc_cases import OK, _case, ids  # noqa: F401  (ids: re-exported for the parametrisations)
from tests.split_cases import E_ARG, E_SHAPE

NT = 256
TILE = {128: (2, 4, 2, 2), 64: (1, 4, 2, 2)}
REACHABLE = {TILE[c] + (m,) for c in (128, 64) for m in (0, 1)}
GEN1, GEN2 = ((3, 1), (7, 1), (11, 1)), ((3, 3), (7, 3), (11, 3))          # the generator's first / second convs of a wide stage
MIX = ((3, 1), (7, 3), (11, 1))


def res_name(inst):
    return 'conv_bf16_res_kernel<%d, %d, %d, %d, %d>' % inst


def halo(kd):
    return max(d * (k - 1) // 2 for k, d in kd)


def branch(id, *, C, L, mode, kd, B=3, rc=OK, aff=None, bias=(True, True, True), out_div=0.0, slope=0.1, short=False, data=None,
           in_offb=0, out_offb=0, nbr=None, null=(), alloc_L=None):
    """One branch-conv record.  kd: ((k, dil), ...) one per branch.  aff: mode 0's input affine (default: present, but not on a short-chain
    or a `data` record); bias[j]: whether bias[j] is set; data: 'zeros' (an input with +0 and -0 sprinkled in) / 'neg' (all negative);
    nbr: the struct's nbr where it is not len(kd), null: struct fields left NULL ('wps1', 'in1', 'in_a', 'in_s'), alloc_L: the length the
    buffers really have (refusals with made-up sizes)."""
    aff = (mode == 0 and not short and data is None) if aff is None else aff
    assert not (aff and (short or mode != 0))
    per = 1 if short else C
    n = tuple(k * per + 3 for k, _ in kd) if mode == 0 else (sum(k * per + 3 for k, _ in kd) + (out_div != 0.0),)
    inst = TILE[128 if C % 128 == 0 else 64] + (mode,) if rc == OK else None
    return _case(id, [res_name(inst)] if rc == OK else [], rc, op='branch', inst=inst, C=C, L=L, mode=mode, kd=tuple(kd), B=B, aff=aff,
                 bias=tuple(bias), out_div=out_div, slope=slope, short=short, data=data, in_offb=in_offb, out_offb=out_offb,
                 nbr=len(kd) if nbr is None else nbr, null=tuple(null), alloc_L=alloc_L or L, n=n, h=halo(kd))


def _modes(id, **kw):
    """The record in both modes; mode 1 divides by the branch count as the generator does (unless the record says otherwise)."""
    m1 = dict(kw)
    m1.setdefault('out_div', float(len(kw['kd'])) if len(kw['kd']) > 1 else 0.0)
    return [branch(id + '_m0', mode=0, **kw), branch(id + '_m1', mode=1, **m1)]


# lengths: below a vector of positions per lane quad, a partial tile, one tile minus 4 / exact / plus 4, two tiles plus 4.  B = 3: the
# tile count is never a multiple of the 8 the grid is cut in
LENGTHS, HALOS, MIXED, SWITCHES, SHORT, THRESHOLDS, REFUSALS = [], [], [], [], [], [], []
for _c in (128, 64):
    for _L in (4, 20, 252, 256, 260, 516):
        LENGTHS += _modes('c%d_L%d' % (_c, _L), C=_c, L=_L, kd=MIX)
    # one branch per halo 0 .. 24: hla == h and hla > h with (hla - h) % 4 = 0, 3, 2, 1, 3, 2, 3, 2, 1, 0, 0; k = 1 starts the ring at c1 = 1
    for _k, _d in ((1, 1), (3, 1), (3, 2), (3, 3), (11, 1), (7, 2), (7, 3), (11, 2), (11, 3), (5, 8), (13, 4)):
        HALOS += _modes('c%d_k%d_d%d' % (_c, _k, _d), C=_c, L=260, kd=((_k, _d),))
    # branches of different halos in one launch (the row of tap 0 is hla - h_j, hla from the largest)
    for _n, _kd in (('mix', MIX), ('gen1', GEN1), ('gen2', GEN2), ('two', ((3, 2), (5, 4))), ('k1_k5', ((1, 1), (5, 1)))):
        MIXED += _modes('c%d_%s' % (_c, _n), C=_c, L=260, kd=_kd)
    _q = dict(C=_c, L=260, kd=MIX)
    SWITCHES += [branch('c%d_m0_no_aff' % _c, mode=0, aff=False, **_q),
                 branch('c%d_m0_no_aff_no_bias_two' % _c, mode=0, aff=False, bias=(False, False, False), C=_c, L=260, kd=MIX[:2])]
    for _m in (0, 1):
        _s = 'c%d_m%d_' % (_c, _m)
        _dv = 3.0 * _m
        SWITCHES += [branch(_s + 'no_bias', mode=_m, bias=(False, False, False), out_div=_dv, **_q),
                     branch(_s + 'bias1_null', mode=_m, bias=(True, False, True), out_div=_dv, **_q),
                     branch(_s + 'bias2_only', mode=_m, bias=(False, False, True), out_div=_dv, **_q),
                     branch(_s + 'slope025', mode=_m, slope=0.25, out_div=_dv, **_q),
                     branch(_s + 'slope1', mode=_m, slope=1.0, out_div=_dv, **_q),
                     branch(_s + 'zeros', mode=_m, data='zeros', out_div=_dv, **_q),
                     branch(_s + 'negative', mode=_m, data='neg', out_div=_dv, **_q)]
    SWITCHES += [branch('c%d_m1_div0' % _c, mode=1, out_div=0.0, **_q), branch('c%d_m1_div2' % _c, mode=1, out_div=2.0, **_q),
                 branch('c%d_m1_div2_two' % _c, mode=1, out_div=2.0, C=_c, L=260, kd=MIX[:2])]
    # short chains: one live input channel per item
    for _n, _kd in (('mix', MIX), ('k1', ((1, 1),)), ('gen2', GEN2)):
        SHORT += _modes('c%d_%s_short' % (_c, _n), C=_c, L=260, kd=_kd, short=True)
# the LDS thresholds of launch_res from both sides
THRESHOLDS += _modes('c128_h24', C=128, L=260, kd=((13, 4),)) + _modes('c64_h32', C=64, L=260, kd=((5, 16),))
THRESHOLDS += _modes('c128_h25', C=128, L=260, kd=((11, 5),), rc=E_SHAPE) + _modes('c64_h33', C=64, L=260, kd=((3, 33),), rc=E_SHAPE)
THRESHOLDS += _modes('c192', C=192, L=8, B=2, kd=((3, 1),), rc=E_SHAPE) + _modes('c256', C=256, L=8, B=2, kd=((3, 1),), rc=E_SHAPE)

# refusals: the documented code, nothing launched, every buffer's bits left alone
_R = dict(C=64, L=8, B=2, kd=MIX)
REFUSALS += _modes('even_k', rc=E_SHAPE, **dict(_R, kd=((3, 1), (4, 1))))
REFUSALS += _modes('L22', rc=E_SHAPE, **dict(_R, L=22))
REFUSALS += _modes('c96', rc=E_SHAPE, **dict(_R, C=96))
REFUSALS += [branch('mode2', mode=2, rc=E_ARG, aff=False, **_R)]
REFUSALS += _modes('nbr0', rc=E_ARG, nbr=0, **_R) + _modes('nbr4', rc=E_ARG, nbr=4, **_R)
REFUSALS += _modes('slope0', rc=E_ARG, slope=0.0, aff=False, **_R)
REFUSALS += _modes('in_plus8', rc=E_SHAPE, in_offb=8, **_R) + _modes('out_plus8', rc=E_SHAPE, out_offb=8, **_R)
REFUSALS += _modes('wps1_null', rc=E_ARG, null=('wps1',), **_R)
# C * L * 2 = 2^31 on buffers of 8 positions: the check stands in v2w_branch_convs_bf16_fwd ahead of launch_res (nothing is launched)
REFUSALS += _modes('lane_offsets_2g', rc=E_SHAPE, **dict(_R, C=128, L=1 << 23, alloc_L=8))
# the affine's halves come together (the kernel reads in_s whenever in_a is set); mode 1 takes neither, and still refuses a half
REFUSALS += _modes('in_s_null', rc=E_ARG, null=('in_s',), aff=False, **_R) + _modes('in_a_null', rc=E_ARG, null=('in_a',), aff=False, **_R)
REFUSALS += [branch('m1_in1_null', mode=1, rc=E_ARG, null=('in1',), **_R)]

BRANCH_TABLE = dict(lengths=LENGTHS, halos=HALOS, mixed=MIXED, switches=SWITCHES, short=SHORT, thresholds=THRESHOLDS, refusals=REFUSALS)
BRANCH_ALL = [c for cases in BRANCH_TABLE.values() for c in cases]


# ---------------------------------------------------------------------------------------------------------------
# operands on the CPU
def branch_operands(c):
    """dict: xs [n_in] (B, C, L) bf16 numbers, in_a / in_s (B, C) or None, wfs [nbr] [k][C][C], biases [nbr] (C) or None each, rounds."""
    rng = S._rng(c)
    B, Cc, L, nb = c['B'], c['C'], c['alloc_L'], len(c['kd'])

    def draw(*shape):
        return R.rne_bf16(S._f32(rng, *shape))
    xs = [draw(B, Cc, L) for _ in range(1 if c['mode'] == 0 else nb)]
    if c['data'] == 'neg':
        xs = [-x.abs() - 2.0 ** -10 for x in xs]
        xs = [R.rne_bf16(x) for x in xs]
    if c['data'] == 'zeros':
        for x in xs:
            x.view(-1)[::5] = 0.0
            x.view(-1)[2::5] = -0.0
    if c['short']:
        live = torch.zeros(B, Cc, 1, dtype=torch.bool)
        for b in range(B):
            live[b, K.live_channel(dict(B=B, ci=Cc), b)] = True
        xs = [torch.where(live, x, torch.zeros_like(x)) for x in xs]
    in_a = in_s = None
    rounds = 0
    if c['aff'] or 'in_a' in c['null'] or 'in_s' in c['null']:
        in_a, in_s = 1 + 0.2 * S._f32(rng, B, Cc), 0.2 * S._f32(rng, B, Cc)
    if c['aff']:
        xs[0], rounds = R.redraw(xs[0], c['slope'], in_a, in_s, lambda n: draw(n))
    wfs = [S._f32(rng, k, Cc, Cc, scale=1.0 / np.sqrt(Cc * k)) for k, _ in c['kd']]
    biases = [S._f32(rng, Cc) if c['bias'][j] else None for j in range(nb)]
    return dict(xs=xs, in_a=in_a, in_s=in_s, wfs=wfs, biases=biases, rounds=rounds)


def branch_reference(c, o, sel=None):
    """[(want, bound)] per output tensor (mode 0: one per branch; mode 1: one), on the batch items `sel` (default: all)."""
    from tests import bf16res_ref as Q
    pick = (lambda t: t) if sel is None else (lambda t: None if t is None else t[sel])
    dils = [d for _, d in c['kd']]
    bs = o['biases']
    if c['mode'] == 0:
        aff = dict(in_a=pick(o['in_a']), in_s=pick(o['in_s'])) if c['aff'] else {}
        return Q.first_convs(pick(o['xs'][0]), o['wfs'], dils, c['n'], slope=c['slope'], biases=bs, **aff)
    return [Q.second_convs([pick(x) for x in o['xs']], o['wfs'], dils, c['n'][0], slope=c['slope'], biases=bs, out_div=c['out_div'])]


FAKE = dict(in_=0x10000000, out=0x20000000, wps=0x30000000, bias=0x40000000, in_a=0x50000000, in_s=0x51000000)


def branch_struct(c, addr):
    """v2w_branch_convs_args; addr: in_ [..], out [..], wps [..], bias [..] lists of 16-byte aligned bases, in_a, in_s (0: NULL)."""
    a = _hip.BranchConvsArgs()
    nb = len(c['kd'])
    for j, (k, d) in enumerate(c['kd']):
        a.k[j], a.dil[j] = k, d
        a.wps[j] = None if 'wps%d' % j in c['null'] else addr['wps'][j]
        a.bias[j] = addr['bias'][j] if c['bias'][j] else None
    for j in range(1 if c['mode'] == 0 else nb):
        a.in_[j] = None if 'in%d' % j in c['null'] else addr['in_'][j] + c['in_offb']
    for j in range(nb if c['mode'] == 0 else 1):
        a.out[j] = addr['out'][j] + c['out_offb']
    a.in_a = addr['in_a'] if (c['aff'] or 'in_s' in c['null']) else None
    a.in_s = addr['in_s'] if (c['aff'] or 'in_a' in c['null']) else None
    a.nbr, a.mode, a.B, a.C, a.L = c['nbr'], c['mode'], c['B'], c['C'], c['L']
    a.slope, a.out_div = c['slope'], c['out_div']
    return a


def branch_dispatch(c):
    """Host-only: (return code, kernel names)."""
    addr = {q: [v + 0x1000000 * j for j in range(3)] for q, v in FAKE.items() if q not in ('in_a', 'in_s')}
    a = branch_struct(c, dict(addr, in_a=FAKE['in_a'], in_s=FAKE['in_s']))
    rc, names = _hip.kernel_names(_hip.load().v2w_branch_convs_bf16_fwd, C.byref(a))
    return (OK if rc == 100 else rc), names


# ---------------------------------------------------------------------------------------------------------------
# The resident transposed conv: (MI, NI, WM, WN, UP, U) -> (k, u) of the generator, the smallest C_out that reaches it
RES_CT = {(2, 4, 1, 4, 2, 2): (4, 2, 32), (1, 4, 1, 4, 2, 2): (4, 2, 16),
          (4, 2, 2, 2, 4, 4): (8, 4, 64), (2, 4, 2, 2, 4, 4): (8, 4, 32), (2, 4, 1, 4, 4, 4): (8, 4, 16),
          (4, 2, 2, 2, 8, 8): (16, 8, 32), (2, 4, 2, 2, 8, 8): (16, 8, 16),
          (5, 2, 4, 1, 5, 5): (11, 5, 128), (2, 2, 4, 1, 8, 5): (11, 5, 32)}


def ct_name(inst):
    return 'convt_bf16_res_kernel<%d, %d, %d, %d, %d, %d>' % inst


def ct_nt(inst):
    return 32 * inst[1] * inst[3]


def res_convt(id, inst, *, L, ci, co=None, B=3, bias=True, stats=True, slope=0.1):
    k, u, co0 = RES_CT[inst]
    c = K.convt(id, inst[:4], k=k, u=u, B=B, ci=ci, co=co or co0, L=L, io=3, stats=stats, slope=slope)
    c.update(kernels=[ct_name(inst)], cfg=inst[:4] + (32, True, 102, True, True), inst=inst, bias=bias)
    return c


CONVT = []
for _i, (_k, _u, _co) in RES_CT.items():
    _s = 'ct_%d_%d_%d_%d_up%d_u%d' % _i
    _nt = ct_nt(_i)
    # L: 4, one tile minus 4 / exact / plus 4, two tiles plus 4; stride 5 serves whole tiles of 64
    for _L in ((64, 128, 192) if _u == 5 else (4, _nt - 4, _nt, _nt + 4, 2 * _nt + 4)):
        CONVT.append(res_convt('%s_L%d' % (_s, _L), _i, L=_L, ci=64))
    _L = 128 if _u == 5 else _nt + 4
    CONVT.append(res_convt(_s + '_ci32_no_bias_slope1', _i, L=_L, ci=32, bias=False, slope=1.0))       # one plane: the nch == 1 path
    _ci = 128 if _nt <= 256 else 64                              # (four planes of a 512-position tile are past the LDS: the chunk kernel's)
    CONVT.append(res_convt('%s_ci%d_no_stats' % (_s, _ci), _i, L=_L, ci=_ci, stats=False))
    CONVT.append(res_convt(_s + '_ci32_no_stats_no_bias', _i, L=_L, ci=32, stats=False, bias=False))
CONVT.append(res_convt('ct_2_2_4_1_up8_u5_co96', (2, 2, 4, 1, 8, 5), L=64, ci=64, co=96))                # three row tiles, none of 128 channels
CONVT.append(res_convt('ct_5_2_4_1_up5_u5_co256', (5, 2, 4, 1, 5, 5), L=64, ci=32, co=256, B=2))         # two row tiles of the exact-phase form


def _fallback(id, tile, **kw):
    c = K.convt(id, tile, io=3, stats=False, **kw)
    c.update(inst=None, bias=True)
    return c


# what the resident kernel declines and conv_bf16_kernel takes: an odd plane count, a stride-5 length that is no whole tile, an `in` 8 bytes
# off (element-wise staging), a slope above 1 (fmaxf(x, slope x) is the leaky-relu for slope <= 1 only)
FALLBACK = [_fallback('fb_ci96', K.CT1, k=8, u=4, B=3, ci=96, co=16, L=260),
            _fallback('fb_u5_L68', K.CT1, k=11, u=5, B=3, ci=64, co=32, L=68),
            _fallback('fb_in_plus8', K.CT1, k=8, u=4, B=3, ci=64, co=16, L=260, in_offb=8),
            _fallback('fb_slope2', K.CT1, k=8, u=4, B=3, ci=64, co=16, L=260, slope=2.0)]
CONVT_ALL = CONVT + FALLBACK

ALL = BRANCH_ALL + CONVT_ALL
assert len({c['id'] for c in ALL}) == len(ALL)
