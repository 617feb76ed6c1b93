"""The cases of tests/test_stage_kernels_gpu.py: one record per call of v2w_resblock2_stage_fwd / _fwd_len / _wino_fwd / _wino_fwd_len /
_small_fwd and v2w_resblock_pair_fwd on the fused narrow-stage kernels (csrc/v2w_resblock_fused.hip, csrc/v2w_stage_small.hip), with the
kernel the call must launch (every template argument spelled out, as _hip.kernel_name_short prints it), its return code, the float offsets of
its operands from a 16-byte boundary and its operation counts.

tests/test_stage_ref_cpu.py drives every record through the name sink (host-only, made-up addresses) and asserts `kernels` and `rc`; the
GPU tests run the same records on real tensors.  `stage_struct` / `pair_array` build the argument structs for both from a table of
addresses, so the alignment of every operand - which selects the vector or the scalar path - is the same in the two runs.

The launcher's geometry, restated (`geometry`): h1max / h2max = the largest dil1 (k - 1) / 2 / dil2 (k - 1) / 2 of the branches; windows of
W = 128 positions while B * ceil(L / nto256) < 224 and 128 - 2 h2max >= 64, nto256 = (256 - 2 h2max) & ~3, else of 256; a tile keeps
nto = (W - 2 h2max) & ~3 outputs and, with the tail, advances by nadv = (nto - 2 hout) & ~3, hout = (post_k - 1) / 2.  With the standard set
(k 3 / 7 / 11, dil2 3) nto is 96 and 224, nadv with post_k = 7 is 88 and 216.  The pair kernel always takes W = 256 with its own h2; the
8-channel kernel W = 512, nto = 512 - 2 h2max.  Templates: resblock2_stage_kernel<C, W / (4 C), 4, POST, BWD, LEN>,
resblock2_stage_wino_kernel<W / 64, LEN>, resblock_pair_kernel<C, 256 / (4 C), 4>.

Operation counts (the bound of a conv phase is n * 2^-24 * S, tests/stage_ref.py): n = k * C products plus, per entry, one for each fp32
operation around them - phase 1: input affine 1 (one fma), leaky-relu 1, bias 1, residual 1; phase 2: leaky-relu 1, bias 1, residual 1 (in the
ResBlock1 pair the residual is x: + 1 for its affine, and phase 1 has none).  Winograd form: segments * C products per class + 2 + 1 + 2
(weight, input and output transform) in place of k * C.  Gradient form: affine 1, mask factor 1, residual 1 / mask factor 1, residual 1 (the
masks' own affine adds none: only a sign is taken from it).  Tail: post_k * C + leaky-relu 1 + bias 1.  Addends of the pair: one addition each."""
import ctypes as C

from wavthruvec_pytorch_amd import _hip

from tests.disc_cases import OK, _case, ids  # noqa: F401  (ids: re-exported for the parametrisations)
from tests.disc_ref import ceil_div
from tests.wino_ref import segments

E_ARG, E_SHAPE = -1, -2
STD = ((3, 1, 3), (7, 1, 3), (11, 1, 3))            # (k, dil1, dil2) per branch: the generator's ResBlock2 set
ALL = ('in_aff', 'bias')


def halos(br):
    return max(d1 * (k - 1) // 2 for k, d1, _ in br), max(d2 * (k - 1) // 2 for k, _, d2 in br)


def geometry(form, B, L, br, post_k=0):
    """dict(W, nto, nadv, hout, h1max, h2max, ntl) of the launch, from its sizes alone."""
    h1max, h2max = halos(br)
    if form == 'small':
        W, nto = 512, 512 - 2 * h2max
    elif form == 'pair':
        W, nto = 256, (256 - 2 * h2max) & ~3
    else:
        nto256 = (256 - 2 * h2max) & ~3
        W = 128 if nto256 > 0 and B * ceil_div(L, nto256) < 224 and 128 - 2 * h2max >= 64 else 256
        nto = (W - 2 * h2max) & ~3
    hout = (post_k - 1) // 2 if post_k else 0
    nadv = (nto - 2 * hout) & ~3 if post_k else nto
    return dict(W=W, nto=nto, nadv=nadv, hout=hout, h1max=h1max, h2max=h2max, ntl=ceil_div(L, nadv))


def _b(v):
    return 'true' if v else 'false'


def stage_name(Cc, W, post=False, bwd=False, len_=False):
    return 'resblock2_stage_kernel<%d, %d, 4, %s, %s, %s>' % (Cc, W // (4 * Cc), _b(post), _b(bwd), _b(len_))


def wino_name(W, len_=False):
    return 'resblock2_stage_wino_kernel<%d, %s>' % (W // 64, _b(len_))


def pair_name(Cc):
    return 'resblock_pair_kernel<%d, %d, 4>' % (Cc, 256 // (4 * Cc))


SMALL_NAME = 'small_stage_kernel'


def stage(id, form, *, C, B, L, W=None, br=STD, flags=ALL, slope=0.1, out_div=3.0, post_k=0, post_b=True, post_slope=0.01, no_out=False,
          lens=None, len_mul=1, offs=(), bwd=None, rc=OK):
    """One record of the section.  form: 'direct' (v2w_resblock2_stage_fwd[_len]), 'wino', 'small'.  W: the window the record must run on
    (checked against `geometry`).  flags: 'in_aff' (in_a / in_s given), 'bias' (every b1_j / b2_j given).  post_k > 0: the fused tail
    (post_b: its bias given; no_out: `out` NULL).  lens: B per-item lengths in units of len_mul positions.  offs: the operands ('in_', 'out',
    'post_out', 'in_a') whose base lies one float past a 16-byte boundary.  bwd: None or dict(aff=.., rowsum=.., slope=..): the gradient form."""
    flags, offs = frozenset(flags), frozenset(offs)
    assert flags <= set(ALL) and offs <= {'in_', 'out', 'post_out', 'in_a'} and (lens is None or len(lens) == B)
    kernels, g = [], None
    if rc == OK:
        g = geometry(form, B, L, br, post_k)
        assert W == g['W'], (id, g)
        kernels = [SMALL_NAME if form == 'small' else wino_name(W, lens is not None) if form == 'wino' else
                   stage_name(C, W, bool(post_k), bwd is not None, lens is not None)]
    aff, bias, act = 'in_aff' in flags, 'bias' in flags, slope != 1.0
    if bwd is None:
        ops1, ops2 = aff + act + bias + 1, act + bias + 1
    else:
        ops1, ops2 = aff + (bwd['slope'] != 1.0) + 1, (bwd['slope'] != 1.0) + 1
    prods = [(len(segments(k)) * C + 5) if form == 'wino' else k * C for k, _, _ in br]
    return _case(id, kernels, rc, op='stage', form=form, C=C, B=B, L=L, W=W, br=tuple(br), flags=flags, slope=slope, out_div=out_div,
                 post_k=post_k, post_b=post_b, post_slope=post_slope, no_out=no_out, lens=lens, len_mul=len_mul, offs=offs, bwd=bwd, geom=g,
                 ops=(ops1, ops2), n1=tuple(p + ops1 for p in prods), n2=tuple(p + ops2 for p in prods),
                 n_p=post_k * C + (post_slope != 1.0) + bool(post_b))


def pair(id, *, C, B, L, ks, d1=1, d2=3, res_mode=0, flags=ALL, adds=0, slope=0.1, out_div=0.0, offs=(), rc=OK):
    """One launch of v2w_resblock_pair_fwd: a problem per entry of ks.  adds: 0, 1 (add0) or 2 (add0 + add1)."""
    flags, offs = frozenset(flags), frozenset(offs)
    aff, bias, act = 'in_aff' in flags, 'bias' in flags, slope != 1.0
    ops1 = aff + act + bias + (res_mode == 0)
    ops2 = act + bias + 1 + (aff if res_mode == 1 else 0)
    return _case(id, [pair_name(C)] if rc == OK else [], rc, op='pair', form='pair', C=C, B=B, L=L, ks=tuple(ks), d1=d1, d2=d2, res_mode=res_mode,
                 flags=flags, adds=adds, slope=slope, out_div=out_div, offs=offs, ops=(ops1, ops2),
                 n1=tuple(k * C + ops1 for k in ks), n2=tuple(k * C + ops2 for k in ks), n_add=adds)


# ---------------------------------------------------------------------------------------------------------------
# Lengths on every window of every kernel: 1, 4, 5 (shorter than every halo), step - 1, step, step + 1, step + 4, 2 step + 4, step + 7
# (L % 4 != 0: scalar staging and stores), step = nto, or nadv with the tail.  Windows of 128: B = 2.  Windows of 256: the smallest B with
# B * ceil(L / nto256) >= 224 - at L = nto256 + 4 that is B = 112, 224 tiles exactly, and B = 111 stays on 128.
def _b256(L, nto256=224):
    return ceil_div(224, ceil_div(L, nto256))


VARIANTS = (('d32', dict(form='direct', C=32)), ('d16', dict(form='direct', C=16)), ('wino', dict(form='wino', C=32)),
            ('post16', dict(form='direct', C=16, post_k=7)))
LENGTHS = []
for _v, _kw in VARIANTS:
    for _W in (128, 256):
        _step = geometry('direct', 1 if _W == 128 else 224, 1, STD, _kw.get('post_k', 0))['nadv']
        for _L in (1, 4, 5, _step - 1, _step, _step + 1, _step + 4, 2 * _step + 4, _step + 7):
            LENGTHS.append(stage('%s_w%d_L%d' % (_v, _W, _L), B=2 if _W == 128 else _b256(_L), L=_L, W=_W, **_kw))
    LENGTHS.append(stage('%s_B111_stays_on_128' % _v, B=111, L=228, W=128, **_kw))
    LENGTHS.append(stage('%s_B112_takes_256' % _v, B=112, L=228, W=256, **_kw))

# ---------------------------------------------------------------------------------------------------------------
# Alignment: `in`, `out`, `post_out`, `in_a` each 4 bytes past a 16-byte boundary, one at a time, at a length that would take the vector path
ALIGN = []
for _v, _kw in VARIANTS:
    for _W in (128, 256):
        _L = 100 if _W == 128 else 228
        for _o in ('in_', 'out', 'in_a') + (('post_out',) if 'post_k' in _kw else ()):
            if _o == 'out' and 'post_k' in _kw:
                continue                                                 # (the tail does not write `out`)
            ALIGN.append(stage('%s_w%d_%s_plus4' % (_v, _W, _o.rstrip('_')), B=2 if _W == 128 else 112, L=_L, W=_W, offs=(_o,), **_kw))

# ---------------------------------------------------------------------------------------------------------------
# Branch sets and optional operands (out_div stays 3 whatever nk is: a division by nk would show)
MIXED4 = ((3, 2, 1), (7, 3, 1), (5, 1, 2), (11, 1, 3))      # d1 != 1: h1max = 9, h2max = 15
BRANCHES = []
for _C in (32, 16):
    def _e(id, **kw):
        kw = dict(dict(form='direct', C=_C, B=2, L=200, W=128), **kw)
        BRANCHES.append(stage('d%d_%s' % (_C, id), **kw))
    _e('nk1', br=((3, 1, 1),), out_div=0.0)
    _e('nk4_mixed', br=MIXED4)
    _e('nk4_mixed_w256', br=MIXED4, B=112, L=228, W=256)
    _e('h1max32', br=((3, 32, 1), (5, 16, 1)))
    _e('h2max32', br=((3, 1, 32), (5, 1, 16)))                            # nto = 64 = W / 2 on the windows of 128
    _e('h2max64', br=((3, 1, 64), (5, 1, 32)), L=132, W=256)            # h2max > 32: windows of 256 whatever the size; nto = 128 = W / 2
    _e('no_affine', flags=('bias',))
    _e('no_bias', flags=('in_aff',))
    _e('bare', flags=(), out_div=0.0, slope=1.0)
    _e('out_div0', out_div=0.0)
for _pk in (1, 3, 9):
    BRANCHES.append(stage('post16_k%d' % _pk, 'direct', C=16, B=2, L=200, W=128, post_k=_pk))
    BRANCHES.append(stage('post16_k%d_w256' % _pk, 'direct', C=16, B=112, L=228, W=256, post_k=_pk))
BRANCHES.append(stage('post16_no_post_b', 'direct', C=16, B=2, L=200, W=128, post_k=7, post_b=False))
BRANCHES.append(stage('post16_out_null', 'direct', C=16, B=2, L=200, W=128, post_k=7, no_out=True))
BRANCHES.append(stage('post16_slope1_div0', 'direct', C=16, B=2, L=203, W=128, post_k=7, post_slope=1.0, out_div=0.0))
BRANCHES.append(stage('wino_nk1', 'wino', C=32, B=2, L=200, W=128, br=((3, 1, 1),), out_div=0.0))
BRANCHES.append(stage('wino_nk4_d2_mixed', 'wino', C=32, B=2, L=200, W=128, br=((3, 1, 1), (5, 1, 2), (7, 1, 3), (11, 1, 3))))
BRANCHES.append(stage('wino_bare', 'wino', C=32, B=2, L=200, W=128, flags=(), out_div=0.0, slope=1.0))
BRANCHES.append(stage('wino_no_affine_w256', 'wino', C=32, B=112, L=228, W=256, flags=('bias',)))

# ---------------------------------------------------------------------------------------------------------------
# Per-item lengths: 0, 1, inside a tile, on a tile seam, L, past L (clamped); len_mul = 2; L % 4 != 0.  Inputs past the end hold NaN.
LENS = []
for _v, _kw in VARIANTS:
    _s1, _s2 = (geometry('direct', _Bq, 1, STD, _kw.get('post_k', 0))['nadv'] for _Bq in (1, 224))
    LENS.append(stage('%s_len' % _v, B=6, L=2 * _s1 + 4, W=128, lens=[0, 1, 50, _s1, 2 * _s1 + 4, 300], **_kw))
    LENS.append(stage('%s_len_mul2' % _v, B=6, L=2 * _s1 + 4, W=128, lens=[0, 1, 25, _s1 // 2, _s1 + 2, 150], len_mul=2, **_kw))
    LENS.append(stage('%s_len_scalar' % _v, B=6, L=2 * _s1 + 7, W=128, lens=[0, 1, 50, _s1, 2 * _s1 + 7, 300], **_kw))
    LENS.append(stage('%s_len_w256' % _v, B=114, L=228, W=256, lens=[0, 1, 100, _s2, 228, 400] * 19, **_kw))
LENS.append(stage('d16_len_in_plus4', 'direct', C=16, B=6, L=196, W=128, lens=[0, 1, 50, 96, 196, 300], offs=('in_',)))

# ---------------------------------------------------------------------------------------------------------------
# Gradient form: both channel counts and windows; bwd_mask2 with and without its affine; with and without bwd_rowsum
GRAD = []
for _C in (32, 16):
    for _W, _B, _Ls in ((128, 2, (5, 100, 103, 196)), (256, 112, (228,))):
        for _L in _Ls:
            for _aff, _rs in ((True, True), (False, False)) if _L in (100, 228) else ((_L != 103, _L != 5),):
                GRAD.append(stage('g%d_w%d_L%d_%s_%s' % (_C, _W, _L, 'aff' if _aff else 'noaff', 'rows' if _rs else 'norows'), 'direct', C=_C,
                                  B=_B, L=_L, W=_W, flags=('in_aff',), slope=1.0, out_div=0.0, bwd=dict(aff=_aff, rowsum=_rs, slope=0.1)))
GRAD.append(stage('g16_nk4_mixed', 'direct', C=16, B=2, L=200, W=128, br=MIXED4, flags=('in_aff',), slope=1.0, out_div=0.0,
                  bwd=dict(aff=True, rowsum=True, slope=0.1)))
GRAD.append(stage('g32_no_in_affine_slope1', 'direct', C=32, B=2, L=100, W=128, flags=(), slope=1.0, out_div=0.0,
                  bwd=dict(aff=False, rowsum=True, slope=1.0)))

# ---------------------------------------------------------------------------------------------------------------
# Pair: both res_modes, one and four problems (a k each), the addends, the lengths around its own nto (236 at k 7, dil2 3)
PAIR = []
for _C in (32, 16):
    for _L in (1, 5, 235, 236, 237, 240, 476, 243):
        PAIR.append(pair('p%d_L%d' % (_C, _L), C=_C, B=2, L=_L, ks=(7,), res_mode=_L % 2))
    for _m in (0, 1):
        PAIR.append(pair('p%d_mode%d_n4_add0' % (_C, _m), C=_C, B=2, L=300, ks=(3, 7, 11, 5), res_mode=_m, adds=1, out_div=3.0))
        PAIR.append(pair('p%d_mode%d_add01' % (_C, _m), C=_C, B=2, L=300, ks=(7,), res_mode=_m, adds=2, out_div=3.0))
        PAIR.append(pair('p%d_mode%d_bare' % (_C, _m), C=_C, B=2, L=303, ks=(7,), res_mode=_m, flags=(), slope=1.0))
    PAIR.append(pair('p%d_in_plus4' % _C, C=_C, B=2, L=300, ks=(7,), offs=('in_',)))
PAIR.append(pair('p64_refused', C=64, B=2, L=300, ks=(7,), rc=E_SHAPE))
PAIR.append(pair('p32_even_k_refused', C=32, B=2, L=300, ks=(4,), rc=E_SHAPE))
PAIR.append(pair('p32_wide_field_refused', C=32, B=2, L=300, ks=(3,), d2=65, rc=E_SHAPE))           # nto = 124 < W / 2

# ---------------------------------------------------------------------------------------------------------------
# The 8-channel kernel: nto = 482 with the standard set
SMALL = [stage('s8_L%d' % _L, 'small', C=8, B=2, L=_L, W=512) for _L in (1, 5, 481, 482, 483, 968, 489)]
SMALL += [stage('s8_nk1', 'small', C=8, B=2, L=300, W=512, br=((3, 1, 1),), out_div=0.0),
          stage('s8_nk4_mixed', 'small', C=8, B=2, L=600, W=512, br=MIXED4),
          stage('s8_halo32', 'small', C=8, B=2, L=600, W=512, br=((3, 32, 1), (3, 1, 32))),
          stage('s8_bare', 'small', C=8, B=2, L=300, W=512, flags=(), slope=1.0, out_div=0.0),
          stage('s8_in_plus4', 'small', C=8, B=2, L=300, W=512, offs=('in_',))]

# ---------------------------------------------------------------------------------------------------------------
# Refusals, with the exact code: nothing is launched, every buffer keeps its bits
_G = dict(flags=('in_aff',), slope=1.0, out_div=0.0)
REFUSALS = [
    stage('d32_k1', 'direct', C=32, B=2, L=100, br=((1, 1, 1),), rc=E_SHAPE),
    stage('d16_k1', 'direct', C=16, B=2, L=100, br=((1, 1, 1),), rc=E_SHAPE),
    stage('d32_h1max33', 'direct', C=32, B=2, L=100, br=((3, 33, 1),), rc=E_SHAPE),
    stage('d16_h1max33', 'direct', C=16, B=2, L=100, br=((3, 33, 1),), rc=E_SHAPE),
    stage('d32_h2max65', 'direct', C=32, B=2, L=100, br=((3, 1, 65),), rc=E_SHAPE),              # nto = 124 < W / 2
    stage('d16_h2max65', 'direct', C=16, B=2, L=100, br=((3, 1, 65),), rc=E_SHAPE),
    stage('d32_even_k', 'direct', C=32, B=2, L=100, br=((3, 1, 1), (4, 1, 1)), rc=E_SHAPE),
    stage('d64', 'direct', C=64, B=2, L=100, rc=E_SHAPE),
    stage('post_on_c32', 'direct', C=32, B=2, L=100, post_k=7, rc=E_SHAPE),
    stage('post_k11', 'direct', C=16, B=2, L=100, post_k=11, rc=E_SHAPE),
    stage('post_k4', 'direct', C=16, B=2, L=100, post_k=4, rc=E_SHAPE),
    stage('grad_with_bias', 'direct', C=16, B=2, L=100, **dict(_G, flags=ALL), bwd=dict(aff=True, rowsum=True, slope=0.1), rc=E_ARG),
    stage('grad_with_slope', 'direct', C=32, B=2, L=100, **dict(_G, slope=0.1), bwd=dict(aff=True, rowsum=True, slope=0.1), rc=E_ARG),
    stage('grad_with_lens', 'direct', C=16, B=2, L=100, **_G, lens=[50, 100], bwd=dict(aff=True, rowsum=False, slope=0.1), rc=E_ARG),
    stage('grad_with_tail', 'direct', C=16, B=2, L=100, **_G, post_k=7, bwd=dict(aff=True, rowsum=False, slope=0.1), rc=E_ARG),
    stage('len_mul0', 'direct', C=16, B=2, L=100, lens=[50, 100], len_mul=0, rc=E_ARG),
    stage('wino_c16', 'wino', C=16, B=2, L=100, rc=E_SHAPE),
    stage('wino_dil1_3', 'wino', C=32, B=2, L=100, br=((3, 3, 1),), rc=E_SHAPE),
    stage('wino_even_k', 'wino', C=32, B=2, L=100, br=((4, 1, 1),), rc=E_SHAPE),
    stage('wino_dil2_5_pairs_short', 'wino', C=32, B=2, L=100, br=((3, 1, 5),), rc=E_SHAPE),     # kept outputs reach column 121, the pairs cover 120
    stage('wino_with_tail', 'wino', C=32, B=2, L=100, post_k=7, rc=E_SHAPE),
    stage('s8_c16', 'small', C=16, B=2, L=100, rc=E_SHAPE),
    stage('s8_halo33', 'small', C=8, B=2, L=100, br=((3, 1, 33),), rc=E_SHAPE),
    stage('s8_halo1_33', 'small', C=8, B=2, L=100, br=((3, 33, 1),), rc=E_SHAPE),
    stage('s8_even_k', 'small', C=8, B=2, L=100, br=((4, 1, 1),), rc=E_SHAPE),
]

TABLE = dict(lengths=LENGTHS, align=ALIGN, branches=BRANCHES, lens=LENS, grad=GRAD, pair=PAIR, small=SMALL, refusals=REFUSALS)
EVERY = [c for cases in TABLE.values() for c in cases]
assert len({c['id'] for c in EVERY}) == len(EVERY)

# every instantiation the library has of these kernels (tests/test_stage_ref_cpu.py checks that each appears in a record)
INSTANTIATIONS = ([stage_name(Cc, W, len_=ln) for Cc in (32, 16) for W in (128, 256) for ln in (False, True)] +
                  [stage_name(Cc, W, bwd=True) for Cc in (32, 16) for W in (128, 256)] +
                  [stage_name(16, W, post=True, len_=ln) for W in (128, 256) for ln in (False, True)] +
                  [wino_name(W, ln) for W in (128, 256) for ln in (False, True)] + [pair_name(32), pair_name(16), SMALL_NAME])


# ---------------------------------------------------------------------------------------------------------------
# the argument structs, from a table of addresses (made up here, real ones in the GPU tests)
SCALARS = ('in_', 'in_a', 'in_s', 'out', 'post_w', 'post_b', 'post_out', 'mask2', 'mask2_a', 'mask2_s', 'len', 'add0', 'add1')
PER_BRANCH = ('wp1', 'b1', 'wp2', 'b2', 'mask1', 'mid', 'rowsum')


def fake_addresses(c):
    """16-byte aligned addresses nothing reads: one table per problem (a stage record is one problem)."""
    n = len(c['ks']) if c['op'] == 'pair' else 1
    out = []
    for i in range(n):
        a = {name: 0x10000000 * (i + 1) + 0x800000 * j for j, name in enumerate(SCALARS)}
        a.update({name: [0x50000000 + 0x4000000 * j + 0x400000 * q + 0x100000 * i for q in range(4)] for j, name in enumerate(PER_BRANCH)})
        out.append(a)
    return out


def _at(c, addr, name):
    return addr[name] + 4 * (name in c['offs'])


def stage_struct(c, addr):
    a = _hip.StageArgs()
    a.in_ = _at(c, addr, 'in_')
    if 'in_aff' in c['flags']:
        a.in_a, a.in_s = _at(c, addr, 'in_a'), addr['in_s']
    for j, (k, d1, d2) in enumerate(c['br']):
        a.wp1[j], a.wp2[j], a.k[j], a.dil1[j], a.dil2[j] = addr['wp1'][j], addr['wp2'][j], k, d1, d2
        if 'bias' in c['flags']:
            a.bias1[j], a.bias2[j] = addr['b1'][j], addr['b2'][j]
    a.out = None if c['no_out'] else _at(c, addr, 'out')
    a.nk, a.B, a.C, a.L, a.slope, a.out_div = len(c['br']), c['B'], c['C'], c['L'], c['slope'], c['out_div']
    if c['post_k']:
        a.post_w, a.post_out, a.post_k, a.post_slope = addr['post_w'], _at(c, addr, 'post_out'), c['post_k'], c['post_slope']
        a.post_b = addr['post_b'] if c['post_b'] else None
    if c['bwd'] is not None:
        for j in range(len(c['br'])):
            a.bwd_mask1[j], a.bwd_mid[j] = addr['mask1'][j], addr['mid'][j]
            a.bwd_rowsum[j] = addr['rowsum'][j] if c['bwd']['rowsum'] else None
        a.bwd_mask2, a.bwd_slope = addr['mask2'], c['bwd']['slope']
        if c['bwd']['aff']:
            a.bwd_mask2_a, a.bwd_mask2_s = addr['mask2_a'], addr['mask2_s']
    return a


def pair_array(c, addrs):
    arr = (_hip.PairArgs * len(c['ks']))()
    for p, addr, k in zip(arr, addrs, c['ks']):
        p.in_, p.wp1, p.wp2, p.out = _at(c, addr, 'in_'), addr['wp1'][0], addr['wp2'][0], addr['out']
        if 'in_aff' in c['flags']:
            p.in_a, p.in_s = addr['in_a'], addr['in_s']
        if 'bias' in c['flags']:
            p.bias1, p.bias2 = addr['b1'][0], addr['b2'][0]
        if c['adds'] >= 1:
            p.add0 = addr['add0']
        if c['adds'] >= 2:
            p.add1 = addr['add1']
        p.B, p.C, p.L, p.k, p.dil1, p.dil2 = c['B'], c['C'], c['L'], k, c['d1'], c['d2']
        p.res_mode, p.slope, p.out_div = c['res_mode'], c['slope'], c['out_div']
    return arr


def bwd_rows(c):
    """Rows of every bwd_rowsum[j] of a gradient-form record: the library's own answer."""
    return _hip.load().v2w_resblock2_stage_bwd_rows(C.byref(stage_struct(c, fake_addresses(c)[0])))


def call(c, addrs, stream=None):
    """Run the record's entry point on the given addresses: with a stream for real, without one through the name sink -> (rc, kernel names)."""
    lib = _hip.load()
    if c['op'] == 'pair':
        fn, args = lib.v2w_resblock_pair_fwd, (pair_array(c, addrs), len(c['ks']))
    else:
        a = stage_struct(c, addrs[0])
        fn = {'direct': lib.v2w_resblock2_stage_fwd, 'wino': lib.v2w_resblock2_stage_wino_fwd, 'small': lib.v2w_resblock2_stage_small_fwd}[c['form']]
        args = (C.byref(a),)
        if c['lens'] is not None:
            assert c['form'] != 'small'
            fn = lib.v2w_resblock2_stage_fwd_len if c['form'] == 'direct' else lib.v2w_resblock2_stage_wino_fwd_len
            args = (C.byref(a), addrs[0]['len'], c['len_mul'])
    if stream is None:
        return _hip.kernel_names(fn, *args)
    return fn(*args, stream), None


def dispatch(c):
    """Host-only: (return code, kernels) of the record.  A process without a GPU reports hipErrorNoDevice (100) from the launch status
    behind the (recorded) launch: counted as OK."""
    rc, names = call(c, fake_addresses(c))
    return (OK if rc == 100 else rc), names
