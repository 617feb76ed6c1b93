"""The cases of tests/test_split_kernels_gpu.py: one record per call of v2w_conv1d_fwd / _fwd_multi with V2W_ALGO_SPLIT (and V2W_ALGO_BF16
where the call lands on the same kernel) on csrc/v2w_conv_split.hip, and per call of v2w_resblock2_stage_split_fwd on
csrc/v2w_stage_split.hip, with the kernels the call must launch, its return code and its chain lengths n (one per problem).

tests/test_split_ref_cpu.py drives every record through the name sink (host-only, made-up pointers) and asserts `kernels` and `rc`; the GPU
tests run the same records on real tensors.  `conv_array` / `stage_struct` build the argument structs for both from a table of addresses,
so the alignment of every operand - which selects the vector or scalar path - is the same in the two runs.  `operands` draws a record's
tensors on the CPU, for both as well.  Kernel names: conv_split_kernel<MI, NI, WM, WN, VEC, BF, HM>, stage_split_kernel<NCH, NI, WN, BF>.

n (tests/split_ref.py has the bound): three accumulations per product, 3 k C_in, plus `ops` counted per switch exactly as
tests/tile_cases.py counts them; a short-chain record (one live input channel per item, every other channel exactly zero, no input affine)
has 3 k + ops; the bf16 records k C_in + ops (k + ops).  A short-chain STAGE record has 3 k + ops in its first conv only: t1 is dense over
the channels, so the second conv keeps 3 k C + ops.

bf16 operands on this file's kernels: v2w_conv1d_bf16 declines C_in % 32 != 0 and in_stride > 1, so an fp32-tensor V2W_ALGO_BF16 call with
C_in = 16 or 48 and C_out % 64 == 0 does reach conv_split_kernel<..., true, 32> (every tile, vector and scalar): the BF16 records."""
import ctypes as C

import numpy as np
import torch

from wavthruvec_pytorch_amd import _hip

from tests import disc_ref as D
from tests.disc_cases import OK, _case, ids  # noqa: F401  (ids: re-exported for the parametrisations)
from tests.tile_cases import OPS

E_ARG, E_SHAPE = -1, -2
F16_MAX = 65504.0
MASK_MIN = 2.0 ** -10

# (MI, NI, WM, WN, HM) and the positions per tile NT = 32 * NI * WN
T128, T64, T256, W128, W64 = (2, 2, 2, 2, 32), (1, 2, 2, 2, 32), (2, 2, 1, 4, 32), (2, 2, 2, 2, 40), (1, 2, 2, 2, 40)
NT = {T128: 128, T64: 128, T256: 256, W128: 128, W64: 128}
TNAME = {T128: 't128', T64: 't64', T256: 't256', W128: 'w128', W64: 'w64'}


def tile_name(tile, vec=True, bf=False):
    return 'conv_split_kernel<%d, %d, %d, %d, %s, %s, %d>' % (tile[:4] + ('true' if vec else 'false', 'true' if bf else 'false', tile[4]))


def conv(id, tile, *, B, ci, co, L, k, dil=1, vec=None, rc=OK, flags=(), slope=0.1, pad_left=-1, out_div=0.0, out_slope=0.0, mask_slope=0.1,
         in_stride=1, in_phase=0, in_ct=0, in_g=0, out_ct=0, out_g=0, in_off=0, out_off=0, short=False, data=None, bf=False, null=(),
         L_alt=None):
    """One conv record.  k: an int or a tuple (one problem per entry: _fwd_multi).  flags: the switches of tile_cases.OPS.  in_off / out_off:
    floats between a 16-byte boundary and the base of `in` / `out`.  short: one live input channel per item (b % C_in).  data: the operand
    range (see `operands`).  bf: V2W_ALGO_BF16.  null: arguments left NULL.  L_alt: the L of every problem but the first (a refusal)."""
    ks = k if isinstance(k, tuple) else (k,)
    flags = frozenset(flags)
    assert flags <= set(OPS) - {'rowsum'} and not ({'acc', 'add0'} <= flags) and not (short and 'in_aff' in flags) and not (bf and 'in_aff' in flags)
    ops = sum(OPS[f] for f in flags) + (slope != 1.0) + (out_div != 0.0) + (out_slope not in (0.0, 1.0))
    vec = (L % 4 == 0 and L >= 4 and in_off == 0 and in_stride == 1) if vec is None else vec
    live = 1 if short else ci
    kernels = [] if rc != OK else [tile_name(tile, vec, bf)]
    return _case(id, kernels, rc, op='conv', tile=tile, B=B, ci=ci, co=co, L=L, ks=ks, dil=dil, flags=flags, slope=slope, pad_left=pad_left,
                 out_div=out_div, out_slope=out_slope, mask_slope=mask_slope, in_stride=in_stride, in_phase=in_phase, in_ct=in_ct, in_g=in_g,
                 out_ct=out_ct, out_g=out_g, in_off=in_off, out_off=out_off, short=short, data=data, bf=bf, null=tuple(null), L_alt=L_alt,
                 ops=ops, n=tuple((1 if bf else 3) * kk * live + ops for kk in ks), big=B * co * L * ci * max(ks) > 1 << 27)


def dgrad(c, tile):
    """The input gradient of a plain record: the same conv of a (B, C_out, L) cotangent with the transposed, tap-reversed weights
    (disc_ref.transpose_flip), the taps left of the output now the forward's right ones."""
    k, dil = c['ks'][0], c['dil']
    left = c['pad_left'] if c['pad_left'] >= 0 else dil * (k - 1) // 2
    d = dict(c, id=c['id'] + '_dgrad', ci=c['co'], co=c['ci'], pad_left=(k - 1) * dil - left, slope=1.0, flags=frozenset(), wT=True, tile=tile)
    d['ops'], d['n'], d['kernels'] = 0, (3 * k * c['co'],), [tile_name(tile, c['L'] % 4 == 0)]
    return d


# ---------------------------------------------------------------------------------------------------------------
# Tiles, from v2w_conv1d_split's arithmetic with tiles256 = B * ceil(L / 256) * (C_out / 128): C_out % 128 == 0: 128 x 128 from
# 2 * tiles256 >= 384, else 64 x 128; other C_out % 64 == 0: 64 x 256; a halo (roundup4(left) or right) past 32: the HM = 40 forms.
KD = ((3, 1), (7, 3), (11, 1))
TILES = []


def _both(id, tile, **kw):
    """Dense and short-chain.  The short-chain batch covers every input channel (hence every residue mod 16 in every chunk)."""
    assert kw['B'] >= kw['ci']
    return [conv(id, tile, **kw), conv(id + '_short', tile, short=True, **kw)]


for _k, _d in KD:
    _s = 'k%d_d%d' % (_k, _d)
    TILES += _both('t128_' + _s, T128, B=192, ci=16, co=128, L=256, k=_k, dil=_d)                 # 2 * tiles256 = 384 exactly
    TILES += _both('t64_' + _s, T64, B=16, ci=16, co=128, L=300, k=_k, dil=_d)
    TILES += _both('t64_ci32_' + _s, T64, B=32, ci=32, co=128, L=130, k=_k, dil=_d)
    TILES += _both('t256_co64_' + _s, T256, B=16, ci=16, co=64, L=300, k=_k, dil=_d)
    TILES += _both('t256_co192_' + _s, T256, B=16, ci=16, co=192, L=300, k=_k, dil=_d)
TILES += _both('t128_L257_k3_d1', T128, B=96, ci=16, co=128, L=257, k=3, dil=1)                   # 96 * 2 tiles256
TILES += _both('t64_below_threshold', T64, B=191, ci=16, co=128, L=8, k=3, dil=1)                 # 2 * 191 < 384
# wide halos: 34 and 38 (the discriminator's k = 5, dilation = period 17 / 19), exactly 40, and roundup4(pad_left) = 36 against a right side of 7
for _id, _kw in (('halo34', dict(k=5, dil=17)), ('halo38', dict(k=5, dil=19)), ('halo40', dict(k=5, dil=20)),
                 ('pad33', dict(k=5, dil=10, pad_left=33))):
    TILES += _both('w64_' + _id, W64, B=16, ci=16, co=64, L=200, **_kw)
    TILES += _both('w128_' + _id, W128, B=192, ci=16, co=128, L=128, **_kw)                       # 2 * tiles256 = 384
TILES += _both('w64_pad37', W64, B=16, ci=16, co=64, L=200, k=3, dil=20, pad_left=37)          # 37 -> 40 staged rows on the left, 3 on the right
TILES += _both('t256_halo32', T256, B=16, ci=16, co=64, L=300, k=5, dil=16)                       # the last halo of the HM = 32 forms
TILES += _both('t256_pad29', T256, B=16, ci=16, co=64, L=300, k=5, dil=10, pad_left=29)           # roundup4(29) = 32 stays

# ---------------------------------------------------------------------------------------------------------------
# Lengths on every tile: 1, shorter than the receptive field (19 at k 7, dilation 3; 69 at k 5, dilation 17), NT - 1, NT, NT + 1, NT + 2
# (L % 4 == 2), and an input / output base 4 bytes past a 16-byte boundary (scalar staging / element-wise epilogue with L % 4 == 0)
def _shape(tile):
    return {T128: dict(B=192, ci=16, co=128), T64: dict(B=2, ci=16, co=128), T256: dict(B=2, ci=16, co=64),
            W128: dict(B=192, ci=16, co=128), W64: dict(B=2, ci=16, co=64)}[tile]


LENGTHS = []
for _t in (T128, T64, T256, W128, W64):
    _kw = dict(k=5, dil=17) if _t[4] == 40 else dict(k=7, dil=3)
    _nt, _tn = NT[_t], TNAME[_t]
    for _L in (1, 5, _nt - 1, _nt, _nt + 1, _nt + 2):
        LENGTHS.append(conv('%s_L%d' % (_tn, _L), _t, L=_L, flags=('bias',), **_kw, **_shape(_t)))
    LENGTHS.append(conv('%s_in_plus4' % _tn, _t, L=_nt, in_off=1, flags=('bias',), **_kw, **_shape(_t)))
    LENGTHS.append(conv('%s_out_plus4' % _tn, _t, L=_nt, out_off=1, flags=('bias',), **_kw, **_shape(_t)))

# ---------------------------------------------------------------------------------------------------------------
# Prologue and epilogue, one switch at a time and then together, on the 64 x 128 and the 128 x 128 tile, vector (L % 4 == 0) and scalar
ALL_ADD = ('in_aff', 'bias', 'res', 'res_aff', 'add0', 'add1')
ALL_ACC = ('in_aff', 'bias', 'res', 'res_aff', 'acc')
EPILOGUES = []
for _t, _sh, _Lv in ((T64, dict(B=2, ci=16, co=128), 72), (T128, dict(B=192, ci=16, co=128), 16)):
    def _e(id, both=True, **kw):
        for v in ((True, False) if both else (None,)):
            q = dict(dict(L=_Lv if v in (True, None) else _Lv + 2, k=3, dil=1), **kw)
            EPILOGUES.append(conv('%s_%s%s' % (TNAME[_t], id, '_scalar' if v is False else ''), _t, **_sh, **q))
    _e('plain', slope=1.0)
    for _f in (('in_aff',), ('bias',), ('res',), ('res', 'res_aff'), ('acc',), ('add0',), ('add0', 'add1')):
        _e('_'.join(_f), flags=_f)
    _e('out_div3', out_div=3.0)
    _e('out_slope', out_slope=0.2)
    _e('mask', flags=('mask',))
    _e('mask_aff', flags=('mask', 'mask_aff'))
    _e('mask_all', flags=('mask', 'mask_aff') + ALL_ADD, out_div=3.0, out_slope=0.2)
    _e('all_add', flags=ALL_ADD, out_div=3.0, out_slope=0.2)
    _e('all_acc', flags=ALL_ACC, out_div=3.0)
    # the de-interleaved phases of a (B, C_in, 2 L) tensor (scalar staging only); channel slices: group 1 of 2 in, group 2 of 3 out
    _e('stride2_phase0', both=False, in_stride=2, in_phase=0)
    _e('stride2_phase1', both=False, in_stride=2, in_phase=1)
    _e('slices', in_ct=2 * _sh['ci'], in_g=1, out_ct=3 * _sh['co'], out_g=2, flags=('bias', 'res', 'add0'))
    # asymmetric padding (the input-gradient form): 18 taps-positions, 5 on the left
    _e('pad_left5', k=7, dil=3, pad_left=5)
    # 2, 3 and 4 problems of different k in one launch
    _e('n2', k=(7, 3), flags=('bias', 'res'))
    _e('n3', k=(11, 7, 3), flags=('bias', 'res'))
    _e('n4_all', k=(11, 7, 5, 3), flags=ALL_ADD, out_div=3.0)

# the matching input gradient of three forward records (C_in = 64 -> C_out = 128: the gradient is a 128 -> 64 conv on the 64 x 256 tile)
DGRAD = []
for _id, _kw in (('k3_d1', dict(k=3, dil=1)), ('k7_d3', dict(k=7, dil=3)), ('k7_d3_pad5', dict(k=7, dil=3, pad_left=5))):
    _f = conv('pair_' + _id, T64, B=2, ci=64, co=128, L=300, **_kw)
    DGRAD += [_f, dgrad(_f, T256)]

# ---------------------------------------------------------------------------------------------------------------
# Operand range, on the 64 x 256 tile, dense and short-chain
RANGE = []
for _data in ('big', 'f16max', 'tiny', 'zero_layer', 'w_small', 'w_pow2'):
    RANGE += _both('range_' + _data, T256, B=16, ci=16, co=64, L=300, k=3, data=_data, slope=1.0 if _data == 'big' else 0.1, flags=('bias',))

# ---------------------------------------------------------------------------------------------------------------
# bf16 operands on the same kernel (C_in = 16: v2w_conv1d_bf16 declines)
BF16 = []
BF16 += _both('bf_t256_k3', T256, B=16, ci=16, co=64, L=300, k=3, bf=True, flags=('bias',))
BF16 += _both('bf_t256_k7_d3', T256, B=16, ci=16, co=64, L=300, k=7, dil=3, bf=True)
BF16 += _both('bf_t256_scalar', T256, B=16, ci=16, co=64, L=254, k=3, bf=True, flags=('bias', 'res'))
BF16 += _both('bf_t64_k3', T64, B=16, ci=16, co=128, L=300, k=3, bf=True, flags=('bias',))
BF16 += _both('bf_t128_k3', T128, B=192, ci=16, co=128, L=256, k=3, bf=True, flags=('bias',))

# ---------------------------------------------------------------------------------------------------------------
# Refusals: the return code only
_R = dict(B=2, ci=16, co=64, L=64, k=3)
REFUSALS = [
    conv('even_k', T256, rc=E_SHAPE, **dict(_R, k=4, pad_left=1)),
    conv('even_k_symmetric', T256, rc=E_SHAPE, **dict(_R, k=4)),
    conv('k1', T256, rc=E_SHAPE, **dict(_R, k=1)),
    conv('halo41', T256, rc=E_SHAPE, dil=41, **_R),
    conv('ci24', T256, rc=E_SHAPE, **dict(_R, ci=24)),
    conv('co32', T256, rc=E_SHAPE, **dict(_R, co=32)),
    conv('co16', T256, rc=E_SHAPE, **dict(_R, co=16)),
    conv('multi_other_L', T256, rc=E_SHAPE, L_alt=60, **dict(_R, k=(3, 3))),
    conv('no_wps', T256, rc=E_ARG, null=('wps',), **_R),
    conv('no_winv', T256, rc=E_ARG, null=('winv',), **_R),
    conv('no_wps_second_problem', T256, rc=E_ARG, null=('wps1',), **dict(_R, k=(3, 3))),
    conv('n5', T256, rc=E_ARG, **dict(_R, k=(3, 3, 3, 3, 3))),
    conv('bf_halo34', T256, rc=E_SHAPE, bf=True, dil=17, **dict(_R, k=5)),   # (the wide-halo form exists for the split-f16 operands only)
]

CONV_TABLE = dict(tiles=TILES, lengths=LENGTHS, epilogues=EPILOGUES, dgrad=DGRAD, range=RANGE, bf16=BF16, refusals=REFUSALS)
CONV_ALL = [c for cases in CONV_TABLE.values() for c in cases]


# ---------------------------------------------------------------------------------------------------------------
# operands on the CPU, one seed per record id and problem
def _rng(c, i=0):
    return np.random.default_rng(sum(map(ord, c['id'].replace('_short', ''))) + 7919 * i)        # dense and short-chain: the same weights


def _f32(rng, *shape, scale=1.0):
    return torch.from_numpy(rng.standard_normal(shape, dtype=np.float32) * np.float32(scale))


def draw_mask(rng, B, Cc, L, a, s):
    """The mask source with |a * m + s| >= 2^-10 in fp64 everywhere (offenders redrawn): fp32 and fp64 agree on the sign of the argument.
    Without the affine it also holds exact +0 and -0, which take the slope."""
    m = _f32(rng, B, Cc, L)
    for _ in range(64):
        arg = D.f64(m) if a is None else D.f64(a)[:, :, None] * D.f64(m) + D.f64(s)[:, :, None]
        bad = arg.abs() < MASK_MIN
        if not bad.any():
            break
        m[bad] = _f32(rng, int(bad.sum()))
    assert not bad.any()
    if a is None and m.numel() >= 6:
        flat = m.view(-1)
        flat[:4] = torch.tensor([0.0, -0.0, 0.0, -0.0])
        flat[-2:] = torch.tensor([-0.0, 0.0])
    return m


def _signal(c, rng, shape):
    """The input tensor's values by the record's operand range."""
    x = _f32(rng, *shape)
    data = c['data']
    pick = torch.from_numpy(rng.integers(0, 4, size=shape))
    pick8 = torch.from_numpy(rng.integers(0, 8, size=shape))
    sign = torch.where(x < 0, -torch.ones_like(x), torch.ones_like(x))
    if data == 'big':                 # past the f16 range on both sides (slope 1): clamped to +-65504
        x = torch.where(pick == 0, torch.full_like(x, 1e5), torch.where(pick == 1, torch.full_like(x, -3e5), x * 1e4))
    elif data == 'f16max':            # exactly on the clamp
        x = torch.where(pick <= 1, sign * F16_MAX, x)
    elif data == 'tiny':              # a_lo zero (6e-8 is about one f16 subnormal step; 3e-5 is itself subnormal) or subnormal (0.1): 1 : 1 : 6
        x = sign * torch.where(pick8 == 0, torch.full_like(x, 6e-8), torch.where(pick8 == 1, torch.full_like(x, 3e-5), torch.full_like(x, 0.1)))
    return x


def _weights(c, rng, k, ci, co):
    wf = _f32(rng, k, ci, co, scale=1.0 / np.sqrt(ci * k))
    data = c['data']
    if data == 'zero_layer':
        wf = torch.zeros_like(wf)
    elif data == 'w_small':           # one weight 2^-20 of the layer's maximum (its lo half is an f16 subnormal)
        wf[k // 2, 3, 5] = wf.abs().max() * 2.0 ** -20 * (1 + 2.0 ** -9)
    elif data == 'w_pow2':            # the maximum an exact power of two: the scaled maximum is exactly 8192
        wf = wf.clamp(-0.2, 0.2)
        wf[0, 1, 2], wf[k - 1, 7, 9] = 0.25, -0.25
    return wf


def operands(c, i=0):
    """The CPU tensors of problem i of a conv record: dict with x (B, in_ct, in_stride * L) (the whole tensor `in` is a slice of), wf
    [k][C_in][C_out] as the conv applies it, and every switch's operand ((B, out_ct, L) ones whole); `ref`: the keyword arguments of
    split_ref.conv1d on the call's slices; isl / osl: the channel slices."""
    rng = _rng(c, i)
    B, ci, co, L, k, f = c['B'], c['ci'], c['co'], c['L'], c['ks'][i], c['flags']
    ict, oct_ = c['in_ct'] or ci, c['out_ct'] or co
    isl, osl = slice(c['in_g'] * ci, (c['in_g'] + 1) * ci), slice(c['out_g'] * co, (c['out_g'] + 1) * co)
    if c.get('wT'):                                          # the forward layer's weights [k][co][ci] -> the stream of its input gradient
        wf = D.transpose_flip(_weights(c, rng, k, co, ci))
    else:
        wf = _weights(c, rng, k, ci, co)
    x = _signal(c, rng, (B, ict, L * c['in_stride']))
    if c['short']:
        live = torch.zeros(B, ict, 1, dtype=torch.bool)
        for b in range(B):
            live[b, c['in_g'] * ci + b % ci] = True
        x = torch.where(live, x, torch.zeros_like(x))
    t = dict(x=x, wf=wf)
    ref = dict(dil=c['dil'], pad_left=c['pad_left'], slope=c['slope'], in_stride=c['in_stride'], in_phase=c['in_phase'],
               out_div=c['out_div'], out_slope=c['out_slope'])

    def small(name, *shape, scale=1.0, shift=0.0):
        t[name] = ref[name] = _f32(rng, *shape, scale=scale) + shift

    def wide(name):
        t[name] = _f32(rng, B, oct_, L)
        ref[name] = t[name][:, osl]

    if 'in_aff' in f:
        small('in_a', B, ci, scale=0.5, shift=1.0), small('in_s', B, ci, scale=0.5)
    if 'bias' in f:
        small('bias', co)
    if 'res' in f:
        wide('res')
    if 'res_aff' in f:
        small('res_a', B, co, scale=0.5, shift=1.0), small('res_s', B, co, scale=0.5)
    if 'add0' in f:
        wide('add0')
    if 'add1' in f:
        wide('add1')
    if 'mask' in f:
        if 'mask_aff' in f:
            small('mask_a', B, co, scale=0.5, shift=1.0), small('mask_s', B, co, scale=0.5)
        m = draw_mask(rng, B, co, L, ref.get('mask_a'), ref.get('mask_s'))
        t['mask_src'] = _f32(rng, B, oct_, L)
        t['mask_src'][:, osl] = m
        ref['mask_src'], ref['mask_slope'] = m, c['mask_slope']
    if 'acc' in f:
        ref['old'] = _f32(rng, B, co, L)
    return dict(t=t, ref=ref, isl=isl, osl=osl)


# ---------------------------------------------------------------------------------------------------------------
# the argument structs, from a table of addresses (made up here, real ones in the GPU tests)
NAMES = ('in_', 'wps', 'winv', 'bias', 'in_a', 'in_s', 'res', 'res_a', 'res_s', 'add0', 'add1', 'mask_src', 'mask_a', 'mask_s', 'out')


def fake_buffers(c):
    """16-byte aligned addresses nothing reads: per problem a dict operand -> buffer base."""
    return [{name: 0x10000000 * (i + 1) + 0x800000 * j for j, name in enumerate(NAMES)} for i in range(len(c['ks']))]


def _used(c, i):
    f = c['flags']
    u = {'in_', 'wps', 'winv', 'out'} | ({'bias', 'res', 'add0', 'add1'} & f)
    u |= {'in_a', 'in_s'} if 'in_aff' in f else set()
    u |= {'res_a', 'res_s'} if 'res_aff' in f else set()
    u |= {'mask_src'} if 'mask' in f else set()
    u |= {'mask_a', 'mask_s'} if 'mask_aff' in f else set()
    return u - set(c['null'] if i == 0 else ()) - {q[:-1] for q in c['null'] if q.endswith(str(i)) and i > 0}


def problem_L(c, i):
    return c['L'] if (i == 0 or c['L_alt'] is None) else c['L_alt']


def offsets(c):
    """Floats from an operand's 16-byte aligned buffer to the base the call gets: (`in`, `out`, the other (B, C_out, L) operands)."""
    i = c['in_off'] + c['in_g'] * c['ci'] * c['L'] * c['in_stride']
    o = c['out_g'] * c['co'] * c['L']
    return i, c['out_off'] + o, o


def conv_array(c, per):
    """The v2w_conv1d_args of every problem of a conv record; per[i]: operand -> 16-byte aligned buffer base of problem i."""
    n = len(c['ks'])
    arr = (_hip.Conv1dArgs * n)()
    oi, oo, oe = offsets(c)
    for i in range(n):
        a, p = arr[i], per[i]
        for name in _used(c, i):
            off = {'in_': oi, 'out': oo, 'res': oe, 'add0': oe, 'add1': oe, 'mask_src': oe}.get(name, 0)
            setattr(a, name, p[name] + 4 * off)
        a.B, a.C_in, a.C_out, a.L, a.k, a.dil = c['B'], c['ci'], c['co'], problem_L(c, i), c['ks'][i], c['dil']
        a.slope, a.algo, a.pad_left, a.accumulate = c['slope'], (_hip.ALGO_BF16 if c['bf'] else _hip.ALGO_SPLIT), c['pad_left'], int('acc' in c['flags'])
        a.out_div, a.out_slope, a.mask_slope = c['out_div'], c['out_slope'], c['mask_slope'] if 'mask' in c['flags'] else 0.0
        a.in_stride, a.in_phase, a.in_ct, a.out_ct = (c['in_stride'] if c['in_stride'] > 1 else 0), c['in_phase'], c['in_ct'], c['out_ct']
    return arr


def call(c, per, stream=None):
    """Run the record's entry point on the given addresses: with a stream for real, without one through the name sink -> (rc, kernel names)."""
    lib = _hip.load()
    arr = conv_array(c, per)
    n = len(c['ks'])
    fn, args = (lib.v2w_conv1d_fwd, (arr,)) if n == 1 else (lib.v2w_conv1d_fwd_multi, (arr, n))
    if stream is None:
        return _hip.kernel_names(fn, *args)
    return fn(*args, stream), None


def dispatch(c):
    """Host-only: (return code, kernels) of the record.  A process without a GPU reports hipErrorNoDevice (100) from the launch status."""
    rc, names = call(c, fake_buffers(c))
    return (OK if rc == 100 else rc), names


# ---------------------------------------------------------------------------------------------------------------
# Stage kernel: v2w_resblock2_stage_split_fwd on fp32 tensors with bf16 = 0 - stage_split_kernel<2, 2, 4, false> (C = 32) and
# <1, 2, 4, false> (C = 16), W = 256 positions per phase.  The launcher's arithmetic: h1max / h2max the largest halo k_j * dil / 2 of the
# first / second convs; a tile keeps nto = (256 - 2 h2max) & ~3 positions and is refused below 128 - so h2max <= 64 is the largest halo of
# the second convs; the first convs' halo is limited by the 160 KiB of LDS alone ((xrows + 256) rows of 4 C + 16 bytes).
def stage_name(Cc):
    return 'stage_split_kernel<%d, 2, 4, false>' % (Cc // 16)


BLOCKS = {                       # (k, dil1, dil2) per branch
    'ref': ((3, 1, 3), (7, 1, 3), (11, 1, 3)),                      # the reference's block set: k = (3, 7, 11), dilations (1, 3)
    'one': ((5, 2, 1),),
    'four': ((3, 5, 1), (11, 2, 1), (5, 1, 16), (9, 3, 16)),        # mixed; h1max = 12, h2max = 64: the largest the launcher accepts
    'past': ((3, 1, 1), (5, 1, 1), (7, 1, 1), (11, 1, 13)),         # h2max = 65: nto = 124 < 128
}


def stage_nto(blocks):
    return (256 - 2 * max(d2 * (k - 1) // 2 for k, _, d2 in blocks)) & ~3


def stage(id, Cc, blocks, *, B, L, rc=OK, aff=True, bias=True, out_div=3.0, in_off=0, short=False, order=None, slope=0.1):
    """One stage record.  order: the placement of the 2 nk fragment streams in their buffer (None: execution order w1_0, w2_0, w1_1, ...)."""
    bl = BLOCKS[blocks]
    assert not (short and (aff or bias))
    live = 1 if short else Cc
    # ops of a phase: leaky-relu (1), the residual's unlrelu division (1), bias (1), residual add (1); conv1 also the input affine (1)
    n1 = tuple(3 * k * live + 2 + int(bias) + 1 + int(aff) for k, _, _ in bl)
    n2 = tuple(3 * k * Cc + 2 + int(bias) + 1 for k, _, _ in bl)        # (t1 is dense over the channels whatever x is)
    return _case(id, [] if rc != OK else [stage_name(Cc)], rc, op='stage', C=Cc, blocks=bl, B=B, L=L, aff=aff, bias=bias, out_div=out_div,
                 in_off=in_off, short=short, order=order, slope=slope, n1=n1, n2=n2)


STAGES = []
for _C in (32, 16):
    for _bn in ('ref', 'one', 'four'):
        _nto = stage_nto(BLOCKS[_bn])
        for _L in (1, 4, _nto - 1, _nto, _nto + 1, _nto + 2):
            STAGES.append(stage('c%d_%s_L%d' % (_C, _bn, _L), _C, _bn, B=2, L=_L))
    _nto = stage_nto(BLOCKS['ref'])
    STAGES.append(stage('c%d_no_aff' % _C, _C, 'ref', B=2, L=_nto + 4, aff=False))
    STAGES.append(stage('c%d_no_bias' % _C, _C, 'ref', B=2, L=_nto + 4, bias=False))
    STAGES.append(stage('c%d_no_div' % _C, _C, 'ref', B=2, L=_nto + 4, out_div=0.0))
    STAGES.append(stage('c%d_in_plus4' % _C, _C, 'ref', B=2, L=_nto + 4, in_off=1))
    STAGES.append(stage('c%d_short' % _C, _C, 'ref', B=_C, L=_nto + 4, aff=False, bias=False, short=True))
    STAGES.append(stage('c%d_short_scalar' % _C, _C, 'four', B=_C, L=stage_nto(BLOCKS['four']) + 2, aff=False, bias=False, short=True))
    STAGES.append(stage('c%d_past_halo' % _C, _C, 'past', B=2, L=256, rc=E_SHAPE))
    STAGES.append(stage('c%d_streams_swapped' % _C, _C, 'ref', B=2, L=64, rc=E_ARG, order=(1, 0, 2, 3, 4, 5)))
    STAGES.append(stage('c%d_streams_by_conv' % _C, _C, 'ref', B=2, L=64, rc=E_ARG, order=(0, 2, 4, 1, 3, 5)))

ALL = CONV_ALL + STAGES
assert len({c['id'] for c in ALL}) == len(ALL)


def stream_halves(c, j):
    """f16 elements of one fragment stream of branch j (without a padding unit): hipops.split_units_halves."""
    return c['blocks'][j][0] * c['C'] * 32 * 2


def stream_offsets(c):
    """f16 element offsets of the 2 nk streams (w1_0, w2_0, w1_1, ...) in one buffer, placed in `order`; and the buffer's length."""
    nk = len(c['blocks'])
    sizes = [stream_halves(c, s // 2) for s in range(2 * nk)]
    order = c['order'] or tuple(range(2 * nk))
    offs, pos = [0] * (2 * nk), 0
    for s in order:
        offs[s] = pos
        pos += sizes[s]
    return offs, pos


def stage_struct(c, addr):
    """v2w_stage_split_args from addresses: in_, out, in_a, in_s, wps (base of the stream buffer), sc (2 nk records of 4 floats), b1 / b2
    (nk rows of C floats)."""
    a = _hip.StageSplitArgs()
    offs, _ = stream_offsets(c)
    Cc = c['C']
    a.in_, a.out = addr['in_'] + 4 * c['in_off'], addr['out']
    if c['aff']:
        a.in_a, a.in_s = addr['in_a'], addr['in_s']
    for j, (k, d1, d2) in enumerate(c['blocks']):
        a.k[j], a.dil1[j], a.dil2[j] = k, d1, d2
        a.wps1[j], a.wps2[j] = addr['wps'] + 2 * offs[2 * j], addr['wps'] + 2 * offs[2 * j + 1]
        a.sc1[j], a.sc2[j] = addr['sc'] + 16 * (2 * j), addr['sc'] + 16 * (2 * j + 1)
        if c['bias']:
            a.bias1[j], a.bias2[j] = addr['b1'] + 4 * Cc * j, addr['b2'] + 4 * Cc * j
    a.nk, a.B, a.C, a.L = len(c['blocks']), c['B'], Cc, c['L']
    a.slope, a.out_div, a.bf16, a.io_bf16 = c['slope'], c['out_div'], 0, 0
    return a


STAGE_FAKE = dict(in_=0x10000000, out=0x20000000, in_a=0x30000000, in_s=0x31000000, wps=0x40000000, sc=0x50000000, b1=0x51000000, b2=0x52000000)


def stage_dispatch(c):
    rc, names = _hip.kernel_names(_hip.load().v2w_resblock2_stage_split_fwd, C.byref(stage_struct(c, STAGE_FAKE)))
    return (OK if rc == 100 else rc), names


def stage_operands(c):
    """CPU tensors of a stage record: x (B, C, L), in_a / in_s (B, C) or None, per branch dict(w1, b1, w2, b2, d1, d2) with [k][C][C] weights."""
    rng = _rng(c)
    B, Cc, L = c['B'], c['C'], c['L']
    x = _f32(rng, B, Cc, L)
    if c['short']:
        live = torch.zeros(B, Cc, 1, dtype=torch.bool)
        for b in range(B):
            live[b, b % Cc] = True
        x = torch.where(live, x, torch.zeros_like(x))
    in_a = _f32(rng, B, Cc, scale=0.5) + 1.0 if c['aff'] else None
    in_s = _f32(rng, B, Cc, scale=0.5) if c['aff'] else None
    brs = []
    for k, d1, d2 in c['blocks']:
        brs.append(dict(w1=_f32(rng, k, Cc, Cc, scale=1.0 / np.sqrt(Cc * k)), b1=_f32(rng, Cc) if c['bias'] else None,
                        w2=_f32(rng, k, Cc, Cc, scale=1.0 / np.sqrt(Cc * k)), b2=_f32(rng, Cc) if c['bias'] else None, d1=d1, d2=d2))
    return x, in_a, in_s, brs
