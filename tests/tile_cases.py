"""The cases of tests/test_tile_kernels_gpu.py: one record per call of v2w_conv1d_fwd / _fwd_multi / _fwd_len / v2w_convt1d_fwd / _fwd_len on
the f32 tile kernel family (csrc/v2w_conv_mfma.hip), with the kernels the call must launch, its return code and its chain lengths n (a tuple: one per problem of the launch).

tests/test_tile_ref_cpu.py drives every record through the name sink (host-only, made-up pointers) and asserts `kernels` and `rc`; the GPU
tests run the same records on real tensors.  `conv_array` / `convt_struct` build the argument structs for both from a table of addresses, so
the alignment of every operand - which selects the vector or scalar path - is the same in the two runs.  Kernel names are the short ones of
_hip.kernel_name_short with every template argument spelled out: <MF, U, MI, NI, WM, WN, CK, NPF, RING, EPI, VEC>.

n (the bound is n * 2^-24 * S, tests/tile_ref.py): k * C_in products of the problem's own k, plus `ops`, one per fp32 operation the
call's switches add to an entry - input affine 1 (a single fma), leaky-relu 1, mask factor 1 (the mask's own affine adds none: only the sign
of its fma enters, and the mask source is drawn so that fp32 and fp64 agree on it), bias 1, residual 1 (+ 1 for its affine), accumulate / add0 1,
add1 1, out_div 1 (the quotient is correctly rounded), out_slope 1.  The split over C_in only reorders the sum.  Transposed conv:
ceil(k / u) * C_in + 2 (leaky-relu, bias)."""
import ctypes as C

from wavthruvec_pytorch_amd import _hip

from tests.disc_cases import OK, _case, ids  # noqa: F401  (ids: re-exported for the parametrisations)
from tests.disc_ref import ceil_div

E_ARG = -1

# <MF, U, MI, NI, WM, WN, CK, NPF, RING> and the positions per tile NT = MF * NI * WN
LAT, T128x64, T128, T64x128 = '32, 1, 1, 1, 2, 2, 32, 2, 4', '32, 1, 2, 1, 2, 2, 32, 2, 4', '32, 1, 2, 2, 2, 2, 32, 3, 4', '32, 1, 1, 2, 2, 2, 32, 3, 4'
CK16, R32, MF16 = '32, 1, 1, 2, 1, 4, 16, 3, 2', '32, 1, 1, 2, 1, 4, 32, 5, 4', '16, 1, 1, 4, 1, 4, 16, 3, 2'
NT = {LAT: 64, T128x64: 64, T128: 128, T64x128: 128, CK16: 256, R32: 256, MF16: 256}
UP_TILE = {64: '32, %d, 1, 1, 2, 2, 16, 1, 2', 32: '32, %d, 1, 1, 1, 4, 16, 2, 2', 16: '16, %d, 1, 2, 1, 4, 16, 2, 2'}    # by C_out (256: as 64)
UP_NT = {64: 64, 32: 128, 16: 128}


def tile_name(tile, epi=0, vec=True):
    return 'conv_tile_kernel<%s, %d, %s>' % (tile, epi, 'true' if vec else 'false')


def reduce_name(vec):
    return 'splitk_reduce_kernel<%s>' % ('true' if vec else 'false')


# fp32 operations per switch (see the module docstring): in_aff is one fma; mask_aff only decides a sign; rowsum is checked on its own
OPS = dict(in_aff=1, bias=1, res=1, res_aff=1, acc=1, add0=1, add1=1, mask=1, mask_aff=0, rowsum=0)


def conv(id, tile, *, B, ci, co, L, k, dil=1, epi=0, vec=True, reduce=None, rc=OK, flags=(), slope=0.1, pad_left=-1, out_div=0.0,
         out_slope=0.0, mask_slope=0.1, in_stride=1, in_phase=0, in_ct=0, in_g=0, out_ct=0, out_g=0, in_off=0, out_off=0, ws=None,
         lens=None, len_mul=1, big=False):
    """One conv record.  k: an int, or a tuple (one problem per entry: _fwd_multi, or _fwd_len with `lens`).  flags: the switches of OPS.
    in_off / out_off: floats between a 16-byte boundary and the base of `in` / `out`.  in_ct / out_ct with in_g / out_g: the call works on
    channel slice g of tensors with that many channels.  ws: None, 'full' (the bytes the library asks for) or 'short' (one byte less).
    lens: per-item lengths (B of them), in units of len_mul positions.  big: the fp64 reference may run as matrix products on the GPU."""
    ks = k if isinstance(k, tuple) else (k,)
    flags = frozenset(flags)
    assert flags <= set(OPS) and not ({'acc', 'add0'} <= flags) and (lens is None or len(lens) == B)
    ops = sum(OPS[f] for f in flags) + (slope != 1.0) + (out_div != 0.0) + (out_slope not in (0.0, 1.0))
    kernels = [] if rc != OK else [tile_name(tile, epi, vec)] + ([] if reduce is None else [reduce_name(reduce)])
    return _case(id, kernels, rc, op='conv', tile=tile, B=B, ci=ci, co=co, L=L, ks=ks, dil=dil, flags=flags, slope=slope, pad_left=pad_left,
                 out_div=out_div, out_slope=out_slope, mask_slope=mask_slope, in_stride=in_stride, in_phase=in_phase, in_ct=in_ct, in_g=in_g,
                 out_ct=out_ct, out_g=out_g, in_off=in_off, out_off=out_off, ws=ws, lens=lens, len_mul=len_mul, big=big,
                 ops=ops, n=tuple(kk * ci + ops for kk in ks))


def dgrad(c):
    """The input gradient of a plain record: the same conv of a (B, C_out, L) cotangent with the transposed, tap-reversed weights, the taps
    left of the output now the forward's right ones.  `kernels` is filled in by hand where the tile differs."""
    k, dil = c['ks'][0], c['dil']
    left = c['pad_left'] if c['pad_left'] >= 0 else dil * (k - 1) // 2
    d = dict(c, id=c['id'] + '_dgrad', ci=c['co'], co=c['ci'], pad_left=(k - 1) * dil - left, slope=1.0, flags=frozenset(), wT=True)
    d['ops'], d['n'] = 0, (k * c['co'],)
    return d


def _pair(id, tile, dtile, **kw):
    f = conv(id, tile, **kw)
    d = dgrad(f)
    d['tile'], d['kernels'] = dtile, [tile_name(dtile, 0, kw.get('vec', True))]
    return [f, d]


# ---------------------------------------------------------------------------------------------------------------
# Tiles: forward and the matching input gradient.  The launcher's arithmetic (v2w_conv1d_mfma), with t64 = B * ceil(L / 64) * (C_out / 64)
# and t128 = B * ceil(L / 128) * (C_out / 128): latency tile while n * t64 < 512; C_out % 128 == 0: 128 x 128 from t128 >= 1024, else
# 128 x 64; C_out % 64 == 0: 64 x 128; C_in % 32 != 0: CK 16; other C_out % 32 == 0: 32 rows; C_out == 16: MF 16.
KD = ((3, 1), (7, 3), (11, 5))
TILES = []
for _k, _d in KD:
    _s = 'k%d_d%d' % (_k, _d)
    TILES += _pair('lat_' + _s, LAT, LAT, B=2, ci=64, co=64, L=200, k=_k, dil=_d)
    TILES += _pair('t128x64_' + _s, T128x64, R32, B=2, ci=32, co=128, L=8192, k=_k, dil=_d)        # t64 = 512, t128 = 128
    TILES += _pair('t64x128_' + _s, T64x128, R32, B=2, ci=32, co=64, L=16384, k=_k, dil=_d)        # t64 = 512
    TILES += _pair('ck16_' + _s, CK16, MF16, B=2, ci=16, co=32, L=300, k=_k, dil=_d)
    TILES += _pair('r32_' + _s, R32, R32, B=2, ci=32, co=32, L=300, k=_k, dil=_d)
    TILES += _pair('r32_co96_' + _s, R32, R32, B=2, ci=32, co=96, L=300, k=_k, dil=_d)
    TILES += _pair('mf16_' + _s, MF16, MF16, B=2, ci=16, co=16, L=300, k=_k, dil=_d)
TILES += _pair('t128_k11_d5', T128, R32, B=2, ci=32, co=128, L=65536, k=11, dil=5, big=True)       # t128 = 1024 exactly
TILES += _pair('lat_halo32', LAT, LAT, B=2, ci=64, co=64, L=200, k=5, dil=16)                      # both halos exactly 32
TILES += _pair('lat_pad30', LAT, LAT, B=2, ci=64, co=64, L=200, k=7, dil=5, pad_left=30)           # roundup4(30) = 32 staged rows on the left, none on the right
TILES += _pair('t128x64_halo32', T128x64, R32, B=2, ci=32, co=128, L=8192, k=5, dil=16)

# ---------------------------------------------------------------------------------------------------------------
# Lengths on every tile: 1, shorter than the receptive field (19 at k 7, dilation 3; 3 at k 3), NT - 1, NT, NT + 1, NT + 2 (L % 4 == 2), and
# an input / output base 4 bytes past a 16-byte boundary.  The batch is the smallest that keeps the shape on its tile.
def _shape(tile, L):
    if tile == LAT:
        return dict(B=2, ci=64, co=64)
    if tile == T128x64:
        return dict(B=ceil_div(256, ceil_div(L, 64)), ci=32, co=128)          # t64 = 2 B ceil(L / 64) >= 512
    if tile == T128:
        return dict(B=ceil_div(1024, ceil_div(L, 128)), ci=32, co=128)        # t128 >= 1024
    if tile == T64x128:
        return dict(B=ceil_div(512, ceil_div(L, 64)), ci=32, co=64)           # t64 >= 512
    return {CK16: dict(B=2, ci=16, co=32), R32: dict(B=2, ci=32, co=32), MF16: dict(B=2, ci=16, co=16)}[tile]


LENGTHS = []
for _t, _tn in ((LAT, 'lat'), (T128x64, 't128x64'), (T128, 't128'), (T64x128, 't64x128'), (CK16, 'ck16'), (R32, 'r32'), (MF16, 'mf16')):
    _k, _d = (3, 1) if _t == T128 else (7, 3)
    _nt = NT[_t]
    for _L in (1, 2 if _t == T128 else 5, _nt - 1, _nt, _nt + 1, _nt + 2):
        LENGTHS.append(conv('%s_L%d' % (_tn, _L), _t, L=_L, k=_k, dil=_d, vec=_L % 4 == 0, big=_t == T128, flags=('bias',), **_shape(_t, _L)))
    LENGTHS.append(conv('%s_in_plus4' % _tn, _t, L=_nt, k=_k, dil=_d, vec=False, in_off=1, big=_t == T128, flags=('bias',), **_shape(_t, _nt)))
    LENGTHS.append(conv('%s_out_plus4' % _tn, _t, L=_nt, k=_k, dil=_d, vec=True, out_off=1, big=_t == T128, flags=('bias',), **_shape(_t, _nt)))

# ---------------------------------------------------------------------------------------------------------------
# Epilogues, one switch at a time and then together, on the latency tile and on the 128 x 64 tile (B = 128 at L = 72: t64 = 512, t128 = 128)
ALL_ADD = ('in_aff', 'bias', 'res', 'res_aff', 'add0', 'add1')
ALL_ACC = ('in_aff', 'bias', 'res', 'res_aff', 'acc')
EPILOGUES = []
for _t, _tn, _sh, _L in ((LAT, 'lat', dict(B=2, ci=64, co=64), 200), (T128x64, 't128x64', dict(B=128, ci=32, co=128), 72)):
    def _e(id, **kw):
        kw = dict(dict(L=_L, k=3, dil=1), **kw)
        EPILOGUES.append(conv('%s_%s' % (_tn, id), _t, **_sh, **kw))
    _e('plain', slope=1.0)
    for _f in (('bias',), ('res',), ('res', 'res_aff'), ('acc',), ('add0',), ('add0', 'add1'), ('in_aff',)):
        _e('_'.join(_f), flags=_f)
    _e('out_div3', out_div=3.0)
    _e('res_out_div3', flags=('res',), out_div=3.0)              # the vector epilogue's prefetched-residual path with the division
    _e('all_add', flags=ALL_ADD, out_div=3.0)
    _e('all_acc', flags=ALL_ACC, out_div=3.0)
    _e('all_add_scalar', flags=ALL_ADD, out_div=3.0, L=_L + 2, vec=False)
    # EPI 2: out_slope
    _e('out_slope', epi=2, out_slope=0.2)
    _e('out_slope_scalar', epi=2, out_slope=0.2, L=_L + 2, vec=False)
    _e('out_slope_all', epi=2, out_slope=0.2, flags=ALL_ADD, out_div=3.0)
    # EPI 1: the mask, without and with its affine, with the row sums (n = NT per row sum), with everything; scalar; the refusal
    _e('mask', epi=1, flags=('mask',))
    _e('mask_aff', epi=1, flags=('mask', 'mask_aff'))
    _e('mask_rowsum', epi=1, flags=('mask', 'rowsum'))
    _e('mask_aff_rowsum_all', epi=1, flags=('mask', 'mask_aff', 'rowsum') + ALL_ADD, out_div=3.0, out_slope=0.2)
    _e('mask_scalar', epi=1, flags=('mask', 'mask_aff', 'bias'), L=_L + 2, vec=False)
    _e('mask_out_plus4', epi=1, flags=('mask',), out_off=1)                  # vector staging, element-wise epilogue
    _e('mask_rowsum_refused', epi=1, flags=('mask', 'rowsum'), L=_L + 2, vec=False, rc=E_ARG)
    # the de-interleaved phases of a (B, C_in, 2 L) tensor; channel slices of wider tensors
    _e('stride2_phase0', in_stride=2, in_phase=0, vec=False)
    _e('stride2_phase1', in_stride=2, in_phase=1, vec=False)
    _e('slices', in_ct=2 * _sh['ci'], in_g=1, out_ct=3 * _sh['co'], out_g=1, flags=('bias', 'res', 'add0'))
    _e('slices_scalar', in_ct=2 * _sh['ci'], in_g=1, out_ct=3 * _sh['co'], out_g=2, flags=('bias', 'res'), L=_L + 1, vec=False)
    # three problems in one launch
    _e('n3', k=(11, 7, 3), flags=('bias', 'res'))
    _e('n3_all', k=(11, 7, 3), flags=ALL_ADD, out_div=3.0)

# ---------------------------------------------------------------------------------------------------------------
# Per-item lengths (EPI 3): 0, 1, inside a tile, on a tile edge, L itself
LENS = [
    conv('lat_len', LAT, epi=3, B=5, ci=64, co=64, L=200, k=7, dil=3, lens=[0, 1, 100, 128, 200], flags=('bias', 'res')),
    conv('lat_len_mul2', LAT, epi=3, B=5, ci=64, co=64, L=200, k=7, dil=3, lens=[0, 1, 50, 64, 100], len_mul=2, flags=('bias',)),
    conv('lat_len_scalar', LAT, epi=3, vec=False, B=5, ci=64, co=64, L=202, k=7, dil=3, lens=[0, 1, 100, 128, 202], flags=('bias', 'res')),
    conv('lat_len_mul2_scalar', LAT, epi=3, vec=False, B=5, ci=64, co=64, L=202, k=7, dil=3, lens=[0, 1, 50, 64, 101], len_mul=2, flags=('bias',)),
    conv('lat_len_n3', LAT, epi=3, B=5, ci=64, co=64, L=200, k=(11, 7, 3), lens=[0, 1, 100, 128, 200], flags=ALL_ADD, out_div=3.0),
    conv('lat_len_past_L', LAT, epi=3, B=5, ci=64, co=64, L=200, k=3, lens=[300, 200, 199, 64, 63]),        # clamped to L
    conv('t128x64_len', T128x64, epi=3, B=128, ci=32, co=128, L=72, k=7, dil=3, lens=[0, 1, 30, 64, 72, 65, 63, 71] * 16, flags=('bias', 'res')),
    conv('t128x64_len_scalar', T128x64, epi=3, vec=False, B=128, ci=32, co=128, L=74, k=7, dil=3, lens=[0, 1, 15, 32, 37, 33, 31, 36] * 16,
         len_mul=2, flags=('bias',)),
    conv('lat_len_out_slope_refused', LAT, epi=3, B=5, ci=64, co=64, L=200, k=7, dil=3, lens=[0, 1, 100, 128, 200], out_slope=0.2, rc=E_ARG),
]

# ---------------------------------------------------------------------------------------------------------------
# Split over C_in: 128 -> 64, k 7, B 1, L 64: one workgroup, four chunks x seven taps -> four slices and the reduce
SPLIT = []


def _sp(id, **kw):
    kw = dict(dict(B=1, ci=128, co=64, L=64, k=7, dil=1, ws='full', reduce=True), **kw)
    SPLIT.append(conv('split_' + id, LAT, **kw))


_sp('vec')
_sp('scalar_L62', L=62, vec=False, reduce=False)
_sp('out_plus4', out_off=1, reduce=False)
_sp('short_ws', ws='short', reduce=None)                          # one byte too small: unsplit, the same values within the bound
_sp('no_ws', ws=None, reduce=None)
for _f in (('bias',), ('res',), ('res', 'res_aff'), ('acc',), ('add0',), ('add0', 'add1'), ('in_aff',)):
    _sp('_'.join(_f), flags=_f)
_sp('out_div3', out_div=3.0)
_sp('res_out_div3', flags=('res',), out_div=3.0)
_sp('all_add', flags=ALL_ADD, out_div=3.0)
_sp('all_acc', flags=ALL_ACC, out_div=3.0)
_sp('all_add_scalar', flags=ALL_ADD, out_div=3.0, L=62, vec=False, reduce=False)
_sp('n3', k=(11, 7, 3), flags=('bias', 'res'))
_sp('n3_all', k=(11, 7, 3), flags=ALL_ADD, out_div=3.0)
_sp('short_chain', ci=64, k=3, reduce=None)                       # 2 chunks x 3 taps < 24 steps: stays whole

# ---------------------------------------------------------------------------------------------------------------
# Upsamplers: ConvTranspose1d(k = 2u (2u + 1 for 5), stride u), C_in = 2 C_out, with the fused statistics rows (n = positions per row)
def convt(id, *, B, ci, co, L, u, k=None, vec=None, stats=True, lens=None, len_mul=1, ws=None, reduce=None, slope=0.1):
    k = k or (2 * u if u % 2 == 0 else 2 * u + 1)
    vec = (L % 4 == 0) if vec is None else vec
    tile = UP_TILE[64 if co % 64 == 0 else co] % u
    kernels = [tile_name(tile, 3 if lens is not None else 0, vec)] + ([] if reduce is None else [reduce_name(reduce)])
    return _case(id, kernels, OK, op='convt', tile=tile, NT=UP_NT[64 if co % 64 == 0 else co], B=B, ci=ci, co=co, L=L, k=k, u=u, stats=stats,
                 lens=lens, len_mul=len_mul, ws=ws, slope=slope, ops=2, n=(ceil_div(k, u) * ci + 2,))


UPS = []
for _u in (2, 4, 5, 8):
    for _co in (64, 32, 16):
        _nt = UP_NT[_co]
        for _L in (1, 3, _nt - 1, _nt, _nt + 1):
            UPS.append(convt('u%d_co%d_L%d' % (_u, _co, _L), B=2, ci=2 * _co, co=_co, L=_L, u=_u))
        UPS.append(convt('u%d_co%d_len' % (_u, _co), B=4, ci=2 * _co, co=_co, L=_nt + 4, u=_u, stats=False, lens=[0, 1, _nt, _nt + 4]))
        UPS.append(convt('u%d_co%d_len_scalar' % (_u, _co), B=4, ci=2 * _co, co=_co, L=_nt + 5, u=_u, stats=False, lens=[0, 1, (_nt + 2) // 2, _nt], len_mul=2))
UPS.append(convt('ups0_split', B=1, ci=512, co=256, L=50, u=5, stats=False, ws='full', reduce=False))
UPS.append(convt('ups0_stats_whole', B=1, ci=512, co=256, L=50, u=5, stats=True, ws='full'))

TABLE = dict(tiles=TILES, lengths=LENGTHS, epilogues=EPILOGUES, lens=LENS, split=SPLIT, ups=UPS)
ALL = [c for cases in TABLE.values() for c in cases]
assert len({c['id'] for c in ALL}) == len(ALL)


# ---------------------------------------------------------------------------------------------------------------
# the argument structs, from a table of addresses (made up here, real ones in the GPU tests)
def offsets(c):
    """Floats from an operand's 16-byte aligned buffer to the base the call gets: (`in`, `out`, the other (B, C_out, L) operands)."""
    i = c['in_off'] + c['in_g'] * c['ci'] * c['L'] * c['in_stride']
    o = c['out_g'] * c['co'] * c['L']
    return i, c['out_off'] + o, o


NAMES = ('in_', 'wp', 'bias', 'in_a', 'in_s', 'res', 'res_a', 'res_s', 'add0', 'add1', 'mask_src', 'mask_a', 'mask_s', 'out', 'rowsum_part')


def fake_buffers(c):
    """16-byte aligned addresses nothing reads: per problem a dict operand -> buffer base, and the bases of the shared buffers."""
    n = len(c['ks']) if c['op'] == 'conv' else 1
    per = [{name: 0x10000000 * (i + 1) + 0x800000 * j for j, name in enumerate(NAMES)} for i in range(n)]
    return per, dict(ws=0x70000000, len=0x7f000000, stats_part=0x7e000000)


def _used(c):
    f = c['flags']
    u = {'in_', 'wp', 'out'} | ({'bias'} & f) | ({'res'} & f) | ({'add0'} & f) | ({'add1'} & f)
    u |= {'in_a', 'in_s'} if 'in_aff' in f else set()
    u |= {'res_a', 'res_s'} if 'res_aff' in f else set()
    u |= {'mask_src'} if 'mask' in f else set()
    u |= {'mask_a', 'mask_s'} if 'mask_aff' in f else set()
    u |= {'rowsum_part'} if 'rowsum' in f else set()
    return u


def conv_array(c, per, shared):
    """The v2w_conv1d_args of every problem of a conv record; per[i]: operand -> 16-byte aligned buffer base of problem i.  The workspace
    size is the library's own answer (v2w_conv1d_splitk_ws_bytes), one byte less for ws = 'short'."""
    n = len(c['ks'])
    arr = (_hip.Conv1dArgs * n)()
    oi, oo, oe = offsets(c)
    used = _used(c)
    for i in range(n):
        a, p = arr[i], per[i]
        for name in used:
            off = {'in_': oi, 'out': oo, 'res': oe, 'add0': oe, 'add1': oe, 'mask_src': oe}.get(name, 0)
            setattr(a, name, p[name] + 4 * off)
        a.B, a.C_in, a.C_out, a.L, a.k, a.dil = c['B'], c['ci'], c['co'], c['L'], c['ks'][i], c['dil']
        a.slope, a.algo, a.pad_left, a.accumulate = c['slope'], _hip.ALGO_MFMA, c['pad_left'], int('acc' in c['flags'])
        a.out_div, a.out_slope, a.mask_slope = c['out_div'], c['out_slope'], c['mask_slope'] if 'mask' in c['flags'] else 0.0
        a.in_stride, a.in_phase, a.in_ct, a.out_ct = (c['in_stride'] if c['in_stride'] > 1 else 0), c['in_phase'], c['in_ct'], c['out_ct']
    if c['ws']:
        arr[0].splitk_ws, arr[0].splitk_ws_bytes = shared['ws'], ws_bytes(c) - (c['ws'] == 'short')
    return arr


def convt_struct(c, per, shared):
    t = _hip.ConvT1dArgs()
    p = per[0]
    t.in_, t.wp, t.bias, t.out = p['in_'], p['wp'], p['bias'], p['out']
    t.stats_part = shared['stats_part'] if c['stats'] else None
    t.B, t.C_in, t.C_out, t.L, t.k, t.u, t.slope, t.algo = c['B'], c['ci'], c['co'], c['L'], c['k'], c['u'], c['slope'], _hip.ALGO_MFMA
    if c['ws']:
        t.splitk_ws = shared['ws']
        t.splitk_ws_bytes = ws_bytes(c)
    return t


def ws_bytes(c):
    """Bytes of split workspace the record's launch asks for (0: it does not split), from its sizes alone."""
    lib = _hip.load()
    if c['op'] == 'convt':
        return lib.v2w_convt1d_splitk_ws_bytes(C.byref(convt_struct(dict(c, ws=None, stats=False), *fake_buffers(c))))
    return lib.v2w_conv1d_splitk_ws_bytes(conv_array(dict(c, ws=None), *fake_buffers(c)), len(c['ks']))


def call(c, per, shared, stream=None):
    """Run the record's entry point on the given addresses: with a stream for real, without one through the name sink -> (rc, kernel names)."""
    lib = _hip.load()
    if c['op'] == 'convt':
        t = convt_struct(c, per, shared)
        fn, args = (lib.v2w_convt1d_fwd, (C.byref(t),)) if c['lens'] is None else (lib.v2w_convt1d_fwd_len, (C.byref(t), shared['len'], c['len_mul']))
    else:
        arr = conv_array(c, per, shared)
        n = len(c['ks'])
        if c['lens'] is not None:
            fn, args = lib.v2w_conv1d_fwd_len, (arr, n, shared['len'], c['len_mul'])
        elif n == 1:
            fn, args = lib.v2w_conv1d_fwd, (arr,)
        else:
            fn, args = lib.v2w_conv1d_fwd_multi, (arr, n)
    if stream is None:
        return _hip.kernel_names(fn, *args)
    return fn(*args, stream), None


def dispatch(c):
    """Host-only: (return code, kernels) of the record.  A process without a GPU reports hipErrorNoDevice (100) from the launch status in
    front of the reduce launch, which ends the call there: (OK, names so far, True) - so the reduce kernel's name (`<true>` / `<false>`) is
    pinned only where this runs with a device; the tile kernel's always.  (Vector or element-wise epilogue is a run-time flag, not a template
    argument: no name shows it.  The records' operand alignment and L % 4 select it, and the GPU run exercises it.)"""
    rc, names = call(c, *fake_buffers(c))
    return (OK if rc == 100 else rc), names, rc == 100
