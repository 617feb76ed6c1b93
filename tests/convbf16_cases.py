"""The cases of tests/test_convbf16_kernels_gpu.py: one record per call of v2w_conv1d_fwd / _fwd_multi with V2W_ALGO_BF16 and of
v2w_convt1d_bf16_fwd that lands on csrc/v2w_conv_bf16.hip, with the conv_bf16_kernel instantiation the call must launch, its return code
and its chain lengths n.  tests/test_convbf16_ref_cpu.py drives every record through the configuration query (v2w_conv1d_bf16_config /
v2w_convt1d_bf16_config) and the name sink - host-only, made-up pointers of the record's alignment - and asserts both; the GPU tests run
the same records on real tensors.  Record format, operand draws and the argument builders are tests/split_cases.py's, with three additions:
io (io_bf16: bit 0 `in`, bit 1 `out` / `res` / `add0` / `add1` stored as bf16), BYTE offsets of `in`, `out` and the other (B, C_out, L)
operands from a 16-byte boundary (in_offb, out_offb, e_offb), and an input affine whose ambiguous elements are redrawn (convbf16_ref).

Instantiations: conv_bf16_kernel<MI, NI, WM, WN, NPF, EPI, IN_BF, OUT_BF, CK, VEC>; a tile is 32 MI WM rows x NT = 32 NI WN positions.
What v2w_conv1d_bf16 can return, read off its dispatcher (tiles = sum over the problems of B * ceil(L / 256) * (C_out / 64)); (MI, NI,
WM, WN, CK, VEC) and the storage / epilogue forms each is reachable with:
  C32   (1, 2, 1, 4, 32, true)    C_out == 32, every problem aligned (L % 4 == 0, 16-byte `in`), fp32 tensors           io 0;      mask
  SCAL  (1, 2, 2, 2, 32, false)   any problem with L % 4 != 0 or an unaligned `in`                                     io 0, 2, 3; mask
  T128  (2, 4, 2, 2, 32, true)    C_out % 128 == 0 and tiles >= 1024                                                   io 0, 2, 3; mask
  ONE64 (1, 4, 2, 2, 64, true)    tiles >= 256, C_in == 64, io 3: the single-chunk form                                io 3
  DEEP8 (1, 2, 4, 2, 64, true)    256 <= tiles < 512, n == 1, C_in >= 512, C_in % 64 == 0, io 2, C_out % 128 == 0      io 2
  DEEP4 (1, 2, 2, 2, 64, true)    128 <= tiles < 512, n == 1, C_in >= 512, C_in % 64 == 0, io 2, otherwise             io 2
  T256  (1, 4, 2, 2, 32, true)    tiles >= 256                                                                         io 0, 2, 3; mask
  T64   (1, 2, 2, 2, 32, true)    everything else                                                                      io 0, 2, 3; mask
(the mask epilogue EPI = 1 is fp32-only and io 1 is refused, so ONE64 / DEEP8 / DEEP4 have one form each): 21 tuples.  The transposed conv
(EPI = 2; rows = C_out * UP, UP = u rounded up to a power of two; IN_BF = OUT_BF = (io == 3), which reaches this file only where the
resident-tile kernel does not answer: u not in (2, 4, 5, 8)):
  (2, 4, 2, 2)  rows % 128 == 0 and B * ceil(L / 256) * (rows / 128) >= 512;  (1, 4, 2, 2)  other rows % 64 == 0;  (1, 4, 1, 4)  other
  rows % 32 == 0;  each with VEC true and false: 12 tuples.  REACHABLE lists all 33; the CPU test asserts that the records cover them.

n: k * C_in + ops (short-chain: k + ops), ops per switch as tests/tile_cases.OPS (+ 1 leaky-relu, + 1 out_div); transposed conv:
ceil(k / u) * C_in + 2."""
import ctypes as C

import numpy as np
import torch

from wavthruvec_pytorch_amd import _hip

from tests import convbf16_ref as R
from tests import split_cases as S
from tests.disc_cases import OK, _case, ids  # noqa: F401  (ids: re-exported for the parametrisations)
from tests.disc_ref import ceil_div
from tests.split_cases import ALL_ACC, ALL_ADD, E_ARG, E_SHAPE  # noqa: F401
from tests.tile_cases import OPS

C32, SCAL, T128, ONE64 = (1, 2, 1, 4, 32, True), (1, 2, 2, 2, 32, False), (2, 4, 2, 2, 32, True), (1, 4, 2, 2, 64, True)
DEEP8, DEEP4, T256, T64 = (1, 2, 4, 2, 64, True), (1, 2, 2, 2, 64, True), (1, 4, 2, 2, 32, True), (1, 2, 2, 2, 32, True)
INAME = {C32: 'c32', SCAL: 'scal', T128: 't128', ONE64: 'one64', DEEP8: 'deep8', DEEP4: 'deep4', T256: 't256', T64: 't64'}
IOS = {C32: (0,), SCAL: (0, 2, 3), T128: (0, 2, 3), ONE64: (3,), DEEP8: (2,), DEEP4: (2,), T256: (0, 2, 3), T64: (0, 2, 3)}
CT2, CT1, CT0 = (2, 4, 2, 2), (1, 4, 2, 2), (1, 4, 1, 4)

# every (MI, NI, WM, WN, CK, VEC, EPI, IN_BF, OUT_BF) the two dispatchers can return (see the module docstring)
REACHABLE = {inst + (0, bool(io & 1), bool(io & 2)) for inst, ios in IOS.items() for io in ios}
REACHABLE |= {inst + (1, False, False) for inst in (C32, SCAL, T128, T256, T64)}
REACHABLE |= {t + (32, v, 2, b, b) for t in (CT2, CT1, CT0) for v in (True, False) for b in (False, True)}
assert len(REACHABLE) == 33


def nt_of(inst):
    return 32 * inst[1] * inst[3]


def kernel_name(cfg):
    """The short kernel name of a (MI, NI, WM, WN, CK, VEC, EPI, IN_BF, OUT_BF) tuple; NPF by the launcher's formula."""
    MI, NI, WM, WN, CK, VEC, EPI, IB, OB = cfg
    nth = 64 * WM * WN
    npf = ((CK // 4) * ((32 * NI * WN + 64) // 4) + nth - 1) // nth
    tf = {True: 'true', False: 'false'}
    return 'conv_bf16_kernel<%d, %d, %d, %d, %d, %d, %s, %s, %d, %s>' % (MI, NI, WM, WN, npf, EPI, tf[IB], tf[OB], CK, tf[VEC])


def conv(id, inst, *, B, ci, co, L, k, dil=1, io=0, rc=OK, flags=(), slope=0.1, pad_left=-1, out_div=0.0, mask_slope=0.1, in_offb=0,
         out_offb=0, e_offb=0, short=False, io_alt=None, L_alt=None, null=(), kernels=None, **extra):
    """One conv record.  inst: the (MI, NI, WM, WN, CK, VEC) the call must launch (None with `kernels`: a fallback to another file's kernel,
    or a refusal).  k: an int or a tuple (one problem per entry: _fwd_multi).  io_alt / L_alt: io_bf16 / L of every problem but the first
    (refusals).  extra: in_ct, out_ct, out_slope, in_stride (refusals and the fallback)."""
    ks = k if isinstance(k, tuple) else (k,)
    flags = frozenset(flags)
    assert flags <= set(OPS) - {'rowsum'} and not ({'acc', 'add0'} <= flags) and not (short and 'in_aff' in flags)
    ops = sum(OPS[f] for f in flags) + (slope != 1.0) + (out_div != 0.0)
    cfg = None
    if rc == OK and inst is not None:
        cfg = inst + (int('mask' in flags), bool(io & 1), bool(io & 2))
        kernels = [kernel_name(cfg)]
    macs = B * co * L * ci * max(ks)
    kw = dict(in_ct=0, in_g=0, out_ct=0, out_g=0, in_stride=1, in_phase=0, out_slope=0.0)
    kw.update(extra)
    return _case(id, kernels or [], rc, op='conv', inst=inst, cfg=cfg, B=B, ci=ci, co=co, L=L, ks=ks, dil=dil, io=io, flags=flags,
                 slope=slope, pad_left=pad_left, out_div=out_div, mask_slope=mask_slope, in_offb=in_offb, out_offb=out_offb, e_offb=e_offb,
                 short=short, io_alt=io_alt, L_alt=L_alt, null=tuple(null), data=None, bf=True, in_off=0, out_off=0, ops=ops,
                 n=tuple(kk * (1 if short else ci) + ops for kk in ks), big=macs > 1 << 24, **kw)


def live_channel(c, b):
    """The one live input channel of item b of a short-chain record: b % C_in where the batch covers the channels, else (DEEP8 / DEEP4:
    C_in = 512 against 128 items) spread so that every residue mod 64 - every slot of every k-step of a 64-channel chunk - and every chunk occurs."""
    B, ci = c['B'], c['ci']
    step = max(1, ci // B)
    per = max(1, B // step)
    return (b * step + b // per) % ci


# ---------------------------------------------------------------------------------------------------------------
# Tiles: every instantiation with (k, dil) = (3, 1), (7, 3), (11, 1) and k = 1, dense and short-chain, at the first storage form it
# allows; the other storage forms at (7, 3).  L: one full tile and a partial one where that is cheap; T128 / DEEP8 / DEEP4 (whose thresholds
# need B = 512 or C_in = 512) run these at a short L and have FULL records of their own.  Every shape has two or more chunks but ONE64.
KD = ((3, 1), (7, 3), (11, 1), (1, 1))


def shape(inst, short=False, full=True):
    """B, C_in, C_out and L that reach `inst` (with the io the caller passes)."""
    b = 64 if short else 2
    return {C32: dict(B=b, ci=64, co=32, L=264), SCAL: dict(B=b, ci=64, co=64, L=134),
            T128: dict(B=256, ci=64, co=128, L=264) if full else dict(B=512, ci=64, co=128, L=40),
            ONE64: dict(B=128, ci=64, co=64, L=264),
            DEEP8: dict(B=128, ci=512, co=128, L=132 if full else 24), DEEP4: dict(B=128, ci=512, co=64, L=132 if full else 24),
            T256: dict(B=128, ci=96, co=64, L=264), T64: dict(B=b, ci=64, co=64, L=136)}[inst]


def _both(id, inst, **kw):
    return [conv(id, inst, **shape(inst, False, False), **kw), conv(id + '_short', inst, short=True, **shape(inst, True, False), **kw)]


TILES = []
for _i in (C32, SCAL, T128, ONE64, DEEP8, DEEP4, T256, T64):
    for _k, _d in KD:
        TILES += _both('%s_io%d_k%d_d%d' % (INAME[_i], IOS[_i][0], _k, _d), _i, io=IOS[_i][0], k=_k, dil=_d)
    for _io in IOS[_i][1:]:
        TILES += _both('%s_io%d_k7_d3' % (INAME[_i], _io), _i, io=_io, k=7, dil=3)
# full tiles through the chunk loop on the three that ran short above
FULL = [conv('t128_full_io%d' % _io, T128, io=_io, k=3, **shape(T128)) for _io in (0, 2, 3)]
FULL += [conv('t128_full_io3_ci96_k7', T128, io=3, k=7, dil=3, **dict(shape(T128), ci=96))]            # 21 taps: the pair walk ends on a single
FULL += [conv('deep8_full', DEEP8, io=2, k=7, **shape(DEEP8)), conv('deep4_full', DEEP4, io=2, k=7, **shape(DEEP4))]
# even k with pad_left >= 0; a halo of exactly 32 on both sides; roundup4(pad_left) = 32 for pad_left 29 .. 32
for _i in (T64, T256):
    _n = INAME[_i]
    TILES += _both(_n + '_k4_pad1', _i, k=4, dil=3, pad_left=3)
    TILES += _both(_n + '_k2_pad0', _i, k=2, dil=5, pad_left=0)
    TILES += _both(_n + '_halo32', _i, k=5, dil=16)
    for _p in (29, 30, 31, 32):
        TILES.append(conv('%s_pad%d' % (_n, _p), _i, k=5, dil=10, pad_left=_p, **shape(_i)))
TILES += _both('t64_io3_halo32', T64, io=3, k=5, dil=16)
TILES += _both('t128_io3_halo32', T128, io=3, k=5, dil=16)
TILES += _both('t128_io3_k4_pad3', T128, io=3, k=4, dil=3, pad_left=3)
# the thresholds from below: 1022 tiles (64 x 256), 254 (64 x 128), 126 with a deep layer (64 x 128, 32-channel chunks)
THRESHOLDS = [conv('below_1024', T256, B=511, ci=32, co=128, L=8, k=3), conv('at_1024', T128, B=512, ci=32, co=128, L=8, k=3),
              conv('below_256', T64, B=127, ci=32, co=128, L=8, k=3), conv('at_256', T256, B=128, ci=32, co=128, L=8, k=3),
              conv('at_1024_co512', T128, B=64, ci=32, co=512, L=260, k=3),
              conv('deep_below_128', T64, B=63, ci=512, co=128, L=8, k=3, io=2), conv('deep_at_128', DEEP4, B=64, ci=512, co=128, L=8, k=3, io=2),
              conv('deep_at_256', DEEP8, B=128, ci=512, co=128, L=8, k=3, io=2), conv('deep_at_512', T256, B=256, ci=512, co=128, L=8, k=3, io=2),
              conv('deep_ci544', T256, B=128, ci=544, co=128, L=8, k=3, io=2), conv('deep_n2', T256, B=64, ci=512, co=128, L=8, k=(3, 3), io=2),
              conv('one64_below_256', T64, B=255, ci=64, co=64, L=8, k=3, io=3), conv('one64_io2', T256, B=256, ci=64, co=64, L=8, k=3, io=2)]

# ---------------------------------------------------------------------------------------------------------------
# Lengths: the aligned ones (4, NT, NT + 4) on every vector instantiation, the others (1, 3, NT - 1, NT + 1, 2 NT + 5 for both tile
# widths) on the element-wise one, which every such call reaches; then `in` / `out` / the addends off a 16-byte boundary
LENGTHS = []
for _i in (C32, T128, ONE64, DEEP8, DEEP4, T256, T64):
    for _L in (4, nt_of(_i), nt_of(_i) + 4):
        if _i in (DEEP8, DEEP4) and _L == 132:
            continue                                         # (the FULL records)
        _sh = dict(shape(_i), L=_L)
        if _i in (T128, ONE64, T256) and _L <= 256:
            _sh['B'] *= 2                                    # (one position tile per item: twice the items for the same tile count)
        LENGTHS.append(conv('%s_L%d' % (INAME[_i], _L), _i, io=IOS[_i][0], k=7, dil=3, flags=('bias',), **_sh))
for _L in (1, 3, 127, 129, 130, 255, 257, 261, 517):
    for _io in (0, 2, 3) if _L in (1, 127, 129, 261) else (0,):
        LENGTHS.append(conv('scal_io%d_L%d' % (_io, _L), SCAL, io=_io, k=7, dil=3, flags=('bias',), **dict(shape(SCAL), L=_L)))
for _io, _offs in ((0, (4, 8, 12)), (3, (2, 6, 8))):
    for _o in _offs:
        LENGTHS.append(conv('scal_io%d_in_plus%d' % (_io, _o), SCAL, io=_io, k=7, dil=3, in_offb=_o, flags=('bias', 'res'), **dict(shape(SCAL), L=136)))
for _io, _offs in ((0, (4, 8, 12)), (2, (2, 6, 8)), (3, (2, 6, 8))):
    for _o in _offs:
        LENGTHS.append(conv('t64_io%d_out_plus%d' % (_io, _o), T64, io=_io, k=7, dil=3, out_offb=_o, flags=('bias', 'res'), **shape(T64)))
    LENGTHS.append(conv('t64_io%d_res_plus%d' % (_io, _offs[0]), T64, io=_io, k=7, dil=3, e_offb=_offs[0], flags=('bias', 'res', 'add0', 'add1'), **shape(T64)))
LENGTHS.append(conv('t256_out_plus4', T256, k=7, dil=3, out_offb=4, flags=('bias', 'res'), **shape(T256)))
LENGTHS.append(conv('t256_in_plus8_out_plus12', SCAL, k=7, dil=3, in_offb=8, out_offb=12, flags=('bias',), **dict(shape(T256), B=2)))

# ---------------------------------------------------------------------------------------------------------------
# Prologue and epilogue switches, singly and together, on every epilogue path: T64 fp32 vector (the pipelined `simple` form; with
# addends or a mask the `extra` loop), T64 fp32 with `out` 4 bytes off (vector staging, element-wise epilogue), T64 with bf16 output /
# bf16 tensors (the pipelined OUT_BF forms), SCAL (element-wise staging and epilogue) in fp32 and bf16; then 2 - 4 problems of different k
SWITCHES = [('plain', dict(slope=1.0)), ('in_aff', dict(flags=('in_aff',))), ('bias', dict(flags=('bias',))), ('res', dict(flags=('res',))),
            ('res_aff', dict(flags=('res', 'res_aff'))), ('acc', dict(flags=('acc',))), ('add0', dict(flags=('add0',))),
            ('add01', dict(flags=('add0', 'add1'))), ('out_div3', dict(out_div=3.0)), ('res_aff_div', dict(flags=('res', 'res_aff'), out_div=3.0)),
            ('all_add', dict(flags=ALL_ADD, out_div=3.0)), ('all_acc', dict(flags=ALL_ACC, out_div=3.0)),
            ('n2', dict(k=(7, 3), flags=('bias', 'res'))), ('n3', dict(k=(11, 7, 3), flags=('bias', 'res', 'acc'))),
            ('n4_all', dict(k=(11, 7, 5, 1), flags=ALL_ADD, out_div=3.0))]
MASKS = [('mask', dict(flags=('mask',))), ('mask_aff', dict(flags=('mask', 'mask_aff'))),
         ('mask_all', dict(flags=('mask', 'mask_aff') + ALL_ADD, out_div=3.0))]
PATHS = [('t64', T64, 0, {}), ('t64_escal', T64, 0, dict(out_offb=4)), ('t64_io2', T64, 2, {}), ('t64_io3', T64, 3, {}),
         ('scal', SCAL, 0, dict(L=134)), ('scal_io3', SCAL, 3, dict(L=134))]
EPILOGUES = []
for _pn, _i, _io, _pk in PATHS:
    for _sn, _sk in SWITCHES + (MASKS if _io == 0 else []):
        _q = dict(dict(shape(_i), k=3, L=136), **_pk)
        _q.update(_sk)
        EPILOGUES.append(conv('%s_%s' % (_pn, _sn), _i, io=_io, **_q))
# the mask epilogue and the addends on the wider tiles (EPI = 1 on 64 x 256, 128 x 256, 32 x 256; the pair walk with three streams)
for _i in (T256, T128, C32):
    for _sn, _sk in MASKS:
        EPILOGUES.append(conv('wide_%s_%s' % (INAME[_i], _sn), _i, k=3, **dict(shape(_i, full=False), **_sk)))
for _i, _io in ((T256, 0), (T256, 3), (T128, 0), (T128, 3), (ONE64, 3), (C32, 0)):
    EPILOGUES.append(conv('%s_io%d_all_add' % (INAME[_i], _io), _i, io=_io, k=3, flags=ALL_ADD, out_div=3.0, **shape(_i, full=False)))
    EPILOGUES.append(conv('%s_io%d_all_acc' % (INAME[_i], _io), _i, io=_io, k=3, flags=ALL_ACC, out_div=3.0, **shape(_i, full=False)))
# 128 x 256 with addends on bf16 tensors, the last tile ending inside the SECOND wave column's first pass (L % 256 in (128, 192]; L = 40
# above ends inside the first column's): a live pass behind a dead one in every wave that has positions
EPILOGUES.append(conv('t128_io3_all_add_L168', T128, io=3, k=3, flags=ALL_ADD, out_div=3.0, **dict(shape(T128, full=False), L=168)))
EPILOGUES.append(conv('t128_io3_all_acc_L168', T128, io=3, k=3, flags=ALL_ACC, out_div=3.0, **dict(shape(T128, full=False), L=168)))
for _i in (DEEP8, DEEP4):
    EPILOGUES.append(conv('%s_all_add' % INAME[_i], _i, io=2, k=3, flags=ALL_ADD, out_div=3.0, **shape(_i, full=False)))

# ---------------------------------------------------------------------------------------------------------------
# What the bf16 kernel declines and the split kernel's bf16 form takes (fp32 tensors): a strided input, C_in % 32 != 0
FALLBACK = [conv('fallback_in_stride2', None, B=2, ci=32, co=64, L=72, k=3, flags=('bias',), in_stride=2, in_phase=1,
                 kernels=[S.tile_name(S.T256, False, True)]),
            conv('fallback_ci48', None, B=2, ci=48, co=64, L=72, k=3, flags=('bias', 'res'), kernels=[S.tile_name(S.T256, True, True)])]

# Refusals: the documented code, nothing launched, every buffer's bits left alone
_R = dict(B=2, ci=32, co=64, L=64, k=3)
REFUSALS = [
    conv('io1', None, rc=E_SHAPE, io=1, **_R),
    conv('mask_io2', None, rc=E_SHAPE, io=2, flags=('mask',), **_R),
    conv('mask_io3', None, rc=E_SHAPE, io=3, flags=('mask',), **_R),
    conv('multi_mixed_io', None, rc=E_ARG, io=3, io_alt=2, **dict(_R, k=(3, 3))),
    conv('multi_other_L', None, rc=E_SHAPE, L_alt=60, **dict(_R, k=(3, 3))),
    conv('in_ct', None, rc=E_SHAPE, in_ct=64, **_R),
    conv('out_ct', None, rc=E_SHAPE, out_ct=128, **_R),
    conv('out_slope', None, rc=E_SHAPE, out_slope=0.2, **_R),
    conv('co32_io3', None, rc=E_SHAPE, io=3, **dict(_R, co=32)),
    conv('co32_io2', None, rc=E_SHAPE, io=2, **dict(_R, co=32)),
    conv('co32_in_plus4', None, rc=E_SHAPE, in_offb=4, **dict(_R, co=32)),
    conv('co32_L62', None, rc=E_SHAPE, **dict(_R, co=32, L=62)),
    conv('halo33_io3', None, rc=E_SHAPE, io=3, dil=33, **_R),
    conv('halo34_io2', None, rc=E_SHAPE, io=2, **dict(_R, k=5, dil=17)),
    conv('halo34_fp32', None, rc=E_SHAPE, **dict(_R, k=5, dil=17)),       # (the split kernel's wide-halo forms are split-f16 only)
    conv('pad_left_past_field', None, rc=E_ARG, pad_left=3, **_R),
    conv('pad_left_past_field_io3', None, rc=E_ARG, io=3, pad_left=7, dil=3, **_R),
    conv('n5', None, rc=E_ARG, **dict(_R, k=(3, 3, 3, 3, 3))),
]

CONV_TABLE = dict(tiles=TILES, full=FULL, thresholds=THRESHOLDS, lengths=LENGTHS, epilogues=EPILOGUES, fallback=FALLBACK, refusals=REFUSALS)
CONV_ALL = [c for cases in CONV_TABLE.values() for c in cases]


# ---------------------------------------------------------------------------------------------------------------
# operands on the CPU
def _store(t, bf):
    return R.rne_bf16(t) if bf else t


def operands(c, i=0):
    """split_cases.operands for problem i, then: the record's own short-chain channels, bf16-stored tensors rounded to bf16 (exact inputs
    from there on), and with an input affine the ambiguous elements of x redrawn (convbf16_ref.redraw).  `rounds`: redraw rounds used."""
    o = S.operands(dict(c, short=False), i)
    t, ref, io = o['t'], o['ref'], c['io']
    rng = np.random.default_rng(S._rng(c, i).integers(1 << 30) + 1)
    x = _store(t['x'], io & 1)
    if c['short']:
        live = torch.zeros(c['B'], c['ci'], 1, dtype=torch.bool)
        for b in range(c['B']):
            live[b, live_channel(c, b)] = True
        x = torch.where(live, x, torch.zeros_like(x))
    o['rounds'] = 0
    if 'in_aff' in c['flags']:
        x, o['rounds'] = R.redraw(x, c['slope'], ref['in_a'], ref['in_s'], lambda n: _store(S._f32(rng, n), io & 1))
    t['x'] = x
    for name in ('res', 'add0', 'add1'):
        if name in t:
            t[name] = ref[name] = _store(t[name], io & 2)
    if 'old' in ref:
        ref['old'] = _store(ref['old'], io & 2)
    return o


def ref_kwargs(c, o):
    """The keyword arguments of convbf16_ref.conv1d from a record's operands."""
    return {q: v for q, v in o['ref'].items() if q not in ('in_stride', 'in_phase', 'out_slope')}


# ---------------------------------------------------------------------------------------------------------------
# argument structs from a table of addresses
def problem_io(c, i):
    return c['io'] if (i == 0 or c['io_alt'] is None) else c['io_alt']


def esize(c, name, i=0):
    io = problem_io(c, i)
    return 2 if ((name == 'in_' and io & 1) or (name in ('out', 'res', 'add0', 'add1') and io & 2)) else 4


def byte_offset(c, name):
    return {'in_': c['in_offb'], 'out': c['out_offb']}.get(name, c['e_offb'] if name in ('res', 'add0', 'add1', 'mask_src') else 0)


def conv_array(c, per):
    """The v2w_conv1d_args of every problem; per[i]: operand -> 16-byte aligned buffer base of problem i."""
    arr = S.conv_array(c, per)
    for i, a in enumerate(arr):
        for name in S._used(c, i):
            if byte_offset(c, name):
                setattr(a, name, per[i][name] + byte_offset(c, name))
        a.algo, a.io_bf16 = _hip.ALGO_BF16, problem_io(c, i)
    return arr


def call(c, per, stream=None):
    lib = _hip.load()
    arr, n = conv_array(c, per), len(c['ks'])
    fn, args = (lib.v2w_conv1d_fwd, (arr,)) if n == 1 else (lib.v2w_conv1d_fwd_multi, (arr, n))
    if stream is None:
        return _hip.kernel_names(fn, *args)
    return fn(*args, stream), None


def dispatch(c):
    """Host-only: (return code, kernel names, the configuration query's (MI, NI, WM, WN, CK, VEC, EPI, IN_BF, OUT_BF) or None)."""
    per = S.fake_buffers(c)
    rc, names = call(c, per)
    cfg = (C.c_int32 * 10)()
    q = _hip.load().v2w_conv1d_bf16_config(conv_array(c, per), len(c['ks']), cfg)
    v = list(cfg)
    return (OK if rc == 100 else rc), names, (tuple(v[:4]) + (v[8], bool(v[9]), v[5], bool(v[6]), bool(v[7])) if q == 0 else None)


# ---------------------------------------------------------------------------------------------------------------
# Transposed conv on this kernel: the generator's (k, u) = (11, 5), (8, 4), (4, 2) and (9, 3); rows = C_out * UP on each of the three
# tiles; L = 1, around one tile width and past two; VEC off by L % 4 != 0 or an unaligned `in`; the general epilogue by an unaligned
# `out`; with and without stats_part.  bf16 tensors at u = 3, which the resident-tile kernel does not take.
def convt(id, tile, *, k, u, B, ci, co, L, io=0, vec=None, rc=OK, stats=None, in_offb=0, out_offb=0, slope=0.1):
    """stats: whether the record carries stats_part; None: fp32 records do, bf16 records (tests/bf16res_cases.py passes True) do not."""
    vec = (L % 4 == 0 and in_offb == 0) if vec is None else vec
    cfg = tile + (32, vec, 2, io == 3, io == 3) if rc == OK else None
    return _case(id, [kernel_name(cfg)] if rc == OK else [], rc, op='convt', tile=tile, cfg=cfg, k=k, u=u, B=B, ci=ci, co=co, L=L, io=io,
                 stats=(io == 0) if stats is None else bool(stats), in_offb=in_offb, out_offb=out_offb, slope=slope, n=ceil_div(k, u) * ci + 2,
                 big=B * co * L * u * ci * ceil_div(k, u) > 1 << 24)


KU = ((11, 5), (8, 4), (4, 2), (9, 3))
CONVT = []
for _k, _u in KU:
    _up = R.convt_geom(_k, _u)[0]
    _s = 'k%d_u%d' % (_k, _u)
    for _L in (1, 252, 255, 256, 260, 516):
        CONVT.append(convt('ct1_%s_L%d' % (_s, _L), CT1, k=_k, u=_u, B=2, ci=64, co=64 // _up, L=_L))
    for _L in (1, 511, 512, 516, 1028):
        CONVT.append(convt('ct0_%s_L%d' % (_s, _L), CT0, k=_k, u=_u, B=2, ci=64, co=32 // _up, L=_L))
    for _L in (8, 5, 260):
        CONVT.append(convt('ct2_%s_L%d' % (_s, _L), CT2, k=_k, u=_u, B=512 // ceil_div(_L, 256), ci=64, co=128 // _up, L=_L))
    CONVT.append(convt('ct1_%s_no_stats' % _s, CT1, k=_k, u=_u, B=2, ci=32, co=64 // _up, L=260, stats=False))
    CONVT.append(convt('ct1_%s_in_plus4' % _s, CT1, k=_k, u=_u, B=2, ci=32, co=64 // _up, L=260, in_offb=4))
    CONVT.append(convt('ct1_%s_out_plus8' % _s, CT1, k=_k, u=_u, B=2, ci=32, co=64 // _up, L=260, out_offb=8))
    CONVT.append(convt('ct0_%s_co96' % _s, CT0, k=_k, u=_u, B=2, ci=32, co=96 // _up, L=516))
CONVT.append(convt('ct2_below_512', CT1, k=8, u=4, B=511, ci=32, co=32, L=8))
for _L in (8, 6):
    CONVT.append(convt('ct1_io3_L%d' % _L, CT1, k=9, u=3, B=2, ci=64, co=16, L=_L + 252, io=3))
    CONVT.append(convt('ct0_io3_L%d' % _L, CT0, k=9, u=3, B=2, ci=64, co=8, L=_L + 508, io=3))
    CONVT.append(convt('ct2_io3_L%d' % _L, CT2, k=9, u=3, B=512, ci=64, co=32, L=_L, io=3))
CONVT.append(convt('ct1_io3_out_plus2', CT1, k=9, u=3, B=2, ci=64, co=16, L=260, io=3, out_offb=2))
CONVT_REFUSALS = [convt('ct_odd_k_minus_u', CT1, rc=E_SHAPE, k=8, u=5, B=2, ci=32, co=8, L=64),
                  convt('ct_u9', CT1, rc=E_SHAPE, k=9, u=9, B=2, ci=32, co=4, L=64),
                  convt('ct_ci48', CT1, rc=E_SHAPE, k=8, u=4, B=2, ci=48, co=16, L=64),
                  convt('ct_rows16', CT1, rc=E_SHAPE, k=4, u=2, B=2, ci=32, co=8, L=64),
                  convt('ct_io2', CT1, rc=E_SHAPE, k=9, u=3, B=2, ci=32, co=16, L=64, io=2)]
CONVT_ALL = CONVT + CONVT_REFUSALS

ALL = CONV_ALL + CONVT_ALL
assert len({c['id'] for c in ALL}) == len(ALL)

CT_FAKE = dict(in_=0x10000000, wp=0x20000000, bias=0x30000000, out=0x40000000, stats_part=0x50000000)


def convt_struct(c, addr):
    a = _hip.ConvT1dArgs()
    a.in_, a.wp, a.bias, a.out = addr['in_'] + c['in_offb'], addr['wp'], addr['bias'], addr['out'] + c['out_offb']
    if c['stats']:
        a.stats_part = addr['stats_part']
    a.B, a.C_in, a.C_out, a.L, a.k, a.u = c['B'], c['ci'], c['co'], c['L'], c['k'], c['u']
    a.slope, a.algo, a.io_bf16 = c['slope'], _hip.ALGO_BF16, c['io']
    return a


def convt_dispatch(c):
    """Host-only: (return code, kernel names, the configuration tuple or None, rows of stats_part or the error code)."""
    lib = _hip.load()
    a = convt_struct(c, CT_FAKE)
    rc, names = _hip.kernel_names(lib.v2w_convt1d_bf16_fwd, C.byref(a))
    cfg = (C.c_int32 * 10)()
    q = lib.v2w_convt1d_bf16_config(C.byref(a), cfg)
    v = list(cfg)
    return ((OK if rc == 100 else rc), names, (tuple(v[:4]) + (v[8], bool(v[9]), v[5], bool(v[6]), bool(v[7])) if q == 0 else None),
            lib.v2w_convt1d_bf16_tiles(C.byref(a)))


def convt_operands(c):
    """x (B, C_in, L), wf [k][C_in][C_out], bias (C_out) on the CPU; x holds bf16 numbers where it is stored so."""
    rng = S._rng(c)
    x = _store(S._f32(rng, c['B'], c['ci'], c['L']), c['io'] & 1)
    return x, S._f32(rng, c['k'], c['ci'], c['co'], scale=1.0 / np.sqrt(c['ci'] * c['k'] / c['u'])), S._f32(rng, c['co'])


# v2w_pack_bf16_convt: (k, u, C_in, C_out); a second (exact-phase) region at (11, 5, 32, 32), (9, 3, 32, 32) and (12, 6, 32, 16)
PACKS = [(11, 5, 32, 8), (11, 5, 32, 32), (8, 4, 32, 16), (4, 2, 64, 32), (9, 3, 32, 32), (12, 6, 32, 16), (16, 8, 32, 4), (2, 2, 32, 16)]
