"""The cases of tests/test_disc_kernels_gpu.py, one record each, with the kernels each launches and its return code.

tests/test_disc_ref_cpu.py drives every record through the name sink (`dispatch`, host-only, made-up pointers) and asserts `kernels` and
`rc`; the GPU tests run the same records on real tensors.  One list, two consumers: a case cannot move to another kernel unnoticed.
Kernel names are the short ones of _hip.kernel_name_short."""
import ctypes as C

from wavthruvec_pytorch_amd import _hip

from tests.disc_ref import ceil_div, roundup4

OK = 0
X, OUT, W, AUX, AUX2, SLAB = 0x100000, 0x4000000, 0x8000000, 0x9000000, 0xa000000, 0xb000000     # 16-byte aligned addresses nothing reads


def _case(id, kernels, rc=OK, **kw):
    return dict(id=id, kernels=kernels, rc=rc, **kw)


# ---------------------------------------------------------------------------------------------------------------
# v2w_phase_split / v2w_phase_merge
def _vec(s):
    return ['phase_split_vec_kernel<%d>' % s]


PHASE_SPLIT = []
for _s in (2, 4, 5, 8):
    for _U in (4, 1028):                    # one thread; 257 threads: a second, partial block
        for _B, _C in ((1, 1), (2, 3)):
            PHASE_SPLIT.append(_case('vec_s%d_U%d_BC%d' % (_s, _U, _B * _C), _vec(_s), B=_B, C=_C, Cg=_C, L=_s * _U, inner=1, s=_s,
                                     ipitch=0, opitch=0, out_off=0))
# rows kernel: two groups, L % s in {1, 2}, both pitches past the valid length, opitch > 1024 (gridDim.y = 2)
for _inner, _L in ((13, 238), (17, 239), (19, 238)):
    _Uq = ceil_div(_L, 3)
    PHASE_SPLIT.append(_case('rows_inner%d_L%d' % (_inner, _L), ['phase_split_rows_kernel'], B=2, C=4, Cg=2, L=_L, inner=_inner, s=3,
                             ipitch=_L * _inner + 5, opitch=roundup4(_Uq * _inner) + 8, out_off=0))
# three rows of 2^22 - 4 floats: the division at its largest argument
_OP = (1 << 22) - 4
PHASE_SPLIT.append(_case('rows_opitch_below_2p22', ['phase_split_rows_kernel'], B=1, C=1, Cg=1, L=3 * (_OP // 19) - 1, inner=19, s=3,
                         ipitch=0, opitch=_OP, out_off=0))
# element-wise kernel: an opitch that is no multiple of 4; an output base one float past a 16-byte boundary
PHASE_SPLIT.append(_case('elem_opitch_odd', ['phase_split_kernel'], B=2, C=4, Cg=2, L=20, inner=5, s=3, ipitch=103, opitch=37, out_off=0))
PHASE_SPLIT.append(_case('elem_out_plus_1', ['phase_split_kernel'], B=2, C=4, Cg=2, L=20, inner=13, s=3, ipitch=260, opitch=92, out_off=1))
PHASE_SPLIT.append(_case('elem_vec_shape_out_plus_1', ['phase_split_kernel'], B=2, C=3, Cg=3, L=32, inner=1, s=4, ipitch=0, opitch=0, out_off=1))
PHASE_SPLIT.append(_case('rows_vec_shape_s3', ['phase_split_rows_kernel'], B=2, C=3, Cg=3, L=24, inner=1, s=3, ipitch=0, opitch=0, out_off=0))

PHASE_MERGE = [_case('merge_inner%d_L%d' % (i, L), ['phase_merge_kernel'], B=2, C=4, Cg=2, L=L, inner=i, s=3,
                     ipitch=roundup4(ceil_div(L, 3) * i) + 4, opitch=L * i + 7)
               for i, L in ((13, 238), (19, 20), (1, 50))]


def split_pitches(c):
    Uq = ceil_div(c['L'], c['s'])
    return Uq, c['ipitch'] or c['L'] * c['inner'], c['opitch'] or Uq * c['inner']


# ---------------------------------------------------------------------------------------------------------------
# v2w_unfold1 / v2w_fold1, v2w_unfold_taps, v2w_zero_tail, v2w_avgpool4 (+ backward)
UNFOLD1 = []
for _inner in (13, 19):
    for _short in (0, 1, _inner - 1):       # H*inner - T: no reflect pad, one sample, the longest pad
        _H = 30
        UNFOLD1.append(_case('mpd_inner%d_pad%d' % (_inner, _short), ['unfold1_kernel'], B=2, T=_H * _inner - _short, H=_H, inner=_inner,
                             s=3, k=5, pad=2, rows=16))
UNFOLD1.append(_case('msd', ['unfold1_kernel'], B=3, T=333, H=333, inner=1, s=1, k=15, pad=7, rows=16))
FOLD1 = [dict(c, kernels=['fold1_kernel']) for c in UNFOLD1]


def unfold1_geom(c):
    Uq = (c['H'] + 2 * c['pad'] - c['k']) // c['s'] + 1
    return Uq, roundup4(Uq * c['inner'])


# L = 8: U = 3 and the last output row reads rows 6 .. 10 of 8
UNFOLD_TAPS = [_case('C%d_inner%d' % (Cc, i), ['unfold_taps_kernel'], B=2, C=Cc, L=8, inner=i, s=3, k=5, pad=2,
                     ipitch=8 * i + 3, opitch=roundup4(3 * i) + 4) for Cc in (1, 32) for i in (1, 13)]

ZERO_TAIL = [_case('valid0', ['zero_tail_kernel'], rows=12, pitch=32, valid=0),
             _case('valid_pitch_minus_1', ['zero_tail_kernel'], rows=12, pitch=32, valid=31),
             _case('grid_stride_twice', ['zero_tail_kernel'], rows=90000, pitch=8, valid=5),       # 270 000 > 1024 * 256 elements
             _case('nothing_to_do', [], rows=12, pitch=32, valid=32)]

AVGPOOL = [_case('L%d' % L, ['avgpool4_kernel'], B=3, L=L) for L in (1, 2, 3, 600, 601)]
AVGPOOL_BWD = [dict(c, kernels=['avgpool4_bwd_kernel']) for c in AVGPOOL]

# ---------------------------------------------------------------------------------------------------------------
# v2w_disc_dz / v2w_disc_dz_merge / v2w_rowsum_reduce
# chain: the longest sequential chain of fp32 adds behind one row sum.  pitch <= 256: a wave per row, ceil(pitch / 64) strided adds per lane
# and the 6 butterfly steps of the wave sum.  pitch > 256: a block per row, ceil(pitch / 256) adds per thread, the 6 steps and the 4 wave totals.
def dz_chain(pitch):
    return ceil_div(pitch, 64) + 6 if pitch <= 256 else ceil_div(pitch, 256) + 6 + 4


DZ = []
for _rows, _pitch in [(r, 32) for r in (1, 5, 7, 12)] + [(r, p) for p in (260, 1028) for r in (1, 3)]:
    for _tail in (0, 3):
        for _ops in ('gd', 'g', 'd'):
            DZ.append(_case('rows%d_pitch%d_tail%d_%s' % (_rows, _pitch, _tail, _ops), ['disc_dz_rows_kernel<false>'], rows=_rows, pitch=_pitch,
                            valid=_pitch - _tail, ops=_ops, slope=0.1, rowsum=True, chain=dz_chain(_pitch)))
DZ.append(_case('slope1_pitch32', ['disc_dz_rows_kernel<false>'], rows=5, pitch=32, valid=29, ops='gd', slope=1.0, rowsum=True, chain=dz_chain(32)))
DZ.append(_case('slope1_pitch260', ['disc_dz_rows_kernel<false>'], rows=3, pitch=260, valid=260, ops='d', slope=1.0, rowsum=True, chain=dz_chain(260)))
DZ.append(_case('no_rowsum', ['disc_dz_rows_kernel<false>'], rows=7, pitch=32, valid=30, ops='gd', slope=0.1, rowsum=False, chain=dz_chain(32)))
DZ.append(_case('neither_g_nor_d', ['disc_dz_rows_kernel<false>'], rows=5, pitch=32, valid=30, ops='', slope=0.1, rowsum=True, chain=dz_chain(32)))

# merge form: s = 3, inner = 13, two groups, L % 3 != 0; L = 7 -> pitch 92 (four rows per block), L = 25 -> pitch 328 (one row per block)
DZ_MERGE = [_case('L%d_%s' % (L, 'g' if g else 'nog'), ['disc_dz_rows_kernel<true>'], B=2, C=4, Cg=2, L=L, inner=13, s=3, g=g, slope=0.1,
                  pitch=roundup4(L * 13), dpitch=roundup4(ceil_div(L, 3) * 13) + 4, chain=dz_chain(roundup4(L * 13)))
            for L in (7, 25) for g in (True, False)]

ROWSUM_REDUCE = [_case('C%d_B%d' % (Cc, B), ['rowsum_reduce_kernel'], B=B, C=Cc) for Cc in (1, 64, 65, 1000) for B in (1, 33)]

# ---------------------------------------------------------------------------------------------------------------
# v2w_cout1_wgrad: chain = ceil(L / 256) fmas per thread and batch item (the block sum and the sum over b are fp64)
COUT1 = [_case('L%d_dil%d_k%d_tap%d' % (L, dil, k, tap0), ['cout1_wgrad_kernel'], B=3, C=64, L=L, k=k, dil=dil, tap0=tap0, chain=ceil_div(L, 256))
         for L in (40, 256, 700) for dil in (1, 13, 19) for k in (2, 3) for tap0 in (0, k - 1)]

# ---------------------------------------------------------------------------------------------------------------
# conv forms on the f32 MFMA tile kernel (forward and input gradient) and on the split-f16 kernel
def _tile(args, epi, vec=True):
    return 'conv_tile_kernel<%s, %d, %s>' % (args, epi, 'true' if vec else 'false')


T64 = '32, 1, 1, 1, 2, 2, 32, 2, 4'              # the 64 x 64 latency tile
T32 = '32, 1, 1, 2, 1, 4, 32, 5, 4'               # 32-row tiles: a C_out that is no multiple of 64 (the two-tap layer's 96 input channels)
H48_64 = '32, 1, 1, 2, 2, 2, 32, 4, 4'           # the halo-48 variants
H48_128 = '32, 1, 2, 2, 2, 2, 32, 4, 4'
# G > 1: one problem per group, four per launch (cig x cog per group); tap0 is the forward's, the input gradient runs at k - 1 - tap0
CONV = [
    _case('twotap_Q0', [_tile(T64, 2)], B=2, G=1, cig=96, cog=128, L=364, k=2, dil=13, tap0=0, out_slope=0.1, dgrad=[_tile(T32, 0)]),
    _case('twotap_Q1', [_tile(T64, 2)], B=2, G=1, cig=96, cog=128, L=364, k=2, dil=13, tap0=1, out_slope=0.1, dgrad=[_tile(T32, 0)]),
    _case('halo48_64', [_tile(H48_64, 2)], B=8, G=1, cig=128, cog=128, L=532, k=5, dil=19, tap0=2, out_slope=0.1, dgrad=[_tile(H48_64, 0)]),
    _case('halo48_128', [_tile(H48_128, 2)], B=64, G=1, cig=256, cog=256, L=1064, k=5, dil=19, tap0=2, out_slope=0.1, dgrad=[_tile(H48_128, 0)]),
    _case('grouped_pad1', [_tile(T64, 2)], B=2, G=4, cig=64, cog=64, L=200, k=4, dil=1, tap0=1, out_slope=0.1, dgrad=[_tile(T64, 0)] * 4),
]
SPLIT = [
    _case('split_twotap_zero_third', ['conv_split_kernel<1, 2, 2, 2, true, false, 32>'], dgrad=[], dgrad_rc=_hip.E_SHAPE, B=2, G=1, cig=96, cog=128, L=364, k=3, dil=13, tap0=1, out_slope=0.1, zero_last_tap=True),
    _case('split_grouped_pad1', ['conv_split_kernel<2, 2, 1, 4, true, false, 32>'],
          dgrad=['conv_split_kernel<2, 2, 1, 4, true, false, 32>'] * 4, dgrad_rc=OK, B=2, G=4, cig=64, cog=64, L=200, k=3, dil=1, tap0=0, out_slope=0.1, zero_last_tap=False),
]

# ---------------------------------------------------------------------------------------------------------------
# v2w_wgrad_slice / v2w_wgrad_groups
def _pipe(mf, wco, wci, nt, wide=False):
    return 'wgrad_pipe_kernel<%d, %d, %d, %d, 1, %s>' % (mf, wco, wci, nt, 'true' if wide else 'false')


RED = 'wgrad_reduce_kernel'
WGRAD = []
for _Lq in (20, 128, 300):        # shorter than the halo, exactly one chunk, a ragged third chunk
    WGRAD += [
        _case('nt1_L%d' % _Lq, [_pipe(16, 1, 1, 1), RED], B=3, c_in=16, c_out=32, Lq=_Lq, k=1, dil=1, tap0=0),
        _case('nt2_tap0_L%d' % _Lq, [_pipe(32, 1, 1, 2), RED], B=3, c_in=96, c_out=128, Lq=_Lq, k=2, dil=13, tap0=0),
        _case('nt2_tap1_L%d' % _Lq, [_pipe(32, 1, 1, 2), RED], B=3, c_in=96, c_out=128, Lq=_Lq, k=2, dil=13, tap0=1),
        _case('nt5_dil7_L%d' % _Lq, [_pipe(32, 2, 2, 5), RED], B=3, c_in=64, c_out=64, Lq=_Lq, k=5, dil=7, tap0=2),
        _case('wide_dil13_L%d' % _Lq, [_pipe(32, 2, 2, 5, True), RED], B=3, c_in=64, c_out=128, Lq=_Lq, k=5, dil=13, tap0=2),
        _case('wide_dil19_L%d' % _Lq, [_pipe(32, 2, 2, 5, True), RED], B=3, c_in=64, c_out=64, Lq=_Lq, k=5, dil=19, tap0=2),
        _case('generic_dil19_L%d' % _Lq, ['wgrad_kernel<32>', RED], B=3, c_in=32, c_out=32, Lq=_Lq, k=5, dil=19, tap0=2),
    ]
# Lq % 4 != 0: the generic kernel, whatever the shape
WGRAD += [
    _case('unaligned_nt1', ['wgrad_kernel<16>', RED], B=3, c_in=16, c_out=32, Lq=301, k=1, dil=1, tap0=0),
    _case('unaligned_nt2', ['wgrad_kernel<32>', RED], B=3, c_in=96, c_out=128, Lq=301, k=2, dil=13, tap0=1),
    _case('unaligned_wide', ['wgrad_kernel<32>', RED], B=3, c_in=64, c_out=64, Lq=301, k=5, dil=19, tap0=2),
]
# slices of wider tensors, the pointers at a later group: group `grp` of x (B, x_ct, Lq) and dy (B, dy_ct, Lq)
WGRAD += [
    _case('slice_nt2', [_pipe(32, 1, 1, 2), RED], B=3, c_in=96, c_out=128, Lq=300, k=2, dil=13, tap0=1, x_ct=288, dy_ct=384, grp=2),
    _case('slice_generic', ['wgrad_kernel<32>', RED], B=3, c_in=32, c_out=32, Lq=128, k=5, dil=19, tap0=2, x_ct=64, dy_ct=96, grp=1),
]
WGRAD_GROUPS = [_case('G4_tap1_dil13_L%d' % Lq, [_pipe(32, 1, 1, 2), RED], B=3, c_in=32, c_out=32, Lq=Lq, k=2, dil=13, tap0=1, G=4)
                for Lq in (128, 300)]


# ---------------------------------------------------------------------------------------------------------------
# host-only dispatch of one record: (return code, kernel names)
def _names(fn, *args):
    rc, names = _hip.kernel_names(fn, *args)
    return (OK if rc == 100 else rc), names       # (a process without a GPU reports hipErrorNoDevice behind a call that declined nothing)


def conv_args(c, dgrad=False, algo=_hip.ALGO_MFMA, group=0):
    """The v2w_conv1d_args of group `group` of a CONV / SPLIT record, with made-up pointers (the GPU tests build theirs through hipops)."""
    a = _hip.Conv1dArgs()
    ci, co = (c['cog'], c['cig']) if dgrad else (c['cig'], c['cog'])
    tap0 = c['k'] - 1 - c['tap0'] if dgrad else c['tap0']
    a.in_, a.out, a.wp, a.wf = X + group * ci * c['L'] * 4, OUT + group * co * c['L'] * 4, W, AUX
    a.wps, a.winv = AUX2, AUX2 + 0x100000
    a.bias = None if dgrad else SLAB
    a.B, a.C_in, a.C_out, a.L, a.k, a.dil = c['B'], ci, co, c['L'], c['k'], c['dil']
    a.slope, a.algo, a.pad_left = 1.0, algo, tap0 * c['dil']
    a.out_slope = 0.0 if dgrad else c['out_slope']
    if c['G'] > 1:
        a.in_ct, a.out_ct = c['G'] * ci, c['G'] * co
    return a


def dispatch_conv(c, dgrad=False, algo=_hip.ALGO_MFMA):
    """Forward: the G groups four per launch (v2w_conv1d_fwd_multi); input gradient: one launch per group.  -> (rc, names) over all launches."""
    lib = _hip.load()
    G = c['G']
    if G == 1:
        return _names(lib.v2w_conv1d_fwd, C.byref(conv_args(c, dgrad, algo)))
    names = []
    if dgrad:
        for g in range(G):
            rc, n = _names(lib.v2w_conv1d_fwd, C.byref(conv_args(c, True, algo, g)))
            names += n
            if rc:
                return rc, names
        return OK, names
    for g0 in range(0, G, 4):
        arr = (_hip.Conv1dArgs * 4)()
        for i in range(4):
            arr[i] = conv_args(c, False, algo, g0 + i)
        rc, n = _names(lib.v2w_conv1d_fwd_multi, arr, 4)
        names += n
        if rc:
            return rc, names
    return OK, names


def dispatch(entry, c):
    lib = _hip.load()
    if entry == 'phase_split':
        return _names(lib.v2w_phase_split, X, OUT + 4 * c['out_off'], c['B'], c['C'], c['Cg'], c['L'], c['inner'], c['s'], c['ipitch'], c['opitch'])
    if entry == 'phase_merge':
        return _names(lib.v2w_phase_merge, X, OUT, c['B'], c['C'], c['Cg'], c['L'], c['inner'], c['s'], c['ipitch'], c['opitch'])
    if entry in ('unfold1', 'fold1'):
        fn = lib.v2w_unfold1 if entry == 'unfold1' else lib.v2w_fold1
        return _names(fn, X, OUT, c['B'], c['T'], c['H'], c['inner'], c['s'], c['k'], c['pad'], c['rows'], unfold1_geom(c)[1])
    if entry == 'unfold_taps':
        return _names(lib.v2w_unfold_taps, X, OUT, c['B'], c['C'], c['L'], c['inner'], c['s'], c['k'], c['pad'], c['ipitch'], c['opitch'])
    if entry == 'zero_tail':
        return _names(lib.v2w_zero_tail, X, c['rows'], c['pitch'], c['valid'])
    if entry == 'avgpool4':
        return _names(lib.v2w_avgpool4, X, OUT, c['B'], c['L'])
    if entry == 'avgpool4_bwd':
        return _names(lib.v2w_avgpool4_bwd, X, OUT, c['B'], c['L'])
    if entry == 'disc_dz':
        return _names(lib.v2w_disc_dz, X, AUX if 'g' in c['ops'] else None, AUX2 if 'd' in c['ops'] else None, OUT,
                      SLAB if c['rowsum'] else None, c['rows'], c['pitch'], c['valid'], c['slope'])
    if entry == 'disc_dz_merge':
        return _names(lib.v2w_disc_dz_merge, X, AUX if c['g'] else None, AUX2, OUT, SLAB, c['B'], c['C'], c['Cg'], c['L'], c['inner'], c['s'],
                      c['dpitch'], c['pitch'], c['slope'])
    if entry == 'rowsum_reduce':
        return _names(lib.v2w_rowsum_reduce, X, OUT, c['B'], c['C'])
    if entry == 'cout1_wgrad':
        return _names(lib.v2w_cout1_wgrad, X, AUX, OUT, c['B'], c['C'], c['L'], c['k'], c['dil'], c['tap0'])
    if entry == 'wgrad_slice':
        grp = c.get('grp', 0)
        return _names(lib.v2w_wgrad_slice, X + grp * c['c_in'] * c['Lq'] * 4, AUX + grp * c['c_out'] * c['Lq'] * 4, OUT, SLAB, c['B'], c['c_in'],
                      c['c_out'], c['Lq'], c['k'], c['dil'], c['tap0'], c.get('x_ct', 0), c.get('dy_ct', 0))
    if entry == 'wgrad_groups':
        return _names(lib.v2w_wgrad_groups, X, AUX, OUT, SLAB, c['B'], c['c_in'], c['c_out'], c['Lq'], c['k'], c['dil'], c['tap0'], c['G'])
    raise KeyError(entry)


# entry point -> its records: the dispatch table of tests/test_disc_ref_cpu.py and the parametrisation of tests/test_disc_kernels_gpu.py
TABLE = dict(phase_split=PHASE_SPLIT, phase_merge=PHASE_MERGE, unfold1=UNFOLD1, fold1=FOLD1, unfold_taps=UNFOLD_TAPS, zero_tail=ZERO_TAIL,
             avgpool4=AVGPOOL, avgpool4_bwd=AVGPOOL_BWD, disc_dz=DZ, disc_dz_merge=DZ_MERGE, rowsum_reduce=ROWSUM_REDUCE, cout1_wgrad=COUT1,
             wgrad_slice=WGRAD, wgrad_groups=WGRAD_GROUPS)


def ids(cases):
    return [c['id'] for c in cases]
