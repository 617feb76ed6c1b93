"""Which kernels the tile launchers pick, call by call, as a literal table (host-only: the name sink and the configuration / workspace
queries, made-up pointers that nothing dereferences).  Every branch of launch_tile / v2w_conv1d_mfma / v2w_convt1d_mfma, the Winograd,
split-f16 and bf16 tile launchers, the fused pair kernel and the v2w_pack_mfma* argument checks: a change of the launch code that moves any
call to another instantiation, another return code, another tile count or another split workspace shows here without a GPU.  No GPU needed."""
import ctypes as C

import pytest

from wavthruvec_pytorch_amd import _hip

OK = 0                       # (a GPU-less process reports 100 = hipErrorNoDevice from hipGetLastError behind a call that declined nothing)
ANON = '(anonymous namespace)::'
LEN = 0x500000               # per-item lengths: a device pointer the sink never dereferences


def _tile(args, epi, vec):
    return 'void %sconv_tile_kernel<%s, %d, %s>(%sMultiArgs)' % (ANON, args, epi, 'true' if vec else 'false', ANON)


def _reduce(vec):
    return 'void %ssplitk_reduce_kernel<%s>(%sSplitEpiArgs)' % (ANON, 'true' if vec else 'false', ANON)


def _wino(vec, lens=False):
    return 'void %sconv_wino%s_kernel<1, 2, 3, %s>(%sMultiArgs)' % (ANON, '_len' if lens else '', 'true' if vec else 'false', ANON)


def conv(B, ci, co, L, k, dil, algo=_hip.ALGO_MFMA, **extra):
    a = _hip.Conv1dArgs()
    a.in_, a.out, a.wp, a.bias = 0x100000, 0x200000, 0x300000, 0x400
    a.wps, a.winv, a.wf = 0x600000, 0x700000, 0x800000
    a.B, a.C_in, a.C_out, a.L, a.k, a.dil, a.slope, a.algo, a.pad_left = B, ci, co, L, k, dil, 0.1, algo, -1
    for n, v in extra.items():
        setattr(a, n, v)
    return a


WS = dict(splitk_ws=0x900000, splitk_ws_bytes=1 << 30)

# (id, args of conv(), number of problems (k of problem i = the tuple's i-th entry when k is a tuple), lengths?,
#  -> return code, kernel names, v2w_conv1d_tile_config (code, ten ints), v2w_conv1d_splitk_ws_bytes)
T64 = '32, 1, 1, 1, 2, 2, 32, 2, 4'
T128 = '32, 1, 2, 2, 2, 2, 32, 3, 4'
T128x64 = '32, 1, 2, 1, 2, 2, 32, 2, 4'
T64x64 = '32, 1, 1, 2, 2, 2, 32, 3, 4'
CONV_CASES = [
    # ---- v2w_conv1d_mfma: the 64 x 64 latency tile (B = 1), unsplit without a workspace, split over C_in with one
    ('lat64', dict(B=1, ci=768, co=512, L=64, k=7, dil=1), 1, False, OK, [_tile(T64, 0, True)], (0, [32, 1, 1, 1, 2, 2, 32, 2, 4, 1]), 1048576),
    ('lat64_slab_vec', dict(B=1, ci=768, co=512, L=64, k=7, dil=1, **WS), 1, False, OK, [_tile(T64, 0, True), _reduce(True)],
     (0, [32, 1, 1, 1, 2, 2, 32, 2, 4, 1]), 1048576),
    ('lat64_slab_scalar', dict(B=1, ci=768, co=512, L=62, k=7, dil=1, **WS), 1, False, OK, [_tile(T64, 0, False), _reduce(False)],
     (0, [32, 1, 1, 1, 2, 2, 32, 2, 4, 1]), 1015808),
    ('lat64_slab_out4', dict(B=1, ci=768, co=512, L=64, k=7, dil=1, out=0x200004, **WS), 1, False, OK, [_tile(T64, 0, True), _reduce(False)],
     (0, [32, 1, 1, 1, 2, 2, 32, 2, 4, 1]), 1048576),
    ('lat64_slab_small_ws', dict(B=1, ci=768, co=512, L=64, k=7, dil=1, splitk_ws=0x900000, splitk_ws_bytes=1024), 1, False, OK,
     [_tile(T64, 0, True)], (0, [32, 1, 1, 1, 2, 2, 32, 2, 4, 1]), 1048576),
    ('lat64_slab_n3', dict(B=1, ci=256, co=256, L=128, k=(11, 7, 3), dil=1, **WS), 3, False, OK, [_tile(T64, 0, True), _reduce(True)],
     (0, [32, 1, 1, 1, 2, 2, 32, 2, 4, 2]), 1572864),
    ('lat64_short_chain', dict(B=1, ci=64, co=64, L=640, k=3, dil=1, **WS), 1, False, OK, [_tile(T64, 0, True)],
     (0, [32, 1, 1, 1, 2, 2, 32, 2, 4, 10]), 0),
    ('lat64_len_slab', dict(B=1, ci=768, co=512, L=64, k=7, dil=1, **WS), 1, True, OK, [_tile(T64, 3, True), _reduce(True)], None, None),
    # ---- 128 x 128 and 128 x 64 (tiles128 on either side of 1024), n = 1 and n = 3
    ('t128', dict(B=32, ci=256, co=256, L=2048, k=7, dil=3), 1, False, OK, [_tile(T128, 0, True)], (0, [32, 1, 2, 2, 2, 2, 32, 3, 4, 512]), 0),
    ('t128x64', dict(B=32, ci=256, co=256, L=1280, k=11, dil=5), 1, False, OK, [_tile(T128x64, 0, True)], (0, [32, 1, 2, 1, 2, 2, 32, 2, 4, 640]), 0),
    ('t128_n3', dict(B=32, ci=256, co=256, L=1280, k=(11, 7, 3), dil=1), 3, False, OK, [_tile(T128, 0, True)],
     (0, [32, 1, 2, 1, 2, 2, 32, 2, 4, 640]), 0),
    ('t128_affine_res', dict(B=32, ci=256, co=256, L=2048, k=3, dil=1, in_a=0xa00000, in_s=0xa10000, res=0xb00000, res_a=0xb10000,
                             res_s=0xb20000, add0=0xc00000, add1=0xc10000, out_div=3.0), 1, False, OK, [_tile(T128, 0, True)],
     (0, [32, 1, 2, 2, 2, 2, 32, 3, 4, 512]), 0),
    # ---- EPI 1 (mask, with and without the row sums) and EPI 2 (out_slope)
    ('t128_epi1', dict(B=32, ci=256, co=256, L=2048, k=7, dil=1, mask_src=0xd00000, mask_a=0xd10000, mask_s=0xd20000, mask_slope=0.1), 1, False,
     OK, [_tile(T128, 1, True)], (0, [32, 1, 2, 2, 2, 2, 32, 3, 4, 512]), 0),
    ('t128_epi1_rowsum', dict(B=32, ci=256, co=256, L=2048, k=7, dil=1, mask_src=0xd00000, mask_slope=0.1, rowsum_part=0xe00000), 1, False,
     OK, [_tile(T128, 1, True)], (0, [32, 1, 2, 2, 2, 2, 32, 3, 4, 512]), 0),
    ('t128_epi1_rowsum_unaligned', dict(B=32, ci=256, co=256, L=2046, k=7, dil=1, mask_src=0xd00000, mask_slope=0.1, rowsum_part=0xe00000), 1,
     False, -1, [], (0, [32, 1, 2, 2, 2, 2, 32, 3, 4, 512]), 0),
    ('t128_epi2', dict(B=32, ci=256, co=256, L=2048, k=7, dil=1, out_slope=0.2), 1, False, OK, [_tile(T128, 2, True)],
     (0, [32, 1, 2, 2, 2, 2, 32, 3, 4, 512]), 0),
    ('t128_epi2_novec', dict(B=32, ci=256, co=256, L=2046, k=7, dil=1, out_slope=0.2), 1, False, OK, [_tile(T128, 2, False)],
     (0, [32, 1, 2, 2, 2, 2, 32, 3, 4, 512]), 0),
    ('t128_epi1_novec', dict(B=32, ci=256, co=256, L=2048, k=7, dil=1, in_=0x100004, mask_src=0xd00000, mask_slope=0.1), 1, False, OK,
     [_tile(T128, 1, False)], (0, [32, 1, 2, 2, 2, 2, 32, 3, 4, 512]), 0),
    # ---- VEC true / false: L = 36, L = 37, a base pointer of 4 mod 16, an input stride
    ('vec_L36', dict(B=32, ci=256, co=256, L=36, k=3, dil=1), 1, False, OK, [_tile(T64, 0, True)], (0, [32, 1, 1, 1, 2, 2, 32, 2, 4, 32]), 4718592),
    ('novec_L37', dict(B=32, ci=256, co=256, L=37, k=3, dil=1), 1, False, OK, [_tile(T64, 0, False)], (0, [32, 1, 1, 1, 2, 2, 32, 2, 4, 32]), 4849664),
    ('novec_base4', dict(B=32, ci=256, co=256, L=1280, k=3, dil=1, in_=0x100004), 1, False, OK, [_tile(T128x64, 0, False)],
     (0, [32, 1, 2, 1, 2, 2, 32, 2, 4, 640]), 0),
    ('novec_stride2', dict(B=32, ci=256, co=256, L=1280, k=3, dil=1, in_stride=2, in_phase=1), 1, False, OK, [_tile(T128x64, 0, False)],
     (0, [32, 1, 2, 1, 2, 2, 32, 2, 4, 640]), 0),
    # ---- the 64-row tile, CK = 16, 32 rows, MF = 16
    ('rows64', dict(B=32, ci=64, co=64, L=20480, k=3, dil=1), 1, False, OK, [_tile(T64x64, 0, True)], (0, [32, 1, 1, 2, 2, 2, 32, 3, 4, 5120]), 0),
    ('ck16', dict(B=32, ci=16, co=32, L=20480, k=7, dil=1), 1, False, OK, [_tile('32, 1, 1, 2, 1, 4, 16, 3, 2', 0, True)],
     (0, [32, 1, 1, 2, 1, 4, 16, 3, 2, 2560]), 0),
    ('rows32', dict(B=32, ci=32, co=32, L=20480, k=7, dil=1), 1, False, OK, [_tile('32, 1, 1, 2, 1, 4, 32, 5, 4', 0, True)],
     (0, [32, 1, 1, 2, 1, 4, 32, 5, 4, 2560]), 0),
    ('mf16', dict(B=32, ci=16, co=16, L=40960, k=7, dil=1), 1, False, OK, [_tile('16, 1, 1, 4, 1, 4, 16, 3, 2', 0, True)],
     (0, [16, 1, 1, 4, 1, 4, 16, 3, 2, 5120]), 0),
    ('no_tile', dict(B=2, ci=5, co=3, L=100, k=7, dil=1), 1, False, -2, [], (-2, [0] * 10), 0),
    # ---- both halo-48 variants, and a halo past them
    ('halo48_128', dict(B=64, ci=256, co=256, L=1024, k=5, dil=19), 1, False, OK, [_tile('32, 1, 2, 2, 2, 2, 32, 4, 4', 0, True)],
     (0, [32, 1, 2, 2, 2, 2, 32, 4, 4, 512]), 0),
    ('halo48_64', dict(B=8, ci=128, co=128, L=1024, k=5, dil=19, out_slope=0.1), 1, False, OK, [_tile('32, 1, 1, 2, 2, 2, 32, 4, 4', 2, True)],
     (0, [32, 1, 1, 2, 2, 2, 32, 4, 4, 64]), 0),
    ('halo_50', dict(B=8, ci=128, co=128, L=1024, k=5, dil=25), 1, False, -2, [], (-2, [0] * 10), 0),
    # ---- per-item lengths (v2w_conv1d_fwd_len): EPI 3, VEC true and false, n = 3; refused with another epilogue
    ('len_t128', dict(B=32, ci=256, co=256, L=2048, k=7, dil=3), 1, True, OK, [_tile(T128, 3, True)], None, None),
    ('len_novec', dict(B=32, ci=256, co=256, L=1281, k=7, dil=3), 1, True, OK, [_tile(T128x64, 3, False)], None, None),
    ('len_n3', dict(B=32, ci=256, co=256, L=1280, k=(11, 7, 3), dil=1, algo=_hip.ALGO_AUTO), 3, True, OK, [_tile(T128, 3, True)], None, None),
    ('len_epi2', dict(B=32, ci=256, co=256, L=2048, k=7, dil=3, out_slope=0.2), 1, True, -1, [], None, None),
    # ---- V2W_ALGO_WINO with and without lengths, VEC true and false, n = 3; a launch too small for it
    ('wino', dict(B=32, ci=256, co=256, L=1280, k=11, dil=3, algo=_hip.ALGO_WINO), 1, False, OK, [_wino(True)], None, None),
    ('wino_n3', dict(B=32, ci=256, co=256, L=1280, k=(11, 7, 3), dil=1, algo=_hip.ALGO_WINO), 3, False, OK, [_wino(True)], None, None),
    ('wino_novec', dict(B=32, ci=256, co=256, L=1282, k=7, dil=1, algo=_hip.ALGO_WINO), 1, False, OK, [_wino(False)], None, None),
    ('wino_novec_base4', dict(B=32, ci=256, co=256, L=1280, k=7, dil=1, algo=_hip.ALGO_WINO, in_=0x100004), 1, False, OK, [_wino(False)], None, None),
    ('wino_len', dict(B=32, ci=256, co=256, L=1280, k=11, dil=3, algo=_hip.ALGO_WINO), 1, True, OK, [_wino(True, True)], None, None),
    ('wino_len_novec', dict(B=32, ci=256, co=256, L=1282, k=3, dil=1, algo=_hip.ALGO_WINO), 1, True, OK, [_wino(False, True)], None, None),
    ('wino_small', dict(B=1, ci=256, co=256, L=1280, k=3, dil=1, algo=_hip.ALGO_WINO), 1, False, -2, [], None, None),
    # ---- V2W_ALGO_BF16 (fp32 tensors, bf16 out, bf16 in and out; bf16 in alone does not exist), V2W_ALGO_SPLIT
    ('bf16_io0', dict(B=32, ci=256, co=256, L=1280, k=7, dil=1, algo=_hip.ALGO_BF16), 1, False, OK,
     ['void %sconv_bf16_kernel<1, 4, 2, 2, 3, 0, false, false, 32, true>(%sMultiArgs)' % (ANON, ANON)], None, None),
    ('bf16_io2', dict(B=32, ci=768, co=512, L=256, k=7, dil=1, algo=_hip.ALGO_BF16, io_bf16=2), 1, False, OK,
     ['void %sconv_bf16_kernel<1, 2, 4, 2, 2, 0, false, true, 64, true>(%sMultiArgs)' % (ANON, ANON)], None, None),
    ('bf16_io3', dict(B=32, ci=64, co=64, L=20480, k=3, dil=1, algo=_hip.ALGO_BF16, io_bf16=3), 1, False, OK,
     ['void %sconv_bf16_kernel<1, 4, 2, 2, 5, 0, true, true, 64, true>(%sMultiArgs)' % (ANON, ANON)], None, None),
    ('bf16_io1', dict(B=32, ci=256, co=256, L=1280, k=7, dil=1, algo=_hip.ALGO_BF16, io_bf16=1), 1, False, -2, [], None, None),
    ('bf16_novec', dict(B=32, ci=256, co=256, L=1281, k=7, dil=1, algo=_hip.ALGO_BF16), 1, False, OK,
     ['void %sconv_bf16_kernel<1, 2, 2, 2, 2, 0, false, false, 32, false>(%sMultiArgs)' % (ANON, ANON)], None, None),
    ('bf16_mask_n3', dict(B=32, ci=256, co=256, L=1280, k=(11, 7, 3), dil=1, algo=_hip.ALGO_BF16, mask_src=0xd00000, mask_slope=0.1), 3, False, OK,
     ['void %sconv_bf16_kernel<2, 4, 2, 2, 3, 1, false, false, 32, true>(%sMultiArgs)' % (ANON, ANON)], None, None),
    ('split', dict(B=32, ci=256, co=256, L=1280, k=7, dil=1, algo=_hip.ALGO_SPLIT), 1, False, OK,
     ['void %sconv_split_kernel<2, 2, 2, 2, true, false, 32>(%sMultiArgs)' % (ANON, ANON)], None, None),
    ('split_novec_n3', dict(B=8, ci=128, co=64, L=1281, k=(11, 7, 3), dil=1, algo=_hip.ALGO_SPLIT), 3, False, OK,
     ['void %sconv_split_kernel<2, 2, 1, 4, false, false, 32>(%sMultiArgs)' % (ANON, ANON)], None, None),
]


def _problems(spec, n):
    ks = spec['k'] if isinstance(spec['k'], tuple) else (spec['k'],) * n
    kw = dict(spec)
    arr = (_hip.Conv1dArgs * n)()
    for i in range(n):
        kw['k'] = ks[i]
        arr[i] = conv(**kw)
    return arr


def _ok(rc, want):
    return rc in (0, 100) if want == OK else rc == want


@pytest.mark.parametrize('case', CONV_CASES, ids=[c[0] for c in CONV_CASES])
def test_conv1d_dispatch(case):
    _id, spec, n, lens, want_rc, want_names, want_cfg, want_ws = case
    lib = _hip.load()
    arr = _problems(spec, n)
    if lens:
        rc, names = _hip.kernel_names(lib.v2w_conv1d_fwd_len, arr, n, LEN, 2, short=False)
    elif n == 1:
        rc, names = _hip.kernel_names(lib.v2w_conv1d_fwd, arr, short=False)
    else:
        rc, names = _hip.kernel_names(lib.v2w_conv1d_fwd_multi, arr, n, short=False)
    print(_id, rc, names)
    if rc == 100:
        want_names = want_names[:1]     # (without a device the launch status in front of the reduce launch ends the call)
    assert _ok(rc, want_rc) and names == want_names, (rc, names)
    if want_cfg is not None:
        cfg = (C.c_int32 * 10)()
        crc = lib.v2w_conv1d_tile_config(arr, cfg)
        ws = lib.v2w_conv1d_splitk_ws_bytes(arr, n)
        print(_id, crc, list(cfg), ws)
        assert (crc, list(cfg)) == (want_cfg[0], want_cfg[1]) and ws == want_ws, (crc, list(cfg), ws)


def convt(B, ci, co, L, k, u, **extra):
    t = _hip.ConvT1dArgs()
    t.in_, t.wp, t.out, t.bias = 0x100000, 0x300000, 0x200000, 0x400
    t.B, t.C_in, t.C_out, t.L, t.k, t.u, t.slope, t.algo = B, ci, co, L, k, u, 0.1, _hip.ALGO_MFMA
    for n, v in extra.items():
        setattr(t, n, v)
    return t


# the transposed-conv tiles (CK = 16), by C_out, and their widths in input positions
CONVT_TILES = {64: '32, %d, 1, 1, 2, 2, 16, 1, 2', 32: '32, %d, 1, 1, 1, 4, 16, 2, 2', 16: '16, %d, 1, 2, 1, 4, 16, 2, 2'}
CONVT_NT = {64: 64, 32: 128, 16: 128}
CONVT_CASES = [(u, co) for u in (2, 4, 5, 8) for co in (64, 32, 16)]


@pytest.mark.parametrize('u,co', CONVT_CASES)
def test_convt1d_dispatch(u, co):
    lib = _hip.load()
    L, B = 1280, 32
    k = 2 * u if u % 2 == 0 else 2 * u + 1
    t = convt(B, 2 * co, co, L, k, u, stats_part=0xe00000)
    tile = CONVT_TILES[co] % u
    rc, names = _hip.kernel_names(lib.v2w_convt1d_fwd, C.byref(t), short=False)
    print(u, co, rc, names)
    assert rc in (0, 100) and names == [_tile(tile, 0, True)], (rc, names)
    cfg = (C.c_int32 * 10)()
    assert lib.v2w_convt1d_tile_config(C.byref(t), cfg) == 0
    assert list(cfg) == [int(x) for x in tile.split(', ')] + [B * ((L + CONVT_NT[co] - 1) // CONVT_NT[co])], list(cfg)
    assert lib.v2w_convt1d_splitk_ws_bytes(C.byref(t)) == 0
    # lengths (no fused statistics with them), aligned and not
    t.stats_part = None
    rc, names = _hip.kernel_names(lib.v2w_convt1d_fwd_len, C.byref(t), LEN, 1, short=False)
    assert rc in (0, 100) and names == [_tile(tile, 3, True)], (rc, names)
    t.L = L + 1
    rc, names = _hip.kernel_names(lib.v2w_convt1d_fwd_len, C.byref(t), LEN, 1, short=False)
    assert rc in (0, 100) and names == [_tile(tile, 3, False)], (rc, names)
    rc, names = _hip.kernel_names(lib.v2w_convt1d_fwd, C.byref(t), short=False)
    assert rc in (0, 100) and names == [_tile(tile, 0, False)], (rc, names)


def test_convt1d_split_over_c_in():
    """The first upsampler at B = 1 (512 -> 256, u = 5, k = 11, T = 50): 32 workgroups, 32 chunks x 11 taps -> eight slices and the reduce."""
    lib = _hip.load()
    t = convt(1, 512, 256, 50, 11, 5, splitk_ws=0x900000, splitk_ws_bytes=1 << 30)
    rc, names = _hip.kernel_names(lib.v2w_convt1d_fwd, C.byref(t), short=False)
    print(rc, names)
    assert rc in (0, 100) and names == [_tile('32, 5, 1, 1, 2, 2, 16, 1, 2', 0, False), _reduce(False)][:1 if rc == 100 else 2], (rc, names)
    assert lib.v2w_convt1d_splitk_ws_bytes(C.byref(t)) == 8 * 256 * 250 * 4
    t.stats_part = 0xe00000              # the fused statistics keep the launch whole
    rc, names = _hip.kernel_names(lib.v2w_convt1d_fwd, C.byref(t), short=False)
    assert rc in (0, 100) and names == [_tile('32, 5, 1, 1, 2, 2, 16, 1, 2', 0, False)], (rc, names)
    assert lib.v2w_convt1d_splitk_ws_bytes(C.byref(t)) == 0


def test_resblock_pair_dispatch():
    lib = _hip.load()
    arr = (_hip.PairArgs * 3)()
    for i, k in enumerate((3, 7, 11)):
        p = arr[i]
        p.in_, p.wp1, p.wp2, p.out = 0x100000, 0x300000 + i * 0x10000, 0x400000 + i * 0x10000, 0x200000 + i * 0x100000
        p.B, p.C, p.L, p.k, p.dil1, p.dil2, p.res_mode, p.slope, p.out_div = 32, 32, 20480, k, 1, 3, 0, 0.1, 0.0
    rc, names = _hip.kernel_names(lib.v2w_resblock_pair_fwd, arr, 3, short=False)
    print(rc, names)
    assert rc in (0, 100) and names == ['void %sresblock_pair_kernel<32, 2, 4>(%sPairMulti)' % (ANON, ANON)], (rc, names)
    for i in range(3):
        arr[i].C = 16
    rc, names = _hip.kernel_names(lib.v2w_resblock_pair_fwd, arr, 1, short=False)
    assert rc in (0, 100) and names == ['void %sresblock_pair_kernel<16, 4, 4>(%sPairMulti)' % (ANON, ANON)], (rc, names)
    arr[0].C = 64
    assert _hip.kernel_names(lib.v2w_resblock_pair_fwd, arr, 1) == (-2, [])


def test_pack_mfma_refusals():
    """v2w_pack_mfma / _dgrad / _batch: V2W_E_ARG for a null pointer or a non-positive size, V2W_E_SHAPE for a shape without a tile
    configuration, V2W_E_ARG for a batch outside 1 .. 65535 (checked before everything else) - and the one kernel otherwise."""
    lib = _hip.load()
    WF, WP = 0x100000, 0x200000
    pack = ['%spack_mfma_kernel(float const*, float*, int, int, int, int, int, int, int)' % ANON]

    def names(fn, *args):
        rc, got = _hip.kernel_names(fn, *args, short=False)
        return (0 if rc == 100 else rc), got

    assert names(lib.v2w_pack_mfma, WF, WP, 7, 256, 256, 1) == (0, pack)
    assert names(lib.v2w_pack_mfma, WF, WP, 11, 512, 256, 5) == (0, pack)
    assert names(lib.v2w_pack_mfma_dgrad, WF, WP, 7, 256, 256) == (0, pack)
    assert names(lib.v2w_pack_mfma_batch, WF, WP, 5, 32, 32, 1, 65535) == (0, pack)
    for fn, tail in ((lib.v2w_pack_mfma, (1,)), (lib.v2w_pack_mfma_dgrad, ()), (lib.v2w_pack_mfma_batch, (1, 4))):
        assert names(fn, None, WP, 7, 256, 256, *tail) == (-1, [])
        assert names(fn, WF, None, 7, 256, 256, *tail) == (-1, [])
        assert names(fn, WF, WP, 0, 256, 256, *tail) == (-1, [])
        assert names(fn, WF, WP, 7, -16, 256, *tail) == (-1, [])
        assert names(fn, WF, WP, 7, 256, 0, *tail) == (-1, [])
        assert names(fn, WF, WP, 7, 24, 256, *tail) == (-2, [])          # C_in % 16
        assert names(fn, WF, WP, 7, 256, 24, *tail) == (-2, [])          # C_out neither 16 nor a multiple of 32
    assert names(lib.v2w_pack_mfma, WF, WP, 7, 256, 256, 0) == (-1, [])
    assert names(lib.v2w_pack_mfma, WF, WP, 7, 256, 256, 3) == (-2, [])  # no stride-3 tile
    assert names(lib.v2w_pack_mfma, WF, WP, 7, 256, 48, 2) == (-2, [])
    assert names(lib.v2w_pack_mfma_batch, WF, WP, 7, 256, 256, 0, 4) == (-1, [])
    for n in (0, -1, 65536):
        assert names(lib.v2w_pack_mfma_batch, WF, WP, 7, 256, 256, 1, n) == (-1, [])
        assert names(lib.v2w_pack_mfma_batch, WF, WP, 7, 24, 256, 1, n) == (-1, [])     # the batch size is checked first
