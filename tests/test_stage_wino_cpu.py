"""Host-only checks of the Winograd form of the fused 32-channel stage kernel: its two entry points in the header, in `_hip.SIGNATURES` and
in the library; which kernel a call reaches (name sink, nothing is launched); and when the planner and the fold choose it.  No GPU needed."""
import ctypes as C
import os
import re

import pytest

from wavthruvec_pytorch_amd import _hip, hipops
from wavthruvec_pytorch_amd.forward_plan import STAGE_WINO_BLOCKS, stage_wino_selected

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'vec2wav_hip.h')
ANON = '(anonymous namespace)::'


def _args(B=32, Cc=32, L=40960, ks=(3, 7, 11), d1=(1, 1, 1), d2=(3, 3, 3)):
    a = _hip.StageArgs()
    a.in_, a.out = 0x100000, 0x200000
    for j, k in enumerate(ks):
        a.wp1[j], a.wp2[j], a.k[j], a.dil1[j], a.dil2[j] = 0x300000 + j * 0x10000, 0x400000 + j * 0x10000, k, d1[j], d2[j]
    a.nk, a.B, a.C, a.L, a.slope, a.out_div = len(ks), B, Cc, L, 0.1, float(len(ks))
    return a


def _kernel(wn, lens=False):
    return 'void %sresblock2_stage_wino_kernel<%d, %s>(%sStageArgs, int)' % (ANON, wn, 'true' if lens else 'false', ANON)


def test_entry_points_in_header_signatures_and_library():
    text = open(HEADER).read()
    assert re.search(r'int v2w_resblock2_stage_wino_fwd\(const v2w_stage_args\* a, void\* stream\);', text)
    assert re.search(r'int v2w_resblock2_stage_wino_tile\(const v2w_stage_args\* a\);', text)
    assert re.search(r'#define V2W_ABI_VERSION 35\b', text), 'new symbols only: the version stays'
    assert _hip.SIGNATURES['v2w_resblock2_stage_wino_fwd'] == (C.c_int, [C.POINTER(_hip.StageArgs), C.c_void_p])
    assert _hip.SIGNATURES['v2w_resblock2_stage_wino_tile'] == (C.c_int, [C.POINTER(_hip.StageArgs)])
    assert _hip.SIGNATURES['v2w_resblock2_stage_wino_fwd'] == _hip.SIGNATURES['v2w_resblock2_stage_fwd'], 'the same struct, the same mirror'
    assert re.search(r'int v2w_resblock2_stage_wino_fwd_len\(const v2w_stage_args\* a, const int32_t\* len, int len_mul, void\* stream\);', text)
    assert _hip.SIGNATURES['v2w_resblock2_stage_wino_fwd_len'] == _hip.SIGNATURES['v2w_resblock2_stage_fwd_len']
    lib = _hip.load()
    assert lib.v2w_resblock2_stage_wino_fwd and lib.v2w_resblock2_stage_wino_tile and lib.v2w_resblock2_stage_wino_fwd_len


def test_stage_wino_dispatch():
    """Windows of 256 positions (224 kept) from 224 workgroups on, of 128 (96 kept) below - the direct kernel's rule - and V2W_E_SHAPE / _ARG
    for what the form does not serve."""
    lib = _hip.load()
    rc, names = _hip.kernel_names(lib.v2w_resblock2_stage_wino_fwd, _args(), short=False)
    assert rc in (0, 100) and names == [_kernel(4)], (rc, names)
    assert hipops.resblock2_stage_wino_tile(32, 32, 40960, [3, 7, 11], [1, 1, 1], [3, 3, 3]) == 224
    rc, names = _hip.kernel_names(lib.v2w_resblock2_stage_wino_fwd, _args(B=1, L=223 * 224), short=False)
    assert rc in (0, 100) and names == [_kernel(2)], (rc, names)
    assert hipops.resblock2_stage_wino_tile(1, 32, 223 * 224, [3, 7, 11], [1, 1, 1], [3, 3, 3]) == 96
    rc, names = _hip.kernel_names(lib.v2w_resblock2_stage_wino_fwd, _args(B=1, L=224 * 224), short=False)
    assert rc in (0, 100) and names == [_kernel(4)], (rc, names)
    # unaligned tensors and L % 4 != 0 run on the same kernels (scalar staging)
    a = _args(L=40961)
    a.in_ = 0x100004
    rc, names = _hip.kernel_names(lib.v2w_resblock2_stage_wino_fwd, a, short=False)
    assert rc in (0, 100) and names == [_kernel(4)], (rc, names)
    for bad in (_args(Cc=16), _args(Cc=64), _args(d1=(1, 3, 1)), _args(ks=(3, 4, 11)), _args(ks=(3, 7, 1))):
        assert _hip.kernel_names(lib.v2w_resblock2_stage_wino_fwd, bad) == (-2, [])
        assert lib.v2w_resblock2_stage_wino_tile(bad) == 0
    post = _args()
    post.post_out = 0x500000
    assert _hip.kernel_names(lib.v2w_resblock2_stage_wino_fwd, post) == (-2, [])
    bwd = _args()
    bwd.bwd_mask2 = 0x500000
    assert _hip.kernel_names(lib.v2w_resblock2_stage_wino_fwd, bwd) == (-2, [])
    null = _args()
    null.wp2[1] = None
    assert _hip.kernel_names(lib.v2w_resblock2_stage_wino_fwd, null) == (-1, [])
    assert _hip.kernel_names(lib.v2w_resblock2_stage_wino_fwd, _args(L=0)) == (-1, [])
    # per-item lengths: the masked instantiations; a null table or len_mul < 1 is an argument error
    LEN = 0x500000
    rc, names = _hip.kernel_names(lib.v2w_resblock2_stage_wino_fwd_len, _args(), LEN, 160, short=False)
    assert rc in (0, 100) and names == [_kernel(4, True)], (rc, names)
    rc, names = _hip.kernel_names(lib.v2w_resblock2_stage_wino_fwd_len, _args(B=1, L=6400), LEN, 160, short=False)
    assert rc in (0, 100) and names == [_kernel(2, True)], (rc, names)
    assert _hip.kernel_names(lib.v2w_resblock2_stage_wino_fwd_len, _args(), None, 160) == (-1, [])
    assert _hip.kernel_names(lib.v2w_resblock2_stage_wino_fwd_len, _args(), LEN, 0) == (-1, [])
    assert _hip.kernel_names(lib.v2w_resblock2_stage_wino_fwd_len, _args(Cc=16), LEN, 160) == (-2, [])
    # the direct form is untouched
    rc, names = _hip.kernel_names(lib.v2w_resblock2_stage_fwd, _args(), short=False)
    assert rc in (0, 100) and names == ['void %sresblock2_stage_kernel<32, 2, 4, false, false, false>(%sStageArgs)' % (ANON, ANON)], (rc, names)


STD = list(STAGE_WINO_BLOCKS)


@pytest.mark.parametrize('flag,precision,algo,Cc,blocks,want', [
    (True, 'f32', hipops.ALGO_AUTO, 32, STD, True),
    (True, 'f32', hipops.ALGO_MFMA, 32, STD, True),
    (False, 'f32', hipops.ALGO_AUTO, 32, STD, False),
    (True, 'f16x3', hipops.ALGO_AUTO, 32, STD, False),
    (True, 'bf16', hipops.ALGO_AUTO, 32, STD, False),
    (True, 'f32', hipops.ALGO_DIRECT, 32, STD, False),
    (True, 'f32', hipops.ALGO_AUTO, 16, STD, False),
    (True, 'f32', hipops.ALGO_AUTO, 64, STD, False),
    (True, 'f32', hipops.ALGO_AUTO, 32, STD[:2], False),
    (True, 'f32', hipops.ALGO_AUTO, 32, [(3, 1, 3), (7, 1, 3), (11, 1, 5)], False),
    (True, 'f32', hipops.ALGO_AUTO, 32, STD[::-1], False),
])
def test_planner_condition(flag, precision, algo, Cc, blocks, want):
    assert stage_wino_selected(flag, precision, algo, Cc, blocks) is want


def test_generator_asks_the_fold_for_the_six_streams_only_when_selected():
    """Generator._wino_stage_layers: both convs of the three blocks of the 32-channel stage, and nothing with the flag off, another precision,
    ALGO_DIRECT or another block set; the flag is part of the plan key."""
    from wavthruvec_pytorch_amd import Generator, synthetic
    h = synthetic.make_hparams(num_wv_feat=768)
    g = Generator(h)
    assert g.wino_stage is True
    i32 = [i for i, up in enumerate(g.ups) if up.out_channels == 32]
    assert len(i32) == 1
    nk = g.num_kernels
    want = {f'resblocks.{i32[0] * nk + j}.convs.{c}' for j in range(nk) for c in (0, 1)}
    assert g._wino_stage_layers() == want and len(want) == 6
    import inspect
    assert 'self.wino_stage' in inspect.getsource(Generator._plan_key)
    g.wino_stage = False
    assert g._wino_stage_layers() == set()
    g.wino_stage = True
    for attr, val in (('precision', 'bf16'), ('precision', 'f16x3'), ('algo', hipops.ALGO_DIRECT)):
        old = getattr(g, attr)
        setattr(g, attr, val)
        assert g._wino_stage_layers() == set(), (attr, val)
        setattr(g, attr, old)
    rb = g.resblocks[i32[0] * nk]
    rb.convs[1].dilation = 5
    assert g._wino_stage_layers() == set()
