"""CPU tests of per-item valid lengths (Generator.forward(lengths=...)): the C ABI surface (the *_fwd_len entry points, header <-> ctypes), what
the name sink reports for launches with lengths and what those entry points refuse, and synthesize's batching helpers.  No GPU needed."""
import ctypes as C
import os
import re

import torch

from wavthruvec_pytorch_amd import _hip, synthesize

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE_LEN = 0x500000         # a device pointer the name sink never dereferences


def _struct_fields(name):
    hdr = open(os.path.join(ROOT, 'include', 'vec2wav_hip.h')).read()
    body = hdr[:hdr.index('} %s;' % name)]
    body = body[body.rindex('typedef struct {'):]
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    return re.findall(r'\b(\w+)(?:\[\d+\])?\s*[;,]', body)


def test_length_entry_points_are_additive():
    """The lengths travel as arguments of four new entry points; the argument structs (and ABI v35 callers) are untouched: every mirror
    still matches its header struct field by field, and the new symbols are declared, bound and treated as launchers."""
    hdr = open(os.path.join(ROOT, 'include', 'vec2wav_hip.h')).read()
    assert int(re.search(r'#define V2W_ABI_VERSION (\d+)', hdr).group(1)) == _hip.ABI_VERSION == _hip.load().v2w_abi_version()
    for cname, mirror in (('v2w_conv1d_args', _hip.Conv1dArgs), ('v2w_convt1d_args', _hip.ConvT1dArgs), ('v2w_stage_args', _hip.StageArgs)):
        names = [n for n, _t in mirror._fields_]
        assert 'len' not in names and _struct_fields(cname) == [n[:-1] if n == 'in_' else n for n in names], cname
    for name in ('v2w_conv1d_fwd_len', 'v2w_convt1d_fwd_len', 'v2w_resblock2_stage_fwd_len', 'v2w_conv_post_tanh_len'):
        assert name in _hip.SIGNATURES and name in _hip.LAUNCHERS and re.search(r'\b%s\s*\(' % name, hdr), name


def _conv_args(B, C_, L, k, dil, algo, ci=None, **extra):
    a = _hip.Conv1dArgs()
    a.in_, a.out, a.wp, a.bias = 0x100000, 0x200000, 0x300000, 0x400
    a.wps, a.winv, a.wf = 0x600000, 0x700000, 0x800000
    a.B, a.C_in, a.C_out, a.L, a.k, a.dil, a.slope, a.algo, a.pad_left = B, ci or C_, C_, L, k, dil, 0.1, algo, -1
    for n, v in extra.items():
        setattr(a, n, v)
    return a


def _conv_len(a, n=1, mul=1, ptr=FAKE_LEN):
    lib = _hip.load()
    return _hip.kernel_names(lib.v2w_conv1d_fwd_len, a if n > 1 else C.byref(a), n, ptr, mul)


def test_name_sink_reports_the_length_kernels():
    lib = _hip.load()
    for algo in (_hip.ALGO_AUTO, _hip.ALGO_MFMA):
        a = _conv_args(32, 512, 256, 7, 1, algo, 768)
        rc, names = _conv_len(a)
        assert rc in (0, 100) and len(names) == 1 and re.fullmatch(r'conv_tile_kernel<32, 1, [^>]*, 3, (true|false)>', names[0]), names
        # the same launch without lengths keeps its name and code (EPI 0)
        rc, plain = _hip.kernel_names(lib.v2w_conv1d_fwd, C.byref(a))
        assert rc in (0, 100) and plain[0] == names[0].replace(', 3, ', ', 0, ')
    a = _conv_args(32, 256, 1280, 11, 3, _hip.ALGO_WINO)
    rc, names = _conv_len(a)
    assert rc in (0, 100) and names and names[0].startswith('conv_wino_len_kernel<'), names
    rc, names = _hip.kernel_names(lib.v2w_conv1d_fwd, C.byref(a))
    assert rc in (0, 100) and names[0].startswith('conv_wino_kernel<')
    arr = (_hip.Conv1dArgs * 3)(*[_conv_args(32, 256, 1280, k, 1, _hip.ALGO_AUTO) for k in (11, 7, 3)])
    rc, names = _conv_len(arr, 3, mul=5)
    assert rc in (0, 100) and len(names) == 1 and ', 3, ' in names[0], names
    # small grid: the split over C_in serves lengths too
    a = _conv_args(1, 512, 64, 7, 1, _hip.ALGO_AUTO, 768)
    a.splitk_ws, a.splitk_ws_bytes = 0x900000, 1 << 30
    rc, names = _conv_len(a)
    assert rc in (0, 100) and names and ', 3, ' in names[0], names
    # transposed conv
    t = _hip.ConvT1dArgs()
    t.in_, t.wp, t.out, t.bias = 0x100000, 0x300000, 0x200000, 0x400
    t.B, t.C_in, t.C_out, t.L, t.k, t.u, t.slope, t.algo = 32, 512, 256, 256, 11, 5, 0.1, _hip.ALGO_AUTO
    rc, names = _hip.kernel_names(lib.v2w_convt1d_fwd_len, C.byref(t), FAKE_LEN, 1)
    assert rc in (0, 100) and re.fullmatch(r'conv_tile_kernel<32, 5, [^>]*, 3, (true|false)>', names[0]), names
    # the stage kernel, with and without the fused tail
    s = _stage_args(16)
    rc, names = _hip.kernel_names(lib.v2w_resblock2_stage_fwd_len, C.byref(s), FAKE_LEN, 160)
    assert rc in (0, 100) and names and all(n.startswith('resblock2_stage_kernel<16,') and n.endswith(', false, false, true>') for n in names)
    rc, plain = _hip.kernel_names(lib.v2w_resblock2_stage_fwd, C.byref(s))
    assert rc in (0, 100) and plain[0].endswith(', false, false, false>')
    s.post_w, s.post_out, s.post_k, s.post_slope = 0xa00000, 0xb00000, 7, 0.01
    rc, names = _hip.kernel_names(lib.v2w_resblock2_stage_fwd_len, C.byref(s), FAKE_LEN, 160)
    assert rc in (0, 100) and names[0].endswith(', true, false, true>'), names
    rc, names = _hip.kernel_names(lib.v2w_conv_post_tanh_len, 0x100000, 0x300000, 0x400, 0x200000, 4, 16, 1000, 7, 0.01, FAKE_LEN, 320)
    assert rc in (0, 100) and names and names[0].startswith('conv_post_tanh_len_kernel<'), names


def _stage_args(Cc, B=32, L=20480):
    s = _hip.StageArgs()
    s.in_, s.out = 0x100000, 0x200000
    for j, (k, d2) in enumerate(((3, 3), (7, 3), (11, 3))):
        s.wp1[j], s.wp2[j], s.k[j], s.dil1[j], s.dil2[j] = 0x300000 + j * 0x10000, 0x400000 + j * 0x10000, k, 1, d2
    s.nk, s.B, s.C, s.L, s.slope, s.out_div = 3, B, Cc, L, 0.1, 3.0
    return s


def test_length_entry_points_refuse_what_their_kernels_do_not_serve():
    """V2W_E_ARG and no kernel named: the kernels without a length form (direct, split-f16, bf16), NULL lengths, len_mul < 1, epilogues the
    length kernels do not carry, the transposed conv's fused statistics and the stage kernel's input-gradient form - nothing runs padded."""
    lib = _hip.load()
    for algo in (_hip.ALGO_SPLIT, _hip.ALGO_BF16, _hip.ALGO_DIRECT):
        assert _conv_len(_conv_args(32, 256, 1280, 7, 1, algo)) == (-1, []), algo
    arr = (_hip.Conv1dArgs * 2)(*[_conv_args(32, 256, 1280, k, 1, _hip.ALGO_SPLIT) for k in (7, 3)])
    assert _conv_len(arr, 2) == (-1, [])
    assert _conv_len(_conv_args(32, 256, 1280, 7, 1, 0), ptr=None) == (-1, [])
    assert _conv_len(_conv_args(32, 256, 1280, 7, 1, 0), mul=0) == (-1, [])
    assert _conv_len(_conv_args(32, 256, 1280, 7, 1, 0, out_slope=0.2)) == (-1, [])
    assert _conv_len(_conv_args(32, 256, 1280, 7, 1, 0, mask_src=0xf00000)) == (-1, [])
    assert _conv_len(_conv_args(32, 256, 640, 7, 1, 0, in_stride=2)) == (-1, [])
    # a shape with no MFMA tile configuration: no direct-kernel fallback with lengths
    assert _conv_len(_conv_args(2, 3, 100, 7, 1, 0, ci=5))[0] == -1
    t = _hip.ConvT1dArgs()
    t.in_, t.wp, t.wf, t.out = 0x100000, 0x300000, 0x800000, 0x200000
    t.B, t.C_in, t.C_out, t.L, t.k, t.u, t.slope, t.algo = 32, 512, 256, 256, 11, 5, 0.1, _hip.ALGO_DIRECT
    assert _hip.kernel_names(lib.v2w_convt1d_fwd_len, C.byref(t), FAKE_LEN, 1) == (-1, [])
    t.algo, t.stats_part = _hip.ALGO_AUTO, 0xc00000
    assert _hip.kernel_names(lib.v2w_convt1d_fwd_len, C.byref(t), FAKE_LEN, 1) == (-1, [])
    s = _stage_args(16)
    for j in range(3):
        s.bwd_mask1[j], s.bwd_mid[j] = 0xc00000, 0xd00000
    s.bwd_mask2, s.slope, s.out_div = 0xe00000, 1.0, 0.0
    assert _hip.kernel_names(lib.v2w_resblock2_stage_fwd_len, C.byref(s), FAKE_LEN, 1) == (-1, [])
    assert _hip.kernel_names(lib.v2w_resblock2_stage_fwd_len, C.byref(_stage_args(16)), None, 1) == (-1, [])


def test_plan_batches_sorts_by_length_and_caps_the_batch():
    assert synthesize.plan_batches([5, 9, 7, 9, 1], 2) == [[1, 3], [2, 0], [4]]
    assert synthesize.plan_batches([3, 4], 8) == [[1, 0]]
    assert synthesize.plan_batches([3, 4, 2], 1) == [[1], [0], [2]]


def test_pad_batch_pads_with_zeros_and_reports_the_lengths():
    feats = [torch.randn(1, 4, t) for t in (5, 9, 7)]
    x, ts = synthesize.pad_batch(feats, [1, 2, 0])
    assert ts == [9, 7, 5] and x.shape == (3, 4, 9)
    assert torch.equal(x[1, :, :7], feats[2][0]) and torch.equal(x[2, :, :5], feats[0][0])
    assert (x[1, :, 7:] == 0).all() and (x[2, :, 5:] == 0).all()


def test_item_noise_is_the_single_run_noise():
    n = synthesize.item_noise(64, 1234)
    ref = torch.randn(1, 64, generator=torch.Generator(device='cpu').manual_seed(1234))
    assert n.shape == (1, 64) and torch.equal(n, ref)


class _FakeGen:
    """Stands in for the Generator on the CPU: y = per-frame mean of x repeated H times (plus a noise/speaker term), so trimming and order
    can be checked without a GPU.  Records the lengths of each call."""

    def __init__(self):
        import types
        self.h = types.SimpleNamespace(upsample_rates=(2, 3), noise_dim=4)
        self.calls = []
        self._p = torch.nn.Parameter(torch.zeros(1))

    def parameters(self):
        yield self._p

    def __call__(self, x, spk, nz, lengths=None):
        self.calls.append(None if lengths is None else list(lengths))
        y = x.mean(1, keepdim=True).repeat_interleave(6, dim=2) + spk[:, :1, None] + nz[:, :1, None]
        if lengths is not None:
            for b, n in enumerate(lengths):
                y[b, :, n * 6:] = 0
        return y


def test_synthesize_many_trims_each_item_and_matches_single_runs():
    g = _FakeGen()
    feats = [torch.randn(1, 3, t) for t in (4, 7, 2)]
    spks = [torch.randn(1, 5) for _ in feats]
    single = [synthesize.synthesize(g, f, s, seed=7) for f, s in zip(feats, spks)]
    g.calls.clear()
    ys = synthesize.synthesize_many(g, feats, spks, seed=7, batch=2)
    assert g.calls == [[7, 4], None]          # longest first, the lone last item as a plain single run
    for y, ref, f in zip(ys, single, feats):
        assert y.shape == (1, 1, f.shape[-1] * 6) and torch.allclose(y, ref)


def test_cli_takes_several_feats_and_spk_embs():
    a = synthesize.parse_args(['--checkpoint', 'c', '--feat', 'a.npy', 'b.npy', 'c.npy', '--spk-emb', 's.pth', '--out', 'wavs', '--batch', '4'])
    assert a.feat == ['a.npy', 'b.npy', 'c.npy'] and a.spk_emb == ['s.pth'] and a.batch == 4
    a = synthesize.parse_args(['--checkpoint', 'c', '--feat', 'a.npy', '--spk-emb', 's.pth', '--out', 'a.wav'])
    assert a.batch == 1 and synthesize.output_paths(a.feat, a.out) == ['a.wav']
    assert synthesize.output_paths(['x/a.npy', 'y/b.npy'], 'o') == [os.path.join('o', 'a.wav'), os.path.join('o', 'b.wav')]
    import pytest
    with pytest.raises(SystemExit):
        synthesize.parse_args(['--checkpoint', 'c', '--feat', 'a.npy', 'b.npy', 'c.npy', '--spk-emb', 's.pth', 't.pth', '--out', 'o'])
