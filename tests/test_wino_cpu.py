"""CPU tests of the Winograd F(2,3) Conv1d path (hipops.ALGO_WINO, ABI v35): the weight transform and its packed layout, the scheme's
accuracy inside the oracle, the C ABI surface (header <-> ctypes) and the kernel the name sink reports.  No GPU needed."""
import os
import re
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import vec2wav_oracle as O
from tests import wino_ref
from wavthruvec_pytorch_amd import _hip, synthetic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return open(os.path.join(ROOT, 'include', 'vec2wav_hip.h')).read()


@pytest.mark.parametrize('k,n', [(3, 4), (5, 7), (7, 10), (9, 12), (11, 15), (2, 0), (1, 0), (4, 0)])
def test_term_counts(k, n):
    if n:
        assert wino_ref.terms(k) == n
    assert _hip.load().v2w_wino_terms(k) == n


@pytest.mark.parametrize('k', [3, 7, 11])
def test_pack_layout_matches_its_definition(k):
    """The vectorised torch reference of the packed stream equals the element-by-element definition of the layout."""
    g = torch.Generator().manual_seed(k)
    wf = torch.randn((k, 64, 64), generator=g)
    a, b = wino_ref.pack_ref(wf), wino_ref.pack_ref_loop(wf)
    assert a.shape == (wino_ref.terms(k) * 64 * 64,) and torch.equal(a, b)


@pytest.mark.parametrize('k,dil,L', [(3, 1, 40), (7, 1, 41), (11, 3, 64), (7, 3, 65), (3, 3, 7), (11, 1, 5), (5, 5, 33), (9, 3, 30)])
def test_transformed_weights_reproduce_the_conv(k, dil, L):
    """The four accumulator classes of output pairs give F.conv1d (fp64: the transform is exact up to rounding), every L mod 2 dil."""
    g = torch.Generator().manual_seed(7 * k + L)
    x = torch.randn((2, 16, L), generator=g, dtype=torch.float64)
    w = torch.randn((8, 16, k), generator=g, dtype=torch.float64)
    b = torch.randn((8,), generator=g, dtype=torch.float64)
    ref = F.conv1d(x, w, b, padding=dil * (k - 1) // 2, dilation=dil)
    got = wino_ref.conv1d(x, w, b, dilation=dil)
    assert (got - ref).abs().max().item() <= 1e-12


def _wino_functional(hits):
    """torch.nn.functional with conv1d replaced by the Winograd scheme for the C_in = C_out >= 64 convs (the wide residual convs)."""
    def conv1d(x, w, bias=None, stride=1, padding=0, dilation=1, groups=1):
        co, ci, k = w.shape
        if ci == co and ci >= 64 and k % 2 == 1 and k >= 3 and stride == 1 and groups == 1 and padding == dilation * (k - 1) // 2:
            hits.append(k)
            return wino_ref.conv1d(x, w, bias, dilation=dilation, padding=padding)
        return F.conv1d(x, w, bias, stride=stride, padding=padding, dilation=dilation, groups=groups)
    ns = types.SimpleNamespace(**{n: getattr(F, n) for n in dir(F) if not n.startswith('__')})
    ns.conv1d = conv1d
    return ns


def test_oracle_with_winograd_convs_stays_on_the_fp32_oracle(monkeypatch):
    """The scheme inside the train-mode oracle at a fixture-sized case: within 5e-7 of the fp32 oracle, and no further from the fp64
    oracle than the fp32 oracle itself (x 1.5)."""
    h = synthetic.make_hparams(num_wv_feat=768)
    sd = synthetic.make_state_dict(h, seed=5)
    inp = synthetic.make_inputs(h, 2, 32, seed=9)
    with torch.no_grad():
        y32, _ = O.generator_forward(sd, h, *inp, training=True, dtype=torch.float32)
        y64, _ = O.generator_forward(sd, h, *inp, training=True, dtype=torch.float64)
        hits = []
        monkeypatch.setattr(O, 'F', _wino_functional(hits))
        yw, _ = O.generator_forward(sd, h, *inp, training=True, dtype=torch.float32)
    assert sorted(set(hits)) == [3, 7, 11] and len(hits) == 18          # 3 stages x 3 branches x 2 convs
    d32 = (yw - y32).abs().max().item()
    assert d32 <= 5e-7, d32
    e_w, e_32 = (yw.double() - y64).abs().max().item(), (y32.double() - y64).abs().max().item()
    assert e_w <= 1.5 * e_32 + 1e-8, (e_w, e_32)


def _struct_fields(header, name):
    end = header.index('} %s;' % name)
    body = header[header.rindex('typedef struct {', 0, end):end]
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    groups = re.findall(r'\b(?:const\s+)?(?:float|double|int32_t|int64_t|void)\s*\*?\s*([a-zA-Z_0-9\[\]]+(?:\s*,\s*[a-zA-Z_0-9\[\]]+)*)\s*;', body)
    return [re.sub(r'\[.*?\]', '', n).strip() for grp in groups for n in grp.split(',')]


def test_abi_v35_surface():
    """ABI v35: V2W_ALGO_WINO, v2w_fold_desc::wpw (last field), v2w_pack_wino / v2w_wino_terms; the ctypes mirrors follow the header."""
    hdr = _header()
    assert int(re.search(r'#define V2W_ABI_VERSION (\d+)', hdr).group(1)) == _hip.ABI_VERSION == 35
    assert int(re.search(r'#define V2W_ALGO_WINO\s+(\d+)', hdr).group(1)) == _hip.ALGO_WINO
    flat = _struct_fields(hdr, 'v2w_fold_desc')
    assert flat == [f[0] for f in _hip.FoldDesc._fields_] and flat[-1] == 'wpw'
    import ctypes as C
    assert _hip.FoldDesc.wpw.offset == _hip.FoldDesc.wpd.offset + 8 and C.sizeof(_hip.FoldDesc) == _hip.FoldDesc.wpw.offset + 8
    for name in ('v2w_pack_wino', 'v2w_wino_terms'):
        assert name in _hip.SIGNATURES and re.search(r'\b%s\s*\(' % name, hdr)
    assert 'v2w_pack_wino' in _hip.LAUNCHERS and 'v2w_wino_terms' not in _hip.LAUNCHERS


def _conv_args(B, C, L, k, dil, algo, ci=None, **extra):
    a = _hip.Conv1dArgs()
    a.in_, a.out, a.wp, a.bias = 0x100000, 0x200000, 0x300000, 0x400
    a.B, a.C_in, a.C_out, a.L, a.k, a.dil, a.slope, a.algo, a.pad_left = B, ci or C, C, L, k, dil, 0.1, algo, -1
    for n, v in extra.items():
        setattr(a, n, v)
    return a


def test_name_sink_reports_the_winograd_kernel():
    """What V2W_ALGO_WINO launches (host-only, nothing is launched): conv_wino_kernel for the residual convs and conv_pre of the benchmark
    shape; V2W_E_SHAPE - and no name - for what the kernel does not take."""
    import ctypes as C
    lib = _hip.load()
    for B, C_, L, k, dil, ci in ((32, 256, 1280, 11, 3, None), (32, 64, 20480, 3, 1, None), (32, 512, 256, 7, 1, 768), (8, 128, 5123, 7, 3, None)):
        rc, names = _hip.kernel_names(lib.v2w_conv1d_fwd, C.byref(_conv_args(B, C_, L, k, dil, _hip.ALGO_WINO, ci)))
        assert rc in (0, 100) and len(names) == 1 and names[0].startswith('conv_wino_kernel<'), (B, C_, L, k, names)
    arr = (_hip.Conv1dArgs * 3)(*[_conv_args(32, 256, 1280, k, 1, _hip.ALGO_WINO) for k in (11, 7, 3)])
    rc, names = _hip.kernel_names(lib.v2w_conv1d_fwd_multi, arr, 3)
    assert rc in (0, 100) and len(names) == 1 and names[0].startswith('conv_wino_kernel<')
    for a in (_conv_args(32, 32, 1280, 3, 1, _hip.ALGO_WINO),                    # C_in < 64
              _conv_args(32, 256, 1280, 4, 1, _hip.ALGO_WINO, pad_left=1),     # even k
              _conv_args(1, 256, 1280, 3, 1, _hip.ALGO_WINO),                  # 40 workgroups: the f32 path splits it over C_in
              _conv_args(32, 256, 1280, 3, 1, _hip.ALGO_WINO, in_stride=2),
              _conv_args(32, 256, 1280, 3, 1, _hip.ALGO_WINO, out_slope=0.2)):
        rc, names = _hip.kernel_names(lib.v2w_conv1d_fwd, C.byref(a))
        assert rc == -2 and names == [], (rc, names)
    # ALGO_AUTO is untouched by the new kernel
    rc, names = _hip.kernel_names(lib.v2w_conv1d_fwd, C.byref(_conv_args(32, 256, 1280, 11, 3, _hip.ALGO_AUTO)))
    assert rc in (0, 100) and names[0].startswith('conv_tile_kernel<')


def test_generator_switch_defaults_on_and_keys_the_launch_plan():
    """Generator.wino defaults on and is part of the launch-plan key, so an A/B in one process re-plans instead of replaying."""
    import inspect
    from wavthruvec_pytorch_amd import Generator
    assert Generator(synthetic.make_hparams()).wino is True
    assert 'self.wino' in inspect.getsource(Generator._plan_key)
