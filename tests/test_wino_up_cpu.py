"""CPU tests of the upsampler form of the Winograd kernel (hipops.convt1d_wino, v2w_convt1d_wino_fwd): the fp64 statement of the phase
decomposition and of the packed stream (tests/wino_up_ref.py) against torch's conv_transpose1d, the entry point's dispatch as the library's
name sink reports it (nothing is launched), the host-only shape query, the fold plan's acceptance, and the planner's selection and decline
rules with a stub library."""
import ctypes as C
import inspect
import re
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import wino_up_ref as R
from wavthruvec_pytorch_amd import _hip, hipops
from wavthruvec_pytorch_amd.forward_plan import ForwardPlanner, wino_up_selected, wino_up_shape

SHAPES = [(64, 32, 4, 2), (128, 64, 8, 4), (256, 128, 8, 4)]       # (C_in, C_out, k, u): ups.3, ups.2, ups.1


@pytest.mark.parametrize('ci,co,k,u', SHAPES + [(32, 16, 4, 2), (64, 8, 8, 4)])
@pytest.mark.parametrize('L', [1, 2, 5, 64, 65])
def test_phase_decomposition_and_stream_give_the_transposed_conv(ci, co, k, u, L):
    r = np.random.default_rng(100 * ci + L)
    w = torch.from_numpy(r.standard_normal((ci, co, k)))
    x = torch.from_numpy(r.standard_normal((2, ci, L)))
    bias = torch.from_numpy(r.standard_normal(co))
    want = F.conv_transpose1d(x, w, bias, stride=u, padding=(k - u) // 2)
    # the phase decomposition itself: y[u t + p - pad] = w[p] x[t] + w[p + u] x[t - 1]
    g0, g1 = R.rows_taps(w, u)
    xp = F.pad(x, (1, 1))
    z = torch.matmul(g0, xp[:, :, 0:L + 1]) + torch.matmul(g1, xp[:, :, 1:L + 2])           # [row][t], t = 0 .. L
    y = z.reshape(2, co, u, L + 1).permute(0, 1, 3, 2).reshape(2, co, u * (L + 1))[:, :, u // 2:u // 2 + u * L] + bias[None, :, None]
    assert (y - want).abs().max().item() <= 1e-12 * max(1.0, want.abs().max().item())
    # ... and through the packed stream: pack (fp64 terms), unpack, evaluate the Winograd way
    T = R.terms(w, u)
    if (u * co) % 32 == 0 and ci % 32 == 0:
        term, row, c = R._index(u * co, ci)
        stream = T[torch.from_numpy(term), torch.from_numpy(row), torch.from_numpy(c)].reshape(-1)
        assert stream.numel() == 3 * u * co * ci
        T2 = R.stream_terms(stream, ci, co, u)
        assert torch.equal(T2, T)
        T = T2
    got, S = R.convt_from_terms(T, x, u, bias)
    assert got.shape == want.shape and (got - want).abs().max().item() <= 1e-12 * max(1.0, want.abs().max().item())
    assert bool((S >= got.abs() * (1 - 1e-12)).all())


def test_stream_layout_spot_values():
    """One float of the stream spelled out: row block 1, chunk 1, unit 2, term 1, lane 37, j 3."""
    ci, co, u = 64, 32, 2
    w = torch.arange(ci * co * 2 * u, dtype=torch.float32).reshape(ci, co, 2 * u)
    s = R.stream_ref(w, u)
    o = (((1 * 2 + 1) * 12 + 2 * 3 + 1) * 64 + 37) * 4 + 3
    row, c = 32 + 37 % 32, 32 + 16 + 2 * 3 + 37 // 32
    chan, ph = row // u, row % u
    assert s[o].item() == (w[c, chan, ph + u] + w[c, chan, ph]).item()
    assert s[o - 256].item() == w[c, chan, ph + u].item() and s[o + 256].item() == w[c, chan, ph].item()


def _args(ci=128, co=64, k=8, u=4, B=2, L=64, **extra):
    a = _hip.ConvT1dArgs()
    a.in_, a.wp, a.bias, a.out = 0x100000, 0x200000, 0x400, 0x300000
    a.B, a.C_in, a.C_out, a.L, a.k, a.u, a.slope = B, ci, co, L, k, u, 0.1
    for q, v in extra.items():
        setattr(a, q, v)
    return a


@pytest.mark.parametrize('kw,aff,want_rc,want', [
    ({}, (None, None), 0, 'conv_wino_up_kernel<4, 1, 2, 3, true>'),
    (dict(L=65), (None, None), 0, 'conv_wino_up_kernel<4, 1, 2, 3, false>'),
    (dict(in_=0x100004), (None, None), 0, 'conv_wino_up_kernel<4, 1, 2, 3, false>'),
    (dict(ci=64, co=32, k=4, u=2, B=1, L=1), (0x500, 0x600), 0, 'conv_wino_up_kernel<2, 1, 2, 3, false>'),
    (dict(ci=256, co=128, B=32, L=1280, stats_part=0x700000), (None, None), 0, 'conv_wino_up_kernel<4, 1, 2, 3, true>'),
    (dict(ci=512, co=256, k=11, u=5), (None, None), -2, None),
    (dict(ci=32, co=16, k=4, u=2), (None, None), -2, None),
    (dict(k=4), (None, None), -2, None),
    (dict(ci=64, co=8), (None, None), -2, None),
    (dict(ci=96 + 16), (None, None), -2, None),
    (dict(io_bf16=1), (None, None), -1, None),
    (dict(wp=0), (None, None), -1, None),
    ({}, (0x500, None), -1, None),
], ids=['ups2', 'scalar_L', 'scalar_align', 'ups3_tiny', 'ups1_stats', 'ups0', 'ups4', 'k_not_2u', 'rows32', 'cin112', 'bf16', 'no_stream', 'half_affine'])
def test_dispatch(kw, aff, want_rc, want):
    rc, names = _hip.kernel_names(_hip.load().v2w_convt1d_wino_fwd, C.byref(_args(**kw)), aff[0], aff[1])
    print(rc, names)
    assert (rc in (0, 100) if want_rc == 0 else rc == want_rc) and names == ([want] if want else [])


@pytest.mark.parametrize('kw,tiles,wgs', [
    (dict(B=1, L=1), 1, 4), (dict(B=3, L=127), 3, 12), (dict(B=3, L=128), 6, 24), (dict(B=3, L=129), 6, 24),
    (dict(ci=256, co=128, B=32, L=1280), 32 * 11, 32 * 11 * 8), (dict(ci=64, co=32, k=4, u=2, B=32, L=20480), 32 * 161, 32 * 161),
    (dict(ci=512, co=256, k=11, u=5), 0, 0), (dict(ci=32, co=16, k=4, u=2), 0, 0),
])
def test_shape_query(kw, tiles, wgs):
    """Position tiles: 64 pairs of the L + 1 positions t = 0 .. L; workgroups: tiles x 64-row blocks of the u * C_out rows."""
    a = _args(**kw)
    assert hipops.convt_wino_tiles(a.B, a.C_in, a.C_out, a.L, a.k, a.u) == (tiles, wgs)


def test_entry_points_are_declared_and_bound():
    import os
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'vec2wav_hip.h')).read()
    assert re.search(r'\bv2w_convt1d_wino_fwd\s*\(', hdr) and re.search(r'\bv2w_convt1d_wino_tiles\s*\(', hdr)
    assert 'v2w_convt1d_wino_fwd' in _hip.LAUNCHERS and 'v2w_convt1d_wino_tiles' not in _hip.LAUNCHERS
    assert _hip.ABI_VERSION == 35 and _hip.load().v2w_abi_version() == 35


def _plan(ci, co, k, u, transposed=1, wpw=0x900000):
    d = (_hip.FoldDesc * 1)()
    d[0].v, d[0].wp, d[0].scale, d[0].wpw = 0x100000, 0x200000, 0x300000, wpw
    d[0].c_in, d[0].c_out, d[0].k, d[0].u, d[0].transposed = ci, co, k, u, transposed
    return _hip.load().v2w_fold_plan(d, 1, (C.c_int32 * 4)())


def test_fold_plan_takes_the_stream_of_a_two_phase_tap_upsampler_only():
    for ci, co, k, u in SHAPES:
        assert _plan(ci, co, k, u) > 0
    assert _plan(512, 256, 11, 5) == -1 and _plan(32, 16, 4, 2) == -1 and _plan(128, 64, 4, 4) == -1
    assert _plan(512, 256, 11, 5, wpw=0) > 0
    assert _plan(64, 64, 3, 1, transposed=0) > 0 and _plan(64, 64, 4, 1, transposed=0) == -1        # the Conv1d rule is unchanged


@pytest.mark.parametrize('wu,i,precision,algo,shape,kw,want', [
    ((1, 2, 3), 2, 'f32', hipops.ALGO_AUTO, (128, 64, 8, 4), {}, True),
    ((1, 2, 3), 3, 'f32', hipops.ALGO_MFMA, (64, 32, 4, 2), {}, True),
    ((1,), 2, 'f32', hipops.ALGO_AUTO, (128, 64, 8, 4), {}, False),
    ((), 2, 'f32', hipops.ALGO_AUTO, (128, 64, 8, 4), {}, False),
    (None, 2, 'f32', hipops.ALGO_AUTO, (128, 64, 8, 4), {}, False),
    ((0, 1, 2, 3, 4), 0, 'f32', hipops.ALGO_AUTO, (512, 256, 11, 5), {}, False),
    ((0, 1, 2, 3, 4), 4, 'f32', hipops.ALGO_AUTO, (32, 16, 4, 2), {}, False),
    ((2,), 2, 'bf16', hipops.ALGO_AUTO, (128, 64, 8, 4), {}, False),
    ((2,), 2, 'f16x3', hipops.ALGO_AUTO, (128, 64, 8, 4), {}, False),
    ((2,), 2, 'f32', hipops.ALGO_DIRECT, (128, 64, 8, 4), {}, False),
    ((2,), 2, 'f32', hipops.ALGO_AUTO, (128, 64, 8, 4), dict(save=True), False),
    ((2,), 2, 'f32', hipops.ALGO_AUTO, (128, 64, 8, 4), dict(lengths=True), False),
    ((2,), 2, 'f32', hipops.ALGO_AUTO, (128, 64, 8, 4), dict(stream=False), False),
])
def test_selection_predicate(wu, i, precision, algo, shape, kw, want):
    assert wino_up_selected(wu, i, precision, algo, *shape, **kw) is want


@pytest.mark.parametrize('ci,co,k,u', SHAPES + [(512, 256, 11, 5), (32, 16, 4, 2), (128, 64, 4, 4), (64, 8, 8, 4)])
def test_python_shape_rule_is_the_librarys(ci, co, k, u):
    assert wino_up_shape(ci, co, k, u) is (hipops.convt_wino_tiles(2, ci, co, 64, k, u)[0] > 0)


def _generator():
    from wavthruvec_pytorch_amd import Generator, synthetic
    return Generator(synthetic.make_hparams(num_wv_feat=768))


def test_switch_default_plan_key_and_fold_names():
    g = _generator()
    assert set(g.wino_up) <= {1, 2, 3}               # shipped on only where it was measured faster
    assert 'self.wino_up' in inspect.getsource(type(g)._plan_key)
    g.wino_up = ()
    assert g._wino_up_layers() == set()
    g.wino_up = (0, 1, 2, 3, 4)
    assert g._wino_up_layers() == {'ups.1', 'ups.2', 'ups.3'}
    g.precision = 'bf16'
    assert g._wino_up_layers() == set()


def test_plan_key_changes_with_the_switch(monkeypatch):
    g = _generator()
    monkeypatch.setattr(torch.cuda, 'current_stream', lambda dev=None: types.SimpleNamespace(cuda_stream=0))
    x = torch.zeros((1, 768, 4))
    g.wino_up = (2,)
    k1 = g._plan_key(x)
    g.wino_up = ()
    k0 = g._plan_key(x)
    g.wino_up = (2,)
    assert k0 != k1 and g._plan_key(x) == k1


def _planner(g, i, *, save=None, st=False, lens=None, training=False, B=32, L=5120):
    pl = ForwardPlanner.__new__(ForwardPlanner)
    pl.g, pl.save, pl.st, pl.lens, pl.lmul, pl.algo, pl.training = g, save, st, lens, 1, g.algo, training
    pl.S = types.SimpleNamespace(tag=None)
    pl.B, pl.L, pl.C, pl.dev, pl.up_done, pl.wps, pl.slab = B, L, g.ups[i].out_channels, 'dev', None, {}, None
    pl.cur, pl.xr = 'cur', 'xr'
    pl.wf, pl.wp = {f'ups.{i}': 'wf'}, {f'ups.{i}': 'wp'}
    pl.buf = lambda name, shape, **kw: (name, shape)
    g._profile = None
    g._fold_key['wpw_up'] = {f'ups.{i}': 'wpw'}
    return pl


def test_planner_routes_the_upsampler_only_in_the_plain_f32_forward(monkeypatch):
    calls = []
    tags = []
    monkeypatch.setattr(hipops, 'convt1d_wino', lambda *a, **k: (calls.append(('wino', a, k)), tags.append(pl.S.tag)) and True)
    monkeypatch.setattr(hipops, 'convt1d', lambda *a, **k: calls.append(('direct', a, k)))
    monkeypatch.setattr(hipops, 'convt_stats_tiles', lambda *a: 7)
    g = _generator()
    g.wino_up = (1, 2, 3)
    pl = _planner(g, 2)
    assert pl.upsample(2) == (0, None)
    kind, a, kw = calls.pop()
    assert kind == 'wino' and tags == ['ups.2'] and a[:2] == ('cur', 'wpw') and a[3] == 'xr'
    assert kw == dict(k=8, u=4, slope=0.1, stats_part=None)
    # train mode: the partial rows are the Winograd launch's tiles
    pl = _planner(g, 2, training=True)
    nt, part = pl.upsample(2)
    want_nt = hipops.convt_wino_tiles(32, 128, 64, 5120, 8, 4)[0]
    assert nt == want_nt == 32 * 41 and part == ('bn.part2', (want_nt * 64 * 2,)) and calls.pop()[2]['stats_part'] == part
    # saved for backward, per-item lengths, the switch off, another precision, the scalar kernels, no stream, 128 workgroups or fewer: today's
    for kw2 in (dict(save={}), dict(lens='lens'), dict(B=1, L=128)):
        monkeypatch.setattr(ForwardPlanner, 'lkw', lambda self, mul=None: {})
        _planner(g, 2, **kw2).upsample(2)
        assert calls.pop()[0] == 'direct', kw2
    for attr, val in (('wino_up', ()), ('wino_up', (1,)), ('precision', 'f16x3'), ('algo', hipops.ALGO_DIRECT)):
        old = getattr(g, attr)
        setattr(g, attr, val)
        _planner(g, 2).upsample(2)
        assert calls.pop()[0] == 'direct', (attr, val)
        setattr(g, attr, old)
    pl = _planner(g, 2)
    g._fold_key['wpw_up'] = {}
    pl.upsample(2)
    assert calls.pop()[0] == 'direct' and calls == []
    # ups.0 and ups.4 are not served whatever the switch says
    g.wino_up = (0, 1, 2, 3, 4)
    for i, L in ((0, 256), (4, 40960)):
        _planner(g, i, L=L).upsample(i)
        assert calls.pop()[0] == 'direct'


def test_a_declined_launch_falls_back_to_the_direct_tile_with_its_own_partial_rows(monkeypatch):
    calls = []
    monkeypatch.setattr(hipops, 'convt1d_wino', lambda *a, **k: False)
    monkeypatch.setattr(hipops, 'convt1d', lambda *a, **k: calls.append((a, k)))
    monkeypatch.setattr(hipops, 'convt_stats_tiles', lambda *a: 7)
    monkeypatch.setattr(ForwardPlanner, 'lkw', lambda self, mul=None: {})
    g = _generator()
    g.wino_up = (2,)
    pl = _planner(g, 2, training=True)
    nt, part = pl.upsample(2)
    assert nt == 7 and part == ('bn.part2', (7 * 64 * 2,))
    (a, kw), = calls
    assert a[:2] == ('cur', 'wf') and kw['stats_part'] == part and kw['wp'] == 'wp'
