"""CPU tests of the fan-out Winograd launch (hipops.conv1d_wino_fan, v2w_conv1d_wino_fan_fwd): the entry point's dispatch as the library's name
sink reports it (nothing is launched), the planner's selection predicate, the plan key, the planner's call and its fall-back, and that the
fold is asked for nothing new."""
import inspect
import re
import types

import pytest

from wavthruvec_pytorch_amd import _hip, hipops
from wavthruvec_pytorch_amd.forward_plan import ForwardPlanner, wino_fan_selected

STD = [(3, 1), (7, 1), (11, 1)]       # (kernel size, first dilation) of the reference's ResBlock2 triple


def _problems(n, C=64, L=128, ks=(3, 7, 11), dils=(1, 1, 1), B=2, ins=(0x100000,) * 3, **extra):
    arr = (_hip.Conv1dArgs * n)()
    for i in range(n):
        a = arr[i]
        a.in_, a.out, a.wp, a.bias = ins[i], 0x200000 + 0x100000 * i, 0x600000 + 0x10000 * i, 0x400
        a.in_a, a.in_s, a.res, a.res_a, a.res_s = 0x500, 0x600, ins[i], 0x500, 0x600
        a.B, a.C_in, a.C_out, a.L, a.k, a.dil, a.slope, a.algo, a.pad_left = B, C, C, L, ks[i], dils[i], 0.1, hipops.ALGO_WINO, -1
        for q, v in extra.items():
            setattr(a, q, v)
    return arr


@pytest.mark.parametrize('n,kw,want_rc,want', [
    (3, {}, 0, 'conv_wino_fan_kernel<1, 2, 3, true>'),
    (3, dict(L=130), 0, 'conv_wino_fan_kernel<1, 2, 3, false>'),
    (2, {}, 0, 'conv_wino_fan_kernel<1, 2, 3, true>'),
    (1, dict(B=32, L=20480), 0, 'conv_wino_fan_kernel<1, 2, 3, true>'),
    (3, dict(dils=(3, 3, 3), L=1280), 0, 'conv_wino_fan_kernel<1, 2, 3, true>'),
    (3, dict(C=128), -2, None),
    (3, dict(C=96), -2, None),
    (3, dict(ks=(3, 4, 11)), -2, None),
    (3, dict(out_div=3.0), -2, None),
    (3, dict(add0=0x700000), -2, None),
    (3, dict(accumulate=1), -2, None),
    (3, dict(ins=(0x100000, 0x100000, 0x180000)), -1, None),
    (3, dict(dils=(1, 1, 3)), -1, None),
    (3, dict(in_s=0), -1, None),
], ids=['three', 'scalar', 'two', 'one', 'dil3', 'C128', 'C96', 'even_k', 'out_div', 'add0', 'accumulate', 'other_in', 'mixed_dil', 'half_affine'])
def test_dispatch(n, kw, want_rc, want):
    rc, names = _hip.kernel_names(_hip.load().v2w_conv1d_wino_fan_fwd, _problems(n, **kw), n)
    print(rc, names)
    assert (rc in (0, 100) if want_rc == 0 else rc == want_rc) and names == ([want] if want else [])


def test_argument_errors():
    lib = _hip.load()
    assert _hip.kernel_names(lib.v2w_conv1d_wino_fan_fwd, _problems(3), 4) == (-1, [])
    assert _hip.kernel_names(lib.v2w_conv1d_wino_fan_fwd, _problems(3), 0) == (-1, [])
    two = _problems(2)
    two[1].out = two[0].out               # two convs, one output
    assert _hip.kernel_names(lib.v2w_conv1d_wino_fan_fwd, two, 2) == (-1, [])


def test_entry_point_is_declared_and_bound():
    import os
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'vec2wav_hip.h')).read()
    assert re.search(r'\bv2w_conv1d_wino_fan_fwd\s*\(', hdr) and 'v2w_conv1d_wino_fan_fwd' in _hip.LAUNCHERS
    assert _hip.SIGNATURES['v2w_conv1d_wino_fan_fwd'][1][0] == _hip.SIGNATURES['v2w_conv1d_fwd_multi'][1][0]
    assert _hip.ABI_VERSION == 35 and _hip.load().v2w_abi_version() == 35


@pytest.mark.parametrize('wf,precision,algo,C,blocks,kw,want', [
    ((64,), 'f32', hipops.ALGO_AUTO, 64, STD, {}, True),
    ((64,), 'f32', hipops.ALGO_MFMA, 64, [(3, 1), (7, 1)], {}, True),
    ((64,), 'f32', hipops.ALGO_AUTO, 64, [(11, 1)], {}, True),
    ((64, 128), 'f32', hipops.ALGO_AUTO, 128, STD, {}, True),
    ((64,), 'f32', hipops.ALGO_AUTO, 128, STD, {}, False),
    ((), 'f32', hipops.ALGO_AUTO, 64, STD, {}, False),
    (None, 'f32', hipops.ALGO_AUTO, 64, STD, {}, False),
    ((64,), 'bf16', hipops.ALGO_AUTO, 64, STD, {}, False),
    ((64,), 'f16x3', hipops.ALGO_AUTO, 64, STD, {}, False),
    ((64,), 'f32', hipops.ALGO_DIRECT, 64, STD, {}, False),
    ((64,), 'f32', hipops.ALGO_AUTO, 64, STD, dict(save=True), False),
    ((64,), 'f32', hipops.ALGO_AUTO, 64, STD, dict(lengths=True), False),
    ((64,), 'f32', hipops.ALGO_AUTO, 64, STD, dict(streams=False), False),
    ((64,), 'f32', hipops.ALGO_AUTO, 64, [(3, 1), (7, 1), (11, 3)], {}, False),
    ((64,), 'f32', hipops.ALGO_AUTO, 64, [(3, 1), (4, 1), (11, 1)], {}, False),
    ((64,), 'f32', hipops.ALGO_AUTO, 64, STD + [(5, 1)], {}, False),
])
def test_selection_predicate(wf, precision, algo, C, blocks, kw, want):
    assert wino_fan_selected(wf, precision, algo, C, blocks, **kw) is want


@pytest.mark.parametrize('n,B,C,L,dil', [(3, 2, 64, 128, 1), (3, 1, 64, 5376, 1), (3, 1, 64, 5377, 1), (1, 2, 64, 8192, 1), (1, 2, 64, 8194, 1),
                                          (3, 8, 64, 2560, 1), (2, 1, 128, 4096, 3), (2, 1, 128, 4224, 3), (3, 32, 64, 20480, 1)])
def test_size_rule_is_the_librarys(n, B, C, L, dil):
    """hipops.wino_multi_taken against the library: V2W_ALGO_WINO through v2w_conv1d_fwd_multi takes a launch exactly where it says so."""
    arr = _problems(n, C=C, L=L, B=B, dils=(dil,) * 3)
    rc, names = _hip.kernel_names(_hip.load().v2w_conv1d_fwd_multi, arr, n)
    taken = rc in (0, 100) and len(names) == 1
    assert (taken or rc == -2) and taken is hipops.wino_multi_taken(n, B, C, L, dil), (rc, names)


def _generator():
    from wavthruvec_pytorch_amd import Generator, synthetic
    return Generator(synthetic.make_hparams(num_wv_feat=768))


def test_switch_default_plan_key_and_fold():
    g = _generator()
    assert tuple(g.wino_fan) in ((64,), ())          # shipped on only where it was measured faster
    src = inspect.getsource(type(g)._plan_key)
    assert 'self.wino_fan' in src and 'self.wino_sum' in src
    # the fold is asked for nothing new: the same layers get Winograd streams whatever the switch says
    names = (g._wino_sum_layers(), g._wino_stage_layers())
    g.wino_fan = ()
    assert (g._wino_sum_layers(), g._wino_stage_layers()) == names
    g.wino_fan = (64, 128, 256)
    assert (g._wino_sum_layers(), g._wino_stage_layers()) == names
    assert set(g._fold_key) == set(_generator()._fold_key)


def test_plan_key_changes_with_the_switch(monkeypatch):
    import torch
    g = _generator()
    monkeypatch.setattr(torch.cuda, 'current_stream', lambda dev=None: types.SimpleNamespace(cuda_stream=0))
    x = torch.zeros((1, 768, 4))
    g.wino_fan = (64,)
    k1 = g._plan_key(x)
    g.wino_fan = ()
    k0 = g._plan_key(x)
    g.wino_fan = (64,)
    assert k0 != k1 and g._plan_key(x) == k1


def _planner(g, save=None, st=False, lens=None):
    nk = g.num_kernels
    i = [i for i, up in enumerate(g.ups) if up.out_channels == 64][0]
    pl = ForwardPlanner.__new__(ForwardPlanner)
    pl.g, pl.save, pl.st, pl.lens, pl.lmul, pl.stage_i, pl.algo, pl.nk, pl.C = g, save, st, lens, 8, i, g.algo, nk, 64
    pl.S = types.SimpleNamespace(tag=None)
    pl.rbs = [g.resblocks[i * nk + j] for j in range(nk)]
    pl.names = [f'resblocks.{i * nk + j}' for j in range(nk)]
    pl.t1s = [f't1_{j}' for j in range(nk)]
    pl.xr, pl.aff = 'xr', ('a', 's')
    g._profile = None
    g._fold_key['wpw'] = {f'{nm}.convs.0': f'wpw_{j}' for j, nm in enumerate(pl.names)}
    return pl


def test_planner_launches_the_fan_only_in_the_plain_f32_forward(monkeypatch):
    calls = []

    def fake(x, branches, **kw):
        calls.append((pl.S.tag, x, branches, kw))
        return True
    monkeypatch.setattr(hipops, 'conv1d_wino_fan', fake)
    g = _generator()
    g.wino_fan = (64,)
    pl = _planner(g)
    assert pl.conv1_fan() is True
    tag, x, branches, kw = calls.pop()
    assert tag == 'bconv0:resblocks.6.0+resblocks.7.0+resblocks.8.0' and x == 'xr'
    assert [(b[0], b[2], b[3]) for b in branches] == [(f'wpw_{j}', f't1_{j}', rb.kernel_size) for j, rb in enumerate(pl.rbs)]
    assert kw == dict(dil=1, slope=0.1, in_affine=('a', 's'), res='xr', res_affine=('a', 's'), only_if_multi_wino=True)
    # saved for backward, per-item lengths, bf16 storage, the switch off, another precision, the scalar kernels: today's launches
    assert _planner(g, save={}).conv1_fan() is False
    assert _planner(g, lens='lens').conv1_fan() is False
    assert _planner(g, st=True).conv1_fan() is False
    for attr, val in (('wino_fan', ()), ('wino_fan', (128,)), ('precision', 'f16x3'), ('precision', 'bf16'), ('algo', hipops.ALGO_DIRECT)):
        old = getattr(g, attr)
        setattr(g, attr, val)
        assert _planner(g).conv1_fan() is False, (attr, val)
        setattr(g, attr, old)
    # a first conv without its Winograd stream (Generator.wino off): today's launches
    pl = _planner(g)
    del g._fold_key['wpw'][pl.names[1] + '.convs.0']
    assert pl.conv1_fan() is False and calls == []


def test_a_declined_fan_falls_back_to_the_multi_launch(monkeypatch):
    g = _generator()
    g.wino_fan = (64,)
    pl = _planner(g)
    seen = []
    monkeypatch.setattr(hipops, 'conv1d_wino_fan', lambda *a, **k: False)
    monkeypatch.setattr(ForwardPlanner, 'launch', lambda self, sfx, probs: seen.append((sfx, sorted(probs))))
    monkeypatch.setattr(ForwardPlanner, 'conv2_sum', lambda self: True)
    monkeypatch.setattr(ForwardPlanner, 'ck', lambda self, nm, io=3: {})
    pl.wf = {f'{nm}.convs.0': 'wf' for nm in pl.names}
    assert pl.rb2_layers(pl.stage_i) is True and seen == [('0', [0, 1, 2])]
    # taken: no multi-problem launch of the first convs
    seen.clear()
    monkeypatch.setattr(hipops, 'conv1d_wino_fan', lambda *a, **k: True)
    assert pl.rb2_layers(pl.stage_i) is True and seen == []


def test_wrapper_declines_lengths_and_small_launches_without_calling_the_library(monkeypatch):
    import torch
    monkeypatch.setattr(_hip, 'load', lambda: pytest.fail('the library was called'))
    x = torch.zeros((2, 64, 128))
    br = [('wpw', None, torch.zeros((2, 64, 128)), 3)]
    assert hipops.conv1d_wino_fan(x, br, dil=1, slope=0.1, lengths=torch.zeros(2, dtype=torch.int32)) is False
    assert hipops.conv1d_wino_fan(x, br, dil=1, slope=0.1, only_if_multi_wino=True) is False
