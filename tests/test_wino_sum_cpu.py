"""CPU tests of the summed Winograd launch (hipops.conv1d_wino_sum, v2w_conv1d_wino_sum_fwd): the fp64 reference tests/wino_sum_ref.py against
torch's own conv1d, which kernel each call reaches and what it declines (name sink, made-up pointers), and the planner's condition,
launch tag and fold request.  No GPU needed."""
import types

import pytest
import torch
import torch.nn.functional as F

from tests import wino_sum_ref
from wavthruvec_pytorch_amd import _hip, hipops
from wavthruvec_pytorch_amd.forward_plan import ForwardPlanner, wino_sum_selected


def test_reference_is_the_sum_of_torch_convs():
    g = torch.Generator().manual_seed(3)
    B, C, L, ks, dil = 2, 8, 37, (3, 7, 11), 3
    s01 = float(torch.tensor(0.1, dtype=torch.float32))      # the slope as the kernel sees it: rounded to fp32 (tile_ref._s)
    xs = [torch.randn(B, C, L, generator=g) for _ in ks]
    wfs = [torch.randn(k, C, C, generator=g) for k in ks]
    bs = [torch.randn(C, generator=g) for _ in ks]
    want = sum(x.double() + F.conv1d(F.leaky_relu(x.double(), s01), w.double().permute(2, 1, 0), b.double(), dilation=dil, padding=dil * (k - 1) // 2)
               for x, w, b, k in zip(xs, wfs, bs, ks)) / 3
    got = wino_sum_ref.wino_sum(xs, wfs, bs, dil=dil, slope=0.1, out_div=3.0)
    assert (got - want).abs().max().item() <= 1e-12 * want.abs().max().item()
    # lengths: an item's kept outputs are those of the item cut to its length
    ends = [L, 9]
    cut = wino_sum_ref.wino_sum([x[1:, :, :9] for x in xs], wfs, bs, dil=dil, slope=0.1, out_div=3.0)
    poisoned = [x.clone() for x in xs]
    for x in poisoned:
        x[1, :, 9:] = float('nan')
    got = wino_sum_ref.wino_sum(poisoned, wfs, bs, dil=dil, slope=0.1, out_div=3.0, lengths=ends)
    assert (got[1:, :, :9] - cut).abs().max().item() <= 1e-12


def _sources(n, C=64, L=132, ks=(3, 7, 11), dils=(3, 3, 3), B=2, **extra):
    arr = (_hip.Conv1dArgs * n)()
    for i in range(n):
        a = arr[i]
        a.in_, a.out, a.wp, a.bias = 0x100000 + 0x10000 * i, 0x200000, 0x300000 + 0x10000 * i, 0x400
        a.B, a.C_in, a.C_out, a.L, a.k, a.dil, a.slope, a.algo, a.pad_left, a.out_div = B, C, C, L, ks[i], dils[i], 0.1, hipops.ALGO_WINO, -1, 3.0
        for q, v in extra.items():
            setattr(a, q, v)
    return arr


@pytest.mark.parametrize('n,kw,lens,want_rc,want', [
    (3, {}, False, 0, 'conv_wino_sum_kernel<1, 2, 3, true>'),
    (3, dict(L=134), False, 0, 'conv_wino_sum_kernel<1, 2, 3, false>'),
    (3, dict(C=128), True, 0, 'conv_wino_sum_len_kernel<1, 2, 3, true>'),
    (2, {}, False, 0, 'conv_wino_sum_kernel<1, 2, 3, true>'),
    (1, dict(B=32, L=20480), False, 0, 'conv_wino_sum_kernel<1, 2, 3, true>'),
    (3, dict(in_a=0x500, in_s=0x600), False, -2, None),
    (3, dict(dils=(3, 3, 1)), False, -2, None),
    (3, dict(ks=(3, 4, 11)), False, -2, None),
    (3, dict(C=96), False, -2, None),
    (3, dict(res=0x700000), False, -1, None),
], ids=['three', 'scalar', 'len_C128', 'two', 'one', 'in_a', 'mixed_dil', 'even_k', 'C96', 'res_set'])
def test_dispatch(n, kw, lens, want_rc, want):
    lib = _hip.load()
    rc, names = _hip.kernel_names(lib.v2w_conv1d_wino_sum_fwd, _sources(n, **kw), n, 0x500000 if lens else None, 2)
    print(rc, names)
    assert (rc in (0, 100) if want_rc == 0 else rc == want_rc) and names == ([want] if want else [])


def test_more_than_three_sources_is_an_argument_error():
    rc, names = _hip.kernel_names(_hip.load().v2w_conv1d_wino_sum_fwd, _sources(3), 4, None, 1)
    assert rc == -1 and names == []


@pytest.mark.parametrize('ws,precision,algo,C,blocks,want', [
    ((64,), 'f32', hipops.ALGO_AUTO, 64, [(3, 3), (7, 3), (11, 3)], True),
    ((64,), 'f32', hipops.ALGO_MFMA, 64, [(3, 3), (7, 3)], True),
    ((64,), 'f32', hipops.ALGO_AUTO, 128, [(3, 3), (7, 3), (11, 3)], False),
    ((64, 128), 'f32', hipops.ALGO_AUTO, 128, [(3, 3), (7, 3), (11, 3)], True),
    ((), 'f32', hipops.ALGO_AUTO, 64, [(3, 3), (7, 3), (11, 3)], False),
    ((64,), 'bf16', hipops.ALGO_AUTO, 64, [(3, 3), (7, 3), (11, 3)], False),
    ((64,), 'f16x3', hipops.ALGO_AUTO, 64, [(3, 3), (7, 3), (11, 3)], False),
    ((64,), 'f32', hipops.ALGO_DIRECT, 64, [(3, 3), (7, 3), (11, 3)], False),
    ((64,), 'f32', hipops.ALGO_AUTO, 64, [(3, 3), (7, 3), (11, 5)], False),
    ((64,), 'f32', hipops.ALGO_AUTO, 64, [(3, 3), (4, 3), (11, 3)], False),
    ((64,), 'f32', hipops.ALGO_AUTO, 64, [(3, 3)], False),
    ((32,), 'f32', hipops.ALGO_AUTO, 32, [(3, 3), (7, 3), (11, 3)], False),
])
def test_planner_condition(ws, precision, algo, C, blocks, want):
    assert wino_sum_selected(ws, precision, algo, C, blocks) is want


def _generator():
    from wavthruvec_pytorch_amd import Generator, synthetic
    return Generator(synthetic.make_hparams(num_wv_feat=768))


def test_generator_asks_the_fold_for_the_second_convs_of_the_selected_stages():
    g = _generator()
    nk = g.num_kernels
    i64 = [i for i, up in enumerate(g.ups) if up.out_channels == 64]
    assert g.wino_sum == (64,) and len(i64) == 1
    assert g._wino_sum_layers() == {f'resblocks.{i64[0] * nk + j}.convs.1' for j in range(nk)}
    import inspect
    assert 'self.wino_sum' in inspect.getsource(type(g)._plan_key)
    g.wino_sum = ()
    assert g._wino_sum_layers() == set()
    g.wino_sum = (64,)
    g.precision = 'bf16'
    assert g._wino_sum_layers() == set()


def _planner(g, save=None, st=False, lens=None):
    nk = g.num_kernels
    i = [i for i, up in enumerate(g.ups) if up.out_channels == 64][0]
    pl = ForwardPlanner.__new__(ForwardPlanner)
    pl.g, pl.save, pl.st, pl.lens, pl.lmul, pl.stage_i, pl.algo, pl.nk, pl.C = g, save, st, lens, 8, i, g.algo, nk, 64
    pl.S = types.SimpleNamespace(tag=None)
    pl.rbs = [g.resblocks[i * nk + j] for j in range(nk)]
    pl.names = [f'resblocks.{i * nk + j}' for j in range(nk)]
    pl.t1s = [f't1_{j}' for j in range(nk)]
    pl.xs = 'xs'
    g._profile = None
    g._fold_key['wpw_sum'] = {f'{nm}.convs.1': f'wpw_{j}' for j, nm in enumerate(pl.names)}
    return pl


def test_planner_launches_the_sum_only_in_the_plain_f32_forward(monkeypatch):
    calls = []

    def fake(sources, out, **kw):
        calls.append((pl.S.tag, sources, out, kw))
        return True
    monkeypatch.setattr(hipops, 'conv1d_wino_sum', fake)
    g = _generator()
    pl = _planner(g)
    assert pl.conv2_sum() is True
    tag, sources, out, kw = calls.pop()
    assert tag == 'bconv1:' + '+'.join(f'{nm}.1' for nm in pl.names) and out == 'xs'
    assert [(s[0], s[1], s[3]) for s in sources] == [(f't1_{j}', f'wpw_{j}', rb.kernel_size) for j, rb in enumerate(pl.rbs)]
    assert kw == dict(dil=3, slope=0.1, out_div=3.0)
    # per-item lengths travel at the stage's output rate
    pl = _planner(g, lens='lens')
    assert pl.conv2_sum() is True
    assert calls.pop()[3] == dict(dil=3, slope=0.1, out_div=3.0, lengths='lens', len_mul=8 * g.ups[pl.stage_i].stride)
    # a forward that saves for backward, bf16 storage, the switch off, another precision, no stream from the fold: today's launches
    assert _planner(g, save={}).conv2_sum() is False
    assert _planner(g, st=True).conv2_sum() is False
    for attr, val in (('wino_sum', ()), ('precision', 'f16x3'), ('precision', 'bf16'), ('algo', hipops.ALGO_DIRECT)):
        old = getattr(g, attr)
        setattr(g, attr, val)
        assert _planner(g).conv2_sum() is False, (attr, val)
        setattr(g, attr, old)
    pl = _planner(g)
    g._fold_key['wpw_sum'] = {}
    assert pl.conv2_sum() is False and calls == []
    # declined by the library: the caller falls back
    monkeypatch.setattr(hipops, 'conv1d_wino_sum', lambda *a, **k: False)
    assert _planner(g).conv2_sum() is False
