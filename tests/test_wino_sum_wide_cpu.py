"""CPU tests of the summed Winograd launch on the wide stages (Generator.wino_sum = (64,) + Generator.wino_sum_wide = (256, 128)): which stages the planner tags
`bconv1:...`, that `()` / `()` leaves every stage on its two launches, which layers ask the fold for a stream of their own, the library's walk
order and the dispatch of the entry point with an order.  No GPU needed."""
import types

import pytest

from wavthruvec_pytorch_amd import _hip, hipops
from wavthruvec_pytorch_amd.forward_plan import ForwardPlanner

SHIPPED = (256, 128, 64)


def _generator():
    from wavthruvec_pytorch_amd import Generator, synthetic
    return Generator(synthetic.make_hparams(num_wv_feat=768))


def _planner(g, i, with_streams=True):
    """A planner standing at the second convs of stage i (as tests/test_wino_sum_cpu.py builds one for the 64-channel stage)."""
    nk = g.num_kernels
    pl = ForwardPlanner.__new__(ForwardPlanner)
    pl.g, pl.save, pl.st, pl.lens, pl.lmul, pl.stage_i, pl.algo, pl.nk, pl.C = g, None, False, None, 8, i, g.algo, nk, g.ups[i].out_channels
    pl.S = types.SimpleNamespace(tag=None)
    pl.rbs = [g.resblocks[i * nk + j] for j in range(nk)]
    pl.names = [f'resblocks.{i * nk + j}' for j in range(nk)]
    pl.t1s = [f't1_{j}' for j in range(nk)]
    pl.xs = 'xs'
    g._profile = None
    # what the fold leaves: `wino` gives the second convs of C >= 128 a stream under 'wpw', the 64-channel ones get theirs under 'wpw_sum'
    key = 'wpw' if pl.C >= 128 else 'wpw_sum'
    g._fold_key['wpw'], g._fold_key['wpw_sum'] = {}, {}
    if with_streams:
        g._fold_key[key] = {f'{nm}.convs.1': f'wpw_{i}_{j}' for j, nm in enumerate(pl.names)}
    return pl


def _tags(g, monkeypatch):
    calls = []
    monkeypatch.setattr(hipops, 'conv1d_wino_sum', lambda sources, out, **kw: calls.append((pl.S.tag, sources, kw)) or True)
    done = {}
    for i, up in enumerate(g.ups):
        pl = _planner(g, i)
        done[up.out_channels] = pl.conv2_sum()
    return done, calls


def test_the_shipped_default():
    """`wino_sum` keeps the stages the fold gives streams of their own (the 64-channel one); `wino_sum_wide` adds the stages that reuse the
    streams `Generator.wino` folds.  Both travel in the plan key."""
    import inspect
    g = _generator()
    assert g.wino_sum == (64,) and g.wino_sum_wide == (256, 128) and tuple(g.wino_sum_wide) + tuple(g.wino_sum) == SHIPPED
    assert 'self.wino_sum_wide' in inspect.getsource(type(g)._plan_key)


def test_plan_tags_are_bconv1_for_exactly_the_listed_stages(monkeypatch):
    g = _generator()
    done, calls = _tags(g, monkeypatch)
    assert done == {C: C in SHIPPED for C in done} and sorted(C for C in done if done[C]) == sorted(SHIPPED)
    nk = g.num_kernels
    want = ['bconv1:' + '+'.join(f'resblocks.{i * nk + j}.1' for j in range(nk)) for i, up in enumerate(g.ups) if up.out_channels in SHIPPED]
    assert [c[0] for c in calls] == want
    for i, (tag, sources, kw) in enumerate(calls):        # the wide stages read the streams `wino` already folds, no order forced
        assert [s[1] for s in sources] == [f'wpw_{i}_{j}' for j in range(nk)] and 'order' not in kw


@pytest.mark.parametrize('ws,wide', [((), ()), ((64,), ()), ((64,), (128,)), ((64,), (256,)), ((), (256, 128)), ((256, 128, 64), ())])
def test_other_settings_leave_the_other_stages_on_their_two_launches(monkeypatch, ws, wide):
    g = _generator()
    g.wino_sum, g.wino_sum_wide = ws, wide
    done, calls = _tags(g, monkeypatch)
    assert sorted(C for C in done if done[C]) == sorted(ws + wide) and len(calls) == len(ws + wide)


def test_the_fold_is_asked_for_no_second_stream():
    """_wino_sum_layers names the second convs of the listed stages; _fold_weights gives such a layer a stream under 'wpw_sum' only where
    `wino` gave it none (`wpwb is None`), and both tables name their buffer 'wpw.<layer>': one buffer per layer, written once."""
    import inspect
    g = _generator()
    nk = g.num_kernels
    def layers(cs):
        return {f'resblocks.{i * nk + j}.convs.1' for i, up in enumerate(g.ups) if up.out_channels in cs for j in range(nk)}
    assert g._wino_sum_layers() == layers((64,))          # wino_sum_wide asks the fold for nothing
    g.wino_sum = SHIPPED                                  # listed here the wide stages are named, and the fold's own condition keeps it to one stream
    assert g._wino_sum_layers() == layers(SHIPPED)
    src = inspect.getsource(type(g)._fold_weights)
    assert 'if mfma_ok and wpwb is None and name in sum_names' in src
    g.wino_sum = ()
    assert g._wino_sum_layers() == set()


def test_without_a_stream_the_stage_keeps_its_two_launches(monkeypatch):
    monkeypatch.setattr(hipops, 'conv1d_wino_sum', lambda *a, **k: pytest.fail('launched without streams'))
    g = _generator()
    for i in range(len(g.ups)):
        assert _planner(g, i, with_streams=False).conv2_sum() is False


def test_library_walk_order_is_the_branch_order():
    """Measured on MI355X (profiles/r14_cfg2_wino_sum_wide_per_layer.txt): no walk order is faster than another beyond the launches' own
    spread, so the library keeps the branch order - and with it the bits of the 64-channel stage."""
    assert hipops.wino_sum_order((3, 7, 11)) == (0, 1, 2)
    assert hipops.wino_sum_order((3, 7)) == (0, 1)
    assert hipops.wino_sum_order((11,)) == (0,)


def _sources(n, C, L=132, ks=(3, 7, 11), B=2):
    arr = (_hip.Conv1dArgs * n)()
    for i in range(n):
        a = arr[i]
        a.in_, a.out, a.wp, a.bias = 0x100000 + 0x10000 * i, 0x200000, 0x300000 + 0x10000 * i, 0x400
        a.B, a.C_in, a.C_out, a.L, a.k, a.dil, a.slope, a.algo, a.pad_left, a.out_div = B, C, C, L, ks[i], 3, 0.1, hipops.ALGO_WINO, -1, 3.0
    return arr


@pytest.mark.parametrize('C,L,lens,order,want_rc,want', [
    (256, 132, False, (0, 1, 2), 0, 'conv_wino_sum_kernel<1, 2, 3, true>'),
    (128, 386, False, (1, 2, 0), 0, 'conv_wino_sum_kernel<1, 2, 3, false>'),
    (256, 200, True, (2, 1, 0), 0, 'conv_wino_sum_len_kernel<1, 2, 3, true>'),
    (128, 132, False, None, 0, 'conv_wino_sum_kernel<1, 2, 3, true>'),
    (128, 132, False, (0, 0, 1), -1, None),
    (128, 132, False, (0, 1, 3), -1, None),
    (128, 132, False, (-1, 1, 2), -1, None),
], ids=['C256', 'scalar_k3_last', 'len_reversed', 'library_order', 'repeated', 'out_of_range', 'negative'])
def test_dispatch_with_an_order(C, L, lens, order, want_rc, want):
    import ctypes
    od = (ctypes.c_int32 * 3)(*order) if order is not None else None
    rc, names = _hip.kernel_names(_hip.load().v2w_conv1d_wino_sum_fwd_order, _sources(3, C, L), 3, 0x500000 if lens else None, 2, od)
    print(rc, names)
    assert (rc in (0, 100) if want_rc == 0 else rc == want_rc) and names == ([want] if want else [])
