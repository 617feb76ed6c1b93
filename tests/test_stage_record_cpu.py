"""CPU tests of the stage record (forward_plan.Stage, Generator.stage_record): what the planner, the weight fold and the backward derive
from a residual stage's blocks, against literal tables; the layer-name sets the fold asks with; the per-branch dicts the hipops stage
wrappers read.  The name sets are the ones the commit before the record computed, written out.  No GPU needed.

The reference configuration's sets at the default switches and with each switch off are pinned elsewhere and not repeated here:
`_wino_stage_layers` in tests/test_stage_wino_cpu.py, `_wino_sum_layers` in tests/test_wino_sum_cpu.py and tests/test_wino_sum_wide_cpu.py,
`_wino_up_layers` in tests/test_wino_up_cpu.py."""
import types

import pytest

from wavthruvec_pytorch_amd import hipops
from wavthruvec_pytorch_amd.forward_plan import STAGE_WINO_BLOCKS, Stage

CONFIGS = {
    'reference': dict(num_wv_feat=768),
    'six_stage_x640': dict(num_wv_feat=768, upsample_rates=[5, 4, 4, 2, 2, 2], upsample_kernel_sizes=[11, 8, 8, 4, 4, 4]),
    'resblock1': dict(num_wv_feat=768, resblock='1'),
}
WIDTHS = {'reference': [256, 128, 64, 32, 16], 'six_stage_x640': [256, 128, 64, 32, 16, 8], 'resblock1': [256, 128, 64, 32, 16]}
STAGE32 = {f'resblocks.{j}.convs.{c}' for j in (9, 10, 11) for c in (0, 1)}
SUM64 = {f'resblocks.{j}.convs.1' for j in (6, 7, 8)}
UPS = {'ups.1', 'ups.2', 'ups.3'}
# (_wino_stage_layers, _wino_sum_layers, _wino_up_layers) at the default switches
LAYER_SETS = {'six_stage_x640': (STAGE32, SUM64, UPS), 'resblock1': (set(), set(), UPS)}


def _generator(name):
    from wavthruvec_pytorch_amd import Generator, synthetic
    return Generator(synthetic.make_hparams(**CONFIGS[name]))


@pytest.mark.parametrize('name', list(CONFIGS))
def test_every_stage_against_the_tables(name):
    g = _generator(name)
    assert g.num_upsamples == len(WIDTHS[name])
    for i, C in enumerate(WIDTHS[name]):
        stg = g.stage_record(i)
        assert isinstance(stg, Stage) and stg.i == i and stg.C == C
        assert stg.rbs == tuple(g.resblocks[3 * i + j] for j in range(3))
        assert stg.names == (f'resblocks.{3 * i}', f'resblocks.{3 * i + 1}', f'resblocks.{3 * i + 2}')
        assert stg.ks == [3, 7, 11] and stg.heavy_first == [2, 1, 0]
        if name == 'resblock1':
            assert not stg.is_rb2 and not stg.is_std
            for n, d in enumerate((1, 3, 5)):
                assert stg.dils(0, n) == [d, d, d] and stg.dils(1, n) == [1, 1, 1]
                assert stg.layer(1, 0, n) == f'resblocks.{3 * i + 1}.convs1.{n}' and stg.layer(2, 1, n) == f'resblocks.{3 * i + 2}.convs2.{n}'
            assert stg.layers(n=2) == {f'resblocks.{3 * i + j}.convs{c}.2' for j in range(3) for c in (1, 2)}
            continue
        assert stg.is_rb2 and stg.is_std
        assert stg.dil1s == [1, 1, 1] and stg.dil2s == [3, 3, 3]
        assert stg.blocks == [(3, 1, 3), (7, 1, 3), (11, 1, 3)] == STAGE_WINO_BLOCKS
        assert stg.pairs(0) == [(3, 1), (7, 1), (11, 1)] and stg.pairs(1) == [(3, 3), (7, 3), (11, 3)]
        assert stg.layer(0, 1) == f'resblocks.{3 * i}.convs.1'
        assert stg.layers() == {f'resblocks.{3 * i + j}.convs.{c}' for j in range(3) for c in (0, 1)}
        assert stg.layers((1,)) == {f'resblocks.{3 * i + j}.convs.1' for j in range(3)}


def test_heavy_first_keeps_the_branch_order_among_equal_kernel_sizes_and_is_std_reads_the_dilations():
    def rb(k, d):
        return types.SimpleNamespace(kernel_size=k, convs=[types.SimpleNamespace(dilation=d[0]), types.SimpleNamespace(dilation=d[1])])
    stg = Stage(0, 32, (rb(7, (1, 3)), rb(3, (1, 3)), rb(7, (1, 3)), rb(11, (1, 3))), ('a', 'b', 'c', 'd'))
    assert stg.heavy_first == [3, 0, 2, 1]
    assert stg.blocks == [(7, 1, 3), (3, 1, 3), (7, 1, 3), (11, 1, 3)]
    assert Stage(0, 32, (rb(3, (1, 3)), rb(7, (1, 3)), rb(11, (1, 5))), ('a', 'b', 'c')).blocks != STAGE_WINO_BLOCKS


@pytest.mark.parametrize('name', list(LAYER_SETS))
def test_layer_sets_at_the_default_switches_and_with_each_switch_off(name):
    g = _generator(name)
    stage, summed, ups = LAYER_SETS[name]
    assert (g._wino_stage_layers(), g._wino_sum_layers(), g._wino_up_layers()) == (stage, summed, ups)
    g.wino_stage = False
    assert (g._wino_stage_layers(), g._wino_sum_layers(), g._wino_up_layers()) == (set(), summed, ups)
    g.wino_stage, g.wino_sum = True, ()
    assert (g._wino_stage_layers(), g._wino_sum_layers(), g._wino_up_layers()) == (stage, set(), ups)
    g.wino_sum, g.wino_up = (64,), ()
    assert (g._wino_stage_layers(), g._wino_sum_layers(), g._wino_up_layers()) == (stage, summed, set())
    g.wino_up = (1, 2, 3)
    for attr, val in (('precision', 'bf16'), ('precision', 'f16x3'), ('algo', hipops.ALGO_DIRECT)):
        old = getattr(g, attr)
        setattr(g, attr, val)
        assert (g._wino_stage_layers(), g._wino_sum_layers(), g._wino_up_layers()) == (set(), set(), set()), (attr, val)
        setattr(g, attr, old)


@pytest.mark.parametrize('key1,key2', [('wp1', 'wp2'), ('wpw1', 'wpw2'), ('wf1', 'wf2'), ('wps1', 'wps2')])
def test_branches_of_a_resblock2_stage(key1, key2):
    g = _generator('reference')
    stg = g.stage_record(3)
    w = {nm: 'w:' + nm for nm in stg.layers()}
    brs = stg.branches(w, key1, key2)
    assert len(brs) == 3
    for j, (br, rb) in enumerate(zip(brs, stg.rbs)):
        assert set(br) == {key1, 'b1', key2, 'b2', 'k', 'dil1', 'dil2'}
        assert br[key1] == f'w:resblocks.{9 + j}.convs.0' and br[key2] == f'w:resblocks.{9 + j}.convs.1'
        assert br['b1'].data_ptr() == rb.convs[0].bias.data_ptr() and br['b2'].data_ptr() == rb.convs[1].bias.data_ptr()
        assert not br['b1'].requires_grad and not br['b2'].requires_grad
        assert (br['k'], br['dil1'], br['dil2']) == ((3, 7, 11)[j], 1, 3)


@pytest.mark.parametrize('n', [0, 1, 2])
def test_branches_of_a_resblock1_pair(n):
    g = _generator('resblock1')
    stg = g.stage_record(4)
    w = {nm: 'w:' + nm for nm in stg.layers(n=n)}
    for key1, key2 in (('wps1', 'wps2'), ('wp1', 'wp2')):
        for j, (br, rb) in enumerate(zip(stg.branches(w, key1, key2, n), stg.rbs)):
            assert set(br) == {key1, 'b1', key2, 'b2', 'k', 'dil1', 'dil2'}
            assert br[key1] == f'w:resblocks.{12 + j}.convs1.{n}' and br[key2] == f'w:resblocks.{12 + j}.convs2.{n}'
            assert br['b1'].data_ptr() == rb.convs1[n].bias.data_ptr() and br['b2'].data_ptr() == rb.convs2[n].bias.data_ptr()
            assert (br['k'], br['dil1'], br['dil2']) == ((3, 7, 11)[j], (1, 3, 5)[n], 1)
