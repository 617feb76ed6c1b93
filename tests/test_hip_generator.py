"""End-to-end GPU parity of `Generator.forward` (HIP, through the C ABI):
 - against every fixture captured from the reference (tests/golden/*.npz), |dy| <= 1e-4 (north_star tolerance);
 - against the oracle on larger seeded inputs the oracle finishes in seconds;
 - at BASELINE.json's full cfg2 size through size-independent properties (determinism, eval-mode batch
   independence, bounded output, shard/whole agreement of the statistics exchange)."""
import numpy as np
import pytest
import torch

from oracle import vec2wav_oracle as O
from tests.golden_util import golden_names, load_golden, case_setup, probe_summary, tol_for
from wavthruvec_pytorch_amd import synthetic

pytestmark = pytest.mark.gpu
TOL = 1e-4   # |dy| bar of BASELINE.json north_star (fp32)


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a MI355X'
    return torch.device('cuda:0')


def build_generator(h, sd, dev, training=True):
    from wavthruvec_pytorch_amd import Generator
    g = Generator(h)
    g.load_state_dict(sd)
    g = g.to(dev)
    g.train(training)
    return g


def to_dev(ts, dev):
    return tuple(t.to(dev) for t in ts)


@pytest.mark.parametrize('algo', ['auto', 'direct', 'f16x3'])
@pytest.mark.parametrize('name', golden_names())
def test_generator_matches_reference_golden(dev, name, algo):
    """algo 'f16x3': the split-f16 precision mode (wide Conv1d layers on the f16 matrix pipe) is held to the SAME 1e-4 bar
    against the same reference goldens as the exact-fp32 path."""
    from wavthruvec_pytorch_amd import hipops
    if algo == 'direct' and name not in ('rb2_train_b2_t8', 'rb1_train_b2_t8', 'rb2_1024_x640_train_b2_t8', 'rb2_6stage_x640_train_b2_t8'):
        pytest.skip('direct (scalar) kernels are cross-checked on four representative cases')
    z, meta = load_golden(name)
    h, sd, inp, inp2 = case_setup(meta)
    mode = meta['mode']
    g = build_generator(h, sd, dev, training=True)
    g.algo = hipops.ALGO_DIRECT if algo == 'direct' else hipops.ALGO_AUTO
    if algo == 'f16x3':
        g.precision = 'f16x3'
    with torch.no_grad():
        if mode == 'evalcal':
            for c in g.cbns:
                c.batch_nrom.momentum = 1.0
            g(*to_dev(inp, dev))
            g.eval()
            y = g(*to_dev(inp, dev))
        elif mode == 'eval':
            g.eval()
            y = g(*to_dev(inp, dev))
        elif mode == 'train2':
            y1 = g(*to_dev(inp, dev))
            assert np.abs(y1.cpu().numpy() - z['y_step1']).max() <= TOL
            y = g(*to_dev(inp2, dev))
        elif mode == 'train_rmwn':
            g.remove_weight_norm()
            assert list(g.state_dict().keys()) == [str(k) for k in z['keys_after_rmwn']]
            y = g(*to_dev(inp, dev))
        else:
            y = g(*to_dev(inp, dev))
    tol = tol_for(meta)
    got = y.cpu().numpy()
    assert got.shape == z['y'].shape
    d = np.abs(got - z['y']).max()
    assert np.isfinite(got).all()
    assert d <= tol, f'{name}: max|dy| = {d}'
    # layer probes the HIP path materialises: conv_pre and every upsampler output
    ptol = 1e-3 if mode != 'eval' else 5e-2
    probes = {'conv_pre': g._ws['act.pre']}
    for i in range(g.num_upsamples):
        probes[f'ups.{i}'] = g._ws[f'act.up{i}']
    for pname, t in probes.items():
        s = probe_summary(t)
        scale = max(1.0, float(np.abs(z[f'probe/{pname}/head']).max()))
        assert np.abs(s['head'] - z[f'probe/{pname}/head']).max() <= ptol * scale, pname
        assert np.abs(s['tail'] - z[f'probe/{pname}/tail']).max() <= ptol * scale, pname
        ref_abs = float(z[f'probe/{pname}/abssum'])
        assert abs(s['abssum'] - ref_abs) <= 1e-4 * ref_abs + 1e-3, pname
    # post-forward buffers: running stats, num_batches_tracked, spectral-norm u / v
    post = g.state_dict()
    for k in z.files:
        if k.startswith('buf/'):
            ref = z[k]
            gotb = post[k[4:]].cpu().numpy()
            if ref.dtype.kind == 'i':
                assert (gotb == ref).all(), k
            else:
                assert np.abs(gotb - ref).max() <= 2e-5 * max(1.0, np.abs(ref).max()), k


def test_generator_split_precision_tracks_f32_path(dev):
    """precision='f16x3' at a size where the wide layers dominate: the output stays within 2e-6 of the exact-fp32 HIP path
    (the parity bar vs the reference is 1e-4), the split kernel really ran, and train-mode buffers agree."""
    h = synthetic.make_hparams(num_wv_feat=768)
    sd = synthetic.make_state_dict(h, seed=5)
    inp = to_dev(synthetic.make_inputs(h, 4, 64, seed=9), dev)
    g32 = build_generator(h, sd, dev, training=True)
    gsp = build_generator(h, sd, dev, training=True)
    gsp.precision = 'f16x3'
    gsp._profile = []
    with torch.no_grad():
        y32 = g32(*inp)
        ysp = gsp(*inp)
    assert len(gsp._fold_key['wps'][1]) == 31          # conv_pre + the 18 residual convs of stages 0-2 (C_out >= 64) + 6 + 6 of the fused C = 32 / 16 stages
    d = (y32 - ysp).abs().max().item()
    assert d <= 2e-6, f'split vs f32 path: max|dy| = {d}'
    for k, v in g32.state_dict().items():
        w = gsp.state_dict()[k]
        if v.dtype.is_floating_point:
            assert (v - w).abs().max().item() <= 1e-5 * max(1.0, v.abs().max().item()), k
    gsp.precision = 'fp8'
    with pytest.raises(ValueError):
        with torch.no_grad():
            gsp(*inp)


def test_generator_bf16_operand_mode(dev):
    """precision='bf16' (BASELINE configs[2]: bf16 compute / fp32 accumulate on the wide Conv1d layers).  SURVEY.md 8(c) measured
    4e-3 for full bf16 autocast of the reference against fp64; this mode rounds only conv operands of 19 layers: bar 4e-3."""
    h = synthetic.make_hparams(num_wv_feat=768)
    sd = synthetic.make_state_dict(h, seed=5)
    inp_cpu = synthetic.make_inputs(h, 4, 64, seed=9)
    want, _ = O.generator_forward({k: v.clone() for k, v in sd.items()}, h, *inp_cpu, training=True)
    g = build_generator(h, sd, dev, training=True)
    g.precision = 'bf16'
    with torch.no_grad():
        y = g(*to_dev(inp_cpu, dev))
    d = (y.cpu() - want).abs().max().item()
    assert np.isfinite(y.cpu().numpy()).all()
    assert 1e-6 < d <= 4e-3, f'max|dy| = {d}'


@pytest.mark.parametrize('B,T', [(2, 33), (1, 7), (3, 50)])
def test_generator_bf16_storage_ragged_lengths(dev, B, T):
    """precision='bf16' with bf16 activation storage at lengths that are not multiples of 4 (and a 5-frame input): every bf16 kernel's
    element-wise staging / epilogue fallback (unaligned rows) against the fp32 oracle, at the small-size bf16 bar."""
    h = synthetic.make_hparams(num_wv_feat=768)
    sd = synthetic.make_state_dict(h, seed=5)
    inp_cpu = synthetic.make_inputs(h, B, T, seed=9)
    want, _ = O.generator_forward({k: v.clone() for k, v in sd.items()}, h, *inp_cpu, training=True)
    g = build_generator(h, sd, dev, training=True)
    g.precision = 'bf16'
    assert g.bf16_storage
    with torch.no_grad():
        y = g(*to_dev(inp_cpu, dev))
    assert y.shape == want.shape and torch.isfinite(y).all()
    d = (y.cpu() - want).abs().max().item()
    assert 1e-6 < d <= 4e-3, f'max|dy| = {d}'


@pytest.mark.parametrize('B,T,feat,rates,ks', [(2, 64, 1024, [8, 5, 4, 2, 2], [16, 11, 8, 4, 4]), (3, 18, 1024, [8, 5, 4, 2, 2], [16, 11, 8, 4, 4]),
                                               (2, 128, 768, [5, 4, 4, 2, 2], [11, 8, 8, 4, 4])])
@pytest.mark.parametrize('training', [True, False])
def test_generator_bf16_storage_other_rates_and_fusion_switches(dev, B, T, feat, rates, ks, training):
    """bf16 activation storage on the x640 generator of BASELINE configs[4] (stride 8 first, the stride-5 upsampler in SECOND place: the
    stage-0 kernel cannot carry it - `fuse_up` declines that stage and the exact-phase / chunked stride-5 kernels run standalone) and on
    the default generator at a length that puts whole 64-position tiles on ups.0: train and eval mode against the fp32 oracle at the
    small-size bf16 bar, and the fused schedule (next upsampler and tail inside the stage kernels) against the unfused one - the same bf16
    operands in both, so they differ by accumulation order and the rounding of the tensors the fusion no longer stores.  Bar: the
    small-size bf16 bar (4e-3) or the reference's own bf16-autocast deviation on the same inputs, whichever is larger."""
    h = synthetic.make_hparams(num_wv_feat=feat, upsample_rates=rates, upsample_kernel_sizes=ks)
    sd = synthetic.make_state_dict(h, seed=7)
    inp_cpu = synthetic.make_inputs(h, B, T, seed=3)
    if not training:
        O.calibrate_running_stats(sd, h, *inp_cpu)      # (a fresh-init eval forward is ill-conditioned, SURVEY 8(c): running statistics := these inputs')
    want, _ = O.generator_forward({k: v.clone() for k, v in sd.items()}, h, *inp_cpu, training=training)
    with torch.autocast('cpu', dtype=torch.bfloat16):       # the reference's own bf16 arithmetic on these inputs, in this mode
        yb, _ = O.generator_forward({k: v.clone() for k, v in sd.items()}, h, *inp_cpu, training=training)
    bar = max(4e-3, (yb.float() - want).abs().max().item())
    outs = []
    for fused in (True, False):
        g = build_generator(h, sd, dev, training=training)
        g.precision = 'bf16'
        g.fuse_up = g.fuse_post = fused
        assert g.bf16_storage
        with torch.no_grad():
            y = g(*to_dev(inp_cpu, dev))
        assert y.shape == want.shape and torch.isfinite(y).all()
        d = (y.cpu() - want).abs().max().item()
        assert 1e-6 < d <= bar, f'fused={fused}: max|dy| = {d} (bar {bar})'
        outs.append(y)
    assert (outs[0] - outs[1]).abs().max().item() <= bar


@pytest.mark.parametrize('B,T,rates,ks', [(3, 64, [5, 4, 4, 2, 2], [11, 8, 8, 4, 4]), (2, 40, [5, 4, 4, 2, 2], [11, 8, 8, 4, 4]),
                                          (2, 20, [8, 5, 4, 2, 2], [16, 11, 8, 4, 4])])
@pytest.mark.parametrize('training', [True, False])
def test_generator_resblock1_bf16_storage(dev, B, T, rates, ks, training):
    """h.resblock == '1' with precision='bf16': bf16 tensors between ALL layers - every (dilated conv, conv) pair of
    models.py:37-44 as one resident-tile launch per pair position (v2w_stage_split_args::rb1), the branch mean in the last one - against
    the fp32 oracle at the small-size bf16 bar, train and calibrated-eval mode."""
    nf = 768 if rates[0] == 5 else 1024
    h = synthetic.make_hparams(num_wv_feat=nf, resblock='1', upsample_rates=rates, upsample_kernel_sizes=ks)
    sd = synthetic.make_state_dict(h, seed=5)
    inp_cpu = synthetic.make_inputs(h, B, T, seed=9)
    if not training:
        O.calibrate_running_stats(sd, h, *inp_cpu)
    want, _ = O.generator_forward({k: v.clone() for k, v in sd.items()}, h, *inp_cpu, training=training)
    g = build_generator(h, sd, dev, training=training)
    g.precision = 'bf16'
    with torch.no_grad():
        y = g(*to_dev(inp_cpu, dev))
    assert g._ws['act.xa_0_0'].dtype == torch.bfloat16 and g._ws['act.rb4'].dtype == torch.bfloat16, 'the activations are not stored as bf16'
    assert y.shape == want.shape and torch.isfinite(y).all()
    d = (y.cpu() - want).abs().max().item()
    assert 1e-6 < d <= 6e-3, f'max|dy| = {d}'
    # ... and no farther from the oracle than fp32 storage with the same bf16 operands is, by more than the storage rounding allows
    g2 = build_generator(h, sd, dev, training=training)
    g2.precision = 'bf16'; g2.bf16_storage = False
    with torch.no_grad():
        y2 = g2(*to_dev(inp_cpu, dev))
    assert (y2.cpu() - want).abs().max().item() <= 6e-3


@pytest.mark.parametrize('training,precision', [(True, 'f32'), (False, 'f32'), (True, 'bf16'), (False, 'bf16'), (False, 'f16x3')])
def test_generator_launch_plan_replays_the_planned_forward(dev, training, precision):
    """schedule.py: the first no-grad forward of a configuration is planned under a recorder, later ones replay the tape with the three input
    pointers and the output rebound.  Replays must equal forwards that are planned every time (`use_launch_plan = False`) bit for bit - on
    NEW inputs, across a parameter update in eval mode (the replayed plan must fold the new weights once and then stop folding), across a
    shape change (buffers are reallocated: the old plans are dropped) and back."""
    h = synthetic.make_hparams(num_wv_feat=768)
    sd = synthetic.make_state_dict(h, seed=5)
    if not training:
        O.calibrate_running_stats(sd, h, *synthetic.make_inputs(h, 2, 16, seed=1))
    ga, gb = build_generator(h, sd, dev, training=training), build_generator(h, sd, dev, training=training)
    ga.precision = gb.precision = precision
    gb.use_launch_plan = False
    inputs = [to_dev(synthetic.make_inputs(h, 2, 16, seed=s), dev) for s in (1, 2, 3)]
    other = to_dev(synthetic.make_inputs(h, 1, 24, seed=4), dev)
    with torch.no_grad():
        for step, inp in enumerate(inputs + [other] + inputs):
            ya, yb = ga(*inp), gb(*inp)
            assert torch.equal(ya, yb), (step, (ya - yb).abs().max().item())
            if step == 1:
                assert len(ga._tapes) >= 1 and not gb._tapes
                assert ga._tape_refused == 0          # every recorded pointer lies in memory the module owns (schedule.TapeNotOwned otherwise)
                n_launch = max(t.launches for t in ga._tapes.values())
                assert 0 < n_launch <= 80
            if step == 2:          # an optimizer step's worth of change, in place (version counters move)
                for g in (ga, gb):
                    g.conv_pre.weight_g.mul_(1.01)
                    g.resblocks[3].convs[0].weight_v.add_(0.001)
        for bname in ('running_mean', 'running_var', 'num_batches_tracked'):
            for ca, cb in zip(ga.cbns, gb.cbns):
                assert torch.equal(getattr(ca.batch_nrom, bname), getattr(cb.batch_nrom, bname))
        if not training:           # eval: a parameter update is followed by ONE forward that folds (its own plan), then the plan without folds again
            for g in (ga, gb):
                g.conv_post.weight_g.mul_(0.99)
            for _ in range(2):
                assert torch.equal(ga(*inputs[0]), gb(*inputs[0]))
            keys = [k for k in ga._tapes if k[0] == tuple(inputs[0][0].shape)]
            # 'ws': the first forward (weights and sigma stale), 'w': the forwards behind the conv updates, 'folded': everything cached
            assert {k[-1] for k in keys} >= {'folded', 'w'}, [k[-1] for k in keys]
            folded = [ga._tapes[k] for k in keys if k[-1] == 'folded'][0]
            refold = [ga._tapes[k] for k in keys if k[-1] == 'w'][0]
            assert folded.launches < refold.launches


@pytest.mark.parametrize('precision', ['bf16', 'f32'])
def test_plan_switches_change_the_schedule_not_the_result(dev, precision):
    """Round-6 switches of the launch plan - the statistics reduction + finalisation as one launch (fuse_bn_finalize), the conditioning chain on a
    second side stream (cond_stream), merged waits for side-stream events (merge_waits) - re-order launches and stream waits only: the output, the
    BatchNorm running statistics and the spectral-norm vectors of a train-mode forward are bit-identical in every setting, planned and replayed
    (B x T = 4 096 frames: where `cond_stream = None` turns the second stream on by itself)."""
    import itertools
    h = synthetic.make_hparams(num_wv_feat=768)
    sd = synthetic.make_state_dict(h, seed=0)
    inp = to_dev(synthetic.make_inputs(h, 16, 256, seed=9), dev)
    ref = None
    for bn, cs, mw in itertools.chain([(True, None, True)], itertools.product((False, True), (False, True), (False, True))):
        g = build_generator(h, sd, dev, training=True)
        g.precision = precision
        g.fuse_bn_finalize, g.cond_stream, g.merge_waits = bn, cs, mw
        with torch.no_grad():
            y1 = g(*inp)              # planned and recorded
            y2 = g(*inp)              # replayed
        torch.cuda.synchronize()
        state = {k: v.clone() for k, v in g.state_dict().items() if 'cbns' in k}
        assert torch.isfinite(y1).all()
        if ref is None:
            ref = (y1.clone(), y2.clone(), state)
            continue
        assert torch.equal(y1, ref[0]) and torch.equal(y2, ref[1]), (bn, cs, mw)
        for k, v in state.items():
            assert torch.equal(v, ref[2][k]), (k, bn, cs, mw)


def test_launch_plan_key_separates_weight_folds_from_sigma(dev):
    """what is stale when a plan is recorded is part of its key, separately for the conv weight folds ('w') and for sigma of the
    spectral norm ('s').  A train-mode no-grad forward leaves the folds cached and sigma_ws holding its own values: the next eval forward
    records a plan with cond_sigma and NO weight fold - that plan must not serve the eval forward behind an in-place conv update (it would
    run on the old folded weights, silently), nor may a weights-only plan serve a forward whose sigma is stale."""
    h = synthetic.make_hparams(num_wv_feat=768)
    sd = synthetic.make_state_dict(h, seed=5)
    O.calibrate_running_stats(sd, h, *synthetic.make_inputs(h, 2, 16, seed=1))
    ga, gb = build_generator(h, sd, dev, training=False), build_generator(h, sd, dev, training=False)
    for g in (ga, gb):
        g.always_refold = False
    gb.use_launch_plan = False
    inp = to_dev(synthetic.make_inputs(h, 2, 16, seed=2), dev)

    def both(check=True):
        ya, yb = ga(*inp), gb(*inp)
        if check:
            assert torch.equal(ya, yb), (ya - yb).abs().max().item()

    with torch.no_grad():
        both()                                                   # eval, everything stale: 'ws'
        for g in (ga, gb):
            g.train()
        both(); both()                                           # train mode: sigma_ws takes the power iteration's values, the folds stay cached
        for g in (ga, gb):
            g.eval()
        both()                                                   # eval, only sigma stale: recorded under 's' (no weight fold on this tape)
        tags = {k[-1] for k in ga._tapes if k[3] is False}
        assert 's' in tags, tags
        for g in (ga, gb):
            g.conv_pre.weight_g.mul_(1.25)
            g.resblocks[7].convs[1].weight_v.add_(0.01)
        both()                                                   # eval, only the weights stale: must fold - 'w', not the 's' tape
        both()
        for g in (ga, gb):
            g.train()
        both()
        for g in (ga, gb):
            g.eval()
            g.ups[1].weight_g.mul_(0.9)
            g.cbns[2].layer.weight_orig.mul_(1.05)
        both()                                                   # both stale again
        both()
        tags = {k[-1] for k in ga._tapes if k[3] is False}
        assert tags >= {'ws', 'w', 's', 'folded'}, tags


def test_backward_is_refused_after_a_refold_from_changed_weights(dev):
    """backward.py: the folded weights a backward reads live in module-owned buffers.  A later forward that folds CHANGED parameters into them
    (here: a replayed launch plan after an in-place update) must make the pending backward fail loudly; a later forward of unchanged
    parameters must not."""
    h = synthetic.make_hparams(num_wv_feat=768)
    g = build_generator(h, synthetic.make_state_dict(h, seed=5), dev, training=True)
    inp = to_dev(synthetic.make_inputs(h, 2, 8, seed=1), dev)
    y = g(*inp)
    with torch.no_grad():
        g(*inp); g(*inp)                       # planned, then replayed: same parameter values, the buffers hold the same folds
    y.sum().backward()
    y = g(*inp)
    with torch.no_grad():
        g.conv_pre.weight_g.mul_(1.5)
        g(*inp)                                # replays the plan: folds the CHANGED weights into the buffers the pending backward reads
    with pytest.raises(RuntimeError, match='re-folded'):
        y.sum().backward()


def test_generator_bf16_storage_falls_back_when_a_layer_has_no_bf16_kernel(dev):
    """precision='bf16' with the default bf16 activation storage on a configuration the bf16-tensor kernels do not cover (a residual
    kernel of 13 taps: the fused narrow-stage kernel stops at 11): the forward must run - with fp32 tensors between the layers -
    instead of raising in the middle, and stay at the bf16-operand bar against the fp32 oracle."""
    h = synthetic.make_hparams(num_wv_feat=768, resblock_kernel_sizes=[3, 7, 13])
    sd = synthetic.make_state_dict(h, seed=5)
    inp_cpu = synthetic.make_inputs(h, 2, 16, seed=9)
    want, _ = O.generator_forward({k: v.clone() for k, v in sd.items()}, h, *inp_cpu, training=True)
    g = build_generator(h, sd, dev, training=True)
    g.precision = 'bf16'
    assert g.bf16_storage and not g._bf16_storage_kernels_exist(2, 16)
    with torch.no_grad():
        y = g(*to_dev(inp_cpu, dev))
    d = (y.cpu() - want).abs().max().item()
    assert torch.isfinite(y).all() and 1e-6 < d <= 4e-3, f'max|dy| = {d}'


def test_generator_cfg3_bf16_full_size(dev):
    """BASELINE configs[2] at its full size (B=64, T=512, bf16 compute / fp32 accumulate, bf16 activation storage) against the
    exact-fp32 HIP path on the same inputs, without the oracle (test_generator_cfg3_full_size_vs_oracle_train holds the real bar:
    the reference's own bf16 autocast deviation, 7e-3 max / 7.5e-4 rms at this size): finite, max <= 1e-2 and rms <= 7.5e-4;
    and the HIP-graph replay of the f16x3 mode is bit-identical to its eager run."""
    h = synthetic.make_hparams(num_wv_feat=768)
    sd = synthetic.make_state_dict(h, seed=0)
    g = build_generator(h, sd, dev, training=True)
    inp = to_dev(synthetic.make_inputs(h, 64, 512, seed=4), dev)
    with torch.no_grad():
        y32 = g(*inp)
        g.precision = 'bf16'
        yb = g(*inp)
    assert yb.shape == (64, 1, 512 * 320) and torch.isfinite(yb).all()
    d = (y32 - yb).abs().max().item()
    rms = (y32 - yb).pow(2).mean().sqrt().item()
    assert 1e-6 < d <= 1e-2 and rms <= 7.5e-4, f'max|y_bf16 - y_f32| = {d}, rms {rms}'
    del y32, yb
    ge = build_generator(h, sd, dev, training=False)
    ge.precision = 'f16x3'
    small = to_dev(synthetic.make_inputs(h, 1, 50, seed=3), dev)
    with torch.no_grad():
        y0 = ge(*small).clone()
    run = ge.capture_graph(*small)
    assert torch.equal(run(*small), y0)


@pytest.mark.parametrize('resblock,B,T,nf,rates,ks', [
    (1, 4, 64, 768, [5, 4, 4, 2, 2], [11, 8, 8, 4, 4]),
    ('1', 2, 40, 768, [5, 4, 4, 2, 2], [11, 8, 8, 4, 4]),
    (1, 2, 33, 1024, [8, 5, 4, 2, 2], [16, 11, 8, 4, 4]),
    (1, 3, 19, 768, [5, 4, 4, 2, 2, 2], [11, 8, 8, 4, 4, 4]),          # six stages, x640: the last residual stage has 8 channels
    ('1', 2, 11, 768, [5, 4, 4, 2, 2, 2], [11, 8, 8, 4, 4, 4]),
])
@pytest.mark.parametrize('training', [True, False])
def test_generator_matches_oracle_medium(dev, resblock, B, T, nf, rates, ks, training):
    """Seeded inputs at sizes the oracle finishes in seconds; eval mode uses calibrated running stats."""
    torch.set_num_threads(max(1, torch.get_num_threads()))
    h = synthetic.make_hparams(num_wv_feat=nf, resblock=resblock, upsample_rates=rates, upsample_kernel_sizes=ks)
    sd = synthetic.make_state_dict(h, seed=3)
    inp = synthetic.make_inputs(h, B, T, seed=77)
    if not training:
        O.calibrate_running_stats(sd, h, *inp)
    want, nb = O.generator_forward(sd, h, *inp, training=training)
    g = build_generator(h, sd, dev, training=training)
    with torch.no_grad():
        y = g(*to_dev(inp, dev))
    d = (y.cpu() - want).abs().max().item()
    assert d <= TOL, f'max|dy| = {d}'
    O.apply_buffers(sd, nb)
    post = g.state_dict()
    for k in nb:
        a, b = post[k].cpu(), sd[k]
        if a.dtype == torch.long:
            assert a.item() == b.item(), k
        else:
            assert (a - b).abs().max().item() <= 2e-5 * max(1.0, b.abs().max().item()), k


def test_generator_cfg2_full_size_properties(dev):
    """BASELINE.json configs[1]: B=32, T=256, 768-d, x320.  Too big for the oracle in test time, so check
    properties that do not depend on size: finite and bounded output, bitwise run-to-run determinism,
    eval-mode batch independence (a sample alone == the same sample inside the batch), and agreement of a
    4-sample slice with the oracle in calibrated eval mode."""
    h = synthetic.make_hparams(num_wv_feat=768)
    sd = synthetic.make_state_dict(h, seed=0)
    B, T = 32, 256
    inp = synthetic.make_inputs(h, B, T, seed=1234)
    g = build_generator(h, sd, dev, training=True)
    with torch.no_grad():
        for c in g.cbns:
            c.batch_nrom.momentum = 1.0          # calibrate: running stats := batch stats
        xin = to_dev(inp, dev)
        y_train = g(*xin)
        assert y_train.shape == (B, 1, T * 320)
        assert torch.isfinite(y_train).all() and y_train.abs().max().item() <= 1.0
        sd_cal = {k: v.clone() for k, v in g.state_dict().items()}
        g.eval()
        y1 = g(*xin)
        y2 = g(*xin)
        assert torch.equal(y1, y2), 'eval forward is not run-to-run deterministic'
        # calibrated eval == train output up to the unbiased/biased variance ratio (n = 32*L per channel)
        assert (y1 - y_train).abs().max().item() < 1e-3
        # batch independence in eval mode
        sl = slice(5, 9)
        ys = g(*(t[sl].contiguous() for t in xin))
        assert (ys - y1[sl]).abs().max().item() <= 1e-6
    # oracle on the 4-sample slice with the calibrated buffers
    sd_cpu = {k: v.cpu() for k, v in sd_cal.items()}
    want, _ = O.generator_forward(sd_cpu, h, *(t[sl] for t in inp), training=False)
    d = (ys.cpu() - want).abs().max().item()
    assert d <= TOL, f'max|dy| = {d}'


def test_generator_train_determinism_and_state_evolution(dev):
    """Two generators fed the same three train steps end in bit-identical outputs and buffers."""
    h = synthetic.make_hparams(num_wv_feat=768)
    sd = synthetic.make_state_dict(h, seed=1)
    outs = []
    for rep in range(2):
        g = build_generator(h, sd, dev, training=True)
        with torch.no_grad():
            for step in range(3):
                y = g(*to_dev(synthetic.make_inputs(h, 3, 9, seed=100 + step), dev))
        outs.append((y.clone(), {k: v.clone() for k, v in g.state_dict().items()}))
    assert torch.equal(outs[0][0], outs[1][0])
    for k in outs[0][1]:
        assert torch.equal(outs[0][1][k], outs[1][1][k]), k
    assert outs[0][1]['cbns.0.batch_nrom.num_batches_tracked'].item() == 3


def test_generator_surface_errors(dev):
    from wavthruvec_pytorch_amd import Generator
    h = synthetic.make_hparams(num_wv_feat=768)
    g = Generator(h).to(dev)
    x, spk, nz = to_dev(synthetic.make_inputs(h, 1, 4), dev)
    with pytest.raises(TypeError):
        g(x)                                   # reference: torch.cat((None, None)) -> TypeError
    with pytest.raises(RuntimeError):
        g(x.cpu(), spk.cpu(), nz.cpu())        # no CPU fallback
    with pytest.raises(RuntimeError):
        g(x[:, :100].contiguous(), spk, nz)    # wrong feature width
    assert g(x.clone().requires_grad_(True), spk, nz).requires_grad   # the latent is an autograd citizen (test_generator_input_gradient...)
    g1 = Generator(synthetic.make_hparams(num_wv_feat=768, resblock='1')).to(dev)
    assert g1(x, spk, nz).requires_grad        # ResBlock1 generators are differentiable too
    with torch.no_grad():
        assert g1(x, spk, nz).shape == (1, 1, 4 * 320)


def _dp_worker(rank, world, port, B, T, out_dir):
    import os
    import torch.distributed as dist
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    from wavthruvec_pytorch_amd.distributed import shard_batch
    dev = torch.device('cuda:0')
    h = synthetic.make_hparams(num_wv_feat=768)
    sd = synthetic.make_state_dict(h, seed=0)
    g = build_generator(h, sd, dev, training=True).enable_sync_batchnorm()
    mine = shard_batch(synthetic.make_inputs(h, B, T, seed=1234), rank, world)
    with torch.no_grad():
        y = g(*to_dev(mine, dev))
    torch.save({'y': y.cpu(), 'sd': {k: v.cpu() for k, v in g.state_dict().items() if 'cbns' in k}},
               os.path.join(out_dir, f'rank{rank}.pt'))
    dist.destroy_process_group()


@pytest.mark.timeout(600)
def test_data_parallel_condbn_two_ranks_one_gpu(dev, tmp_path):
    """Two processes (both on cuda:0, gloo rendezvous) each run the HIP forward on their batch shard with the per-stage
    statistics all-reduced: the gathered output and the post-forward buffers equal the single-process global-batch run."""
    import os
    import socket
    import torch.multiprocessing as mp
    B, T, world = 5, 12, 2
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        port = s.getsockname()[1]
    mp.get_context('spawn')
    mp.spawn(_dp_worker, args=(world, port, B, T, str(tmp_path)), nprocs=world, join=True)
    h = synthetic.make_hparams(num_wv_feat=768)
    sd = synthetic.make_state_dict(h, seed=0)
    full = synthetic.make_inputs(h, B, T, seed=1234)
    g = build_generator(h, sd, dev, training=True)
    with torch.no_grad():
        y_ref = g(*to_dev(full, dev)).cpu()
    parts = [torch.load(os.path.join(str(tmp_path), f'rank{r}.pt')) for r in range(world)]
    got = torch.cat([p['y'] for p in parts], dim=0)
    assert (got - y_ref).abs().max().item() <= 2e-6
    want, _ = O.generator_forward(sd, h, *full, training=True)
    assert (got - want).abs().max().item() <= TOL
    ref_sd = g.state_dict()
    for r in range(world):
        for k, v in parts[r]['sd'].items():
            a, b = v, ref_sd[k].cpu()
            if a.dtype == torch.long:
                assert a.item() == b.item(), k
            else:
                assert (a - b).abs().max().item() <= 1e-6 * max(1.0, b.abs().max().item()), k


def _ddp_worker(rank, world, port, B, T, out_dir):
    import os
    import torch.distributed as dist
    from torch.nn.parallel import DistributedDataParallel
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    from wavthruvec_pytorch_amd.distributed import shard_batch
    dev = torch.device('cuda:0')
    h = synthetic.make_hparams(num_wv_feat=768)
    sd = synthetic.make_state_dict(h, seed=0)
    g = build_generator(h, sd, dev, training=True).enable_sync_batchnorm()
    ddp = DistributedDataParallel(g)                                   # vec2wav/train.py:92
    full = synthetic.make_inputs(h, B, T, seed=99)
    dy = torch.from_numpy(np.random.default_rng(7).standard_normal((B, 1, T * 320)).astype(np.float32))
    mine = shard_batch(full, rank, world)
    lo, hi = rank * B // world, (rank + 1) * B // world
    y = ddp(*to_dev(mine, dev))
    (y * dy[lo:hi].to(dev)).sum().backward()
    torch.save({n: p.grad.cpu() for n, p in g.named_parameters()}, os.path.join(out_dir, f'grad{rank}.pt'))
    dist.destroy_process_group()


@pytest.mark.timeout(900)
def test_ddp_wrapped_generator_two_ranks_one_gpu(dev, tmp_path):
    """`DistributedDataParallel(generator)` (train.py:92) over the HIP autograd path: two ranks on batch shards with synchronised
    CondBN statistics (forward AND backward sums) - the averaged gradients x world equal the single-process global-batch gradients."""
    import os
    import socket
    import torch.multiprocessing as mp
    B, T, world = 4, 10, 2
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        port = s.getsockname()[1]
    mp.spawn(_ddp_worker, args=(world, port, B, T, str(tmp_path)), nprocs=world, join=True)
    h = synthetic.make_hparams(num_wv_feat=768)
    sd = synthetic.make_state_dict(h, seed=0)
    full = synthetic.make_inputs(h, B, T, seed=99)
    dy = torch.from_numpy(np.random.default_rng(7).standard_normal((B, 1, T * 320)).astype(np.float32))
    g = build_generator(h, sd, dev, training=True)
    y = g(*to_dev(full, dev))
    (y * dy.to(dev)).sum().backward()
    g0 = torch.load(os.path.join(str(tmp_path), 'grad0.pt'))
    g1 = torch.load(os.path.join(str(tmp_path), 'grad1.pt'))
    bad = {}
    for n, p in g.named_parameters():
        assert torch.equal(g0[n], g1[n]), n                           # DDP left identical (averaged) gradients on both ranks
        ref = p.grad.cpu()
        floor = 0.25 if (n.startswith('ups.') and n.endswith('.bias')) else 1e-6   # analytically zero under train-mode BN
        err = (g0[n] * world - ref).abs().max().item() / max(ref.abs().max().item(), floor)
        if err > 4e-3:
            bad[n] = err
    assert not bad, sorted(bad.items(), key=lambda kv: -kv[1])[:8]


def test_graph_capture_matches_eager(dev):
    """HIP-graph replay of the eval forward (inference sizes are launch-bound) == the eager launches, bit for bit."""
    h = synthetic.make_hparams(num_wv_feat=768)
    sd = synthetic.make_state_dict(h, seed=0)
    inp = to_dev(synthetic.make_inputs(h, 1, 50, seed=5), dev)
    inp2 = to_dev(synthetic.make_inputs(h, 1, 50, seed=6), dev)
    g = build_generator(h, sd, dev, training=False)
    with torch.no_grad():
        want1, want2 = g(*inp).clone(), g(*inp2).clone()
        run = g.capture_graph(*inp)
        got1 = run(*inp).clone()
        got2 = run(*inp2).clone()
    assert torch.equal(got1, want1) and torch.equal(got2, want2)
    # train mode captures too: the statistics, the spectral-norm step and the weight fold are all in-graph
    gt = build_generator(h, sd, dev, training=True)
    ge = build_generator(h, sd, dev, training=True)
    with torch.no_grad():
        run_t = gt.capture_graph(*inp, warmup=1)     # the warm-up executes one train step; the capture only records
        ge(*inp)
        y_g = run_t(*inp2).clone()
        y_e = ge(*inp2)
    assert torch.equal(y_g, y_e)
    assert gt.cbns[0].batch_nrom.num_batches_tracked.item() == ge.cbns[0].batch_nrom.num_batches_tracked.item() == 2


def test_two_captured_generators_replay_concurrently(dev):
    """ABI v28: the split-over-C_in scratch belongs to the module (Generator._slab), not to the library.  Two generators with different
    weights, captured at the inference size whose conv_pre / ups.0 / stage-0 launches ARE split (B = 1, T = 50), replay at the same time
    on two streams, many times over: every replay equals the module's own eager result bit for bit (with the library's old
    per-(device, stream) slab both graphs wrote one buffer)."""
    h = synthetic.make_hparams(num_wv_feat=768)
    gens, runs, wants, inps = [], [], [], []
    for seed in (0, 5):
        sd = synthetic.make_state_dict(h, seed=seed)
        inp = to_dev(synthetic.make_inputs(h, 1, 50, seed=20 + seed), dev)
        O.calibrate_running_stats(sd, h, *synthetic.make_inputs(h, 1, 50, seed=20 + seed))
        g = build_generator(h, sd, dev, training=False)
        with torch.no_grad():
            wants.append(g(*inp).clone())
            runs.append(g.capture_graph(*inp))
        assert any(sl.t is not None and sl.t.numel() > 0 for sl in g._slabs.values()), 'no launch of this size was split: the test would prove nothing'
        gens.append(g); inps.append(inp)
    ptrs = [{sl.t.data_ptr() for sl in g._slabs.values() if sl.t is not None} for g in gens]
    assert not (ptrs[0] & ptrs[1])                                # one scratch per module
    streams = [torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)]
    torch.cuda.synchronize()
    outs = [[], []]
    for _ in range(20):
        for i in (0, 1):
            with torch.cuda.stream(streams[i]):
                runs[i].graph.replay()                            # (the static inputs still hold inps[i] from the capture)
                outs[i].append(runs[i](*inps[i]).clone())
    torch.cuda.synchronize()
    for i in (0, 1):
        for y in outs[i]:
            assert torch.equal(y, wants[i])


def test_synthesize_entry_end_to_end(dev, tmp_path):
    """Checkpoint file + text2vec-format latents + speaker-embedding file -> wav, equal to the oracle's eval forward."""
    import os
    import wave
    from wavthruvec_pytorch_amd import synthesize as S, utils
    h = synthetic.make_hparams(num_wv_feat=768)
    sd = synthetic.make_state_dict(h, seed=0)
    x, spk, nz = synthetic.make_inputs(h, 1, 20, seed=3)
    O.calibrate_running_stats(sd, h, x, spk, nz)                      # a "trained" checkpoint: sensible running stats
    d = str(tmp_path)
    utils.save_checkpoint(os.path.join(d, 'g_00000042'), {'generator': sd})
    np.save(os.path.join(d, 'utt_feat_postnet.npy'), x.permute(0, 2, 1).numpy())     # (1, T, C) as text2vec/eval.py writes
    torch.save(spk.reshape(1, 1, -1), os.path.join(d, 'spk.pth'))
    rc = S.main(['--checkpoint', d, '--feat', os.path.join(d, 'utt_feat_postnet.npy'), '--spk-emb', os.path.join(d, 'spk.pth'),
                 '--out', os.path.join(d, 'o.wav'), '--seed', '7'])
    assert rc == 0
    noise = torch.randn(1, 192, generator=torch.Generator().manual_seed(7))
    want, _ = O.generator_forward(sd, h, x, spk, noise, training=False)
    with wave.open(os.path.join(d, 'o.wav')) as w:
        assert w.getframerate() == 16000 and w.getnframes() == 20 * 320
        pcm = np.frombuffer(w.readframes(w.getnframes()), dtype='<i2').astype(np.float32) / 32767.0
    assert np.abs(pcm - want.reshape(-1).clamp(-1, 1).numpy()).max() <= 1e-4 + 1.0 / 32767



@pytest.mark.parametrize('training,B,T,resblock,precision', [(True, 2, 8, 1, 'f32'), (True, 3, 21, 1, 'f32'), (False, 2, 8, 1, 'f32'),
                                                             (True, 2, 9, '1', 'f32'), (False, 2, 8, '1', 'f32'), (True, 2, 12, 1, 'f16x3')])
def test_generator_backward_matches_oracle_autograd(dev, training, B, T, resblock, precision):
    """`loss.backward()` through the HIP generator (train.py:214): every parameter gradient against torch autograd through the
    oracle on the CPU in fp64.  Bar: |dg| error <= 4e-3 of the largest entry of that gradient (this side reduces up to 1e5 positions in fp32).
    resblock 1 (int) = the reference default ResBlock2, '1' = ResBlock1.
    The fp32 oracle is no reference here: its gradients move with its reduction order, i.e. with torch's CPU thread count, by up to
    1.4e-2 on these inputs.  Two cases are that ill-conditioned in fp32, this path's gradients as much as the fp32 oracle's: ResBlock1 at
    T = 9 (every parameter, 1.3e-2 measured) and T = 12 (the parameters ahead of the first BatchNorm - fcs.0, cbns.0, ups.0, conv_pre -
    6.7e-3).  Those are held to the 2e-2 of test_generator_six_stages_backward_and_bf16, everything else to 4e-3."""
    h = synthetic.make_hparams(num_wv_feat=768, resblock=resblock)
    sd = synthetic.make_state_dict(h, seed=0)
    inp = synthetic.make_inputs(h, B, T, seed=21)
    dy = torch.from_numpy(np.random.default_rng(5).standard_normal((B, 1, T * 320)).astype(np.float32))
    if not training:
        O.calibrate_running_stats(sd, h, *inp)
    y_ref, g_ref, _ = O.generator_gradients(sd, h, *[t.double() for t in inp], dy, training=training, dtype=torch.float64)
    y_ref = y_ref.float()
    loose = {('1', 9): ('',), (1, 12): ('fcs.0.', 'cbns.0.', 'ups.0.', 'conv_pre.')}.get((resblock, T), ())
    g = build_generator(h, sd, dev, training=training)
    g.precision = precision          # 'f16x3': forward AND input-gradient convs of the wide layers on the split-f16 kernel
    y = g(*to_dev(inp, dev))
    assert y.requires_grad
    assert (y.detach().cpu() - y_ref).abs().max().item() <= TOL
    (y * dy.to(dev)).sum().backward()
    missing = [n for n, p in g.named_parameters() if p.grad is None]
    assert not missing, missing
    worst = {}
    for n, p in g.named_parameters():
        ref = g_ref[n]
        err = (p.grad.cpu() - ref).abs().max().item()
        # train-mode BatchNorm removes the per-channel mean, so d(ups.bias) is exactly 0 in exact arithmetic: both sides
        # only hold rounding noise there and are compared on an absolute scale
        floor = 0.25 if (training and n.startswith('ups.') and n.endswith('.bias')) else 1e-6
        worst[n] = (err / max(ref.abs().max().item(), floor), err, ref.abs().max().item())
    bad = {n: e for n, e in worst.items() if e[0] > (2e-2 if loose and n.startswith(loose) else 4e-3)}
    assert not bad, sorted(bad.items(), key=lambda kv: -kv[1][0])[:8]
    # the forward under autograd equals the no_grad forward bit for bit (same kernels, unfused schedule aside)
    g2 = build_generator(h, sd, dev, training=training)
    g2.precision = precision
    with torch.no_grad():
        y2 = g2(*to_dev(inp, dev))
    assert (y2 - y.detach()).abs().max().item() <= (1e-6 if precision == 'f32' else 5e-6)


def test_generator_backward_with_the_one_kernel_narrow_stages(dev):
    """`fuse_stage_backward` (opt-in): the input gradients of the 32- and 16-channel stages from v2w_resblock2_stage_fwd's backward form - every
    parameter gradient against the oracle's autograd at the bar of test_generator_backward_matches_oracle_autograd, and equal (to rounding) to
    the default schedule's."""
    B, T = 2, 20
    h = synthetic.make_hparams(num_wv_feat=768)
    sd = synthetic.make_state_dict(h, seed=0)
    inp = synthetic.make_inputs(h, B, T, seed=21)
    dy = torch.from_numpy(np.random.default_rng(5).standard_normal((B, 1, T * 320)).astype(np.float32))
    _, g_ref, _ = O.generator_gradients(sd, h, *[t.double() for t in inp], dy, training=True, dtype=torch.float64)   # (fp64: see above)
    got = {}
    for on in (True, False):
        g = build_generator(h, sd, dev, training=True)
        g.fuse_stage_backward = on
        (g(*to_dev(inp, dev)) * dy.to(dev)).sum().backward()
        got[on] = {n: p.grad.cpu() for n, p in g.named_parameters()}
    bad = {}
    for n, ref in g_ref.items():
        floor = 0.25 if (n.startswith('ups.') and n.endswith('.bias')) else 1e-6
        sc = max(ref.abs().max().item(), floor)
        if (got[True][n] - ref).abs().max().item() / sc > 4e-3 or (got[True][n] - got[False][n]).abs().max().item() / sc > 1e-3:
            bad[n] = ((got[True][n] - ref).abs().max().item() / sc, (got[True][n] - got[False][n]).abs().max().item() / sc)
    assert not bad, sorted(bad.items(), key=lambda kv: -kv[1][0])[:8]


@pytest.mark.parametrize('resblock', [1, '1'])
def test_generator_bf16_training_gradients_vs_reference_autocast(dev, resblock):
    """A training step in the bf16 arithmetic (`precision = 'bf16'`: forward, input-gradient and - v2w_wgrad_bf16 - weight-gradient convs
    from bf16 operands with fp32 accumulation; vec2wav/train.py:167,214 under torch.autocast).  bf16 gradients of a freshly initialised
    five-stage network sit 10 - 50 % off the fp32 ones for the early layers - for the reference's own autocast backward just as much - so
    the bar is the reference's, over the parameters: per parameter d = max|g - g_fp32| / max|g_fp32| for this path and for the oracle's
    modules under torch.autocast(bfloat16) on the same inputs; the median of d_hip / d_autocast <= 1, its 90th percentile <= 1.25, the mean of
    d_hip <= the mean of d_autocast and no parameter farther than the autocast run's worst one (measured: median 0.5, 90 % 0.8 - 0.9; a few
    conditioning biases with small deviations on both sides reach 5 x)."""
    B, T = 2, 16
    h = synthetic.make_hparams(num_wv_feat=768, resblock=resblock)
    sd = synthetic.make_state_dict(h, seed=0)
    inp = synthetic.make_inputs(h, B, T, seed=21)
    dy = torch.from_numpy(np.random.default_rng(5).standard_normal((B, 1, T * 320)).astype(np.float32))
    _, g_ref, _ = O.generator_gradients(sd, h, *inp, dy, training=True)
    with torch.autocast('cpu', dtype=torch.bfloat16):
        _, g_ac, _ = O.generator_gradients(sd, h, *inp, dy, training=True)
    g = build_generator(h, sd, dev, training=True)
    g.precision = 'bf16'
    (g(*to_dev(inp, dev)) * dy.to(dev)).sum().backward()

    def deviation(got, ref, n):
        floor = 0.25 if (n.startswith('ups.') and n.endswith('.bias')) else 1e-6
        e = got.float() - ref
        return (e.abs().max().item() / max(ref.abs().max().item(), floor),
                e.pow(2).mean().sqrt().item() / max(ref.pow(2).mean().sqrt().item(), floor))

    d_hip, d_ac = {}, {}
    for n, p in g.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), n
        d_hip[n], d_ac[n] = deviation(p.grad.cpu(), g_ref[n], n)[0], deviation(g_ac[n], g_ref[n], n)[0]
    ratio = np.sort([d_hip[n] / max(d_ac[n], 1e-9) for n in d_hip])
    print(f'[bf16 gradients vs fp32 oracle, resblock={resblock}] hip / reference-autocast deviation: median {ratio[len(ratio) // 2]:.2f}, '
          f'90% {ratio[9 * len(ratio) // 10]:.2f}, max {ratio[-1]:.2f}; mean deviation hip {np.mean(list(d_hip.values())):.3f} '
          f'autocast {np.mean(list(d_ac.values())):.3f}; worst parameter hip {max(d_hip.values()):.2f} autocast {max(d_ac.values()):.2f}')
    # half of the parameters at least as close as the reference's autocast, nine in ten within 1.25 x, none farther than its worst one
    assert ratio[len(ratio) // 2] <= 1.0 and ratio[9 * len(ratio) // 10] <= 1.25, ratio[[len(ratio) // 2, 9 * len(ratio) // 10]]
    assert np.mean(list(d_hip.values())) <= np.mean(list(d_ac.values()))
    assert max(d_hip.values()) <= max(d_ac.values()), max(d_hip, key=d_hip.get)
    d_hip = list(d_hip.values())
    assert max(d_hip) > 1e-4        # (the bf16 kernels did run)


@pytest.mark.parametrize('training,resblock', [(True, 1), (False, 1), (True, '1')])
def test_generator_input_gradient_matches_oracle_autograd(dev, training, resblock):
    """dL/dx of the latent input (the reference's Generator is an ordinary autograd citizen, models.py:116-123): conv_pre's input-gradient
    conv, against autograd through the oracle; with the parameters frozen the same value comes out (only x asks)."""
    B, T = 2, 12
    h = synthetic.make_hparams(num_wv_feat=768, resblock=resblock)
    sd = synthetic.make_state_dict(h, seed=0)
    inp = synthetic.make_inputs(h, B, T, seed=21)
    dy = torch.from_numpy(np.random.default_rng(5).standard_normal((B, 1, T * 320)).astype(np.float32))
    if not training:
        O.calibrate_running_stats(sd, h, *inp)
    _y, g_ref, _ = O.generator_gradients(sd, h, *[t.double() for t in inp], dy, training=training, dtype=torch.float64, want_x=True)
    ref = g_ref['__x__']
    x, spk, nz = to_dev(inp, dev)
    got = []
    for freeze in (False, True):
        g = build_generator(h, sd, dev, training=training)
        g.requires_grad_(not freeze)
        xg = x.clone().requires_grad_(True)
        (g(xg, spk, nz) * dy.to(dev)).sum().backward()
        assert xg.grad is not None and xg.grad.shape == x.shape
        assert (xg.grad.cpu() - ref).abs().max().item() <= 4e-3 * ref.abs().max().item(), (freeze, (xg.grad.cpu() - ref).abs().max().item())
        assert all((p.grad is None) == freeze for p in g.parameters())
        got.append(xg.grad)
    assert torch.equal(got[0], got[1])


def test_generator_backward_wide_halo_resblock2(dev):
    """ResBlock2 with kernel 11 x dilation 7: halo 35 > the 32 positions the f32 tile kernel's staging slots cover, so those convs have
    no tile configuration and run on the direct kernel - in the forward AND in the backward, whose merged-branch launches
    (ALGO_MFMA, no fallback) must not be chosen for such a stage (the probe used k = 3, dilation 1)."""
    h = synthetic.make_hparams(num_wv_feat=768, resblock_dilation_sizes=[[1, 3, 5], [1, 3, 5], [1, 7, 5]])
    sd = synthetic.make_state_dict(h, seed=0)
    B, T = 2, 8
    inp = synthetic.make_inputs(h, B, T, seed=21)
    dy = torch.from_numpy(np.random.default_rng(5).standard_normal((B, 1, T * 320)).astype(np.float32))
    y_ref, g_ref, _ = O.generator_gradients(sd, h, *[t.double() for t in inp], dy, training=True, dtype=torch.float64)   # (fp64: see above)
    y_ref = y_ref.float()
    g = build_generator(h, sd, dev, training=True)
    y = g(*to_dev(inp, dev))
    assert (y.detach().cpu() - y_ref).abs().max().item() <= TOL
    (y * dy.to(dev)).sum().backward()
    bad = {}
    for n, p in g.named_parameters():
        ref = g_ref[n]
        floor = 0.25 if (n.startswith('ups.') and n.endswith('.bias')) else 1e-6
        err = (p.grad.cpu() - ref).abs().max().item() / max(ref.abs().max().item(), floor)
        if err > 4e-3:
            bad[n] = err
    assert not bad, sorted(bad.items(), key=lambda kv: -kv[1])[:8]


@pytest.mark.parametrize('precision', ['f32', 'bf16'])
def test_generator_six_stages_backward_and_bf16(dev, precision):
    """upsample_rates (5, 4, 4, 2, 2, 2): the sixth stage runs ResBlock2 on 512 / 2^6 = 8 channels, below every fused-stage and MFMA tile
    shape.  f32: forward and every parameter gradient against the oracle's autograd.  bf16: the forward stays as close to the fp32
    oracle as bf16 operands allow (the bar of test_generator_bf16_operand_mode) whichever kernels the 8-channel layers fall to."""
    h = synthetic.make_hparams(num_wv_feat=768, upsample_rates=[5, 4, 4, 2, 2, 2], upsample_kernel_sizes=[11, 8, 8, 4, 4, 4])
    sd = synthetic.make_state_dict(h, seed=0)
    B, T = 2, 9
    inp = synthetic.make_inputs(h, B, T, seed=21)
    dy = torch.from_numpy(np.random.default_rng(5).standard_normal((B, 1, T * 640)).astype(np.float32))
    # fp64 oracle.  Through six stages the fp32 oracle's OWN gradients of the parameters ahead of the first BatchNorm (fcs.0, cbns.0,
    # ups.0, conv_pre) sit 0.5 - 1.1 % off its fp64 form on these inputs (every later parameter: 2e-6), and so do the HIP path's:
    # those are held to 2e-2, everything else to the 4e-3 of the five-stage tests
    y_ref, g_ref, _ = O.generator_gradients(sd, h, *[t.double() for t in inp], dy, training=True, dtype=torch.float64)
    y_ref = y_ref.float()
    g = build_generator(h, sd, dev, training=True)
    if precision == 'bf16':
        g.precision = 'bf16'
        with torch.no_grad():
            y = g(*to_dev(inp, dev))
        assert y.shape == (B, 1, T * 640) and torch.isfinite(y).all()
        d = (y.cpu() - y_ref).abs().max().item()
        assert 1e-6 < d <= 4e-3, f'max|dy| = {d}'
        return
    y = g(*to_dev(inp, dev))
    assert (y.detach().cpu() - y_ref).abs().max().item() <= TOL
    (y * dy.to(dev)).sum().backward()
    bad = {}
    for n, p in g.named_parameters():
        assert p.grad is not None, n
        ref = g_ref[n]
        floor = 0.25 if (n.startswith('ups.') and n.endswith('.bias')) else 1e-6
        err = (p.grad.cpu().double() - ref).abs().max().item() / max(ref.abs().max().item(), floor)
        if err > (2e-2 if n.startswith(('fcs.0.', 'cbns.0.', 'ups.0.', 'conv_pre.')) else 4e-3):
            bad[n] = err
    assert not bad, sorted(bad.items(), key=lambda kv: -kv[1])[:8]


@pytest.mark.parametrize('precision', ['f32', 'f16x3'])
def test_generator_weights_follow_the_optimizer(dev, precision):
    """The folded / packed weights are cached per parameter version: after `optim_g.step()` (train.py:215) the next forward - train
    mode and the eval-mode cache alike - runs on the updated parameters: equal to a fresh module loaded from the stepped
    state_dict and different from the forward before the step."""
    h = synthetic.make_hparams(num_wv_feat=768)
    sd = synthetic.make_state_dict(h, seed=0)
    inp = to_dev(synthetic.make_inputs(h, 2, 9, seed=31), dev)
    g = build_generator(h, sd, dev, training=True)
    g.precision = precision
    opt = torch.optim.AdamW(g.parameters(), 1e-2, betas=(0.8, 0.99))
    y1 = g(*inp)
    y1.square().mean().backward()
    opt.step()
    g.eval()
    with torch.no_grad():
        e1 = g(*inp)                  # eval forward: fills the eval-mode fold cache
    g.train()
    g(*inp).square().mean().backward()
    opt.step()                        # parameters move again: the eval cache is stale now
    stepped = {k: v.clone() for k, v in g.state_dict().items()}
    g.eval()
    with torch.no_grad():
        e2 = g(*inp)
    g2 = build_generator(h, stepped, dev, training=False)
    g2.precision = precision
    with torch.no_grad():
        e3 = g2(*inp)
    assert torch.equal(e2, e3)
    assert (e2 - e1).abs().max().item() > 1e-4 and (y1.detach() - e1).abs().max().item() > 1e-4


# ---------------------------------------------------------------------------------------------------------------
# Full-size parity against the pinned oracle (one CPU forward each: cfg2 ~12 s, cfg5 ~12 s, cfg3 ~1 min on the box's cores)
def _reference_bf16_deviation(sd, h, inp, want, training=True):
    """How far the REFERENCE's own bf16 arithmetic (the oracle's modules under torch.autocast(bfloat16), the only bf16 mode the
    reference's stack offers; inference.py / train.py run fp32) lands from its fp32 result on these inputs: (max, rms).  The
    deviation grows with the number of samples the max runs over (2e-3 at B=2 x T=50, 7e-3 at B=64 x T=512), so a bf16 bar is
    only meaningful at the same size on the same inputs."""
    with torch.autocast('cpu', dtype=torch.bfloat16):
        yb, _ = O.generator_forward(dict(sd), h, *inp, training=training)
    e = yb.float() - want
    return e.abs().max().item(), e.pow(2).mean().sqrt().item()


def _full_size_case(dev, h, B, T, seed, precisions, training=True):
    """HIP forward at a BASELINE configuration's full size vs ONE oracle forward: y (per precision mode with its
    bar), BatchNorm running statistics, num_batches_tracked and the spectral-norm u / v after the step (f32 path).  A bar of
    'ref-bf16' means: no farther (max AND rms) from the fp32 oracle than the reference's own bf16 autocast run is.
    training=False: calibrated eval (running statistics := the batch statistics of these inputs, SURVEY 8(c): a fresh-init eval
    forward is ill-conditioned), buffers must stay untouched."""
    sd = synthetic.make_state_dict(h, seed=0)
    inp = synthetic.make_inputs(h, B, T, seed=seed)
    if not training:
        O.calibrate_running_stats(sd, h, *inp)
    want, nb = O.generator_forward(sd, h, *inp, training=training)
    xin = to_dev(inp, dev)
    out = {}
    for prec, bar in precisions:
        g = build_generator(h, sd, dev, training=training)
        storage = True
        if prec == 'bf16-operands':
            prec, storage = 'bf16', False
        g.precision = prec
        g.bf16_storage = storage
        with torch.no_grad():
            y = g(*xin)
        assert y.shape == want.shape and torch.isfinite(y).all()
        e = y.cpu() - want
        d = e.abs().max().item()
        out[prec if storage else 'bf16-operands'] = d
        if bar == 'ref-bf16':
            if 'ref' not in out:
                out['ref'] = _reference_bf16_deviation(sd, h, inp, want, training)
            rmax, rrms = out['ref']
            rms = e.pow(2).mean().sqrt().item()
            print(f'[bf16 vs fp32 oracle @ B={B} T={T}] storage={storage}: max {d:.2e} rms {rms:.2e}; reference autocast: max {rmax:.2e} rms {rrms:.2e}')
            assert d <= rmax and rms <= rrms, f'{prec} (storage={storage}): max {d} rms {rms} vs reference autocast max {rmax} rms {rrms}'
        else:
            assert d <= bar, f'{prec}: max|dy| = {d} > {bar}'
        if prec == 'f32':
            ref = dict(sd)
            O.apply_buffers(ref, nb)
            post = g.state_dict()
            for k in nb:
                a, b = post[k].cpu(), ref[k]
                if a.dtype == torch.long:
                    assert a.item() == b.item(), k
                else:
                    assert (a - b).abs().max().item() <= 2e-5 * max(1.0, b.abs().max().item()), k
        del g, y
        torch.cuda.empty_cache()
    return out


@pytest.mark.timeout(900)
def test_generator_cfg2_full_size_vs_oracle_train(dev):
    """BASELINE configs[1] (the bench line): B=32, T=256, 768-d, x320, fp32, TRAIN mode - BatchNorm statistics reduced over
    32 x L elements per channel (2.6 M at the last stage), the place fp32 summation order matters most.  |dy| <= 1e-4 for the
    exact-fp32 path AND the split-f16 mode; running statistics and spectral-norm state equal the oracle's."""
    h = synthetic.make_hparams(num_wv_feat=768)
    _full_size_case(dev, h, 32, 256, 1234, [('f32', TOL), ('f16x3', TOL)])


@pytest.mark.timeout(900)
def test_generator_cfg2_full_size_vs_oracle_eval(dev):
    """The same configuration in EVAL mode at full size (the inference pipeline's mode: running statistics, no spectral-norm step,
    weights folded once): every sample of the batch against the oracle's calibrated-eval forward, buffers unchanged."""
    h = synthetic.make_hparams(num_wv_feat=768)
    _full_size_case(dev, h, 32, 256, 1234, [('f32', TOL), ('f16x3', TOL)], training=False)


@pytest.mark.timeout(900)
def test_generator_cfg2_bf16_full_size_vs_oracle_eval(dev):
    """The inference schedule bench.py reports as `inference_bf16` - eval mode, bf16 compute / fp32 accumulate, bf16 tensors between the
    layers, B=32 x T=256: no farther from the fp32 oracle's calibrated-eval forward (max and rms) than the oracle under bf16 autocast in
    the same mode on the same inputs."""
    h = synthetic.make_hparams(num_wv_feat=768)
    d = _full_size_case(dev, h, 32, 256, 1234, [('bf16', 'ref-bf16')], training=False)
    assert d['bf16'] > 1e-6        # really ran in bf16


@pytest.mark.timeout(1200)
def test_generator_resblock1_full_size_vs_oracle_train(dev):
    """The ResBlock1 generator (h.resblock == '1', models.py:13-44: 2 665 GFLOP at this size) at the cfg2 shape
    B=32 x T=256, fp32, train mode: |dy| <= 1e-4 against the pinned oracle, buffers equal (bench.py reports it as resblock1_f32)."""
    h = synthetic.make_hparams(num_wv_feat=768, resblock='1')
    _full_size_case(dev, h, 32, 256, 1234, [('f32', TOL)])


@pytest.mark.timeout(1800)
def test_generator_resblock1_bf16_full_size_vs_oracle_train(dev):
    """The ResBlock1 generator at the cfg2 shape in the configs[2] arithmetic (bf16 compute / fp32 accumulate, bf16 tensors between the layers):
    held, like cfg3, to the reference's own bf16-autocast deviation on the same inputs (max and rms)."""
    h = synthetic.make_hparams(num_wv_feat=768, resblock='1')
    _full_size_case(dev, h, 32, 256, 1234, [('bf16', 'ref-bf16')])


@pytest.mark.timeout(900)
def test_generator_cfg5_full_size_vs_oracle_train(dev):
    """BASELINE configs[4]: 1024-d latents, upsample (8,5,4,2,2) x640 with kernels (16,11,8,4,4), B=16, T=256, fp32, train mode."""
    h = synthetic.make_hparams(num_wv_feat=1024, upsample_rates=[8, 5, 4, 2, 2], upsample_kernel_sizes=[16, 11, 8, 4, 4])
    _full_size_case(dev, h, 16, 256, 55, [('f32', TOL)])


@pytest.mark.timeout(1800)
def test_generator_cfg3_full_size_vs_oracle_train(dev):
    """BASELINE configs[2]: B=64, T=512 (10.5 M samples).  The fp32 oracle is the reference for BOTH the exact-fp32 path (1e-4)
    and the configuration's own arithmetic - bf16 compute / fp32 accumulate, with bf16 activation storage (the default of
    precision='bf16') and with fp32 storage (bf16_storage=False).  The reference defines no bf16 tolerance, so the bar is the
    reference's own bf16 behaviour measured here on the same inputs: both modes must sit no farther from the fp32 oracle (max and
    rms) than the oracle run under bf16 autocast does (7e-3 max / 7.5e-4 rms at this size)."""
    h = synthetic.make_hparams(num_wv_feat=768)
    d = _full_size_case(dev, h, 64, 512, 4, [('f32', TOL), ('bf16', 'ref-bf16'), ('bf16-operands', 'ref-bf16')])
    assert d['bf16'] > 1e-6 and d['bf16-operands'] > 1e-6     # the bf16 modes really ran in bf16
    assert d['bf16-operands'] <= 4e-3                           # operand-only rounding keeps the small-size bar even here


# ---------------------------------------------------------------------------------------------------------------
# RCCL (backend "nccl") and non-current-device coverage: need two GPUs in ONE box; skipped on the single-GPU boxes
def _rccl_worker(rank, world, port, B, T, out_dir):
    import os
    import torch.distributed as dist
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    os.environ.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')
    dev = torch.device('cuda', rank)          # NO torch.cuda.set_device: the reference never calls it (train.py:63-94)
    dist.init_process_group('nccl', rank=rank, world_size=world, device_id=dev)
    from wavthruvec_pytorch_amd.distributed import shard_batch
    h = synthetic.make_hparams(num_wv_feat=768)
    sd = synthetic.make_state_dict(h, seed=0)
    g = build_generator(h, sd, dev, training=True).enable_sync_batchnorm()
    assert g.stat_sync.backend == 'nccl'
    mine = shard_batch(synthetic.make_inputs(h, B, T, seed=1234), rank, world)
    with torch.no_grad():
        y = g(*to_dev(mine, dev))
    torch.save({'y': y.cpu(), 'sd': {k: v.cpu() for k, v in g.state_dict().items() if 'cbns' in k}},
               os.path.join(out_dir, f'rank{rank}.pt'))
    dist.barrier(device_ids=[rank])
    dist.destroy_process_group()


@pytest.mark.timeout(600)
def test_data_parallel_condbn_two_ranks_rccl(dev, tmp_path):
    """Two ranks on two GPUs over RCCL: the device-tensor fp64 all-reduce of the CondBN statistics (distributed.py) and a
    generator living on a device that is NOT the current one (rank 1: cuda:1 with current device 0)."""
    if torch.cuda.device_count() < 2:
        pytest.skip('needs two GPUs in one box (RCCL cannot run two ranks on one device)')
    import os
    import socket
    import torch.multiprocessing as mp
    B, T, world = 5, 12, 2
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        port = s.getsockname()[1]
    mp.spawn(_rccl_worker, args=(world, port, B, T, str(tmp_path)), nprocs=world, join=True)
    h = synthetic.make_hparams(num_wv_feat=768)
    sd = synthetic.make_state_dict(h, seed=0)
    full = synthetic.make_inputs(h, B, T, seed=1234)
    want, _ = O.generator_forward(sd, h, *full, training=True)
    parts = [torch.load(os.path.join(str(tmp_path), f'rank{r}.pt')) for r in range(world)]
    got = torch.cat([p['y'] for p in parts], dim=0)
    assert (got - want).abs().max().item() <= TOL
    for k, v in parts[0]['sd'].items():
        assert torch.equal(v, parts[1]['sd'][k]), k          # both ranks end with identical buffers


def _rccl_single_rank_worker(rank, port, B, T, out_dir, use_ddp):
    """ONE rank over RCCL on the one GPU of a test box: `init_process_group('nccl', world_size=1, device_id=cuda:0)` creates a real
    communicator, and `BNStatSync` issues its all-reduces on it (distributed.py: one-rank RCCL groups run the collective)."""
    import os
    import torch.distributed as dist
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    os.environ.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')
    dev = torch.device('cuda', 0)
    dist.init_process_group('nccl', rank=0, world_size=1, device_id=dev)
    h = synthetic.make_hparams(num_wv_feat=768)
    sd = synthetic.make_state_dict(h, seed=0)
    inp = synthetic.make_inputs(h, B, T, seed=1234)
    dy = torch.from_numpy(np.random.default_rng(7).standard_normal((B, 1, T * 320)).astype(np.float32))
    # the un-synchronised run of the same global batch (world 1: the shard IS the batch)
    g0 = build_generator(h, sd, dev, training=True)
    with torch.no_grad():
        y0 = g0(*to_dev(inp, dev))
    gd = build_generator(h, sd, dev, training=True).enable_sync_batchnorm()
    assert not gd.stat_sync.single_rank_collective                  # the product default: a one-rank group issues no collective
    with torch.no_grad():
        gd(*to_dev(inp, dev))
    assert gd.stat_sync.calls == 0
    g = build_generator(h, sd, dev, training=True).enable_sync_batchnorm(single_rank_collective=True)
    assert g.stat_sync.backend == 'nccl' and g.stat_sync.world_size == 1 and g.stat_sync.single_rank_collective
    with torch.no_grad():
        y = g(*to_dev(inp, dev))
    assert g.stat_sync.calls == g.num_upsamples                      # one all-reduce per stage really went out
    assert torch.equal(y, y0)                                        # a one-rank sum changes nothing, bit for bit
    for k, v in g.state_dict().items():
        if 'cbns' in k:
            assert torch.equal(v, g0.state_dict()[k]), k
    # forward + backward under autograd (train.py:167-214), optionally through DistributedDataParallel (train.py:92)
    g2 = build_generator(h, sd, dev, training=True).enable_sync_batchnorm(single_rank_collective=True)
    model = g2
    if use_ddp:
        from torch.nn.parallel import DistributedDataParallel
        model = DistributedDataParallel(g2, device_ids=[0])
    yb = model(*to_dev(inp, dev))
    (yb * dy.to(dev)).sum().backward()
    assert g2.stat_sync.calls == 2 * g2.num_upsamples                # + one all-reduce of the CondBN backward sums per stage
    torch.cuda.synchronize()
    torch.save({'y': y.cpu(), 'yb': yb.detach().cpu(), 'grads': {n: p.grad.cpu() for n, p in g2.named_parameters()},
                'sd': {k: v.cpu() for k, v in g.state_dict().items() if 'cbns' in k}}, os.path.join(out_dir, 'rank0.pt'))
    dist.barrier(device_ids=[0])
    dist.destroy_process_group()


@pytest.mark.timeout(900)
@pytest.mark.parametrize('use_ddp', [False, True])
def test_rccl_single_rank_condbn_forward_backward(dev, tmp_path, use_ddp):
    """The RCCL (`backend='nccl'`) branch of the data-parallel CondBN on real hardware: a one-rank communicator on the box's one
    GPU (BASELINE configs[3] needs 8; the driver runs that).  Executes `init_process_group(device_id=...)`, the fp64 device
    all-reduce of `[sum | sumsq | count]` on the compute stream between the transposed conv and `bn_finalize` (with the
    conditioning side stream joined around it), the backward's all-reduce of the CondBN sums, and DDP's own bucket all-reduce -
    and checks forward, every parameter gradient and the post-forward buffers against the pinned oracle (train.py:58-60, 91-94)."""
    import os
    import socket
    import torch.multiprocessing as mp
    B, T = 5, 12
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        port = s.getsockname()[1]
    mp.spawn(_rccl_single_rank_worker, args=(port, B, T, str(tmp_path), use_ddp), nprocs=1, join=True)
    got = torch.load(os.path.join(str(tmp_path), 'rank0.pt'))
    h = synthetic.make_hparams(num_wv_feat=768)
    sd = synthetic.make_state_dict(h, seed=0)
    inp = synthetic.make_inputs(h, B, T, seed=1234)
    dy = torch.from_numpy(np.random.default_rng(7).standard_normal((B, 1, T * 320)).astype(np.float32))
    want, nb = O.generator_forward(sd, h, *inp, training=True)
    assert (got['y'] - want).abs().max().item() <= TOL
    assert (got['yb'] - want).abs().max().item() <= TOL
    ref = dict(sd)
    O.apply_buffers(ref, nb)
    for k, v in got['sd'].items():
        if v.dtype == torch.long:
            assert v.item() == ref[k].item(), k
        else:
            assert (v - ref[k]).abs().max().item() <= 2e-5 * max(1.0, ref[k].abs().max().item()), k
    _, g_ref, _ = O.generator_gradients(sd, h, *[t.double() for t in inp], dy, training=True, dtype=torch.float64)   # (fp64: see above)
    bad = {}
    for n, gr in got['grads'].items():
        floor = 0.25 if (n.startswith('ups.') and n.endswith('.bias')) else 1e-6
        err = (gr - g_ref[n]).abs().max().item() / max(g_ref[n].abs().max().item(), floor)
        if err > 4e-3:
            bad[n] = err
    assert not bad, sorted(bad.items(), key=lambda kv: -kv[1])[:8]


def test_generator_on_a_non_current_device():
    """`Generator(h).to('cuda:1')` driven while the current device is 0 (train.py:63-94 never calls set_device): forward and
    backward agree with the same model on cuda:0."""
    if torch.cuda.device_count() < 2:
        pytest.skip('needs two GPUs')
    h = synthetic.make_hparams(num_wv_feat=768)
    sd = synthetic.make_state_dict(h, seed=0)
    inp = synthetic.make_inputs(h, 2, 9, seed=5)
    ys, grads = [], []
    assert torch.cuda.current_device() == 0
    for d in (0, 1):
        devd = torch.device('cuda', d)
        g = build_generator(h, sd, devd, training=True)
        y = g(*to_dev(inp, devd))
        y.square().sum().backward()
        assert torch.cuda.current_device() == 0
        ys.append(y.detach().cpu())
        grads.append({n: p.grad.cpu() for n, p in g.named_parameters()})
    assert torch.equal(ys[0], ys[1])
    for n in grads[0]:
        assert torch.equal(grads[0][n], grads[1][n]), n


# ---------------------------------------------------------------------------------------------------------------
# bench.py launcher contract
def _run_bench(args, env_extra=None, timeout=600, expect_ok=True):
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ)
    for k in ('RANK', 'LOCAL_RANK', 'WORLD_SIZE', 'MASTER_ADDR', 'MASTER_PORT'):
        env.pop(k, None)
    env.update(env_extra or {})
    cmd = [sys.executable, os.path.join(root, 'bench.py')] + args
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=timeout)
    if r.returncode != 0 and expect_ok:
        # multi-process rendezvous on a freshly booted box fails once in a while (seen once in six full runs, round 6; not reproducible in
        # isolation): ONE more attempt, the first failure on stderr for the record - the assertions then hold the second attempt to the contract
        sys.stderr.write(f'[bench launcher test] first attempt exited {r.returncode}:\n{r.stderr[-3000:]}\n')
        r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=timeout)
    return r


@pytest.mark.timeout(900)
def test_bench_self_launches_the_ranks_it_was_asked_for(dev):
    """`python bench.py --gpus 2` with no launcher: starts 2 ranks itself and reports n_gpus == 2 (on a single-GPU box through the
    one-device / gloo test hooks), and its N=1 line carries the same metric.  Without the hooks, asking for more GPUs than the box
    has must FAIL (never a silent single-GPU line)."""
    import json
    small = ['--steps', '2', '--warmup', '1', '--no-cpu-baseline', '--no-alt', '--batch', '2', '--frames', '16']
    ngpu = torch.cuda.device_count()
    hooks = {} if ngpu >= 2 else {'V2W_BENCH_DEVICE': '0', 'V2W_BENCH_BACKEND': 'gloo'}
    r = _run_bench(['--gpus', '2'] + small, hooks)
    assert r.returncode == 0, r.stderr[-2000:]
    line = [l for l in r.stdout.splitlines() if l.startswith('{')]
    assert len(line) == 1, r.stdout
    d = json.loads(line[0])
    assert d['n_gpus'] == 2 and d['config']['global_batch'] == 4 and d['scaling'] == 'weak'
    assert d['rccl_ranks'] == (2 if ngpu >= 2 else None)
    r1 = _run_bench(['--gpus', '1'] + small)
    assert r1.returncode == 0, r1.stderr[-2000:]
    d1 = json.loads([l for l in r1.stdout.splitlines() if l.startswith('{')][0])
    assert d1['n_gpus'] == 1 and d1['rccl_ranks'] == 1 and d1['metric'] == d['metric']
    too_many = _run_bench(['--gpus', str(ngpu + 1)] + small, expect_ok=False)
    assert too_many.returncode != 0 and not [l for l in too_many.stdout.splitlines() if l.startswith('{')]


@pytest.mark.timeout(1200)
def test_bench_eight_ranks_first_contact(dev):
    """The driver's 8-GPU command line, on whatever this box has: `bench.py --gpus 8` at the real per-rank workload (B = 32 x T = 256), eight
    processes that each run the train-mode forward with the CondBN statistics all-reduced every stage.  On a box with fewer than 8 GPUs
    the ranks share device 0 and meet over gloo (test hooks); the bookkeeping - one JSON line, n_gpus 8, global batch 256, weak scaling,
    a throughput that counts all eight shards - is the same code an 8-GPU node runs."""
    import json
    ngpu = torch.cuda.device_count()
    hooks = {} if ngpu >= 8 else {'V2W_BENCH_DEVICE': '0', 'V2W_BENCH_BACKEND': 'gloo'}
    r = _run_bench(['--gpus', '8', '--steps', '2', '--warmup', '1', '--no-cpu-baseline', '--no-alt'], hooks, timeout=1100)
    assert r.returncode == 0, r.stderr[-3000:]
    line = [l for l in r.stdout.splitlines() if l.startswith('{')]
    assert len(line) == 1 and len([l for l in r.stdout.splitlines() if l.strip()]) == 1, r.stdout[-2000:]
    d = json.loads(line[0])
    assert d['n_gpus'] == 8 and d['config']['global_batch'] == 256 and d['scaling'] == 'weak' and d['steps'] == 2
    assert d['rccl_ranks'] == (8 if ngpu >= 8 else None)
    assert abs(d['value'] - 8 * 32 * 256 * 320 / (d['ms_per_step'] * 1e-3)) <= 1e-6 * d['value']      # whole-job samples / max-over-ranks time


# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['1', 1])
def test_standalone_resblock_forward_matches_the_oracle(dev, kind):
    """`ResBlock1(h, C, k, d)(x)` / `ResBlock2(...)(x)` are callable in the reference (models.py:37-44, 65-70); here they run their
    convs through the C ABI.  Checked against the oracle's block restatement."""
    from wavthruvec_pytorch_amd.models import ResBlock1, ResBlock2
    h = synthetic.make_hparams(num_wv_feat=768, resblock=kind)
    rng = np.random.default_rng(5)
    C, L, k = 32, 500, 7
    rb = (ResBlock1(h, C, k, (1, 3, 5)) if kind == '1' else ResBlock2(h, C, k, (1, 3))).to(dev)
    sd = {n: v.detach().cpu() for n, v in rb.state_dict().items()}
    x = torch.from_numpy(rng.standard_normal((2, C, L)).astype(np.float32))
    want = O._resblock({'rb.' + n: v for n, v in sd.items()}, 'rb', x, k, (1, 3, 5) if kind == '1' else (1, 3), kind == '1', torch.float32)
    with torch.no_grad():
        got = rb(x.to(dev))
    assert (got.cpu() - want).abs().max().item() <= 2e-5
    # ... and differentiable, as the reference's modules are: input and every parameter gradient against autograd through the oracle's block
    dy = torch.from_numpy(rng.standard_normal((2, C, L)).astype(np.float32))
    leaves = {n: v.clone().requires_grad_(True) for n, v in sd.items()}
    xr = x.clone().requires_grad_(True)
    (O._resblock({'rb.' + n: v for n, v in leaves.items()}, 'rb', xr, k, (1, 3, 5) if kind == '1' else (1, 3), kind == '1', torch.float32) * dy).sum().backward()
    xg = x.to(dev).requires_grad_(True)
    out = rb(xg)
    assert out.requires_grad and torch.equal(out.detach(), got)
    (out * dy.to(dev)).sum().backward()
    assert (xg.grad.cpu() - xr.grad).abs().max().item() <= 2e-3 * xr.grad.abs().max().item()
    for n, p in rb.named_parameters():
        assert p.grad is not None, n
        ref = leaves[n].grad
        assert (p.grad.cpu() - ref).abs().max().item() <= 4e-3 * max(ref.abs().max().item(), 1e-6), n
    xg2 = x.to(dev).requires_grad_(True)       # only the input asks
    rb.requires_grad_(False)
    rb(xg2).backward(dy.to(dev))
    assert torch.allclose(xg2.grad, xg.grad, rtol=0, atol=1e-6 * xr.grad.abs().max().item() + 1e-7)


def test_backward_uses_the_spectral_norm_state_of_its_own_forward(dev):
    """Two train-mode forwards, then backward through the FIRST: the spectral-norm u / v advanced in between, and the gradient of
    `weight_orig` must be the one of the first forward's sigma = u^T W v (the live buffers were read at backward time)."""
    h = synthetic.make_hparams(num_wv_feat=768)
    sd = synthetic.make_state_dict(h, seed=0)
    inp = to_dev(synthetic.make_inputs(h, 2, 6, seed=8), dev)
    dy = torch.from_numpy(np.random.default_rng(1).standard_normal((2, 1, 6 * 320)).astype(np.float32)).to(dev)
    g1 = build_generator(h, sd, dev, training=True)
    y = g1(*inp)
    (y * dy).sum().backward()
    ref = {n: p.grad.clone() for n, p in g1.named_parameters() if 'cbns' in n}
    g2 = build_generator(h, sd, dev, training=True)
    y = g2(*inp)
    with torch.no_grad():
        g2(*inp)                      # a second forward before the backward of the first: u, v move on
    (y * dy).sum().backward()
    for n, p in g2.named_parameters():
        if 'cbns' in n:
            assert torch.equal(p.grad, ref[n]), n


def test_direct_kernels_refuse_autograd_with_a_clear_message(dev):
    from wavthruvec_pytorch_amd import hipops
    h = synthetic.make_hparams(num_wv_feat=768)
    g = build_generator(h, synthetic.make_state_dict(h, seed=0), dev, training=True)
    g.algo = hipops.ALGO_DIRECT
    with pytest.raises(NotImplementedError, match='ALGO_AUTO'):
        g(*to_dev(synthetic.make_inputs(h, 1, 4, seed=1), dev))
