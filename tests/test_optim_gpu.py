"""GPU tests of the multi-tensor AdamW kernel (v2w_adamw_multi) and of optim.AdamW: every entry of p, exp_avg and exp_avg_sq against the
fp64 restatement tests/optim_ref.py at the bound the header's operation list gives, guard regions around everything the kernel writes,
the parameters' version counters (the caches of folded / packed weights are keyed on them), and training steps against torch's."""
import numpy as np
import pytest
import torch

from oracle import disc_oracle as D
from tests import optim_ref as R
from wavthruvec_pytorch_amd import AdamW, _hip, hipops, synthetic
from wavthruvec_pytorch_amd import optim as optim_mod

pytestmark = pytest.mark.gpu
TOL = 1e-4          # the project's bar on O(1) outputs
PAD = 32            # guard floats on either side of every tensor the kernel writes
SENTINEL = 12345.678


@pytest.fixture(scope='module')
def dev():
    _hip.load()
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


@pytest.fixture
def launches(monkeypatch):
    """The launch counts hipops.adamw_multi returns, one entry per call optim.AdamW makes."""
    seen = []
    orig = hipops.adamw_multi
    monkeypatch.setattr(optim_mod.hipops, 'adamw_multi', lambda *a, **kw: (seen.append(orig(*a, **kw)), seen[-1])[1])
    return seen


def _guarded(values, phase, dev):
    """(buffer, view): `values` placed `phase` floats past a 16-byte line inside a buffer whose other floats hold the sentinel."""
    n = values.size
    buf = torch.full((PAD + n + PAD + 4,), SENTINEL, device=dev)
    assert buf.data_ptr() % 16 == 0
    view = buf[PAD + phase:PAD + phase + n]
    view.copy_(torch.from_numpy(values))
    return buf, view


def _borders_intact(buf, view):
    off = (view.data_ptr() - buf.data_ptr()) // 4
    return bool((buf[:off] == SENTINEL).all()) and bool((buf[off + view.numel():] == SENTINEL).all())


@pytest.mark.parametrize('t', R.KERNEL_STEPS)
def test_kernel_matches_the_fp64_restatement_per_entry(dev, t, launches):
    """One step from random fp32 state at step number t.  c = 2 x the roundings the header counts on each output's path
    (p': 15, m': 3, v': 4 -> c = 30 / 6 / 8), times 2^-24, times the magnitudes of optim_ref."""
    assert R.ROUNDINGS == {'p': 15, 'm': 3, 'v': 4}
    rng = np.random.default_rng(R.KERNEL_SEED)
    h = R.make_hyper(step=t, **R.KERNEL_HYPER)
    cases = R.kernel_cases(_hip.ADAMW_MAX_ITEMS)
    params, rows = [], []
    opt_state = {}
    for numel, kind in cases:
        p, g, m, v = R.kernel_state(numel, rng)
        ph = {'p_view': (1, 0, 0, 0), 'g_view': (0, 1, 0, 0), 'all_view': (1, 1, 1, 1)}.get(kind, (0, 0, 0, 0))
        bufs = [_guarded(x, k, dev) for x, k in zip((p, g, m, v), ph)]
        shape = (6, 35) if kind == 'g_strided' else (numel,)
        par = bufs[0][1].view(shape).requires_grad_()
        if kind == 'g_strided':
            par.grad = bufs[1][1].view(shape).t().contiguous().t()
            assert not par.grad.is_contiguous() and torch.equal(par.grad.flatten().cpu(), torch.from_numpy(g))
        elif kind != 'no_grad':
            par.grad = bufs[1][1]
        if kind != 'no_grad':
            opt_state[par] = dict(step=torch.tensor(float(t - 1)), exp_avg=bufs[2][1].view(shape), exp_avg_sq=bufs[3][1].view(shape))
        assert [b[1].data_ptr() % 16 for b in bufs] == [4 * k for k in ph]
        params.append(par)
        rows.append((kind, (p, g, m, v), bufs))
    opt = AdamW(params, **R.KERNEL_HYPER)
    for par, st in opt_state.items():
        opt.state[par] = st
    versions = [p._version for p in params]
    opt.step()
    torch.cuda.synchronize()
    assert launches == [2]                                     # MAX_ITEMS + 3 items: ceil((MAX_ITEMS + 3) / MAX_ITEMS) launches, one call
    worst = 0.0
    for par, ver, (kind, (p, g, m, v), bufs) in zip(params, versions, rows):
        assert all(_borders_intact(*bufs[k]) for k in (0, 2, 3)), kind
        got = tuple(bufs[k][1].cpu().numpy() for k in (0, 2, 3))
        assert np.array_equal(bufs[1][1].cpu().numpy(), g)                                   # the gradient is only read
        if kind == 'no_grad':
            assert all(np.array_equal(a, b) for a, b in zip(got, (p, m, v))) and par not in opt.state and par._version == ver
            continue
        rp, rm, rv, mags = R.adamw_ref(p, g, m, v, h)
        ratio = R.worst_ratio(got, (rp, rm, rv), R.bounds(mags))
        worst = max(worst, ratio)
        assert ratio <= 1.0, (kind, p.size, ratio)
        assert float(opt.state[par]['step']) == t and par._version > ver
        assert not np.array_equal(got[0], p) or p.size < 4                                   # the step did move the parameter
    print(f't={t}: worst |delta| / bound = {worst:.3f}')


def _flat(ts):
    return torch.cat([x.detach().flatten() for x in ts]).cpu().numpy()


def test_lockstep_over_five_steps_on_the_generators_parameters(dev, launches):
    """optim.AdamW under ExponentialLR on the generator's 131 parameter tensors, random gradients: every step against optim_ref from the
    kernel's own previous state, at the kernel test's bound; state['step'] and group['lr'] as torch's."""
    from wavthruvec_pytorch_amd import Generator
    h = synthetic.make_hparams(num_wv_feat=768)
    g = Generator(h)
    g.load_state_dict(synthetic.make_state_dict(h, seed=0))
    params = list(g.to(dev).parameters())
    assert len(params) == 131
    kw = dict(lr=2e-4, betas=(0.8, 0.99), eps=1e-8, weight_decay=0.01)
    opt = AdamW(params, **kw)
    sched = torch.optim.lr_scheduler.ExponentialLR(opt, gamma=0.9)
    gen = torch.Generator(device=dev).manual_seed(7)
    m0 = v0 = np.zeros(sum(p.numel() for p in params), dtype=np.float32)
    for t in range(1, 6):
        lr = opt.param_groups[0]['lr']
        assert abs(lr - 2e-4 * 0.9 ** (t - 1)) <= 1e-12
        for p in params:
            p.grad = torch.randn(p.shape, device=dev, generator=gen) * 1e-2
        p0, g0 = _flat(params), _flat([p.grad for p in params])
        opt.step()
        sched.step()
        hyper = R.make_hyper(step=t, **dict(kw, lr=lr))
        rp, rm, rv, mags = R.adamw_ref(p0, g0, m0, v0, hyper)
        got = (_flat(params), _flat([opt.state[p]['exp_avg'] for p in params]), _flat([opt.state[p]['exp_avg_sq'] for p in params]))
        assert R.worst_ratio(got, (rp, rm, rv), R.bounds(mags)) <= 1.0, t
        assert all(float(opt.state[p]['step']) == t and not opt.state[p]['step'].is_cuda for p in params)
        m0, v0 = got[1], got[2]
    assert launches == [-(-131 // _hip.ADAMW_MAX_ITEMS)] * 5


def test_stepped_parameters_bump_their_version_and_the_weight_caches_follow(dev):
    """The kernel writes through raw pointers: without increment_version the eval-mode fold of the generator and the discriminators'
    per-version weight records would go on serving the weights from before the step."""
    from wavthruvec_pytorch_amd import Generator
    from wavthruvec_pytorch_amd.discriminators import DiscriminatorP, DiscriminatorS
    h = synthetic.make_hparams(num_wv_feat=768)
    g = Generator(h)
    g.load_state_dict(synthetic.make_state_dict(h, seed=0))
    g = g.to(dev).eval()
    inp = tuple(x.to(dev) for x in synthetic.make_inputs(h, 1, 8, seed=3))
    mpd_sd = synthetic.make_disc_state_dict(synthetic.mpd_state_dict_spec(), seed=13)
    msd_sd = synthetic.make_disc_state_dict(synthetic.msd_state_dict_spec(), seed=13)
    dp, ds = DiscriminatorP(synthetic.DEFAULT_PERIODS[1]), DiscriminatorS()
    dp.load_state_dict({k[len('discriminators.1.'):]: v for k, v in mpd_sd.items() if k.startswith('discriminators.1.')})
    ds.load_state_dict({k[len('discriminators.1.'):]: v for k, v in msd_sd.items() if k.startswith('discriminators.1.')})
    dp, ds = dp.to(dev), ds.to(dev)
    y = synthetic.make_audio_pair(1, 1500, seed=3)[0].to(dev)
    with torch.no_grad():
        before = [g(*inp), dp(y)[0], ds(y)[0]]               # fills the eval-mode fold cache / the per-version weight records
    gen = torch.Generator(device=dev).manual_seed(1)
    params = [p for mod in (g, dp, ds) for p in mod.parameters()]
    for p in params:
        p.grad = torch.randn(p.shape, device=dev, generator=gen)
    versions = [p._version for p in params]
    AdamW(params, 1e-2, betas=(0.8, 0.99)).step()
    assert all(p._version > ver for p, ver in zip(params, versions))
    g2 = Generator(h)
    g2.load_state_dict(g.state_dict())
    dp2, ds2 = DiscriminatorP(dp.period), DiscriminatorS()
    dp2.load_state_dict(dp.state_dict())
    ds2.load_state_dict(ds.state_dict())
    with torch.no_grad():
        after = [g(*inp), dp(y)[0], ds(y)[0]]
        fresh = [g2.to(dev).eval()(*inp), dp2.to(dev)(y)[0], ds2.to(dev)(y)[0]]
    for b, a, f in zip(before, after, fresh):
        assert (a - f).abs().max().item() <= TOL
        assert (a - b).abs().max().item() > 10 * TOL         # the step moved the outputs: a stale cache would fail the line above


def test_three_training_steps_match_torchs_adamw(dev):
    """The B=2, T=8 generator (the rb2_train_b2_t8 shape), three steps with optim.AdamW against the same three with
    torch.optim.AdamW(foreach=False): final waveforms and parameters at the 1e-4 bar.

    lr = 2e-4 (the reference's) and eps = 1e-3, not torch's default 1e-8.  The two runs see bit-identical gradients at step 1 only; from
    step 2 on their parameters differ in the last bits, and so do the gradients' rounding errors d (up to 1.4e-6 at this shape: fp32
    against fp64 on the CPU oracle).  Adam divides by sqrt(v) + eps, so d moves an update by up to lr * d / (sqrt(v) + eps).  Where a
    gradient IS its rounding error - the ups.*.bias ahead of the batch norms have an exactly zero gradient, 3e-20 in fp64 and up to 4e-8
    in fp32 - eps = 1e-8 turns the noise into updates of +-lr, and any two correct implementations end up O(lr) apart there.  The
    generator then amplifies a parameter difference about 50 to 100 times into the waveform.  Measured with this test:
        lr 2e-3, eps 1e-8: parameters 1.6e-3 apart (0.8 lr)
        lr 2e-3, eps 1e-4: parameters 2.7e-5 apart (lr * d / eps = 2.8e-5), waveforms 1.1e-3 apart; moved by 5.9e-3 / 0.54
    With lr = 2e-4 and eps = 1e-3 the same estimate gives lr * d / eps = 2.8e-7 on the parameters and a few 1e-5 on the waveforms,
    inside the bar, while parameters with |g| >> eps (conv_post.bias: 0.25) still move by lr per step - 6e-4, six times the bar, so an
    optimizer that did nothing, or stepped the wrong way, fails.  The step at eps = 1e-8 is checked per entry by the two tests above."""
    from wavthruvec_pytorch_amd import Generator
    h = synthetic.make_hparams(num_wv_feat=768)
    sd = synthetic.make_state_dict(h, seed=0)
    inp = tuple(x.to(dev) for x in synthetic.make_inputs(h, 2, 8, seed=31))
    outs = []
    for cls, extra in ((AdamW, {}), (torch.optim.AdamW, dict(foreach=False))):
        g = Generator(h)
        g.load_state_dict(sd)
        g = g.to(dev).train()
        opt = cls(g.parameters(), 2e-4, betas=(0.8, 0.99), eps=1e-3, **extra)
        ys = []
        for _ in range(3):
            opt.zero_grad()
            y = g(*inp)
            y.square().mean().backward()
            opt.step()
            ys.append(y.detach())
        with torch.no_grad():
            ys.append(g(*inp))
        outs.append((ys, [p.detach().clone() for p in g.parameters()]))
    (ya, pa), (yb, pb) = outs
    dy = max((a - b).abs().max().item() for a, b in zip(ya, yb))
    dp = max((a - b).abs().max().item() for a, b in zip(pa, pb))
    moved_y = (ya[-1] - ya[0]).abs().max().item()
    moved_p = max((a - v.to(dev)).abs().max().item() for a, v in zip(pa, (sd[k] for k, _ in Generator(h).named_parameters())))
    print(f'waveforms {dy:.3e} parameters {dp:.3e} apart; three steps moved them by {moved_y:.3e} / {moved_p:.3e}')
    assert dy <= TOL
    assert dp <= TOL
    assert moved_y > 10 * TOL and moved_p > 3 * TOL          # three steps moved both beyond the bar


def test_frozen_discriminators_are_skipped(dev):
    """`with frozen(mpd, msd):` around the generator step's discriminator forwards leaves their parameters without gradients: the optimizer
    skips them (no state, no launch for them) and steps what has a gradient."""
    from types import SimpleNamespace
    from wavthruvec_pytorch_amd.discriminators import MultiPeriodDiscriminator, MultiScaleDiscriminator, frozen
    mpd = MultiPeriodDiscriminator(SimpleNamespace(periods=synthetic.DEFAULT_PERIODS))
    mpd.load_state_dict(synthetic.make_disc_state_dict(synthetic.mpd_state_dict_spec(), seed=17))
    msd = MultiScaleDiscriminator()
    msd.load_state_dict(synthetic.make_disc_state_dict(synthetic.msd_state_dict_spec(), seed=17))
    mpd, msd = mpd.to(dev).train(), msd.to(dev).train()
    y, y_hat = (x.to(dev) for x in synthetic.make_audio_pair(2, 2100, seed=12))
    yh = y_hat.clone().requires_grad_(True)                  # stands for the generator's output: the one tensor that does get a gradient
    dparams = list(mpd.parameters()) + list(msd.parameters())
    opt = AdamW([dict(params=dparams), dict(params=[yh])], 1e-2, betas=(0.8, 0.99))
    before = [p.detach().clone() for p in dparams]
    with frozen(mpd, msd):
        loss = D.smooth_loss(mpd(y, yh)) + D.smooth_loss(msd(y, yh))
    loss.backward()
    assert all(p.grad is None for p in dparams) and yh.grad is not None
    opt.step()
    torch.cuda.synchronize()
    assert all(torch.equal(a, p) for a, p in zip(before, dparams)) and all(p not in opt.state for p in dparams)
    assert float(opt.state[yh]['step']) == 1 and not torch.equal(yh.detach(), y_hat)
