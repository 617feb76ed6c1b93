"""GPU tests of the global-norm clip and the non-finite guard: the sum of squares and the norm against fp64 of the same fp32 data at the
bound the header derives (tests/clip_ref.py), determinism and what the launches leave alone, optim.clip_grad_norm_ against the fp64
restatement, the clipped AdamW step per entry, a non-finite gradient with and without skip_nonfinite, and AdamW(max_grad_norm) on the
generator's own gradients against clip_grad_norm_ + AdamW in fp64 on the CPU."""
import math

import numpy as np
import pytest
import torch

from tests import clip_ref as K
from tests import optim_ref as R
from wavthruvec_pytorch_amd import AdamW, _hip, clip_grad_norm_, hipops, synthetic

pytestmark = pytest.mark.gpu
TOL = 1e-4
PAD = 32
SENTINEL = 12345.678
M = _hip.ADAMW_MAX_ITEMS
NUMELS = (1, 3, 255, 257, 8191, 8193, 300_001)
VIEWS = ((257, 1), (8193, 2), (1029, 3))                 # (numel, floats past a 16-byte line)


@pytest.fixture(scope='module')
def dev():
    _hip.load()
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def _guarded(values, phase, dev):
    """(buffer, view): `values` placed `phase` floats past a 16-byte line inside a buffer whose other floats hold the sentinel."""
    n = values.size
    buf = torch.full((PAD + n + PAD + 4,), SENTINEL, device=dev)
    assert buf.data_ptr() % 16 == 0
    view = buf[PAD + phase:PAD + phase + n]
    view.copy_(torch.from_numpy(values))
    assert view.data_ptr() % 16 == 4 * phase
    return buf, view


def _borders_intact(buf, view):
    off = (view.data_ptr() - buf.data_ptr()) // 4
    return bool((buf[:off] == SENTINEL).all()) and bool((buf[off + view.numel():] == SENTINEL).all())


def _shapes(count):
    shapes = [(n, 0) for n in NUMELS] + list(VIEWS)
    return shapes + [(2 + i % 7, 0) for i in range(count - len(shapes))]


def _gradients(count, dev, seed, mixed=True):
    """[(numpy fp32 values, phase, guard buffer, GPU view)]: N(0, 1) times 1e-6, 1 or 1e6 per tensor when `mixed`."""
    rng = np.random.default_rng(seed)
    rows = []
    for i, (n, ph) in enumerate(_shapes(count)):
        x = (rng.standard_normal(n) * ((1e-6, 1.0, 1e6)[i % 3] if mixed else 1.0)).astype(np.float32)
        rows.append((x, ph) + _guarded(x, ph, dev))
    return rows


def _expected_partials(rows):
    """(fp64 sum of squares of every workgroup's own elements, the largest chunk of the calls) from the restated plan, call by call."""
    sums, chunk = [], 0
    for i0 in range(0, len(rows), M):
        part = rows[i0:i0 + M]
        starts, ch = K.plan([r[0].size for r in part], [r[1] for r in part])
        chunk = max(chunk, ch)
        for (x, ph, _b, _v), a, b in zip(part, starts, starts[1:]):
            sums += [float((x[e0:e1].astype(np.float64) ** 2).sum()) for e0, e1 in K.spans(x.size, ph, b - a)]
    return np.array(sums), chunk


@pytest.mark.parametrize('count', [10, M + 1, 2 * M + 1])
def test_norm_against_fp64_of_the_same_data(dev, count):
    """10, 81 and 161 tensors: one, two and three launches into one partials buffer.  Every partial against the fp64 sum over its own
    chunk at 2 (T + 10) u, the norm at 2 ((T + 10) / 2 + 1) u, the coefficient at one rounding more; T = 32 at these sizes."""
    rows = _gradients(count, dev, seed=count)
    views = [r[3] for r in rows]
    want, chunk = _expected_partials(rows)
    assert chunk == 2048 and K.sumsq_roundings(chunk) == 42
    n = hipops.grad_sumsq_partials(views)
    assert n == want.size > count
    buf = torch.full((n + 8,), SENTINEL, device=dev)
    got, cnt = hipops.grad_sumsq_multi(views, buf)
    assert cnt == n and got is buf
    first = buf.clone()
    hipops.grad_sumsq_multi(views, buf)
    assert torch.equal(first, buf)                                             # the same call gives the same bits
    assert bool((buf[n:] == SENTINEL).all())                                   # nothing past the used range is written
    assert all(_borders_intact(b, v) and np.array_equal(v.cpu().numpy(), x) for x, _ph, b, v in rows)
    parts = buf[:n].cpu().numpy().astype(np.float64)
    assert (want > 0).all()                                                    # no workgroup of these sizes is empty
    ratio = np.abs(parts - want) / (2 * K.sumsq_roundings(chunk) * R.U32 * want)
    exact = K.total_norm([r[0] for r in rows])
    out = torch.tensor([7.0, 7.0, 7.0, 3.0], device=dev)
    assert hipops.grad_norm_finish(buf, n, float('inf'), out) is out
    o = out.cpu().numpy().astype(np.float64)
    rn = abs(o[0] - exact) / (2 * K.norm_roundings(chunk) * R.U32 * exact)
    print(f'{count} tensors, {n} partials: worst partial / bound {ratio.max():.3f}, norm / bound {rn:.3f}')
    assert ratio.max() <= 1.0 and rn <= 1.0
    assert o[1] == 1.0 and o[2] == 1.0 and o[3] == 3.0                         # norm only; finite: the counter keeps its value
    half = float(np.float32(0.5 * exact))                                      # max_norm travels as an fp32
    out2 = hipops.grad_norm_finish(buf, n, half)
    o2 = out2.cpu().numpy().astype(np.float64)
    want_c = K.clip_coef(exact, half)
    assert o2[0] == o[0] and abs(o2[1] - want_c) <= 2 * (K.norm_roundings(chunk) + 1) * R.U32 * want_c and o2[2] == 1.0 and o2[3] == 0.0
    assert hipops.grad_norm_finish(buf, n, 0.0).cpu().tolist()[1] == 0.0


def _ulps(got, want):
    """|got - want| in units of the fp32 spacing at |want| (want: float64)."""
    return np.abs(got.astype(np.float64) - want) / np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)


def test_stand_alone_clip(dev):
    rows = _gradients(M + 3, dev, seed=2, mixed=False)
    params = []
    for x, _ph, _b, v in rows + [(None, 0, None, None)]:
        p = torch.zeros(v.shape if v is not None else (5,), device=dev, requires_grad=True)
        p.grad = v                                                             # the last parameter has no gradient: skipped
        params.append(p)
    grads = [r[0] for r in rows]
    views = [r[3] for r in rows]
    exact = K.total_norm(grads)
    low = hipops.grad_norm_finish(*hipops.grad_sumsq_multi(views), float('inf'))[0].clone()
    # below max_norm: the coefficient is exactly 1 and no bit moves
    got = clip_grad_norm_(params, 2.0 * exact)
    assert got.shape == () and got.is_cuda and torch.equal(got, low)
    assert all(np.array_equal(v.cpu().numpy(), x) and _borders_intact(b, v) for x, _ph, b, v in rows)
    assert clip_grad_norm_(params[3], 2.0 * exact).item() > 0                  # a single tensor, as torch takes it
    # above: against the fp64 restatement
    half = float(np.float32(0.5 * exact))                                      # max_norm travels as an fp32
    _n, coef, scaled = K.clip_ref(grads, half)
    assert 0.49 < coef < 0.51
    got = clip_grad_norm_(params, half, error_if_nonfinite=True)
    assert torch.equal(got, low) and abs(got.item() - exact) <= 2 * K.norm_roundings(2048) * R.U32 * exact
    worst = max(float(_ulps(v.cpu().numpy(), s).max()) for (_x, _ph, _b, v), s in zip(rows, scaled))
    print(f'clipped gradients: worst {worst:.3f} ulp from the fp64 restatement')
    assert worst <= 2.0
    assert all(_borders_intact(b, v) for _x, _ph, b, v in rows) and params[-1].grad is None


def _state_rows(dev, seed):
    """Random (p, g, m, v) of M + 3 tensors: the sizes of _shapes, with a view on p only, on g only and on all four among them."""
    rng = np.random.default_rng(seed)
    rows = []
    for i, (n, ph) in enumerate(_shapes(M + 3)):                               # (three workgroups in place of the 300 001)
        n = n if n != 300_001 else 2 * 2048 * 4 + 5
        phases = {7: (1, 0, 0, 0), 8: (0, 1, 0, 0)}.get(i, (ph,) * 4)
        vals = R.kernel_state(n, rng)
        rows.append((vals, [_guarded(x, k, dev) for x, k in zip(vals, phases)]))
    return rows


def _lists(rows):
    return tuple([r[1][k][1] for r in rows] for k in range(4))


HYPER = dict(lr=1e-2, betas=(0.8, 0.99), eps=1e-6)


@pytest.mark.parametrize('wd', [0.0, 0.01])
@pytest.mark.parametrize('t', [1, 2, 1000])
def test_clipped_step_matches_the_fp64_restatement_per_entry(dev, t, wd):
    """adamw_multi_clipped from a GIVEN fp32 coefficient against the restatement at that coefficient: 2 x (4 / 6 / 18) roundings."""
    assert K.step_roundings(1) == {'m': 4, 'v': 6, 'p': 18}
    rows = _state_rows(dev, seed=100 + t)
    coef = np.float32(0.3712)
    clip = torch.tensor([1.0, float(coef), 1.0, 0.0], device=dev)
    assert hipops.adamw_multi_clipped(*_lists(rows), clip, weight_decay=wd, step=t, **HYPER) == 2
    torch.cuda.synchronize()
    h = R.make_hyper(step=t, weight_decay=wd, **HYPER)
    worst = 0.0
    for (p, g, m, v), bufs in rows:
        assert all(_borders_intact(*b) for b in bufs)
        assert np.array_equal(bufs[1][1].cpu().numpy(), g)                     # the gradient is only read
        got = tuple(bufs[k][1].cpu().numpy() for k in (0, 2, 3))
        rp, rm, rv, mags = K.clipped_adamw_ref(p, g, m, v, h, coef)
        ratio = R.worst_ratio(got, (rp, rm, rv), K.step_bounds(mags, 1))
        worst = max(worst, ratio)
        assert ratio <= 1.0, (p.size, ratio)
        assert not np.array_equal(got[0], p) or p.size < 4
    print(f't={t} wd={wd}: worst |delta| / bound = {worst:.3f}')
    assert clip.cpu().tolist() == [1.0, float(coef), 1.0, 0.0]


def test_coefficient_one_gives_the_bits_of_the_plain_step_and_a_skipped_step_writes_nothing(dev):
    a, b, c = (_state_rows(dev, seed=7) for _ in range(3))
    kw = dict(weight_decay=0.01, step=3, **HYPER)
    hipops.adamw_multi(*_lists(a), **kw)
    parts, n = hipops.grad_sumsq_multi(_lists(b)[1])
    clip = hipops.grad_norm_finish(parts, n, float('inf'))                     # the route optim.AdamW(skip_nonfinite=True) takes
    hipops.adamw_multi_clipped(*_lists(b), clip, skip_nonfinite=True, **kw)
    assert clip.cpu().tolist()[1:] == [1.0, 1.0, 0.0]
    for (_va, ba), (_vb, bb) in zip(a, b):
        assert all(torch.equal(x[0], y[0]) for x, y in zip(ba, bb))            # whole buffers: values and guards
    # the flag says non-finite: with skip_nonfinite nothing is written, without it the step is taken
    bad = torch.tensor([float('inf'), 0.5, 0.0, 1.0], device=dev)
    hipops.adamw_multi_clipped(*_lists(c), bad, skip_nonfinite=True, **kw)
    for (vals, bufs) in c:
        assert all(np.array_equal(bufs[k][1].cpu().numpy(), vals[k]) and _borders_intact(*bufs[k]) for k in range(4))
    hipops.adamw_multi_clipped(*_lists(c), bad, skip_nonfinite=False, **kw)
    assert all(not np.array_equal(bufs[2][1].cpu().numpy(), vals[2]) for vals, bufs in c)


def _ninety(dev, seed=4):
    gen = torch.Generator(device=dev).manual_seed(seed)
    ps = [torch.randn(5000 if i == 40 else 2 + i % 7, device=dev, generator=gen).requires_grad_() for i in range(90)]
    for p in ps:
        p.grad = torch.randn(p.shape, device=dev, generator=gen)
    return ps


def _snapshot(opt, ps):
    return [tuple(x.detach().clone() for x in (p, opt.state[p]['exp_avg'], opt.state[p]['exp_avg_sq'])) if p in opt.state
            else (p.detach().clone(),) for p in ps]


def test_a_non_finite_gradient_is_skipped_counted_and_reported(dev):
    """One inf, then one NaN, in one gradient of 90 (ordinary data: nothing here faults)."""
    ps = _ninety(dev)
    opt = AdamW(ps, 1e-2, betas=(0.8, 0.99), max_grad_norm=1.0, skip_nonfinite=True)
    opt.step()                                                                 # a finite step first: the moments are not zero
    assert opt.nonfinite_steps() == 0 and math.isfinite(opt.grad_norm.item()) and opt.grad_norm.shape == () and opt.grad_norm.is_cuda
    for count, bad in ((1, float('inf')), (2, float('nan'))):
        ps[17].grad[1] = bad
        before = _snapshot(opt, ps)
        opt.step()
        assert not math.isfinite(opt.grad_norm.item())
        assert opt.nonfinite_steps() == count
        assert all(torch.equal(x, y) for b, a in zip(before, _snapshot(opt, ps)) for x, y in zip(b, a))
    ps[17].grad[1] = 0.25
    before = _snapshot(opt, ps)
    opt.step()
    assert opt.nonfinite_steps() == 2 and math.isfinite(opt.grad_norm.item())
    assert all(not torch.equal(b[0], a[0]) for b, a in zip(before, _snapshot(opt, ps)))
    assert all(float(opt.state[p]['step']) == 4 for p in ps)                   # the CPU counters count the skipped steps too
    # skip_nonfinite alone: the norm with max_norm = inf, coefficient 1 - the plain step's bits on finite gradients
    qs, rs = _ninety(dev, seed=9), _ninety(dev, seed=9)
    guarded, plain = AdamW(qs, 1e-2, skip_nonfinite=True), AdamW(rs, 1e-2)
    guarded.step(), plain.step()
    assert all(torch.equal(q, r) for q, r in zip(qs, rs)) and guarded.nonfinite_steps() == 0
    qs[3].grad[0] = float('nan')
    before = _snapshot(guarded, qs)
    guarded.step()
    assert guarded.nonfinite_steps() == 1 and all(torch.equal(x, y) for b, a in zip(before, _snapshot(guarded, qs)) for x, y in zip(b, a))


@pytest.mark.parametrize('bad', [float('inf'), float('nan')])
def test_without_skip_a_non_finite_norm_propagates_as_under_torch(dev, bad):
    """torch: norm inf -> coefficient 0 -> inf * 0 = NaN in that entry, 0 elsewhere; norm NaN -> every entry NaN."""
    ps, qs, rs = _ninety(dev), _ninety(dev), _ninety(dev)
    for x in (ps, qs, rs):
        x[17].grad[1] = bad
    # the stand-alone clip against torch's on the same gradients
    ours, theirs = clip_grad_norm_(ps, 1.0), torch.nn.utils.clip_grad_norm_(qs, 1.0)
    assert not math.isfinite(ours.item()) and (math.isnan(ours.item()) == math.isnan(theirs.item()))
    for p, q in zip(ps, qs):
        assert torch.equal(torch.isnan(p.grad), torch.isnan(q.grad))
        assert torch.equal(torch.nan_to_num(p.grad, nan=3.0), torch.nan_to_num(q.grad, nan=3.0))
    assert int(sum(torch.isnan(p.grad).sum() for p in ps)) == (1 if bad == float('inf') else sum(p.numel() for p in ps))
    with pytest.raises(RuntimeError, match='non-finite'):
        clip_grad_norm_(rs, 1.0, error_if_nonfinite=True)
    assert rs[17].grad[0].item() == _ninety(dev)[17].grad[0].item()            # refused before anything was scaled
    # the fused step on the unscaled gradients against torch's step on the gradients torch clipped
    kw = dict(lr=1e-2, betas=(0.8, 0.99), eps=1e-6, weight_decay=0.01)
    start = [r.detach().cpu().numpy().copy() for r in rs]
    fused, ref = AdamW(rs, max_grad_norm=1.0, **kw), torch.optim.AdamW(qs, foreach=False, **kw)
    fused.step(), ref.step()
    assert fused.nonfinite_steps() == 1 and not math.isfinite(fused.grad_norm.item())
    h = R.make_hyper(step=1, **kw)
    for r, q, p0 in zip(rs, qs, start):
        nan = torch.isnan(q.detach())
        assert torch.equal(torch.isnan(r.detach()), nan)
        for name in ('exp_avg', 'exp_avg_sq'):
            assert torch.equal(torch.isnan(fused.state[r][name]), torch.isnan(ref.state[q][name]))
        if bad == float('inf'):                                                # the finite entries stepped on g * 0
            z = np.zeros(p0.shape)
            rp, rm, rv, mags = K.clipped_adamw_ref(p0, z, z, z, h, 0.0)
            keep = ~nan.cpu().numpy()
            got = (r.detach().cpu().numpy(), fused.state[r]['exp_avg'].cpu().numpy(), fused.state[r]['exp_avg_sq'].cpu().numpy())
            bnd = K.step_bounds(mags, 1)
            assert R.worst_ratio([x[keep] for x in got], [x[keep] for x in (rp, rm, rv)], {k: b[keep] for k, b in bnd.items()}) <= 1.0


def test_generator_steps_with_max_grad_norm_match_fp64_clip_and_adamw(dev):
    """The B=2, T=8 generator, one forward and backward, AdamW(max_grad_norm = half the measured norm) against
    torch.nn.utils.clip_grad_norm_ + torch.optim.AdamW in fp64 on the CPU from copies of the same gradients.  The hyperparameters are
    exact in fp32 (and so are the bias corrections of step 1), so both sides step with the same constants.  Bound: the coefficient comes
    with (T + 10) / 2 + 2 = 23 roundings at chunk 2048 and g * coef adds one: step_bounds(g_roundings=24).  Then the weight caches (keyed
    on the version counters the step bumps) and a second step against the restatement from the kernel's own state."""
    from wavthruvec_pytorch_amd import Generator
    hp = synthetic.make_hparams(num_wv_feat=768)
    sd = synthetic.make_state_dict(hp, seed=0)
    g = Generator(hp)
    g.load_state_dict(sd)
    g = g.to(dev)
    inp = tuple(x.to(dev) for x in synthetic.make_inputs(hp, 2, 8, seed=31))
    params = list(g.parameters())
    kw = dict(lr=2.0 ** -12, betas=(0.75, 0.984375), eps=2.0 ** -20, weight_decay=2.0 ** -7)
    with torch.no_grad():
        y_before = g.eval()(*inp)                                              # fills the eval-mode fold cache
    g.train()
    g_roundings = 1 + K.norm_roundings(2048) + 1
    assert g_roundings == 24
    opt = None
    m0 = v0 = None
    for t in (1, 2):
        g.zero_grad()
        g(*inp).square().mean().backward()
        params = [p for p in g.parameters() if p.grad is not None]
        assert len(params) >= 100
        p0 = [p.detach().cpu().numpy().astype(np.float64).ravel() for p in params]
        g0 = [p.grad.detach().cpu().numpy().astype(np.float64).ravel() for p in params]
        norm = K.total_norm(g0)
        if opt is None:
            opt = AdamW(g.parameters(), max_grad_norm=float(np.float32(0.5 * norm)), **kw)          # (max_norm travels as an fp32)
            m0, v0 = [np.zeros(x.size) for x in p0], [np.zeros(x.size) for x in p0]
        max_norm = opt.max_grad_norm
        coef = K.clip_coef(norm, max_norm)
        assert coef < (0.51 if t == 1 else 1.0), (t, coef)                     # it clips, at both steps
        versions = [p._version for p in params]
        opt.step()
        assert all(p._version > ver for p, ver in zip(params, versions))
        assert abs(opt.grad_norm.item() - norm) <= 2 * K.norm_roundings(2048) * R.U32 * norm
        assert all(np.array_equal(p.grad.detach().cpu().numpy().ravel(), x.astype(np.float32)) for p, x in zip(params, g0))
        got = [(p.detach().cpu().numpy().ravel(), opt.state[p]['exp_avg'].cpu().numpy().ravel(), opt.state[p]['exp_avg_sq'].cpu().numpy().ravel())
               for p in params]
        h = R.make_hyper(step=t, **kw)
        if t == 1:
            qs = [torch.from_numpy(x.copy()).requires_grad_() for x in p0]
            for q, x in zip(qs, g0):
                q.grad = torch.from_numpy(x.copy())
            tn = torch.nn.utils.clip_grad_norm_(qs, max_norm, foreach=False)
            assert abs(tn.item() - norm) <= 1e-12 * norm
            ref = torch.optim.AdamW(qs, foreach=False, **kw)
            ref.step()
        worst = 0.0
        for i, (x, gx, mx, vx) in enumerate(zip(p0, g0, m0, v0)):
            rp, rm, rv, mags = K.clipped_adamw_ref(x, gx, mx, vx, h, coef)
            want = (qs[i].detach().numpy(), ref.state[qs[i]]['exp_avg'].numpy(), ref.state[qs[i]]['exp_avg_sq'].numpy()) if t == 1 else (rp, rm, rv)
            worst = max(worst, R.worst_ratio(got[i], want, K.step_bounds(mags, g_roundings)))
        print(f'step {t}: coefficient {coef:.4f}, worst |delta| / bound = {worst:.3f}')
        assert worst <= 1.0, t
        m0, v0 = [x[1].astype(np.float64) for x in got], [x[2].astype(np.float64) for x in got]
        if t == 1:                                                             # a stale fold cache would serve the weights from before the step
            g2 = Generator(hp)
            g2.load_state_dict(g.state_dict())
            with torch.no_grad():
                after, fresh = g.eval()(*inp), g2.to(dev).eval()(*inp)
            g.train()
            assert (after - fresh).abs().max().item() <= TOL and (after - y_before).abs().max().item() > 10 * TOL
    assert opt.nonfinite_steps() == 0
