"""GPU tests of the exponential moving average of the weights: v2w_adamw_ema_multi per entry - p, m, v bit for bit those of the step without
the average, every e' within 3u (|e| + |p'|) of the exact value from the kernel's own stored p' (tests/ema_ref.py) - at every size, phase
and launch boundary; v2w_ema_multi and v2w_swap_multi on the same lists; what a skipped step leaves alone; optim.AdamW(ema_decay) over
five steps against the fp64 restatements and through a state_dict round trip; and swap_ema / ema_state_dict on a small generator, where
the weight caches have to follow the exchange both ways."""
import copy

import numpy as np
import pytest
import torch

from tests import clip_ref as K
from tests import ema_ref as E
from tests import optim_ref as R
from wavthruvec_pytorch_amd import AdamW, Generator, _hip, ema_state_dict, hipops, synthetic

pytestmark = pytest.mark.gpu
PAD = 32            # guard floats on either side of every tensor a kernel writes
SENTINEL = 12345.678
M = _hip.ADAMW_EMA_MAX_ITEMS
# 8192 floats are one workgroup's minimum chunk (2048 units): the last size spans three workgroups and ends off a 16-byte line
SIZES = (1, 3, 4, 5, 1023, 8192, 2 * 8192 + 5)
# (numel, phases of p, g, m, v, e in floats past a 16-byte line): e alone off the others' phase (float by float), all five alike (16-byte
# accesses behind a partial first unit)
PHASED = ((1029, (0, 0, 0, 0, 1)), (1030, (1, 1, 1, 1, 1)), (8192 + 6, (3, 3, 3, 3, 3)))
HYPER = dict(lr=1e-2, betas=(0.8, 0.99), eps=1e-6, weight_decay=0.1)
COEF = np.float32(0.3712)


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


def _shapes():
    return [(n, (0,) * 5) for n in SIZES] + list(PHASED)


def _values(shapes, seed):
    """[(p, g, m, v, e)] in numpy fp32 at the scales of tests/optim_ref.py; the average is drawn like the parameter."""
    rng = np.random.default_rng(seed)
    return [R.kernel_state(n, rng) + (R.kernel_state(n, rng)[0],) for n, _ph in shapes]


def _on_gpu(shapes, values, dev):
    """[[(buffer, view) of p, g, m, v, e]] - fresh guarded copies of the same values."""
    return [[_guarded(x, k, dev) for x, k in zip(vals, ph)] for (_n, ph), vals in zip(shapes, values)]


def _lists(rows, which=range(5)):
    return tuple([r[k][1] for r in rows] for k in which)


def _check_step(shapes, dev, seed, clip, decay, launches):
    """One step with the average against the same step without it on copies of the same values.  Returns the worst |e' - exact| / bound."""
    values = _values(shapes, seed)
    a, b = _on_gpu(shapes, values, dev), _on_gpu(shapes, values, dev)
    kw = dict(step=3, **HYPER)
    clip_t = torch.tensor([1.0, float(COEF), 1.0, 0.0], device=dev) if clip else None
    if clip:
        hipops.adamw_multi_clipped(*_lists(a, range(4)), clip_t, **kw)
    else:
        hipops.adamw_multi(*_lists(a, range(4)), **kw)
    assert hipops.adamw_ema_multi(*_lists(b), clip_t, ema_decay=decay, **kw) == launches
    torch.cuda.synchronize()
    omd = E.omd32(decay)
    worst = 0.0
    for (n, ph), vals, ra, rb in zip(shapes, values, a, b):
        for k in range(4):                                                     # whole buffers: p', m', v' and g bit for bit, guards included
            assert torch.equal(ra[k][0], rb[k][0]), (n, ph, 'pgmv'[k])
        assert np.array_equal(rb[1][1].cpu().numpy(), vals[1])                 # the gradient is only read
        assert _borders_intact(*rb[4]) and _borders_intact(*ra[4]), (n, ph)
        assert np.array_equal(ra[4][1].cpu().numpy(), vals[4])                 # the step without the average never saw e
        p_new, e_new = rb[0][1].cpu().numpy(), rb[4][1].cpu().numpy()
        assert not np.array_equal(p_new, vals[0]) or n < 4                     # the step did move the parameter
        ratio = E.worst_ratio(e_new, E.ema_exact(vals[4], p_new, omd), E.ema_bound(vals[4], p_new))
        assert ratio <= 1.0, (n, ph, ratio)
        if float(omd) > 0.0:
            assert not np.array_equal(e_new, vals[4]) or n < 4                 # and the average
        worst = max(worst, ratio)
    if clip:
        assert clip_t.cpu().tolist() == [1.0, float(COEF), 1.0, 0.0]
    return worst


@pytest.mark.parametrize('decay', [0.999, 0.37])
@pytest.mark.parametrize('clip', [False, True])
def test_step_with_average_per_entry_at_every_size_and_phase(dev, clip, decay):
    worst = _check_step(_shapes(), dev, seed=11, clip=clip, decay=decay, launches=1)
    print(f'clip={clip} decay={decay}: worst |e\' - exact| / bound = {worst:.3f}')


@pytest.mark.parametrize('clip', [False, True])
@pytest.mark.parametrize('count', [1, M, M + 1])
def test_launch_boundary(dev, count, clip):
    """1, 64 and 65 tensors: 65 is two launches of hipops.adamw_ema_multi, the second of one item."""
    assert M == 64
    shapes = [(2 + i % 7 if i else 5, (0,) * 5) for i in range(count)]
    if count > 2:
        shapes[-1] = (8192 + 3, (2,) * 5)                                      # the last tensor (alone in its launch at 65) has two workgroups
    _check_step(shapes, dev, seed=count, clip=clip, decay=0.99, launches=-(-count // M))


def test_decay_one_leaves_every_bit_of_the_average(dev):
    """ema_omd == 0 (decay 1.0 is served at the hipops level): fma(0, p' - e, e) = e for finite inputs."""
    shapes = _shapes()
    values = _values(shapes, 5)
    rows = _on_gpu(shapes, values, dev)
    before = [r[4][0].clone() for r in rows]
    hipops.adamw_ema_multi(*_lists(rows), ema_decay=1.0, step=1, **HYPER)
    assert all(torch.equal(r[4][0], b) for r, b in zip(rows, before))
    assert all(not torch.equal(r[0][1], torch.from_numpy(v[0]).to(dev)) or v[0].size < 4 for r, v in zip(rows, values))
    hipops.ema_multi(*_lists(rows, (0, 4)), ema_decay=1.0)
    assert all(torch.equal(r[4][0], b) for r, b in zip(rows, before))


PAIR_SHAPES = [(n, (0, 0)) for n in SIZES] + [(1029, (0, 1)), (1030, (1, 1)), (8192 + 6, (3, 3))]


def _pair_rows(dev, seed, extra=0):
    rng = np.random.default_rng(seed)
    shapes = PAIR_SHAPES + [(2 + i % 7, (0, 0)) for i in range(extra)]
    values = [(R.kernel_state(n, rng)[0], R.kernel_state(n, rng)[0]) for n, _ph in shapes]
    return shapes, values, [[_guarded(x, k, dev) for x, k in zip(vals, ph)] for (_n, ph), vals in zip(shapes, values)]


@pytest.mark.parametrize('decay', [0.999, 0.0])
def test_average_alone_per_entry(dev, decay):
    """v2w_ema_multi on the same sizes and phases, 81 tensors (two launches): p is only read, e' within the bound of the exact value."""
    extra = _hip.ADAMW_MAX_ITEMS + 1 - len(PAIR_SHAPES)
    shapes, values, rows = _pair_rows(dev, seed=21, extra=extra)
    assert hipops.ema_multi([r[0][1] for r in rows], [r[1][1] for r in rows], ema_decay=decay) == 2
    omd = E.omd32(decay)
    worst = 0.0
    for (n, ph), (p, e), r in zip(shapes, values, rows):
        assert np.array_equal(r[0][1].cpu().numpy(), p) and all(_borders_intact(*x) for x in r), (n, ph)
        got = r[1][1].cpu().numpy()
        ratio = E.worst_ratio(got, E.ema_exact(e, p, omd), E.ema_bound(e, p))
        assert ratio <= 1.0, (n, ph, ratio)
        assert not np.array_equal(got, e) or n < 4
        worst = max(worst, ratio)
    print(f'decay={decay}: worst |e\' - exact| / bound = {worst:.3f}')


def test_swap_is_bit_exact_both_ways_and_twice_restores_every_bit(dev):
    extra = _hip.ADAMW_MAX_ITEMS + 1 - len(PAIR_SHAPES)
    shapes, values, rows = _pair_rows(dev, seed=22, extra=extra)
    ps, es = [r[0][1] for r in rows], [r[1][1] for r in rows]
    before = [(r[0][0].clone(), r[1][0].clone()) for r in rows]
    assert hipops.swap_multi(ps, es) == 2
    for (n, ph), (p, e), r in zip(shapes, values, rows):
        assert np.array_equal(r[0][1].cpu().numpy(), e) and np.array_equal(r[1][1].cpu().numpy(), p), (n, ph)
        assert all(_borders_intact(*x) for x in r), (n, ph)
    hipops.swap_multi(ps, es)
    assert all(torch.equal(r[0][0], b[0]) and torch.equal(r[1][0], b[1]) for r, b in zip(rows, before))
    # NaN payloads and infinities travel as bits too
    odd = torch.tensor([float('nan'), float('inf'), -0.0, 1e-42, -float('inf')], device=dev)
    other = torch.arange(5.0, device=dev)
    bits = odd.view(torch.int32).clone()
    hipops.swap_multi([odd], [other])
    assert torch.equal(other.view(torch.int32), bits) and torch.equal(odd, torch.arange(5.0, device=dev))


def _three(dev, seed):
    gen = torch.Generator(device=dev).manual_seed(seed)
    return [torch.randn(n, device=dev, generator=gen).requires_grad_() for n in (5, 1023, 2 * 8192 + 5)]


def _set_grads(ps, gen, scale=1.0):
    for p in ps:
        p.grad = torch.randn(p.shape, device=p.device, generator=gen) * scale


def _state(opt, ps):
    return [tuple(opt.state[p][k].detach().clone() for k in ('exp_avg', 'exp_avg_sq', 'ema')) + (p.detach().clone(),) for p in ps]


def test_a_skipped_step_moves_neither_the_state_nor_the_average(dev):
    """One inf in one gradient (ordinary data: nothing here faults): with skip_nonfinite every bit of p, m, v and e stays and the step is
    counted; with a finite gradient after it the step proceeds."""
    ps = _three(dev, 1)
    gen = torch.Generator(device=dev).manual_seed(2)
    opt = AdamW(ps, 1e-2, betas=(0.8, 0.99), ema_decay=0.99, skip_nonfinite=True)
    _set_grads(ps, gen)
    opt.step()                                                                 # a finite step first: moments and averages exist and differ from p
    assert opt.nonfinite_steps() == 0
    _set_grads(ps, gen)
    ps[1].grad[17] = float('inf')
    before = _state(opt, ps)
    opt.step()
    assert opt.nonfinite_steps() == 1
    assert all(torch.equal(x, y) for b, a in zip(before, _state(opt, ps)) for x, y in zip(b, a))
    ps[1].grad[17] = 0.25
    opt.step()
    assert opt.nonfinite_steps() == 1
    after = _state(opt, ps)
    assert all(not torch.equal(b[k], a[k]) for b, a in zip(before, after) for k in range(4))
    # the same at the hipops level, the flag handed over as it is: nothing is written, the average included
    shapes = _shapes()
    values = _values(shapes, 9)
    rows = _on_gpu(shapes, values, dev)
    bad = torch.tensor([float('inf'), 0.5, 0.0, 1.0], device=dev)
    hipops.adamw_ema_multi(*_lists(rows), bad, ema_decay=0.5, skip_nonfinite=True, step=2, **HYPER)
    assert all(np.array_equal(r[k][1].cpu().numpy(), v[k]) and _borders_intact(*r[k]) for r, v in zip(rows, values) for k in range(5))
    hipops.adamw_ema_multi(*_lists(rows), bad, ema_decay=0.5, skip_nonfinite=False, step=2, **HYPER)
    assert all(not np.array_equal(r[4][1].cpu().numpy(), v[4]) for r, v in zip(rows, values))


def _np(t):
    return t.detach().cpu().numpy().astype(np.float64).ravel()


def test_five_optimizer_steps_against_fp64_and_through_a_state_dict(dev):
    """AdamW(ema_decay=0.99, max_grad_norm=1.0) on three tensors, N(0, 1) gradients (the norm is about 130: every step clips).  Each step
    from the kernel's own previous state: p, m, v against clip_ref at an exactly computed coefficient (the coefficient comes with
    (T + 10) / 2 + 2 = 23 roundings at chunk 2048 and g * coef adds one: step_bounds(g_roundings=24), as in tests/test_clip_gpu.py), e
    against ema_ref from the stored p'.  Over the five steps e against the closed form of the stored parameters at the sum of the
    per-step bounds (an error made at step t reaches e_T times d^(T-t) <= 1).  After step 3 the state_dict goes into a fresh optimizer on
    copies of the parameters: both continue with identical bits."""
    kw = dict(lr=2.0 ** -7, betas=(0.75, 0.984375), eps=2.0 ** -20, weight_decay=2.0 ** -7)          # exact in fp32
    decay = 0.99
    omd = E.omd32(decay)
    ps = _three(dev, 3)
    opt = AdamW(ps, ema_decay=decay, max_grad_norm=1.0, **kw)
    gen = torch.Generator(device=dev).manual_seed(4)
    g_roundings = 1 + K.norm_roundings(2048) + 1
    assert g_roundings == 24
    e_start = [_np(p) for p in ps]                                             # the average starts as a clone of p before the first update
    stored, acc = [[] for _ in ps], [0.0 for _ in ps]
    twin = None
    worst = worst_e = 0.0
    for t in range(1, 6):
        _set_grads(ps, gen)
        if twin is not None:
            for q, p in zip(twin[0], ps):
                q.grad = p.grad.clone()
        p0, g0 = [_np(p) for p in ps], [_np(p.grad) for p in ps]
        if t == 1:
            m0, v0, e0 = [np.zeros(x.size) for x in p0], [np.zeros(x.size) for x in p0], list(e_start)
        coef = K.clip_coef(K.total_norm(g0), 1.0)
        assert coef < 0.02
        opt.step()
        if twin is not None:
            twin[1].step()
        h = R.make_hyper(step=t, **kw)
        for i, p in enumerate(ps):
            st = opt.state[p]
            got = (_np(p), _np(st['exp_avg']), _np(st['exp_avg_sq']))
            rp, rm, rv, mags = K.clipped_adamw_ref(p0[i], g0[i], m0[i], v0[i], h, coef)
            worst = max(worst, R.worst_ratio(got, (rp, rm, rv), K.step_bounds(mags, g_roundings)))
            e_new = _np(st['ema'])
            bnd = E.ema_bound(e0[i], got[0])
            worst_e = max(worst_e, E.worst_ratio(e_new, E.ema_exact(e0[i], got[0], omd), bnd))
            stored[i].append(got[0])
            acc[i] = acc[i] + bnd
            m0[i], v0[i], e0[i] = got[1], got[2], e_new
            assert st['ema'].shape == p.shape and st['ema'].is_cuda
        assert worst <= 1.0 and worst_e <= 1.0, (t, worst, worst_e)
        if t == 3:
            sd = copy.deepcopy(opt.state_dict())
            assert all(list(s) == ['step', 'exp_avg', 'exp_avg_sq', 'ema'] for s in sd['state'].values())
            qs = [p.detach().clone().requires_grad_() for p in ps]
            fresh = AdamW(qs, ema_decay=decay, max_grad_norm=1.0, **kw)
            fresh.load_state_dict(sd)
            twin = (qs, fresh)
    print(f'five steps: worst step / bound {worst:.3f}, worst average / bound {worst_e:.3f}')
    for i in range(len(ps)):
        want = E.ema_closed_form(e_start[i], stored[i], omd)
        assert E.worst_ratio(e0[i], want, acc[i]) <= 1.0
        assert np.abs(e0[i] - stored[i][-1]).max() > 100 * acc[i].max()       # the average is not the parameter
    qs, fresh = twin
    assert [len(x) for x in (fresh.ema_parameters(), opt.ema_parameters())] == [3, 3]
    for p, q in zip(ps, qs):
        assert torch.equal(p.detach(), q.detach()) and float(fresh.state[q]['step']) == 5
        assert all(torch.equal(opt.state[p][k], fresh.state[q][k]) for k in ('exp_avg', 'exp_avg_sq', 'ema'))
    # a loaded state without an average starts it from the current parameter
    sd = copy.deepcopy(opt.state_dict())
    for s in sd['state'].values():
        del s['ema']
    rs = [p.detach().clone().requires_grad_() for p in ps]
    late = AdamW(rs, ema_decay=decay, max_grad_norm=1.0, **kw)
    late.load_state_dict(sd)
    assert late.ema_parameters() == []
    for r, p in zip(rs, ps):
        r.grad = p.grad.clone()
    r0 = [_np(r) for r in rs]
    late.step()
    for r, x in zip(rs, r0):
        got = _np(r)
        assert E.worst_ratio(_np(late.state[r]['ema']), E.ema_exact(x, got, omd), E.ema_bound(x, got)) <= 1.0


def test_swap_ema_and_the_averaged_checkpoint_on_a_small_generator(dev):
    """Two training-mode steps on synthetic gradients, then eval: the forward inside swap_ema() is bit for bit the forward of a second
    generator loaded from ema_state_dict (same weights, folds and launches), and the forward after the context is bit for bit the one
    before it - the fold / pack caches followed the exchange both ways, though no storage pointer moved."""
    hp = synthetic.make_hparams(num_wv_feat=64)
    g = Generator(hp)
    g.load_state_dict(synthetic.make_state_dict(hp, seed=0))
    g = g.to(dev).train()
    inp = tuple(x.to(dev) for x in synthetic.make_inputs(hp, 2, 8, seed=31))
    params = list(g.parameters())
    opt = AdamW(params, 1e-2, betas=(0.8, 0.99), ema_decay=0.5)
    gen = torch.Generator(device=dev).manual_seed(6)
    for _ in range(2):
        _set_grads(params, gen, scale=1e-2)
        opt.step()
    pairs = opt.ema_parameters()
    assert [p for p, _e in pairs] == params and all(not torch.equal(p.detach(), e) for p, e in pairs if p.numel() > 4)
    g.eval()
    sd = ema_state_dict(opt, g)
    assert list(sd) == list(g.state_dict())
    g2 = Generator(hp)
    g2.load_state_dict(sd)
    g2 = g2.to(dev).eval()
    ptrs = [(p.data_ptr(), e.data_ptr()) for p, e in pairs]
    weights = [p.detach().clone() for p in params]
    with torch.no_grad():
        before = g(*inp)                                                       # fills the eval-mode caches with the weights
        versions = [p._version for p in params]
        with opt.swap_ema() as same:
            assert same is opt and all(p._version > v for p, v in zip(params, versions))
            assert all(torch.equal(e, w) for (_p, e), w in zip(pairs, weights))           # the weights wait in the state
            inside = g(*inp)
            with pytest.raises(RuntimeError, match='re-entrant'):
                with opt.swap_ema():
                    pass
            with pytest.raises(RuntimeError, match='swap_ema'):
                opt.step()
            assert all(torch.equal(e, w) for (_p, e), w in zip(pairs, weights))           # the refusals exchanged nothing
        after = g(*inp)
        want = g2(*inp)
    assert torch.equal(inside, want)
    assert torch.equal(after, before)
    assert (inside - before).abs().max().item() > 1e-3                         # the averages are other weights: a stale cache fails above
    assert all(torch.equal(p.detach(), w) for p, w in zip(params, weights))
    assert ptrs == [(p.data_ptr(), e.data_ptr()) for p, e in pairs]
    # an exception inside the context still exchanges back
    with pytest.raises(KeyError):
        with opt.swap_ema():
            raise KeyError('x')
    assert all(torch.equal(p.detach(), w) for p, w in zip(params, weights))
    with torch.no_grad():
        assert torch.equal(g(*inp), before)
    _set_grads(params, gen, scale=1e-2)
    opt.step()                                                                 # and stepping works again
