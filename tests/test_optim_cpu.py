"""CPU tests of the AdamW entry points (v2w_adamw_multi / v2w_adamw_multi_plan) and of optim.AdamW: the C ABI surface, the host-only work
split against a restatement in Python, what the name sink reports, what the entry point refuses, the fp64 restatement (tests/optim_ref.py)
against torch.optim.AdamW, that the kernel tests' bound can see a wrong step, and the class on CPU parameters (torch's own step).  No GPU
needed: nothing is launched."""
import copy
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from tests import optim_ref as R
from wavthruvec_pytorch_amd import AdamW, Generator, _hip, hipops, synthetic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('v2w_adamw_multi_plan', 'v2w_adamw_multi')
FAKE = 0x7f0000100000       # 16-byte aligned "device" pointers: the plan, the dry run and the name sink never dereference them
GAP = 1 << 44               # between the fake p, g, m, v: more than the largest numel the entry point takes (2^42 floats)
DRY = C.c_void_p(-1)        # the dry-run stream: every check of the real call, no launch


def _header():
    return open(os.path.join(ROOT, 'include', 'vec2wav_hip.h')).read()


def _struct_fields(hdr, name):
    body = hdr[:hdr.index('} %s;' % name)]
    body = body[body.rindex('typedef struct {'):]
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    return re.findall(r'\b(\w+)(?:\[\d+\])?\s*[;,]', body)


def _items(numels, phases=None):
    """Descriptor array on fake pointers; phases[i] = (p, g, m, v) offsets in floats past a 16-byte line."""
    arr = (_hip.AdamWItem * max(len(numels), 1))()
    for i, (d, n) in enumerate(zip(arr, numels)):
        ph = phases[i] if phases else (0, 0, 0, 0)
        base = FAKE + i * (1 << 36)
        d.p, d.g, d.m, d.v = (base + k * GAP + 4 * ph[k] for k in range(4))
        d.numel = n
    return arr


def _hyper(**kw):
    args = dict(lr=2e-4, betas=(0.8, 0.99), eps=1e-8, weight_decay=0.01, step=1)
    args.update(kw)
    return hipops.adamw_hyper(**args)


def test_adamw_entry_points_are_declared_bound_and_additive():
    hdr = _header()
    assert int(re.search(r'#define V2W_ABI_VERSION (\d+)', hdr).group(1)) == _hip.ABI_VERSION == 35 == _hip.load().v2w_abi_version()
    for name in NAMES:
        assert name in _hip.SIGNATURES and re.search(r'\b%s\s*\(' % name, hdr), name
    assert 'v2w_adamw_multi' in _hip.LAUNCHERS and 'v2w_adamw_multi_plan' not in _hip.LAUNCHERS
    assert _struct_fields(hdr, 'v2w_adamw_item') == [n for n, _ in _hip.AdamWItem._fields_]
    assert _struct_fields(hdr, 'v2w_adamw_hyper') == [n for n, _ in _hip.AdamWHyper._fields_]
    assert C.sizeof(_hip.AdamWItem) == 40 and C.sizeof(_hip.AdamWHyper) == 32
    assert int(re.search(r'#define V2W_ADAMW_MAX_ITEMS\s+(\d+)', hdr).group(1)) == _hip.ADAMW_MAX_ITEMS >= 64
    assert int(re.search(r'#define V2W_ADAMW_TARGET_WGS\s+(\d+)', hdr).group(1)) == _hip.ADAMW_TARGET_WGS
    # the arithmetic the header states for the by-value table: items + starts + 7 constants + n within the library's 3584 bytes
    assert _hip.ADAMW_MAX_ITEMS * 40 + (_hip.ADAMW_MAX_ITEMS + 1) * 4 + 28 + 4 <= 3584
    # the rounding counts the tests' bound rests on are the ones the header states
    for k, word in (('m', "roundings on m'"), ('v', "roundings on v'"), ('p', "roundings on p'")):
        assert re.search(r'\b%d %s' % (R.ROUNDINGS[k], re.escape(word)), hdr), k
    h = _hyper(step=3)
    r = R.make_hyper(lr=2e-4, betas=(0.8, 0.99), eps=1e-8, weight_decay=0.01, step=3)
    assert all(getattr(h, n) == float(getattr(r, n)) for n, _ in _hip.AdamWHyper._fields_ if n != '_pad')


def _plan_restated(numels, phases=None):
    """include/vec2wav_hip.h, v2w_adamw_multi_plan: units of four floats (cut at p's 16-byte lines when the four pointers share their
    phase), a chunk that deals about ADAMW_TARGET_WGS workgroups, >= 1 per tensor."""
    units = []
    for i, n in enumerate(numels):
        ph = phases[i] if phases else (0, 0, 0, 0)
        units.append((n + (ph[0] if len(set(ph)) == 1 else 0) + 3) // 4)
    chunk = max(2048, -(-sum(units) // _hip.ADAMW_TARGET_WGS))
    starts = [0]
    for u in units:
        starts.append(starts[-1] + max(1, -(-u // chunk)))
    return starts


def _generator_numels():
    g = Generator(synthetic.make_hparams(num_wv_feat=768))
    numels = [p.numel() for p in g.parameters()]
    assert len(numels) == 131 and sum(numels) == 8581602
    return numels


PLAN_CASES = {
    'one_float': ([1], None),
    'mixed': ([1, 37, 4099, 250_000, 2_752_512, 12, 3 * 2048 * 4], None),                    # over four orders of magnitude
    'max_items_tiny': ([5] * _hip.ADAMW_MAX_ITEMS, None),
    'phases': ([4 * 2048 * 3] * 5, [(0, 0, 0, 0), (1, 1, 1, 1), (3, 3, 3, 3), (1, 0, 0, 0), (2, 2, 2, 0)]),
    'huge': ([1 << 33, 7], None),
}


@pytest.mark.parametrize('case', sorted(PLAN_CASES))
def test_plan_matches_its_restatement(case):
    numels, phases = PLAN_CASES[case]
    n = len(numels)
    arr = _items(numels, phases)
    starts = (C.c_int32 * (n + 1))()
    nwg = _hip.load().v2w_adamw_multi_plan(arr, n, starts)
    starts = list(starts)
    assert starts == _plan_restated(numels, phases) and nwg == starts[-1]
    assert starts[0] == 0 and all(b - a >= 1 for a, b in zip(starts, starts[1:]))             # monotone, every tensor has a workgroup
    assert nwg <= _hip.ADAMW_TARGET_WGS + n
    assert hipops.adamw_plan(arr, n) == (starts, nwg)
    if case == 'phases':       # a shared phase adds the floats before the first 16-byte line; a mixed one does not
        assert [b - a for a, b in zip(starts, starts[1:])] == [3, 4, 4, 3, 3]


def test_plan_of_the_generators_parameters_in_chunks():
    numels = _generator_numels()
    launches = 0
    for i0 in range(0, len(numels), _hip.ADAMW_MAX_ITEMS):
        part = numels[i0:i0 + _hip.ADAMW_MAX_ITEMS]
        starts, nwg = hipops.adamw_plan(_items(part), len(part))
        assert starts == _plan_restated(part) and nwg == starts[-1] <= _hip.ADAMW_TARGET_WGS + len(part)
        assert all(b - a >= 1 for a, b in zip(starts, starts[1:]))
        launches += 1
    assert launches == -(-131 // _hip.ADAMW_MAX_ITEMS)


def test_name_sink_lists_the_one_kernel():
    lib = _hip.load()
    arr = _items([1, 4099, 250_000], [(0, 0, 0, 0), (1, 1, 1, 1), (1, 0, 2, 0)])
    rc, names = _hip.kernel_names(lib.v2w_adamw_multi, arr, 3, C.byref(_hyper()))
    assert rc in (0, 100) and names == ['adamw_multi_kernel'], names


def test_entry_point_refuses_bad_arguments_with_an_error_code():
    lib = _hip.load()
    M = _hip.ADAMW_MAX_ITEMS

    def run(arr, n, h):
        rc = lib.v2w_adamw_multi(arr, n, C.byref(h) if h is not None else None, DRY)
        assert _hip.kernel_names(lib.v2w_adamw_multi, arr, n, C.byref(h) if h is not None else None) == (rc, []) or rc == 0
        return rc

    ok = _hyper()
    assert run(_items([7] * M), M, ok) == 0
    assert run(_items([7, 1 << 42]), 2, ok) == 0
    assert run(None, 1, ok) == _hip.E_ARG and run(_items([7]), 1, None) == _hip.E_ARG
    assert run(_items([7] * (M + 1)), M + 1, ok) == _hip.E_ARG and run(_items([7]), 0, ok) == _hip.E_ARG
    for field in ('p', 'g', 'm', 'v'):
        arr = _items([7, 9])
        setattr(arr[1], field, None)
        assert run(arr, 2, ok) == _hip.E_ARG, field
        arr = _items([7, 9])
        setattr(arr[1], field, getattr(arr[1], field) + 2)                  # not 4-byte aligned
        assert run(arr, 2, ok) == _hip.E_ARG, field
        arr = _items([7, 9])
        setattr(arr[1], field, getattr(arr[1], field) + 4)                  # 4-byte aligned is enough
        assert run(arr, 2, ok) == 0, field
    assert run(_items([7, 0]), 2, ok) == _hip.E_ARG and run(_items([-3]), 1, ok) == _hip.E_ARG
    assert run(_items([(1 << 42) + 1]), 1, ok) == _hip.E_SHAPE               # more units than the plan counts
    starts = (C.c_int32 * 3)()
    assert lib.v2w_adamw_multi_plan(_items([(1 << 42) + 1]), 1, starts) == _hip.E_SHAPE
    assert lib.v2w_adamw_multi_plan(_items([7]), 1, None) == _hip.E_ARG
    for kw in (dict(betas=(1.0, 0.99)), dict(betas=(-0.1, 0.99)), dict(betas=(0.8, 1.0)), dict(betas=(0.8, -1e-3)), dict(eps=-1e-8),
               dict(lr=-1e-4), dict(lr=float('nan'))):
        assert run(_items([7]), 1, _hyper(**kw)) == _hip.E_ARG, kw
    for field in ('bias_corr1', 'bias_corr2_sqrt'):
        for bad in (0.0, -0.5):
            h = _hyper()
            setattr(h, field, bad)
            assert run(_items([7]), 1, h) == _hip.E_ARG, (field, bad)
    assert run(_items([7]), 1, _hyper(betas=(0.0, 0.0), lr=0.0, eps=0.0, weight_decay=0.0)) == 0
    # p, m, v of one item overlapping each other (g may alias nothing it is written through)
    for a, b in (('p', 'm'), ('p', 'v'), ('m', 'v')):
        arr = _items([100])
        setattr(arr[0], b, getattr(arr[0], a) + 4 * 99)
        assert run(arr, 1, ok) == _hip.E_ARG, (a, b)
        setattr(arr[0], b, getattr(arr[0], a) + 4 * 100)                     # back to back: no overlap
        assert run(arr, 1, ok) == 0, (a, b)
        setattr(arr[0], b, getattr(arr[0], a) - 4 * 99)
        assert run(arr, 1, ok) == _hip.E_ARG, (a, b)


def test_wrapper_refuses_what_it_cannot_hand_to_the_kernel():
    t = [torch.zeros(4)]
    with pytest.raises(RuntimeError, match='must live on a GPU'):
        hipops.adamw_multi(t, t, t, t, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, step=1)
    with pytest.raises(ValueError):
        hipops.adamw_multi(t, t, t, [], lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, step=1)
    with pytest.raises(ValueError, match='step'):
        hipops.adamw_hyper(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, step=0)
    assert hipops.adamw_multi([], [], [], [], lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, step=1) == 0


@pytest.mark.parametrize('wd', [0.0, 0.01])
def test_restatement_is_pinned_to_torch(wd):
    """Five steps of torch.optim.AdamW(foreach=False) on fp64 CPU tensors under ExponentialLR against optim_ref stepping its own state with
    fp64 hyperparameters.  Either evaluation puts at most ROUNDINGS (15 / 3 / 4) fp64 roundings on an output of ONE step from the same
    state, and the two states are compared after each step and then BOTH continue from torch's: the bound is the kernel tests' with
    u = 2^-53."""
    gen = torch.Generator().manual_seed(3)
    ps = [torch.randn(n, generator=gen, dtype=torch.float64).requires_grad_() for n in (1, 7, 300)]
    opt = torch.optim.AdamW(ps, 2e-3, betas=(0.8, 0.99), eps=1e-8, weight_decay=wd, foreach=False)
    sched = torch.optim.lr_scheduler.ExponentialLR(opt, gamma=0.7)
    lrs = []
    for t in range(1, 6):
        lr = opt.param_groups[0]['lr']
        lrs.append(lr)
        h = R.make_hyper(lr=lr, betas=(0.8, 0.99), eps=1e-8, weight_decay=wd, step=t, dtype=np.float64)
        before = []
        for p in ps:
            p.grad = torch.randn(p.shape, generator=gen, dtype=torch.float64) * 0.3
            st = opt.state[p]
            m = st['exp_avg'].numpy().copy() if st else np.zeros(p.shape)
            v = st['exp_avg_sq'].numpy().copy() if st else np.zeros(p.shape)
            before.append((p.detach().numpy().copy(), p.grad.numpy().copy(), m, v))
        opt.step()
        sched.step()
        for p, (p0, g0, m0, v0) in zip(ps, before):
            rp, rm, rv, mags = R.adamw_ref(p0, g0, m0, v0, h)
            st = opt.state[p]
            got = (p.detach().numpy(), st['exp_avg'].numpy(), st['exp_avg_sq'].numpy())
            assert R.worst_ratio(got, (rp, rm, rv), R.bounds(mags, u=R.U64)) <= 1.0
            assert float(st['step']) == t
    assert len(set(lrs)) == 5                                             # the learning rate did change under the comparison


@pytest.mark.parametrize('t', [1, 3])
@pytest.mark.parametrize('alter', R.ALTERATIONS)
def test_the_bound_can_see_a_wrong_step(alter, t):
    """At the kernel test's own inputs (same seed, sizes and hyperparameters) each deliberately wrong step misses the bound by at least
    100 x somewhere - and the right one, evaluated in fp32 by numpy in the header's order, stays inside it."""
    rng = np.random.default_rng(R.KERNEL_SEED)
    h = R.make_hyper(step=t, **R.KERNEL_HYPER)
    worst = 0.0
    for numel, kind in R.kernel_cases(_hip.ADAMW_MAX_ITEMS):
        p, g, m, v = R.kernel_state(numel, rng)
        want = R.adamw_ref(p, g, m, v, h)
        wrong = R.adamw_ref(p, g, m, v, h, alter=alter)
        worst = max(worst, R.worst_ratio(wrong[:3], want[:3], R.bounds(want[3])))
    assert worst >= 100.0, worst


def test_the_bound_holds_for_the_headers_operations_in_numpy_fp32():
    """The header's operation list evaluated with numpy float32 (fma emulated in float64 and rounded once - exact for these operands' products
    up to double rounding, which the factor two covers) stays inside the bound at the kernel test's inputs: the bound is not too tight for a
    correct kernel."""
    f = np.float32
    rng = np.random.default_rng(R.KERNEL_SEED)
    for t in R.KERNEL_STEPS:
        h = R.make_hyper(step=t, **R.KERNEL_HYPER)
        d = {k: float(getattr(h, k)) for k in vars(h)}
        decay, omb1, omb2 = f(1.0 - d['lr'] * d['weight_decay']), f(1.0 - d['beta1']), f(1.0 - d['beta2'])
        rbc2, step = f(1.0 / d['bias_corr2_sqrt']), f(d['lr'] / d['bias_corr1'])
        fma = lambda a, b, c: (a.astype(np.float64) * np.float64(b) + c.astype(np.float64)).astype(f)      # noqa: E731
        for numel, kind in R.kernel_cases(_hip.ADAMW_MAX_ITEMS)[:10]:
            p, g, m, v = R.kernel_state(numel, rng)
            pd = p * decay
            m1 = fma(g - m, omb1, m)
            v1 = fma(v, h.beta2, omb2 * (g * g))
            den = fma(np.sqrt(v1), rbc2, np.full_like(v1, h.eps))
            p1 = fma(m1 / den, -step, pd)
            rp, rm, rv, mags = R.adamw_ref(p, g, m, v, h)
            assert R.worst_ratio((p1, m1, v1), (rp, rm, rv), R.bounds(mags)) <= 1.0


def _pair(seed=0, cls_kw=None):
    torch.manual_seed(seed)
    ps = [torch.randn(5, 3, requires_grad=True), torch.randn(7, requires_grad=True), torch.randn((), requires_grad=True)]
    qs = [p.detach().clone().requires_grad_() for p in ps]
    kw = dict(lr=1e-2, betas=(0.8, 0.99), weight_decay=0.01)
    kw.update(cls_kw or {})
    return ps, qs, AdamW(ps, **kw), torch.optim.AdamW(qs, **kw)


def _steps(ps, qs, a, b, n, seed):
    gen = torch.Generator().manual_seed(seed)
    for _ in range(n):
        for p, q in zip(ps, qs):
            p.grad = torch.randn(p.shape, generator=gen)
            q.grad = p.grad.clone()
        a.step()
        b.step()


def _same_state(a, b):
    sa, sb = a.state_dict(), b.state_dict()
    assert sa['param_groups'] == sb['param_groups'] and sa['state'].keys() == sb['state'].keys()
    for k in sa['state']:
        assert sa['state'][k].keys() == sb['state'][k].keys()
        for name, val in sa['state'][k].items():
            assert torch.equal(val, sb['state'][k][name]) and val.dtype == sb['state'][k][name].dtype, (k, name)


def test_cpu_parameters_take_torchs_own_step_bit_for_bit():
    ps, qs, a, b = _pair()
    sched = [torch.optim.lr_scheduler.ExponentialLR(o, gamma=0.9) for o in (a, b)]
    for i in range(3):
        _steps(ps, qs, a, b, 1, seed=10 + i)
        for s in sched:
            s.step()
    assert all(torch.equal(p, q) for p, q in zip(ps, qs))
    _same_state(a, b)
    assert a.step(lambda: torch.tensor(2.5)).item() == 2.5               # torch's signature: the closure's loss comes back
    # state_dict() round-trips both ways between the two classes, and both continue alike
    ps2, qs2, a2, b2 = _pair(seed=1)
    b.step()
    a2.load_state_dict(copy.deepcopy(b.state_dict()))
    b2.load_state_dict(copy.deepcopy(a.state_dict()))
    with torch.no_grad():
        for dst, src in zip(ps2 + qs2, qs + ps):
            dst.copy_(src)
    _same_state(a2, b)
    _steps(ps2, qs2, a2, b2, 2, seed=20)
    _steps(ps, qs, a, b, 2, seed=20)
    assert all(torch.equal(x, y) for x, y in zip(ps2 + qs2, qs + ps))


def test_state_dict_with_python_int_steps_loads_and_steps():
    """The form torch 1.8 wrote (the reference's checkpoints): `step` a Python int."""
    ps, qs, a, b = _pair()
    _steps(ps, qs, a, b, 2, seed=5)
    sd = copy.deepcopy(b.state_dict())
    for st in sd['state'].values():
        st['step'] = int(st['step'].item())
    ps2, qs2, a2, b2 = _pair(seed=2)
    a2.load_state_dict(copy.deepcopy(sd))
    b2.load_state_dict(copy.deepcopy(sd))
    with torch.no_grad():
        for dst, src in zip(ps2 + qs2, ps + ps):
            dst.copy_(src)
    _steps(ps2, qs2, a2, b2, 1, seed=6)
    assert all(torch.equal(x, y) for x, y in zip(ps2, qs2))
    assert all(float(st['step']) == 3 for st in a2.state_dict()['state'].values())


@pytest.mark.parametrize('flag', ['amsgrad', 'maximize', 'capturable', 'differentiable'])
def test_unserved_variants_raise_at_construction(flag):
    with pytest.raises(ValueError, match=flag):
        AdamW([torch.zeros(3, requires_grad=True)], **{flag: True})
    AdamW([torch.zeros(3, requires_grad=True)], **{flag: False})
