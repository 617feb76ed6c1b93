"""CPU tests of the exponential moving average of the weights (v2w_adamw_ema_multi, v2w_ema_multi, v2w_swap_multi; hipops.adamw_ema_multi /
ema_multi / swap_multi; optim.AdamW(ema_decay), swap_ema, ema_state_dict): the fp64 restatement tests/ema_ref.py against its closed form,
the C ABI surface and the two new structs, the by-value table's arithmetic, the host-only plans against a restatement in Python, what the
name sink reports, what the entry points and the Python surface refuse, and the checkpoint helper on a hand-filled optimizer state.  No GPU
needed: nothing is launched."""
import copy
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from tests import ema_ref as E
from tests import optim_ref as R
from wavthruvec_pytorch_amd import AdamW, _hip, ema_state_dict, hipops
from wavthruvec_pytorch_amd import optim as optim_mod

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('v2w_adamw_ema_multi_plan', 'v2w_adamw_ema_multi', 'v2w_ema_multi_plan', 'v2w_ema_multi', 'v2w_swap_multi')
PLANS = ('v2w_adamw_ema_multi_plan', 'v2w_ema_multi_plan')
FAKE = 0x7f0000100000       # 16-byte aligned "device" pointers: the plan, the dry run and the name sink never dereference them
GAP = 1 << 44               # between the fake p, g, m, v, e: more than the largest numel the entry points take (2^42 floats)
DRY = C.c_void_p(-1)        # the dry-run stream: every check of the real call, no launch
BUF = C.c_void_p(FAKE + (1 << 50))
FIVE = ('p', 'g', 'm', 'v', 'e')


def _header():
    return open(os.path.join(ROOT, 'include', 'vec2wav_hip.h')).read()


def _struct_fields(hdr, name):
    body = hdr[:hdr.index('} %s;' % name)]
    body = body[body.rindex('typedef struct {'):]
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    return re.findall(r'\b(\w+)(?:\[\d+\])?\s*[;,]', body)


def _items(numels, phases=None):
    """v2w_adamw_ema_item array on fake pointers; phases[i] = (p, g, m, v, e) offsets in floats past a 16-byte line."""
    arr = (_hip.AdamWEmaItem * max(len(numels), 1))()
    for i, (d, n) in enumerate(zip(arr, numels)):
        ph = phases[i] if phases else (0,) * 5
        base = FAKE + i * (1 << 36)
        d.p, d.g, d.m, d.v, d.e = (base + k * GAP + 4 * ph[k] for k in range(5))
        d.numel = n
    return arr


def _pairs(numels, phases=None):
    """v2w_ema_item / v2w_swap_item array on fake pointers; phases[i] = (p, e)."""
    arr = (_hip.EmaItem * max(len(numels), 1))()
    for i, (d, n) in enumerate(zip(arr, numels)):
        ph = phases[i] if phases else (0, 0)
        base = FAKE + i * (1 << 36)
        d.p, d.e, d.numel = base + 4 * ph[0], base + GAP + 4 * ph[1], n
    return arr


def _hyper(**kw):
    args = dict(lr=2e-4, betas=(0.8, 0.99), eps=1e-8, weight_decay=0.01, step=1)
    args.update(kw)
    return hipops.adamw_hyper(**args)


def test_restatement_against_the_closed_form_over_50_steps():
    """The recurrence e <- e + omd (p_t - e) in fp64 against d^T e_0 + (1 - d) sum d^(T-1-t) p_t: 50 steps, each with two fp64 roundings
    on magnitudes <= max|p| + |e_0|, and the closed form's own sum - 50 x 4 x 2^-53 of that magnitude covers both."""
    rng = np.random.default_rng(50)
    for decay in (0.0, 0.5, 0.99, 0.999):
        omd = E.omd32(decay)
        assert 0.0 <= float(omd) <= 1.0 and abs(float(omd) - (1.0 - decay)) <= R.U32
        e0 = rng.standard_normal(300).astype(np.float32)
        ps = [(rng.standard_normal(300) * 10.0 ** rng.uniform(-2, 0, 300)).astype(np.float32) for _ in range(50)]
        e = e0.astype(np.float64)
        for p in ps:
            e = E.ema_exact(e, p, omd)
        want = E.ema_closed_form(e0, ps, omd)
        mag = np.abs(e0) + np.max(np.abs(np.stack(ps)), axis=0)
        assert np.all(np.abs(e - want) <= 50 * 4 * R.U64 * mag)
    assert np.array_equal(E.ema_exact(e0, ps[0], np.float32(0.0)), e0.astype(np.float64))                 # decay 1: the average stays
    assert np.array_equal(E.ema_closed_form(e0, ps[:3], np.float32(1.0)), ps[2].astype(np.float64))      # decay 0: the last parameter


def test_the_bound_holds_for_the_headers_two_lines_in_numpy_fp32_and_can_see_a_wrong_average():
    """de = p' - e and e' = fma(omd, de, e) in numpy float32 (the fma as a float64 product and sum rounded once) stay inside 3u (|e| + |p'|);
    an average that used decay for 1 - decay, or the parameter from before the step, misses it by far."""
    f = np.float32
    rng = np.random.default_rng(3)
    omd = E.omd32(0.99)
    worst = 0.0
    for n in (1, 5, 8192 + 5):
        p_old, _g, _m, _v = R.kernel_state(n, rng)
        p_new = (p_old * f(0.999) - f(1e-2) * rng.standard_normal(n).astype(f)).astype(f)
        e = (p_old + f(1e-3) * rng.standard_normal(n).astype(f)).astype(f)
        de = (p_new - e).astype(f)
        got = (np.float64(omd) * de.astype(np.float64) + e.astype(np.float64)).astype(f)
        want, bnd = E.ema_exact(e, p_new, omd), E.ema_bound(e, p_new)
        worst = max(worst, E.worst_ratio(got, want, bnd))
        if n > 1:
            assert E.worst_ratio(E.ema_exact(e, p_new, f(0.99)), want, bnd) >= 100.0
            assert E.worst_ratio(E.ema_exact(e, p_old, omd), want, bnd) >= 100.0
    assert worst <= 1.0, worst


def test_entry_points_structs_and_the_item_limit():
    hdr = _header()
    assert int(re.search(r'#define V2W_ABI_VERSION (\d+)', hdr).group(1)) == _hip.ABI_VERSION == 35 == _hip.load().v2w_abi_version()
    lib = _hip.load()
    for name in NAMES:
        assert name in _hip.SIGNATURES and re.search(r'\b%s\s*\(' % name, hdr) and hasattr(lib, name), name
        assert (name in _hip.LAUNCHERS) == (name not in PLANS), name
    # the two new structs (and the writable twin of the second) against the ctypes mirrors: names, order, offsets, sizes
    assert _struct_fields(hdr, 'v2w_adamw_ema_item') == [n for n, _ in _hip.AdamWEmaItem._fields_] == ['p', 'g', 'm', 'v', 'e', 'numel']
    assert _struct_fields(hdr, 'v2w_ema_item') == _struct_fields(hdr, 'v2w_swap_item') == [n for n, _ in _hip.EmaItem._fields_] == ['p', 'e', 'numel']
    assert C.sizeof(_hip.AdamWEmaItem) == 48 and C.sizeof(_hip.EmaItem) == 24
    assert [getattr(_hip.AdamWEmaItem, n).offset for n in ('p', 'g', 'm', 'v', 'e', 'numel')] == [0, 8, 16, 24, 32, 40]
    assert [getattr(_hip.EmaItem, n).offset for n in ('p', 'e', 'numel')] == [0, 8, 16]
    assert re.search(r'const float\*\s+p;\s+float\*\s+e;\s+int64_t numel;\s+\} v2w_ema_item;', hdr)          # p is only read there
    assert re.search(r'\n\s+float\*\s+p;\s+float\*\s+e;\s+int64_t numel;\s+\} v2w_swap_item;', hdr)           # and written here
    # the library reads the fields where the mirror puts them: a plan from numel and from each pointer's phase
    starts = (C.c_int32 * 2)()
    assert lib.v2w_adamw_ema_multi_plan(_items([4 * 2048 * 3]), 1, starts) == 3
    assert lib.v2w_adamw_ema_multi_plan(_items([4 * 2048 * 3], [(1,) * 5]), 1, starts) == 4
    assert lib.v2w_ema_multi_plan(_pairs([4 * 2048 * 3], [(2, 2)]), 1, starts) == 4
    # the by-value table: items + starts + 7 constants + ema_omd + n within the library's 3584 bytes, as the header states
    M = _hip.ADAMW_EMA_MAX_ITEMS
    assert int(re.search(r'#define V2W_ADAMW_EMA_MAX_ITEMS\s+(\d+)', hdr).group(1)) == M == 64
    assert M * 48 + (M + 1) * 4 + 28 + 4 + 4 == 3368 <= 3584 and '= 3368 bytes' in hdr
    assert _hip.ADAMW_MAX_ITEMS * 24 + (_hip.ADAMW_MAX_ITEMS + 1) * 4 + 4 == 2248 <= 3584 and '= 2248' in hdr
    assert re.search(r'\b%d roundings on e\'' % E.ROUNDINGS, hdr) and '3u (|e| + |p\'|)' in hdr
    assert 'does not move the average either' in hdr                                                     # what a skipped step leaves alone


def _plan_restated(numels, phases, width):
    """include/vec2wav_hip.h: units of four floats (cut at p's 16-byte lines when ALL `width` pointers share their phase), a chunk that
    deals about ADAMW_TARGET_WGS workgroups, >= 1 per tensor."""
    units = []
    for i, n in enumerate(numels):
        ph = phases[i] if phases else (0,) * width
        assert len(ph) == width
        units.append((n + (ph[0] if len(set(ph)) == 1 else 0) + 3) // 4)
    chunk = max(2048, -(-sum(units) // _hip.ADAMW_TARGET_WGS))
    starts = [0]
    for u in units:
        starts.append(starts[-1] + max(1, -(-u // chunk)))
    return starts


N3 = 4 * 2048 * 3           # three workgroups exactly; one more with a shared phase > 0
PLAN_CASES = {
    'one_float': ([1], None),
    'mixed': ([1, 37, 4099, 250_000, 2_752_512, 12, N3], None),
    'max_items_tiny': ([5] * 64, None),
    # all five alike (16-byte path with a head), then each single pointer off the others' phase (float by float: no head counted)
    'phases': ([N3] * 8, [(0,) * 5, (1,) * 5, (3,) * 5] + [tuple(int(k == j) for k in range(5)) for j in range(5)]),
    'huge': ([1 << 33, 7], None),
}


@pytest.mark.parametrize('case', sorted(PLAN_CASES))
def test_plans_match_their_restatement(case):
    numels, phases = PLAN_CASES[case]
    n = len(numels)
    lib = _hip.load()
    starts = (C.c_int32 * (n + 1))()
    nwg = lib.v2w_adamw_ema_multi_plan(_items(numels, phases), n, starts)
    starts = list(starts)
    assert starts == _plan_restated(numels, phases, 5) and nwg == starts[-1]
    assert starts[0] == 0 and all(b - a >= 1 for a, b in zip(starts, starts[1:]))             # monotone, every tensor has a workgroup
    assert nwg <= _hip.ADAMW_TARGET_WGS + n
    if case == 'phases':       # a phase shared by all FIVE adds the floats before the first 16-byte line; any single stray pointer does not
        assert [b - a for a, b in zip(starts, starts[1:])] == [3, 4, 4, 3, 3, 3, 3, 3]
    # the pair plan: the phase over p and e
    pph = [(ph[0], ph[4]) for ph in phases] if phases else None
    pstarts = (C.c_int32 * (n + 1))()
    assert lib.v2w_ema_multi_plan(_pairs(numels, pph), n, pstarts) == _plan_restated(numels, pph, 2)[-1]
    assert list(pstarts) == _plan_restated(numels, pph, 2)
    if case == 'phases':
        assert [b - a for a, b in zip(pstarts, pstarts[1:])] == [3, 4, 4, 3, 3, 3, 3, 3]
    # where the fifth pointer agrees, the plan is v2w_adamw_multi_plan's of the first four
    if case != 'phases':
        four = (_hip.AdamWItem * n)()
        for d, s in zip(four, _items(numels)):
            d.p, d.g, d.m, d.v, d.numel = s.p, s.g, s.m, s.v, s.numel
        assert hipops.adamw_plan(four, n) == (starts, nwg)


def test_name_sink_lists_each_entrys_kernel():
    lib = _hip.load()
    arr = _items([1, 4099, 250_000], [(0,) * 5, (1,) * 5, (0, 0, 0, 0, 1)])
    h = C.byref(_hyper())
    for fn, args, kernel in ((lib.v2w_adamw_ema_multi, (arr, 3, h, None, 0, 0.001), 'adamw_ema_multi_kernel'),
                             (lib.v2w_adamw_ema_multi, (arr, 3, h, None, 1, 0.001), 'adamw_ema_multi_kernel'),
                             (lib.v2w_adamw_ema_multi, (arr, 3, h, BUF, 1, 0.001), 'adamw_ema_multi_clipped_kernel'),
                             (lib.v2w_ema_multi, (_pairs([1, 4099], [(0, 0), (0, 1)]), 2, 0.001), 'ema_multi_kernel'),
                             (lib.v2w_swap_multi, (_pairs([1, 4099], [(0, 0), (0, 1)]), 2), 'swap_multi_kernel')):
        rc, names = _hip.kernel_names(fn, *args)
        assert rc in (0, 100) and names == [kernel], (kernel, rc, names)
    # the existing steps are the kernels they were
    four = (_hip.AdamWItem * 1)()
    four[0].p, four[0].g, four[0].m, four[0].v, four[0].numel = FAKE, FAKE + GAP, FAKE + 2 * GAP, FAKE + 3 * GAP, 9
    assert _hip.kernel_names(lib.v2w_adamw_multi, four, 1, h)[1] == ['adamw_multi_kernel']
    assert _hip.kernel_names(lib.v2w_adamw_multi_clipped, four, 1, h, BUF, 0)[1] == ['adamw_multi_clipped_kernel']


def test_entry_points_refuse_bad_arguments_with_an_error_code():
    lib = _hip.load()
    M, M2 = _hip.ADAMW_EMA_MAX_ITEMS, _hip.ADAMW_MAX_ITEMS
    EA, ES = _hip.E_ARG, _hip.E_SHAPE
    odd = C.c_void_p(BUF.value + 2)
    ok = _hyper()

    def named(fn, *args):
        """the dry run's code; a refused call names no kernel"""
        rc = fn(*args, DRY)
        assert rc == 0 or _hip.kernel_names(fn, *args) == (rc, [])
        return rc

    step = lambda arr, n, h=ok, clip=None, skip=0, omd=0.001: named(lib.v2w_adamw_ema_multi, arr, n, C.byref(h) if h is not None else None, clip, skip, omd)  # noqa: E731
    assert step(_items([7] * M), M) == 0 and step(_items([7] * M), M, clip=BUF, skip=1) == 0
    assert step(_items([7, 1 << 42]), 2) == 0
    assert step(_items([7] * (M + 1)), M + 1) == EA and step(_items([7]), 0) == EA and step(None, 1) == EA and step(_items([7]), 1, h=None) == EA
    assert step(_items([7]), 1, clip=odd) == EA
    assert step(_items([7, 0]), 2) == EA and step(_items([-3]), 1) == EA and step(_items([(1 << 42) + 1]), 1) == ES
    for omd, want in ((0.0, 0), (1.0, 0), (-1e-6, EA), (1.0 + 1e-6, EA), (float('nan'), EA), (float('inf'), EA)):
        assert step(_items([7]), 1, omd=omd) == want, omd
    for field in FIVE:
        arr = _items([7, 9])
        setattr(arr[1], field, None)
        assert step(arr, 2) == EA, field
        arr = _items([7, 9])
        setattr(arr[1], field, getattr(arr[1], field) + 2)                  # not 4-byte aligned
        assert step(arr, 2) == EA, field
        arr = _items([7, 9])
        setattr(arr[1], field, getattr(arr[1], field) + 4)                  # 4-byte aligned is enough
        assert step(arr, 2) == 0, field
    for a, b in (('p', 'm'), ('p', 'v'), ('m', 'v'), ('p', 'e'), ('m', 'e'), ('v', 'e')):
        arr = _items([100])
        setattr(arr[0], b, getattr(arr[0], a) + 4 * 99)
        assert step(arr, 1) == EA, (a, b)
        setattr(arr[0], b, getattr(arr[0], a) + 4 * 100)                     # back to back: no overlap
        assert step(arr, 1) == 0, (a, b)
        setattr(arr[0], b, getattr(arr[0], a) - 4 * 99)
        assert step(arr, 1) == EA, (a, b)
    bad = hipops.adamw_hyper(lr=float('nan'), betas=(0.8, 0.99), eps=1e-8, weight_decay=0.0, step=1)
    assert step(_items([7]), 1, h=bad) == EA and step(_items([7]), 1, h=_hyper(betas=(1.0, 0.99))) == EA

    ema = lambda arr, n, omd=0.001: named(lib.v2w_ema_multi, arr, n, omd)   # noqa: E731
    swap = lambda arr, n, omd=None: named(lib.v2w_swap_multi, arr, n)       # noqa: E731
    for run in (ema, swap):
        assert run(_pairs([7] * M2), M2) == 0 and run(_pairs([7, 1 << 42]), 2) == 0
        assert run(_pairs([7] * (M2 + 1)), M2 + 1) == EA and run(_pairs([7]), 0) == EA and run(None, 1) == EA
        assert run(_pairs([7, 0]), 2) == EA and run(_pairs([(1 << 42) + 1]), 1) == ES
        for field in ('p', 'e'):
            arr = _pairs([7, 9])
            setattr(arr[1], field, None)
            assert run(arr, 2) == EA, field
            arr = _pairs([7, 9])
            setattr(arr[1], field, getattr(arr[1], field) + 2)
            assert run(arr, 2) == EA, field
        arr = _pairs([100])
        arr[0].e = arr[0].p + 4 * 99                                         # p and e of one item overlap
        assert run(arr, 1) == EA
        arr[0].e = arr[0].p + 4 * 100
        assert run(arr, 1) == 0
    for omd, want in ((0.0, 0), (1.0, 0), (-0.5, EA), (1.5, EA), (float('nan'), EA)):
        assert ema(_pairs([7]), 1, omd) == want, omd
    starts = (C.c_int32 * 3)()
    assert lib.v2w_adamw_ema_multi_plan(_items([7]), 1, None) == EA and lib.v2w_ema_multi_plan(_pairs([7]), 1, None) == EA
    assert lib.v2w_adamw_ema_multi_plan(_items([(1 << 42) + 1]), 1, starts) == ES and lib.v2w_ema_multi_plan(_pairs([7] * 3), 0, starts) == EA
    assert lib.v2w_adamw_ema_multi_plan(_items([7] * (M + 1)), M + 1, (C.c_int32 * (M + 2))()) == EA


HYP = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, step=1)


def test_wrappers_refuse_what_they_cannot_hand_to_the_kernels():
    t = [torch.zeros(4)]
    for call in (lambda: hipops.adamw_ema_multi(t, t, t, t, t, ema_decay=0.999, **HYP),
                 lambda: hipops.adamw_ema_multi(t, t, t, t, t, torch.zeros(4), ema_decay=0.999, skip_nonfinite=True, **HYP),
                 lambda: hipops.ema_multi(t, t, ema_decay=0.999),
                 lambda: hipops.swap_multi(t, t)):
        with pytest.raises(RuntimeError, match='must live on a GPU'):
            call()
    for call in (lambda: hipops.adamw_ema_multi([], [], [], [], [], ema_decay=0.999, **HYP),
                 lambda: hipops.ema_multi([], [], ema_decay=0.999),
                 lambda: hipops.swap_multi([], []),
                 lambda: hipops.adamw_ema_multi(t, t, t, t, [], ema_decay=0.999, **HYP),
                 lambda: hipops.ema_multi(t, [], ema_decay=0.999),
                 lambda: hipops.swap_multi(t, t + t)):
        with pytest.raises(ValueError):
            call()
    for bad in (-0.1, 1.5, float('nan')):
        with pytest.raises(ValueError, match='ema_decay'):
            hipops.adamw_ema_multi(t, t, t, t, t, ema_decay=bad, **HYP)
        with pytest.raises(ValueError, match='ema_decay'):
            hipops.ema_multi(t, t, ema_decay=bad)
    assert hipops.ema_omd(1.0) == 0.0 and hipops.ema_omd(0.0) == 1.0         # both ends are served at this level


def _params(seed=0):
    gen = torch.Generator().manual_seed(seed)
    ps = [torch.randn(5, 3, generator=gen).requires_grad_(), torch.randn(7, generator=gen).requires_grad_()]
    for p in ps:
        p.grad = torch.randn(p.shape, generator=gen)
    return ps


@pytest.mark.parametrize('bad', [-0.1, 1.0, float('nan')])
def test_constructor_refuses_a_decay_outside_the_half_open_interval(bad):
    with pytest.raises(ValueError, match='ema_decay'):
        AdamW(_params(), ema_decay=bad)


def test_constructor_keeps_the_keyword_out_of_the_state_dict_and_none_is_torchs_optimizer():
    a = AdamW(_params(), 1e-2, betas=(0.8, 0.99), ema_decay=0.999)
    assert a.ema_decay == 0.999 and AdamW(_params(), ema_decay=0).ema_decay == 0.0
    assert all('ema_decay' not in g for g in a.param_groups) and 'ema_decay' not in a.defaults
    assert a.ema_parameters() == []
    # without the keyword: torch's state after one CPU step, key for key and bit for bit
    ps, qs = _params(), _params()
    plain, ref = AdamW(ps, 1e-2, betas=(0.8, 0.99)), torch.optim.AdamW(qs, 1e-2, betas=(0.8, 0.99))
    assert plain.ema_decay is None
    plain.step(), ref.step()
    sa, sb = plain.state_dict(), ref.state_dict()
    assert sa['param_groups'] == sb['param_groups'] and sa['state'].keys() == sb['state'].keys()
    for k in sa['state']:
        assert list(sa['state'][k]) == list(sb['state'][k]) == ['step', 'exp_avg', 'exp_avg_sq']
        assert all(torch.equal(sa['state'][k][name], sb['state'][k][name]) for name in sb['state'][k])
    assert all(torch.equal(p, q) for p, q in zip(ps, qs)) and plain.ema_parameters() == []
    with pytest.raises(RuntimeError, match='ema_decay'):
        with plain.swap_ema():
            pass


def test_cpu_parameters_with_a_decay_raise_value_error_and_nothing_moves():
    ps = _params()
    before = [p.detach().clone() for p in ps]
    opt = AdamW(ps, 1e-2, ema_decay=0.999)
    with pytest.raises(ValueError, match='GPU'):
        opt.step()
    assert all(torch.equal(p, b) for p, b in zip(ps, before)) and len(opt.state) == 0


class _Tiny(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.conv = torch.nn.Conv1d(2, 3, 3)
        self.bn = torch.nn.BatchNorm1d(3)
        self.head = torch.nn.Linear(3, 1, bias=False)
        self.frozen = torch.nn.Parameter(torch.full((2,), 5.0))        # a parameter the optimizer has no state for


def test_ema_state_dict_keeps_keys_and_order_and_takes_the_averages():
    """A hand-filled optimizer state (no step was taken): every parameter with an average is replaced by a clone of it, buffers and the
    parameter without one come through as they are, and the result loads into a fresh module."""
    torch.manual_seed(0)
    mod = _Tiny()
    mod.bn.running_mean.fill_(0.25)
    stepped = [p for n, p in mod.named_parameters() if n != 'frozen']
    opt = AdamW(mod.parameters(), 1e-2, ema_decay=0.9)
    for i, p in enumerate(stepped):
        opt.state[p] = dict(step=torch.tensor(1.0), exp_avg=torch.zeros_like(p), exp_avg_sq=torch.zeros_like(p),
                            ema=torch.full_like(p, 10.0 + i))
    pairs = opt.ema_parameters()
    assert [p for p, _e in pairs] == stepped and all(e is opt.state[p]['ema'] for p, e in pairs)
    ref = mod.state_dict()
    out = ema_state_dict(opt, mod)
    assert out is not ref and type(out) is type(ref) and list(out) == list(ref)
    assert list(out) == ['frozen', 'conv.weight', 'conv.bias', 'bn.weight', 'bn.bias', 'bn.running_mean', 'bn.running_var',
                         'bn.num_batches_tracked', 'head.weight']
    names = {id(p): n for n, p in mod.named_parameters()}
    for i, p in enumerate(stepped):
        got = out[names[id(p)]]
        assert got.shape == p.shape and bool((got == 10.0 + i).all()) and got.data_ptr() != opt.state[p]['ema'].data_ptr()
        assert not got.requires_grad
    for key in ('frozen', 'bn.running_mean', 'bn.running_var', 'bn.num_batches_tracked'):
        assert torch.equal(out[key], ref[key]) and out[key].dtype == ref[key].dtype
    assert all(torch.equal(a, b) for a, b in zip(ref.values(), mod.state_dict().values()))                 # the module was not touched
    fresh = _Tiny()
    fresh.load_state_dict(out)
    assert bool((fresh.head.weight == 10.0 + len(stepped) - 1).all()) and bool((fresh.bn.running_mean == 0.25).all())
    assert optim_mod.ema_state_dict is ema_state_dict
    # the averages travel in the optimizer's state dict by torch's own mechanism
    opt2 = AdamW(_Tiny().parameters(), 1e-2, ema_decay=0.9)
    opt2.load_state_dict(copy.deepcopy(opt.state_dict()))
    assert [float(e.flatten()[0]) for _p, e in opt2.ema_parameters()] == [10.0 + i for i in range(len(stepped))]
