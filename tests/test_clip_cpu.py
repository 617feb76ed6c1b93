"""CPU tests of the global-norm clip and the non-finite guard (v2w_grad_sumsq_multi, v2w_grad_norm_finish, v2w_scale_multi,
v2w_adamw_multi_clipped; optim.clip_grad_norm_ and AdamW(max_grad_norm, skip_nonfinite)): the fp64 restatement tests/clip_ref.py against
torch, the C ABI surface, the host-only partials query against the plan, what the entry points refuse, that the derived norm bound holds
for the kernel's order of operations and can see a wrong sum, and the Python surface on CPU tensors.  No GPU needed: nothing is launched."""
import copy
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

from tests import clip_ref as K
from tests import optim_ref as R
from wavthruvec_pytorch_amd import AdamW, Generator, _hip, clip_grad_norm_, hipops, synthetic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('v2w_grad_sumsq_partials', 'v2w_grad_sumsq_multi', 'v2w_grad_norm_finish', 'v2w_scale_multi', 'v2w_adamw_multi_clipped')
FAKE = 0x7f0000100000       # 16-byte aligned "device" pointers: the plan, the dry run and the name sink never dereference them
GAP = 1 << 44
DRY = C.c_void_p(-1)
BUF = C.c_void_p(FAKE + (1 << 50))


def _header():
    return open(os.path.join(ROOT, 'include', 'vec2wav_hip.h')).read()


def _items(numels, phases=None, g_only=False):
    """Descriptors on fake pointers, all four `phases[i]` floats past a 16-byte line; g_only leaves p, m and v NULL."""
    arr = (_hip.AdamWItem * max(len(numels), 1))()
    for i, (d, n) in enumerate(zip(arr, numels)):
        ph = phases[i] if phases else 0
        base = FAKE + i * (1 << 36) + 4 * ph
        d.g, d.numel = base + GAP, n
        if not g_only:
            d.p, d.m, d.v = base, base + 2 * GAP, base + 3 * GAP
    return arr


def _hyper():
    return hipops.adamw_hyper(lr=2e-4, betas=(0.8, 0.99), eps=1e-8, weight_decay=0.01, step=1)


@pytest.mark.parametrize('wd', [0.0, 0.01])
@pytest.mark.parametrize('where', ['above', 'below', 'equal'])
def test_restatement_is_pinned_to_torch(where, wd):
    """torch.nn.utils.clip_grad_norm_ + torch.optim.AdamW(foreach=False) on fp64 CPU tensors against clip_ref: norm, coefficient, scaled
    gradients and the step, with u = 2^-53 (the sum of squares of 308 terms: a relative 308 u at most, taken as the roundings on g')."""
    gen = torch.Generator().manual_seed(5)
    ps = [torch.randn(n, generator=gen, dtype=torch.float64).requires_grad_() for n in (1, 7, 300)]
    grads = [torch.randn(p.shape, generator=gen, dtype=torch.float64) * 0.3 for p in ps]
    norm = K.total_norm([g.numpy() for g in grads])
    max_norm = {'above': 0.5 * norm, 'below': 2.0 * norm, 'equal': norm}[where]
    want_norm, coef, scaled = K.clip_ref([g.numpy() for g in grads], max_norm)
    assert (coef < 0.51) if where == 'above' else (coef == 1.0 if where == 'below' else 1.0 - 1e-5 < coef < 1.0)
    for p, g in zip(ps, grads):
        p.grad = g.clone()
    got_norm = torch.nn.utils.clip_grad_norm_(ps, max_norm, foreach=False)
    assert abs(float(got_norm) - want_norm) <= 308 * R.U64 * want_norm
    for p, s in zip(ps, scaled):
        assert np.abs(p.grad.numpy() - s).max() <= (308 + 2) * R.U64 * np.abs(s).max()
    hyper = dict(lr=2e-3, betas=(0.8, 0.99), eps=1e-8, weight_decay=wd)
    opt = torch.optim.AdamW(ps, foreach=False, **hyper)
    before = [p.detach().numpy().copy() for p in ps]
    opt.step()
    h = R.make_hyper(step=1, dtype=np.float64, **hyper)
    for p, p0, g in zip(ps, before, grads):
        z = np.zeros(p0.shape)
        rp, rm, rv, mags = K.clipped_adamw_ref(p0, g.numpy(), z, z, h, coef)
        st = opt.state[p]
        got = (p.detach().numpy(), st['exp_avg'].numpy(), st['exp_avg_sq'].numpy())
        assert R.worst_ratio(got, (rp, rm, rv), K.step_bounds(mags, g_roundings=310, u=R.U64)) <= 1.0


def test_entry_points_are_declared_bound_and_additive():
    hdr = _header()
    assert int(re.search(r'#define V2W_ABI_VERSION (\d+)', hdr).group(1)) == _hip.ABI_VERSION == 35 == _hip.load().v2w_abi_version()
    lib = _hip.load()
    for name in NAMES:
        assert name in _hip.SIGNATURES and re.search(r'\b%s\s*\(' % name, hdr) and hasattr(lib, name), name
        assert (name in _hip.LAUNCHERS) == (name != 'v2w_grad_sumsq_partials'), name
    # the roundings clip_ref's bounds rest on are the ones the header states
    for k, word in (('m', "roundings on m'"), ('v', "on v'"), ('p', "on p'")):
        assert re.search(r'\b%d %s' % (K.step_roundings(1)[k], re.escape(word)), hdr), k
    assert K.step_roundings(1) == {'m': 4, 'v': 6, 'p': 18}
    assert '(T + 10) / 2 + 1' in hdr and 'T = 4 * ceil(chunk_i / 256)' in hdr
    assert K.sumsq_roundings(2048) == 42 and K.norm_roundings(2048) == 22 and 'that is 22 u' in hdr
    assert (K.MIN_CHUNK, K.TARGET_WGS, K.THREADS) == (2048, _hip.ADAMW_TARGET_WGS, 256)


PLAN_CASES = {
    'one_float': ([1], None),
    'mixed': ([1, 37, 4099, 250_000, 2_752_512, 12, 3 * 2048 * 4], None),
    'max_items_tiny': ([5] * _hip.ADAMW_MAX_ITEMS, None),
    'phases': ([4 * 2048 * 3] * 5, [0, 1, 3, 0, 2]),
    'huge': ([1 << 33, 7], None),
}


@pytest.mark.parametrize('case', sorted(PLAN_CASES))
def test_partials_query_equals_the_plan(case):
    """The shapes of tests/test_optim_cpu.py: the query (it looks at g and numel only) returns what v2w_adamw_multi_plan returns for items
    whose four pointers have g's phase, and what clip_ref.plan restates."""
    numels, phases = PLAN_CASES[case]
    n = len(numels)
    lib = _hip.load()
    starts, nwg = hipops.adamw_plan(_items(numels, phases), n)
    assert lib.v2w_grad_sumsq_partials(_items(numels, phases, g_only=True), n) == nwg == starts[-1]
    assert K.plan(numels, phases or [0] * n)[0] == starts
    if case == 'phases':
        assert [b - a for a, b in zip(starts, starts[1:])] == [3, 4, 4, 3, 4]


def test_partials_of_the_generators_parameters_in_chunks():
    g = Generator(synthetic.make_hparams(num_wv_feat=768))
    numels = [p.numel() for p in g.parameters()]
    assert len(numels) == 131
    lib = _hip.load()
    total = 0
    for i0 in range(0, len(numels), _hip.ADAMW_MAX_ITEMS):
        part = numels[i0:i0 + _hip.ADAMW_MAX_ITEMS]
        starts, nwg = hipops.adamw_plan(_items(part), len(part))
        assert lib.v2w_grad_sumsq_partials(_items(part, g_only=True), len(part)) == nwg
        assert K.plan(part, [0] * len(part)) == (starts, 2048)      # the chunk the header's "22 u at the generator's list" rests on
        total += nwg
    assert 131 <= total <= 2 * _hip.ADAMW_TARGET_WGS + 131


def test_name_sink_lists_each_entrys_kernel():
    lib = _hip.load()
    arr = _items([1, 4099, 250_000], [0, 1, 2])
    for fn, args, kernel in ((lib.v2w_grad_sumsq_multi, (arr, 3, BUF), 'grad_sumsq_kernel'),
                             (lib.v2w_scale_multi, (arr, 3, BUF), 'grad_scale_kernel'),
                             (lib.v2w_grad_norm_finish, (BUF, 7, 1.0, BUF), 'grad_norm_finish_kernel'),
                             (lib.v2w_adamw_multi_clipped, (arr, 3, C.byref(_hyper()), BUF, 1), 'adamw_multi_clipped_kernel')):
        rc, names = _hip.kernel_names(fn, *args)
        assert rc in (0, 100) and names == [kernel], (kernel, rc, names)
    # the step without a coefficient is the kernel it was
    assert _hip.kernel_names(lib.v2w_adamw_multi, arr, 3, C.byref(_hyper()))[1] == ['adamw_multi_kernel']


def test_entry_points_refuse_bad_arguments_with_an_error_code():
    lib = _hip.load()
    M = _hip.ADAMW_MAX_ITEMS
    E = _hip.E_ARG
    odd = C.c_void_p(BUF.value + 2)

    def named(fn, *args):
        """the dry run's code; a refused call names no kernel"""
        rc = fn(*args, DRY)
        assert rc == 0 or _hip.kernel_names(fn, *args) == (rc, [])
        return rc

    for fn in (lib.v2w_grad_sumsq_multi, lib.v2w_scale_multi):
        run = lambda arr, n, buf=BUF: named(fn, arr, n, buf)                   # noqa: E731
        assert run(_items([7] * M, g_only=True), M) == 0                        # p, m and v are not looked at
        assert run(_items([7, 1 << 42], g_only=True), 2) == 0
        assert run(None, 1) == E and run(_items([7]), 0) == E and run(_items([7] * (M + 1)), M + 1) == E
        assert run(_items([7]), 1, None) == E and run(_items([7]), 1, odd) == E
        assert run(_items([7, 0]), 2) == E and run(_items([-3]), 1) == E
        assert run(_items([(1 << 42) + 1]), 1) == _hip.E_SHAPE
        arr = _items([7, 9])
        arr[1].g = None
        assert run(arr, 2) == E
        arr = _items([7, 9])
        arr[1].g += 2
        assert run(arr, 2) == E
        arr[1].g += 2                                                           # 4-byte aligned is enough
        assert run(arr, 2) == 0
    q = lib.v2w_grad_sumsq_partials
    assert q(None, 1) == E and q(_items([7]), 0) == E and q(_items([7] * (M + 1)), M + 1) == E and q(_items([0]), 1) == E
    assert q(_items([(1 << 42) + 1]), 1) == _hip.E_SHAPE and q(_items([7] * M), M) == M

    fin = lambda p, n, mx, out: named(lib.v2w_grad_norm_finish, p, n, mx, out)  # noqa: E731
    assert fin(BUF, 1, 0.0, BUF) == 0 and fin(BUF, 5000, float('inf'), BUF) == 0
    assert fin(None, 1, 1.0, BUF) == E and fin(BUF, 1, 1.0, None) == E and fin(odd, 1, 1.0, BUF) == E and fin(BUF, 1, 1.0, odd) == E
    assert fin(BUF, 0, 1.0, BUF) == E and fin(BUF, -4, 1.0, BUF) == E
    assert fin(BUF, 1, -1e-3, BUF) == E and fin(BUF, 1, float('nan'), BUF) == E and fin(BUF, 1, float('-inf'), BUF) == E

    ok = _hyper()
    step = lambda arr, n, h=ok, clip=BUF, skip=0: named(lib.v2w_adamw_multi_clipped, arr, n, C.byref(h) if h is not None else None, clip, skip)  # noqa: E731
    assert step(_items([7] * M), M) == 0 and step(_items([7]), 1, skip=1) == 0
    assert step(_items([7]), 1, clip=None) == E and step(_items([7]), 1, clip=odd) == E
    assert step(None, 1) == E and step(_items([7]), 1, h=None) == E and step(_items([7]), 0) == E and step(_items([7] * (M + 1)), M + 1) == E
    assert step(_items([7, 0]), 2) == E and step(_items([(1 << 42) + 1]), 1) == _hip.E_SHAPE
    for field in ('p', 'g', 'm', 'v'):                                          # every check of v2w_adamw_multi
        arr = _items([7, 9])
        setattr(arr[1], field, None)
        assert step(arr, 2) == E, field
        arr = _items([7, 9])
        setattr(arr[1], field, getattr(arr[1], field) + 2)
        assert step(arr, 2) == E, field
    arr = _items([100])
    arr[0].m = arr[0].p + 4 * 99
    assert step(arr, 1) == E
    bad = hipops.adamw_hyper(lr=float('nan'), betas=(0.8, 0.99), eps=1e-8, weight_decay=0.0, step=1)
    assert step(_items([7]), 1, h=bad) == E


def _norm_in_kernel_order(tensors, drop_tensor=None, drop_chunk=None):
    """The norm from the header's operations replayed in numpy fp32: one call's plan, every workgroup's partial, the fp64 finish."""
    numels = [t.size for t in tensors]
    starts, chunk = K.plan(numels, [0] * len(tensors))
    partials = np.concatenate([K.sumsq_partials_fp32(t, 0, b - a) for t, a, b in zip(tensors, starts, starts[1:])])
    assert partials.size == starts[-1] and partials.dtype == np.float32
    keep = np.ones(partials.size, dtype=bool)
    if drop_tensor is not None:
        keep[starts[drop_tensor]:starts[drop_tensor + 1]] = False
    if drop_chunk is not None:
        keep[drop_chunk] = False
    return np.float32(math.sqrt(K.finish_fp64(partials[keep]))), chunk, partials, starts


def test_the_norm_bound_holds_in_the_kernels_order_and_can_see_a_wrong_sum():
    """Tensors of ONE magnitude (a dropped piece is visible only if it carries more of the sum than the bound allows: the smallest
    tensor here, 255 of 319 010 entries, carries 8e-4 of it; the bound is 2 * 22 u = 2.6e-6 of the norm, 5.2e-6 of the sum)."""
    rng = np.random.default_rng(11)
    tensors = [rng.standard_normal(n).astype(np.float32) for n in (255, 257, 8191, 8193, 300_001, 2113)]
    exact = K.total_norm(tensors)
    got, chunk, partials, starts = _norm_in_kernel_order(tensors)
    assert chunk == 2048 and starts[-1] > len(tensors)                        # the large tensor has several workgroups
    bound = 2 * K.norm_roundings(chunk) * R.U32 * exact
    assert abs(float(got) - exact) <= bound
    # every workgroup's partial against the fp64 sum of its own elements
    for t, a, b in zip(tensors, starts, starts[1:]):
        for w, (e0, e1) in enumerate(K.spans(t.size, 0, b - a)):
            s = float((t[e0:e1].astype(np.float64) ** 2).sum())
            assert abs(float(partials[a + w]) - s) <= 2 * K.sumsq_roundings(chunk) * R.U32 * s
    for kw in (dict(drop_tensor=0), dict(drop_tensor=1), dict(drop_chunk=starts[4] + 3), dict(drop_chunk=starts[5] - 1)):
        wrong = _norm_in_kernel_order(tensors, **kw)[0]
        assert abs(float(wrong) - exact) > 100 * bound, kw


def _params(seed=0, dtype=torch.float32):
    gen = torch.Generator().manual_seed(seed)
    ps = [torch.randn(5, 3, generator=gen).to(dtype).requires_grad_(), torch.randn(7, generator=gen).to(dtype).requires_grad_()]
    for p in ps:
        p.grad = torch.randn(p.shape, generator=gen).to(dtype)
    return ps


def test_constructor_keeps_the_keywords_out_of_the_state_dict():
    ps = _params()
    a = AdamW(ps, 1e-2, betas=(0.8, 0.99), max_grad_norm=1000.0, skip_nonfinite=True)
    assert a.max_grad_norm == 1000.0 and a.skip_nonfinite is True and a.grad_norm is None and a.nonfinite_steps() == 0
    plain = AdamW(_params(), 1e-2, betas=(0.8, 0.99))
    assert plain.max_grad_norm is None and plain.skip_nonfinite is False
    for group in a.param_groups:
        assert 'max_grad_norm' not in group and 'skip_nonfinite' not in group
    assert 'max_grad_norm' not in a.defaults and 'skip_nonfinite' not in a.defaults
    # the state dict round-trips with torch.optim.AdamW, both ways
    qs = _params()
    b = torch.optim.AdamW(qs, 1e-2, betas=(0.8, 0.99))
    b.step()
    a.load_state_dict(copy.deepcopy(b.state_dict()))
    sa, sb = a.state_dict(), b.state_dict()
    assert sa['param_groups'] == sb['param_groups'] and sa['state'].keys() == sb['state'].keys()
    for k in sa['state']:
        assert all(torch.equal(sa['state'][k][name], sb['state'][k][name]) for name in sb['state'][k])
    c = torch.optim.AdamW(_params(1), 1e-2, betas=(0.8, 0.99))
    c.load_state_dict(copy.deepcopy(sa))
    assert c.state_dict()['param_groups'] == sb['param_groups']
    with pytest.raises(ValueError, match='max_grad_norm'):
        AdamW(_params(), max_grad_norm=-1.0)
    with pytest.raises(ValueError, match='max_grad_norm'):
        AdamW(_params(), max_grad_norm=float('nan'))


def test_what_is_not_served_raises_value_error():
    ps = _params()
    with pytest.raises(ValueError, match='norm_type'):
        clip_grad_norm_(ps, 1.0, norm_type=1)
    with pytest.raises(ValueError, match='norm_type'):
        clip_grad_norm_(ps, 1.0, norm_type=float('inf'))
    with pytest.raises(ValueError, match='fp32'):
        clip_grad_norm_(_params(dtype=torch.float16), 1.0)
    with pytest.raises(ValueError, match='GPU'):                                # no quiet fall-back to torch's on CPU gradients
        clip_grad_norm_(ps, 1.0)
    with pytest.raises(ValueError, match='max_norm'):
        clip_grad_norm_(ps, -1.0)
    before = [p.grad.clone() for p in ps]
    for kw in (dict(max_grad_norm=1.0), dict(skip_nonfinite=True)):
        opt = AdamW(ps, 1e-2, **kw)
        with pytest.raises(ValueError, match='GPU'):                            # CPU groups keep torch's step, which has no clip
            opt.step()
    assert all(torch.equal(p.grad, g) for p, g in zip(ps, before)) and len(opt.state) == 0
    # nothing to clip: torch's answers
    assert clip_grad_norm_([], 1.0).item() == 0.0
    assert clip_grad_norm_([torch.zeros(3, requires_grad=True)], 1.0).item() == 0.0


def test_wrappers_refuse_what_they_cannot_hand_to_the_kernels():
    t = [torch.zeros(4)]
    for call in (lambda: hipops.grad_sumsq_multi(t), lambda: hipops.scale_multi(t, torch.ones(1)),
                 lambda: hipops.grad_norm_finish(torch.zeros(4), 4, 1.0),
                 lambda: hipops.adamw_multi_clipped(t, t, t, t, torch.zeros(4), lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, step=1)):
        with pytest.raises(RuntimeError, match='must live on a GPU'):
            call()
    with pytest.raises(ValueError):
        hipops.grad_sumsq_multi([])
    with pytest.raises(ValueError):
        hipops.adamw_multi_clipped(t, t, t, [], torch.zeros(4), lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, step=1)
    assert hipops.scale_multi([], torch.ones(1)) == 0 and hipops.grad_sumsq_partials([]) == 0
