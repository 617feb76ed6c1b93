"""tests/wgrad_ref.py pinned against independent statements of the same weight gradient (an explicit loop over (t, ci, co), central
differences of the fp64 forward), its bit-exact bf16 activation against a scalar numpy statement, and the dispatch table of the weight-gradient
kernel tests (tests/wgrad_cases.py through the name sink: which kernels every GPU case launches).  No GPU needed."""
import numpy as np
import pytest
import torch

from tests import wgrad_cases as K
from tests import wgrad_ref as R


def _rnd(seed, *shape):
    return torch.from_numpy(np.random.default_rng(seed).standard_normal(shape))


def _close(a, b, tol=1e-12):
    assert a.shape == b.shape, (a.shape, b.shape)
    assert (a - b).abs().max().item() <= tol * max(1.0, b.abs().max().item())


def _loop(act, dy, k, dil, u):
    """dW[t][ci][co] by the definitions of the two layers, one entry at a time.  Conv1d: y[q] += w[t] act[q + (t - (k-1)/2) dil];
    ConvTranspose1d: y[u q - pad + t] += w[t] act[q]."""
    B, ci, Lq = act.shape
    co, Ly = dy.shape[1], dy.shape[2]
    dw = torch.zeros(k, ci, co, dtype=torch.float64)
    for t in range(k):
        for i in range(ci):
            for o in range(co):
                acc = 0.0
                for b in range(B):
                    for q in range(Lq):
                        if u == 1:
                            p = q + (t - (k - 1) // 2) * dil
                            if 0 <= p < Lq:
                                acc += act[b, i, p].item() * dy[b, o, q].item()
                        else:
                            p = u * q - (k - u) // 2 + t
                            if 0 <= p < Ly:
                                acc += act[b, i, q].item() * dy[b, o, p].item()
                dw[t, i, o] = acc
    return dw


@pytest.mark.parametrize('u,k,dil', [(1, 3, 1), (1, 5, 2), (1, 4, 1), (2, 4, 1), (2, 5, 1), (5, 11, 1)])
def test_reference_is_the_explicit_loop_and_the_central_difference(u, k, dil):
    B, ci, co, Lq = 2, 2, 3, 7
    x, a, s, dy = _rnd(1, B, ci, Lq), _rnd(2, B, ci), _rnd(3, B, ci), _rnd(4, B, co, u * Lq)
    want, S = R.wgrad(x, a, s, dy, k, dil, u, 0.1)
    act = R.act_f64(x, a, s, 0.1)
    z = a[:, :, None] * x + s[:, :, None]
    _close(act, torch.where(z > 0, z, z * float(np.float32(0.1))), 0.0)
    _close(want, _loop(act, dy, k, dil, u))
    _close(S, _loop(act.abs(), dy.abs(), k, dil, u))
    assert (S >= want.abs() - 1e-12).all()
    # <forward(act, w), dy> is linear in w: its central difference along one weight is that weight's gradient
    h = 0.5
    shape = (co, ci, k) if u == 1 else (ci, co, k)
    fd = torch.zeros(k, ci, co, dtype=torch.float64)
    for t in range(k):
        for i in range(ci):
            for o in range(co):
                e = torch.zeros(shape, dtype=torch.float64)
                e[(o, i, t) if u == 1 else (i, o, t)] = h
                fd[t, i, o] = ((R.forward(act, e, k, dil, u) - R.forward(act, -e, k, dil, u)) * dy).sum() / (2 * h)
    _close(want, fd)
    # no affine, slope 1: the plain signal
    _close(R.wgrad(x, None, None, dy, k, dil, u, 1.0)[0], _loop(x, dy, k, dil, u))


def _bf16_rne(v):
    """float32 array -> the nearest bf16 (ties to even) as float32, on the bit patterns."""
    b = np.asarray(v, dtype=np.float32).view(np.uint32).astype(np.uint64)
    b = (b + 0x7fff + ((b >> 16) & 1)) & 0xffff0000
    return b.astype(np.uint32).view(np.float32)


@pytest.mark.parametrize('stored', ['f32', 'bf16'])
def test_bf16_activation_is_the_fp32_fma_rounded_once(stored):
    x, a, s = R.draw_exact(np.random.default_rng(5), 3, 4, 257)
    assert x.abs().min().item() >= R.X_MIN
    if stored == 'bf16':
        x = x.bfloat16()
        assert x.float().abs().min().item() >= R.X_MIN
    xf = x.float().numpy()
    # a * x + s in fp64 is exact for this draw, so its one rounding to fp32 is the fused multiply-add
    z64 = a.numpy().astype(np.float64)[:, :, None] * xf.astype(np.float64) + s.numpy().astype(np.float64)[:, :, None]
    z = z64.astype(np.float32)
    assert np.array_equal(R.affine_f32(x.float(), a, s).numpy(), z)
    v = np.where(z > 0, z, (z * np.float32(0.1)).astype(np.float32))
    assert np.array_equal(R.act_bf16(x, a, s, 0.1).numpy(), _bf16_rne(v).astype(np.float64))
    v0 = np.where(xf > 0, xf, (xf * np.float32(0.1)).astype(np.float32))
    assert np.array_equal(R.act_bf16(x, None, None, 0.1).numpy(), _bf16_rne(v0).astype(np.float64))
    # the draw really reaches both signs and bf16 values that are not fp32-exact to begin with
    assert (z > 0).any() and (z < 0).any() and (_bf16_rne(v) != v).any()


def test_an_inexact_affine_is_refused():
    x = torch.full((1, 1, 4), 1.0 + 2.0 ** -23)
    with pytest.raises(AssertionError):
        R.affine_f32(x, torch.full((1, 1), 1.0 + 2.0 ** -20), torch.zeros(1, 1))          # a off the 1/16 grid
    with pytest.raises(AssertionError):
        R.affine_f32(x * 2.0 ** -40, torch.ones(1, 1), torch.full((1, 1), 0.5))           # x far below 2^-10: the sum needs more than 53 bits


# ---------------------------------------------------------------------------------------------------------------
# the dispatch table: one row per GPU case
ROWS = [(e, c) for e, cases in K.TABLE.items() for c in cases]


def test_record_ids_are_unique():
    names = [c['id'] for _, c in ROWS]
    assert len(set(names)) == len(names)


@pytest.mark.parametrize('entry,c', ROWS, ids=['%s-%s' % (e, c['id']) for e, c in ROWS])
def test_dispatch_of_every_gpu_case(entry, c):
    rc, names = K.dispatch(c)
    print(entry, c['id'], rc, names)
    assert (rc, names) == (c['rc'], c['kernels']), (rc, names)
    # the slab count is positive exactly when the call runs - but for the refusals the count cannot see (it gets neither k > 64, nor the
    # dilation, nor a pointer): those records say `plan_ok`
    assert (K.slabs(c) > 0) == (c['rc'] == K.OK or c.get('plan_ok', False))
    assert c['n'] == (R.chain(c) if c['rc'] == K.OK else 0)


def test_the_table_reaches_every_branch():
    ok = [c for _, c in ROWS if c['rc'] == K.OK]
    seen = {n for c in ok for n in c['kernels']}
    # what try_pipe can return
    need = ['wgrad_pipe_kernel<%s, %d, 1, false>' % (cfg, nt) for cfg in ('32, 2, 2', '32, 1, 1', '16, 1, 1') for nt in (1, 2, 3, 4, 5, 6, 7)]
    need += ['wgrad_pipe_kernel<32, 2, 2, 5, 1, true>',
             'wgrad_pipe_kernel<32, 2, 2, 6, 5, false>', 'wgrad_pipe_kernel<32, 2, 2, 5, 5, false>', 'wgrad_pipe_kernel<32, 2, 2, 4, 4, false>',
             'wgrad_pipe_kernel<32, 1, 2, 4, 2, false>', 'wgrad_pipe_kernel<16, 1, 2, 4, 2, false>',
             'wgrad_kernel<32>', 'wgrad_kernel<16>', 'wgrad_reduce_kernel', 'wgrad_reduce16_kernel', 'wgrad_bf16_reduce_kernel']
    # what v2w_wgrad_bf16 can ask of wgb_launch_nt: one or three taps per wave on the tap-sharing arrangement, the group sizes of odd k <= 11 on
    # 2 x 2 (1, 3, 5, 7, 5 + 4, 6 + 5).  Two taps are instantiated for both, but no odd k asks for them.
    for bf in ('false', 'true'):
        need += ['wgrad_bf16_kernel<%d, 1, 1, %d, %s>' % (mf, nt, bf) for mf in (32, 16) for nt in (1, 3)]
        need += ['wgrad_bf16_kernel<32, 2, 2, %d, %s>' % (nt, bf) for nt in (1, 3, 4, 5, 6, 7)]
    assert [n for n in need if n not in seen] == []
    assert sorted(seen) == sorted(need)            # and nothing the list does not know
    # what the names cannot show: the generic kernel once per phase, both reduce kernels at the threshold, slabs that walk several items
    assert any(c['kernels'].count('wgrad_kernel<32>') == 8 and c['u'] == 8 for c in K.WGRAD_T)
    f32 = [c for c in K.WGRAD if c['rc'] == K.OK]
    nslab = {c['id']: K.slabs(c) for c in f32 if c['id'].startswith('reduce')}
    assert sorted(set(nslab.values())) == [124, 128, 160]
    assert all((n >= 128) == ('wgrad_reduce16_kernel' in c['kernels']) for c in f32 for n in [K.slabs(c)])
    for c in [c for c in f32 + K.WGRAD_BF16 if c['id'].startswith('S_below_items')]:
        items = c['B'] * -(-c['Lq'] // 128)
        assert K.slabs(c) == 32 < items
    # the S < items records at Lq = 1408 put two items of different batch entries into one slab: per = 2, 11 chunks per entry
    assert any(c['Lq'] == 1408 for c in f32) and any(c['Lq'] == 1408 for c in K.WGRAD_BF16)
