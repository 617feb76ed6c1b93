"""fp64 restatement of the AdamW step of include/vec2wav_hip.h (v2w_adamw_multi) and the bound its tests use.

    p  <- p * (1 - lr*wd)
    m  <- m + (1-b1)*(g - m)
    v  <- b2*v + (1-b2)*g*g
    p  <- p - (lr / bias_corr1) * m / (sqrt(v)/bias_corr2_sqrt + eps)

evaluated in numpy float64 from the inputs as given (fp32 tensors and the fp32-rounded hyperparameter struct for the kernel tests; fp64
ones for the pin against torch).  `adamw_ref` also returns, per entry, the magnitudes the bound is built from.

The bound.  The header states the kernel's operations: every one a correctly rounded fp32 operation, ROUNDINGS[k] of them on the path of
output k (m': 3, v': 4, p': 15), and to first order |m' - exact| <= 3u (|m| + |g|), |v' - exact| <= 4u (|v| + g g),
|p' - exact| <= 15u (|p| + step (|m| + |g|) / den), u = 2^-24.  The tests allow twice that (the second-order terms, and the fp64 evaluation
itself): c = 2 * ROUNDINGS[k].  A c above 32 would mean the kernel does something its header does not say.
"""
from types import SimpleNamespace

import numpy as np

ROUNDINGS = {'p': 15, 'm': 3, 'v': 4}
U32 = 2.0 ** -24
U64 = 2.0 ** -53
ALTERATIONS = ('no_decay', 'no_bias_corr', 'eps_in_sqrt', 'l2_decay')


def make_hyper(*, lr, betas, eps, weight_decay, step, dtype=np.float32):
    """The fields of v2w_adamw_hyper for step number `step`: the bias corrections in double, everything rounded once to `dtype`."""
    b1, b2 = float(betas[0]), float(betas[1])
    f = dtype
    return SimpleNamespace(lr=f(lr), beta1=f(b1), beta2=f(b2), eps=f(eps), weight_decay=f(weight_decay),
                           bias_corr1=f(1.0 - b1 ** step), bias_corr2_sqrt=f((1.0 - b2 ** step) ** 0.5))


def adamw_ref(p, g, m, v, h, alter=None):
    """(p', m', v', mags) in float64.  `alter`: one of ALTERATIONS - a deliberately wrong step (what the bound must be able to see)."""
    assert alter is None or alter in ALTERATIONS
    p, g, m, v = (np.asarray(x, dtype=np.float64) for x in (p, g, m, v))
    lr, b1, b2, eps, wd = (float(x) for x in (h.lr, h.beta1, h.beta2, h.eps, h.weight_decay))
    bc1, bc2s = float(h.bias_corr1), float(h.bias_corr2_sqrt)
    if alter == 'no_bias_corr':
        bc1 = bc2s = 1.0
    if alter == 'l2_decay':
        g = g + wd * p
    p1 = p if alter == 'no_decay' else p * (1.0 - lr * wd)
    m1 = m + (1.0 - b1) * (g - m)
    v1 = b2 * v + (1.0 - b2) * g * g
    den = (np.sqrt(v1 + eps) / bc2s) if alter == 'eps_in_sqrt' else (np.sqrt(v1) / bc2s + eps)
    step = lr / bc1
    upd = step * m1 / den
    mg = np.abs(m) + np.abs(g)
    mags = dict(p=np.abs(p), update=np.abs(upd), mg=mg, vg=np.abs(v) + g * g, update_mag=step * mg / den)
    return p1 - upd, m1, v1, mags


def bounds(mags, u=U32):
    """Per-entry bounds on |p' - ref|, |m' - ref|, |v' - ref| (see the module docstring); `update_mag` >= `update` stands for the update
    with |m| + |g| in place of m', which the rounding errors of m' scale with when m and g cancel."""
    c = {k: 2 * n for k, n in ROUNDINGS.items()}
    assert max(c.values()) <= 32
    return dict(p=c['p'] * u * (mags['p'] + mags['update_mag']), m=c['m'] * u * mags['mg'], v=c['v'] * u * mags['vg'])


# ---- the inputs of the kernel tests (tests/test_optim_gpu.py) and of the CPU check that the bound can tell a wrong step from a right one
# lr and weight_decay are larger than the reference's (2e-4, 0.01): at |p| ~ 1 the reference's decay term lr*wd*|p| = 2e-6 is 30 ulps of
# p, below 100 x the bound (100 * 30 * 2^-24 = 1.8e-4 relative); 1e-2 * 0.1 = 1e-3 is 5 times above it.  eps = 1e-6 and gradients down to
# 1e-4 make "eps inside the square root" visible (sqrt(v + eps) against sqrt(v) + eps where v ~ eps).
KERNEL_HYPER = dict(lr=1e-2, betas=(0.8, 0.99), eps=1e-6, weight_decay=0.1)
KERNEL_STEPS = (1, 1000)
KERNEL_SEED = 20240


def kernel_state(numel, rng):
    """Random fp32 (p, g, m, v) of one tensor: scales drawn per entry over two to four orders of magnitude, v >= 0."""
    def scaled(lo, hi):
        return rng.standard_normal(numel) * 10.0 ** rng.uniform(lo, hi, numel)
    p = scaled(-2, 0)
    g = scaled(-4, 0)
    m = scaled(-4, 0)
    v = scaled(-4, 0) ** 2
    return tuple(x.astype(np.float32) for x in (p, g, m, v))


def worst_ratio(got, want, bnd):
    """max over the entries and the three outputs of |got - want| / bound."""
    worst = 0.0
    for k, (a, b) in zip('pmv', zip(got, want)):
        d = np.abs(np.asarray(a, dtype=np.float64) - b)
        with np.errstate(divide='ignore', invalid='ignore'):
            r = np.where(d == 0, 0.0, d / bnd[k])
        worst = max(worst, float(r.max()))
    return worst


def kernel_cases(max_items, min_chunk_units=2048):
    """[(numel, kind)] of the kernel test's tensor list: every stepped tensor is one item of ONE call of max_items + 3 items (two launches).
    kind: 'plain'; 'p_view' / 'g_view' (the parameter / the gradient is a [1:] view: 4-byte phase on that pointer only); 'all_view' (all
    four are: a shared phase, 16-byte accesses behind a partial first unit); 'g_strided' (a non-contiguous gradient); 'no_grad' (grad is
    None: not an item, must stay untouched)."""
    cases = [(n, 'plain') for n in (1, 3, 4, 5, 1023)]
    cases.append((2 * min_chunk_units * 4 + 5, 'plain'))        # three workgroups, ends off a 16-byte line
    cases += [(777, 'p_view'), (1030, 'g_view'), (1029, 'all_view'), (6 * 35, 'g_strided'), (64, 'no_grad')]
    stepped = sum(k != 'no_grad' for _, k in cases)
    cases += [(2 + i % 7, 'plain') for i in range(max_items + 3 - stepped)]
    return cases
