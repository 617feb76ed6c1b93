"""fp64 CPU definition of the generator's weight gradients (v2w_wgrad, v2w_wgrad_bf16) and the forward-error bound their GPU tests use.

The operation is stated through torch: dW of `F.conv1d` (u = 1) or `F.conv_transpose1d` (stride u, padding (k - u) / 2) applied to
act = leaky_relu(a * x + s), by fp64 autograd, permuted to the library's [k][C_in][C_out] - never through the kernels' phase and offset
tables.  The Conv1d pads (k - 1) / 2 * dil zeros on the left and (k - 1 - (k - 1) / 2) * dil on the right, so that dy has Lq positions: for odd
k that is `padding = dil * (k - 1) // 2`, for k = 4 the centre tap is tap 1.  tests/test_wgrad_ref_cpu.py pins it against an explicit loop
over (t, ci, co) and against central differences of the forward.

Every gradient comes with S, the same gradient of |act| against |dy|: the summed magnitudes of an entry's terms.  A sum of n terms done in
fp32 in any order is within n * 2^-24 * S of the exact one (disc_ref.sum_bound); the deterministic slab order only reorders the sum.
n = B * Lq, one more for the affine's fma and one for the slope's multiply (each moves every term by at most 2^-24 of itself).  No number here
was read off a kernel.

The bf16 entry's operands are the ones its header defines: act computed in fp32 and rounded once to bf16, dy rounded to bf16.  Products of
bf16 values are exact in fp32, so the same bound holds with n = B * Lq and S on the rounded operands - provided the reference rounds the SAME
fp32 activation: an operand that flips a bf16 tie is no summation error.  `draw_exact` therefore draws a and s on a 1/16 grid and keeps
|x| >= 2^-10; a * x + s is then exact in fp64 (`affine_f32` asserts it with a two-sum residual) and its rounding to fp32 is the kernel's fma."""
import numpy as np
import torch
import torch.nn.functional as F

from tests.disc_ref import f64, sum_bound, worst_ratio  # noqa: F401  (the bound and the comparison of the sibling files)

X_MIN = 2.0 ** -10


def draw_exact(rng, B, C, L):
    """x (B, C, L) float32 with |x| >= 2^-10, a in [0.75, 1.25] and s in [-0.5, 0.5] on the 1/16 grid, (B, C) float32."""
    x = rng.standard_normal((B, C, L), dtype=np.float32)
    x = np.where(np.abs(x) < X_MIN, np.copysign(np.float32(X_MIN), x), x).astype(np.float32)
    a = (rng.integers(12, 21, (B, C)) / 16.0).astype(np.float32)
    s = (rng.integers(-8, 9, (B, C)) / 16.0).astype(np.float32)
    return torch.from_numpy(x), torch.from_numpy(a), torch.from_numpy(s)


def affine_f32(x, a, s):
    """fl32(a * x + s), one rounding (the kernel's fmaf), from operands for which the fp64 value is exact; asserted, not assumed."""
    x, a, s = f64(x), f64(a)[:, :, None], f64(s)[:, :, None]
    m = a * 16.0
    assert torch.equal(m, m.round()) and m.abs().max().item() <= 32     # a = m / 16: the product has at most 6 + 24 significant bits
    p = a * x
    t = p + s
    bb = t - p
    assert ((p - (t - bb)) + (s - bb)).abs().max().item() == 0.0, 'a * x + s is not exact in fp64: the draw left its grid'
    return t.to(torch.float32)


def act_bf16(x, a, s, slope):
    """The activated signal as v2w_wgrad_bf16 stages it, bit for bit: fp32 fma (none without the affine), one fp32 multiply by the slope where
    !(v > 0), one rounding to bf16 (nearest even).  x: float32 or bfloat16 tensor.  -> float64 tensor of bf16 values."""
    v = x.to(torch.float32) if a is None else affine_f32(x.to(torch.float32), a, s)
    v = torch.where(v > 0, v, v * torch.tensor(np.float32(slope)))
    assert v.dtype == torch.float32
    return v.to(torch.bfloat16).to(torch.float64)


def act_f64(x, a, s, slope):
    """leaky_relu(a * x + s) in fp64 with the slope the kernel gets, float32(slope)."""
    z = f64(x) if a is None else f64(a)[:, :, None] * f64(x) + f64(s)[:, :, None]
    return F.leaky_relu(z, float(np.float32(slope)))


def forward(act, w, k, dil, u):
    """The layer whose weight gradient is wanted.  u = 1: w (C_out, C_in, k), Conv1d with the centre at tap (k - 1) / 2; u > 1: w (C_in, C_out, k),
    ConvTranspose1d of stride u and padding (k - u) / 2, its first u * Lq positions (all of them when k - u is even).  -> (B, C_out, u * Lq)."""
    if u == 1:
        c = (k - 1) // 2
        return F.conv1d(F.pad(act, (c * dil, (k - 1 - c) * dil)), w, None, dilation=dil)
    return F.conv_transpose1d(act, w, None, stride=u, padding=(k - u) // 2)[:, :, :u * act.shape[2]]       # (an odd k - u gives one position more than dy has)


def _dw(act, dy, k, dil, u):
    B, ci, Lq = act.shape
    co = dy.shape[1]
    w = torch.zeros((co, ci, k) if u == 1 else (ci, co, k), dtype=torch.float64, requires_grad=True)
    y = forward(act, w, k, dil, u)
    assert y.shape == dy.shape, (tuple(y.shape), tuple(dy.shape))
    g, = torch.autograd.grad(y, w, dy)
    return g.permute(2, 1, 0) if u == 1 else g.permute(2, 0, 1)          # -> [k][C_in][C_out]


def dw_of(act, dy, k, dil, u):
    """(dW [k][C_in][C_out], S) of the layer for the activated signal `act` and the cotangent `dy`, both fp64."""
    act, dy = f64(act), f64(dy)
    return _dw(act, dy, k, dil, u), _dw(act.abs(), dy.abs(), k, dil, u)


def wgrad(x, a, s, dy, k, dil, u, slope):
    """v2w_wgrad: (dW, S) in fp64 from the fp32 operands; a, s None: no affine."""
    return dw_of(act_f64(x, a, s, slope), dy, k, dil, u)


def wgrad_bf16(x, a, s, dy, k, dil, slope):
    """v2w_wgrad_bf16: (dW, S) in fp64 from the operands rounded the way the header states.  x, dy: float32 or bfloat16 tensors."""
    return dw_of(act_bf16(x, a, s, slope), dy.to(torch.bfloat16).to(torch.float64), k, dil, 1)


def chain(c):
    """n of a record, recomputed: B * Lq terms, plus (fp32 entry) one for the affine and one for slope != 1."""
    n = c['B'] * c['Lq']
    if 'stored' not in c:
        n += int(c['affine']) + int(np.float32(c['slope']) != np.float32(1))
    return n
