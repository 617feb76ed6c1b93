"""fp64 CPU definitions of the operations behind the discriminator entry points (csrc/v2w_disc.hip, v2w_wgrad_slice / v2w_wgrad_groups and
the conv forms the MPD / MSD path feeds to v2w_conv1d_fwd), and the forward-error bounds their GPU tests use.

Every function states its operation with reshapes, pads and strided slices of whole axes - never with the kernels' flat-index arithmetic -
and the backward operations are torch autograd through those statements.  tests/test_disc_ref_cpu.py pins each of them against an
independent statement (F.conv1d with a stride, F.conv2d with a (k, 1) kernel, F.avg_pool1d, F.pad + unfold, oracle/disc_oracle.py).

Tensors are "logical": (B, C, L, inner) views without row pitches.  `pitched` / `unpitched` move between them and the (B, C, pitch) buffers
the entry points read and write.  Every sum also returns S, the sum of the magnitudes of its terms per output entry: a sum of n terms done
in fp32 in any order is within n * 2^-24 * S of the exact one (`sum_bound`), and none of these bounds was read off a kernel.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -24           # fp32 unit roundoff


def f64(t):
    if isinstance(t, np.ndarray):
        t = torch.from_numpy(t)
    return t.detach().to(torch.float64)


# ---------------------------------------------------------------------------------------------------------------
# row pitches
def pitched(x, pitch, fill=0.0):
    """(..., L, inner) or (..., n) logical rows -> (..., pitch) rows whose tail [n, pitch) holds `fill`."""
    rows = x.reshape(*x.shape[:-2], -1) if x.dim() >= 4 else x
    out = torch.full((*rows.shape[:-1], pitch), fill, dtype=x.dtype)
    out[..., :rows.shape[-1]] = rows
    return out


def unpitched(buf, L, inner):
    """(B, C, pitch) -> (B, C, L, inner): the valid part of every row."""
    return buf[..., :L * inner].reshape(*buf.shape[:-1], L, inner)


# ---------------------------------------------------------------------------------------------------------------
# movement
def phase_split(x, Cg, s):
    """x (B, C, L, inner) -> (B, s*C, U, inner), U = ceil(L / s): within each group of Cg channels the s phases x[..., r::s, :] are stacked
    phase-major (phase r of the group's channel j is the group's channel r*Cg + j); positions past L read 0."""
    B, C, L, inner = x.shape
    Uq = -(-L // s)
    xp = F.pad(x, (0, 0, 0, s * Uq - L))
    return xp.reshape(B, C // Cg, Cg, Uq, s, inner).permute(0, 1, 4, 2, 3, 5).reshape(B, s * C, Uq, inner)


def phase_merge(xs, Cg, s, L):
    """The inverse of `phase_split` on the valid part: xs (B, s*C, U, inner) -> (B, C, L, inner)."""
    B, sC, Uq, inner = xs.shape
    C = sC // s
    return xs.reshape(B, C // Cg, s, Cg, Uq, inner).permute(0, 1, 3, 4, 2, 5).reshape(B, C, Uq * s, inner)[:, :, :L]


def reflect_rows(x, H, inner):
    """x (B, T) -> (B, H, inner): reflect pad on the right up to H*inner samples (the reference's DiscriminatorP.forward), read as rows."""
    B, T = x.shape
    n = H * inner - T
    assert 0 <= n < T
    xp = torch.cat((x, x[:, T - 1 - n:T - 1].flip(1)), dim=1) if n else x
    return xp.reshape(B, H, inner)


def _shifted_rows(x2, s, k, pad, Uq):
    """x2 (B, C, H, inner) -> (B, k, C, Uq, inner): entry [j][u] is row s*u + j - pad of x2, zero outside [0, H)."""
    xz = F.pad(x2, (0, 0, pad, pad + s))
    return torch.stack([xz[:, :, j:j + s * (Uq - 1) + 1:s] for j in range(k)], dim=1)


def unfold1(x, H, inner, s, k, pad, rows):
    """x (B, T) -> (B, rows, U, inner), U = (H + 2 pad - k)/s + 1: row j < k holds rows s*u + j - pad of the reflect-padded (H, inner) view
    (zero rows outside [0, H)); rows k .. rows-1 are zero."""
    Uq = (H + 2 * pad - k) // s + 1
    sh = _shifted_rows(reflect_rows(x, H, inner).unsqueeze(1), s, k, pad, Uq)[:, :, 0]
    return F.pad(sh, (0, 0, 0, 0, 0, rows - k))


def fold1(dxu, T, H, inner, s, k, pad):
    """Backward of `unfold1`: dxu (B, rows, U, inner) -> (dx (B, T), S), fp64 autograd through the definition; S is the same map on |dxu|
    (unfold1 only copies, so its adjoint only adds)."""
    dxu = f64(dxu)
    x = torch.zeros(dxu.shape[0], T, dtype=torch.float64, requires_grad=True)
    y = unfold1(x, H, inner, s, k, pad, dxu.shape[1])
    dx, = torch.autograd.grad(y, x, dxu, retain_graph=True)
    S, = torch.autograd.grad(y, x, dxu.abs())
    return dx, S


def unfold_taps(x, s, k, pad):
    """x (B, C, L, inner) -> (B, k*C, U, inner), U = (L + 2 pad - k)/s + 1: channel j*C + c holds rows s*u + j - pad of channel c (0 outside)."""
    B, C, L, inner = x.shape
    Uq = (L + 2 * pad - k) // s + 1
    return _shifted_rows(x, s, k, pad, Uq).reshape(B, k * C, Uq, inner)


def zero_tail(x, valid):
    """x (rows, pitch): [valid, pitch) of every row set to 0, the rest kept."""
    out = x.clone()
    out[:, valid:] = 0
    return out


def _avgpool4(x):
    Lo = x.shape[1] // 2 + 1
    xp = F.pad(x, (2, 2 + 2))
    win = torch.stack([xp[:, j:j + 2 * (Lo - 1) + 1:2] for j in range(4)], dim=0)
    return win.sum(0) / 4, win.abs().sum(0) / 4


def avgpool4(x):
    """AvgPool1d(4, 2, padding=2), the zero padding counted: x (B, L) -> (out (B, L/2 + 1), S)."""
    return _avgpool4(f64(x))


def avgpool4_bwd(dout, L):
    """Backward of `avgpool4` by autograd: dout (B, L/2 + 1) -> (dx (B, L), S)."""
    dout = f64(dout)
    x = torch.zeros(dout.shape[0], L, dtype=torch.float64, requires_grad=True)
    y, _ = _avgpool4(x)
    dx, = torch.autograd.grad(y, x, dout, retain_graph=True)
    S, = torch.autograd.grad(y, x, dout.abs())
    return dx, S


# ---------------------------------------------------------------------------------------------------------------
# dz = (g + d) * lrelu'(f) and its sums
def dz(f, g, d, slope):
    """fp64 dz = (g + d) * (f > 0 ? 1 : slope); g or d None counts as 0.  f is the ACTIVATED map: +0, -0 and NaN take the slope."""
    f = f64(f)
    v = torch.zeros_like(f)
    if d is not None:
        v = v + f64(d)
    if g is not None:
        v = v + f64(g)
    return v * torch.where(f > 0, torch.ones_like(f), torch.full_like(f, float(np.float32(slope))))


def dz_f32(f, g, d, slope):
    """The same value as the two fp32 operations the header states, in numpy float32: one add, then one multiply where !(f > 0).
    slope == 1 multiplies nothing."""
    f = np.asarray(f, dtype=np.float32)
    v = np.zeros_like(f)
    if d is not None:
        v = np.asarray(d, dtype=np.float32).copy()
    if g is not None:
        v = (v + np.asarray(g, dtype=np.float32)).astype(np.float32)
    if np.float32(slope) != np.float32(1):
        v = np.where(f > 0, v, (v * np.float32(slope)).astype(np.float32))
    return v.astype(np.float32)


def dz_merge_d(dxs, Cg, s, L):
    """d of the merged form: the phase-stacked gradient dxs (B, s*C, U, inner) of the strided layer above, merged back to (B, C, L, inner)."""
    return phase_merge(dxs, Cg, s, L)


def rowsum(dzv):
    """(..., n) -> (sum over the row, S = sum of magnitudes), fp64."""
    dzv = f64(dzv)
    return dzv.sum(-1), dzv.abs().sum(-1)


def rowsum_reduce_f32(rs):
    """rs (B, C) float32 -> db (C,) float32: the sequential fp64 sum over b in the order b = 0, 1, ..., rounded once."""
    rs = np.asarray(rs, dtype=np.float32)
    acc = np.zeros(rs.shape[1], dtype=np.float64)
    for b in range(rs.shape[0]):
        acc = acc + rs[b].astype(np.float64)
    return acc.astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------
# Conv1d with taps at (t - tap0)*dil and explicit zero padding
def _conv(x, w, bias, dil, tap0):
    # one matrix product per tap on the explicitly padded signal (tests/test_disc_ref_cpu.py pins it against F.conv1d / F.conv2d)
    k, L = w.shape[2], x.shape[2]
    xp = F.pad(x, (tap0 * dil, (k - 1 - tap0) * dil))
    out = sum(torch.matmul(w[:, :, t], xp[:, :, t * dil:t * dil + L]) for t in range(k))
    return out if bias is None else out + bias[None, :, None]


def wf_to_w(wf):
    """[k][C_in][C_out] (the library's layout) -> torch's (C_out, C_in, k)."""
    return wf.permute(2, 1, 0).contiguous()


def conv(x, wf, bias, dil, tap0, out_slope=0.0):
    """out[b][o][l] = lrelu_{out_slope}(bias[o] + sum_{t,c} wf[t][c][o] x[b][c][l + (t - tap0)*dil]), x zero outside [0, L): (out, S) in fp64.
    out_slope == 0 stores the sum itself.  S counts |bias| as a term."""
    x, w = f64(x), wf_to_w(f64(wf))
    b = None if bias is None else f64(bias)
    z = _conv(x, w, b, dil, tap0)
    S = _conv(x.abs(), w.abs(), None if b is None else b.abs(), dil, tap0)
    if out_slope:
        z = F.leaky_relu(z, float(np.float32(out_slope)))
    return z, S


def conv_groups(x, wf4, bias, dil, tap0, out_slope=0.0):
    """Grouped form: x (B, G*cig, L), wf4 [G][k][cig][cog], bias (G*cog) -> (B, G*cog, L); group g reads the channel slice g of x."""
    G, _, cig, cog = wf4.shape
    outs = [conv(x[:, g * cig:(g + 1) * cig], wf4[g], None if bias is None else bias[g * cog:(g + 1) * cog], dil, tap0, out_slope)
            for g in range(G)]
    return torch.cat([o for o, _ in outs], 1), torch.cat([s for _, s in outs], 1)


def conv_grads(x, wf, dy, dil, tap0):
    """Input and weight gradient of `conv` (no activation) for the cotangent dy, by fp64 autograd through the same conv:
    (dx, S_dx, dwf, S_dwf), the weight gradient in the [k][C_in][C_out] layout.  The conv is bilinear, so the magnitudes' sums are the same
    gradients of conv(|x|, |w|) for |dy|."""
    x, w, dy = f64(x).requires_grad_(True), wf_to_w(f64(wf)).requires_grad_(True), f64(dy)
    dx, dw = torch.autograd.grad(_conv(x, w, None, dil, tap0), (x, w), dy)
    xa, wa = x.detach().abs().requires_grad_(True), w.detach().abs().requires_grad_(True)
    Sx, Sw = torch.autograd.grad(_conv(xa, wa, None, dil, tap0), (xa, wa), dy.abs())
    return dx, Sx, dw.permute(2, 1, 0), Sw.permute(2, 1, 0)


def transpose_flip(wf):
    """[k][C_in][C_out] -> [k][C_out][C_in] with the taps reversed: the weights with which the input gradient is the forward conv of dy
    at tap0' = k - 1 - tap0."""
    return wf.flip(0).transpose(1, 2).contiguous()


# ---------------------------------------------------------------------------------------------------------------
# bounds
def sum_bound(n, S):
    """|fp32 sum - exact sum| <= n * 2^-24 * S for n terms of summed magnitude S (any order; products rounded with their adds)."""
    return n * U * S


def worst_ratio(got, want, bound):
    """max over entries of |got - want| / bound (0/0 counts as 0, x/0 as inf, a non-finite `got` as inf): <= 1 means the bound holds everywhere."""
    got, want = f64(got), f64(want)
    err = (got - want).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound)
    ratio = torch.where(torch.isfinite(got), ratio, torch.full_like(ratio, float('inf')))
    return ratio.max().item() if ratio.numel() else 0.0


def ceil_div(a, b):
    return -(-a // b)


def roundup4(n):
    return (n + 3) // 4 * 4


def rows_kernel_quotient(rem, inner):
    """The fp32 estimate-and-correct division of phase_split_rows_kernel, evaluated in numpy float32 on an int array `rem`:
    inv = float32(1)/float32(inner); u = int(float32(rem) * inv); one step down if u*inner > rem, else one step up if (u+1)*inner <= rem."""
    rem = np.asarray(rem, dtype=np.int64)
    if inner == 1:
        return rem.copy()
    inv = np.float32(1) / np.float32(inner)
    u = (rem.astype(np.float32) * inv).astype(np.float32).astype(np.int64)
    down = u * inner > rem
    up = ~down & ((u + 1) * inner <= rem)
    return u - down.astype(np.int64) + up.astype(np.int64)


assert math.isclose(U, 5.9604644775390625e-08)
