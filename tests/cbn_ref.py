"""fp64 CPU statements of what the entry points of csrc/v2w_cbn.hip compute (include/vec2wav_hip.h, oracle/vec2wav_oracle.py), and the
forward-error bounds their GPU tests use (tests/test_cbn_kernels_gpu.py).  Numpy float64 throughout; exact rationals where a variance cancels.

Every sum returns S with its value, the summed magnitudes of its terms: n fp32 roundings on an entry's chain keep it within n * 2^-24 * S.
The chain is cut at every buffer a call leaves in memory (z_ws, the new v, sigma_ws, stats, slices), so that each bound is one summation
bound plus first-order propagation of bounds already computed; the n of every chain is counted in tests/cbn_cases.py.  None of these
bounds was read off a kernel.  tests/test_cbn_ref_cpu.py pins the values against F.linear, the oracle's spectral_norm_weight,
F.batch_norm and the oracle's batch_norm_no_affine."""
from fractions import Fraction

import numpy as np

U = 2.0 ** -24            # fp32 unit roundoff
U64 = 2.0 ** -53          # fp64


def f64(x):
    return np.asarray(x.detach().cpu().numpy() if hasattr(x, 'detach') else x, dtype=np.float64)


def worst_ratio(got, want, bound):
    """max |got - want| / bound over the entries (0 / 0 counts as 0, x / 0 as inf, a non-finite `got` as inf)."""
    got, want, bound = np.asarray(got, dtype=np.longdouble), np.asarray(want, dtype=np.longdouble), np.asarray(bound, dtype=np.longdouble)
    err = np.abs(got - want)
    with np.errstate(divide='ignore', invalid='ignore'):
        r = np.where(err == 0, 0.0, err / bound)
    r = np.where(np.isfinite(got), r, np.inf)
    return float(r.max()) if r.size else 0.0


# ---------------------------------------------------------------------------------------------------------------
# conditioning: z, the power iteration, sigma, [gamma | beta]
def linear(x, w, b=None):
    """x (B, D), w (J, D), b (J) -> (x w^T + b, S), both (B, J)."""
    x, w = f64(x), f64(w)
    val, S = x @ w.T, np.abs(x) @ np.abs(w).T
    if b is not None:
        val, S = val + f64(b), S + np.abs(f64(b))
    return val, S


def cond_z(spk, noise, fc_w, fc_b):
    """z = fcs(cat(spk, noise)); without an fcs layer the input itself (S = 0: a copy)."""
    sn = f64(spk) if noise is None else np.concatenate([f64(spk), f64(noise)], 1)
    if fc_w is None:
        return sn, np.zeros_like(sn)
    return linear(sn, fc_w, fc_b)


def quotient(p, dp, q, dq, roundings=1):
    """p / q with |error of p| <= dp, |error of q| <= dq, to first order: (dp + |p / q| dq) / |q| + roundings * 2^-24 |p / q|."""
    r = p / q
    return r, (dp + np.abs(r) * dq) / np.abs(q) + roundings * U * np.abs(r)


def norm(p, dp, n):
    """sqrt(sum p^2) of a vector whose entries carry the bounds dp, the squares summed in fp32 on a chain of n, one rounding for the root."""
    n2 = float((p * p).sum())
    dn2 = float((2 * np.abs(p) * dp + dp * dp).sum()) + n * U * n2
    q = np.sqrt(n2)
    return q, dn2 / (2 * q) + U * q


def sn_new_v(W, u, n_col, n_sq):
    """v = normalize(W^T u): (v, bound).  The kernel multiplies by the rounded reciprocal of the norm: two roundings."""
    W, u = f64(W), f64(u)
    col, S = W.T @ u, np.abs(W).T @ np.abs(u)
    dcol = n_col * U * S
    q, dq = norm(col, dcol, n_sq)
    return quotient(col, dcol, q, dq, 2)


def sn_wv(W, v, n_row):
    W, v = f64(W), f64(v)
    return W @ v, n_row * U * (np.abs(W) @ np.abs(v))


def sn_new_u(W, v, n_row, n_sq):
    """u = normalize(W v) for the v in memory: (u, bound, W v, its bound)."""
    wv, dwv = sn_wv(W, v, n_row)
    q, dq = norm(wv, dwv, n_sq)
    u, du = quotient(wv, dwv, q, dq, 2)
    return u, du, wv, dwv


def sn_sigma(u, du, wv, dwv, n):
    """sigma = u . (W v): (value, bound); in eval mode u is the stored vector, du = 0."""
    u = f64(u)
    return float(u @ wv), float((du * np.abs(wv) + np.abs(u) * dwv).sum()) + n * U * float(np.abs(u * wv).sum())


def gamma_beta(W, b, z, sigma, n_row, dz=None):
    """[gamma | beta] = (W z) / sigma + b for the z (B, 128) and sigma given (sigma exact: the one in memory): (value, bound), (B, R).
    dz: a bound on z, propagated through the row sum."""
    W, z = f64(W), f64(z)
    row, S = z @ W.T, np.abs(z) @ np.abs(W).T
    drow = n_row * U * S + (0.0 if dz is None else dz @ np.abs(W).T)
    g, dg = quotient(row, drow, float(sigma), 0.0)
    val = g + f64(b)
    return val, dg + U * np.abs(val)


def affine_eval(gb, dgb, rm, rv, eps):
    """a = gamma / sqrt(running_var + eps), s = beta - a * running_mean from [gamma | beta] (B, 2C) with bound dgb: one rounding each for
    rstd (the cast of an fp64 value), the product and the fma.  -> (a, da, s, ds)."""
    C = gb.shape[1] // 2
    rm, rv = f64(rm), f64(rv)
    rstd = 1.0 / np.sqrt(rv + float(np.float32(eps)))
    drstd = (U + 4 * U64) * rstd
    a = gb[:, :C] * rstd
    da = dgb[:, :C] * rstd + np.abs(gb[:, :C]) * drstd + U * np.abs(a)
    s = gb[:, C:] - a * rm
    return a, da, s, dgb[:, C:] + da * np.abs(rm) + U * np.abs(s)


# ---------------------------------------------------------------------------------------------------------------
# sums
def channel_sums(x):
    """x (B, C, L) -> (sum, sum of squares, sum of magnitudes) per channel."""
    x = f64(x)
    return x.sum((0, 2)), (x * x).sum((0, 2)), np.abs(x).sum((0, 2))


def stats_bound(n, B, S):
    """v2w_bn_stats: n fp32 roundings per lane and batch item, then fp64: 64 B partial sums and splits added."""
    return (n * U + 64 * B * U64) * S


def row_sums(part):
    """part (ntiles, C, 2) float32 -> (sums (2, C): [sum | sumsq], their summed magnitudes), in extended precision: an fp64 sum of the rows in any
    order is within ntiles * 2^-53 * magnitudes of it (the conversion of a float is exact)."""
    p = np.asarray(part).astype(np.longdouble)
    return p.sum(0).T, np.abs(p).sum(0).T


def slice_sums(part, nslices):
    """slices[s][stat][c]: rows [ntiles s / nslices, ntiles (s + 1) / nslices) of part, an empty slice exactly 0 -> (sums, magnitudes), (nslices, 2, C)."""
    nt = part.shape[0]
    out = np.zeros((nslices, 2, part.shape[1]), dtype=np.longdouble)
    mag = np.zeros_like(out)
    for s in range(nslices):
        lo, hi = nt * s // nslices, nt * (s + 1) // nslices
        if hi > lo:
            out[s], mag[s] = row_sums(part[lo:hi])
    return out, mag


# ---------------------------------------------------------------------------------------------------------------
# finalisation
def finalize(s1, s2, count, gb, rm, rv, momentum, eps, ds1=0.0, ds2=0.0):
    """v2w_bn_finalize(training) / _finalize_slices / the second half of _reduce_finalize from the sums s1, s2 (C) as given (fp64 values taken
    exactly: mean and variance in rationals), gb (B, 2C), the old running statistics -> dict of (value, bound) for a, s, rm, rv.
    ds1, ds2: bounds on the sums themselves when they are not the ones in memory.

    The kernels compute var = s2 / count - mean^2 in fp64: with M = max(E[x^2], mean^2) the two quotients, the square and the difference lose
    at most 5 * 2^-53 * M, i.e. kappa * 5 * 2^-53 relative to var + eps, kappa = M / (var + eps) - carried here from the record's data.  The
    clamp at 0 is 1-Lipschitz.  On top: rstd's cast, gamma * rstd, (float)mean, the fma, the cast of each running statistic."""
    m, e = float(np.float32(momentum)), float(np.float32(eps))
    Cn = len(s1)
    mean, var, M = np.empty(Cn), np.empty(Cn), np.empty(Cn)
    for c in range(Cn):
        mq = Fraction(float(s1[c])) / Fraction(count)
        e2 = Fraction(float(s2[c])) / Fraction(count)
        vq = e2 - mq * mq
        mean[c], var[c], M[c] = float(mq), float(max(vq, Fraction(0))), float(max(e2, mq * mq))
    dmean = ds1 / count
    dvar = 5 * U64 * M + ds2 / count + 2 * np.abs(mean) * dmean
    rstd = 1.0 / np.sqrt(var + e)
    drstd = rstd * (0.5 * dvar / (var + e) + 3 * U64 + U)
    gb, rm, rv = f64(gb), f64(rm), f64(rv)
    gamma, beta = gb[:, :Cn], gb[:, Cn:]
    a = gamma * rstd
    da = np.abs(gamma) * drstd + U * np.abs(a)
    s = beta - a * mean
    ds = da * np.abs(mean) + np.abs(a) * (np.abs(mean) * (U + U64) + dmean) + U * np.abs(s)
    f = count / (count - 1.0) if count > 1 else 1.0
    unb = var * f
    dunb = (dvar + 3 * U64 * var) * f
    new_rm = (1 - m) * rm + m * mean
    new_rv = (1 - m) * rv + m * unb
    d_rm = U * np.abs(new_rm) + 4 * U64 * (np.abs(rm) + np.abs(mean)) + m * (dmean + U64 * np.abs(mean))
    d_rv = U * np.abs(new_rv) + 4 * U64 * (np.abs(rv) + unb) + m * dunb
    return dict(a=(a, da), s=(s, ds), rm=(new_rm, d_rm), rv=(new_rv, d_rv), kappa=M / (var + e), mean=mean, var=var)


def finalize_eval(gb, rm, rv, eps):
    """v2w_bn_finalize(training = 0): the running statistics as they are."""
    gb = f64(gb)
    a, da, s, ds = affine_eval(gb, np.zeros_like(gb), rm, rv, eps)
    return dict(a=(a, da), s=(s, ds))


def one_pass_loss_bound(kappa, n):
    """How far rstd from fp32-accumulated sums (each within n * 2^-24 of its magnitudes) may lie from the two-pass value, relative: the
    variance loses 3 n 2^-24 E[x^2] (sumsq once, the mean twice), rstd half of that over var + eps."""
    return 1.5 * kappa * n * U


def affine_apply(x, a, s):
    """out = a[b, c] * x + s[b, c]: one fma per element -> (out, bound)."""
    out = f64(a)[:, :, None] * f64(x) + f64(s)[:, :, None]
    return out, U * np.abs(out)
