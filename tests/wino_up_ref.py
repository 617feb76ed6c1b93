"""fp64 CPU statement of the upsampler form of the Winograd kernel (v2w_convt1d_wino_fwd, include/vec2wav_hip.h): the phase decomposition
of ConvTranspose1d(k = 2 u, stride u, padding u / 2), the weight stream the batched fold writes for it (v2w_fold_desc::wpw of a transposed
layer), and what each output entry may differ by.

Phase decomposition.  y[u t + p - pad] = w[p] x[t] + w[p + u] x[t - 1], t = 0 .. L, x[-1] = x[L] = 0: per phase p a two-tap conv with taps
(g0, g1) = (w[p + u], w[p]) on (x[t - 1], x[t]), i.e. ONE Conv1d over u * C_out rows (row = co * u + p) followed by a pixel shuffle.
Two-tap Winograd segment (csrc/v2w_wino.h), per output pair (t, t + 1), t even, with x0, x1, x2 = x[t - 1], x[t], x[t + 1]:
    M0 = G0 (x0 - x1)   M1 = G1 x1   M3 = G2 (x1 - x2)      G0, G1, G2 = g0, g0 + g1, g1
    z(t) = M0 + M1      z(t + 1) = M1 - M3
Stream.  3 * u * C_out * C_in floats in MFMA A-fragment order [32-row block][32-channel chunk][unit gg of 8 channels][term]: float
(((rb * nch + ch) * 12 + gg * 3 + term) * 64 + lane) * 4 + j holds G_term of row rb * 32 + lane % 32, channel ch * 32 + gg * 8 + 2 j + lane / 32.

Bound.  An entry is a chain of fp32 operations on the operands AS THE KERNEL ROUNDS THEM - the transformed weights G and the input
differences - so S is the sum of the magnitudes |G| * |x difference| of the terms that enter it, plus |bias|; n fp32 roundings on the
chain keep it within n * 2^-24 * S to first order (tests/disc_ref.sum_bound's form).  n = 2 C_in products per entry (two of M0, M1, M3) plus:
1 rounding of G1 = g0 + g1, 1 of the input difference, 2 of the staging (affine fma, leaky-relu multiply), 1 output transform, 1 bias.
"""
import numpy as np
import torch

from tests.disc_ref import f64

U24 = 2.0 ** -24
EXTRA_OPS = 6       # see above


def n_ops(c_in):
    return 2 * c_in + EXTRA_OPS


def rows_taps(w, u):
    """w [C_in][C_out][k = 2 u] -> (g0, g1), each [u * C_out][C_in], row = co * u + p: the taps on x[t - 1] and x[t]."""
    ci, co, k = w.shape
    assert k == 2 * u
    g0 = w[:, :, u:].permute(1, 2, 0).reshape(co * u, ci)
    g1 = w[:, :, :u].permute(1, 2, 0).reshape(co * u, ci)
    return g0, g1


def terms(w, u):
    """[3][u * C_out][C_in]: G0, G1, G2 in the dtype of w (fp32: G1 rounds as the fold rounds it)."""
    g0, g1 = rows_taps(w, u)
    return torch.stack([g0, g0 + g1, g1])


def _index(rows, ci):
    nrb, nch = rows // 32, ci // 32
    rb, ch, gg, term, lane, j = np.indices((nrb, nch, 4, 3, 64, 4))
    return term, rb * 32 + lane % 32, ch * 32 + gg * 8 + 2 * j + lane // 32


def stream_ref(w, u):
    """The stream of w (fp32 in, fp32 out, flat)."""
    T = terms(w.float(), u)
    term, row, c = _index(T.shape[1], T.shape[2])
    return T[torch.from_numpy(term), torch.from_numpy(row), torch.from_numpy(c)].reshape(-1).contiguous()


def stream_terms(stream, c_in, c_out, u):
    """The inverse of the layout: a flat stream -> [3][u * C_out][C_in]."""
    rows = u * c_out
    term, row, c = _index(rows, c_in)
    T = torch.zeros((3, rows, c_in), dtype=stream.dtype)
    T[torch.from_numpy(term), torch.from_numpy(row), torch.from_numpy(c)] = stream.reshape(term.shape)
    return T


def activate(x, slope=1.0, in_a=None, in_s=None):
    x = f64(x)
    if in_a is not None:
        x = f64(in_a)[:, :, None] * x + f64(in_s)[:, :, None]
    return x if slope == 1.0 else torch.where(x > 0, x, x * float(np.float32(slope)))


def convt_from_terms(T, act, u, bias=None):
    """The transposed conv evaluated the Winograd way from the terms T [3][u * C_out][C_in] and the activated signal act (B, C_in, L), fp64:
    -> (value, S), each (B, C_out, u * L).  S: per entry the summed magnitudes of the products that enter it (+ |bias|)."""
    T = f64(T)
    B, ci, L = act.shape
    rows = T.shape[1]
    co, pad = rows // u, u // 2
    npair = (L + 2) // 2                       # t = 0 .. L in pairs (2 P, 2 P + 1)
    xp = torch.zeros((B, ci, 2 * npair + 2), dtype=torch.float64)
    xp[:, :, 1:L + 1] = act                    # xp[i] = x[i - 1]
    x0, x1, x2 = xp[:, :, 0:2 * npair:2], xp[:, :, 1:2 * npair + 1:2], xp[:, :, 2:2 * npair + 2:2]

    def run(t0, t1, t3, d01, v1, d12, sign):
        M0, M1, M3 = torch.matmul(t0, d01), torch.matmul(t1, v1), torch.matmul(t3, d12)
        return M0 + M1, M1 + sign * M3
    za, zb = run(T[0], T[1], T[2], x0 - x1, x1, x1 - x2, -1.0)
    sa, sb = run(T[0].abs(), T[1].abs(), T[2].abs(), (x0 - x1).abs(), x1.abs(), (x1 - x2).abs(), 1.0)

    def shuffle(a, b):
        z = torch.stack([a, b], dim=-1).reshape(B, rows, 2 * npair)              # [row][t]
        z = z.reshape(B, co, u, 2 * npair).permute(0, 1, 3, 2).reshape(B, co, 2 * npair * u)      # [co][u t + p]
        return z[:, :, pad:pad + u * L]
    z, S = shuffle(za, zb), shuffle(sa, sb)
    if bias is not None:
        z, S = z + f64(bias)[None, :, None], S + f64(bias).abs()[None, :, None]
    return z, S
