"""fp64 restatement of the resampler (wavthruvec_pytorch_amd/audio.py, csrc/v2w_resample.hip) that shares no code with audio.py: every
coefficient comes straight from t(p, k) = (k / M - p / L) * base, per output sample, with no table and no k0.

    h(p, k) = sinc(pi t) cos^2(pi t / (2 lpw)) base / M  where |t| < lpw, else 0        base = min(M, L) * rolloff
    y[q L + p] = sum_k h(p, k) x[q M + k],  x = 0 outside [0, n);    N = ceil(L n / M)

It also holds the cases of the two test files and the bound: an output is a sum of NT products in fp32, by fma or not and in any order, so
|got - exact| <= nt * 2^-24 * sum_j |h_j x_j| with nt = NT + 1 against fp64 arithmetic on the kernel's own fp32 table, and NT + 2 against the
fp64 coefficients here (one more rounding per product: the table's cast to fp32)."""
import math

import numpy as np

U = 2.0 ** -24
LPW, ROLLOFF = 6, 0.99

# orig, new -> M, L, NT, min k0, max k0 + NT - 1 (the issue's table; the last two ratios list NT only)
TABLE = {(16000, 48000): (1, 3, 13, -6, 7), (16000, 24000): (2, 3, 13, -6, 8), (16000, 44100): (160, 441, 13, -6, 166),
         (16000, 22050): (320, 441, 13, -6, 326), (44100, 16000): (441, 160, 34, -16, 455), (48000, 16000): (3, 1, 37, -18, 18),
         (16000, 8000): (2, 1, 25, -12, 12), (8, 3): (8, 3, 33, -16, 22), (7, 5): (7, 5, 17, None, None), (5, 7): (5, 7, 13, None, None)}
# the ratios of the device tests: M : L as (orig, new)
RATIOS = [(1, 3), (2, 3), (3, 1), (2, 1), (160, 441), (441, 160), (8, 3), (7, 5)]


def rid(r):
    return '%dto%d' % r


def ratio(orig, new):
    g = math.gcd(orig, new)
    return orig // g, new // g


def coeff(p, k, M, L, lpw=LPW, rolloff=ROLLOFF):
    """h(p, k) for integer arrays p, k (broadcast), fp64."""
    base = min(M, L) * rolloff
    t = (np.asarray(k, dtype=np.float64) / M - np.asarray(p, dtype=np.float64) / L) * base
    with np.errstate(divide='ignore', invalid='ignore'):
        s = np.where(t == 0, 1.0, np.sin(np.pi * t) / (np.pi * t))
    return np.where(np.abs(t) < lpw, s * np.cos(np.pi * t / (2 * lpw)) ** 2 * base / M, 0.0)


def reach(M, L, lpw=LPW, rolloff=ROLLOFF):
    """An integer R with h(p, k) == 0 for every |k - M p / L| > R."""
    return int(math.ceil(lpw * M / (min(M, L) * rolloff))) + 1


def length(n, orig, new):
    M, L = ratio(orig, new)
    return -(-n * L // M)


def resample(x, orig, new, lpw=LPW, rolloff=ROLLOFF):
    """x (n,) fp64 -> (y (N,), S (N,)): the outputs and sum_k |h(p, k) x[q M + k]|, every coefficient from t(p, k)."""
    M, L = ratio(orig, new)
    x = np.asarray(x, dtype=np.float64)
    n = x.size
    N = length(n, orig, new)
    R = reach(M, L, lpw, rolloff)
    o = np.arange(N, dtype=np.int64)
    q, p = o // L, o % L
    k = (M * p) // L + np.arange(-R - 1, R + 2, dtype=np.int64)[:, None]           # (taps, N)
    h = coeff(p[None, :], k, M, L, lpw, rolloff)
    s = q[None, :] * M + k
    xs = np.where((s >= 0) & (s < n), x[np.clip(s, 0, n - 1)], 0.0)
    prod = h * xs
    return prod.sum(axis=0), np.abs(prod).sum(axis=0)


def apply_table(x, h, k0, M, L):
    """fp64 arithmetic on a GIVEN table (the kernel's fp32 one, say): x (n,) -> (y (N,), S (N,)), y[q L + p] = sum_j h[p][j] x[q M + k0[p] + j]."""
    x = np.asarray(x, dtype=np.float64)
    h = np.asarray(h, dtype=np.float64)
    n, NT = x.size, h.shape[1]
    N = -(-n * L // M)
    o = np.arange(N, dtype=np.int64)
    q, p = o // L, o % L
    s = q[None, :] * M + np.asarray(k0, dtype=np.int64)[p][None, :] + np.arange(NT, dtype=np.int64)[:, None]
    xs = np.where((s >= 0) & (s < n), x[np.clip(s, 0, n - 1)], 0.0)
    prod = h[p].T * xs
    return prod.sum(axis=0), np.abs(prod).sum(axis=0)


def bound(nt, S):
    return nt * U * np.asarray(S, dtype=np.float64)


def k0_closed(p, M, L, lpw=LPW, rolloff=ROLLOFF):
    """floor(M p / L - lpw M / base) + 1 in exact rational arithmetic (rolloff as the double it is)."""
    from fractions import Fraction
    base = min(M, L) * Fraction(rolloff)
    return math.floor(Fraction(M * p, L) - lpw * M / base) + 1


def nt_closed(M, L, lpw=LPW, rolloff=ROLLOFF):
    from fractions import Fraction
    return math.ceil(2 * lpw * M / (min(M, L) * Fraction(rolloff)))


def lengths_for(M, L, NT, tile):
    """Input lengths n of the device cases of one ratio: 1, NT - 1, the smallest n whose N = ceil(L n / M) is tile - 1, tile, tile + 1 and
    2 tile + 3 (or the first N past it that some n gives), and one that is no multiple of 4."""
    def n_of(N):                       # the smallest n with ceil(L n / M) >= N
        return max(1, -(-((N - 1) * M + 1) // L))
    ns = [1, max(NT - 1, 2)] + [n_of(N) for N in (tile - 1, tile, tile + 1, 2 * tile + 3)]
    odd = n_of(tile // 2) | 1
    ns.append(odd if odd % 4 else odd + 2)
    return sorted(set(ns))


def signal(seed, n, i16=False):
    """Seeded noise with a slow sine under it: float32 in about [-1, 1], or int16 PCM."""
    rng = np.random.default_rng(seed)
    x = 0.4 * rng.standard_normal(n) + 0.3 * np.sin(np.arange(n) * 0.01 + seed)
    if i16:
        return np.clip(np.round(x * 12000.0), -32768, 32767).astype(np.int16)
    return x.astype(np.float32)


def f64_of(x):
    """The samples the kernel reads: int16 PCM as x / 32768 (exact), float32 as it is."""
    x = np.asarray(x)
    return x.astype(np.float64) / 32768.0 if x.dtype == np.int16 else x.astype(np.float64)
