"""fp64 restatement of the spectral-norm entry points of include/vec2wav_hip.h (v2w_sn_step / v2w_sn_bwd), the bounds their GPU tests
use, and the one case list.

    step, training:  a = W^T u;  v' = a / max(||a||, 1e-12);  t = W v';  u' = t / max(||t||, 1e-12);  sigma = u' . t;  wf[j][c][o] = w[o][c][j] / sigma
    step, eval:      t = W v;  sigma = u . t;  wf as above (u, v untouched)
    backward:        dw[o][c][j] = dwf[j][c][o] / sigma - (sum(dwf . w) / sigma^2) u[o] v[c k + j]

evaluated in numpy float64 from the fp32 inputs as given.

The bounds.  The header lists every fp32 operation and, per quantity, the number n of roundings on the path to one entry (`counts`).  A
sum of terms done in fp32 with n roundings on the longest path is within n * 2^-24 * S of the exact sum, S the summed magnitudes of its
terms (the convention of tests/disc_ref.py).  The quantities here are chained - v' is a quotient of a sum and a norm of sums, t a sum
over v' - so each result carries E, its bound in units of u = 2^-24, built to first order from the header's counts alone:
    a sum  x = sum_i y_i z_i  with n roundings, y exact, z known to within E_z:   E_x = n * S + sum_i |y_i| E_z_i,  S = sum_i |y_i z_i|
    a square sum  q = sum x_i^2:   E_q = n * q + 2 sum |x_i| E_x_i;    r = sqrt(q):  E_r = E_q / (2 r) + r   (one rounding)
    a quotient  x / d:   E = E_x / d + |x / d| (E_d / d + 1);    max(r, eps) is eps exactly where r < eps (E = 0), else r
`step_ref` takes E of u and v on entry (zero for inputs the kernel reads as given), so two steps in a row are bounded by chaining.
None of this was read off a kernel.
"""
import math

import numpy as np

U = 2.0 ** -24
EPS = 1e-12
BAND, TILE = 64, 64


def cdiv(a, b):
    return -(-a // b)


def counts(R, N, vec=None):
    """The bracketed rounding counts of the header for an R x N matrix; vec: the 16-byte path (N % 4 == 0 on 16-byte aligned pointers)."""
    vec = (N % 4 == 0) if vec is None else vec
    nb, tiles = cdiv(R, BAND), cdiv(R, TILE) * cdiv(N, TILE)
    return dict(a=16 + 3 + nb - 1, q=cdiv(N, 1024) + 22, t=(cdiv(N, 256) + 8) if vec else (cdiv(N, 64) + 6), p=cdiv(R, 256) + 10,
                dot=26 + cdiv(tiles, 256) + 10, nb=nb, tiles=tiles)


def plan_ref(shapes):
    """The work split the header states for v2w_sn_plan: per layer (blk_t, blk_r, blk_s, ws_off, keep_off), then (grid_t, grid_r, grid_s,
    ws_bytes, keep_bytes)."""
    bt = br = bs = ws = keep = 0
    rows = []
    for co, ci, k in shapes:
        R, N = co, ci * k
        c = counts(R, N)
        rows.append((bt, br, bs, ws, keep))
        bt += c['nb'] * cdiv(N, 256)
        br += cdiv(R, 4)
        bs += c['tiles']
        ws += cdiv(max(c['nb'] * N + R, c['tiles']), 4) * 4
        keep += 4 + cdiv(R, 4) * 4 + cdiv(N, 4) * 4
    return rows, (bt, br, bs, ws * 4, keep * 4)


def _norm(x, Ex, n):
    q = float(x @ x)
    Eq = n * q + 2.0 * float(np.abs(x) @ Ex)
    r = math.sqrt(q)
    Er = (Eq / (2.0 * r) + r) if r > 0 else 0.0
    return (r, Er) if r > EPS else (EPS, 0.0)


def step_ref(w, u, v, training, Eu=None, Ev=None, vec=None):
    """w (C_out, C_in / groups, k), u (C_out,), v (C_in / groups * k,) -> dict(v, u, sigma, wf, E=dict(v, u, sigma, wf)) in float64."""
    co, ci, k = w.shape[:3]
    R, N = co, ci * k
    W = np.asarray(w, dtype=np.float64).reshape(R, N)
    A = np.abs(W)
    u = np.asarray(u, dtype=np.float64)
    v = np.asarray(v, dtype=np.float64)
    Eu = np.zeros(R) if Eu is None else Eu
    Ev = np.zeros(N) if Ev is None else Ev
    c = counts(R, N, vec)
    if training:
        a = W.T @ u
        Ea = c['a'] * (A.T @ np.abs(u)) + A.T @ Eu
        dn, Edn = _norm(a, Ea, c['q'])
        v = a / dn
        Ev = Ea / dn + np.abs(v) * (Edn / dn + 1.0)
    t = W @ v
    Et = c['t'] * (A @ np.abs(v)) + A @ Ev
    if training:
        du, Edu = _norm(t, Et, c['p'])
        u = t / du
        Eu = Et / du + np.abs(u) * (Edu / du + 1.0)
    sigma = float(u @ t)
    Es = c['p'] * float(np.abs(u) @ np.abs(t)) + float(np.abs(t) @ Eu) + float(np.abs(u) @ Et)
    wf = W.reshape(co, ci, k).transpose(2, 1, 0) / sigma
    Ewf = np.abs(wf) * (Es / abs(sigma) + 1.0)
    return dict(v=v, u=u, sigma=sigma, wf=wf, E=dict(v=Ev, u=Eu, sigma=Es, wf=Ewf))


def bwd_ref(dwf, w, u, v, sigma):
    """dwf [k][C_in / groups][C_out], w (C_out, C_in / groups, k), the kept u, v, sigma (read as given) -> (dw shaped like w, E).
    Roundings: g = dwf / sigma (1), uv = u v (1), coef = dot / (sigma sigma) (the dot's count and 2), the final fma (1, on |g| + |coef uv|):
    E = 2 |g| + |uv| (n_dot * S_dot / sigma^2 + 4 |coef|)."""
    co, ci, k = w.shape[:3]
    W = np.asarray(w, dtype=np.float64).reshape(co, ci, k)
    dW = np.asarray(dwf, dtype=np.float64).transpose(2, 1, 0)
    sigma = float(sigma)
    dot = float((dW * W).sum())
    Sdot = float(np.abs(dW * W).sum())
    coef = dot / (sigma * sigma)
    g = dW / sigma
    uv = np.outer(np.asarray(u, dtype=np.float64), np.asarray(v, dtype=np.float64)).reshape(co, ci, k)
    E = 2.0 * np.abs(g) + np.abs(uv) * (counts(co, ci * k)['dot'] * Sdot / (sigma * sigma) + 4.0 * abs(coef))
    return g - coef * uv, E


def worst_ratio(got, want, E):
    """max over the entries of |got - want| / (2^-24 E); 0 where they agree exactly."""
    d = np.abs(np.asarray(got, dtype=np.float64) - want)
    with np.errstate(divide='ignore', invalid='ignore'):
        r = np.where(d == 0, 0.0, d / (U * np.asarray(E, dtype=np.float64)))
    return float(np.max(r))


# ---- the case list: (C_out, C_in / groups, k)
def real_shapes():
    """The eight weight_orig shapes of the spectral-normed DiscriminatorS (DISC_S_LAYERS + DISC_S_POST): rows x row lengths 128 x 15,
    128 x 1312, 256 x 328, 512 x 656, 1024 x 1312, 1024 x 2624, 1024 x 5120, 1 x 3072."""
    from wavthruvec_pytorch_amd.synthetic import DISC_S_LAYERS, DISC_S_POST
    return [(co, ci // g, k) for ci, co, k, _s, g, _p in list(DISC_S_LAYERS) + [DISC_S_POST]]


# 1 x 3 (C_out = 1, a row shorter than a vector access), 3 x 7 (N = 3 mod 4), 17 x 15 (N = 3 mod 4, several taps and channels), 130 x 33
# (N = 1 mod 4, C_out over two bands / tiles and no multiple of the wave), 64 x 4 (one 16-byte access per row)
EDGE_SHAPES = [(1, 1, 3), (3, 1, 7), (17, 3, 5), (130, 11, 3), (64, 2, 2)]
SEED = 4711


def cases():
    return real_shapes() + EDGE_SHAPES


def make_case(shape, rng, scale=None):
    """fp32 (w, u, v, dwf) of one case: w uniform in +-1/sqrt(fan_in) as the modules initialise it (or +-scale), u and v unit vectors."""
    co, ci, k = shape
    bound = scale if scale is not None else 1.0 / math.sqrt(ci * k)
    w = rng.uniform(-bound, bound, size=(co, ci, k)).astype(np.float32)
    u = rng.standard_normal(co)
    v = rng.standard_normal(ci * k)
    u = (u / max(np.linalg.norm(u), EPS)).astype(np.float32)
    v = (v / max(np.linalg.norm(v), EPS)).astype(np.float32)
    dwf = (rng.standard_normal((k, ci, co)) * 10.0 ** rng.uniform(-3, 0, size=(k, ci, co))).astype(np.float32)
    return w, u, v, dwf
