"""fp64 restatement of the global-norm clip and the clipped AdamW step of include/vec2wav_hip.h (v2w_grad_sumsq_multi, v2w_grad_norm_finish,
v2w_scale_multi, v2w_adamw_multi_clipped), the bounds their tests use, and a replay of the kernels' summation order in numpy fp32.
It builds on tests/optim_ref.py (the AdamW step and its magnitudes).

    norm = sqrt(sum over every gradient entry of g^2)           coef = min(1, max_norm / (norm + 1e-6))
    g'   = g * coef                                             then the AdamW step of optim_ref on g'

The bounds (u = 2^-24; the tests allow twice the first-order count, as tests/optim_ref.py does, for the second-order terms and the fp64
evaluation itself).
  Sum of squares of one workgroup: a thread's fma chain holds at most T = 4 * ceil(chunk / 256) terms, chunk = the plan's units per
  workgroup; the block sum adds 6 (butterfly over 64 lanes) + 4 (the waves).  Every term is >= 0, so the relative errors add:
      |partial - exact| <= (T + 10) u * exact                                      sumsq_roundings(chunk)
  The norm is the square root of the fp64 sum of the partials, rounded once to fp32: half the relative error, plus one:
      |norm - exact| <= ((T + 10) / 2 + 1) u * exact                               norm_roundings(chunk)
  The coefficient (< 1) = max_norm / (norm + 1e-6) in fp64, rounded once: the norm's relative error plus one: norm_roundings + 1.
  The clipped step from a GIVEN fp32 coefficient: g' = g * coef is one more rounding wherever g enters - m': 3 + 1, v': 4 + 2 (g' enters
  twice), p': 15 + 3 (through m' once and v' twice): step_roundings(1).  Against a coefficient computed EXACTLY (the whole
  clip_grad_norm_ + AdamW in fp64) the coefficient's own relative error counts as further roundings on g':
  step_roundings(1 + norm_roundings + 1).
"""
import math

import numpy as np

from tests import optim_ref as R

CLIP_EPS = 1e-6
THREADS = 256
MIN_CHUNK = 2048
TARGET_WGS = 2048
TREE = 6 + 4


def total_norm(grads):
    return math.sqrt(sum(float((np.asarray(g, dtype=np.float64) ** 2).sum()) for g in grads))


def clip_coef(norm, max_norm):
    c = float(max_norm) / (norm + CLIP_EPS)          # inf / inf is NaN, and stays one (torch.clamp)
    return min(1.0, c) if c == c else c


def clip_ref(grads, max_norm):
    """(norm, coefficient, scaled gradients) in float64."""
    norm = total_norm(grads)
    coef = clip_coef(norm, max_norm)
    return norm, coef, [np.asarray(g, dtype=np.float64) * coef for g in grads]


def clipped_adamw_ref(p, g, m, v, h, coef):
    """optim_ref.adamw_ref on g * coef: (p', m', v', mags), the magnitudes taken at the scaled gradient."""
    return R.adamw_ref(p, np.asarray(g, dtype=np.float64) * float(coef), m, v, h)


def sumsq_roundings(chunk):
    return 4 * -(-chunk // THREADS) + TREE


def norm_roundings(chunk):
    return sumsq_roundings(chunk) / 2 + 1


def step_roundings(g_roundings=1):
    return {'m': R.ROUNDINGS['m'] + g_roundings, 'v': R.ROUNDINGS['v'] + 2 * g_roundings, 'p': R.ROUNDINGS['p'] + 3 * g_roundings}


def step_bounds(mags, g_roundings=1, u=R.U32):
    """optim_ref.bounds with the roundings of the clipped step: per-entry bounds on |p' - ref|, |m' - ref|, |v' - ref|."""
    c = {k: 2 * n for k, n in step_roundings(g_roundings).items()}
    return dict(p=c['p'] * u * (mags['p'] + mags['update_mag']), m=c['m'] * u * mags['mg'], v=c['v'] * u * mags['vg'])


# ---- the work split of one call (at most 80 tensors) and the kernels' order of summation
def plan(numels, phases):
    """(starts, chunk): v2w_adamw_multi_plan for gradients `phases[i]` floats past a 16-byte line (p = m = v = g)."""
    units = [(n + ph + 3) // 4 for n, ph in zip(numels, phases)]
    chunk = max(MIN_CHUNK, -(-sum(units) // TARGET_WGS))
    starts = [0]
    for u in units:
        starts.append(starts[-1] + max(1, -(-u // chunk)))
    return starts, chunk


def spans(numel, phase, nwg):
    """[(e0, e1)] element ranges of the nwg workgroups of one tensor (units of four floats cut at the 16-byte lines)."""
    units = (numel + phase + 3) // 4
    chunk = -(-units // nwg)
    out = []
    for w in range(nwg):
        u0, u1 = w * chunk, min((w + 1) * chunk, units)
        out.append((min(max(4 * u0 - phase, 0), numel), min(max(4 * u1 - phase, 0), numel)) if u1 > u0 else (0, 0))
    return out


def _tree(v, dtype):
    """v2w_block_sum over (..., 256): butterfly over the 64 lanes of each wave, then the four waves in order from 0."""
    v = v.reshape(v.shape[:-1] + (4, 64)).astype(dtype)
    lane = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        v = (v + v[..., lane ^ off]).astype(dtype)
    t = np.zeros(v.shape[:-2], dtype=dtype)
    for w in range(4):
        t = (t + v[..., w, 0]).astype(dtype)
    return t


def sumsq_partials_fp32(g, phase, nwg):
    """The nwg partials of one fp32 tensor as the kernel forms them, in numpy float32 (the fma as a float64 product and sum rounded once:
    the product of two fp32 is exact in fp64, the double rounding of the sum is what the tests' factor two covers)."""
    g = np.asarray(g, dtype=np.float32)
    numel = g.size
    units = (numel + phase + 3) // 4
    chunk = -(-units // nwg)
    iters = -(-chunk // THREADS)
    x = np.zeros((nwg, iters * THREADS * 4), dtype=np.float64)
    flat = np.zeros(4 * units, dtype=np.float64)
    flat[phase:phase + numel] = g
    for w in range(nwg):
        part = flat[4 * w * chunk:4 * min((w + 1) * chunk, units)]
        x[w, :part.size] = part
    x = x.reshape(nwg, iters, THREADS, 4)                      # unit t0 + i * 256 of the chunk belongs to thread t0
    acc = np.zeros((nwg, THREADS), dtype=np.float32)
    for i in range(iters):
        for j in range(4):
            acc = (x[:, i, :, j] * x[:, i, :, j] + acc.astype(np.float64)).astype(np.float32)
    return _tree(acc, np.float32)


def finish_fp64(partials):
    """v2w_grad_norm_finish's sum: thread t adds its run of ceil(n / 256) partials in index order, then the block sum, all in float64."""
    partials = np.asarray(partials, dtype=np.float64)
    per = -(-partials.size // THREADS)
    x = np.zeros(per * THREADS)
    x[:partials.size] = partials
    x = x.reshape(THREADS, per)
    acc = np.zeros(THREADS)
    for k in range(per):
        acc = acc + x[:, k]
    return float(_tree(acc, np.float64))
