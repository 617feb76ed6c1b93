"""fp64 oracle of the GAN loss terms over a padded batch (include/vec2wav_hip.h, v2w_*_multi_len), stated on masked numpy arrays.

A tensor is (B, C, V) - B items, C rows per item, V floats per row (a score: C = 1); `ext` (B,) the floats at the head of each of an item's
rows that count, clamped to [0, V].  den = C * sum_b v_b.
  L1     term = sum_counted |a - b| / den (0 when den == 0);   da = sgn(a - b) * (scale * gout / den) on the counted floats, +0.0 elsewhere
  LSGAN  term = sum_counted (t - s)^2 / den (0 when den == 0); ds = 2 (s - t) g / den on the counted floats, +0.0 elsewhere
"""
import numpy as np


def as_rows(x, B):
    """(B, C, ...) or (B, N) array -> (B, C, V) float64."""
    x = np.asarray(x, dtype=np.float64)
    assert x.shape[0] == B
    return x.reshape(B, 1, -1) if x.ndim == 2 else x.reshape(B, x.shape[1], -1)


def counted(ext, B, C, V):
    v = np.clip(np.asarray(ext, dtype=np.int64), 0, V)
    on = np.arange(V)[None, None, :] < v[:, None, None]
    return np.broadcast_to(on, (B, C, V)), int(C * v.sum())


def l1_term(a, b, ext):
    B = a.shape[0]
    a3, b3 = as_rows(a, B), as_rows(b, B)
    on, den = counted(ext, *a3.shape)
    return float(np.abs(np.ma.masked_array(a3 - b3, mask=~on)).sum() / den) if den else 0.0


def l1_grad(a, b, ext, coef_num):
    """da (float64, shaped like a): sgn(a - b) * coef_num / den on the counted floats, +0.0 elsewhere; db = -da there."""
    B = a.shape[0]
    a3, b3 = as_rows(a, B), as_rows(b, B)
    on, den = counted(ext, *a3.shape)
    d = np.zeros(a3.shape)
    if den:
        d[on] = np.sign(a3 - b3)[on] * (coef_num / den)
    return d.reshape(np.shape(a)), on.reshape(np.shape(a))


def lsgan_term(s, target, ext):
    B = s.shape[0]
    s3 = as_rows(s, B)
    on, den = counted(ext, *s3.shape)
    return float(((target - np.ma.masked_array(s3, mask=~on)) ** 2).sum() / den) if den else 0.0


def lsgan_grad(s, target, ext, g):
    B = s.shape[0]
    s3 = as_rows(s, B)
    on, den = counted(ext, *s3.shape)
    d = np.zeros(s3.shape)
    if den:
        d[on] = 2.0 * (s3 - target)[on] * g / den
    return d.reshape(np.shape(s)), on.reshape(np.shape(s))
