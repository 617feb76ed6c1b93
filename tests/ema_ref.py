"""fp64 restatement of the exponential moving average of include/vec2wav_hip.h (v2w_adamw_ema_multi, v2w_ema_multi) and the bound its
tests use.  It builds on tests/optim_ref.py (u = 2^-24).

    ema_omd = fp32(1 - decay)                    computed in double, rounded once: what the caller hands the kernel
    e'      = e + ema_omd * (p' - e)             p' the STORED fp32 parameter after the step (v2w_ema_multi: the parameter as it is)

The bound.  The kernel's two lines are de = p' - e and e' = fma(ema_omd, de, e), each one correctly rounded fp32 operation; with the
rounding of ema_omd itself the header counts 3 roundings on e', on the magnitude |e| + |p'| (|de| <= |p'| + |e|, ema_omd <= 1,
|e'| <= |e| + |p'|):  |e' - exact| <= 3u (|e| + |p'|).  The restatement starts from the fp32 ema_omd, so two of the three are in play and
the third covers the second-order terms and the fp64 evaluation: the tests use the bound as it stands, no factor on it.

Over T steps from stored parameters p_1 .. p_T the recurrence has the closed form, with d = 1 - ema_omd,
    e_T = d^T e_0 + (1 - d) sum_{t=1..T} d^(T-t) p_t
and an error made at step t reaches e_T multiplied by d^(T-t) <= 1: the accumulated bound is the sum of the per-step bounds.
"""
import numpy as np

from tests import optim_ref as R

ROUNDINGS = 3


def omd32(decay):
    """ema_omd as the kernel receives it: 1 - decay in double, rounded once to fp32."""
    return np.float32(1.0 - float(decay))


def ema_exact(e, p_new, omd):
    """e' in float64 from fp32 (or float64) e, the stored p' and the fp32 ema_omd."""
    e, p_new = np.asarray(e, dtype=np.float64), np.asarray(p_new, dtype=np.float64)
    return e + float(omd) * (p_new - e)


def ema_bound(e, p_new, u=R.U32):
    """Per-entry bound on |e' - ema_exact|: 3u (|e| + |p'|)."""
    return ROUNDINGS * u * (np.abs(np.asarray(e, dtype=np.float64)) + np.abs(np.asarray(p_new, dtype=np.float64)))


def ema_closed_form(e0, ps, omd):
    """e_T = d^T e_0 + (1 - d) sum_t d^(T-1-t) p_t for ps = [p_0 .. p_(T-1)] (the parameter after step t + 1), d = 1 - omd, in float64."""
    d = 1.0 - float(omd)
    T = len(ps)
    out = d ** T * np.asarray(e0, dtype=np.float64)
    for t, p in enumerate(ps):
        out = out + (1.0 - d) * d ** (T - 1 - t) * np.asarray(p, dtype=np.float64)
    return out


def worst_ratio(got, want, bnd):
    """max over the entries of |got - want| / bound (0 where they agree exactly)."""
    d = np.abs(np.asarray(got, dtype=np.float64) - want)
    with np.errstate(divide='ignore', invalid='ignore'):
        r = np.where(d == 0, 0.0, d / bnd)
    return float(r.max())
