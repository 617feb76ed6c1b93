"""What csrc/v2w_stft_loss.hip computes, twice over, on the CPU (tests/test_stft_loss_cpu.py, tests/test_stft_loss_gpu.py):

(a) the kernels' statements as include/vec2wav_hip.h words them, in fp64 from the float32 `spec` operands of a call - the three sums, sc,
    mag and d spec - each with what the device may differ by: first-order propagation of the header's roundings with u = 2^-24 and the
    device-function constants tests/mel_ref.py measured (E_MAG = 3.5 u relative on a magnitude, DIV_C u on a quotient, LOG_C u |log| on logf):
      d = Y - X          |dd| <= E_MAG (X + Y) + u |d| =: Ed
      Sd                 sum of 2 |d| Ed + Ed^2;   Sy: (2 E_MAG + E_MAG^2) Sy;   fp64 sums add n 2^-53 of the sum of the absolute terms
      |log Y - log X|    2 E_MAG (the arguments) + LOG_C u (|log X| + |log Y| + 2 E_MAG) + u |l| per entry
      sc                 the extremes of sqrt((Sd +- ESd) / (Sy -+ ESy)) (exact, not first order: Sd may be tiny), + u sc for the stored fp32
      mag                ESl / N + u mag
      d spec             c_sc, c_mag: u relative each (the fp64 quotient rounded once);  r = 1 / X: E_MAG + DIV_C u;  m = c_mag r: + 2 u;
                         dX = fma(c_sc, d, m): |c_sc| Ed + u |t1| + (E_MAG + DIV_C u + 2 u) |t2| + u (|t1| + |t2|), t1 = c_sc d, t2 = m;
                         w = dX r and the store w Re: (|Re| / X) (E_dX + (E_MAG + DIV_C u + 2 u) (|t1| + |t2|))
    An entry with |X / Y - 1| < mel_ref.GAP cannot be given a sign of X - Y (the fp32 magnitudes may order the other way): `dspec` marks it.
(b) the end-to-end oracle: torch.stft on the reflect-padded signal exactly as tests/stft_ref.py's oracle_acc frames it, in a chosen dtype,
    the loss in stock torch ops and d x by autograd.

Signals are stft_ref.signal's: x (generated) from seed 1, y (target) from seed 2 - independent, so |log Y - log X| is not concentrated at 0."""
import numpy as np
import torch

from tests import mel_ref as R
from tests import stft_ref as S

U = R.U
E_R = R.E_MAG + R.DIV_C * U            # 1 / X
E_M = E_R + 2 * U                      # c_mag * r: c_mag's rounding and the product's
SEED_X, SEED_Y = 1, 2


def signals(B, L):
    return S.signal(B, L, SEED_X), S.signal(B, L, SEED_Y)


# ---------------------------------------------------------------------------------------------------------------
# (a) the kernels' statements
def parts(spec, F, nb):
    """spec (B, Cs, FP) float32 -> (Re, Im, magnitude) in fp64 over (B, nb, F)."""
    s = R.f64(spec)
    re, im = s[:, :nb, :F], s[:, nb:2 * nb, :F]
    return re, im, np.sqrt(re * re + im * im + R.C9)


def sums(spec_x, spec_y, F, nb):
    """-> (values, bounds): dicts with Sd, Sy, Sl (what v2w_stft_loss_multi leaves in `sums`), sc and mag (fp32 stores)."""
    _, _, X = parts(spec_x, F, nb)
    _, _, Y = parts(spec_y, F, nb)
    N = X.size
    d = Y - X
    Ed = R.E_MAG * (X + Y) + U * np.abs(d)
    lx, ly = np.log(X), np.log(Y)
    l = np.abs(ly - lx)
    acc = N * 2.0 ** -53
    v = dict(Sd=float((d * d).sum()), Sy=float((Y * Y).sum()), Sl=float(l.sum()))
    b = dict(Sd=float((2 * np.abs(d) * Ed + Ed * Ed).sum()) + acc * v['Sd'],
             Sy=(2 * R.E_MAG + R.E_MAG ** 2 + acc) * v['Sy'],
             Sl=float((2 * R.E_MAG + R.LOG_C * U * (np.abs(lx) + np.abs(ly) + 2 * R.E_MAG) + U * l).sum()) + acc * v['Sl'])
    v['sc'], v['mag'] = np.sqrt(v['Sd']) / np.sqrt(v['Sy']), v['Sl'] / N
    hi = np.sqrt((v['Sd'] + b['Sd']) / (v['Sy'] - b['Sy']))
    lo = np.sqrt(max(v['Sd'] - b['Sd'], 0.0) / (v['Sy'] + b['Sy']))
    b['sc'] = max(hi - v['sc'], v['sc'] - lo) + U * hi
    b['mag'] = b['Sl'] / N + U * v['mag']
    return v, b


def totals(vals, bounds):
    """total[0], total[1] of a call: the means over its resolutions in fp64, stored in fp32."""
    out = {}
    for k in ('sc', 'mag'):
        m = float(np.mean([v[k] for v in vals]))
        out[k] = (m, float(np.mean([b[k] for b in bounds])) + U * m)
    return out


def g_of(gout, gterm, n):
    """g_r of the backward in the kernel's fp32 operations: gout / n, then + gterm[r] (an absent one is 0)."""
    f = np.float32
    a = f(gout) / f(n) if gout is not None else f(0)
    return float(f(a) + (f(gterm) if gterm is not None else f(0)))


def dspec(spec_x, spec_y, F, nb, Sd, Sy, g_sc, g_mag):
    """-> (dRe, dIm, bRe, bIm, unsure): v2w_stft_loss_multi_bwd's gradient over (B, nb, F) from the sums the call is handed (the device's own),
    its bounds, and the entries whose sign of X - Y the fp32 magnitudes need not share."""
    re, im, X = parts(spec_x, F, nb)
    _, _, Y = parts(spec_y, F, nb)
    N = X.size
    c_sc = g_sc / (np.sqrt(Sd) * np.sqrt(Sy)) if Sd > 0 else 0.0
    c_mag = g_mag / N
    d = X - Y
    t1, t2 = c_sc * d, c_mag * np.sign(d) / X
    dX = t1 + t2
    Ed = R.E_MAG * (X + Y) + U * np.abs(d)
    a12 = np.abs(t1) + np.abs(t2)
    EdX = abs(c_sc) * Ed + U * np.abs(t1) + E_M * np.abs(t2) + U * a12
    bw = (EdX + (E_R + 2 * U) * a12) / X
    return dX * re / X, dX * im / X, bw * np.abs(re), bw * np.abs(im), np.abs(X / Y - 1) < R.GAP


# (nb, F, FP, Cs, B): one frame; F % 4 = 2 and 3 with whole pad units behind them; nb = 1025 with an even count of pad rows (192 - 130 and
# 2112 - 2050 are both even: 'odd' adds a case whose last pad row stands alone); a call that mixes them
SHAPES = dict(one_frame=(65, 1, 4, 192, 1), tail2=(65, 6, 8, 192, 2), tail3=(65, 7, 12, 192, 3), nb1025=(1025, 9, 16, 2112, 1),
              odd=(33, 5, 8, 67, 2))
KERNEL_CASES = dict({k: [k] for k in SHAPES}, mixed=['tail3', 'nb1025', 'one_frame'])
MAX_UNSURE = 0.005                     # share of a case's entries that may go unchecked for |X / Y - 1| < GAP


def case_specs(name, same=False):
    """-> [(shape, spec_x, spec_y)] of one kernel-level case; the seed is the position of the shape's name in SHAPES."""
    order = list(SHAPES)
    out = []
    for s in KERNEL_CASES[name]:
        nb, F, FP, Cs, B = SHAPES[s]
        out.append((SHAPES[s],) + tuple(random_specs(100 + order.index(s), B, nb, F, FP, Cs, same)))
    return out


def random_specs(seed, B, nb, F, FP, Cs, same=False):
    """A loud random spectrum pair (|re|, |im| ~ 3) with junk where the kernels have no business: NaN in the rows >= 2 nb (never read),
    huge finite values of both signs in the columns >= F (loaded, selected away: their squares are Inf)."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(2):
        s = np.full((B, Cs, FP), np.nan, dtype=np.float32)
        s[:, :2 * nb, :F] = (3.0 * rng.standard_normal((B, 2 * nb, F))).astype(np.float32)
        s[:, :2 * nb, F:] = np.where(rng.uniform(size=(B, 2 * nb, FP - F)) < 0.5, -3.0e38, 3.0e38).astype(np.float32)
        out.append(s)
    if same:
        out[1][:, :2 * nb, :F] = out[0][:, :2 * nb, :F]
    return out


# ---------------------------------------------------------------------------------------------------------------
# (b) the end-to-end oracle
def spectrum(y, geo, dtype):
    """y (B, L) tensor -> (Re, Im) (B, nb, F) of torch.stft on the reflect-padded signal (stft_ref.oracle_acc's framing)."""
    n_fft, hop, win = geo
    pad = int((n_fft - hop) / 2)
    yp = torch.nn.functional.pad(y.unsqueeze(1), (pad, pad), mode='reflect').squeeze(1)
    sp = torch.stft(yp, n_fft, hop_length=hop, win_length=win, window=torch.hann_window(win, dtype=dtype), center=False, return_complex=True)
    return sp.real, sp.imag


def loss_of_spectra(rx, ix, ry, iy):
    """(sc, mag) in stock torch ops; the norm's subgradient at 0 is torch's (0)."""
    X = torch.sqrt(rx.pow(2) + ix.pow(2) + 1e-9)
    Y = torch.sqrt(ry.pow(2) + iy.pow(2) + 1e-9)
    sc = torch.linalg.vector_norm(Y - X) / torch.linalg.vector_norm(Y)
    return sc, (torch.log(Y) - torch.log(X)).abs().mean()


def oracle(x, y, resolutions, dtype, w_sc=1.0, w_mag=1.0):
    """-> (sc, mag, dx): the means over the resolutions as Python floats and d (w_sc sc + w_mag mag) / d x (B, L) in fp64 numpy."""
    xt = torch.from_numpy(np.asarray(x, dtype=np.float32)).to(dtype).requires_grad_(True)
    yt = torch.from_numpy(np.asarray(y, dtype=np.float32)).to(dtype)
    terms = [loss_of_spectra(*spectrum(xt, g, dtype), *spectrum(yt, g, dtype)) for g in resolutions]
    sc = sum(t[0] for t in terms) / len(terms)
    mag = sum(t[1] for t in terms) / len(terms)
    (w_sc * sc + w_mag * mag).backward()
    return sc.detach().double().item(), mag.detach().double().item(), xt.grad.double().numpy()


def oracle_gaps(x, y, resolutions, w_sc=1.0, w_mag=1.0):
    """The oracle against itself, float32 against float64, on the CPU: dict(sc, mag, dx: the fp64 results; rel_sc, rel_mag: the relative
    gaps of the two scalars; gap_dx: max |dx32 - dx64|)."""
    s64, m64, d64 = oracle(x, y, resolutions, torch.float64, w_sc, w_mag)
    s32, m32, d32 = oracle(x, y, resolutions, torch.float32, w_sc, w_mag)
    return dict(sc=s64, mag=m64, dx=d64, rel_sc=abs(s32 - s64) / abs(s64), rel_mag=abs(m32 - m64) / abs(m64),
                gap_dx=float(np.abs(d32 - d64).max()))
