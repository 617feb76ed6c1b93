"""fp64 CPU statements of what the seven first entry points of csrc/v2w_mel.hip compute, as include/vec2wav_hip.h words them (not as the kernels
index), and what each entry may differ by (tests/test_mel_kernels_gpu.py; the records are tests/mel_cases.py's).  Numpy throughout; torch
only for the autograd that gives v2w_mel_finish_bwd its value.  Every function takes the fp32 operands of the call and returns
(value, bound) per entry; bound None means the kernel moves or adds floats in a fixed order and is held bit for bit.

The bounds, with u = 2^-24 and every n counted from the code:
  mag   t = re*re + im*im + 1e-9f is three roundings on a sum of positive terms (at most: an fma saves one), |dt| <= 3 u t, so sqrt(t) moves
        by 1.5 u relative; sqrtf adds SQRT_C u:                                              e_mag = (1.5 + SQRT_C) u, relative to mag
  acc   nb fmas in a row on the stored magnitudes:      |d acc| <= (nb u + e_mag) S,  S = sum_c |basis[m][c]| mag[c]  (= acc for basis >= 0)
  out   log moves by -log1p(-|d acc| / acc) (exact, not first order) and logf adds LOG_C u |log|; a clamped entry is logf(1e-5f) alone.
  d     = g / acc on the closed side of the clamp: |d| (e_acc / (1 - e_acc) + DIV_C u),  e_acc = |d acc| / acc
  dm    n_mels fmas on signed terms: n_mels u sum_m |basisT[c][m] d[m]| + sum_m |basisT[c][m]| |dd[m]|
  s     = dm / mag: |ddm| / mag + |s| (e_mag + DIV_C u);  the two stores s * re, s * im add u |s re| each.
An (m, f) entry cannot be given a side of the clamp when its fp64 acc lies within |d acc| of 1e-5f: the records keep every acc at least
2^-10 (relative) away from it (tests/test_mel_ref_cpu.py asserts both), so that no entry is ever excluded.

The device functions.  The ROCm installation ships no document that states an error for sqrtf, logf or the fp32 division, so each was measured once
on an MI355X against fp64 on arguments the kernels compute exactly (tests/test_mel_kernels_gpu.py::test_device_function_errors repeats it):
  division  g / b through mel_finish_bwd_kernel (one bin of magnitude 2^k, one mel of weight b): DIV_MEASURED u relative
  sqrtf     1 / sqrtf(1 + im^2) through the same kernel (t exact in 24 bits): the quotient is, in every probe, the correctly rounded
            quotient of the correctly rounded root, whose own worst error on those arguments is SQRT_MEASURED u relative
  logf      logf(b * x) through mel_finish_kernel (b x exact in 24 bits) over [2^-17, 2^10]: LOG_MEASURED u relative to |log|
Each constant is twice the measured figure, rounded up to an integer, as tests/stage_ref.py does for tanhf (1.253 -> 3)."""
import numpy as np
import torch

U = 2.0 ** -24
C9 = float(np.float32(1e-9))          # the two constants as the kernels hold them
C5 = float(np.float32(1e-5))
GAP = 2.0 ** -10                      # every record keeps |acc / 1e-5f - 1| >= GAP

DIV_MEASURED, DIV_C = 0.9901, 2       # units of 2^-24, relative; every one of 16 384 quotients was the correctly rounded one
SQRT_MEASURED, SQRT_C = 0.9910, 2     # every one of 16 384 roots the correctly rounded one (1 / sqrtf as a whole: 1.4234)
LOG_MEASURED, LOG_C = 3.0495, 7       # at a = 0.0181026; 16 384 arguments in [1e-5, 2^11], some within a few percent of 1
E_MAG = (1.5 + SQRT_C) * U


def f64(x):
    return np.asarray(x.detach().cpu().numpy() if hasattr(x, 'detach') else x, dtype=np.float64)


def worst_ratio(got, want, bound):
    """max |got - want| / bound over the entries (0 / 0 counts as 0, x / 0 as inf, a non-finite `got` as inf)."""
    got, want, bound = f64(got), f64(want), f64(bound)
    err = np.abs(got - want)
    with np.errstate(divide='ignore', invalid='ignore'):
        r = np.where(err == 0, 0.0, err / bound)
    r = np.where(np.isfinite(got), r, np.inf)
    return float(r.max()) if r.size else 0.0


def roundup4(n):
    return (n + 3) // 4 * 4


def frames(n, hop, pad):
    """Frames of an item of n samples, n_fft = 2 pad + hop: reflect padding needs n > pad, one frame needs n + 2 pad >= n_fft."""
    return (n - hop) // hop + 1 if n > pad and n >= hop else 0


def item_samples(lens, len_mul, L=None):
    n = np.maximum(np.asarray(lens, dtype=np.int64) * len_mul, 0)
    return n if L is None else np.minimum(n, L)


# ---------------------------------------------------------------------------------------------------------------
# the two phase calls and the adjoint
def gather_map(L, hop, pad, FP):
    """src (hop, FP): xp[b][p][f] = y[b][src[p][f]], -1 where it is 0 (past the padded signal).  The reflection is numpy's own."""
    ypad = np.pad(np.arange(L, dtype=np.int64), (pad, pad), mode='reflect') if pad else np.arange(L, dtype=np.int64)
    i = np.arange(FP, dtype=np.int64)[None, :] * hop + np.arange(hop, dtype=np.int64)[:, None]
    return np.where(i < L + 2 * pad, ypad[np.minimum(i, L + 2 * pad - 1)], -1), i


def phases(y, hop, pad, FP):
    """v2w_mel_phases: y (B, L) -> xp (B, hop, FP), a gather."""
    y = np.asarray(y, dtype=np.float32)
    src, _ = gather_map(y.shape[1], hop, pad, FP)
    return np.where(src[None] >= 0, y[:, np.maximum(src, 0)], np.float32(0)), None


def phases_len(y, hop, pad, FP, lens, len_mul):
    """v2w_mel_phases_len: item b is the B = 1 call on y[b, :Lb] over that call's roundup4(F_b + k - 1) columns, zero elsewhere."""
    y = np.asarray(y, dtype=np.float32)
    B, L = y.shape
    k = (2 * pad + hop) // hop
    out = np.zeros((B, hop, FP), dtype=np.float32)
    for b, Lb in enumerate(item_samples(lens, len_mul, L)):
        Fb = frames(int(Lb), hop, pad)
        if Fb:
            FPb = roundup4(Fb + k - 1)
            own = phases(y[b:b + 1, :Lb], hop, pad, FPb)[0][0]
            out[b, :, :min(FP, FPb)] = own[:, :FP]
    return out, None


def phases_bwd(dxp, L, hop, pad):
    """v2w_mel_phases_bwd: dy[b][s] = the float32 sum of dxp over the padded positions that read y[s], in the order the header's kernel
    documents: the sample itself, the left reflection, the right reflection.  The transpose of gather_map; positions the forward never reads
    (src = -1) contribute nothing, whatever dxp holds there."""
    dxp = np.asarray(dxp, dtype=np.float32)
    B, _, FP = dxp.shape
    src, i = gather_map(L, hop, pad, FP)
    dy = np.zeros((B, L), dtype=np.float32)
    kind = np.where(i < pad, 1, np.where(i >= L + pad, 2, 0))
    for kk in (0, 1, 2):
        sel = (src >= 0) & (kind == kk)
        s = src[sel]
        assert len(np.unique(s)) == len(s)                        # a sample has one position of each kind at most
        dy[:, s] = dxp[:, sel] if kk == 0 else dy[:, s] + dxp[:, sel]
    return dy, None


# ---------------------------------------------------------------------------------------------------------------
# finish
def _parts(spec, basis, F, nb, keep=None):
    """mag (B, nb, F), acc, S, |d acc| (B, n_mels, F) in fp64; `keep` (B, F) bool: frames outside read as zeros (they may hold NaN)."""
    spec, basis = f64(spec), f64(basis)
    re, im = spec[:, :nb, :F], spec[:, nb:2 * nb, :F]
    if keep is not None:
        re, im = np.where(keep[:, None, :], re, 0.0), np.where(keep[:, None, :], im, 0.0)
    mag = np.sqrt(re * re + im * im + C9)
    acc = np.einsum('mc,bcf->bmf', basis, mag)
    S = np.einsum('mc,bcf->bmf', np.abs(basis), mag)
    return dict(re=re, im=im, mag=mag, acc=acc, S=S, dacc=(nb * U + E_MAG) * S)


def clamp_gap(spec, basis, F, nb, keep=None):
    """min over the entries of |acc / 1e-5f - 1|, and max of |d acc| / |acc - 1e-5f|: the first must be >= GAP, the second < 1."""
    p = _parts(spec, basis, F, nb, keep)
    d = np.abs(p['acc'] - C5)
    if keep is not None:
        d = np.where(keep[:, None, :], d, np.inf)
    with np.errstate(divide='ignore'):
        return float((d / C5).min()), float((p['dacc'] / d).max())


def _finish(p):
    acc, open_ = p['acc'], p['acc'] >= C5
    value = np.log(np.maximum(acc, C5))
    with np.errstate(divide='ignore', invalid='ignore'):
        rel = np.where(open_, p['dacc'] / acc, 0.0)
    return value, -np.log1p(-rel) + LOG_C * U * np.abs(value)


def finish(spec, basis, F, nb):
    """v2w_mel_finish: spec (B, Cs, FP), basis (n_mels, nb) -> log(max(basis @ sqrt(re^2 + im^2 + 1e-9f), 1e-5f)) (B, n_mels, F)."""
    return _finish(_parts(spec, basis, F, nb))


def item_frames(lens, len_mul, hop, n_fft, F):
    """F_b of v2w_mel_finish_len: the frames of len[b] * len_mul samples (the call takes no L), clamped to F."""
    pad = (n_fft - hop) // 2
    return np.array([min(frames(int(n), hop, pad), F) for n in item_samples(lens, len_mul)], dtype=np.int64)


def finish_len(spec, basis, F, nb, lens, len_mul, hop, n_fft):
    """v2w_mel_finish_len: frames f < F_b as finish, exactly 0.0 in [F_b, F)."""
    keep = np.arange(F)[None, :] < item_frames(lens, len_mul, hop, n_fft, F)[:, None]
    value, bound = _finish(_parts(spec, basis, F, nb, keep))
    return np.where(keep[:, None, :], value, 0.0), np.where(keep[:, None, :], bound, 0.0)


def finish_torch(spec, basis, F, nb):
    """The same value in torch fp64, for autograd: the clamp written as a select whose closed side (acc >= 1e-5f) passes the gradient."""
    re, im = spec[:, :nb, :F], spec[:, nb:2 * nb, :F]
    acc = torch.einsum('mc,bcf->bmf', basis, torch.sqrt(re * re + im * im + C9))
    return torch.log(torch.where(acc >= C5, acc, torch.full_like(acc, C5)))


def finish_bwd(spec, basis, gout, F, nb):
    """v2w_mel_finish_bwd: d spec (B, 2 nb, F) of sum(gout * finish(spec)): rows [0, nb) d re, [nb, 2 nb) d im.  The rest of dspec (pad rows,
    columns >= F) is the caller's and keeps its bits."""
    t = torch.from_numpy(f64(spec)[:, :2 * nb, :F].copy()).requires_grad_(True)
    out = finish_torch(t, torch.from_numpy(f64(basis)), F, nb)
    value = torch.autograd.grad(out, t, torch.from_numpy(f64(gout)))[0].numpy()
    p = _parts(spec, basis, F, nb)
    ab, n_mels = np.abs(f64(basis)), basis.shape[0]
    open_ = p['acc'] >= C5
    with np.errstate(divide='ignore', invalid='ignore'):
        d = np.where(open_, f64(gout) / p['acc'], 0.0)
        ea = np.where(open_, p['dacc'] / p['acc'], 0.0)
    dd = np.abs(d) * (ea / (1 - ea) + DIV_C * U)
    ddm = n_mels * U * np.einsum('mc,bmf->bcf', ab, np.abs(d)) + np.einsum('mc,bmf->bcf', ab, dd)
    s = np.einsum('mc,bmf->bcf', f64(basis), d) / p['mag']
    ds = ddm / p['mag'] + np.abs(s) * (E_MAG + DIV_C * U)
    bound = np.concatenate([ds * np.abs(p['re']) + U * np.abs(s * p['re']), ds * np.abs(p['im']) + U * np.abs(s * p['im'])], 1)
    return value, bound


# ---------------------------------------------------------------------------------------------------------------
# the kernels' own operation order in numpy float32 (tests/test_mel_ref_cpu.py: the bound holds on it, and not on a perturbed basis)
def fma32(a, b, c):
    """fmaf on float32 arrays: the product is exact in fp64; the one fp64 rounding of the sum sits 29 bits below the fp32 one."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def finish_emulated(spec, basis, F, nb):
    f32 = np.float32
    spec, basis = np.asarray(spec, dtype=f32), np.asarray(basis, dtype=f32)
    re, im = spec[:, :nb, :F], spec[:, nb:2 * nb, :F]
    mag = np.sqrt((re * re + im * im).astype(f32) + f32(1e-9)).astype(f32)
    acc = np.zeros((spec.shape[0], basis.shape[0], F), dtype=f32)
    for c in range(nb):
        acc = fma32(basis[None, :, c, None], mag[:, None, c, :], acc)
    return np.log(np.maximum(acc, f32(1e-5)).astype(np.float64)).astype(f32), acc, mag


def finish_bwd_emulated(spec, basis, gout, F, nb):
    f32 = np.float32
    spec, basis, gout = np.asarray(spec, dtype=f32), np.asarray(basis, dtype=f32), np.asarray(gout, dtype=f32)
    _, acc, mag = finish_emulated(spec, basis, F, nb)
    with np.errstate(divide='ignore', invalid='ignore'):
        d = np.where(acc >= f32(1e-5), (gout / acc).astype(f32), f32(0))
    dm = np.zeros_like(mag)
    for m in range(basis.shape[0]):
        dm = fma32(basis[m][None, :, None], d[:, m, None, :], dm)
    s = (dm / mag).astype(f32)
    return np.concatenate([s * spec[:, :nb, :F], s * spec[:, nb:2 * nb, :F]], 1).astype(f32)


# ---------------------------------------------------------------------------------------------------------------
# mel.py's chain against the oracle: the DFT conv's bound carried to the end, to first order
def through_finish(re, im, dre, dim, basis, nb):
    """(value, bound) of log(max(basis @ mag, 1e-5f)) for fp64 (re, im) (B, nb, F) known to (dre, dim):
    |d mag| <= (|re| dre + |im| dim) / mag + e_mag mag, |d acc| = basis @ |d mag| + nb u S, then d acc / acc through the log."""
    basis = f64(basis)
    mag = np.sqrt(re * re + im * im + C9)
    dmag = (np.abs(re) * dre + np.abs(im) * dim) / mag + E_MAG * mag
    acc = np.einsum('mc,bcf->bmf', basis, mag)
    dacc = np.einsum('mc,bcf->bmf', np.abs(basis), dmag) + nb * U * np.einsum('mc,bcf->bmf', np.abs(basis), mag)
    value = np.log(np.maximum(acc, C5))
    assert (np.abs(acc - C5) > dacc).all(), 'an entry of the chain lies within its bound of the clamp'
    rel = np.where(acc >= C5, dacc / acc, 0.0)
    return value, -np.log1p(-rel) + LOG_C * U * np.abs(value)
