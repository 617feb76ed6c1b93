"""What the length-aware entry points of csrc/v2w_stft_loss.hip compute (v2w_stft_loss_multi_len, _len_bwd), on the CPU, beside
tests/stft_loss_ref.py whose `parts`, constants and bound formulas it keeps (tests/test_stft_loss_len_cpu.py, tests/test_stft_loss_len_gpu.py):

(a) the kernels' statements in fp64 from the float32 `spec` operands: stft_loss_ref's (a) over the entries (b, bin, f < F_b) only, with
    N = nb * sum_b F_b in the place of B * nb * F.  The bounds are that module's, term for term: a masked entry adds nothing to a sum and
    nothing to a bound, and its d spec is exactly +0.0 (bound 0).  N == 0: every value and every bound is 0.
(b) the end-to-end oracle for a padded batch of unequal lengths: per resolution and per item that has a frame, stft_loss_ref.spectrum on
    x[b, :n_b] and y[b, :n_b] (torch.stft on the item's own reflect-padded samples); the items' spectra joined along the frame axis; sc and mag
    in stock torch ops over the joined entries (stft_loss_ref.loss_of_spectra); d x by autograd, in float64 and in float32.  A resolution
    in which no item has a frame contributes 0 to both means."""
import functools

import numpy as np
import torch

from tests import mel_ref as R
from tests import stft_loss_ref as SL
from tests import stft_ref as S

U = R.U


def frames(n, hop, n_fft):
    """Frames of n samples, as v2w_mel_finish_geo_len states them: pad = (n_fft - hop) / 2 rounded down."""
    pad = (n_fft - hop) // 2
    n = int(n)
    return (n + 2 * pad - n_fft) // hop + 1 if n > pad and n + 2 * pad >= n_fft else 0


def item_frames(lens, len_mul, hop, n_fft, F):
    """F_b: the frames of len[b] * len_mul samples, clamped to F (a negative length: no frame)."""
    return [min(frames(int(n) * len_mul, hop, n_fft), F) for n in lens]


def keep_of(Fb, nb, F):
    """(B, nb, F) bool: the entries a call counts."""
    k = np.arange(F)[None, :] < np.asarray(Fb)[:, None]
    return np.broadcast_to(k[:, None, :], (len(Fb), nb, F))


# ---------------------------------------------------------------------------------------------------------------
# (a) the kernels' statements
def _valid(spec, F, nb, keep):
    with np.errstate(all='ignore'):                         # (the junk past F_b: Inf and NaN that the mask drops)
        re, im, X = SL.parts(spec, F, nb)
    return re[keep], im[keep], X[keep]


def sums(spec_x, spec_y, F, nb, Fb):
    """-> (values, bounds): dicts with Sd, Sy, Sl, N (the four doubles v2w_stft_loss_multi_len leaves in `sums`), sc and mag."""
    keep = keep_of(Fb, nb, F)
    _, _, X = _valid(spec_x, F, nb, keep)
    _, _, Y = _valid(spec_y, F, nb, keep)
    N = X.size
    assert N == nb * sum(Fb)
    if N == 0:
        z = dict(Sd=0.0, Sy=0.0, Sl=0.0, N=0.0, sc=0.0, mag=0.0)
        return z, dict(z)
    d = Y - X
    Ed = R.E_MAG * (X + Y) + U * np.abs(d)
    lx, ly = np.log(X), np.log(Y)
    l = np.abs(ly - lx)
    acc = N * 2.0 ** -53
    v = dict(Sd=float((d * d).sum()), Sy=float((Y * Y).sum()), Sl=float(l.sum()), N=float(N))
    b = dict(Sd=float((2 * np.abs(d) * Ed + Ed * Ed).sum()) + acc * v['Sd'],
             Sy=(2 * R.E_MAG + R.E_MAG ** 2 + acc) * v['Sy'],
             Sl=float((2 * R.E_MAG + R.LOG_C * U * (np.abs(lx) + np.abs(ly) + 2 * R.E_MAG) + U * l).sum()) + acc * v['Sl'], N=0.0)
    v['sc'], v['mag'] = np.sqrt(v['Sd']) / np.sqrt(v['Sy']), v['Sl'] / N
    hi = np.sqrt((v['Sd'] + b['Sd']) / (v['Sy'] - b['Sy']))
    lo = np.sqrt(max(v['Sd'] - b['Sd'], 0.0) / (v['Sy'] + b['Sy']))
    b['sc'] = max(hi - v['sc'], v['sc'] - lo) + U * hi
    b['mag'] = b['Sl'] / N + U * v['mag']
    return v, b


def dspec(spec_x, spec_y, F, nb, Fb, Sd, Sy, N, g_sc, g_mag):
    """-> (dRe, dIm, bRe, bIm, unsure) over (B, nb, F): v2w_stft_loss_multi_len_bwd's gradient from the four doubles the call is handed, its
    bounds, and the valid entries whose sign of X - Y the fp32 magnitudes need not share.  Entries at or past F_b: value 0, bound 0."""
    keep = keep_of(Fb, nb, F)
    out = [np.zeros(keep.shape) for _ in range(4)] + [np.zeros(keep.shape, dtype=bool)]
    if not keep.any():
        return tuple(out)
    re, im, X = _valid(spec_x, F, nb, keep)
    _, _, Y = _valid(spec_y, F, nb, keep)
    c_sc = g_sc / (np.sqrt(Sd) * np.sqrt(Sy)) if Sd > 0 else 0.0
    c_mag = g_mag / N if N > 0 else 0.0
    d = X - Y
    t1, t2 = c_sc * d, c_mag * np.sign(d) / X
    dX = t1 + t2
    Ed = R.E_MAG * (X + Y) + U * np.abs(d)
    a12 = np.abs(t1) + np.abs(t2)
    EdX = abs(c_sc) * Ed + U * np.abs(t1) + SL.E_M * np.abs(t2) + U * a12
    bw = (EdX + (SL.E_R + 2 * U) * a12) / X
    for o, val in zip(out, (dX * re / X, dX * im / X, bw * np.abs(re), bw * np.abs(im), np.abs(X / Y - 1) < R.GAP)):
        o[keep] = val
    return tuple(out)


# Kernel-level cases.  The shapes are stft_loss_ref.SHAPES' (nb, F, FP, Cs) at B = 3 or 4; (hop, n_fft) and the lengths are chosen for the
# frame counts in the comments (frames(n) = n // hop for n >= n_fft at n_fft = 2 hop and at hop 2 with n_fft 8; (n - 4) // 3 + 1 at hop 3
# with n_fft 6; tests/test_stft_loss_len_cpu.py holds the comments to `item_frames`).  Together:
# a count of 0, of 1, counts with F_b % 4 = 1, 2 and 3, F itself, and a count clamped from above F.
SHAPES = dict(one_frame=(65, 1, 4, 192, 3), tail2=(65, 6, 8, 192, 3), tail3=(65, 7, 12, 192, 4), nb1025=(1025, 9, 16, 2112, 3),
              odd=(33, 5, 8, 67, 3), tail3_b3=(65, 7, 12, 192, 3))
CASES = dict(
    one_frame=dict(shapes=['one_frame'], geo=[(4, 8)], lens=[3, 4, 20], len_mul=1),                      # F_b 0, 1, 1 (5 clamped)
    tail2=dict(shapes=['tail2'], geo=[(4, 8)], lens=[12, 4, 1], len_mul=2),                              # 6 = F, 2, 0 (n = 2 <= pad)
    tail3=dict(shapes=['tail3'], geo=[(4, 8)], lens=[12, 36, 4, 20], len_mul=1),                         # 3, 7 (9 clamped), 1, 5
    nb1025=dict(shapes=['nb1025'], geo=[(2, 8)], lens=[6, -5, 4], len_mul=3),                            # 9 = F, 0 (negative), 6
    odd=dict(shapes=['odd'], geo=[(3, 6)], lens=[4, 24, 10], len_mul=1),                                 # 1, 5 (7 clamped), 3
    mixed=dict(shapes=['tail3_b3', 'nb1025', 'one_frame'], geo=[(4, 8), (2, 8), (8, 16)], lens=[10, 3, 20], len_mul=2),
    # mixed, n = 20, 6, 40: (4, 8) 5, 1, 7 (10 clamped); (2, 8) 9 (10 clamped), 3, 9 (20 clamped); (8, 16) 1 (2 clamped), 0, 1 (5 clamped)
    full=dict(shapes=['tail3_b3', 'nb1025', 'one_frame'], geo=[(4, 8), (2, 8), (8, 16)], lens=[18, 14, 50], len_mul=2),   # every F_b = F
    none=dict(shapes=['tail2', 'odd'], geo=[(4, 8), (3, 6)], lens=[1, 2, -7], len_mul=1))               # every F_b = 0
SEED = 300                             # + the position of the shape's name in SHAPES


@functools.lru_cache(maxsize=None)
def case_specs(name):
    """-> [(shape, (hop, n_fft), F_b list, spec_x, spec_y)] of one kernel-level case: stft_loss_ref.random_specs (NaN in the rows >= 2 nb,
    +-3e38 in the columns >= F) with NaN and +-3e38 in every column [F_b, F) of item b as well.  The seeds are held to the condition of the
    device test: the fp64 reference alone leaves at most stft_loss_ref.MAX_UNSURE of a resolution's valid entries without a sign."""
    c = CASES[name]
    order = list(SHAPES)
    out = []
    for s, (hop, n_fft) in zip(c['shapes'], c['geo']):
        nb, F, FP, Cs, B = SHAPES[s]
        assert B == len(c['lens'])
        Fb = item_frames(c['lens'], c['len_mul'], hop, n_fft, F)
        seed = SEED + order.index(s)
        sx, sy = SL.random_specs(seed, B, nb, F, FP, Cs)
        rng = np.random.default_rng(seed + 1000)
        junk = np.array([np.nan, 3.0e38, -3.0e38], dtype=np.float32)
        for a in (sx, sy):
            for b, f in enumerate(Fb):
                a[b, :2 * nb, f:F] = junk[rng.integers(0, 3, size=(2 * nb, F - f))]
        v, _ = sums(sx, sy, F, nb, Fb)
        unsure = dspec(sx, sy, F, nb, Fb, v['Sd'], v['Sy'], v['N'], 1.0, 1.0)[4]
        assert unsure.sum() <= SL.MAX_UNSURE * max(v['N'], 1), (name, s, int(unsure.sum()), v['N'])
        out.append((SHAPES[s], (hop, n_fft), Fb, sx, sy))
    return out


# ---------------------------------------------------------------------------------------------------------------
# (b) the end-to-end oracle for a padded batch of unequal lengths
def samples_of(lens, len_mul, L):
    return [min(max(int(n) * len_mul, 0), L) for n in lens]


def ragged_oracle(x, y, ns, resolutions, dtype, w_sc=1.0, w_mag=1.0):
    """x, y (B, L) float32, ns: the items' sample counts -> (sc, mag, dx): the means over the resolutions as Python floats and
    d (w_sc sc + w_mag mag) / d x (B, L) in fp64 numpy (0 past n_b and for an item without a frame)."""
    xt = torch.from_numpy(np.asarray(x, dtype=np.float32)).to(dtype).requires_grad_(True)
    yt = torch.from_numpy(np.asarray(y, dtype=np.float32)).to(dtype)
    sc, mag = xt.new_zeros(()), xt.new_zeros(())
    for n_fft, hop, win in resolutions:
        items = [b for b, n in enumerate(ns) if frames(n, hop, n_fft)]
        if not items:
            continue
        sp = [SL.spectrum(t[b:b + 1, :ns[b]], (n_fft, hop, win), dtype) for b in items for t in (xt, yt)]          # x_b, y_b, x_b', ...
        rx, ix, ry, iy = (torch.cat([sp[2 * i + j][p] for i in range(len(items))], dim=2) for j in (0, 1) for p in (0, 1))
        s, m = SL.loss_of_spectra(rx, ix, ry, iy)
        sc, mag = sc + s, mag + m
    sc, mag = sc / len(resolutions), mag / len(resolutions)
    if not sc.requires_grad:                                # no item has a frame in any resolution
        return 0.0, 0.0, np.zeros(xt.shape)
    (w_sc * sc + w_mag * mag).backward()
    return sc.detach().double().item(), mag.detach().double().item(), xt.grad.double().numpy()


def ragged_gaps(x, y, ns, resolutions, w_sc=1.0, w_mag=1.0):
    """The ragged oracle against itself, float32 against float64 (stft_loss_ref.oracle_gaps' dict)."""
    s64, m64, d64 = ragged_oracle(x, y, ns, resolutions, torch.float64, w_sc, w_mag)
    s32, m32, d32 = ragged_oracle(x, y, ns, resolutions, torch.float32, w_sc, w_mag)
    return dict(sc=s64, mag=m64, dx=d64, rel_sc=abs(s32 - s64) / abs(s64), rel_mag=abs(m32 - m64) / abs(m64),
                gap_dx=float(np.abs(d32 - d64).max()))


def small_cases():
    """(resolutions, L, lens, len_mul, w_mag) at stft_ref.SMALL, B = 3: L the largest of stft_ref.lengths_of, one item at L, one at each
    other listed length in turn (pad + 1, exactly one frame, the % hop edge), one without a frame (pad samples: no reflection; 1 at pad 0)."""
    from wavthruvec_pytorch_amd import mel
    out = []
    for geo in S.SMALL:
        g = mel.stft_geometry(*geo)
        Ls = S.lengths_of(geo[0], geo[1], g['pad'])
        L = Ls[-1]
        none = max(g['pad'], 1)
        assert S.frames(L, g) and not S.frames(none, g)
        for i, m in enumerate(Ls[:-1]):
            lens = [(L, m, none), (m, none, L), (none, L, m)][i % 3]
            out.append(((geo,), L, lens, 1, 1.0))
    return out


def large_case():
    """The three LARGE resolutions as one module at B = 2, L = 8192, lengths 8192 and 5000 (as 1024 and 625 times 8), sc + 2 mag."""
    return (tuple(S.LARGE), S.LARGE_L, (1024, 625), 8, 2.0)


@functools.lru_cache(maxsize=None)
def case_oracle(case):
    """The ragged oracle's fp64 results and its own float32 gaps on one end-to-end case (CPU, once)."""
    res, L, lens, len_mul, w_mag = case
    x, y = SL.signals(len(lens), L)
    return ragged_gaps(x, y, samples_of(lens, len_mul, L), res, 1.0, w_mag)
