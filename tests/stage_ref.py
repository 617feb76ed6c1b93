"""fp64 CPU statement of what the fused narrow-stage kernels compute (csrc/v2w_resblock_fused.hip, csrc/v2w_stage_small.hip) behind
v2w_resblock2_stage_fwd / _fwd_len / _wino_fwd / _wino_fwd_len / _small_fwd and v2w_resblock_pair_fwd, as include/vec2wav_hip.h documents the
calls (not as the kernels index their tiles), and what each entry may differ by.  The helpers are those of tests/disc_ref.py (f64, U) and
tests/tile_ref.py (lrelu, taps_sum, mask_factor, unspecified_past); tests/wino_ref.py has the segments and classes of the Winograd form.

Every function returns (value, bound) per entry, eps = 2^-24 throughout, first order, no tuned constant:

  one conv phase    the value is a sum of k * C products, a bias and a residual; with S the sum of their magnitudes a chain of n fp32 operations
                    on it, in any order and any split, is within n * eps * S: n = k * C plus one per fp32 operation of the prologue and the
                    epilogue (input affine, leaky-relu, bias, residual) - tests/stage_cases.py counts them per record and hands them in.
  two phases        t1_j = x + conv1_j(lrelu(x)) + b1_j carries the field E1_j = n1 * eps * S1_j; leaky-relu is 1-Lipschitz, so it reaches
                    r_j = t1_j + conv2_j(lrelu(t1_j)) + b2_j as E1_j + taps_sum(E1_j, |w2_j|) - also where the fp32 and the fp64 t1 lie on
                    opposite sides of 0 - and  E(r_j) = E1_j + taps_sum(E1_j, |w2_j|) + n2 * eps * S2_j.  Where t1_j is forced to 0 (outside
                    [0, L), at and past an item's end) E1_j is 0.
  branch sum        + (nk - 1) * eps * sum_j |r_j|;  the division scales the bound and adds eps * |quotient|.
  Winograd form     the same propagation with each phase's S and n taken from the Winograd form: an entry is y0 = M0 + M1 + M2 or
                    y1 = M1 - M2 - M3 of its pair, M_c = sum over segments and channels of G_c * u_c.  G_1 = ((g0 + g2) + g1) / 2 can cancel,
                    so its rounding is relative to sum |g| / 2, not to |G_1|: `wino_mag` replaces every transformed weight by the (half-)sum of
                    the magnitudes of the taps it is formed from, every transformed operand by the sum of the magnitudes of its two rows, and
                    takes the larger of the entry's two possible roles (first or second output of a pair: which one it is depends on the tile
                    it falls in, which this statement does not know).  n = segments * C products per class + 2 (weight transform) + 1 (input
                    transform) + 2 (output transform).  The error field E1_j propagates through the same magnitudes.
  gradient form     the same two phases on the header's two formulas; the masks are inputs, their sign is exact, a factor lrelu'() scales
                    the conv's S and its propagated error.
  tail              arg = conv_post(lrelu(out, post_slope)) + post_b: E_arg = taps_sum(E_out, |post_w|) + n_p * eps * S_p; |tanh'| <= 1, so
                    y = tanh(arg) is within E_arg + TANH_C * eps.

TANH_C: the device tanhf's own error in units of 2^-24, doubled and rounded up.  Measured on an MI355X by
test_stage_kernels_gpu.py::test_device_tanhf_error (a tail record whose pre-activation is an exact fp32 number, 114 688 arguments over
[-9, 9], against fp64 tanh of the same argument): 1.253 * 2^-24 (at a = 0.66635), hence TANH_C = 3.

  split-f16 form    (csrc/v2w_stage_split.hip, `split=True`) every product is the sum of three f16 x f16 products: n counts three accumulations
                    per product, and each phase adds the per-product terms of tests/split_ref.py on its own operand and weights,
                    3 * 2^-22 * (sum of |a w|) + 2^-25 * W1 + 2^-38 * wmax * A1.  The residuals x and t1_j exist only as the (hi, lo) halves of
                    their ACTIVATED values; v = unlrelu(hi + lo) is granted 2^-22 |v| (`rebuilt`) and one fp32 division by the slope on the
                    negative side, counted in n.  (Where lo is an f16 subnormal, |a| below about 2^-3, hi + lo is in principle only within
                    2^-25 of a; that floor is NOT granted here, and the records hold without it.)

With lengths, x and every t1_j are zero at and past min(L, len[b] * len_mul); entries there are unspecified (NaN in value and bound), except
the tail's, which are exactly 0 (bound 0)."""
import torch
import torch.nn.functional as F

from tests import split_ref
from tests.disc_ref import U, f64
from tests.tile_ref import _s, lrelu, mask_factor, taps_sum, unspecified_past
from tests.wino_ref import CLASSES, segments

TANH_MEASURED = 1.253       # worst |tanhf(a) - tanh(a)| / 2^-24 seen on the MI355X (at a = 0.66635)
TANH_C = 3                  # 2 * TANH_MEASURED, rounded up to an integer


def _rows(t, v):
    return f64(t)[:, :, None] * v


def _bias(b):
    return 0.0 if b is None else f64(b)[None, :, None]


def _keep(t, ends):
    return torch.arange(t.shape[2])[None, None, :] < torch.as_tensor(ends)[:, None, None]


def _zero_past(t, ends):
    return t if ends is None else torch.where(_keep(t, ends), t, torch.zeros_like(t))


def affine(x, in_a=None, in_s=None, ends=None):
    """x = in_a * in + in_s per (b, c); with `ends` zero at and past the item's end, whatever the tensor holds there."""
    x = _zero_past(f64(x), ends)                                     # (before the arithmetic: the tensor may hold NaN there)
    if in_a is not None:
        x = _rows(in_a, x) + f64(in_s)[:, :, None]
    return _zero_past(x, ends)


def wino_mag(act, wf, dil):
    """The magnitude sum of the Winograd F(2,3) form of conv_{k, dil}(act; wf) per output entry (see the module docstring): the larger of
    the entry's sum as the first (y0: classes 0, 1, 2) and as the second (y1: classes 1, 2, 3) output of a pair (t, t + dil)."""
    A, Wm = f64(act).abs(), f64(wf).abs()
    k, L = Wm.shape[0], A.shape[2]
    h = dil * (k - 1) // 2
    P = h + dil
    ap = F.pad(A, (P, P))

    def row(off):
        return ap[:, :, P + off:P + off + L]

    def mm(G, u):
        return torch.matmul(G.transpose(0, 1), u)
    roles = []
    for t0, use in ((0, (0, 1, 2)), (-dil, (1, 2, 3))):              # the position of the pair's first output relative to the entry
        tot = torch.zeros(A.shape[0], Wm.shape[2], L, dtype=torch.float64)
        for s0, n in segments(k):
            x = [row(t0 - h + (s0 + j) * dil) for j in range(n + 1)]
            g = [Wm[s0 + j] for j in range(n)]
            if n == 3:
                half = (g[0] + g[1] + g[2]) / 2
                G, u = [g[0], half, half, g[2]], [x[0] + x[2], x[1] + x[2], x[2] + x[1], x[1] + x[3]]
            elif n == 2:
                G, u = [g[0], g[0] + g[1], g[1]], [x[0] + x[1], x[1], x[1] + x[2]]
            else:
                G, u = [g[0], g[0]], [x[0], x[1]]
            for cls, Gc, uc in zip(CLASSES[n], G, u):
                if cls in use:
                    tot = tot + mm(Gc, uc)
        roles.append(tot)
    return torch.maximum(roles[0], roles[1])


def phase(act, wf, dil, wino=False):
    """conv_{k, dil}(act; wf), symmetric zero padding -> (sum, the magnitude sum of the form that computes it)."""
    k = wf.shape[0]
    z, S = taps_sum(act, wf, dil, dil * (k - 1) // 2)
    return z, (wino_mag(act, wf, dil) if wino else S)


def spread(E, wf, dil, wino=False):
    """An error field E >= 0 on a conv's operand, as it reaches the conv's output."""
    if wino:
        return wino_mag(E, wf, dil)
    return taps_sum(E, f64(wf).abs(), dil, dil * (wf.shape[0] - 1) // 2)[0]


def split_terms(act, S, wf, dil):
    """The per-product terms of the split-f16 form on one conv phase (tests/split_ref.py): S is the phase's sum of |a w|."""
    h = dil * (wf.shape[0] - 1) // 2
    W1 = taps_sum(torch.ones_like(act), f64(wf).abs(), dil, h)[0]
    A1 = taps_sum(act.abs(), torch.ones_like(f64(wf)), dil, h)[0]
    return split_ref.REL * S + split_ref.A_FLOOR * W1 + split_ref.W_FLOOR * f64(wf).abs().max() * A1


def rebuilt(v):
    """What a residual rebuilt from the halves of its activated value may differ from v by (see the module docstring)."""
    return 2.0 ** -22 * v.abs()


def two_convs(x, br, n1, n2, slope, ends=None, wino=False, res_mode=0, split=False):
    """One branch on x (B, C, L), br = dict(w1, b1, w2, b2, d1, d2) with the weights [k][C][C]:
    res_mode 0: t1 = x + conv1(lrelu(x)) + b1, r = t1 + conv2(lrelu(t1)) + b2;  res_mode 1: t1 = conv1(lrelu(x)) + b1, r = x + conv2(lrelu(t1)) + b2.
    split: the split-f16 form (res_mode 0, no Winograd).  -> (r, E(r), t1, E1)."""
    assert not split or (res_mode == 0 and not wino)
    a1 = lrelu(x, slope)
    c1, S1 = phase(a1, br['w1'], br['d1'], wino)
    X1 = split_terms(a1, S1, br['w1'], br['d1']) + rebuilt(x) if split else 0.0
    t1, S1 = c1 + _bias(br['b1']), S1 + (0.0 if br['b1'] is None else _bias(br['b1']).abs())
    if res_mode == 0:
        t1, S1 = t1 + x, S1 + x.abs()
    t1, E1 = _zero_past(t1, ends), _zero_past(n1 * U * S1 + X1, ends)
    a2 = lrelu(t1, slope)
    c2, S2 = phase(a2, br['w2'], br['d2'], wino)
    X2 = split_terms(a2, S2, br['w2'], br['d2']) + rebuilt(t1) if split else 0.0
    res = t1 if res_mode == 0 else x
    r = res + c2 + _bias(br['b2'])
    S2 = res.abs() + S2 + (0.0 if br['b2'] is None else _bias(br['b2']).abs())
    Er = (E1 if res_mode == 0 else 0.0) + spread(E1, br['w2'], br['d2'], wino) + n2 * U * S2 + X2
    return r, Er, t1, E1


def _divide(v, E, out_div):
    if out_div:
        v = v / _s(out_div)
        E = E / abs(_s(out_div)) + U * v.abs()
    return v, E


def section(x_in, branches, n1, n2, *, slope, in_a=None, in_s=None, out_div=0.0, ends=None, wino=False, split=False):
    """v2w_resblock2_stage_fwd / _wino_fwd / _small_fwd (and their _len forms): out = ((r_0 + r_1) + ...) / out_div.  n1 / n2: the chain
    lengths of every branch's two phases.  -> (value, bound), NaN at and past an item's end."""
    x = affine(x_in, in_a, in_s, ends)
    tot = E = R = None
    for j, br in enumerate(branches):
        r, Er, _, _ = two_convs(x, br, n1[j], n2[j], slope, ends, wino, split=split)
        tot, E, R = (r, Er, r.abs()) if tot is None else (tot + r, E + Er, R + r.abs())
    E = E + (len(branches) - 1) * U * R
    tot, E = _divide(tot, E, out_div)
    if ends is not None:
        tot, E = unspecified_past(tot, ends), unspecified_past(E, ends)
    return tot, E


def tail(out, E_out, post_w, post_b, n_p, *, post_slope, ends=None, c=None):
    """post_out (B, 1, L) = tanh(conv_post(lrelu(out, post_slope)) + post_b), post_w [post_k][C][1]; with `ends` the operand is zero at and past
    the item's end and so is the result (exactly).  -> (value, bound, arg)."""
    c = TANH_C if c is None else c
    if ends is not None:                                             # (`out` is NaN there)
        keep = _keep(out, ends)
        out, E_out = torch.where(keep, out, torch.zeros_like(out)), torch.where(keep, E_out, torch.zeros_like(E_out))
    z = lrelu(out, post_slope)
    k = post_w.shape[0]
    arg, S = taps_sum(z, post_w, 1, (k - 1) // 2)
    if post_b is not None:
        arg, S = arg + f64(post_b)[None, :, None], S + f64(post_b).abs()[None, :, None]
    E = spread(E_out, post_w, 1) + n_p * U * S + c * U
    y = torch.tanh(arg)
    if ends is not None:
        keep = _keep(y, ends)
        y, E = torch.where(keep, y, torch.zeros_like(y)), torch.where(keep, E, torch.zeros_like(E))
    return y, E, arg


def pair(x_in, br, n1, n2, n_add, *, slope, res_mode, in_a=None, in_s=None, add0=None, add1=None, out_div=0.0):
    """One problem of v2w_resblock_pair_fwd: out = ((add0 [+ add1]) + r) [/ out_div].  n_add: the fp32 additions the addends cost."""
    x = affine(x_in, in_a, in_s)
    r, E, _, _ = two_convs(x, br, n1, n2, slope, res_mode=res_mode)
    if add0 is not None:
        a = f64(add0) if add1 is None else f64(add0) + f64(add1)
        mag = r.abs() + f64(add0).abs() + (0.0 if add1 is None else f64(add1).abs())
        r, E = a + r, E + n_add * U * mag
    return _divide(r, E, out_div)


def section_bwd(g_in, branches, mask1, n1, n2, *, mask2, mask2_a=None, mask2_s=None, bwd_slope, in_a=None, in_s=None):
    """The input-gradient form of v2w_resblock2_stage_fwd, the header's two formulas: dr = in_a * in + in_s,
        bwd_mid[j] = dt1_j = dr + lrelu'(mask1[j]) * conv(dr; w1_j, d1_j)
        out        = sum_j dt1_j + lrelu'(mask2_a * mask2 + mask2_s) * sum_j conv(dt1_j; w2_j, d2_j)
    with w1_j / w2_j the weights as the convs apply them ([k][C][C]: the transposed, tap-reversed ones of the forward's conv2_j / conv1_j).
    -> (out, E_out, [(dt1_j, E1_j)])."""
    dr = affine(g_in, in_a, in_s)
    f2, _ = mask_factor(mask2, mask2_a, mask2_s, bwd_slope)
    tot = E = R = None
    mids = []
    for j, br in enumerate(branches):
        f1, _ = mask_factor(mask1[j], None, None, bwd_slope)
        c1, S1 = phase(dr, br['w1'], br['d1'])
        t1, S1 = dr + f1 * c1, dr.abs() + f1.abs() * S1
        E1 = n1[j] * U * S1
        mids.append((t1, E1))
        c2, S2 = phase(t1, br['w2'], br['d2'])
        r, S2 = t1 + f2 * c2, t1.abs() + f2.abs() * S2
        Er = E1 + f2.abs() * spread(E1, br['w2'], br['d2']) + n2[j] * U * S2
        tot, E, R = (r, Er, r.abs()) if tot is None else (tot + r, E + Er, R + r.abs())
    return tot, E + (len(branches) - 1) * U * R, mids
