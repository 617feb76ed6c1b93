"""fp64 CPU statement of what the split-f16 kernels compute (csrc/v2w_conv_split.hip behind v2w_conv1d_fwd / _fwd_multi with V2W_ALGO_SPLIT,
csrc/v2w_stage_split.hip behind v2w_resblock2_stage_split_fwd, the packers v2w_pack_split / v2w_pack_bf16 / v2w_split_pack_batch), as
include/vec2wav_hip.h documents the calls, and what each entry may differ by.  Value and magnitude sum S are tests/tile_ref.py's (conv1d =
activate + taps_sum + epilogue) with one addition the header states: the activated operand is clamped to [-65504, 65504] before it enters.

The bound, derived (nobody tunes it; eps = 2^-24):

  operands      a: the fp32 activated, clamped operand; v = scale * w, scale the layer's power of two with max |v| in [8192, 16384).
                Each is split x = x_hi + x_lo + e_x:  x_hi = rne_f16(x), x_lo = rne_f16(x - x_hi)  (x - x_hi is exact in fp32).
                |x_lo| <= 2^-11 |x|.  e_x is the rounding of x_lo: <= 2^-11 |x_lo| <= 2^-22 |x| while x_lo is a normal f16 number, and
                <= 2^-25 (half the f16 subnormal spacing 2^-24) where it is subnormal - for a and for v alike that is a magnitude below about 2^-3 (|x_lo| <=
                2^-11 |x| < 2^-14), for v hence a weight some 2^-16 of the layer's maximum or less.  In units of w the floor of v is
                2^-25 / scale, and 1 / scale <= 2^-13 wmax (max |v| >= 2^13): <= 2^-38 wmax.
  one product   kept are a_hi v_hi + a_hi v_lo + a_lo v_hi, each exact in fp32 (11 x 11 bits).  With (a_hi + a_lo)(v_hi + v_lo) = kept +
                a_lo v_lo:   a w - kept / scale = a_lo w_lo + e_a w + (a_hi + a_lo) e_w,   so to first order
                    |error| <= 3 * 2^-22 |a w|  +  2^-25 |w|  +  2^-38 wmax |a|
                (the dropped lo * lo term and the rounding of each lo half; the subnormal floor of a_lo; the same floor of w_lo).
  the sum       three accumulations per product and `ops` further fp32 operations (tests/tile_cases.OPS counts them per switch; the
                multiplication by winv = 1 / scale is exact): n = 3 k C_in + ops, and n * eps * S for the chain (disc_ref.sum_bound).
  per entry         bound = (n * 2^-24 + 3 * 2^-22) * S  +  2^-25 * W1  +  2^-38 * wmax * A1
                W1: the sum of |w| over the taps and channels that land inside [0, L); A1: the sum of |a| over the same window; both in
                the scaling of the epilogue (mask factor, out_div), as S is.

With one live input channel per item (the short-chain records) n = 3 k + ops and the bound is about 22 bits of the single products: a lost
lo term (2^-12 of a product), a swap of hi and lo, a channel permuted inside a 16-channel chunk or a wrong winv exceeds it by orders of
magnitude; `without_a_lo` states the first of these on the CPU and tests/test_split_ref_cpu.py shows that the records see it.

bf16 operands in the same kernel (`conv1d_bf16`): the operand rounding is unambiguous without an input affine - leaky-relu as ONE fp32
multiply, then rne to bf16, weights rne to bf16 - and is emulated here; products of two bf16 numbers are exact in fp32, so the bound is
n * 2^-24 * S on the rounded operands with n = k C_in + ops.

The packers are stated bit for bit from the comment above pack_split_kernel: `pack_split`, `pack_bf16`, `unpack_split`."""
import math

import numpy as np
import torch

from tests import tile_ref as R
from tests.disc_ref import U, f64

F16_MAX = 65504.0
REL = 3 * 2.0 ** -22             # per product: lo * lo dropped, each lo half rounded
A_FLOOR = 2.0 ** -25             # half the f16 subnormal spacing: the absolute error of a subnormal a_lo
W_FLOOR = 2.0 ** -38             # the same for w_lo, in units of the layer's max |w| (1 / scale <= 2^-13 wmax)


def clamp(act):
    return act.clamp(-F16_MAX, F16_MAX)


def _left(k, dil, pad_left):
    if pad_left < 0:
        assert k % 2 == 1
        return dil * (k - 1) // 2
    return pad_left


def _mask_kw(epi):
    return {q: epi[q] for q in ('mask_src', 'mask_a', 'mask_s', 'mask_slope', 'out_div') if q in epi}


def epilogue_scale(like, epi):
    """(zeros, the factor by which the epilogue scales the conv's sum: |mask factor| / out_div) in the shape of `like`."""
    one = torch.ones_like(like)
    return R.epilogue(torch.zeros_like(one), one, **_mask_kw(epi))


def conv1d(x, wf, n, *, dil=1, pad_left=-1, slope=1.0, in_a=None, in_s=None, in_stride=1, in_phase=0, **epi):
    """v2w_conv1d_fwd with V2W_ALGO_SPLIT (one problem of _fwd_multi): -> (value, bound) (B, C_out, L), n = 3 k C_in + ops."""
    left = _left(wf.shape[0], dil, pad_left)
    act = clamp(R.activate(x, slope, in_a, in_s, in_stride, in_phase))
    z, S = R.taps_sum(act, wf, dil, left)
    W1 = R.taps_sum(torch.ones_like(act), f64(wf).abs(), dil, left)[0]
    A1 = R.taps_sum(act.abs(), torch.ones_like(f64(wf)), dil, left)[0]
    floor = A_FLOOR * W1 + W_FLOOR * f64(wf).abs().max() * A1
    floor = floor * epilogue_scale(floor, epi)[1]
    value, S = R.epilogue(z, S, **epi)
    return value, (n * U + REL) * S + floor


# ---------------------------------------------------------------------------------------------------------------
# the split itself, in numpy float32 / float16 (both round to nearest even)
def halves(v):
    """fp32 array -> (hi, lo) float16 arrays: hi = rne(v), lo = rne(v - hi)."""
    v = np.asarray(v, dtype=np.float32)
    hi = v.astype(np.float16)
    return hi, (v - hi.astype(np.float32)).astype(np.float16)


def split_scale(wf):
    """scale = 2^(14 - ex) with max |w| = f * 2^ex, f in [0.5, 1); 1 for a zero or non-finite maximum."""
    mx = float(np.max(np.abs(np.asarray(wf, dtype=np.float32)))) if np.size(wf) else 0.0
    if not (mx > 0.0) or not (mx < 3.0e38):
        return 1.0
    return math.ldexp(1.0, 14 - math.frexp(mx)[1])


def activate_f32(x, slope):
    """The kernel's operand without an input affine, in fp32: leaky-relu as one multiply, then the clamp."""
    x = np.asarray(x, dtype=np.float32)
    v = x if slope == 1.0 else np.where(x > 0, x, (x * np.float32(slope)).astype(np.float32))
    return np.clip(v, np.float32(-F16_MAX), np.float32(F16_MAX)).astype(np.float32)


def without_a_lo(x, wf, *, dil=1, pad_left=-1, slope=1.0):
    """What a kernel that drops the a_lo * w_hi products is short of, per entry (fp64): sum of a_lo * w_hi / scale.  No input affine."""
    scale = split_scale(wf)
    _, a_lo = halves(activate_f32(x, slope))
    w_hi, _ = halves(np.asarray(wf, dtype=np.float32) * np.float32(scale))
    left = _left(wf.shape[0], dil, pad_left)
    return R.taps_sum(f64(a_lo.astype(np.float64)), f64(w_hi.astype(np.float64)) / scale, dil, left)[0]


def conv1d_bf16(x, wf, n, *, dil=1, pad_left=-1, slope=1.0, **epi):
    """The same call with V2W_ALGO_BF16 operands on this file's kernel (no input affine): -> (value, bound), n = k C_in + ops."""
    xt = torch.as_tensor(x, dtype=torch.float32)
    a = xt if slope == 1.0 else torch.where(xt > 0, xt, xt * float(np.float32(slope)))
    a, w = f64(a.bfloat16().float()), f64(torch.as_tensor(wf, dtype=torch.float32).bfloat16().float())
    z, S = R.taps_sum(a, w, dil, _left(wf.shape[0], dil, pad_left))
    value, S = R.epilogue(z, S, **epi)
    return value, n * U * S


# ---------------------------------------------------------------------------------------------------------------
# fragment layout: 16-byte element (((mb * nch + ch) * K + t) * 2 + hl) * 64 + lane holds, for j = 0 .. 7, part_hl of
# scale * wf[t][ch * 16 + 8 * (lane >> 5) + j][mb * 32 + (lane & 31)]; rows past C_out are zero
def _fragments(v):
    """[K][C_in][C_out] -> [mb][ch][K][64 lanes][8]: the channel and row of every fragment slot."""
    K, ci, co = v.shape
    nmb, nch = -(-co // 32), ci // 16
    vp = np.zeros((K, ci, nmb * 32), dtype=v.dtype)
    vp[:, :, :co] = v
    # ci = ch * 16 + half * 8 + j, co = mb * 32 + r, lane = half * 32 + r
    return vp.reshape(K, nch, 2, 8, nmb, 32).transpose(4, 1, 0, 2, 5, 3).reshape(nmb, nch, K, 64, 8)


def pack_split(wf):
    """wf [K][C_in][C_out] fp32 -> (int16 [mb][ch][K][2][64][8]: the documented elements of wps, (sc[0], sc[1]) = (1 / scale, scale))."""
    wf = np.asarray(wf, dtype=np.float32)
    scale = split_scale(wf)
    hi, lo = halves(wf * np.float32(scale))
    out = np.stack((_fragments(hi), _fragments(lo)), axis=3)
    return np.ascontiguousarray(out).view(np.int16), (np.float32(1.0) / np.float32(scale), np.float32(scale))


def pack_bf16(wf):
    """The hi slots of v2w_pack_bf16: int16 [mb][ch][K][64][8] = bits of rne_bf16(w); sc = (1, 1); the lo slots are not written."""
    bits = torch.from_numpy(np.ascontiguousarray(np.asarray(wf, dtype=np.float32))).bfloat16().view(torch.int16).numpy()
    return np.ascontiguousarray(_fragments(bits))


def unpack_split(frag, sc0, K, ci, co):
    """The inverse on the documented elements: int16 [mb][ch][K][2][64][8] -> fp64 [K][C_in][C_out] of (hi + lo) * sc0."""
    v = frag.view(np.float16).astype(np.float64)
    v = v[:, :, :, 0] + v[:, :, :, 1]                                        # [mb][ch][K][64][8]
    nmb, nch = v.shape[0], v.shape[1]
    w = v.reshape(nmb, nch, K, 2, 32, 8).transpose(2, 1, 3, 5, 0, 4).reshape(K, ci, nmb * 32)
    return w[:, :, :co] * float(sc0)


def fragment_count(K, ci, co):
    """int16 elements of the documented part of wps."""
    return K * ci * (-(-co // 32) * 32) * 2
