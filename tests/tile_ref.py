"""fp64 CPU statement of what the f32 tile kernel family computes behind v2w_conv1d_fwd / _fwd_multi / _fwd_len and v2w_convt1d_fwd / _fwd_len,
as include/vec2wav_hip.h documents the calls (not as csrc/v2w_conv_mfma.hip indexes its tiles), and what each entry may differ by.

Tensors are the call's logical operands: `x` is the C_in-channel slice the call reads (B, C_in, in_stride * L), every epilogue operand the
C_out-channel slice it touches (B, C_out, L); where those slices sit in wider tensors (in_ct / out_ct) and at which byte offset is the
caller's business (tests/test_tile_kernels_gpu.py).  Sums are matrix products per tap over explicitly padded signals; the helpers shared with
the discriminator reference (f64, sum_bound, worst_ratio, transpose_flip, wf_to_w) are tests/disc_ref.py's.

Every function returns (value, S).  S is, per entry, the sum of the magnitudes of every term that enters it: the |w| * |act(x)| products, then
|bias|, |residual term|, |addends|, scaled as the value is scaled (mask factor, out_div).  A chain of n fp32 operations on such a sum, in
any order and any split into partial sums, is within n * 2^-24 * S of the exact value to first order (disc_ref.sum_bound): n = k * C_in for
the products plus one per fp32 operation the prologue (input affine, leaky-relu) and the epilogue add - tile_cases.py counts them per record.
out_slope does not scale S: where the fp32 and the exact value straddle 0 the stored values differ by at most the values' own distance.
"""
import numpy as np
import torch
import torch.nn.functional as F

from tests.disc_ref import f64


def _s(v):
    """A float argument of the call as the kernel sees it: rounded to fp32."""
    return float(np.float32(v))


def lrelu(v, slope):
    return v if slope == 1.0 else torch.where(v > 0, v, v * _s(slope))


def _rows(t, v):
    """(B, C) per-row table against a (B, C, L) tensor."""
    return f64(t)[:, :, None] * v


def activate(x, slope=1.0, in_a=None, in_s=None, in_stride=1, in_phase=0, lengths=None):
    """The conv operand: the phase x[..., in_stride * l + in_phase], then in_a * x + in_s per (b, c), then leaky_relu(slope); with `lengths`
    (B end positions) the ACTIVATED signal is zero at and past the item's end, whatever x holds there."""
    x = f64(x)[:, :, in_phase::in_stride] if in_stride > 1 else f64(x)
    if lengths is not None:                      # (before the arithmetic: the tensor may hold NaN there)
        keep = torch.arange(x.shape[2], device=x.device)[None, None, :] < torch.as_tensor(lengths, device=x.device)[:, None, None]
        x = torch.where(keep, x, torch.zeros_like(x))
    if in_a is not None:
        x = _rows(in_a, x) + f64(in_s)[:, :, None]
    x = lrelu(x, slope)
    if lengths is not None:
        x = torch.where(keep, x, torch.zeros_like(x))
    return x


def taps_sum(act, wf, dil, pad_left):
    """out[b][o][l] = sum_{t, c} wf[t][c][o] * act[b][c][l - pad_left + t * dil], act zero outside [0, L): (sum, the same sum of magnitudes)."""
    k, L = wf.shape[0], act.shape[2]
    w = f64(wf)
    right = (k - 1) * dil - pad_left
    assert right >= 0
    ap = F.pad(act, (pad_left, right))

    def run(a, ww):
        return sum(torch.matmul(ww[t].transpose(0, 1), a[:, :, t * dil:t * dil + L]) for t in range(k))
    return run(ap, w), run(ap.abs(), w.abs())


def mask_factor(mask_src, mask_a, mask_s, mask_slope):
    """lrelu'(mask_a * mask_src + mask_s): 1 where the argument is > 0, mask_slope elsewhere (+0, -0 included); and the argument itself."""
    m = f64(mask_src)
    arg = m if mask_a is None else _rows(mask_a, m) + f64(mask_s)[:, :, None]
    return torch.where(arg > 0, torch.ones_like(arg), torch.full_like(arg, _s(mask_slope))), arg


def epilogue(z, S, *, bias=None, res=None, res_a=None, res_s=None, old=None, add0=None, add1=None, out_div=0.0, out_slope=0.0,
             mask_src=None, mask_a=None, mask_s=None, mask_slope=1.0):
    """value = (add0 [+ add1] | old) + (mask * z + bias + (res_a * res + res_s)), then / out_div, then leaky_relu(out_slope), in the header's
    order; `old` is what `out` held (accumulate)."""
    if mask_src is not None:
        f, _ = mask_factor(mask_src, mask_a, mask_s, mask_slope)
        z, S = z * f, S * f.abs()
    if bias is not None:
        z, S = z + f64(bias)[None, :, None], S + f64(bias).abs()[None, :, None]
    if res is not None:
        r = f64(res) if res_a is None else _rows(res_a, f64(res)) + f64(res_s)[:, :, None]
        z, S = z + r, S + r.abs()
    assert old is None or add0 is None
    for t in (old, add0, add1):
        if t is not None:
            z, S = z + f64(t), S + f64(t).abs()
    if out_div:
        z, S = z / _s(out_div), S / abs(_s(out_div))
    if out_slope and out_slope != 1.0:
        z = lrelu(z, out_slope)
    return z, S


def conv1d(x, wf, *, dil=1, pad_left=-1, slope=1.0, in_a=None, in_s=None, in_stride=1, in_phase=0, lengths=None, **epi):
    """v2w_conv1d_fwd (one problem of _fwd_multi / _fwd_len): x (B, C_in, in_stride * L), wf [k][C_in][C_out] -> (value, S) (B, C_out, L).
    pad_left < 0: the symmetric dil * (k - 1) / 2.  With `lengths` the entries at and past an item's end are unspecified: NaN in both."""
    k = wf.shape[0]
    if pad_left < 0:
        assert k % 2 == 1
        pad_left = dil * (k - 1) // 2
    act = activate(x, slope, in_a, in_s, in_stride, in_phase, lengths)
    z, S = taps_sum(act, wf, dil, pad_left)
    z, S = epilogue(z, S, **epi)
    if lengths is not None:
        z, S = unspecified_past(z, lengths), unspecified_past(S, lengths)
    return z, S


def unspecified_past(t, ends):
    keep = torch.arange(t.shape[2], device=t.device)[None, None, :] < torch.as_tensor(ends, device=t.device)[:, None, None]
    return torch.where(keep, t, torch.full_like(t, float('nan')))


def convt1d(x, wf, u, *, slope=1.0, bias=None, lengths=None):
    """v2w_convt1d_fwd: leaky_relu -> ConvTranspose1d(k, stride u, padding (k - u) / 2) -> + bias.  x (B, C_in, L), wf [k][C_in][C_out]
    -> (value, S) (B, C_out, u * L): out[j] = sum_{q, t : j = u q + t - pad} wf[t] act[q], stated on the zero-stuffed signal.  With `lengths`
    (input positions) the outputs at and past u * end are unspecified: NaN."""
    k = wf.shape[0]
    assert k >= u and (k - u) % 2 == 0
    p = (k - u) // 2
    act = activate(x, slope, lengths=lengths)
    B, Cc, L = act.shape
    xs = torch.zeros(B, Cc, (L - 1) * u + 1, dtype=torch.float64, device=act.device)
    xs[:, :, ::u] = act
    xp = F.pad(xs, (k - 1 - p, p + u - 1))
    w = f64(wf)

    def run(a, ww):
        return sum(torch.matmul(ww[t].transpose(0, 1), a[:, :, k - 1 - t:k - 1 - t + L * u]) for t in range(k))
    z, S = run(xp, w), run(xp.abs(), w.abs())
    if bias is not None:
        z, S = z + f64(bias)[None, :, None], S + f64(bias).abs()[None, :, None]
    if lengths is not None:
        ends = [e * u for e in lengths]
        z, S = unspecified_past(z, ends), unspecified_past(S, ends)
    return z, S


def tile_sums(v, NT):
    """Per position tile and row: v (B, C, L) -> (sum, sum of magnitudes, sum of squares) as (B * ceil(L / NT), C) each, tile index
    b * ceil(L / NT) + l // NT - the rows of rowsum_part (NT output positions) and stats_part (NT INPUT positions: pass NT * u)."""
    v = f64(v)
    B, Cc, L = v.shape
    ntl = -(-L // NT)
    vp = F.pad(v, (0, ntl * NT - L)).reshape(B, Cc, ntl, NT).permute(0, 2, 1, 3).reshape(B * ntl, Cc, NT)
    return vp.sum(-1), vp.abs().sum(-1), (vp * vp).sum(-1)
