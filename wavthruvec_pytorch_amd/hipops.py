"""Tensor-level wrappers over the C ABI (one function per entry point of include/vec2wav_hip.h).

torch is plumbing here: it owns device memory and the stream; every arithmetic step runs in the
HIP kernels.  All wrappers require contiguous CUDA(ROCm) tensors - fp32 unless the wrapper says bf16 - and
there is deliberately no CPU path.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import torch

from . import _hip

ALGO_AUTO, ALGO_DIRECT, ALGO_MFMA, ALGO_SPLIT, ALGO_BF16, ALGO_WINO = (_hip.ALGO_AUTO, _hip.ALGO_DIRECT, _hip.ALGO_MFMA, _hip.ALGO_SPLIT,
                                                                        _hip.ALGO_BF16, _hip.ALGO_WINO)


def _chk(t: Optional[torch.Tensor], name: str, dtype=torch.float32):
    if t is None:
        return
    if not t.is_cuda:
        raise RuntimeError(f'{name} must live on a GPU: the Vec2Wav HIP path has no CPU fallback')
    if t.dtype != dtype:
        raise TypeError(f'{name} must be {dtype}, got {t.dtype}')
    if not t.is_contiguous():
        raise RuntimeError(f'{name} must be contiguous')


def _stream(t: torch.Tensor) -> int:
    return torch.cuda.current_stream(t.device).cuda_stream


def _declined(rc: int, name: str) -> bool:
    """True when the library declined the shape (V2W_E_SHAPE: nothing was launched, the caller falls through); raises on any other error."""
    if rc == _hip.E_SHAPE:
        return True
    _hip.check(rc, name)
    return False


def _aff(pair):
    """Device pointers of an optional per-sample affine `(a, s)`: NULL for a missing pair - or member: V2W_E_ARG where the library needs both."""
    return (None, None) if pair is None else (_hip.ptr(pair[0]), _hip.ptr(pair[1]))


def _addends(a, add):
    """`add0` / `add1` of an args struct: the up to two tensors a launch adds before its division."""
    add = list(add or [])
    a.add0 = _hip.ptr(add[0]) if len(add) > 0 else None
    a.add1 = _hip.ptr(add[1]) if len(add) > 1 else None


def fold_conv_weight(v, g, out=None, scratch=None):
    """weight_v (C_out,C_in,k), weight_g (C_out,1,1)|None -> wf [k][C_in][C_out]."""
    _chk(v, 'v'); _chk(g, 'g')
    co, ci, k = v.shape
    if out is None:
        out = torch.empty((k, ci, co), device=v.device, dtype=torch.float32)
    if scratch is None:
        scratch = torch.empty((co,), device=v.device, dtype=torch.float32)
    _hip.check(_hip.load().v2w_wn_fold_conv(v.data_ptr(), _hip.ptr(g), out.data_ptr(), scratch.data_ptr(),
                                            co, ci, k, _stream(v)), 'v2w_wn_fold_conv')
    return out


def fold_convt_weight(v, g, out=None, scratch=None):
    """ConvTranspose1d weight_v (C_in,C_out,k), weight_g (C_in,1,1)|None -> wf [k][C_in][C_out]."""
    _chk(v, 'v'); _chk(g, 'g')
    ci, co, k = v.shape
    if out is None:
        out = torch.empty((k, ci, co), device=v.device, dtype=torch.float32)
    if scratch is None:
        scratch = torch.empty((ci,), device=v.device, dtype=torch.float32)
    _hip.check(_hip.load().v2w_wn_fold_convt(v.data_ptr(), _hip.ptr(g), out.data_ptr(), scratch.data_ptr(),
                                             ci, co, k, _stream(v)), 'v2w_wn_fold_convt')
    return out


def transpose_flip(wf, out=None):
    """wf [k][C_in][C_out] -> dgrad weights [k][C_out][C_in] (taps reversed)."""
    k, ci, co = wf.shape
    if out is None:
        out = torch.empty((k, co, ci), device=wf.device, dtype=torch.float32)
    _hip.check(_hip.load().v2w_wf_transpose_flip(wf.data_ptr(), out.data_ptr(), k, ci, co, _stream(wf)), 'v2w_wf_transpose_flip')
    return out


def gather_transpose(wf, t_start, t_step, n, out=None):
    """out[m][C_out][C_in] = wf[t_start + m*t_step][C_in][C_out], m < n (dgrad weights of one transposed-conv phase)."""
    k, ci, co = wf.shape
    if out is None:
        out = torch.empty((n, co, ci), device=wf.device, dtype=torch.float32)
    _hip.check(_hip.load().v2w_wf_gather_transpose(wf.data_ptr(), out.data_ptr(), k, ci, co, t_start, t_step, n, _stream(wf)),
               'v2w_wf_gather_transpose')
    return out


def pack_mfma(wf, out=None, u=1):
    """wf [k][C_in][C_out] -> the same weights as the MFMA A-fragment stream of that layer (u = 1 conv, stride for convT),
    or None when the layer has no MFMA tile configuration."""
    k, ci, co = wf.shape
    if out is None:
        out = torch.empty((k * ci * co,), device=wf.device, dtype=torch.float32)
    rc = _hip.load().v2w_pack_mfma(wf.data_ptr(), out.data_ptr(), k, ci, co, u, _stream(wf))
    return None if _declined(rc, 'v2w_pack_mfma') else out


def pack_mfma_dgrad(wf):
    """wf [k][C_in][C_out] of a conv layer -> the MFMA fragment stream of its input-gradient conv (C_out -> C_in channels, taps reversed),
    or None when that shape has no MFMA tile configuration (then: transpose_flip + the direct kernel)."""
    k, ci, co = wf.shape
    out = torch.empty((k * ci * co,), device=wf.device, dtype=torch.float32)
    rc = _hip.load().v2w_pack_mfma_dgrad(wf.data_ptr(), out.data_ptr(), k, co, ci, _stream(wf))
    return None if _declined(rc, 'v2w_pack_mfma_dgrad') else out


def pack_mfma_batch(w4):
    """w4 [n][k][C_in][C_out] contiguous -> the n packed MFMA streams [n][k*C_in*C_out] in one launch."""
    _chk(w4, 'w4')
    n, k, ci, co = w4.shape
    out = torch.empty((n, k * ci * co), device=w4.device, dtype=torch.float32)
    _hip.check(_hip.load().v2w_pack_mfma_batch(w4.data_ptr(), out.data_ptr(), k, ci, co, 1, n, _stream(w4)), 'v2w_pack_mfma_batch')
    return out


def split_supported(c_in, c_out, u=1):
    """True when the split-f16 kernel (ALGO_SPLIT) serves this layer shape."""
    return bool(_hip.load().v2w_split_supported(c_in, c_out, u))


def split_halves(k, c_in, c_out):
    """Elements (f16) of the wps buffer of one layer: two halves per weight + one 2 KiB unit of padding (the kernel's
    stage copies always move whole tap pairs)."""
    return k * c_in * ((c_out + 31) // 32 * 32) * 2 + 1024      # C_out = 16 is zero-padded to one 32-row block


def split_packable(c_in, c_out):
    """True when pack_split / SplitPlan accept the layer shape (the fused C = 32 stage kernel consumes such fragments too)."""
    return bool(_hip.load().v2w_split_packable(c_in, c_out))


def split_units_halves(k, c_in, c_out):
    """f16 elements of the fragment units of one layer WITHOUT the trailing padding unit (slices of a shared stage buffer)."""
    return k * c_in * ((c_out + 31) // 32 * 32) * 2


def wino_terms(k):
    """Weight matrices of the Winograd F(2,3) form of a k-tap conv (4 / 10 / 15 for k = 3 / 7 / 11); 0 when k is not served."""
    return int(_hip.load().v2w_wino_terms(k))


def pack_wino(wf, out=None):
    """wf [k][C_in][C_out] -> the ALGO_WINO weight stream (v2w_pack_wino: the transformed weights of every segment term in A-fragment
    order), or None when the shape is not served."""
    k, ci, co = wf.shape
    n = wino_terms(k) * ci * co
    if n == 0:
        return None
    if out is None:
        out = torch.empty((n,), device=wf.device, dtype=torch.float32)
    rc = _hip.load().v2w_pack_wino(wf.data_ptr(), out.data_ptr(), k, ci, co, _stream(wf))
    return None if _declined(rc, 'v2w_pack_wino') else out


def pack_split(wf, out=None, sc=None, bf16=False):
    """wf [k][C_in][C_out] -> (wps, sc): the (hi, lo) half-precision MFMA fragments of scale*wf for ALGO_SPLIT and the 4-float
    scale record (sc[0] = 1/scale is the kernel's `winv`)."""
    k, ci, co = wf.shape
    if out is None:
        out = torch.empty((split_halves(k, ci, co),), device=wf.device, dtype=torch.float16)
    if sc is None:
        sc = torch.empty((4,), device=wf.device, dtype=torch.float32)
    fn = _hip.load().v2w_pack_bf16 if bf16 else _hip.load().v2w_pack_split
    _hip.check(fn(wf.data_ptr(), out.data_ptr(), sc.data_ptr(), k, ci, co, _stream(wf)), 'v2w_pack_bf16' if bf16 else 'v2w_pack_split')
    return out, sc


def _conv1d_args(a, x, wf, bias, out, *, k, dil=1, slope=1.0, in_affine=None, res=None, res_affine=None,
                 accumulate=False, out_div=0.0, algo=ALGO_AUTO, wp=None, add=None, mask=None, mask_slope=1.0,
                 in_stride=0, in_phase=0, pad_left=-1, L=None, wps=None, out_slope=0.0, group=None, io_bf16=0, rowsum=None, in_ct=0):
    B, ci, Lx = x.shape
    L = Lx if L is None else L       # strided input: the conv length is Lx / in_stride
    co = out.shape[1]
    a.out_slope = out_slope
    a.rowsum_part = _hip.ptr(rowsum)   # masked f32 MFMA launches: [tiles][C_out][2] per-tile sums of the stored values (bias gradients)
    a.io_bf16 = io_bf16        # ALGO_BF16 only: bit 0 x is bf16, bit 1 out / res / add are bf16 (activation storage of BASELINE configs[2])
    xoff = ooff = 0
    if group is not None:             # (g, C_in per group, C_out per group): this call computes ONE group of a grouped conv
        g, cig, cog = group
        a.in_ct, a.out_ct = ci, co
        xoff, ooff = g * cig * Lx * 4, g * cog * out.shape[2] * 4
        ci, co = cig, cog
    if in_ct:                          # `x` is a C_in-channel slice (a view) of a tensor with in_ct channels per batch item
        a.in_ct = in_ct
    a.in_stride, a.in_phase, a.pad_left = in_stride, in_phase, pad_left
    a.in_ = x.data_ptr() + xoff
    a.in_a, a.in_s = _aff(in_affine)
    a.wf = _hip.ptr(wf); a.wp = _hip.ptr(wp); a.bias = _hip.ptr(bias)
    if wps is not None:           # (fragments, scale record) of pack_split
        a.wps, a.winv = wps[0].data_ptr(), wps[1].data_ptr()
    a.res = _hip.ptr(res)
    a.res_a, a.res_s = _aff(res_affine)
    _addends(a, add)
    if mask is not None:          # (mask_src, (mask_a, mask_s) | None)
        a.mask_src = mask[0].data_ptr()
        a.mask_a, a.mask_s = _aff(mask[1])
    a.mask_slope = mask_slope
    a.out = out.data_ptr() + ooff
    a.B, a.C_in, a.C_out, a.L, a.k, a.dil = B, ci, co, L, k, dil
    a.slope = slope; a.accumulate = int(accumulate); a.out_div = out_div; a.algo = algo


def _len_ptr(lengths, len_mul):
    """Per-item valid lengths of a launch (the *_fwd_len entry points): `lengths` a (B,) int32 tensor on the launch's device - item b's sequence
    ends at lengths[b] * len_mul positions of the call's input rate.  Returns its device pointer."""
    if lengths.dtype != torch.int32 or not lengths.is_cuda or lengths.dim() != 1 or not lengths.is_contiguous():
        raise ValueError('lengths must be a contiguous 1-d int32 tensor on the GPU')
    if int(len_mul) < 1:
        raise ValueError('len_mul must be >= 1')
    return lengths.data_ptr()


def _fwd_or_len(fwd, fwd_len, lengths, len_mul):
    """(entry point, its name, the arguments it takes in front of the stream): `fwd` and none - or, with per-item `lengths`, `fwd_len` and
    (lengths pointer, len_mul)."""
    if lengths is None:
        return getattr(_hip.load(), fwd), fwd, ()
    return getattr(_hip.load(), fwd_len), fwd_len, (_len_ptr(lengths, len_mul), int(len_mul))


def _pop_len(kw):
    """(kwargs without lengths / len_mul, lengths, len_mul)"""
    kw = dict(kw)
    return kw, kw.pop('lengths', None), int(kw.pop('len_mul', 1))


class SplitKSlab:
    """Caller-owned scratch of the split over C_in (v2w_conv1d_args::splitk_ws, ABI v28): launches too small to fill the chip - inference at
    B = 1 - store per-slice partial sums here and a second kernel adds them.  The library allocates nothing: the OWNER of a slab (a
    Generator, one slab per stream it launches on) passes it to conv1d / conv1d_multi / convt1d as `splitk_ws=`; launches that share a
    slab must be ordered on one stream.  Grow-only, so a warmed-up module never allocates inside a HIP graph capture; a slab that is outgrown is
    kept (`retired`), never freed under a captured graph that writes its partial sums there."""

    def __init__(self):
        self.t = None
        self.retired = []     # superseded slabs stay alive with their owner: a HIP graph or a launch plan recorded earlier holds their address

    def ensure(self, nbytes, device):
        if self.t is None or self.t.device != device or self.t.numel() * 4 < nbytes:
            if self.t is not None:
                self.retired.append(self.t)
            self.t = torch.empty(((nbytes + 3) // 4,), device=device, dtype=torch.float32)
        return self.t


def _attach_slab(a, slab, nbytes, device):
    if slab is not None and nbytes > 0:
        t = slab.ensure(int(nbytes), device)
        a.splitk_ws, a.splitk_ws_bytes = t.data_ptr(), t.numel() * 4


_SPLITK_BYTES = {}      # what a launch's split over C_in needs depends on its sizes and switches alone: asked of the library once per combination


def _splitk_bytes(a, n):
    """Bytes of split-over-C_in scratch the launch of these n problems would use (0: unsplit).  The library's answer depends on EVERY problem of
    a multi-problem launch - tap count and dilation (the widest halo picks the tile variant and the grid), the epilogue kind of each - so the key
    holds them all (keyed by problem 0 alone, two launches that differ in problems 1.. could share a stale byte count)."""
    qs = [a[i] for i in range(n)] if n > 1 else [a]
    key = (n,) + tuple((q.B, q.C_in, q.C_out, q.L, q.k, q.dil, q.algo, q.accumulate, q.in_stride, q.pad_left, q.in_ct, q.out_ct, q.io_bf16,
                        bool(q.res), bool(q.add0), bool(q.add1), bool(q.mask_src), bool(q.in_a), bool(q.rowsum_part), bool(q.wps), bool(q.wp),
                        q.out_div != 0.0, q.out_slope != 0.0) for q in qs)
    v = _SPLITK_BYTES.get(key)
    if v is None:
        v = _SPLITK_BYTES[key] = int(_hip.load().v2w_conv1d_splitk_ws_bytes(a if n > 1 else C.byref(a), n))
    return v


def conv1d(x, wf, bias, out, splitk_ws=None, **kw):
    """Fused [affine] -> leaky_relu -> dilated Conv1d -> +bias [+res] [+= out | + add0 (+ add1)] [/ out_div]; see the header.
    splitk_ws: a SplitKSlab (f32 MFMA path only; without one a small launch simply runs unsplit)."""
    if kw.get('wpw') is not None:
        conv1d_wino_multi([(x, wf, bias, out, kw)], splitk_ws=splitk_ws)
        return out
    kw.pop('wpw', None)
    kw, lengths, len_mul = _pop_len(kw)
    a = _hip.Conv1dArgs()
    _conv1d_args(a, x, wf, bias, out, **kw)
    if splitk_ws is not None:
        _attach_slab(a, splitk_ws, _splitk_bytes(a, 1), x.device)
    fn, name, la = _fwd_or_len('v2w_conv1d_fwd', 'v2w_conv1d_fwd_len', lengths, len_mul)
    _hip.check(fn(C.byref(a), *((1, *la) if la else ()), _stream(x)), name)     # (v2w_conv1d_fwd_len - f32 MFMA / Winograd kernels only - takes a count)
    return out


def _conv1d_launch(problems, splitk_ws=None, *, nmin=2, over=None) -> bool:
    """One launch of nmin <= n <= 4 problems (x, wf, bias, out, kwargs without `wpw`) that share B, C_in, C_out, L; `over`: per-problem
    overrides of the kwargs.  False when there was nothing to launch in one piece or the library declined (V2W_E_SHAPE: nothing was launched)."""
    n = len(problems)
    if not nmin <= n <= 4:
        return False
    arr = (_hip.Conv1dArgs * n)()
    lengths = len_mul = None
    for i, (a, (x, wf, bias, out, kw)) in enumerate(zip(arr, problems)):
        kw, lengths, len_mul = _pop_len(kw)          # (every problem of a launch carries the same lengths, or none does)
        _conv1d_args(a, x, wf, bias, out, **{**kw, **(over[i] if over else {})})
    x0 = problems[0][0]
    if splitk_ws is not None:
        _attach_slab(arr[0], splitk_ws, _splitk_bytes(arr, n), x0.device)
    fn, _name, la = _fwd_or_len('v2w_conv1d_fwd_multi', 'v2w_conv1d_fwd_len', lengths, len_mul)
    return not _declined(fn(arr, n, *la, _stream(x0)), 'v2w_conv1d_fwd_multi')


def _without_wpw(problems):
    return [(x, wf, bias, out, {q: v for q, v in kw.items() if q != 'wpw'}) for x, wf, bias, out, kw in problems]


def conv1d_multi(problems, splitk_ws=None):
    """`problems`: list of (x, wf, bias, out, kwargs) sharing B, C_in, C_out, L.  One launch when the MFMA path takes them
    (heaviest first), otherwise one launch each."""
    if any(kw.get('wpw') is not None for *_r, kw in problems):
        return conv1d_wino_multi(problems, splitk_ws=splitk_ws)
    problems = _without_wpw(problems)
    if _conv1d_launch(problems, splitk_ws):
        return
    for x, wf, bias, out, kw in problems:
        conv1d(x, wf, bias, out, splitk_ws=splitk_ws, **kw)


def conv1d_wino_multi(problems, splitk_ws=None):
    """conv1d_multi on the Winograd F(2,3) kernel (ALGO_WINO): every problem's kwargs carry `wpw=` (its pack_wino stream) next to the
    f32 MFMA `algo` / `wp` it runs on when the Winograd kernel declines the launch (V2W_E_SHAPE: nothing was launched)."""
    plain = _without_wpw(problems)
    if all(kw.get('wpw') is not None for *_r, kw in problems):
        if _conv1d_launch(plain, nmin=1, over=[{'algo': ALGO_WINO, 'wp': kw['wpw']} for *_r, kw in problems]):
            return
    conv1d_multi(plain, splitk_ws=splitk_ws)


def conv1d_wino_sum(sources, out, *, dil, slope, out_div=0.0, in_affine=None, lengths=None, len_mul=1, order=None):
    """The summed form of the Winograd F(2,3) kernel (v2w_conv1d_wino_sum_fwd): `sources` = up to three (x_j, wpw_j, bias_j, k_j) of one
    dilation - the second convs of a ResBlock2 stage's branches - in ONE launch on one accumulator:
    out = (sum_j x_j + sum_j conv_j(lrelu(x_j)) + sum_j bias_j) [/ out_div].  Returns False (nothing launched) when the library declines
    the shape (V2W_E_SHAPE); the caller then issues the convs one by one.  `order`: the order in which a workgroup walks the sources (a
    permutation of range(len(sources)); v2w_conv1d_wino_sum_fwd_order) - None: the library's choice (wino_sum_order)."""
    n = len(sources)
    arr = (_hip.Conv1dArgs * max(n, 1))()
    for a, (x, wpw, bias, k) in zip(arr, sources):
        _conv1d_args(a, x, None, bias, out, k=k, dil=dil, slope=slope, out_div=out_div, algo=ALGO_WINO, wp=wpw, in_affine=in_affine)
    lp = _len_ptr(lengths, len_mul) if lengths is not None else None
    if order is None:
        rc = _hip.load().v2w_conv1d_wino_sum_fwd(arr, n, lp, int(len_mul), _stream(out))
    else:
        rc = _hip.load().v2w_conv1d_wino_sum_fwd_order(arr, n, lp, int(len_mul), (C.c_int32 * max(n, 1))(*order), _stream(out))
    return not _declined(rc, 'v2w_conv1d_wino_sum_fwd')


def wino_multi_taken(n, B, c_out, L, dil):
    """Does a V2W_ALGO_WINO launch of n problems of these sizes pass the library's size rule (v2w_conv1d_wino: more than 128 workgroups of
    64 channels x 64 output pairs; below that the caller's f32 MFMA stream runs, split over C_in)?  Host arithmetic, the library's."""
    npairs = dil * ((L + 2 * dil - 1) // (2 * dil))
    return n * B * ((npairs + 63) // 64) * (c_out // 64) > 128


def conv1d_wino_fan(x, branches, *, dil, slope, in_affine=None, res=None, res_affine=None, lengths=None, len_mul=1, only_if_multi_wino=False):
    """The fan-out form of the Winograd F(2,3) kernel (v2w_conv1d_wino_fan_fwd): `branches` = up to three (wpw_j, bias_j, out_j, k_j) of one
    dilation over the SAME input `x` - the first convs of a ResBlock2 stage's branches - in ONE launch that stages x once per tile:
    out_j = conv_j(lrelu(in_affine(x))) + bias_j [+ res_affine(res)], the bits of each conv's own ALGO_WINO launch.  Returns False (nothing
    launched) when the library declines the shape (V2W_E_SHAPE: more than 64 input channels, ...) and for a call with per-item lengths, which
    this form does not serve; the caller then issues conv1d_multi.  `only_if_multi_wino`: also decline a launch that conv1d_wino_multi would
    not run on the Winograd kernel (too few workgroups: its f32 MFMA fallback rounds otherwise) - the planner's "the same bits either way"."""
    if lengths is not None:
        return False
    n = len(branches)
    if only_if_multi_wino and not wino_multi_taken(n, x.shape[0], branches[0][2].shape[1], x.shape[2], dil):
        return False
    arr = (_hip.Conv1dArgs * max(n, 1))()
    for a, (wpw, bias, out, k) in zip(arr, branches):
        _conv1d_args(a, x, None, bias, out, k=k, dil=dil, slope=slope, algo=ALGO_WINO, wp=wpw, in_affine=in_affine, res=res, res_affine=res_affine)
    rc = _hip.load().v2w_conv1d_wino_fan_fwd(arr, n, _stream(x))
    return not _declined(rc, 'v2w_conv1d_wino_fan_fwd')


def wino_sum_order(ks):
    """The order in which the summed launch walks sources of kernel sizes `ks` when none is given (v2w_wino_sum_order; host only)."""
    n = len(ks)
    out = (C.c_int32 * n)()
    _hip.check(_hip.load().v2w_wino_sum_order((C.c_int32 * n)(*ks), n, out), 'v2w_wino_sum_order')
    return tuple(out)


def _convt_shape(B, c_in, c_out, L, k, u):
    """A ConvT1dArgs with the problem sizes filled in."""
    a = _hip.ConvT1dArgs()
    a.B, a.C_in, a.C_out, a.L, a.k, a.u = B, c_in, c_out, L, k, u
    return a


def convt1d(x, wf, bias, out, *, k, u, slope=1.0, algo=ALGO_AUTO, wp=None, stats_part=None, splitk_ws=None, lengths=None, len_mul=1):
    """Fused leaky_relu -> ConvTranspose1d(k, stride u, padding (k-u)//2) -> +bias.  lengths / len_mul: per-item valid lengths at the INPUT
    rate (see _len_ptr; v2w_convt1d_fwd_len); outputs past lengths[b] * len_mul * u are unspecified."""
    B, ci, L = x.shape
    a = _convt_shape(B, ci, out.shape[1], L, k, u)
    a.in_ = x.data_ptr(); a.wf = _hip.ptr(wf); a.wp = _hip.ptr(wp); a.bias = _hip.ptr(bias); a.out = out.data_ptr()
    a.stats_part = _hip.ptr(stats_part)
    a.slope = slope; a.algo = algo
    if splitk_ws is not None:
        _attach_slab(a, splitk_ws, _hip.load().v2w_convt1d_splitk_ws_bytes(C.byref(a)), x.device)
    fn, name, la = _fwd_or_len('v2w_convt1d_fwd', 'v2w_convt1d_fwd_len', lengths, len_mul)
    _hip.check(fn(C.byref(a), *la, _stream(x)), name)
    return out


def convt_wino_tiles(B, c_in, c_out, L, k, u):
    """(position tiles = rows of `stats_part`, workgroups) of the launch convt1d_wino would make for this problem, (0, 0) when the
    upsampler form of the Winograd kernel does not serve the shape (v2w_convt1d_wino_tiles; host only)."""
    a = _convt_shape(B, c_in, c_out, L, k, u)
    wgs = C.c_int32(0)
    tiles = _hip.load().v2w_convt1d_wino_tiles(C.byref(a), C.byref(wgs))
    return (int(tiles), int(wgs.value)) if tiles > 0 else (0, 0)


def convt1d_wino(x, wpw, bias, out, *, k, u, slope=1.0, in_affine=None, stats_part=None):
    """The upsampler form of the Winograd F(2,3) kernel (v2w_convt1d_wino_fwd): leaky_relu -> ConvTranspose1d(k = 2 u, stride u, padding
    u // 2) -> + bias as ONE two-tap conv over u * C_out rows with a pixel-shuffle store; `wpw` = the layer's Winograd stream (the batched
    fold's), `stats_part`: [convt_wino_tiles(...)[0]][C_out][2] per-tile (sum, sumsq).  Returns False (nothing launched) when the library
    declines the shape (V2W_E_SHAPE); the caller then runs convt1d."""
    B, ci, L = x.shape
    a = _convt_shape(B, ci, out.shape[1], L, k, u)
    a.in_ = x.data_ptr(); a.wp = _hip.ptr(wpw); a.bias = _hip.ptr(bias); a.out = out.data_ptr()
    a.stats_part = _hip.ptr(stats_part)
    a.slope = slope
    rc = _hip.load().v2w_convt1d_wino_fwd(C.byref(a), *_aff(in_affine), _stream(x))
    return not _declined(rc, 'v2w_convt1d_wino_fwd')


def pack_bf16_convt(wf, u, out=None):
    """ConvTranspose1d weights wf [k][C_in][C_out] -> bf16 fragments of the virtual 3-tap conv v2w_convt1d_bf16_fwd runs, or None when
    the shape is not served."""
    k, ci, co = wf.shape
    nbytes = int(_hip.load().v2w_pack_bf16_convt_bytes(k, ci, co, u))
    if nbytes == 0:
        return None
    if out is None or out.numel() * out.element_size() < nbytes:
        out = torch.empty((nbytes // 2,), device=wf.device, dtype=torch.bfloat16)
    _hip.check(_hip.load().v2w_pack_bf16_convt(wf.data_ptr(), out.data_ptr(), k, ci, co, u, _stream(wf)), 'v2w_pack_bf16_convt')
    return out


def _convt_bf16_args(x, wps, bias, out, k, u, slope, stats_part, io_bf16=0):
    B, ci, L = x.shape
    a = _convt_shape(B, ci, out.shape[1], L, k, u)
    a.in_ = x.data_ptr(); a.wf = None; a.wp = _hip.ptr(wps); a.bias = _hip.ptr(bias); a.out = _hip.ptr(out)
    a.stats_part = _hip.ptr(stats_part)
    a.slope = slope; a.algo = ALGO_BF16; a.io_bf16 = io_bf16
    return a


def convt_bf16_stats_tiles(x, out, k, u, io_bf16=0):
    """Rows of `stats_part` the bf16 transposed conv fills for exactly this call (tensors, io_bf16: the kernel and with it the tile
    width follow them); 0: shape not served."""
    n = _hip.load().v2w_convt1d_bf16_tiles(C.byref(_convt_bf16_args(x, None, None, out, k, u, 1.0, None, io_bf16)))
    return n if n > 0 else 0


def convt1d_bf16(x, wps, bias, out, *, k, u, slope=1.0, stats_part=None, io_bf16=0):
    """Fused leaky_relu -> ConvTranspose1d(k, stride u, padding (k-u)//2) -> +bias on the bf16 matrix pipe (fp32 accumulate).
    io_bf16 = 3: x and out are bf16 tensors."""
    _hip.check(_hip.load().v2w_convt1d_bf16_fwd(C.byref(_convt_bf16_args(x, wps, bias, out, k, u, slope, stats_part, io_bf16)), _stream(x)),
               'v2w_convt1d_bf16_fwd')
    return out


def cond_gamma_beta(spk, noise, fc_w: Sequence, fc_b: Sequence, sn_w: Sequence, sn_b: Sequence,
                    sn_u: Sequence, sn_v: Sequence, gb: Sequence, z_ws, sigma_ws, training: bool):
    """All stages' [gamma|beta] in one call; sn_u / sn_v are updated in place when training."""
    n = len(fc_w)
    if n > _hip.V2W_MAX_STAGES:
        raise ValueError(f'at most {_hip.V2W_MAX_STAGES} upsample stages are supported')
    a = _hip.CondArgs()
    a.spk = spk.data_ptr(); a.noise = noise.data_ptr()
    for i in range(n):
        a.fc_w[i] = fc_w[i].data_ptr(); a.fc_b[i] = fc_b[i].data_ptr()
        a.sn_w[i] = sn_w[i].data_ptr(); a.sn_b[i] = sn_b[i].data_ptr()
        a.sn_u[i] = sn_u[i].data_ptr(); a.sn_v[i] = sn_v[i].data_ptr()
        a.gb[i] = gb[i].data_ptr()
        a.C[i] = sn_w[i].shape[0] // 2
    a.z_ws = z_ws.data_ptr(); a.sigma_ws = sigma_ws.data_ptr()
    a.n_stages = n; a.B = spk.shape[0]; a.spk_dim = spk.shape[1]; a.noise_dim = noise.shape[1]
    a.training = int(training)
    _hip.check(_hip.load().v2w_cond_gamma_beta(C.byref(a), _stream(spk)), 'v2w_cond_gamma_beta')


def _cond_args(a, spk, noise, fc_w, fc_b, sn_w, sn_b, sn_u, sn_v, sigma_ws):
    n = len(sn_w)
    if n > _hip.V2W_MAX_STAGES:
        raise ValueError(f'at most {_hip.V2W_MAX_STAGES} upsample stages are supported')
    a.spk = _hip.ptr(spk); a.noise = _hip.ptr(noise)
    for i in range(n):
        a.fc_w[i] = _hip.ptr(fc_w[i]) if fc_w is not None else None
        a.fc_b[i] = _hip.ptr(fc_b[i]) if fc_b is not None else None
        a.sn_w[i] = sn_w[i].data_ptr(); a.sn_b[i] = _hip.ptr(sn_b[i]) if sn_b is not None else None
        a.sn_u[i] = _hip.ptr(sn_u[i]) if sn_u is not None else None
        a.sn_v[i] = _hip.ptr(sn_v[i]) if sn_v is not None else None
        a.C[i] = sn_w[i].shape[0] // 2
    a.sigma_ws = sigma_ws.data_ptr()
    a.n_stages = n
    if spk is not None:
        a.B = spk.shape[0]; a.spk_dim = spk.shape[1]; a.noise_dim = noise.shape[1]


def cond_sigma(sn_w: Sequence, sn_u: Sequence, sn_v: Sequence, sigma_ws, training: bool = False):
    """sigma_ws[i] = u_i . (W_i v_i) of every stage (eval: no power iteration - a function of the parameters alone)."""
    a = _hip.CondArgs()
    _cond_args(a, None, None, None, None, sn_w, None, sn_u, sn_v, sigma_ws)
    a.training = int(training)
    _hip.check(_hip.load().v2w_cond_sigma(C.byref(a), _stream(sigma_ws)), 'v2w_cond_sigma')


def cond_affine_eval(spk, noise, fc_w: Sequence, fc_b: Sequence, sn_w: Sequence, sn_b: Sequence, sigma_ws,
                     running_mean: Sequence, running_var: Sequence, eps: Sequence, a_out: Sequence, s_out: Sequence):
    """Eval mode: the folded per-sample affine (a, s) of every stage's Conditional BatchNorm from (spk, noise) in ONE launch
    (sigma_ws from cond_sigma for the current parameters)."""
    e = _hip.CondEvalArgs()
    _cond_args(e.c, spk, noise, fc_w, fc_b, sn_w, sn_b, None, None, sigma_ws)
    for i in range(len(sn_w)):
        e.running_mean[i] = running_mean[i].data_ptr(); e.running_var[i] = running_var[i].data_ptr()
        e.a_out[i] = a_out[i].data_ptr(); e.s_out[i] = s_out[i].data_ptr()
        e.eps[i] = eps[i]
    _hip.check(_hip.load().v2w_cond_affine_eval(C.byref(e), _stream(spk)), 'v2w_cond_affine_eval')


def bn_stats(x, stats, partial_ws):
    """x (B,C,L) -> stats[2C+1] fp64 = [sum | sumsq | count]."""
    B, Cc, L = x.shape
    _hip.check(_hip.load().v2w_bn_stats(x.data_ptr(), stats.data_ptr(), partial_ws.data_ptr(), B, Cc, L, _stream(x)),
               'v2w_bn_stats')
    return stats


def bn_finalize(stats, gb, running_mean, running_var, num_batches_tracked, a_out, s_out, *, training: bool,
                momentum=0.1, eps=1e-5):
    B, C2 = gb.shape
    _hip.check(_hip.load().v2w_bn_finalize(_hip.ptr(stats), gb.data_ptr(), running_mean.data_ptr(), running_var.data_ptr(),
                                           _hip.ptr(num_batches_tracked), a_out.data_ptr(), s_out.data_ptr(),
                                           B, C2 // 2, int(training), momentum, eps, _stream(gb)), 'v2w_bn_finalize')


BN_SLICES = 128


def bn_reduce_finalize_slices(part, ntiles, count, slices, gb, running_mean, running_var, num_batches_tracked, a_out, s_out, *,
                              momentum=0.1, eps=1e-5):
    """Train-mode BatchNorm statistics of a layer whose producer left `ntiles` rows of partial sums, and their fold into (a, s), as two short
    launches: slices of whole rows -> fp64 sums per slice (`slices`: >= BN_SLICES * 2 C doubles), then the finalize kernel adds the slices."""
    B, C2 = gb.shape
    Cc = C2 // 2
    lib, st = _hip.load(), _stream(part)
    _hip.check(lib.v2w_bn_reduce_slices(part.data_ptr(), ntiles, Cc, slices.data_ptr(), BN_SLICES, st), 'v2w_bn_reduce_slices')
    _hip.check(lib.v2w_bn_finalize_slices(slices.data_ptr(), BN_SLICES, float(count), gb.data_ptr(), running_mean.data_ptr(),
                                          running_var.data_ptr(), _hip.ptr(num_batches_tracked), a_out.data_ptr(), s_out.data_ptr(),
                                          B, Cc, momentum, eps, st), 'v2w_bn_finalize_slices')


def affine_apply(x, a, s, out):
    B, Cc, L = x.shape
    _hip.check(_hip.load().v2w_affine_apply(x.data_ptr(), a.data_ptr(), s.data_ptr(), out.data_ptr(), B, Cc, L, _stream(x)),
               'v2w_affine_apply')
    return out


def conv_post_tanh(x, wf, bias, out, *, k, slope, lengths=None, len_mul=1):
    """lengths / len_mul (fp32 input only): per-item valid lengths; out[b, 0, lengths[b] * len_mul:] is stored as exactly 0."""
    B, ci, L = x.shape
    if lengths is not None:
        if x.dtype != torch.float32:
            raise NotImplementedError('conv_post_tanh: per-item lengths need fp32 input')
        _hip.check(_hip.load().v2w_conv_post_tanh_len(x.data_ptr(), wf.data_ptr(), _hip.ptr(bias), out.data_ptr(),
                                                      B, ci, L, k, slope, _len_ptr(lengths, len_mul), int(len_mul), _stream(x)), 'v2w_conv_post_tanh_len')
        return out
    if x.dtype == torch.bfloat16:        # bf16 activation storage: the tail reads bf16, computes and writes fp32
        _hip.check(_hip.load().v2w_conv_post_tanh_bf16in(x.data_ptr(), wf.data_ptr(), _hip.ptr(bias), out.data_ptr(),
                                                         B, ci, L, k, slope, _stream(x)), 'v2w_conv_post_tanh_bf16in')
        return out
    _hip.check(_hip.load().v2w_conv_post_tanh(x.data_ptr(), wf.data_ptr(), _hip.ptr(bias), out.data_ptr(),
                                              B, ci, L, k, slope, _stream(x)), 'v2w_conv_post_tanh')
    return out


def conv_tile_config(B, c_in, c_out, L, k, dil=1, u=1, prefix=False):
    """Name of the conv_tile_kernel instantiation the MFMA path picks for this problem, or None (direct kernel).  The instantiation's
    last template argument (VEC: vector staging) depends on the alignment and stride of the actual input, which a shape query cannot
    know: the name carries the value an aligned, unit-stride tensor of this length gets (L % 4 == 0); `prefix=True` returns the name
    up to that argument, for `startswith` matching of trace names."""
    cfg = (C.c_int32 * 10)()
    if u == 1:
        a = _hip.Conv1dArgs(); a.B, a.C_in, a.C_out, a.L, a.k, a.dil = B, c_in, c_out, L, k, dil
        a.pad_left = -1
        rc = _hip.load().v2w_conv1d_tile_config(C.byref(a), cfg)
    else:
        a = _convt_shape(B, c_in, c_out, L, k, u)
        rc = _hip.load().v2w_convt1d_tile_config(C.byref(a), cfg)
    if rc != 0:
        return None
    # forward instantiation (EPI = 0: no optional epilogue)
    pre = 'conv_tile_kernel<' + ', '.join(str(v) for v in cfg[:9]) + ', 0, '
    return pre if prefix else pre + ('true>' if L % 4 == 0 else 'false>')


def conv_bf16_config(B, nprob, c_in, c_out, L, k, dil=1, u=1, io_bf16=3):
    """Name of the conv_bf16_kernel instantiation a V2W_ALGO_BF16 launch of `nprob` such problems runs (aligned tensors), or None."""
    cfg = (C.c_int32 * 10)()
    if u == 1:
        arr = (_hip.Conv1dArgs * nprob)()
        for a in arr:
            a.B, a.C_in, a.C_out, a.L, a.k, a.dil = B, c_in, c_out, L, k, dil
            a.pad_left = -1
            a.io_bf16 = io_bf16
        rc = _hip.load().v2w_conv1d_bf16_config(arr, nprob, cfg)
    else:
        a = _convt_shape(B, c_in, c_out, L, k, u)
        a.io_bf16 = io_bf16
        a.slope = 0.1              # (the generator's upsamplers; the resident-tile kernel rebuilds nothing from it but checks 0 < slope <= 1)
        rc = _hip.load().v2w_convt1d_bf16_config(C.byref(a), cfg)
    if rc != 0:
        return None
    v = list(cfg)
    if v[5] == 102:         # the resident-tile transposed conv (v2w_convt_bf16_res.hip)
        return 'convt_bf16_res_kernel<' + ', '.join(str(x) for x in v[:5]) + f', {v[9]}>'      # (..., UP, U)
    tf = lambda b: 'true' if b else 'false'
    return 'conv_bf16_kernel<' + ', '.join(str(x) for x in v[:6]) + f', {tf(v[6])}, {tf(v[7])}, {v[8]}, {tf(v[9])}>'


def conv_rowsum_tiles(B, nprob, c_in, c_out, L, k, dil=1):
    """Rows of the `rowsum` array a masked f32 MFMA launch of `nprob` problems of this shape fills per problem (0: no tile configuration)."""
    cfg = (C.c_int32 * 10)()
    a = _hip.Conv1dArgs(); a.B, a.C_in, a.C_out, a.L, a.k, a.dil = B * nprob, c_in, c_out, L, k, dil
    a.pad_left = -1
    if _hip.load().v2w_conv1d_tile_config(C.byref(a), cfg) != 0:
        return 0
    return cfg[9] // nprob


def convt_stats_tiles(B, c_in, c_out, L, k, u):
    """Rows of the `stats_part` array the MFMA transposed conv fills for this problem (0: direct kernel, no fused stats)."""
    cfg = (C.c_int32 * 10)()
    a = _convt_shape(B, c_in, c_out, L, k, u)
    return int(cfg[9]) if _hip.load().v2w_convt1d_tile_config(C.byref(a), cfg) == 0 else 0


def bn_reduce_partials(part, ntiles, Cc, count, stats):
    _hip.check(_hip.load().v2w_bn_reduce_partials(part.data_ptr(), ntiles, Cc, float(count), stats.data_ptr(), _stream(part)),
               'v2w_bn_reduce_partials')
    return stats


def bn_reduce_finalize(part, ntiles, count, stats, gb, running_mean, running_var, num_batches_tracked, a_out, s_out, *, momentum=0.1, eps=1e-5):
    """bn_reduce_partials + bn_finalize(training=True) in one launch (v2w_bn_reduce_finalize): same values, bit for bit."""
    B, C2 = gb.shape
    _hip.check(_hip.load().v2w_bn_reduce_finalize(part.data_ptr(), ntiles, float(count), gb.data_ptr(), running_mean.data_ptr(),
                                                  running_var.data_ptr(), _hip.ptr(num_batches_tracked), stats.data_ptr(), a_out.data_ptr(),
                                                  s_out.data_ptr(), B, C2 // 2, momentum, eps, _stream(gb)), 'v2w_bn_reduce_finalize')
    return a_out, s_out


class FoldPlan:
    """Device-resident descriptor table for v2w_fold_pack_batch: every MFMA layer folded + packed in two launches."""

    def __init__(self, layers, device):
        """layers: list of (v, g|None, wp, c_in, c_out, k, u, transposed[, wf|None[, wpd|None[, wpw|None]]]) with tensors already on `device`; wf: the
        plain layout [k][C_in][C_out] as well, wpd: the fragment stream of the layer's input-gradient conv as well (training forwards), wpw: the
        layer's ALGO_WINO stream as well."""
        n = len(layers)
        self.n = n
        layers = [tuple(l) + (None,) * (11 - len(l)) for l in layers]
        rows = [(l[3] if l[7] else l[4]) for l in layers]
        self.scale = torch.empty((sum(rows),), device=device, dtype=torch.float32)
        descs = (_hip.FoldDesc * n)()
        off = 0
        for d, (v, g, wp, ci, co, k, u, tr, wf, wpd, wpw), r in zip(descs, layers, rows):
            d.v = v.data_ptr(); d.g = _hip.ptr(g); d.wp = wp.data_ptr()
            d.wf = _hip.ptr(wf); d.wpd = _hip.ptr(wpd); d.wpw = _hip.ptr(wpw)
            d.scale = self.scale.data_ptr() + 4 * off
            d.c_in, d.c_out, d.k, d.u, d.transposed = ci, co, k, u, int(tr)
            off += r
        starts = (C.c_int32 * (2 * (n + 1)))()
        lds = _hip.load().v2w_fold_plan(descs, n, starts)
        _hip.check(0 if lds > 0 else (lds or -1), 'v2w_fold_plan')
        self.lds = lds
        self.nblk_scale, self.nblk_pack = starts[n], starts[2 * n + 1]
        self.descs_dev = torch.frombuffer(bytearray(bytes(descs)), dtype=torch.uint8).to(device)
        self.starts_dev = torch.tensor(list(starts), dtype=torch.int32, device=device)
        self.key = tuple((v.data_ptr(), 0 if g is None else g.data_ptr(), wp.data_ptr()) for (v, g, wp, *_r) in layers)

    def run(self):
        _hip.check(_hip.load().v2w_fold_pack_batch(self.descs_dev.data_ptr(), self.starts_dev.data_ptr(), self.n,
                                                   self.nblk_scale, self.nblk_pack, self.lds,
                                                   torch.cuda.current_stream(self.scale.device).cuda_stream),
                   'v2w_fold_pack_batch')


class SplitPlan:
    """Device-resident descriptor table for v2w_split_pack_batch: every split-f16 layer folded (weight norm) and packed into
    its (hi, lo) fragment stream in three launches."""

    def __init__(self, layers, device, bf16=False):
        """layers: list of (v (C_out, C_in, k), g|None, wps, sc) with tensors already on `device`; bf16: fragments for ALGO_BF16."""
        n = len(layers)
        self.n = n
        self.bf16 = bool(bf16)
        self.rowscale = torch.empty((sum(v.shape[0] for v, *_ in layers),), device=device, dtype=torch.float32)
        descs = (_hip.SplitDesc * n)()
        starts = [0] * (2 * (n + 1))
        off = blocks = 0
        for i, (d, (v, g, wps, sc)) in enumerate(zip(descs, layers)):
            co, ci, k = v.shape
            d.v = v.data_ptr(); d.g = _hip.ptr(g); d.wps = wps.data_ptr(); d.sc = sc.data_ptr()
            d.rowscale = self.rowscale.data_ptr() + 4 * off
            d.c_in, d.c_out, d.k, d.mode = ci, co, k, int(bf16)
            starts[i], starts[n + 1 + i] = off, blocks
            off += co
            blocks += ((co + 31) // 32) * (ci // 16)
        starts[n], starts[2 * n + 1] = off, blocks
        self.nblk_rows, self.nblk_pack = off, blocks
        self.k_max = max(v.shape[2] for v, *_ in layers)
        self.descs_dev = torch.frombuffer(bytearray(bytes(descs)), dtype=torch.uint8).to(device)
        self.starts_dev = torch.tensor(starts, dtype=torch.int32, device=device)
        self.key = tuple((v.data_ptr(), 0 if g is None else g.data_ptr(), w.data_ptr()) for (v, g, w, _s) in layers)

    def run(self):
        _hip.check(_hip.load().v2w_split_pack_batch(self.descs_dev.data_ptr(), self.starts_dev.data_ptr(), self.n,
                                                    self.nblk_rows, self.nblk_pack, self.k_max, int(self.bf16),
                                                    torch.cuda.current_stream(self.rowscale.device).cuda_stream),
                   'v2w_split_pack_batch')


def resblock_pair_multi(problems):
    """`problems`: list of dicts(x, in_affine, wp1, b1, wp2, b2, out, k, dil1, dil2, res_mode, slope, add, out_div) sharing B, C, L.
    Returns False (nothing launched) when the fused pair kernel does not take the shape."""
    n = len(problems)
    arr = (_hip.PairArgs * n)()
    for a, q in zip(arr, problems):
        x = q['x']
        B, Cc, L = x.shape
        a.in_ = x.data_ptr()
        a.in_a, a.in_s = _aff(q.get('in_affine'))
        a.wp1 = q['wp1'].data_ptr(); a.bias1 = _hip.ptr(q['b1']); a.wp2 = q['wp2'].data_ptr(); a.bias2 = _hip.ptr(q['b2'])
        _addends(a, q.get('add'))
        a.out = q['out'].data_ptr()
        a.B, a.C, a.L, a.k, a.dil1, a.dil2 = B, Cc, L, q['k'], q['dil1'], q['dil2']
        a.res_mode = q['res_mode']; a.slope = q['slope']; a.out_div = q.get('out_div', 0.0)
    rc = _hip.load().v2w_resblock_pair_fwd(arr, n, _stream(problems[0]['x']))
    return not _declined(rc, 'v2w_resblock_pair_fwd')


def _stage_shape(a, B, Cc, L, ks, dil1s, dil2s):
    """nk, B, C, L and the branches' k / dil1 / dil2 of a StageArgs or a StageSplitArgs; returns `a`."""
    for j, (k, d1, d2) in enumerate(zip(ks, dil1s, dil2s)):
        a.k[j], a.dil1[j], a.dil2[j] = k, d1, d2
    a.nk, a.B, a.C, a.L = len(ks), B, Cc, L
    return a


def _branch_shapes(branches):
    """(ks, dil1s, dil2s) of a list of branch dicts."""
    return [q['k'] for q in branches], [q['dil1'] for q in branches], [q['dil2'] for q in branches]


def _post(a, post):
    """post_* of a stage struct from (wf [k][C][1], bias | None, y (B, 1, L) fp32, k, slope): the generator's tail fused behind the C = 16 stage."""
    if post is not None:
        a.post_w, a.post_b, a.post_out = post[0].data_ptr(), _hip.ptr(post[1]), post[2].data_ptr()
        a.post_k, a.post_slope = post[3], post[4]


def _stage_args(x, in_affine, branches, out, slope, out_div, keys, post=None):
    """A filled StageArgs; `keys`: the names under which the branch dicts hold the first / second conv's weights."""
    a = _stage_shape(_hip.StageArgs(), *x.shape, *_branch_shapes(branches))
    a.in_ = x.data_ptr(); a.in_a, a.in_s = _aff(in_affine)
    for j, br in enumerate(branches):
        a.wp1[j] = br[keys[0]].data_ptr(); a.bias1[j] = _hip.ptr(br['b1'])
        a.wp2[j] = br[keys[1]].data_ptr(); a.bias2[j] = _hip.ptr(br['b2'])
    a.out = _hip.ptr(out)
    a.slope = slope; a.out_div = out_div
    _post(a, post)
    return a


def _stage_split_args(B, Cc, L, ks, dil1s, dil2s, *, slope, out_div, bf16=True, io_bf16=3, rb1=False, branches=(), in_affine=None, post=None,
                      up=None):
    """A filled StageSplitArgs: the sizes and switches a shape query asks with and - launches - the branches' weights (dicts(wps1, b1, wps2,
    b2)), the input affine, the fused tail and the fused upsampler (wps, bias, out, stats_part, k, u, slope; a query gives the last three)."""
    a = _stage_shape(_hip.StageSplitArgs(), B, Cc, L, ks, dil1s, dil2s)
    a.rb1, a.slope, a.out_div, a.bf16, a.io_bf16 = int(rb1), slope, out_div, int(bf16), io_bf16
    a.in_a, a.in_s = _aff(in_affine)
    for j, q in enumerate(branches):
        a.wps1[j], a.sc1[j], a.bias1[j] = q['wps1'][0].data_ptr(), q['wps1'][1].data_ptr(), _hip.ptr(q['b1'])
        a.wps2[j], a.sc2[j], a.bias2[j] = q['wps2'][0].data_ptr(), q['wps2'][1].data_ptr(), _hip.ptr(q['b2'])
    if up is not None:
        a.up_wps, a.up_bias, a.up_out, a.up_stats_part = (_hip.ptr(t) for t in up[:4])
        a.up_k, a.up_u, a.up_slope = up[4:]
    _post(a, post)
    return a


def resblock1_pairs_ok(B, Cc, L, ks, dil1s, dil2s, *, slope) -> bool:
    """Shape query: would resblock1_pairs_bf16 take these problems (kernel sizes `ks`, dilations of the first / second conv of the pair)?"""
    a = _stage_split_args(B, Cc, L, ks, dil1s, dil2s, slope=slope, out_div=0.0, rb1=True)
    return _hip.load().v2w_resblock2_stage_split_config(C.byref(a)) == 0


def resblock2_stage_split_ok(B, Cc, L, ks, dil1s, dil2s, *, slope, bf16=True, io_bf16=3) -> bool:
    """Shape query: would resblock2_stage_split run this stage (nk branches of kernel sizes `ks`, dilations `dil1s` / `dil2s`) as one
    kernel on aligned tensors?  Asked of the library (v2w_resblock2_stage_split_config), nothing is launched."""
    a = _stage_split_args(B, Cc, L, ks, dil1s, dil2s, slope=slope, out_div=float(len(ks)), bf16=bf16, io_bf16=io_bf16)
    return _hip.load().v2w_resblock2_stage_split_config(C.byref(a)) == 0


def resblock2_stage_up_tiles(B, Cc, L, ks, dil1s, dil2s, *, slope, up_k, up_u, up_slope) -> int:
    """Rows of the `stats_part` array the stage kernel WITH the next stage's upsampler fused behind it fills (resblock2_stage_split(up=...)),
    or 0 when the library does not run this stage fused (shape query, nothing is launched)."""
    a = _stage_split_args(B, Cc, L, ks, dil1s, dil2s, slope=slope, out_div=float(len(ks)), up=(None, None, None, None, up_k, up_u, up_slope))
    n = _hip.load().v2w_resblock2_stage_up_tiles(C.byref(a))
    return n if n > 0 else 0


def resblock1_pairs_bf16(ins, in_affine, branches, outs, *, slope, out_div=0.0, add=None):
    """ResBlock1 on bf16 tensors (v2w_stage_split_args::rb1): len(branches) independent problems in one launch, problem p computing
    outs[p] = (x_p + conv2_p(lrelu(conv1_p(lrelu x_p) + b1_p)) + b2_p [+ add[0] + add[1]]) / out_div with x_p = a * ins[p] + s.  `branches`:
    dicts(wps1, b1, wps2, b2, k, dil1, dil2) as for resblock2_stage_split; `add`: up to two bf16 tensors the LAST problem adds before the
    division.  Returns False when the shape is not taken."""
    a = _stage_split_args(*ins[0].shape, *_branch_shapes(branches), slope=slope, out_div=out_div, rb1=True, branches=branches, in_affine=in_affine)
    for j in range(len(branches)):
        a.in_b[j] = ins[j].data_ptr(); a.out_b[j] = outs[j].data_ptr()
    _addends(a, add)
    rc = _hip.load().v2w_resblock2_stage_split_fwd(C.byref(a), _stream(ins[0]))
    return not _declined(rc, 'v2w_resblock2_stage_split_fwd (rb1)')


def resblock2_stage_split(x, in_affine, branches, out, *, slope, out_div, bf16=False, io_bf16=0, post=None, up=None):
    """Split-operand (f16x3 / bf16) form of resblock2_stage for C == 32.  `branches`: list of dicts(wps1, b1, wps2, b2, k, dil1, dil2)
    with wps* = (fragments, scale record) of pack_split / SplitPlan.  Returns False when the shape is not taken.
    up = (wps of pack_bf16_convt, bias, out (B, C / 2, u L) bf16, stats_part | None, k, u, slope): the NEXT stage's upsampler run on the
    stage's output inside the same kernel (`out` may be None: it is not written)."""
    a = _stage_split_args(*x.shape, *_branch_shapes(branches), slope=slope, out_div=out_div, bf16=bf16, io_bf16=io_bf16, branches=branches,
                          in_affine=in_affine, post=post, up=up)
    a.in_ = x.data_ptr(); a.out = _hip.ptr(out)
    rc = _hip.load().v2w_resblock2_stage_split_fwd(C.byref(a), _stream(x))
    return not _declined(rc, 'v2w_resblock2_stage_split_fwd')


def branch_convs_bf16(mode, ins, in_affine, wps, biases, outs, ks, dils, *, slope, out_div=0.0):
    """The first (mode 0) or second (mode 1) convs of the residual branches of a wide ResBlock2 stage on bf16 tensors in ONE launch
    (v2w_branch_convs_bf16_fwd).  mode 0: ins = [x], outs = [t1_j]; mode 1: ins = [t1_j], outs = [out].  False: shape not served."""
    a = _hip.BranchConvsArgs()
    n = len(wps)
    x = ins[0]
    for t in list(ins) + list(outs):
        if t.dtype != torch.bfloat16 or not t.is_contiguous() or t.shape != x.shape:
            raise ValueError('branch_convs_bf16: contiguous bf16 (B, C, L) tensors of one shape')
    B, Cc, L = x.shape
    for j in range(n):
        a.wps[j] = wps[j].data_ptr(); a.bias[j] = _hip.ptr(biases[j]); a.k[j] = ks[j]; a.dil[j] = dils[j]
    for j, t in enumerate(ins):
        a.in_[j] = t.data_ptr()
    for j, t in enumerate(outs):
        a.out[j] = t.data_ptr()
    a.in_a, a.in_s = _aff(in_affine)
    a.nbr, a.mode, a.B, a.C, a.L = n, mode, B, Cc, L
    a.slope, a.out_div = slope, out_div
    rc = _hip.load().v2w_branch_convs_bf16_fwd(C.byref(a), _stream(x))
    return not _declined(rc, 'v2w_branch_convs_bf16_fwd')


def resblock2_stage(x, in_affine, branches, out, *, slope, out_div, post=None, bwd=None, lengths=None, len_mul=1):
    """Whole ResBlock2 residual section of a narrow stage in one kernel.  `branches`: list of dicts(wp1, b1, wp2, b2, k, dil1, dil2).
    post = (wf [k][C][1], bias | None, y (B, 1, L) fp32, k, slope): the generator's tail fused behind the 16-channel stage - `out` may be None,
    it is not written.  bwd = (t1s [nk], dt1s [nk], xr, (a, s) | None, mask_slope[, rowsums [nk]]): the section's input gradient instead (v2w_stage_args::bwd_*:
    x = dL/d(out), in_affine = (1 / nk, 0), wp1 / wp2 the transposed streams of conv2 / conv1, slope 1).
    lengths / len_mul (forward form): per-item valid lengths (see _len_ptr; v2w_resblock2_stage_fwd_len); with `post`, y[b, 0, lengths[b] *
    len_mul:] is exactly 0.
    Returns False (nothing launched) when the shape is not taken."""
    a = _stage_args(x, in_affine, branches, out, slope, out_div, ('wp1', 'wp2'), post)
    if bwd is not None:
        t1s, dt1s, xr, xaff, mslope = bwd[:5]
        rowsums = bwd[5] if len(bwd) > 5 else None
        for j in range(len(branches)):
            a.bwd_mask1[j] = t1s[j].data_ptr(); a.bwd_mid[j] = dt1s[j].data_ptr()
            a.bwd_rowsum[j] = _hip.ptr(rowsums[j]) if rowsums is not None else None
        a.bwd_mask2 = xr.data_ptr()
        a.bwd_mask2_a, a.bwd_mask2_s = _aff(xaff)
        a.bwd_slope = mslope
    fn, _name, la = _fwd_or_len('v2w_resblock2_stage_fwd', 'v2w_resblock2_stage_fwd_len', lengths, len_mul)
    return not _declined(fn(C.byref(a), *la, _stream(x)), 'v2w_resblock2_stage_fwd')


def resblock2_stage_wino(x, in_affine, branches, out, *, slope, out_div, lengths=None, len_mul=1):
    """Winograd F(2,3) form of `resblock2_stage` for the plain forward of a 32-channel stage (v2w_resblock2_stage_wino_fwd).  `branches`:
    list of dicts(wpw1, b1, wpw2, b2, k, dil1, dil2) with the pack_wino streams of the layers.  Returns False (nothing launched) when the
    shape is not taken."""
    a = _stage_args(x, in_affine, branches, out, slope, out_div, ('wpw1', 'wpw2'))
    fn, _name, la = _fwd_or_len('v2w_resblock2_stage_wino_fwd', 'v2w_resblock2_stage_wino_fwd_len', lengths, len_mul)
    return not _declined(fn(C.byref(a), *la, _stream(x)), 'v2w_resblock2_stage_wino_fwd')


def resblock2_stage_wino_tile(B, Cc, L, ks, dil1s, dil2s) -> int:
    """Outputs one tile of `resblock2_stage_wino` keeps (tiles start that many positions apart; 0: shape not taken).  Host only."""
    return _hip.load().v2w_resblock2_stage_wino_tile(C.byref(_stage_shape(_hip.StageArgs(), B, Cc, L, ks, dil1s, dil2s)))


def resblock2_stage_bwd_rows(B, Cc, L, ks, dil1s, dil2s) -> int:
    """Rows of [C][2] floats per branch the input-gradient form of `resblock2_stage` writes into its `rowsums` buffers (0: shape not taken).
    dil1s / dil2s as handed to the kernel (conv2's dilations first)."""
    return _hip.load().v2w_resblock2_stage_bwd_rows(C.byref(_stage_shape(_hip.StageArgs(), B, Cc, L, ks, dil1s, dil2s)))


def resblock2_stage_small(x, in_affine, branches, out, *, slope, out_div):
    """The same section for an 8-channel stage (v2w_resblock2_stage_small_fwd: fp32 FMAs, x read once, t1_j in LDS).  `branches`: list of
    dicts(wf1, b1, wf2, b2, k, dil1, dil2) with the FOLDED weights [k][C][C].  Returns False when the shape is not taken."""
    a = _stage_args(x, in_affine, branches, out, slope, out_div, ('wf1', 'wf2'))
    rc = _hip.load().v2w_resblock2_stage_small_fwd(C.byref(a), _stream(x))
    return not _declined(rc, 'v2w_resblock2_stage_small_fwd')


def wgrad(x, dy, *, k, dil=1, u=1, slope=1.0, x_affine=None, out=None):
    """Weight gradient dwf [k][C_in][C_out] of a fused lrelu -> Conv1d (u = 1) or lrelu -> ConvTranspose1d (stride u).
    x (B, C_in, Lq) is the forward conv's input (before the affine / activation), dy (B, C_out, u*Lq) the output gradient."""
    B, ci, Lq = x.shape
    co = dy.shape[1]
    lib = _hip.load()
    ns = lib.v2w_wgrad_slabs(B, ci, co, Lq)
    if ns == 0:
        raise _hip.HipLibraryError(f'v2w_wgrad: no configuration for C_in={ci}, C_out={co}')
    if out is None:
        out = torch.empty((k, ci, co), device=x.device, dtype=torch.float32)
    slab = torch.empty((ns * k * ci * co,), device=x.device, dtype=torch.float32)
    xa, xs = _aff(x_affine)
    _hip.check(lib.v2w_wgrad(x.data_ptr(), xa, xs, dy.data_ptr(), out.data_ptr(), slab.data_ptr(), B, ci, co, Lq, k, dil, u, slope,
                             _stream(x)), 'v2w_wgrad')
    return out


def wgrad_bf16(x, dy, *, k, dil=1, slope=1.0, x_affine=None, out=None):
    """Conv1d weight gradient dwf [k][C_in][C_out] from bf16 operands with fp32 accumulation (v2w_wgrad_bf16): x and dy both fp32 (rounded
    on the way in) or both bf16 tensors.  Returns None when the layer shape has no bf16 instantiation (the caller runs `wgrad`)."""
    B, ci, Lq = x.shape
    co = dy.shape[1]
    if x.dtype != dy.dtype or x.dtype not in (torch.float32, torch.bfloat16):
        raise TypeError('v2w_wgrad_bf16: x and dy must both be float32 or both bfloat16')
    lib = _hip.load()
    ns = lib.v2w_wgrad_bf16_slabs(B, ci, co, Lq, k)
    if ns == 0:
        return None
    if out is None:
        out = torch.empty((k, ci, co), device=x.device, dtype=torch.float32)
    slab = torch.empty((ns * k * ci * co,), device=x.device, dtype=torch.float32)
    xa, xs = _aff(x_affine)
    rc = lib.v2w_wgrad_bf16(x.data_ptr(), xa, xs, dy.data_ptr(), out.data_ptr(), slab.data_ptr(), B, ci, co, Lq, k, dil, slope,
                            3 if x.dtype == torch.bfloat16 else 0, _stream(x))
    if rc == _hip.E_SHAPE:
        return None
    _hip.check(rc, 'v2w_wgrad_bf16')
    return out


def convt1d_dgrad(dy, wf, out, *, k, u, mask=None, mask_slope=1.0, algo=ALGO_AUTO):
    """Input gradient of the fused lrelu -> ConvTranspose1d(k, stride u, pad (k-u)/2): dx = lrelu'(x) * sum over the u
    output phases of a small Conv1d on that phase of dy.  dy (B, C_out, u*L), wf [k][C_in][C_out], out (B, C_in, L)."""
    pad = (k - u) // 2
    L = out.shape[2]
    B, co = dy.shape[0], dy.shape[1]
    # float4-aligned lengths: de-interleave dy once into its u phases stacked along the channels (B, u*C_out, L) - one streaming pass -
    # so that every phase conv reads unit-stride rows through the vector staging path (the strided form stages element by element and
    # ran at less than half the forward's rate)
    dyp = None
    if algo == ALGO_AUTO and L % 4 == 0 and conv_tile_config(B, co, out.shape[1], L, 3) is not None:
        dyp = phase_split(dy, L=L * u, inner=1, s=u)                    # (B, u * C_out, L)
    for r in range(u):
        t0, c = (r + pad) % u, (r + pad) // u
        nt = (k - t0 + u - 1) // u
        wr = gather_transpose(wf, t0, u, nt)                   # [nt][C_out][C_in]
        if dyp is not None:
            conv1d(dyp[:, r * co:(r + 1) * co, :], wr, None, out, k=nt, dil=1, slope=1.0, accumulate=(r > 0), wp=pack_mfma(wr), mask=mask,
                   mask_slope=mask_slope, pad_left=c, in_ct=u * co, algo=algo)
        else:
            conv1d(dy, wr, None, out, k=nt, dil=1, slope=1.0, accumulate=(r > 0), wp=pack_mfma(wr), mask=mask, mask_slope=mask_slope,
                   in_stride=u, in_phase=r, pad_left=c, L=L, algo=algo)
    return out


# ---------------------------------------------------------------------------------------------------------------
# backward building blocks
def cbn_backward(dx, xr, gb, stats, running_mean, running_var, *, training, eps=1e-5, sync=None):
    """CondBN backward: returns (dxr, dgb).  `sync(csum)` all-reduces the per-channel sums in data-parallel runs."""
    B, Cc, L = dx.shape
    dev = dx.device
    lib = _hip.load()
    s12 = torch.empty((2 * B * Cc,), device=dev)
    dgb = torch.empty((B, 2 * Cc), device=dev)
    csum = torch.empty((2 * Cc,), device=dev, dtype=torch.float64)
    st = _stream(dx)
    _hip.check(lib.v2w_cbn_bwd_sums(dx.data_ptr(), xr.data_ptr(), gb.data_ptr(), _hip.ptr(stats), running_mean.data_ptr(),
                                    running_var.data_ptr(), s12.data_ptr(), dgb.data_ptr(), csum.data_ptr(), B, Cc, L,
                                    int(training), eps, st), 'v2w_cbn_bwd_sums')
    if sync is not None and training:
        sync(csum)
    tab = torch.empty((B * Cc + 2 * Cc,), device=dev)
    dxr = torch.empty_like(dx)
    _hip.check(lib.v2w_cbn_bwd_apply(dx.data_ptr(), xr.data_ptr(), gb.data_ptr(), _hip.ptr(stats), csum.data_ptr(),
                                     running_mean.data_ptr(), running_var.data_ptr(), tab.data_ptr(), dxr.data_ptr(), B, Cc, L,
                                     int(training), eps, st), 'v2w_cbn_bwd_apply')
    return dxr, dgb


def tail_backward(dy, y, x, wf, *, k, slope):
    """tanh + conv_post backward: returns (dx, dwf [k][C_in][1], dp) - d bias = dp.sum()."""
    B, ci, L = x.shape
    dev = x.device
    dp = torch.empty((B, 1, L), device=dev)
    part = torch.empty((ci * k * 512,), device=dev, dtype=torch.float64)
    dx = torch.empty_like(x)
    dwf = torch.empty((k, ci, 1), device=dev)
    _hip.check(_hip.load().v2w_tail_bwd(dy.data_ptr(), y.data_ptr(), x.data_ptr(), wf.data_ptr(), dp.data_ptr(), part.data_ptr(),
                                        dx.data_ptr(), dwf.data_ptr(), B, ci, L, k, slope, _stream(x)), 'v2w_tail_bwd')
    return dx, dwf, dp


def wn_backward(dwf, v, g, transposed):
    """(dwf [k][C_in][C_out], weight_v, weight_g | None) -> (dv, dg | None)."""
    k, ci, co = dwf.shape
    dv = torch.empty_like(v)
    dg = torch.empty_like(g) if g is not None else None
    _hip.check(_hip.load().v2w_wn_bwd(dwf.data_ptr(), v.data_ptr(), _hip.ptr(g), dv.data_ptr(), _hip.ptr(dg), ci, co, k,
                                      int(transposed), _stream(dwf)), 'v2w_wn_bwd')
    return dv, dg


def cond_backward(dgb, z, sn_w, sn_u, sn_v, sigma, spk, noise):
    """One stage's conditioning backward -> (d weight_orig, d layer.bias, d fcs.weight, d fcs.bias)."""
    B, R = dgb.shape
    dev = dgb.device
    d_w = torch.empty_like(sn_w); d_b = torch.empty((R,), device=dev)
    D = spk.shape[1] + noise.shape[1]
    d_fw = torch.empty((128, D), device=dev); d_fb = torch.empty((128,), device=dev)
    ws = torch.empty((B * 128 + 1,), device=dev)
    _hip.check(_hip.load().v2w_cond_bwd(dgb.data_ptr(), z.data_ptr(), sn_w.data_ptr(), sn_u.data_ptr(), sn_v.data_ptr(),
                                        sigma.data_ptr(), spk.data_ptr(), noise.data_ptr(), d_w.data_ptr(), d_b.data_ptr(),
                                        d_fw.data_ptr(), d_fb.data_ptr(), ws.data_ptr(), B, R // 2, spk.shape[1], noise.shape[1],
                                        _stream(dgb)), 'v2w_cond_bwd')
    return d_w, d_b, d_fw, d_fb


def channel_sum(x):
    """sum over (B, L) per channel of x (B, C, L) -> (C,) fp32: bias gradients (fp64 accumulation inside)."""
    B, Cc, L = x.shape
    stats = torch.empty((2 * Cc + 1,), device=x.device, dtype=torch.float64)
    part = torch.empty((2 * Cc * _hip.V2W_BN_SPLITS,), device=x.device, dtype=torch.float64)
    bn_stats(x, stats, part)
    return stats[:Cc].float()


# ---------------------------------------------------------------------------------------------------------------
# discriminator path (csrc/v2w_disc.hip).  Feature maps are (B, C, pitch) buffers of which [:, :, :L * inner] is valid (L rows of `inner`
# columns: inner = the period of a period discriminator, 1 otherwise); B, the channel counts and every pitch come from the tensors.
def _pitch4(n):
    return (n + 3) // 4 * 4


def _out(out, shape, like, name, pitched=False):
    """`out`, checked, or a new fp32 tensor of `shape` on `like`'s device.  pitched: the caller's `out` chooses its own row pitch (the last
    dimension; the library checks that the valid part fits)."""
    if out is None:
        return torch.empty(shape, device=like.device, dtype=torch.float32)
    _chk(out, name)
    n = len(shape) - 1 if pitched else len(shape)
    if out.dim() != len(shape) or tuple(out.shape[:n]) != tuple(shape[:n]):
        raise ValueError(f'{name}: expected {tuple(shape)}{" (any row pitch)" if pitched else ""}, got {tuple(out.shape)}')
    return out


def phase_split(x, *, L, inner, s, cg=None, out=None):
    """x (B, C, ipitch) -> out (B, s * C, opitch), default opitch = roundup4(ceil(L / s) * inner): the s phases of the L rows stacked along the
    channels, group by group (cg channels per group, default C), zero past L."""
    _chk(x, 'x')
    B, Cc, ip = x.shape
    out = _out(out, (B, s * Cc, _pitch4(-(-L // s) * inner)), x, 'out', pitched=True)
    _hip.check(_hip.load().v2w_phase_split(x.data_ptr(), out.data_ptr(), B, Cc, Cc if cg is None else cg, L, inner, s, ip, out.shape[2], _stream(x)),
               'v2w_phase_split')
    return out


def unfold_taps(x, *, L, inner, s, k, pad, out=None):
    """x (B, C, ipitch) -> out (B, k * C, opitch), default opitch = roundup4(U * inner), U = (L + 2 pad - k) / s + 1: tap j of a k-tap
    stride-s conv as channels j * C .. of a 1-tap conv."""
    _chk(x, 'x')
    B, Cc, ip = x.shape
    out = _out(out, (B, k * Cc, _pitch4(((L + 2 * pad - k) // s + 1) * inner)), x, 'out', pitched=True)
    _hip.check(_hip.load().v2w_unfold_taps(x.data_ptr(), out.data_ptr(), B, Cc, L, inner, s, k, pad, ip, out.shape[2], _stream(x)), 'v2w_unfold_taps')
    return out


def zero_tail(x, *, valid):
    """x (..., pitch), in place: [valid, pitch) of every row becomes 0.  Returns x."""
    _chk(x, 'x')
    pitch = x.shape[-1]
    _hip.check(_hip.load().v2w_zero_tail(x.data_ptr(), x.numel() // pitch, pitch, valid, _stream(x)), 'v2w_zero_tail')
    return x


def unfold1(x, *, H, inner, s, k, pad, rows, out=None):
    """x (B, 1, T) or (B, T), read as H rows of `inner` columns (reflect-padded on the right to H * inner) -> out (B, rows, opitch), default
    opitch = roundup4(U * inner), U = (H + 2 pad - k) / s + 1: row j is tap j of the k-tap stride-s conv, rows k .. are 0."""
    _chk(x, 'x')
    B, T = x.shape[0], x.shape[-1]
    out = _out(out, (B, rows, _pitch4(((H + 2 * pad - k) // s + 1) * inner)), x, 'out', pitched=True)
    _hip.check(_hip.load().v2w_unfold1(x.data_ptr(), out.data_ptr(), B, T, H, inner, s, k, pad, rows, out.shape[2], _stream(x)), 'v2w_unfold1')
    return out


def fold1(dxu, *, T, H, inner, s, k, pad, out=None):
    """Backward of unfold1: dxu (B, rows, ipitch) -> dx (B, 1, T), the reflected tail folded back."""
    _chk(dxu, 'dxu')
    B, rows, ip = dxu.shape
    if out is None:
        out = torch.empty((B, 1, T), device=dxu.device, dtype=torch.float32)
    _chk(out, 'out')
    if out.numel() != B * T:
        raise ValueError(f'out: expected {B} x {T} elements, got {tuple(out.shape)}')
    _hip.check(_hip.load().v2w_fold1(dxu.data_ptr(), out.data_ptr(), B, T, H, inner, s, k, pad, rows, ip, _stream(dxu)), 'v2w_fold1')
    return out


def disc_dz(f, g, d, *, valid, slope, out=None, rowsum=None):
    """dz = (g + d) * lrelu'(f) on [:valid] of every row, 0 behind: f (..., pitch) the activated feature map, g its dense gradient (rows x
    valid) or None, d a pitched gradient like f or None.  rowsum (optional, at least one float per row) receives the sum of each dz row."""
    _chk(f, 'f'); _chk(g, 'g'); _chk(d, 'd'); _chk(rowsum, 'rowsum')
    pitch = f.shape[-1]
    rows = f.numel() // pitch
    out = _out(out, tuple(f.shape), f, 'out')
    if (g is not None and g.numel() != rows * valid) or (d is not None and d.shape != f.shape) or out.shape != f.shape \
            or (rowsum is not None and rowsum.numel() < rows):
        raise ValueError('disc_dz: g must hold rows x valid elements, d and out must be shaped like f, rowsum must hold a float per row')
    _hip.check(_hip.load().v2w_disc_dz(f.data_ptr(), _hip.ptr(g), _hip.ptr(d), out.data_ptr(), _hip.ptr(rowsum), rows, pitch, valid, slope,
                                       _stream(f)), 'v2w_disc_dz')
    return out


def disc_dz_merge(f, g, dxs, *, cg, L, inner, s, slope, out=None, rowsum=None):
    """disc_dz with d given as dxs (B, s * C, dpitch), the phase-stacked input gradient of the stride-s layer above (cg channels per group):
    f (B, C, pitch) (or its B * C rows), valid = L * inner."""
    _chk(f, 'f'); _chk(g, 'g'); _chk(dxs, 'dxs'); _chk(rowsum, 'rowsum')
    B, sC, dp = dxs.shape
    Cc, pitch = sC // s, f.shape[-1]
    out = _out(out, tuple(f.shape), f, 'out')
    if sC % s or f.numel() != B * Cc * pitch or out.shape != f.shape or (g is not None and g.numel() != B * Cc * L * inner) \
            or (rowsum is not None and rowsum.numel() < B * Cc):
        raise ValueError('disc_dz_merge: f and out must hold B x C rows for dxs (B, s * C, dpitch), g their valid parts, rowsum a float per row')
    _hip.check(_hip.load().v2w_disc_dz_merge(f.data_ptr(), _hip.ptr(g), dxs.data_ptr(), out.data_ptr(), _hip.ptr(rowsum), B, Cc, cg, L, inner, s,
                                             dp, pitch, slope, _stream(f)), 'v2w_disc_dz_merge')
    return out


def rowsum_reduce(rowsum, out=None):
    """rowsum (B, C) (the row sums of disc_dz) -> the bias gradient db (C,): the sum over the batch items, fp64, in fixed order."""
    _chk(rowsum, 'rowsum')
    B, Cc = rowsum.shape
    out = _out(out, (Cc,), rowsum, 'out')
    _hip.check(_hip.load().v2w_rowsum_reduce(rowsum.data_ptr(), out.data_ptr(), B, Cc, _stream(rowsum)), 'v2w_rowsum_reduce')
    return out


def cout1_wgrad(x, dz, *, k, dil, tap0, out=None):
    """Weight gradient dwf [k][C][1] of a C_out = 1 conv with taps at (t - tap0) * dil: x (B, C, L), dz (B, 1, L)."""
    _chk(x, 'x'); _chk(dz, 'dz')
    B, Cc, L = x.shape
    if tuple(dz.shape) != (B, 1, L):
        raise ValueError(f'dz: expected {(B, 1, L)}, got {tuple(dz.shape)}')
    out = _out(out, (k, Cc, 1), x, 'out')
    _hip.check(_hip.load().v2w_cout1_wgrad(x.data_ptr(), dz.data_ptr(), out.data_ptr(), B, Cc, L, k, dil, tap0, _stream(x)), 'v2w_cout1_wgrad')
    return out


def wgrad_groups(x, dy, *, groups, k, dil, tap0, out=None, slab=None):
    """Weight gradients dwf [G][k][C_in / G][C_out / G] of every group of a grouped Conv1d (taps at (t - tap0) * dil) in one launch per tap
    group: x (B, C_in, Lq), dy (B, C_out, Lq).  slab: the scratch of the position splits (allocated here when None)."""
    _chk(x, 'x'); _chk(dy, 'dy')
    B, ci, Lq = x.shape
    co = dy.shape[1]
    if dy.shape[0] != B or dy.shape[2] != Lq or ci % groups or co % groups:
        raise ValueError(f'wgrad_groups: x {tuple(x.shape)} and dy {tuple(dy.shape)} do not form {groups} groups of one batch and length')
    ci, co = ci // groups, co // groups
    lib = _hip.load()
    if lib.v2w_wgrad_slabs(B, ci, co, Lq) == 0:
        raise _hip.HipLibraryError(f'v2w_wgrad_groups: no configuration for C_in={ci}, C_out={co}')
    out = _out(out, (groups, k, ci, co), x, 'out')
    n = groups * lib.v2w_wgrad_group_slabs(B, ci, co, Lq, groups) * k * ci * co
    if slab is None:
        slab = torch.empty((n,), device=x.device, dtype=torch.float32)
    _chk(slab, 'slab')
    if slab.numel() < n:
        raise ValueError(f'slab: {n} floats needed, got {slab.numel()}')
    _hip.check(lib.v2w_wgrad_groups(x.data_ptr(), dy.data_ptr(), out.data_ptr(), slab.data_ptr(), B, ci, co, Lq, k, dil, tap0, groups, _stream(x)),
               'v2w_wgrad_groups')
    return out


def avgpool4(x, out=None):
    """AvgPool1d(4, 2, padding=2) along the last axis: x (..., L) -> out (..., L / 2 + 1)."""
    _chk(x, 'x')
    L = x.shape[-1]
    out = _out(out, tuple(x.shape[:-1]) + (L // 2 + 1,), x, 'out')
    _hip.check(_hip.load().v2w_avgpool4(x.data_ptr(), out.data_ptr(), x.numel() // L, L, _stream(x)), 'v2w_avgpool4')
    return out


def avgpool4_bwd(g, *, L, out=None):
    """Backward of avgpool4: g (..., L / 2 + 1) -> dx (..., L)."""
    _chk(g, 'g')
    if g.shape[-1] != L // 2 + 1:
        raise ValueError(f'g: expected rows of {L // 2 + 1}, got {tuple(g.shape)}')
    out = _out(out, tuple(g.shape[:-1]) + (L,), g, 'out')
    _hip.check(_hip.load().v2w_avgpool4_bwd(g.data_ptr(), out.data_ptr(), g.numel() // g.shape[-1], L, _stream(g)), 'v2w_avgpool4_bwd')
    return out


def conv1d_groups(x, w4, bias, out, packs, *, dil, pad_left, out_slope=0.0, algo=ALGO_AUTO):
    """A grouped stride-1 conv as one problem per group on channel slices: x (B, G * C_in, L), w4 [G][k][C_in][C_out], bias (G * C_out,) or
    None, out (B, G * C_out, L); packs[g]: group g's pack_mfma stream (or None) - with algo = ALGO_SPLIT its pack_split pair.  One launch
    when G == 1, otherwise the groups four per launch."""
    G, k, ci, co = w4.shape
    probs = []
    for g in range(G):
        kw = dict(k=k, dil=dil, slope=1.0, pad_left=pad_left, out_slope=out_slope, algo=algo, group=(g, ci, co) if G > 1 else None)
        kw['wps' if algo == ALGO_SPLIT else 'wp'] = packs[g]
        probs.append((x, w4[g], None if bias is None else bias[g * co:(g + 1) * co], out, kw))
    if G == 1:
        conv1d(*probs[0][:4], **probs[0][4])
    else:
        for i in range(0, G, 4):
            conv1d_multi(probs[i:i + 4])
    return out


# ---- spectral norm of the first scale discriminator's conv weights (include/vec2wav_hip.h: v2w_sn_plan / v2w_sn_step / v2w_sn_bwd)
class SnPlan:
    """The planned descriptor table of one layer set - layers: (w (C_out, C_in / groups, k[, 1]), u (C_out,), v (C_in / groups * k,),
    wf [k][C_in / groups][C_out]) - on the device, its grids and its workspace.  `keep_views(keep, i)` -> (sigma, u, v) of layer i in a
    keep slab of a step."""

    def __init__(self, layers):
        n = len(layers)
        if not 1 <= n <= _hip.SN_MAX_LAYERS:
            raise ValueError(f'sn: 1 .. {_hip.SN_MAX_LAYERS} layers per call, got {n}')
        descs = (_hip.SnDesc * n)()
        self.shapes = []
        for d, (w, u, v, wf) in zip(descs, layers):
            _chk(w, 'w'); _chk(u, 'u'); _chk(v, 'v'); _chk(wf, 'wf')
            co, ci, k = w.shape[:3]
            if w.numel() != co * ci * k or u.numel() != co or v.numel() != ci * k or tuple(wf.shape) != (k, ci, co):
                raise ValueError(f'sn: w {tuple(w.shape)}, u {tuple(u.shape)}, v {tuple(v.shape)}, wf {tuple(wf.shape)} do not belong together')
            d.w, d.u, d.v, d.wf = w.data_ptr(), u.data_ptr(), v.data_ptr(), wf.data_ptr()
            d.c_out, d.c_in, d.k = co, ci, k
            self.shapes.append((co, ci, k))
        self.grids = _hip.SnGrids()
        rc = _hip.load().v2w_sn_plan(descs, n, C.byref(self.grids))
        _hip.check(0 if rc > 0 else int(rc or -1), 'v2w_sn_plan')
        dev = layers[0][0].device
        self.n, self.device = n, dev
        self.keep_off = [int(d.keep_off) for d in descs]
        self.keep_floats = self.grids.keep_bytes // 4
        self.descs_dev = torch.frombuffer(bytearray(bytes(descs)), dtype=torch.uint8).to(dev)
        self.ws = torch.empty((self.grids.ws_bytes // 4,), device=dev, dtype=torch.float32)
        self.tensors = [tuple(l) for l in layers]       # what the descriptors point at stays alive with the plan

    def keep_views(self, keep, i):
        co, ci, k = self.shapes[i]
        o = self.keep_off[i]
        ou, ov = o + 4, o + 4 + (co + 3) // 4 * 4
        return keep[o], keep[ou:ou + co], keep[ov:ov + ci * k]


_SN_PLANS = {}


def sn_plan(layers) -> SnPlan:
    """The cached SnPlan of this layer set (keyed by the tensors' addresses and shapes)."""
    if not layers:
        raise ValueError('sn: no layers')
    for l in layers:
        for t, name in zip(l, ('w', 'u', 'v', 'wf')):
            _chk(t, name)
    key = tuple((t.data_ptr(), tuple(t.shape)) for l in layers for t in l) + (str(layers[0][0].device),)
    plan = _SN_PLANS.get(key)
    if plan is None:
        plan = _SN_PLANS[key] = SnPlan(layers)
    return plan


def sn_step(layers, training):
    """One spectral-norm step of every layer (w, u, v, wf) in one v2w_sn_step: with `training` v <- norm(W^T u), u <- norm(W v) in place;
    sigma = u . W v; wf = W / sigma in the fold layout.  -> (plan, keep): keep is this call's slab of (sigma, u, v) per layer
    (`plan.keep_views(keep, i)`), which `sn_backward` reads."""
    plan = sn_plan(layers)
    keep = torch.empty((plan.keep_floats,), device=plan.device, dtype=torch.float32)
    _hip.check(_hip.load().v2w_sn_step(plan.descs_dev.data_ptr(), plan.n, int(bool(training)), C.byref(plan.grids), keep.data_ptr(),
                                       plan.ws.data_ptr(), plan.grids.ws_bytes, _stream(keep)), 'v2w_sn_step')
    return plan, keep


def sn_backward(plan: SnPlan, keep, dwfs, outs=None):
    """dwfs[i]: the gradient wrt layer i's folded weight [k][C_in / groups][C_out], or None -> dw[i] shaped (C_out, C_in / groups, k)
    (None where dwfs[i] is): dwf / sigma - (sum(dwf . w) / sigma^2) u v^T, one v2w_sn_bwd for all of them."""
    if len(dwfs) != plan.n:
        raise ValueError(f'sn_backward: {plan.n} layers planned, {len(dwfs)} gradients given')
    _chk(keep, 'keep')
    pd, po = (_hip._fp * plan.n)(), (_hip._fp * plan.n)()
    dws = [None] * plan.n
    for i, g in enumerate(dwfs):
        if g is None:
            continue
        co, ci, k = plan.shapes[i]
        _chk(g, 'dwf')
        if tuple(g.shape) != (k, ci, co):
            raise ValueError(f'sn_backward: dwf[{i}] must be {(k, ci, co)}, got {tuple(g.shape)}')
        dws[i] = _out(None if outs is None else outs[i], (co, ci, k), g, 'dw')
        pd[i], po[i] = g.data_ptr(), dws[i].data_ptr()
    _hip.check(_hip.load().v2w_sn_bwd(plan.descs_dev.data_ptr(), plan.n, C.byref(plan.grids), keep.data_ptr(), pd, po,
                                      plan.ws.data_ptr(), plan.grids.ws_bytes, _stream(keep)), 'v2w_sn_bwd')
    return dws


# ---- GAN training losses (include/vec2wav_hip.h: v2w_l1_mean_multi / v2w_lsgan_multi and their backwards)
def _dense_suffix(dims):
    """How many trailing (size, stride) pairs form one contiguous run of floats."""
    n, run = 0, 1
    for size, stride in reversed(dims):
        if stride != run:
            break
        run *= size
        n += 1
    return n


def _dims(t):
    return [(s, st) for s, st in zip(t.shape, t.stride()) if s != 1]


def _rows_at(t, dims, k, aligned):
    """(rows, valid, pitch) of `t` with its last k (non-unit) dims as one row, or None when the leading dims do not sit one pitch apart
    (or, with `aligned`, pitched rows do not begin on 16-byte lines)."""
    if k == len(dims):                                    # dense: one run; cut at the last dim only when it would not fit an int32
        numel = t.numel()
        if numel < 2 ** 31:
            return 1, numel, numel
        last = dims[-1][0]
        return numel // last, last, last
    if k == 0:
        return None
    valid = 1
    for size, _ in dims[-k:]:
        valid *= size
    rows, pitch = 1, dims[-k - 1][1]
    for i in range(len(dims) - k - 1, -1, -1):
        if dims[i][1] != pitch * rows:
            return None
        rows *= dims[i][0]
    if pitch < valid or valid >= 2 ** 31 or pitch >= 2 ** 31:
        return None
    if aligned and pitch != valid and (pitch % 4 or t.data_ptr() % 16):
        return None
    return rows, valid, pitch


def loss_rows(t, like=None, aligned=True):
    """The (rows, valid, pitch) descriptor of a tensor for the loss kernels - `rows` rows of `valid` contiguous floats, `pitch` floats
    apart - straight from its strides, or None when it has no such form and must be made contiguous.  Dense tensors, last-dim slices
    of pitched (B, C, P) buffers, their 4-D (b, C, U, inner) views and leading-dim slices of all of these qualify.  `like`: the other
    tensor of an L1 pair (same shape): both are cut into the same rows.  `aligned`: pitched rows must start on 16-byte lines and
    pitch % 4 == 0 (the L1 kernels' 16-byte loads; the LSGAN kernels read float by float)."""
    if t.numel() == 0:
        raise ValueError('loss of an empty tensor')
    dims = _dims(t)
    k = _dense_suffix(dims)
    if like is not None:
        if like.shape != t.shape:
            raise ValueError(f'shapes differ: {tuple(t.shape)} and {tuple(like.shape)}')
        k = min(k, _dense_suffix(_dims(like)))
    return _rows_at(t, dims, k, aligned)


def loss_rows_len(t, B, aligned=True):
    """`loss_rows` for a map or score of a padded batch of B items - (B, C, U), (B, C, U, inner) or (B, N): the rows are the (b, c) rows
    (the b rows of a score), never a longer run, so that every row lies in one item; None when the tensor has no such form."""
    if t.dim() < 2 or t.shape[0] != B:
        raise ValueError(f'a map or score of a batch of {B} items is (B, C, ...) or (B, N), got {tuple(t.shape)}')
    if t.numel() == 0:
        raise ValueError('loss of an empty tensor')
    lead = 2 if t.dim() >= 3 else 1
    valid = 1
    for size, stride in reversed(list(zip(t.shape[lead:], t.stride()[lead:]))):
        if size != 1 and stride != valid:
            return None
        valid *= size
    rows = 1
    pitch = None
    for size, stride in reversed(list(zip(t.shape[:lead], t.stride()[:lead]))):
        if size != 1:
            if pitch is None:
                pitch = stride
            if stride != pitch * rows:
                return None
        rows *= size
    pitch = valid if pitch is None else pitch
    if pitch < valid or valid >= 2 ** 31 or pitch >= 2 ** 31:
        return None
    if aligned and pitch != valid and (pitch % 4 or t.data_ptr() % 16):
        return None
    return rows, valid, pitch


def _ext_check(ext, n, dev):
    """The extent table of n descriptors (`discriminators.MapLengths` rows): int32 (n, B), contiguous, on the tensors' device -> B."""
    if not torch.is_tensor(ext) or ext.dtype != torch.int32 or ext.dim() != 2 or ext.shape[0] != n or not ext.is_contiguous():
        raise ValueError(f'ext must be a contiguous int32 tensor of {n} rows, one per descriptor')
    if ext.device != dev:
        raise RuntimeError('the extent table must live on the device of the maps')
    return int(ext.shape[1])


def _loss_check(t, name):
    if not t.is_cuda:
        raise RuntimeError(f'{name} must live on a GPU: the HIP loss kernels have no CPU fallback')
    if t.dtype != torch.float32:
        raise TypeError(f'{name} must be torch.float32, got {t.dtype}')


def _l1_pair_array(pairs, B=None):
    """ctypes descriptors of the pairs and the tensors they point into (contiguous copies where a view has no row form).  B: the pairs are
    maps of a padded batch of B items, cut into their (b, c) rows (loss_rows_len)."""
    n = len(pairs)
    arr = (_hip.L1Pair * max(n, 1))()
    keep = []
    for i, (a, b) in enumerate(pairs):
        _loss_check(a, 'a'); _loss_check(b, 'b')
        if a.device != pairs[0][0].device or b.device != a.device:
            raise RuntimeError('all tensors of one loss call must live on one device')
        a, b = a.detach(), b.detach()
        for _ in range(3):
            if B is not None and a.shape != b.shape:
                raise ValueError(f'shapes differ: {tuple(a.shape)} and {tuple(b.shape)}')
            fa, fb = (loss_rows(a, b), loss_rows(b, a)) if B is None else (loss_rows_len(a, B), loss_rows_len(b, B))
            if fa is not None and fb is not None:
                break
            if fa is None:
                a = a.contiguous()
            if fb is None:
                b = b.contiguous()
        assert fa[:2] == fb[:2], (fa, fb)
        keep += [a, b]
        d = arr[i]
        d.a, d.b, d.rows, d.valid, d.pitch_a, d.pitch_b = a.data_ptr(), b.data_ptr(), fa[0], fa[1], fa[2], fb[2]
    return arr, keep


def _multi_plan(entry, arr, n):
    """(starts, workgroups) of the host-only plan query `entry` for n descriptors."""
    starts = (C.c_int32 * (n + 1))()
    nwg = getattr(_hip.load(), entry)(arr, n, starts)
    if nwg <= 0:
        _hip.check(nwg or -1, entry)
    return list(starts), nwg


def l1_plan(arr, n):
    """(starts, workgroups) of v2w_l1_multi_plan for n descriptors."""
    return _multi_plan('v2w_l1_multi_plan', arr, n)


def l1_mean_multi(pairs, scale=1.0, ext=None):
    """pairs: [(a, b), ...] of equal-shaped fp32 GPU tensors (at most 64) -> (terms (n,), total ()): terms[i] = mean |a_i - b_i|,
    total = scale * sum(terms); one streaming and one finishing launch, deterministic.  The views the discriminators return are read
    in place (loss_rows).
    ext: int32 GPU tensor (n, B) - the pairs are maps (B, C, ...) of a padded batch and row (b, c) of pair i counts its first ext[i, b]
    floats (v2w_l1_mean_multi_len: the mean is over the counted floats, 0 when there are none; the others are selected away)."""
    n = len(pairs)
    if n == 0:
        raise ValueError('no pairs')
    B = None if ext is None else _ext_check(ext, n, pairs[0][0].device)
    arr, keep = _l1_pair_array(pairs, B)
    dev = keep[0].device
    with torch.cuda.device(dev):
        lib = _hip.load()
        nbytes = lib.v2w_l1_multi_scratch_bytes(arr, n)
        if nbytes <= 0:
            _hip.check(int(nbytes) or -1, 'v2w_l1_multi_scratch_bytes')
        scratch = torch.empty((nbytes // 8,), device=dev, dtype=torch.float64)
        terms = torch.empty((n,), device=dev, dtype=torch.float32)
        total = torch.empty((), device=dev, dtype=torch.float32)
        if ext is None:
            _hip.check(lib.v2w_l1_mean_multi(arr, n, float(scale), terms.data_ptr(), total.data_ptr(), scratch.data_ptr(), _stream(keep[0])),
                       'v2w_l1_mean_multi')
        else:
            _hip.check(lib.v2w_l1_mean_multi_len(arr, n, ext.data_ptr(), B, float(scale), terms.data_ptr(), total.data_ptr(),
                                                 scratch.data_ptr(), _stream(keep[0])), 'v2w_l1_mean_multi_len')
    return terms, total


def l1_mean_multi_bwd(pairs, scale, gout, need_a=None, need_b=None, ext=None):
    """Gradients of `gout * l1_mean_multi(pairs, scale, ext)[1]`: ([da_i | None], [db_i | None]), dense, shaped like the inputs; one launch.
    gout: a one-element fp32 GPU tensor, read by the kernel.  need_a / need_b: per pair, which sides to write (default: all).
    ext: as in l1_mean_multi; every float that is not counted gets +0.0."""
    n = len(pairs)
    need_a = [True] * n if need_a is None else list(need_a)
    need_b = [True] * n if need_b is None else list(need_b)
    B = None if ext is None else _ext_check(ext, n, pairs[0][0].device)
    arr, keep = _l1_pair_array(pairs, B)
    dev = keep[0].device
    _loss_check(gout, 'gout')
    if gout.numel() != 1:
        raise ValueError('gout must hold one element')
    da = [torch.empty(a.shape, device=dev, dtype=torch.float32) if w else None for (a, _), w in zip(pairs, need_a)]
    db = [torch.empty(b.shape, device=dev, dtype=torch.float32) if w else None for (_, b), w in zip(pairs, need_b)]
    for i in range(n):
        arr[i].da, arr[i].db = _hip.ptr(da[i]), _hip.ptr(db[i])
    if any(need_a) or any(need_b):
        with torch.cuda.device(dev):
            if ext is None:
                _hip.check(_hip.load().v2w_l1_mean_multi_bwd(arr, n, float(scale), gout.data_ptr(), _stream(keep[0])), 'v2w_l1_mean_multi_bwd')
            else:
                _hip.check(_hip.load().v2w_l1_mean_multi_len_bwd(arr, n, ext.data_ptr(), B, float(scale), gout.data_ptr(), _stream(keep[0])),
                           'v2w_l1_mean_multi_len_bwd')
    return da, db


def _lsgan_array(scores, targets, B=None):
    n = len(scores)
    if len(targets) != n:
        raise ValueError('one target per score tensor')
    arr = (_hip.LsganItem * max(n, 1))()
    keep = []
    for i, (s, t) in enumerate(zip(scores, targets)):
        _loss_check(s, 'score')
        if s.device != scores[0].device:
            raise RuntimeError('all tensors of one loss call must live on one device')
        s = s.detach()
        rows_of = (lambda t: loss_rows(t, aligned=False)) if B is None else (lambda t: loss_rows_len(t, B, aligned=False))
        form = rows_of(s)
        if form is None:
            s = s.contiguous()
            form = rows_of(s)
        keep.append(s)
        d = arr[i]
        d.s, d.rows, d.valid, d.pitch, d.target = s.data_ptr(), form[0], form[1], form[2], float(t)
    return arr, keep


def lsgan_multi(scores, targets, ext=None):
    """scores: fp32 GPU tensors (at most 64), targets: 0 / 1 each -> (terms (n,), total ()): terms[i] = mean (target_i - s_i)^2,
    total = sum(terms); one launch.  ext: int32 GPU tensor (n, B) - the scores are (B, N) (or (B, C, ...)) of a padded batch, each row
    counts its first ext[i, b] floats (v2w_lsgan_multi_len)."""
    n = len(scores)
    if n == 0:
        raise ValueError('no scores')
    B = None if ext is None else _ext_check(ext, n, scores[0].device)
    arr, keep = _lsgan_array(scores, targets, B)
    dev = keep[0].device
    terms = torch.empty((n,), device=dev, dtype=torch.float32)
    total = torch.empty((), device=dev, dtype=torch.float32)
    with torch.cuda.device(dev):
        if ext is None:
            _hip.check(_hip.load().v2w_lsgan_multi(arr, n, terms.data_ptr(), total.data_ptr(), _stream(keep[0])), 'v2w_lsgan_multi')
        else:
            _hip.check(_hip.load().v2w_lsgan_multi_len(arr, n, ext.data_ptr(), B, terms.data_ptr(), total.data_ptr(), _stream(keep[0])),
                       'v2w_lsgan_multi_len')
    return terms, total


def lsgan_multi_bwd(scores, targets, gout=None, gterms=None, need=None, ext=None):
    """Gradients of lsgan_multi: ds_i = 2 (s_i - target_i) * (gout + gterms[i]) / numel_i, dense, shaped like the scores; one launch.
    gout (one element) / gterms (n): fp32 GPU tensors, read by the kernel; one of them may be None.  ext: as in lsgan_multi (numel_i is the
    count of the counted floats; the others get +0.0)."""
    n = len(scores)
    need = [True] * n if need is None else list(need)
    B = None if ext is None else _ext_check(ext, n, scores[0].device)
    arr, keep = _lsgan_array(scores, targets, B)
    dev = keep[0].device
    for g, name, cnt in ((gout, 'gout', 1), (gterms, 'gterms', n)):
        if g is not None:
            _loss_check(g, name)
            if g.numel() != cnt or not g.is_contiguous():
                raise ValueError(f'{name} must hold {cnt} contiguous element(s)')
    ds = [torch.empty(s.shape, device=dev, dtype=torch.float32) if w else None for s, w in zip(scores, need)]
    for i in range(n):
        arr[i].ds = _hip.ptr(ds[i])
    if any(need):
        with torch.cuda.device(dev):
            if ext is None:
                _hip.check(_hip.load().v2w_lsgan_multi_bwd(arr, n, _hip.ptr(gout), _hip.ptr(gterms), _stream(keep[0])), 'v2w_lsgan_multi_bwd')
            else:
                _hip.check(_hip.load().v2w_lsgan_multi_len_bwd(arr, n, ext.data_ptr(), B, _hip.ptr(gout), _hip.ptr(gterms), _stream(keep[0])),
                           'v2w_lsgan_multi_len_bwd')
    return ds


def map_extents(lens, len_mul, L, chains, layers):
    """lens: int32 GPU tensor (B,); chains (n, 4) {period, pools, depth, size} and layers (n_layers, 3) {k, stride, pad}: int32 GPU tensors
    -> ext (n, B) int32, the floats per row that exist for each item (include/vec2wav_hip.h v2w_map_extents); one launch, no sync."""
    for t, name in ((lens, 'lens'), (chains, 'chains'), (layers, 'layers')):
        if not t.is_cuda or t.dtype != torch.int32 or not t.is_contiguous():
            raise ValueError(f'{name} must be a contiguous int32 GPU tensor')
    n, B = chains.shape[0], lens.numel()
    ext = torch.empty((n, B), dtype=torch.int32, device=lens.device)
    with torch.cuda.device(lens.device):
        _hip.check(_hip.load().v2w_map_extents(lens.data_ptr(), int(len_mul), int(L), B, chains.data_ptr(), n, layers.data_ptr(),
                                               layers.shape[0], ext.data_ptr(), _stream(lens)), 'v2w_map_extents')
    return ext


def mask_tail(x, lens, len_mul=1):
    """x (B, ..., L) fp32 contiguous GPU tensor, lens int32 GPU (B,) -> x with x[b, ..., m_b:] = +0.0 by select, m_b = min(lens[b] * len_mul,
    L) (v2w_mask_tail); one launch."""
    _loss_check(x, 'x')
    if x.dim() < 2 or not x.is_contiguous() or x.numel() == 0:
        raise ValueError('mask_tail: x must be a non-empty contiguous (B, ..., L) tensor')
    B, L = x.shape[0], x.shape[-1]
    if lens.dtype != torch.int32 or lens.numel() != B or lens.device != x.device:
        raise ValueError(f'lens must hold {B} int32 on the device of x')
    out = torch.empty_like(x)
    with torch.cuda.device(x.device):
        _hip.check(_hip.load().v2w_mask_tail(x.data_ptr(), out.data_ptr(), x.numel() // L, B, L, lens.data_ptr(), int(len_mul), _stream(x)),
                   'v2w_mask_tail')
    return out


# ---- multi-tensor launches over flat tensors (csrc/v2w_multi.h): AdamW, the global-norm clip, the average of the weights
def adamw_plan(arr, n):
    """(starts, workgroups) of v2w_adamw_multi_plan for n descriptors."""
    return _multi_plan('v2w_adamw_multi_plan', arr, n)


def adamw_hyper(*, lr, betas, eps, weight_decay, step):
    """The v2w_adamw_hyper of step number `step` (>= 1): the bias corrections are computed in double and rounded once to fp32."""
    step = int(step)
    if step < 1:
        raise ValueError(f'step must be >= 1, got {step}')
    b1, b2 = float(betas[0]), float(betas[1])
    return _hip.AdamWHyper(float(lr), b1, b2, float(eps), float(weight_decay), 1.0 - b1 ** step, (1.0 - b2 ** step) ** 0.5, 0)


_FIELD = {'param': 'p', 'grad': 'g', 'exp_avg': 'm', 'exp_avg_sq': 'v', 'ema': 'e'}


def _flat_items(item, what, lists, copied=None, in_place=()):
    """(descriptors of ctypes type `item`, the tensors they point into) of `lists` = {name: tensors}, entry for entry one tensor of each
    name: fp32 contiguous GPU tensors on one device, of the numel (> 0) of the first list's.  A non-contiguous tensor of the list `copied`
    is copied for reading, unless that list is also among the ones written `in_place`: then it is refused."""
    names = list(lists)
    dev = lists[names[0]][0].device
    items = list(zip(*lists.values()))
    arr = (item * max(len(items), 1))()
    keep = []
    for i, (d, ts) in enumerate(zip(arr, items)):
        numel = ts[0].numel()
        for name, t in zip(names, ts):
            t = t.detach()
            if name == copied and t.is_cuda and t.dtype == torch.float32 and not t.is_contiguous():
                if name in in_place:
                    raise ValueError(f'{name}[{i}] is not contiguous: it cannot be scaled in place')
                t = t.contiguous()
            _chk(t, f'{name}[{i}]')
            if t.device != dev:
                raise RuntimeError(f'all tensors of one {what} call must live on one device')
            if t.numel() != numel:
                raise ValueError(f'{name}[{i}] has {t.numel()} elements, its parameter {numel}')
            keep.append(t)
            setattr(d, _FIELD[name], t.data_ptr())
        if numel == 0:
            raise ValueError(f'{names[0]}[{i}] is empty')
        d.numel = numel
    return arr, keep


def _chunks_of(arr, n, item, limit):
    """(pointer to the first descriptor, count) of every run of at most `limit` descriptors of type `item`."""
    for i0 in range(0, n, limit):
        yield C.cast(C.byref(arr, i0 * C.sizeof(item)), C.POINTER(item)), min(limit, n - i0)


def _launch_chunks(entry, arr, n, item, limit, on, extra=()):
    """lib.`entry`(descriptors, count, *extra, stream) for every run of at most `limit` of the n descriptors, on the device and the current
    stream of the tensor `on`; `extra`: the arguments in between, or a function (descriptors, count) -> them.  Returns the launches."""
    launches = 0
    with torch.cuda.device(on.device):
        fn = getattr(_hip.load(), entry)
        stream = _stream(on)
        for chunk, k in _chunks_of(arr, n, item, limit):
            _hip.check(fn(chunk, k, *(extra(chunk, k) if callable(extra) else extra), stream), entry)
            launches += 1
    return launches


def _adamw_step(entry, params, grads, exp_avgs, exp_avg_sqs, emas=None, clip=None, *, ema_decay=None, skip_nonfinite=False, **hyper):
    """The three steps' common course; `entry`: v2w_adamw_multi, v2w_adamw_multi_clipped (clip required) or v2w_adamw_ema_multi (emas
    required, clip optional, an empty list refused)."""
    lists = {'param': params, 'grad': grads, 'exp_avg': exp_avgs, 'exp_avg_sq': exp_avg_sqs}
    if emas is not None:
        lists['ema'] = emas
    n = len(params)
    if any(len(ts) != n for ts in lists.values()):
        plural = [name + 's' for name in lists]
        raise ValueError(f'{", ".join(plural[:-1])} and {plural[-1]} must have one entry per tensor')
    if emas is not None and n == 0:
        raise ValueError('adamw_ema_multi: no tensors')
    omd = None if emas is None else ema_omd(ema_decay)
    if clip is not None or entry == 'v2w_adamw_multi_clipped':
        _clip_buffer(clip, 'clip', 4)
    if n == 0:
        return 0
    hyper = adamw_hyper(**hyper)
    item, limit = (_hip.AdamWItem, _hip.ADAMW_MAX_ITEMS) if emas is None else (_hip.AdamWEmaItem, _hip.ADAMW_EMA_MAX_ITEMS)
    arr, keep = _flat_items(item, entry[4:], lists, copied='grad')
    if clip is not None and clip.device != keep[0].device:
        raise RuntimeError('clip must live on the parameters\' device')
    extra = (C.byref(hyper),)
    if emas is not None:
        extra += (_hip.ptr(clip), int(bool(skip_nonfinite)), omd)
    elif clip is not None:
        extra += (clip.data_ptr(), int(bool(skip_nonfinite)))
    return _launch_chunks(entry, arr, n, item, limit, keep[0], extra)


def adamw_multi(params, grads, exp_avgs, exp_avg_sqs, *, lr, betas, eps, weight_decay, step):
    """One AdamW step (decoupled weight decay, no amsgrad) of every tensor of the lists, in place on params / exp_avgs / exp_avg_sqs:
    ceil(n / ADAMW_MAX_ITEMS) launches on the current stream.  `step` is the number of THIS step (1 for the first).  fp32 GPU tensors on
    one device; params and moments must be contiguous (they are written in place), a non-contiguous gradient is copied.  Returns the
    number of launches.  The parameters' version counters are NOT bumped (the kernels write through raw pointers): optim.AdamW does."""
    return _adamw_step('v2w_adamw_multi', params, grads, exp_avgs, exp_avg_sqs,
                       lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, step=step)


# ---- global-norm clipping and the non-finite guard (include/vec2wav_hip.h: v2w_grad_sumsq_multi and its neighbours)
def _clip_buffer(t, name, floats):
    _chk(t, name)
    if t.numel() < floats:
        raise ValueError(f'{name} must hold {floats} floats, got {t.numel()}')


def _grad_array(grads, in_place=False):
    """(descriptors with g and numel set, the tensors they point into).  A non-contiguous gradient is copied for reading; one that is to be
    written in place is refused."""
    return _flat_items(_hip.AdamWItem, 'gradient', {'grad': grads}, copied='grad', in_place=('grad',) if in_place else ())


def _sumsq_partials(arr, n):
    lib = _hip.load()
    total = 0
    for chunk, k in _chunks_of(arr, n, _hip.AdamWItem, _hip.ADAMW_MAX_ITEMS):
        w = lib.v2w_grad_sumsq_partials(chunk, k)
        if w <= 0:
            _hip.check(w or -1, 'v2w_grad_sumsq_partials')
        total += w
    return total


def grad_sumsq_partials(grads):
    """The floats grad_sumsq_multi writes for these gradients: the workgroups of its launches (host only)."""
    if len(grads) == 0:
        return 0
    arr, _keep = _grad_array(grads)
    return _sumsq_partials(arr, len(grads))


def grad_sumsq_multi(grads, partials=None):
    """Per-workgroup sums of squares of every gradient of the list: ceil(n / ADAMW_MAX_ITEMS) launches into consecutive ranges of
    `partials` (fp32, GPU; allocated when None, otherwise it must hold grad_sumsq_partials(grads) floats - the rest of it is left
    alone).  Returns (partials, count); deterministic, no atomics."""
    n = len(grads)
    if n == 0:
        raise ValueError('no gradients')
    arr, keep = _grad_array(grads)
    dev = keep[0].device
    count = _sumsq_partials(arr, n)
    if partials is None:
        partials = torch.empty((count,), device=dev, dtype=torch.float32)
    _clip_buffer(partials, 'partials', count)
    if partials.device != dev:
        raise RuntimeError('partials must live on the gradients\' device')
    at = [0]

    def its_range(chunk, k):                              # every launch writes behind the one before
        first = partials.data_ptr() + 4 * at[0]
        at[0] += _hip.load().v2w_grad_sumsq_partials(chunk, k)
        return (first,)
    _launch_chunks('v2w_grad_sumsq_multi', arr, n, _hip.AdamWItem, _hip.ADAMW_MAX_ITEMS, keep[0], its_range)
    return partials, count


def grad_norm_finish(partials, count, max_norm, out=None):
    """out[0] = the L2 norm the first `count` partials add up to, out[1] = min(1, max_norm / (norm + 1e-6)), out[2] = 1.0 when the norm
    is finite else 0.0, out[3] += 1 - out[2]; one launch of one workgroup, nothing is read back.  `out`: 4 fp32 on the GPU (zeros when
    None).  max_norm = inf gives the norm alone (coefficient 1)."""
    count = int(count)
    _clip_buffer(partials, 'partials', max(count, 1))
    with torch.cuda.device(partials.device):
        if out is None:
            out = torch.zeros((4,), device=partials.device, dtype=torch.float32)
        _clip_buffer(out, 'out', 4)
        _hip.check(_hip.load().v2w_grad_norm_finish(partials.data_ptr(), count, float(max_norm), out.data_ptr(), _stream(partials)),
                   'v2w_grad_norm_finish')
    return out


def scale_multi(grads, coef):
    """g *= coef[0] in place for every gradient of the list, the coefficient read from GPU memory by the kernel (`coef`: fp32, at least
    one element - e.g. grad_norm_finish(...)[1:]); ceil(n / ADAMW_MAX_ITEMS) launches.  A coefficient of exactly 1.0 changes no bit."""
    n = len(grads)
    if n == 0:
        return 0
    arr, keep = _grad_array(grads, in_place=True)
    _clip_buffer(coef, 'coef', 1)
    return _launch_chunks('v2w_scale_multi', arr, n, _hip.AdamWItem, _hip.ADAMW_MAX_ITEMS, keep[0], (coef.data_ptr(),))


def adamw_multi_clipped(params, grads, exp_avgs, exp_avg_sqs, clip, *, skip_nonfinite=False, lr, betas, eps, weight_decay, step):
    """adamw_multi on g * clip[1], `clip` the four floats of grad_norm_finish on the GPU, read by the kernel: the gradients are not
    written, the host reads nothing.  With skip_nonfinite and clip[2] == 0 (a non-finite norm) the launches write nothing."""
    return _adamw_step('v2w_adamw_multi_clipped', params, grads, exp_avgs, exp_avg_sqs, None, clip, skip_nonfinite=skip_nonfinite,
                       lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, step=step)


# ---- exponential moving average of the weights (include/vec2wav_hip.h: v2w_adamw_ema_multi, v2w_ema_multi, v2w_swap_multi)
def ema_omd(ema_decay):
    """1 - decay for a decay in [0, 1] (ValueError otherwise, NaN included): computed in double here, rounded once to fp32 on the way in."""
    d = float(ema_decay)
    if not 0.0 <= d <= 1.0:
        raise ValueError(f'ema_decay must lie in [0, 1], got {ema_decay}')
    return 1.0 - d


def _pair_array(ps, es, what):
    """(EmaItem descriptors, the tensors they point into) of two lists of fp32 GPU tensors on one device, entry for entry of one size."""
    if len(ps) != len(es):
        raise ValueError(f'{what}: params and emas must have one entry per tensor')
    if len(ps) == 0:
        raise ValueError(f'{what}: no tensors')
    return _flat_items(_hip.EmaItem, what, {'param': ps, 'ema': es})


def adamw_ema_multi(params, grads, exp_avgs, exp_avg_sqs, emas, clip=None, *, ema_decay, skip_nonfinite=False, lr, betas, eps, weight_decay,
                    step):
    """adamw_multi (clip None) or adamw_multi_clipped (`clip`: the four floats of grad_norm_finish on the GPU) with the exponential moving
    average of every parameter updated in the same pass: emas[i] <- emas[i] + (1 - ema_decay) (params[i]' - emas[i]), in place;
    params / exp_avgs / exp_avg_sqs get the bits the other two wrappers give.  ceil(n / ADAMW_EMA_MAX_ITEMS) launches; returns their
    number.  With skip_nonfinite and clip[2] == 0 nothing is written, the averages included."""
    return _adamw_step('v2w_adamw_ema_multi', params, grads, exp_avgs, exp_avg_sqs, emas, clip, ema_decay=ema_decay,
                       skip_nonfinite=skip_nonfinite, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, step=step)


def ema_multi(params, emas, *, ema_decay):
    """emas[i] <- emas[i] + (1 - ema_decay) (params[i] - emas[i]) in place, params only read: for tensors something else steps, and for
    buffers.  fp32 contiguous GPU tensors on one device; ceil(n / ADAMW_MAX_ITEMS) launches, returns their number."""
    omd = ema_omd(ema_decay)
    arr, keep = _pair_array(params, emas, 'ema_multi')
    return _launch_chunks('v2w_ema_multi', arr, len(params), _hip.EmaItem, _hip.ADAMW_MAX_ITEMS, keep[0], (omd,))


def swap_multi(params, emas):
    """Exchanges the contents of params[i] and emas[i] in place, bit for bit; no storage pointer moves.  ceil(n / ADAMW_MAX_ITEMS)
    launches, returns their number.  The parameters' version counters are NOT bumped: optim.AdamW.swap_ema does."""
    arr, keep = _pair_array(params, emas, 'swap_multi')
    return _launch_chunks('v2w_swap_multi', arr, len(params), _hip.EmaItem, _hip.ADAMW_MAX_ITEMS, keep[0])
