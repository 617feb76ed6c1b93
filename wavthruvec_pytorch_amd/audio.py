"""Sample-rate conversion and peak normalisation on the MI355X: the two ends of the audio path.

The reference reads every training target through `librosa.load(path, sr=16000)` and `normalize(audio) * 0.95` on a host core
(vec2wav/dataset.py:16-20,133), and its generator is a 16 kHz model whose output playback pipelines want at 44.1 or 48 kHz.  Both are one
band-limited rational-ratio resampler: `resample` is the polyphase form of torchaudio.functional.resample's Hann-windowed sinc
(lowpass_filter_width 6, rolloff 0.99), restated here (torchaudio is not a dependency), in one launch of v2w_resample on the caller's batch
with per-item lengths; `peak=0.95` adds librosa.util.normalize(...) * 0.95 per item (v2w_peak_scale).  The filter:

    g = gcd(orig, new);  M = orig / g (input step);  L = new / g (phases);  base = min(M, L) * rolloff
    t(p, k) = (k / M - p / L) * base
    h[p][k] = sinc(pi t) * cos(pi t / (2 lpw))^2 * base / M   where |t| < lpw, else exactly 0
    y[q L + p] = sum_k h[p][k] x[q M + k],  x = 0 outside [0, n);   N = ceil(L n / M) outputs for n inputs

Per phase the non-zero taps are one run k0[p] .. k0[p] + NT - 1: 34 multiply-adds per output at 441 : 160, where the strided-conv form of the
same filter spends 475.  Row sums of h (the gain at DC) lie between 1.00003 and 1.0009, as torchaudio's do; nothing is renormalised.
Forward only; there is no CPU path.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, Tuple

import numpy as np
import torch

from . import _hip, hipops, mel

_CONSTS: Dict[Tuple, dict] = {}


def _ratio(orig_freq, new_freq):
    orig, new = int(orig_freq), int(new_freq)
    if orig != orig_freq or new != new_freq or orig < 1 or new < 1:
        raise ValueError(f'resample: orig_freq and new_freq must be positive integers, got {orig_freq!r} and {new_freq!r}')
    g = math.gcd(orig, new)
    return orig // g, new // g


def resample_table(orig_freq, new_freq, lowpass_filter_width=6, rolloff=0.99):
    """-> dict(M, L, NT, k0 (L,) int64, h (L, NT) float64): the polyphase filter of the module docstring, on the host in fp64.  k0[p] and the
    run's length come from the |t| < lpw mask itself, evaluated with the integer numerator k L - p M (no rounding before the product with
    base / (M L)), not from the closed forms k0[p] = floor(M p / L - lpw M / base) + 1 and NT = ceil(2 lpw M / base); NT is the longest run,
    a shorter one is padded with zeros at its end."""
    M, L = _ratio(orig_freq, new_freq)
    lpw = int(lowpass_filter_width)
    if lpw < 1 or lpw != lowpass_filter_width:
        raise ValueError('resample: lowpass_filter_width must be a positive integer')
    if not 0.0 < float(rolloff) <= 1.0:
        raise ValueError('resample: rolloff must lie in (0, 1]')
    base = min(M, L) * float(rolloff)
    reach = int(math.ceil(lpw * M / base)) + 2                     # |k - M p / L| of every tap is below lpw M / base
    centre = (M * np.arange(L, dtype=np.int64)) // L
    k = centre[:, None] + np.arange(-reach, reach + 1, dtype=np.int64)[None, :]
    num = k * L - M * np.arange(L, dtype=np.int64)[:, None]         # t = num * base / (M L)
    t = num.astype(np.float64) * (base / (M * L))
    inside = np.abs(t) < lpw
    pt = np.pi * t
    sinc = np.where(num == 0, 1.0, np.sin(pt) / np.where(num == 0, 1.0, pt))
    full = np.where(inside, sinc * np.cos(pt / (2 * lpw)) ** 2 * (base / M), 0.0)
    first = inside.argmax(axis=1)
    count = inside.sum(axis=1)
    assert (count >= 1).all() and all(inside[p, first[p]:first[p] + count[p]].all() for p in range(L))      # one run per phase
    NT = int(count.max())
    full = np.concatenate([full, np.zeros((L, NT))], axis=1)
    h = np.stack([full[p, first[p]:first[p] + NT] for p in range(L)])
    k0 = k[np.arange(L), first]
    return dict(M=M, L=L, NT=NT, k0=k0.astype(np.int64), h=np.ascontiguousarray(h))


def resampled_length(n, orig_freq, new_freq):
    """Samples `resample` gives n input samples: ceil(L n / M)."""
    M, L = _ratio(orig_freq, new_freq)
    return -(-int(n) * L // M)


def _constants(orig, new, lpw, rolloff, device):
    """The table on the device, cached per (orig, new, lpw, rolloff, device).  orig == new: the one-tap identity (M = L = NT = 1, h = 1)."""
    key = (orig, new, lpw, rolloff, str(device))
    c = _CONSTS.get(key)
    if c is None:
        if orig == new:
            t = dict(M=1, L=1, NT=1, k0=np.zeros(1, dtype=np.int64), h=np.ones((1, 1)))
        else:
            t = resample_table(orig, new, lpw, rolloff)
        c = dict(M=t['M'], L=t['L'], NT=t['NT'], h=torch.from_numpy(t['h'].astype(np.float32)).to(device),
                 k0=torch.from_numpy(t['k0'].astype(np.int32)).to(device))
        _CONSTS[key] = c
    return c


def _plan(c, B, Lout, orig, new):
    g = _hip.ResampleGrids()
    rc = _hip.load().v2w_resample_plan(c['M'], c['L'], c['NT'], B, Lout, C.byref(g))
    if rc == _hip.E_SHAPE:
        raise ValueError(f'resample: {orig} -> {new} Hz reduces to {c["M"]} : {c["L"]} with {c["NT"]} taps per phase; the table of L * NT '
                         f'coefficients and one input window (2 M + 256 M / L samples) do not fit 64 KiB of LDS '
                         f'(include/vec2wav_hip.h: L * (NT + 2) + 2 M + 256 M / L must stay below 16384), or B * N / 256 passes 2^31')
    _hip.check(rc, 'v2w_resample_plan')
    return g


@_hip.on_tensor_device
def resample(x, orig_freq, new_freq, *, lengths=None, lowpass_filter_width=6, rolloff=0.99, peak=None):
    """x (B, n) or (n,) on the GPU, float32 or int16 PCM (read as x / 32768, exact) -> float32 (B, N), N = resampled_length(n, orig, new).
    lengths (mel.check_lengths' conventions): item b holds n_b = min(lengths[b], n) samples, out[b, :N_b] is what x[b:b+1, :n_b] alone gives,
    out[b, N_b:] is +0.0 and x[b, n_b:] is never loaded.  peak=0.95: each item divided by its own max |out_b| and multiplied by peak
    (librosa.util.normalize(...) * 0.95); an item whose maximum is below FLT_MIN keeps its bits.  orig_freq == new_freq: the float32 copy (one
    tap of 1.0 through the same kernel: lengths, the int16 scale and peak apply; a -0.0 comes out +0.0).
    ValueError: shapes, dtypes, lengths, a ratio whose table does not fit the kernel's LDS.  NotImplementedError: x requires grad under grad
    mode (forward only).  RuntimeError: CPU tensors (there is no CPU fallback)."""
    if not torch.is_tensor(x) or x.dim() not in (1, 2) or x.dtype not in (torch.float32, torch.int16):
        raise ValueError('resample: x must be a float32 or int16 tensor of shape (B, n) or (n,)')
    if x.dim() == 1:
        x = x.unsqueeze(0)
    B, n = x.shape
    if B < 1 or n < 1:
        raise ValueError(f'resample: empty input {tuple(x.shape)}')
    orig, new = int(orig_freq), int(new_freq)
    M, L = _ratio(orig_freq, new_freq)
    lpw, rolloff = int(lowpass_filter_width), float(rolloff)
    if peak is not None and not (math.isfinite(peak) and peak > 0):
        raise ValueError('resample: peak must be a positive number')
    src = None if lengths is None else mel.check_lengths(lengths, B, n)
    N = -(-n * L // M)
    if N > 2 ** 31 - 1 or n > 2 ** 31 - 1:
        raise ValueError('resample: more than 2^31 - 1 samples per item')
    if x.requires_grad and torch.is_grad_enabled():
        raise NotImplementedError('resample is forward only: x must not require grad')
    if not x.is_cuda:
        raise RuntimeError('resample runs on the MI355X HIP path only (no CPU fallback)')
    dev = x.device
    c = _constants(orig, new, lpw, rolloff, dev)
    g = _plan(c, B, N, orig, new)
    lib, st = _hip.load(), torch.cuda.current_stream(dev).cuda_stream
    x = x.detach().contiguous()
    out = torch.empty((B, N), dtype=torch.float32, device=dev)                      # (the kernel writes every float)
    part = torch.empty((B, g.tiles), dtype=torch.float32, device=dev) if peak is not None else None
    lens = None if src is None else mel._lengths_buffer(src, dev)
    _hip.check(lib.v2w_resample(x.data_ptr(), int(x.dtype == torch.int16), out.data_ptr(), B, n, N, c['h'].data_ptr(), c['k0'].data_ptr(),
                                c['M'], c['L'], c['NT'], _hip.ptr(lens), _hip.ptr(part), st), 'v2w_resample')
    if peak is not None:
        _hip.check(lib.v2w_peak_scale(out.data_ptr(), B, N, part.data_ptr(), g.tiles, float(peak), st), 'v2w_peak_scale')
    return out


def peak_normalize(y, peak=0.95, lengths=None):
    """librosa.util.normalize(y) * peak per item of y (B, n) or (n,), for audio that needs no rate change: `resample` at equal rates."""
    return resample(y, 1, 1, lengths=lengths, peak=peak)


class _MaskTailFn(torch.autograd.Function):
    """mask_tail on the GPU: the same kernel each way (the backward of a select is the select of the gradient).  `lens` is the call's own
    int32 tensor, kept by reference."""

    @staticmethod
    def forward(ctx, y, lens, len_mul):
        ctx.lens, ctx.len_mul = lens, len_mul
        return hipops.mask_tail(y.detach().contiguous(), lens, len_mul)

    @staticmethod
    @_hip.on_tensor_device
    def backward(ctx, g):
        return hipops.mask_tail(g.contiguous().float(), ctx.lens, ctx.len_mul), None, None


@_hip.on_tensor_device
def mask_tail(y, lengths, len_mul=1):
    """y (B, ..., L) float32 -> y with y[b, ..., n_b:] = +0.0, n_b = min(lengths[b] * len_mul, L) (mel.check_lengths' conventions), by select:
    NaN or Inf past n_b does not pass, and n_b = L returns y's bits.  Differentiable: the gradient passes on the valid part and is +0.0
    past it.  One launch each way (v2w_mask_tail); CPU tensors take the torch expression.
    A trainer that batches padded utterances applies this to the generated batch before the discriminators - the train-mode generator
    writes non-zero audio in the padding, which the discriminators would score and the `lengths=` losses would still see through the
    convs' windows at an utterance's last positions."""
    if not torch.is_tensor(y) or y.dim() < 2 or y.dtype != torch.float32:
        raise ValueError('mask_tail: y must be a float32 tensor of shape (B, ..., L)')
    B, L = y.shape[0], y.shape[-1]
    src = mel.check_lengths(lengths, B, L, len_mul)
    if not y.is_cuda:
        n = (src.to(torch.int64) * int(len_mul)).clamp(0, L).view(B, *([1] * (y.dim() - 1)))
        return torch.where(torch.arange(L).view(*([1] * (y.dim() - 1)), L) < n, y, torch.zeros((), dtype=y.dtype))
    lens = src.to(device=y.device, dtype=torch.int32).contiguous()
    if torch.is_grad_enabled() and y.requires_grad:
        return _MaskTailFn.apply(y, lens, int(len_mul))
    return hipops.mask_tail(y.detach().contiguous(), lens, int(len_mul))
