"""`mel_spectrogram` of the generated audio on the MI355X.

Mirror of the reference's `dataset.mel_spectrogram(y, n_fft, num_mels, sampling_rate, hop_size, win_size, fmin, fmax, center=False)`
(vec2wav/dataset.py:53-77; call sites train.py:172-174, 266-269, 282-284): same name, argument order and result
`(B, num_mels, frames)` = log(clamp(mel_basis @ |STFT|, 1e-5)), differentiable with respect to y (the training loss
back-propagates through it, train.py:204).

The STFT runs as ONE fused Conv1d on the f32 MFMA tile kernel: the reflect-padded signal is de-interleaved by hop phase
(`v2w_mel_phases_geo`), the windowed DFT rows are the conv weights, and `v2w_mel_finish_geo` does magnitude -> filterbank -> log, for any
geometry with 1 <= hop_size <= n_fft, 1 <= win_size <= n_fft <= 2048 (`stft_geometry`): the conv contracts over the window's support only -
ceil(win_size / hop_size) taps over hop_size channels rounded up to 32, the first of them `left = (n_fft - win_size) // 2` samples into the
frame.  At the reference geometry 1024 / 256 / 1024 and its like (win_size == n_fft, n_fft % hop_size == 0, hop_size % 32 == 0) that is hop
input channels x n_fft/hop taps, what the first entry points (`v2w_mel_phases`, `v2w_mel_finish`; kept for C callers) run on the same kernels.  Batches of unequal lengths (the reference's validation loop, batched: validate.py) take the per-item
form of the two ends (`lengths=`) and the masked L1 `mel_l1`.  `mel_loss` is the training loss of train.py:172-176,204 in one call, the L1 fused
into the finish kernel, with or without per-item lengths, forward and backward.  Constants (DFT rows, hann window, Slaney mel filterbank = librosa.filters.mel of the
reference's librosa, restated because librosa is not a dependency here) are built once per configuration with numpy in fp64.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Tuple

import numpy as np
import torch

from . import _hip, hipops

_CONSTS: Dict[Tuple, dict] = {}


def _hz_to_mel(f):
    f = np.asanyarray(f, dtype=np.float64)
    f_sp = 200.0 / 3
    logstep = np.log(6.4) / 27.0
    return np.where(f >= 1000.0, 1000.0 / f_sp + np.log(np.maximum(f, 1e-30) / 1000.0) / logstep, f / f_sp)


def _mel_to_hz(m):
    m = np.asanyarray(m, dtype=np.float64)
    f_sp = 200.0 / 3
    logstep = np.log(6.4) / 27.0
    return np.where(m >= 1000.0 / f_sp, 1000.0 * np.exp(logstep * (m - 1000.0 / f_sp)), f_sp * m)


def mel_filterbank(sr, n_fft, n_mels, fmin=0.0, fmax=None):
    """(n_mels, n_fft//2 + 1) float32: triangular filters on the Slaney mel scale with area normalisation, the published
    algorithm of librosa.filters.mel(sr, n_fft, n_mels, fmin, fmax, htk=False, norm='slaney') (dataset.py:9,64)."""
    fmax = sr / 2.0 if fmax is None else fmax
    fftfreqs = np.linspace(0, sr / 2.0, 1 + n_fft // 2)
    mel_f = _mel_to_hz(np.linspace(_hz_to_mel(fmin), _hz_to_mel(fmax), n_mels + 2))
    fdiff = np.diff(mel_f)
    ramps = mel_f[:, None] - fftfreqs[None, :]
    lower = -ramps[:-2] / fdiff[:-1, None]
    upper = ramps[2:] / fdiff[1:, None]
    w = np.maximum(0, np.minimum(lower, upper)) * (2.0 / (mel_f[2:n_mels + 2] - mel_f[:n_mels]))[:, None]
    return w.astype(np.float32)


MAX_N_FFT = 2048        # nb = 1025 bins: what the finish kernels' 8-frame block holds in 64 KiB of LDS next to 80 mels
CHANNEL_BLOCK = 32      # the DFT conv's input channels: C_in % 32 == 0 is what the f32 tile kernel's wide configurations take (v2w_layer_cfg)


def stft_geometry(n_fft, hop_size, win_size):
    """The frame geometry of `mel_spectrogram` (host only, no GPU): the reference's arithmetic (dataset.py:66-70) for any 1 <= hop_size <= n_fft,
    1 <= win_size <= n_fft <= 2048, a ValueError that names the condition otherwise.
      pad   samples of reflection per side, int((n_fft - hop_size) / 2): rounded down when the difference is odd
      left  zero weights before the window inside a frame, (n_fft - win_size) // 2 (torch.stft centres a short window)
      k     taps of the DFT conv: frame f multiplies ypad[f * hop + left + t] for t < win_size only, so k = ceil(win_size / hop_size)
      cp    its input channels: hop_size rounded up to CHANNEL_BLOCK; the channels [hop_size, cp) are zeros on both operands
      nb    bins, n_fft // 2 + 1;  cs: the 2 nb DFT rows rounded up to the conv tile's row block (64)
      old   win_size == n_fft, n_fft % hop_size == 0, hop_size % 32 == 0: the geometries the first entry points serve (cp == hop_size, left == 0,
            k == n_fft / hop_size: the same kernels, the same bits); here it only selects `_dft_conv_bwd`'s one-launch form"""
    n_fft, hop, win = int(n_fft), int(hop_size), int(win_size)
    if not 1 <= n_fft <= MAX_N_FFT:
        raise ValueError(f'mel_spectrogram (HIP): needs 1 <= n_fft <= {MAX_N_FFT}, got n_fft = {n_fft}')
    if not 1 <= hop <= n_fft:
        raise ValueError(f'mel_spectrogram (HIP): needs 1 <= hop_size <= n_fft, got hop_size = {hop}, n_fft = {n_fft}')
    if not 1 <= win <= n_fft:
        raise ValueError(f'mel_spectrogram (HIP): needs 1 <= win_size <= n_fft, got win_size = {win}, n_fft = {n_fft}')
    nb = n_fft // 2 + 1
    return dict(n_fft=n_fft, hop=hop, win=win, pad=int((n_fft - hop) / 2), left=(n_fft - win) // 2, k=-(-win // hop),
                cp=-(-hop // CHANNEL_BLOCK) * CHANNEL_BLOCK, nb=nb, cs=(2 * nb + 63) // 64 * 64,
                old=win == n_fft and n_fft % hop == 0 and hop % 32 == 0)


def dft_conv_weights(n_fft, hop_size, win_size):
    """-> (geometry, w): the windowed DFT rows as the DFT conv's weights, numpy fp64 (host only).  w[j][p][c] = Wd[c][left + j * hop + p] for
    p < hop and j * hop + p < win_size, else 0; rows c < nb are cos(2 pi c n / n_fft) * hann(n - left), rows nb <= c < 2 nb the -sin ones,
    the rest (up to cs) zeros.  With xg[p][f] = ypad[f * hop + left + p]:  S[c][f] = sum_{j < k} sum_{p < hop} w[j][p][c] * xg[p][f + j]."""
    g = stft_geometry(n_fft, hop_size, win_size)
    n_fft, hop, win, nb, k, cs = g['n_fft'], g['hop'], g['win'], g['nb'], g['k'], g['cs']
    t = np.arange(k * hop, dtype=np.float64)                    # offset into the window's support (the last tap may run past it)
    hann = np.where(t < win, 0.5 - 0.5 * np.cos(2.0 * np.pi * t / win), 0.0)           # torch.hann_window(win_size): periodic
    if win == 1:
        hann[0] = 1.0                                           # (torch.hann_window(1) is [1.])
    ang = 2.0 * np.pi * np.outer(np.arange(nb, dtype=np.float64), t + g['left']) / n_fft
    wd = np.zeros((cs, k * hop), dtype=np.float64)
    wd[:nb] = np.cos(ang) * hann
    wd[nb:2 * nb] = -np.sin(ang) * hann
    w = np.zeros((k, g['cp'], cs), dtype=np.float64)
    w[:, :hop, :] = wd.reshape(cs, k, hop).transpose(1, 2, 0)   # [tap j][channel p][row c] = Wd[c][j*hop + p]
    return g, w


def _constants(n_fft, num_mels, sampling_rate, hop_size, win_size, fmin, fmax, device):
    key = (n_fft, num_mels, sampling_rate, hop_size, win_size, fmin, fmax, str(device))
    c = _CONSTS.get(key)
    if c is None:
        g, w = dft_conv_weights(n_fft, hop_size, win_size)
        wf = torch.from_numpy(np.ascontiguousarray(w).astype(np.float32)).to(device)
        c = dict(g, wf=wf, wp=hipops.pack_mfma(wf),
                 basis=torch.from_numpy(mel_filterbank(sampling_rate, g['n_fft'], num_mels, fmin, fmax)).to(device))
        _CONSTS[key] = c
    return c


def mel_frames(n_samples, n_fft, hop_size):
    """Frames `mel_spectrogram` (center=False) gives a signal of n_samples: the reflect padding of (n_fft - hop)/2 per side needs more samples
    than that and a frame needs n_fft padded ones, else 0 (the reference raises there)."""
    pad = int((n_fft - hop_size) / 2)
    n = int(n_samples)
    return (n + 2 * pad - n_fft) // hop_size + 1 if n > pad and n + 2 * pad >= n_fft else 0


_LEN_BUFS: Dict[Tuple, torch.Tensor] = {}


def check_lengths(lengths, B, L=None, len_mul=1):
    """The `lengths` argument of a ragged call -> an integer tensor of B entries (a list's or host tensor's values validated: 1 <= n and,
    given L, n * len_mul <= L; a device tensor is taken as it is, without a sync - the kernels clamp it)."""
    len_mul = int(len_mul)
    if len_mul < 1:
        raise ValueError('len_mul must be >= 1')
    if torch.is_tensor(lengths):
        if lengths.dtype.is_floating_point or lengths.dtype.is_complex or lengths.dtype == torch.bool or tuple(lengths.shape) != (B,):
            raise ValueError(f'lengths must hold {B} integers')
        src = lengths.detach()
    else:
        vals = [int(n) for n in lengths]
        if len(vals) != B:
            raise ValueError(f'lengths must hold {B} integers, got {len(vals)}')
        src = torch.tensor(vals, dtype=torch.int64)
    if not src.is_cuda and src.numel():
        if int(src.min()) < 1:
            raise ValueError('lengths must be >= 1')
        if L is not None and int(src.max()) * len_mul > L:
            raise ValueError(f'lengths * len_mul must not exceed L = {L}')
    return src


def _lengths_buffer(src, device):
    """The module-owned int32 device buffer the kernels read, written on the current stream (in order with the launches on both sides)."""
    key = (str(device), torch.cuda.current_stream(device).cuda_stream, src.numel())
    buf = _LEN_BUFS.get(key)
    if buf is None:
        buf = _LEN_BUFS[key] = torch.empty((src.numel(),), dtype=torch.int32, device=device)
    buf.copy_(src.to(torch.int32))
    return buf


def _frame_counts(c, L, who):
    """-> (F, FP): the frames of a signal of L samples and the columns of its phase buffer, with the two conditions on the length."""
    pad = c['pad']
    if pad >= L:
        raise RuntimeError(f'{who}: reflect padding needs more than (n_fft - hop)/2 samples')
    if L + 2 * pad < c['n_fft']:
        raise RuntimeError(f'{who}: the padded signal is shorter than one frame of n_fft samples')
    F = (L + 2 * pad - c['n_fft']) // c['hop'] + 1
    return F, (F + c['k'] - 1 + 3) // 4 * 4


_PHASES = {(False, False): 'v2w_mel_phases_geo', (True, False): 'v2w_mel_phases_geo_len',
           (False, True): 'v2w_mel_phases_geo_bwd', (True, True): 'v2w_mel_phases_geo_len_bwd'}       # (lengths, backward)


def _phases(lib, st, c, src, dst_ptr, B, L, FP, lens=None, len_mul=1, bwd=False):
    """One phase launch on the caller's library handle and stream.  Forward: src = y (B, L) -> xp (B, cp, FP) at dst_ptr; backward: src = dxp
    -> dy (B, L).  lens (B int32 on the device): the per-item form."""
    name = _PHASES[lens is not None, bwd]
    tail = () if lens is None else (lens.data_ptr(), len_mul)
    _hip.check(getattr(lib, name)(src.data_ptr(), dst_ptr, B, L, c['n_fft'], c['win'], c['hop'], c['cp'], c['pad'], c['left'], c['k'], FP,
                                  *tail, st), name)


def _spectrum(y, cfg, lens=None, len_mul=1):
    """-> (spec, constants, geometry): the first two launches of the forward, the phases step and the DFT conv.  lens (B int32 on the device):
    the per-item form of the phases step; the DFT conv runs on the whole padded batch either way."""
    n_fft, num_mels, sampling_rate, hop_size, win_size, fmin, fmax = cfg
    B, L = y.shape
    c = _constants(n_fft, num_mels, sampling_rate, hop_size, win_size, fmin, fmax, y.device)
    F, FP = _frame_counts(c, L, 'mel_spectrogram')
    lib, st = _hip.load(), torch.cuda.current_stream(y.device).cuda_stream
    xp = torch.empty((B, c['cp'], FP), device=y.device)
    _phases(lib, st, c, y, xp.data_ptr(), B, L, FP, lens, len_mul)
    spec = torch.empty((B, c['cs'], FP), device=y.device)
    hipops.conv1d(xp, c['wf'], None, spec, k=c['k'], dil=1, slope=1.0, pad_left=0, wp=c['wp'])
    return spec, c, (B, L, c['pad'], F, FP)


def _forward(y, cfg, lens=None, len_mul=1):
    """-> (out, spec, geometry): the three launches of the forward; `spec` is what the backward needs.  lens: the per-item form of the two
    ends (forward only)."""
    num_mels = cfg[1]
    spec, c, (B, L, pad, F, FP) = _spectrum(y, cfg, lens, len_mul)
    lib, st = _hip.load(), torch.cuda.current_stream(y.device).cuda_stream
    out = torch.empty((B, num_mels, F), device=y.device)
    fin = (spec.data_ptr(), c['basis'].data_ptr(), out.data_ptr(), B, c['cs'], FP, F, c['nb'], num_mels)
    if lens is None:
        _hip.check(lib.v2w_mel_finish_geo(*fin, st), 'v2w_mel_finish_geo')
    else:
        _hip.check(lib.v2w_mel_finish_geo_len(*fin, lens.data_ptr(), len_mul, c['hop'], c['n_fft'], st), 'v2w_mel_finish_geo_len')
    return out, spec, (B, L, pad, F, FP)


BWD_ROWS = 128         # DFT rows per launch of the input-gradient conv at the geometries the `_geo` calls serve (see _dft_conv_bwd)


def _dft_conv_bwd(c, dspec, dxp, by_rows=False):
    """dspec (B, cs, FP) -> dxp (B, cp, FP): the DFT conv's input gradient.  One launch at the geometries the first entry points serve (their
    bits; `by_rows`: mel_loss, which has no earlier bits to keep, goes BWD_ROWS at a time there too - at 1024 / 256 / 1024 the one chain of
    4 x 1088 terms put its d y at 2.7 - 9.5 times the oracle's float32 gap).  Elsewhere the cs rows go BWD_ROWS at a time, each launch adding its sum to dxp (`accumulate`): a dot product of k * cs fp32
    terms added in one chain drifts by about sqrt(k * cs / 2) roundings (51 at 1024 / 120 / 600, 72 at n_fft 2048), which put d y at 7.7 and
    4.8 times the float32 gap of torch.stft's FFT there; chains of k * BWD_ROWS terms joined by cs / BWD_ROWS additions bring it to 2.4 and
    1.6 (64 rows per launch measure the same, 256 rows 3.3 and 1.8: DESIGN.md 3d''')."""
    k, cs = c['k'], c['cs']
    if (c['old'] and not by_rows) or cs <= BWD_ROWS:
        hipops.conv1d(dspec, c['wT'], None, dxp, k=k, dil=1, slope=1.0, pad_left=k - 1, wp=c['wTp'])
        return
    if 'wT_rows' not in c:
        parts = [c['wT'][:, r:r + BWD_ROWS, :].contiguous() for r in range(0, cs, BWD_ROWS)]
        c['wT_rows'] = [(w, hipops.pack_mfma(w)) for w in parts]
    for i, (w, wp) in enumerate(c['wT_rows']):
        r = i * BWD_ROWS
        hipops.conv1d(dspec[:, r:r + BWD_ROWS], w, None, dxp, k=k, dil=1, slope=1.0, pad_left=k - 1, wp=wp, in_ct=cs, accumulate=i > 0)


def _bwd_constants(c):
    """The constants of a configuration with what its backward adds to them (built at the first backward)."""
    if 'wT' not in c:
        # wT[j'][row c][phase p] = Wd[c][left + (k-1-j')*hop + p]
        c['wT'] = c['wf'].flip(0).transpose(1, 2).contiguous()
        c['wTp'] = hipops.pack_mfma(c['wT'])
        c['basisT'] = c['basis'].t().contiguous()
    return c


def _backward(g, spec, geom, cfg):
    """d out (B, num_mels, F) -> d y (B, L): finish^T -> the DFT conv's input gradient (the same MFMA conv kernel with the
    tap-flipped transposed rows, pad_left = k-1) -> phase re-interleave with the reflections folded back."""
    n_fft, num_mels, sampling_rate, hop_size, win_size, fmin, fmax = cfg
    B, L, pad, F, FP = geom
    dev = spec.device
    c = _bwd_constants(_constants(n_fft, num_mels, sampling_rate, hop_size, win_size, fmin, fmax, dev))
    lib, st = _hip.load(), torch.cuda.current_stream(dev).cuda_stream
    g = g.contiguous().float()
    dspec = torch.zeros_like(spec)
    _hip.check(lib.v2w_mel_finish_geo_bwd(spec.data_ptr(), c['basis'].data_ptr(), c['basisT'].data_ptr(), g.data_ptr(), dspec.data_ptr(),
                                          B, c['cs'], FP, F, c['nb'], num_mels, st), 'v2w_mel_finish_geo_bwd')
    return _spectrum_backward(c, dspec, geom)


def _spectrum_backward(c, dspec, geom, lens=None, len_mul=1, by_rows=False):
    """d spec (B, cs, FP) -> d y (B, L): the backward of `_spectrum`.  lens: the per-item form of the phase backward (the reflection about
    the item's own last sample, +0.0 past it); the DFT conv's input gradient runs on the whole padded batch either way."""
    B, L, pad, F, FP = geom
    dev = dspec.device
    lib, st = _hip.load(), torch.cuda.current_stream(dev).cuda_stream
    dxp = torch.empty((B, c['cp'], FP), device=dev)
    _dft_conv_bwd(c, dspec, dxp, by_rows)
    dy = torch.empty((B, L), device=dev)
    _phases(lib, st, c, dxp, dy.data_ptr(), B, L, FP, lens, len_mul, bwd=True)
    return dy


class _MelFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, y, cfg):
        out, spec, geom = _forward(y.detach().contiguous().float(), cfg)
        ctx.save_for_backward(spec)
        ctx.geom, ctx.cfg = geom, cfg
        return out

    @staticmethod
    @_hip.on_tensor_device
    def backward(ctx, g):
        (spec,) = ctx.saved_tensors
        return _backward(g, spec, ctx.geom, ctx.cfg), None


@_hip.on_tensor_device
def mel_spectrogram(y, n_fft, num_mels, sampling_rate, hop_size, win_size, fmin, fmax, center=False, *, lengths=None, len_mul=1):
    """y (B, L) float32 on the GPU -> (B, num_mels, frames) float32; differentiable with respect to y (the training loss
    F.l1_loss(y_mel, mel_spectrogram(y_g_hat.squeeze(1), ...)), train.py:172-174,204).

    Any frame geometry with 1 <= hop_size <= n_fft and 1 <= win_size <= n_fft <= 2048 (a ValueError names the condition otherwise), with the
    reference's arithmetic: reflect padding of int((n_fft - hop_size) / 2) samples per side, a periodic hann window of win_size samples
    centred in the frame, (L + 2 pad - n_fft) // hop_size + 1 frames.  center=True is not implemented.  A hop_size far below 32 pays for 32
    channels per tap.

    lengths (optional, no-grad only; B integers, a list or a tensor on any device) and len_mul: item b holds min(lengths[b] * len_mul, L)
    samples - a batch of generated utterances of unequal length as Generator.forward(lengths=...) returns it, len_mul = prod(upsample_rates).
    out[b, :, :F_b] is then what y[b:b+1, :n_b] alone gives (F_b = mel_frames(n_b, n_fft, hop_size)), out[b, :, F_b:] is exactly 0 - the zero
    padding of a padded target mel (dataset.py:194-218) - and y[b, n_b:] has no effect, whatever it holds."""
    if center:
        raise NotImplementedError('mel_spectrogram (HIP): center=False only (the reference never passes True)')
    stft_geometry(n_fft, hop_size, win_size)               # ValueError outside 1 <= hop_size, win_size <= n_fft <= 2048
    src = None
    if lengths is not None:
        if y.dim() != 2:
            raise ValueError('mel_spectrogram(lengths=...): y must be (B, L)')
        src = check_lengths(lengths, y.shape[0], y.shape[1], len_mul)
        if torch.is_grad_enabled() and y.requires_grad:
            raise NotImplementedError('mel_spectrogram(lengths=...): no-grad only (the backward with per-item lengths is not implemented)')
    if not y.is_cuda:
        raise RuntimeError('mel_spectrogram runs on the MI355X HIP path only (no CPU fallback)')
    cfg = (n_fft, num_mels, sampling_rate, hop_size, win_size, fmin, fmax)
    if src is not None:
        with torch.no_grad():
            return _forward(y.detach().contiguous().float(), cfg, _lengths_buffer(src, y.device), int(len_mul))[0]
    if torch.is_grad_enabled() and y.requires_grad:
        return _MelFn.apply(y, cfg)
    with torch.no_grad():
        return _forward(y.detach().contiguous().float(), cfg)[0]


@_hip.on_tensor_device
def mel_l1(a, b, lengths, len_mul=1, *, n_fft, hop_size):
    """Masked L1 between two padded mel batches a, b (B, num_mels, F) float32 on the GPU, no-grad: item i counts its first
    F_i = min(mel_frames(lengths[i] * len_mul, n_fft, hop_size), F) frames.  -> (total, per_item): per_item[i] = mean |a - b| over item i's
    num_mels x F_i elements (F.l1_loss of the trimmed pair; 0 for F_i = 0), total = the mean over every valid element of the batch.
    Deterministic (fixed-order fp64 sums, no atomics); an item's value does not depend on the other items."""
    n_fft, hop_size = int(n_fft), int(hop_size)
    if not 1 <= hop_size <= n_fft:
        raise ValueError(f'mel_l1: needs 1 <= hop_size <= n_fft, got hop_size = {hop_size}, n_fft = {n_fft}')
    if not (a.is_cuda and b.is_cuda):
        raise RuntimeError('mel_l1 runs on the MI355X HIP path only (no CPU fallback)')
    if a.dim() != 3 or a.shape != b.shape or a.device != b.device:
        raise ValueError('mel_l1: a and b must be (B, num_mels, F) tensors of one shape on one device')
    B, Cm, F = a.shape
    len_mul = int(len_mul)
    src = check_lengths(lengths, B, None, len_mul)          # (frame counts past F are clamped to F)
    with torch.no_grad():
        a = a.detach().contiguous().float()
        b = b.detach().contiguous().float()
        lens = _lengths_buffer(src, a.device)
        lib, st = _hip.load(), torch.cuda.current_stream(a.device).cuda_stream
        G = lib.v2w_l1_masked_plan(Cm, F)
        _hip.check(min(G, 0), 'v2w_l1_masked_plan')
        ws = torch.empty((B * G,), dtype=torch.float64, device=a.device)
        per_item = torch.empty((B,), device=a.device)
        total = torch.empty((1,), device=a.device)
        _hip.check(lib.v2w_l1_masked_geo(a.data_ptr(), b.data_ptr(), B, Cm, F, lens.data_ptr(), len_mul, hop_size, n_fft,
                                         per_item.data_ptr(), total.data_ptr(), ws.data_ptr(), st), 'v2w_l1_masked_geo')
    return total[0], per_item


def _loss_launch(spec, c, geom, tgt, frames_first, num_mels, lens, len_mul, scale):
    """The fused finish + L1 and its finishing launch on `spec` -> (total (1,), per_item (B,), coef (1,)), all on the device."""
    B, L, pad, F, FP = geom
    dev = spec.device
    lib, st = _hip.load(), torch.cuda.current_stream(dev).cuda_stream
    Ft = tgt.shape[1] if frames_first else tgt.shape[2]
    nbytes = C.c_longlong(0)
    tiles = lib.v2w_mel_loss_plan(B, F, c['nb'], num_mels, C.byref(nbytes))
    _hip.check(min(tiles, 0), 'v2w_mel_loss_plan')
    ws = torch.empty((nbytes.value // 8,), dtype=torch.float64, device=dev)
    per_item, total, coef = torch.empty((B,), device=dev), torch.empty((1,), device=dev), torch.empty((1,), device=dev)
    strides = (num_mels, 1) if frames_first else (1, Ft)
    _hip.check(lib.v2w_mel_loss_fwd(spec.data_ptr(), c['basis'].data_ptr(), tgt.data_ptr(), *strides, B, c['cs'], FP, F, Ft, c['nb'], num_mels,
                                    lens.data_ptr() if lens is not None else None, len_mul, c['hop'], c['n_fft'], scale,
                                    per_item.data_ptr(), total.data_ptr(), coef.data_ptr(), ws.data_ptr(), st), 'v2w_mel_loss_fwd')
    return total, per_item, coef


class _MelLossFn(torch.autograd.Function):
    """total, per_item = mel_loss's two results; saves spec, the target, coef and its own copy of the lengths (the module's buffer is
    rewritten by the next ragged call).  Backward: fused finish backward -> the DFT conv's input gradient -> phase backward."""

    @staticmethod
    def forward(ctx, y, tgt, cfg, lens, len_mul, scale, frames_first):
        spec, c, geom = _spectrum(y.detach().contiguous().float(), cfg, lens, len_mul)
        total, per_item, coef = _loss_launch(spec, c, geom, tgt, frames_first, cfg[1], lens, len_mul, scale)
        ctx.save_for_backward(spec, tgt, coef, None if lens is None else lens.clone())
        ctx.geom, ctx.cfg, ctx.len_mul, ctx.frames_first = geom, cfg, len_mul, frames_first
        ctx.mark_non_differentiable(per_item)
        return total.reshape(()), per_item

    @staticmethod
    @_hip.on_tensor_device
    def backward(ctx, g, _g_per_item):
        spec, tgt, coef, lens = ctx.saved_tensors
        n_fft, num_mels, sampling_rate, hop_size, win_size, fmin, fmax = ctx.cfg
        B, L, pad, F, FP = ctx.geom
        dev = spec.device
        c = _bwd_constants(_constants(n_fft, num_mels, sampling_rate, hop_size, win_size, fmin, fmax, dev))
        lib, st = _hip.load(), torch.cuda.current_stream(dev).cuda_stream
        g = g.detach().reshape(1).contiguous().float()
        Ft = tgt.shape[1] if ctx.frames_first else tgt.shape[2]
        strides = (num_mels, 1) if ctx.frames_first else (1, Ft)
        dspec = torch.zeros_like(spec)
        _hip.check(lib.v2w_mel_loss_bwd(spec.data_ptr(), c['basis'].data_ptr(), c['basisT'].data_ptr(), tgt.data_ptr(), *strides,
                                        g.data_ptr(), coef.data_ptr(), dspec.data_ptr(), B, c['cs'], FP, F, Ft, c['nb'], num_mels,
                                        lens.data_ptr() if lens is not None else None, ctx.len_mul, c['hop'], c['n_fft'], st),
                   'v2w_mel_loss_bwd')
        return _spectrum_backward(c, dspec, ctx.geom, lens, ctx.len_mul, by_rows=True), None, None, None, None, None, None


@_hip.on_tensor_device
def mel_loss(y_hat, y_mel, n_fft, num_mels, sampling_rate, hop_size, win_size, fmin, fmax, *,
             lengths=None, len_mul=1, scale=1.0, frames_first=True, per_item=False):
    """The mel L1 training loss in one call, differentiable with respect to y_hat: scale * F.l1_loss(y_mel[:, :F], mel_spectrogram(y_hat,
    ...).permute(0, 2, 1)) (train.py:172-176,204), with the L1 fused into the mel's last kernel - the (B, num_mels, F) mel is never stored.

    y_hat (B, L) or (B, 1, L) float32 on the GPU; y_mel the padded target, (B, F_t, num_mels) when frames_first (train.py's y_mel) else
    (B, num_mels, F_t), never differentiated.  Without lengths F_t >= F = mel_frames(L) is required.

    lengths (B integers, a list or a tensor on any device; a device tensor is taken without a sync) and len_mul, as in mel_spectrogram: item b
    holds n_b = min(lengths[b] * len_mul, L) samples and counts F_b = min(mel_frames(n_b), F, F_t) frames of the mel that y_hat[b:b+1, :n_b]
    alone gives.  The loss is scale * (sum of |mel - target| over the valid entries) / (num_mels * sum_b F_b), mel_l1's `total`; 0 when no
    entry is valid.  y_hat[b, n_b:] and the target past F_b have no effect, whatever they hold, and d y_hat[b, n_b:] is exactly +0.0.

    -> the loss (0-dim), and with per_item=True also the detached (B,) per-item means (mel_l1's `per_item`).  Deterministic: fixed-order
    fp64 sums, no atomics."""
    g = stft_geometry(n_fft, hop_size, win_size)           # ValueError outside 1 <= hop_size, win_size <= n_fft <= 2048
    num_mels = int(num_mels)
    if y_hat.dim() == 3 and y_hat.shape[1] == 1:
        y = y_hat.reshape(y_hat.shape[0], y_hat.shape[2])
    elif y_hat.dim() == 2:
        y = y_hat
    else:
        raise ValueError('mel_loss: y_hat must be (B, L) or (B, 1, L)')
    B, L = y.shape
    want = (B, -1, num_mels) if frames_first else (B, num_mels, -1)
    if y_mel.dim() != 3 or any(w >= 0 and s != w for s, w in zip(y_mel.shape, want)):
        raise ValueError('mel_loss: y_mel must be (B, F_t, num_mels) when frames_first, else (B, num_mels, F_t)')
    Ft = y_mel.shape[1] if frames_first else y_mel.shape[2]
    if torch.is_grad_enabled() and y_mel.requires_grad:
        raise NotImplementedError('mel_loss: the target y_mel is not differentiated')
    F = mel_frames(L, g['n_fft'], g['hop'])
    src = None
    if lengths is not None:
        src = check_lengths(lengths, B, L, len_mul)
        if Ft < 1:
            raise ValueError('mel_loss: y_mel holds no frame')
    elif Ft < F:
        raise ValueError(f'mel_loss: y_mel holds {Ft} frames, y_hat gives {F}')
    if not (y.is_cuda and y_mel.is_cuda):
        raise RuntimeError('mel_loss runs on the MI355X HIP path only (no CPU fallback)')
    if y.device != y_mel.device:
        raise ValueError('mel_loss: y_hat and y_mel must be on one device')
    cfg = (n_fft, num_mels, sampling_rate, hop_size, win_size, fmin, fmax)
    tgt = y_mel.detach().contiguous().float()
    lens = None if src is None else _lengths_buffer(src, y.device)
    args = (tgt, cfg, lens, int(len_mul), float(scale), bool(frames_first))
    if torch.is_grad_enabled() and y.requires_grad:
        total, per = _MelLossFn.apply(y, *args)
    else:
        with torch.no_grad():
            spec, c, geom = _spectrum(y.detach().contiguous().float(), cfg, lens, int(len_mul))
            total, per, _coef = _loss_launch(spec, c, geom, tgt, bool(frames_first), num_mels, lens, int(len_mul), float(scale))
            total = total.reshape(())
    return (total, per.detach()) if per_item else total
