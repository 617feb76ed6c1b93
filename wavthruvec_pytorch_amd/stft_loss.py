"""Multi-resolution STFT loss on the MI355X (Yamamoto et al., Parallel WaveGAN): for every resolution (n_fft, hop_size, win_size) the spectral
convergence ||Y - X||_F / ||Y||_F and the log-magnitude L1 mean |log Y - log X| between the generated and the target audio, averaged over the
resolutions - the first auxiliary term trainers of HiFi-GAN-style vocoders add to the generator's loss.

The framing is `mel_spectrogram`'s (mel.stft_geometry), NOT torch.stft(center=True): reflect padding of int((n_fft - hop_size) / 2) samples
per side, a periodic hann window of win_size samples centred in the frame, F = mel_frames(L, n_fft, hop_size) frames, magnitudes
X = sqrt(Re^2 + Im^2 + 1e-9) over the n_fft // 2 + 1 bins (the magnitude of v2w_mel_finish: no zero norm and no log 0).

Per resolution the two phase launches write both signals into the halves of one (2 B, cp, FP) buffer and the DFT conv runs once over the 2 B
items (its input channels 64 per launch, for the accuracy of the log term's gradient: _dft_conv_fwd); then every resolution together: one streaming launch, one finishing launch (v2w_stft_loss_multi) and, in the backward, one launch that
writes every resolution's d spec (v2w_stft_loss_multi_bwd), followed per resolution by the input-gradient conv on the generated half and the
phases' backward.  No complex spectrum and no magnitude is ever stored; the loss values stay on the device.

A padded batch of unequal lengths (`lengths`, `len_mul`, as in mel.mel_loss): item b holds n_b = min(lengths[b] * len_mul, L) samples and
counts the F_b = mel_frames(n_b, n_fft, hop_size) frames that y_hat[b:b+1, :n_b] and y[b:b+1, :n_b] alone give (reflected about their own last
sample).  Per resolution there is still ONE Frobenius ratio and ONE mean, over the valid entries (b, bin, f < F_b) of the whole batch; the
same launches in their length-aware forms (v2w_mel_phases_geo_len, v2w_stft_loss_multi_len, _len_bwd, v2w_mel_phases_geo_len_bwd), no
frame count ever on the host.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _hip, mel

DEFAULT_RESOLUTIONS = ((1024, 120, 600), (2048, 240, 1200), (512, 50, 240))
_MEL = (1, 16000)       # (num_mels, sampling_rate) of the mel._constants key: the loss reads the DFT rows only, never the filterbank


def _constants(res, device):
    n_fft, hop, win = res
    return mel._constants(n_fft, _MEL[0], _MEL[1], hop, win, 0, None, device)


FWD_CHANNELS = 64      # input channels (hop phases) per launch of the forward DFT conv (see _dft_conv_fwd)


def _dft_conv_fwd(c, xp, spec):
    """xp (2 B, cp, FP) -> spec (2 B, cs, FP): the DFT conv, the cp input channels FWD_CHANNELS at a time, each launch adding its sum to spec
    (`accumulate`) - the forward's counterpart of mel._dft_conv_bwd.  In one launch a spec entry is one chain of k * cp fp32 terms; its drift of
    about sqrt(k * cp) roundings is 2.5 - 3 times the error of torch.stft's float32 FFT.  mel_spectrogram tolerates that (a filterbank sum and a
    log follow); here the log term's gradient, sgn(X - Y) / (N X) * Re / X, carries a spec error d as d / X^2, and at the entry of the smallest
    X that put d y_hat at 1024 / 120 / 600 at 5.8 times the oracle's float32 gap and the three-resolution module at 3.6.  Chains of
    k * FWD_CHANNELS terms joined by cp / FWD_CHANNELS additions bring them to 2.3 and 1.4 (32 channels per launch measure the same, 128
    channels 5.8 and 3.6; 0.19 ms of 2.5 at B = 32 x 81 920: DESIGN.md 3d'''').  A geometry with cp <= FWD_CHANNELS is one launch."""
    from . import hipops
    k, cp = c['k'], c['cp']
    if cp <= FWD_CHANNELS:
        hipops.conv1d(xp, c['wf'], None, spec, k=k, dil=1, slope=1.0, pad_left=0, wp=c['wp'])
        return
    key = 'wf_blocks_%d' % FWD_CHANNELS
    if key not in c:
        parts = [c['wf'][:, p:p + FWD_CHANNELS, :].contiguous() for p in range(0, cp, FWD_CHANNELS)]
        c[key] = [(w, hipops.pack_mfma(w)) for w in parts]
    for i, (w, wp) in enumerate(c[key]):
        p = i * FWD_CHANNELS
        hipops.conv1d(xp[:, p:p + FWD_CHANNELS], w, None, spec, k=k, dil=1, slope=1.0, pad_left=0, wp=wp, in_ct=cp, accumulate=i > 0)


def _items(cs, specs, B, geoms, dspecs=None):
    arr = (_hip.StftLossItem * len(cs))()
    for i, (d, c, spec, (F, FP)) in enumerate(zip(arr, cs, specs, geoms)):
        d.spec_x, d.spec_y = spec.data_ptr(), spec[B:].data_ptr()
        d.dspec_x = dspecs[i].data_ptr() if dspecs is not None else None
        d.B, d.Cs, d.FP, d.F, d.nb = B, c['cs'], FP, F, c['nb']
    return arr


def _geo_arrays(cs):
    """The HOST arrays (hop, n_fft) of the length-aware launches, one entry per resolution."""
    n = len(cs)
    return (C.c_int32 * n)(*[c['hop'] for c in cs]), (C.c_int32 * n)(*[c['n_fft'] for c in cs])


def _forward(x, y, resolutions, lens=None, len_mul=1):
    """x, y (B, L) float32 contiguous on one device -> (total (2,), sums fp64, specs, geoms); sums holds (Sd, Sy, Sl) per resolution, with
    lens (B int32 on the device) (Sd, Sy, Sl, N)."""
    B, L = x.shape
    dev = x.device
    lib, st = _hip.load(), torch.cuda.current_stream(dev).cuda_stream
    cs = [_constants(r, dev) for r in resolutions]
    geoms = [mel._frame_counts(c, L, 'stft_loss') for c in cs]
    specs = []
    for c, (F, FP) in zip(cs, geoms):
        xp = torch.empty((2 * B, c['cp'], FP), device=dev)
        mel._phases(lib, st, c, x, xp.data_ptr(), B, L, FP, lens, len_mul)
        mel._phases(lib, st, c, y, xp[B:].data_ptr(), B, L, FP, lens, len_mul)
        spec = torch.empty((2 * B, c['cs'], FP), device=dev)
        _dft_conv_fwd(c, xp, spec)
        specs.append(spec)
    n = len(cs)
    arr = _items(cs, specs, B, geoms)
    nbytes = lib.v2w_stft_loss_scratch_bytes(arr, n)
    _hip.check(min(nbytes, 0), 'v2w_stft_loss_scratch_bytes')
    scratch = torch.empty((nbytes // 8,), dtype=torch.float64, device=dev)
    total = torch.empty((2,), device=dev)
    sums = torch.empty(((3 if lens is None else 4) * n,), dtype=torch.float64, device=dev)
    out = (None, None, total.data_ptr(), sums.data_ptr(), scratch.data_ptr(), st)
    if lens is None:
        _hip.check(lib.v2w_stft_loss_multi(arr, n, *out), 'v2w_stft_loss_multi')
    else:
        _hip.check(lib.v2w_stft_loss_multi_len(arr, n, *_geo_arrays(cs), lens.data_ptr(), len_mul, *out), 'v2w_stft_loss_multi_len')
    return total, sums, specs, geoms


def _backward(g_sc, g_mag, sums, specs, geoms, resolutions, B, L, lens=None, len_mul=1):
    """-> d x (B, L): one launch for every resolution's d spec, then per resolution the input-gradient conv and the phases' backward."""
    dev = sums.device
    lib, st = _hip.load(), torch.cuda.current_stream(dev).cuda_stream
    cs = [mel._bwd_constants(_constants(r, dev)) for r in resolutions]
    dspecs = [torch.empty((B, c['cs'], FP), device=dev) for c, (_F, FP) in zip(cs, geoms)]     # (the kernel writes every float)
    arr = _items(cs, specs, B, geoms, dspecs)
    g_sc, g_mag = g_sc.contiguous().float(), g_mag.contiguous().float()
    grads = (sums.data_ptr(), g_sc.data_ptr(), g_mag.data_ptr(), None, None, st)
    if lens is None:
        _hip.check(lib.v2w_stft_loss_multi_bwd(arr, len(cs), *grads), 'v2w_stft_loss_multi_bwd')
    else:
        _hip.check(lib.v2w_stft_loss_multi_len_bwd(arr, len(cs), *_geo_arrays(cs), lens.data_ptr(), len_mul, *grads),
                   'v2w_stft_loss_multi_len_bwd')
    dx = None
    for c, dspec, (_F, FP) in zip(cs, dspecs, geoms):
        dxp = torch.empty((B, c['cp'], FP), device=dev)
        mel._dft_conv_bwd(c, dspec, dxp)
        d = torch.empty((B, L), device=dev)
        mel._phases(lib, st, c, dxp, d.data_ptr(), B, L, FP, lens, len_mul, bwd=True)
        dx = d if dx is None else dx.add_(d)
    return dx


class _StftLossFn(torch.autograd.Function):
    """(sc, mag) of the whole module; saves the sums, the specs and its own copy of the lengths (mel's buffer is rewritten by the next ragged
    call)."""

    @staticmethod
    def forward(ctx, x, y, resolutions, lens, len_mul):
        total, sums, specs, geoms = _forward(x.detach().contiguous(), y.detach().contiguous(), resolutions, lens, len_mul)
        ctx.save_for_backward(sums, None if lens is None else lens.clone(), *specs)
        ctx.geoms, ctx.resolutions, ctx.shape, ctx.len_mul = geoms, resolutions, tuple(x.shape), len_mul
        sc, mag = total.unbind(0)
        return sc, mag

    @staticmethod
    @_hip.on_tensor_device
    def backward(ctx, g_sc, g_mag):
        sums, lens, *specs = ctx.saved_tensors
        return _backward(g_sc, g_mag, sums, specs, ctx.geoms, ctx.resolutions, *ctx.shape, lens, ctx.len_mul), None, None, None, None


def _check_resolutions(resolutions):
    res = tuple(tuple(int(v) for v in r) for r in resolutions)
    if not 1 <= len(res) <= _hip.STFT_LOSS_MAX_ITEMS or any(len(r) != 3 for r in res):
        raise ValueError(f'stft_loss: 1 .. {_hip.STFT_LOSS_MAX_ITEMS} resolutions (n_fft, hop_size, win_size), got {resolutions!r}')
    for r in res:
        mel.stft_geometry(*r)               # ValueError outside 1 <= hop_size, win_size <= n_fft <= 2048, in stft_geometry's words
    return res


@_hip.on_tensor_device
def _loss(y_hat, y, resolutions, lengths=None, len_mul=1):
    if y.requires_grad:
        raise ValueError('stft_loss: the target y must not require grad (the loss differentiates with respect to y_hat only)')
    if y_hat.dim() == 3 and y_hat.shape[1] == 1:
        y_hat = y_hat.squeeze(1)
    if y.dim() == 3 and y.shape[1] == 1:
        y = y.squeeze(1)
    if y_hat.dim() != 2 or y_hat.shape != y.shape:
        raise ValueError(f'stft_loss: y_hat and y must be (B, L) or (B, 1, L) of one shape, got {tuple(y_hat.shape)} and {tuple(y.shape)}')
    src = None if lengths is None else mel.check_lengths(lengths, y_hat.shape[0], y_hat.shape[1], len_mul)
    if not (y_hat.is_cuda and y.is_cuda):
        raise RuntimeError('stft_loss runs on the MI355X HIP path only (no CPU fallback)')
    if y_hat.device != y.device:
        raise ValueError('stft_loss: y_hat and y must be on one device')
    y_hat, y = y_hat.float(), y.float()
    lens = None if src is None else mel._lengths_buffer(src, y_hat.device)
    if torch.is_grad_enabled() and y_hat.requires_grad:
        return _StftLossFn.apply(y_hat, y, resolutions, lens, int(len_mul))
    with torch.no_grad():
        sc, mag = _forward(y_hat.detach().contiguous(), y.detach().contiguous(), resolutions, lens, int(len_mul))[0].unbind(0)
    return sc, mag


def stft_loss(y_hat, y, n_fft, hop_size, win_size, *, lengths=None, len_mul=1):
    """One resolution: y_hat (generated), y (target) (B, L) or (B, 1, L) float32 on the GPU -> (sc, mag), 0-dim tensors on the device:
    sc = ||Y - X||_F / ||Y||_F and mag = mean |log Y - log X| over the (B, n_fft // 2 + 1, F) magnitudes, differentiable with respect to
    y_hat.  The frames are `mel_spectrogram`'s (reflect padding of int((n_fft - hop_size) / 2) per side, the window centred in the frame,
    mel_frames(L, n_fft, hop_size) of them), not those of torch.stft(center=True); any 1 <= hop_size <= n_fft, 1 <= win_size <= n_fft <= 2048.
    ValueError: y requires grad, the shapes differ, a geometry outside those limits.  RuntimeError: CPU tensors (there is no CPU fallback), a
    signal too short for the reflection or for one frame.

    lengths (B integers, a list or a tensor on any device; a device tensor is taken without a sync) and len_mul, as in mel_loss: a padded batch
    of unequal lengths.  Item b holds n_b = min(lengths[b] * len_mul, L) samples and counts the F_b = mel_frames(n_b, n_fft, hop_size) frames
    that y_hat[b:b+1, :n_b] and y[b:b+1, :n_b] alone give, the right-hand reflection about the item's own last sample.  The definition is still
    one Frobenius ratio and one mean over the valid entries of the WHOLE batch: sc = sqrt(sum (Y - X)^2) / sqrt(sum Y^2) and
    mag = sum |log Y - log X| / ((n_fft // 2 + 1) * sum_b F_b), the sums over (b, bin, f < F_b); both 0 when no item has a frame.  With
    lengths a B = 1 batch therefore equals the dense loss of y_hat[:, :n_b], y[:, :n_b].  y_hat[b, n_b:] and y[b, n_b:] have no effect,
    whatever they hold, and d y_hat[b, n_b:] is exactly +0.0.  An item too short for the reflection or for one frame counts nothing and gets
    a zero gradient; it is no error (L itself must still pass the two conditions above).  ValueError: what mel.check_lengths refuses (a
    wrong count, a float tensor, a host value < 1 or with lengths * len_mul > L, len_mul < 1)."""
    return _loss(y_hat, y, _check_resolutions([(n_fft, hop_size, win_size)]), lengths, len_mul)


class MultiResolutionSTFTLoss(torch.nn.Module):
    """forward(y_hat, y, lengths=None, len_mul=1) -> (sc_loss, mag_loss): the means over `resolutions` ((n_fft, hop_size, win_size), at most 8)
    of `stft_loss`'s two values, every resolution in the same three launches after its own STFT; one autograd node for the whole module.  The
    framing is `mel_spectrogram`'s, not torch.stft(center=True) (see `stft_loss`).

    lengths, len_mul: a padded batch of unequal lengths, as in `stft_loss` and `mel_loss` - per resolution one Frobenius ratio and one mean
    over the valid entries of the whole batch, each item's frames those of its own n_b = min(lengths[b] * len_mul, L) samples; with lengths a
    B = 1 batch equals the dense loss of y_hat[:, :n_b], y[:, :n_b].  An item too short for one resolution counts nothing in that resolution
    and gets no gradient from it."""

    def __init__(self, resolutions=DEFAULT_RESOLUTIONS):
        super().__init__()
        self.resolutions = _check_resolutions(resolutions)

    def forward(self, y_hat, y, lengths=None, len_mul=1):
        return _loss(y_hat, y, self.resolutions, lengths, len_mul)

    def extra_repr(self):
        return 'resolutions=%r' % (self.resolutions,)
