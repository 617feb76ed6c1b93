#!/usr/bin/env python3
"""mel_spectrogram (dataset.py:53-77) of the cfg2 generator output (B=32, 81 920 samples each) on the HIP path.

Without arguments: the reference geometry 1024 / 256 / 1024, forward.  --n_fft / --hop / --win / --mels / --sr choose another frame geometry;
--detail adds the forward + backward time, the two DFT convs alone (the same launches on buffers of the same shapes) and the contraction
length k x padded hop against n_fft, as one JSON line."""
import argparse, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from wavthruvec_pytorch_amd import hipops, mel
from wavthruvec_pytorch_amd.mel import mel_spectrogram

ap = argparse.ArgumentParser()
ap.add_argument('--n_fft', type=int, default=1024)
ap.add_argument('--hop', type=int, default=256)
ap.add_argument('--win', type=int, default=1024)
ap.add_argument('--mels', type=int, default=80)
ap.add_argument('--sr', type=int, default=16000)
ap.add_argument('--detail', action='store_true')
a = ap.parse_args()
cfg = (a.n_fft, a.mels, a.sr, a.hop, a.win, 0, None)
dev = torch.device('cuda:0')
B, L = 32, 81920
y = torch.tanh(torch.randn(B, L, device=dev))


def timed(fn, n=10, warm=3):
    for _ in range(warm): r = fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n): r = fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n, r


ms, m = timed(lambda: mel_spectrogram(y, *cfg))
g = mel.stft_geometry(a.n_fft, a.hop, a.win)
F = m.shape[2]
fl = 2.0 * B * F * g['k'] * g['cp'] * 2 * g['nb']
print(f'mel_spectrogram B={B} L={L} -> {tuple(m.shape)}: {ms:.3f} ms ({fl / ms / 1e9:.1f} TFLOP/s on the DFT, {B * L / ms / 1e3:.0f} M samples/s)')
if a.detail:
    yg = y.clone().requires_grad_(True)
    G = torch.randn_like(m)

    def both():
        yg.grad = None
        (mel_spectrogram(yg, *cfg) * G).sum().backward()
        return yg.grad
    ms_fb, _ = timed(both)
    c = mel._constants(*cfg, dev)
    FP = (F + c['k'] - 1 + 3) // 4 * 4
    xp, spec = torch.randn(B, c['cp'], FP, device=dev), torch.empty(B, c['cs'], FP, device=dev)
    ms_cf, _ = timed(lambda: hipops.conv1d(xp, c['wf'], None, spec, k=c['k'], dil=1, slope=1.0, pad_left=0, wp=c['wp']))
    dxp = torch.empty_like(xp)
    ms_cb, _ = timed(lambda: mel._dft_conv_bwd(c, spec, dxp))
    print(json.dumps(dict(geometry=[a.n_fft, a.hop, a.win], mels=a.mels, B=B, L=L, frames=F, taps=g['k'], channels=g['cp'],
                          contraction_over_n_fft=round(g['k'] * g['cp'] / a.n_fft, 4), forward_ms=round(ms, 4),
                          forward_backward_ms=round(ms_fb, 4), dft_conv_forward_ms=round(ms_cf, 4), dft_conv_backward_ms=round(ms_cb, 4),
                          conv_share_forward=round(ms_cf / ms, 3), conv_share_forward_backward=round((ms_cf + ms_cb) / ms_fb, 3))))
