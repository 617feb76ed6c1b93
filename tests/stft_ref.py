"""What the any-geometry entry points of csrc/v2w_mel.hip compute (v2w_mel_phases_geo, _geo_len, _geo_bwd), restated in numpy as
include/vec2wav_hip.h words them, beside tests/mel_ref.py (whose finish statements and bounds serve the _geo finish calls unchanged), and the
geometries and signals that tests/test_stft_geometry_cpu.py and tests/test_stft_geometry_gpu.py share.

A geometry is wavthruvec_pytorch_amd.mel.stft_geometry's dict: hop, cp >= hop channels, pad, left, k, n_fft.  The three phase calls move or
add floats in a fixed order and are held bit for bit."""
import numpy as np
import torch

from tests import mel_ref as R

SR = 16000
# (n_fft, hop, win): the small ones run at 8 mels, the three resolutions of a multi-resolution STFT loss at 80 mels
SMALL = [(128, 32, 128), (128, 32, 96), (128, 32, 75), (128, 48, 128), (128, 25, 100), (128, 128, 128)]
LARGE = [(512, 50, 240), (1024, 120, 600), (2048, 240, 1200)]
LARGE_B, LARGE_L, LARGE_MELS, SMALL_MELS = 2, 8192, 80, 8


def gid(g):
    return '%d_%d_%d' % tuple(g)


def cfg_of(geo, mels):
    """The positional arguments of mel_spectrogram after y."""
    n_fft, hop, win = geo
    return (n_fft, mels, SR, hop, win, 0, None)


def lengths_of(n_fft, hop, pad):
    """The smallest lengths at which something can still go wrong: pad + 1 (the shortest the reflection takes: no frame where the padded signal
    is still below n_fft, else the fewest there are), the shortest with exactly one frame (where pad + 1 does not already give two), and
    lengths whose (L + 2 pad - n_fft) % hop is 0 and hop - 1 (two and three frames past the first)."""
    one = max(pad + 1, n_fft - 2 * pad)
    base = max(n_fft - 2 * pad, 0) + 2 * hop
    while base <= pad:
        base += hop
    return sorted({pad + 1, one, base, base + hop - 1})


def signal(B, L, seed):
    """Seeded uniform noise of amplitude 0.5."""
    return np.random.default_rng(seed).uniform(-0.5, 0.5, (B, L)).astype(np.float32)


def frames(n, g):
    return (n + 2 * g['pad'] - g['n_fft']) // g['hop'] + 1 if n > g['pad'] and n + 2 * g['pad'] >= g['n_fft'] else 0


def columns(L, g):
    """FP of mel.py's launches for a signal of L samples."""
    return R.roundup4(frames(L, g) + g['k'] - 1)


def gather_map(L, g, FP):
    """src (cp, FP): xp[b][p][f] = y[b][src[p][f]], -1 where it is +0.0 (the padding channels, past the padded signal); i: the padded
    position f * hop + left + p.  The reflection is numpy's own."""
    pad = g['pad']
    ypad = np.pad(np.arange(L, dtype=np.int64), (pad, pad), mode='reflect') if pad else np.arange(L, dtype=np.int64)
    p = np.arange(g['cp'], dtype=np.int64)[:, None]
    i = np.arange(FP, dtype=np.int64)[None, :] * g['hop'] + g['left'] + p
    ok = (p < g['hop']) & (i < L + 2 * pad)
    return np.where(ok, ypad[np.minimum(i, L + 2 * pad - 1)], -1), i


def phases(y, g, FP):
    """v2w_mel_phases_geo: y (B, L) -> xp (B, cp, FP), a gather."""
    y = np.asarray(y, dtype=np.float32)
    src, _ = gather_map(y.shape[1], g, FP)
    return np.where(src[None] >= 0, y[:, np.maximum(src, 0)], np.float32(0))


def phases_len(y, g, FP, lens, len_mul=1):
    """v2w_mel_phases_geo_len: item b is the B = 1 call on y[b, :Lb] over that call's roundup4(F_b + k - 1) columns, +0.0 elsewhere."""
    y = np.asarray(y, dtype=np.float32)
    B, L = y.shape
    out = np.zeros((B, g['cp'], FP), dtype=np.float32)
    for b, Lb in enumerate(R.item_samples(lens, len_mul, L)):
        Lb = int(Lb)
        if frames(Lb, g):
            FPb = columns(Lb, g)
            out[b, :, :min(FP, FPb)] = phases(y[b:b + 1, :Lb], g, FPb)[0][:, :FP]
    return out


def phases_bwd(dxp, L, g):
    """v2w_mel_phases_geo_bwd: the transpose of gather_map in float32, added in the header's order: the sample's own position, its left
    reflection, its right reflection.  Positions the forward never reads (src = -1) contribute nothing, whatever dxp holds there."""
    dxp = np.asarray(dxp, dtype=np.float32)
    B, _, FP = dxp.shape
    src, i = gather_map(L, g, FP)
    dy = np.zeros((B, L), dtype=np.float32)
    kind = np.where(i < g['pad'], 1, np.where(i >= L + g['pad'], 2, 0))
    for kk in (0, 1, 2):
        sel = (src >= 0) & (kind == kk)
        s = src[sel]
        assert len(np.unique(s)) == len(s)                        # a sample has one position of each kind at most
        dy[:, s] = dxp[:, sel] if kk == 0 else dy[:, s] + dxp[:, sel]
    return dy


def contract(w, g, ypad):
    """S (B, 2 nb, F) in fp64: the DFT conv of mel.dft_conv_weights' w (k, cp, cs) over the padded signal ypad (B, L + 2 pad), written as
    the header states it: S[c][f] = sum_j sum_p w[j][p][c] * xg[p][f + j], xg[p][f] = ypad[f * hop + left + p] (0 past the end)."""
    B, Lp = ypad.shape
    hop, k = g['hop'], g['k']
    F = (Lp - g['n_fft']) // hop + 1
    z = np.concatenate([np.asarray(ypad, dtype=np.float64), np.zeros((B, (F + k) * hop + g['left']))], 1)
    xg = np.stack([z[:, g['left'] + p:g['left'] + p + (F + k - 1) * hop:hop] for p in range(hop)], 1)          # (B, hop, F + k - 1)
    S = np.zeros((B, 2 * g['nb'], F))
    for j in range(k):
        S += np.einsum('pc,bpf->bcf', w[j, :hop, :2 * g['nb']], xg[:, :, j:j + F])
    return S


def oracle_acc(y, cfg):
    """The fp64 filterbank sums (B, num_mels, F) of oracle.mel_oracle.mel_spectrogram(y, *cfg, dtype=float64), before the clamp and the log."""
    from oracle import mel_oracle as M
    n_fft, mels, sr, hop, win, fmin, fmax = cfg
    y = torch.as_tensor(y).double()
    pad = int((n_fft - hop) / 2)
    yp = torch.nn.functional.pad(y.unsqueeze(1), (pad, pad), mode='reflect').squeeze(1)
    spec = torch.stft(yp, n_fft, hop_length=hop, win_length=win, window=torch.hann_window(win, dtype=torch.float64), center=False,
                      return_complex=True)
    mag = torch.sqrt(spec.real.pow(2) + spec.imag.pow(2) + 1e-9)
    return torch.matmul(torch.from_numpy(M.mel_filterbank(sr, n_fft, mels, fmin, fmax)).double(), mag).numpy()


def near_clamp(y, cfg):
    """(B, num_mels, F) bool: entries whose fp64 filterbank sum lies within mel_ref.GAP (relative) of the 1e-5 clamp."""
    return np.abs(oracle_acc(y, cfg) / R.C5 - 1) < R.GAP


def oracle_gaps(y, cfg, G):
    """The oracle against itself, float32 against float64, on the CPU: (out64, dy64, max |out32 - out64| outside `near_clamp`,
    max |dy32 - dy64|) for the loss sum(G * out); G is zeroed on the near-clamp entries by the caller."""
    from oracle import mel_oracle as M
    res = {}
    for dt in (torch.float64, torch.float32):
        t = torch.from_numpy(np.asarray(y, dtype=np.float32)).to(dt).requires_grad_(True)
        out = M.mel_spectrogram(t, *cfg, dtype=dt)
        (out * torch.from_numpy(G).to(dt)).sum().backward()
        res[dt] = (out.detach().double().numpy(), t.grad.double().numpy())
    (o64, d64), (o32, d32) = res[torch.float64], res[torch.float32]
    keep = ~near_clamp(y, cfg)
    return o64, d64, float(np.abs(o32 - o64)[keep].max()), float(np.abs(d32 - d64).max())
