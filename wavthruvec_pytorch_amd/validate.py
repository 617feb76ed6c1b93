"""The reference's validation loop, batched (vec2wav/train.py:246-289).

The reference validates one whole utterance at a time, at B = 1:

    y_g_hat = generator(wv_feat, spk_emb, noise)
    y_g_hat_mel = mel_spectrogram(y_g_hat.squeeze(1), n_fft, num_mels, sampling_rate, hop_size, win_size, fmin, fmax_for_loss)
    y_mel = y_mel[:, :y_g_hat_mel.shape[1], :]                       (both as (1, frames, num_mels); train.py:269-273)
    val_err_tot += F.l1_loss(y_mel, y_g_hat_mel).item()

`mel_errors` runs the same three steps on batches of utterances of unequal length: one ragged forward (Generator.forward(lengths=...)), one
ragged `mel_spectrogram(lengths=ts, len_mul=prod(upsample_rates))` and one masked `mel_l1` against the zero-padded targets per batch; every
utterance gets the error of its own single run.  Precision 'f32', eval mode, no gradients (what the ragged forward serves).
"""
from __future__ import annotations

from typing import Sequence

import torch

from .mel import mel_frames, mel_l1, mel_spectrogram
from .synthesize import item_noise, pad_batch, plan_batches


def pad_targets(y_mels: Sequence[torch.Tensor], idx: Sequence[int], frames: Sequence[int], F: int) -> torch.Tensor:
    """The loader's (frames_i, num_mels) targets of the items `idx`, each cropped to its generated frame count (train.py:273), transposed and
    zero-padded to (n, num_mels, F) - the padding collate_fn_tensor / pad_2D_tensor give a batch of target mels (dataset.py:194-218)."""
    num_mels = y_mels[idx[0]].shape[-1]
    tgt = torch.zeros((len(idx), num_mels, F), dtype=torch.float32)
    for j, i in enumerate(idx):
        m = y_mels[i]
        if m.dim() != 2 or m.shape[1] != num_mels:
            raise ValueError(f'y_mels[{i}]: expected (frames, {num_mels}), got {tuple(m.shape)}')
        if m.shape[0] < frames[j]:
            raise ValueError(f'y_mels[{i}] holds {m.shape[0]} frames, the generated audio {frames[j]} (the reference\'s l1_loss would not '
                             'broadcast either)')
        tgt[j, :, :frames[j]] = m[:frames[j]].t()
    return tgt


@torch.no_grad()
def mel_errors(g, feats: Sequence[torch.Tensor], spks: Sequence[torch.Tensor], y_mels: Sequence[torch.Tensor], h, seed: int = 1234,
               batch: int = 8) -> torch.Tensor:
    """Per-utterance validation mel errors, in input order, as a float32 CPU tensor; their mean is the reference's `val_err`.

    feats: (1, C, T_i) latents and spks: (1, spk_dim) embeddings as `synthesize.synthesize_many` takes them; y_mels[i]: the loader's
    (frames_i, num_mels) target of utterance i; h: the hyperparameters (n_fft, num_mels, sampling_rate, hop_size, win_size, fmin,
    fmax_for_loss, upsample_rates).  Up to `batch` utterances, neighbours in length, share a forward; a batch of one takes the same path with
    lengths=[T].  Every utterance runs with the noise of a single run seeded with `seed` (synthesize.item_noise)."""
    if not (len(feats) == len(spks) == len(y_mels)):
        raise ValueError('feats, spks and y_mels must have one entry per utterance')
    dev = next(g.parameters()).device
    hop_total = 1
    for u in h.upsample_rates:
        hop_total *= u
    nz = item_noise(h.noise_dim, seed)
    out = torch.zeros((len(feats),), dtype=torch.float32, device=dev)
    for idx in plan_batches([f.shape[-1] for f in feats], batch):
        x, ts = pad_batch(feats, idx)
        frames = [mel_frames(t * hop_total, h.n_fft, h.hop_size) for t in ts]
        if min(frames) < 1:
            raise ValueError('an utterance is too short for one mel frame (the reference\'s reflect padding raises there)')
        tgt = pad_targets(y_mels, idx, frames, mel_frames(max(ts) * hop_total, h.n_fft, h.hop_size))
        spk = torch.cat([spks[i] for i in idx])
        y = g(x.to(dev), spk.to(dev), nz.expand(len(idx), -1).contiguous().to(dev), lengths=ts)
        mel = mel_spectrogram(y.squeeze(1), h.n_fft, h.num_mels, h.sampling_rate, h.hop_size, h.win_size, h.fmin, h.fmax_for_loss,
                              lengths=ts, len_mul=hop_total)
        _total, per_item = mel_l1(mel, tgt.to(dev), ts, hop_total, n_fft=h.n_fft, hop_size=h.hop_size)
        out[torch.tensor(idx, device=dev)] = per_item
    return out.cpu()
