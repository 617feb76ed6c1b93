#!/usr/bin/env python3
"""vec2wav inference entry: text2vec latents + speaker embedding -> 16 kHz waveform on the MI355X HIP path.

The reference has no such script: `text2vec/eval.py:121-122` writes `*_feat_postnet.npy` of shape
(1, T, n_feat_dim) and the only Generator inference code is the validation loop of `vec2wav/train.py:246-291`.
This closes the text2vec -> vec2wav hand-off with the reference's own wire formats:

  generator checkpoint   `g_%08d` = torch.save({'generator': state_dict})          vec2wav/train.py:228-230, utils.py:39-58
  latents                `.npy` (1, T, C) or (T, C) float32                        text2vec/eval.py:121-122, prepare_data.py
  speaker embedding      `{spk}.pth` tensor (1, 1, 192) -> squeezed to (1, 192)    vec2wav/pre_spk_emb.py, dataset.py:181-185
  noise                  randn(1, noise_dim)                                       vec2wav/train.py:256

    python -m wavthruvec_pytorch_amd.synthesize --checkpoint run/g_00100000 --feat a_feat_postnet.npy \
        --spk-emb SSB0005.pth --out a.wav [--num-wv-feat 768] [--remove-weight-norm] [--seed 1234]

Several utterances: `--feat a.npy b.npy c.npy --spk-emb s.pth --out wavs/ --batch 8` writes wavs/a.wav, wavs/b.wav, wavs/c.wav (`--out` is a
directory; one `--spk-emb` for all files or one per file).  `--batch N` puts up to N utterances, sorted by length, into one padded forward
with per-item lengths (Generator.forward(lengths=...), precision 'f32'); every file gets the samples - and the noise - of its own single run.

`--sampling-rate` is the MODEL's rate (what the generator was trained at; it goes into the wav header).  `--out-rate R` delivers the audio at
R Hz instead: every utterance is resampled on the GPU from `--sampling-rate` to R (audio.resample, the whole ragged batch in one call) and the
header carries R.  Without it nothing changes.
"""
from __future__ import annotations

import argparse
import os
import wave
from typing import List, Sequence

import numpy as np
import torch

from . import synthetic
from .models import Generator
from .utils import load_checkpoint, scan_checkpoint


def load_latents(path: str) -> torch.Tensor:
    """`.npy` (1, T, C) / (T, C) -> channels-first (1, C, T) float32 (the permute of dataset.py:212-213)."""
    a = np.load(path)
    if a.ndim == 2:
        a = a[None]
    if a.ndim != 3 or a.shape[0] != 1:
        raise ValueError(f'{path}: expected latents of shape (1, T, C) or (T, C), got {a.shape}')
    return torch.from_numpy(np.ascontiguousarray(a.astype(np.float32))).permute(0, 2, 1).contiguous()


def load_speaker_embedding(path: str) -> torch.Tensor:
    """`{spk}.pth` saved as (1, 1, 192) (pre_spk_emb.py) -> (1, 192) float32."""
    t = torch.load(path, map_location='cpu')
    t = torch.as_tensor(t, dtype=torch.float32)
    return t.reshape(1, -1).contiguous()


def write_wav(path: str, audio: torch.Tensor, sampling_rate: int) -> None:
    """(1, 1, N) float in [-1, 1] -> 16-bit PCM mono wav (what train.py's SummaryWriter.add_audio consumers expect)."""
    pcm = (audio.detach().reshape(-1).clamp(-1.0, 1.0).cpu().numpy() * 32767.0).round().astype('<i2')
    with wave.open(path, 'wb') as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(sampling_rate)
        w.writeframes(pcm.tobytes())


def build_generator(checkpoint: str, h, device, remove_weight_norm: bool = False) -> Generator:
    """`checkpoint` is a `g_%08d` file or a directory holding them (newest is taken, utils.py:53-58)."""
    path = checkpoint
    if os.path.isdir(checkpoint):
        path = scan_checkpoint(checkpoint, 'g_')
        if path is None:
            raise FileNotFoundError(f'no g_???????? checkpoint in {checkpoint}')
    sd = load_checkpoint(path, 'cpu')['generator']
    g = Generator(h)
    g.load_state_dict(sd)
    g = g.to(device).eval()
    if remove_weight_norm:
        g.remove_weight_norm()      # folded weights are cached in eval mode either way; this mirrors the HiFi-GAN idiom
    return g


@torch.no_grad()
def synthesize(g: Generator, feat: torch.Tensor, spk_emb: torch.Tensor, seed: int = 1234, noise=None) -> torch.Tensor:
    dev = next(g.parameters()).device
    if noise is None:
        gen = torch.Generator(device='cpu').manual_seed(seed)
        noise = torch.randn(feat.shape[0], g.h.noise_dim, generator=gen)
    return g(feat.to(dev), spk_emb.to(dev), noise.to(dev))


def item_noise(noise_dim: int, seed: int) -> torch.Tensor:
    """(1, noise_dim): the noise a single run of one file with this seed draws (`synthesize`)."""
    gen = torch.Generator(device='cpu').manual_seed(seed)
    return torch.randn(1, noise_dim, generator=gen)


def plan_batches(lengths: Sequence[int], batch: int) -> List[List[int]]:
    """Indices of the items of each forward: longest first (ties in input order), at most `batch` per forward - neighbours in length share a
    batch, which keeps the padding small."""
    if batch < 1:
        raise ValueError('--batch must be >= 1')
    order = sorted(range(len(lengths)), key=lambda i: (-int(lengths[i]), i))
    return [order[i:i + batch] for i in range(0, len(order), batch)]


def pad_batch(feats: Sequence[torch.Tensor], idx: Sequence[int]):
    """(1, C, T_i) latents of the items `idx` -> ((n, C, max T_i) zero-padded, [T_i])."""
    ts = [feats[i].shape[-1] for i in idx]
    x = feats[idx[0]].new_zeros((len(idx), feats[idx[0]].shape[1], max(ts)))
    for j, i in enumerate(idx):
        x[j, :, :ts[j]] = feats[i][0]
    return x, ts


@torch.no_grad()
def synthesize_many(g: Generator, feats: Sequence[torch.Tensor], spks: Sequence[torch.Tensor], seed: int = 1234, batch: int = 1) -> List[torch.Tensor]:
    """One (1, 1, T_i * prod(upsample_rates)) waveform per (1, C, T_i) latent, in input order: up to `batch` items per forward (per-item
    lengths; a forward of one item is the plain single run).  spks: one (1, spk_dim) embedding per item."""
    dev = next(g.parameters()).device
    hop = 1
    for u in g.h.upsample_rates:
        hop *= u
    nz = item_noise(g.h.noise_dim, seed)
    out: List[torch.Tensor] = [None] * len(feats)
    for idx in plan_batches([f.shape[-1] for f in feats], batch):
        if len(idx) == 1:
            out[idx[0]] = synthesize(g, feats[idx[0]], spks[idx[0]], noise=nz)
            continue
        x, ts = pad_batch(feats, idx)
        spk = torch.cat([spks[i] for i in idx])
        y = g(x.to(dev), spk.to(dev), nz.expand(len(idx), -1).contiguous().to(dev), lengths=ts)
        for j, i in enumerate(idx):
            out[i] = y[j:j + 1, :, :ts[j] * hop]
    return out


@torch.no_grad()
def resample_many(ys: Sequence[torch.Tensor], sampling_rate: int, out_rate: int) -> List[torch.Tensor]:
    """(1, 1, N_i) waveforms at `sampling_rate` -> (1, 1, ceil(N_i * out_rate / sampling_rate)) at `out_rate`: one zero-padded batch with
    per-item lengths through one audio.resample call."""
    from . import audio
    ns = [int(y.shape[-1]) for y in ys]
    batch = ys[0].new_zeros((len(ys), max(ns)))
    for i, y in enumerate(ys):
        batch[i, :ns[i]] = y.reshape(-1)
    out = audio.resample(batch, sampling_rate, out_rate, lengths=ns)
    return [out[i:i + 1, :audio.resampled_length(n, sampling_rate, out_rate)].unsqueeze(0) for i, n in enumerate(ns)]


def output_paths(feats: Sequence[str], out: str) -> List[str]:
    """`--out` is the .wav of a single `--feat`, else a directory that receives <feat name without .npy>.wav per file."""
    if len(feats) == 1:
        return [out]
    names = [os.path.splitext(os.path.basename(f))[0] + '.wav' for f in feats]
    if len(set(names)) != len(names):
        raise ValueError('--feat: several files share a name; their .wav files would collide in --out')
    return [os.path.join(out, n) for n in names]


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--checkpoint', required=True, help='g_%%08d file or directory')
    ap.add_argument('--feat', required=True, nargs='+', help='text2vec *_feat_postnet.npy (1, T, C), one or more')
    ap.add_argument('--spk-emb', required=True, nargs='+', help='{spk}.pth (1, 1, 192): one for all files or one per file')
    ap.add_argument('--out', required=True, help='output .wav (one --feat) or directory (several)')
    ap.add_argument('--batch', type=int, default=1, help='most utterances per forward (per-item lengths, precision f32); default 1')
    ap.add_argument('--num-wv-feat', type=int, default=None, help='latent width (default: taken from the .npy)')
    ap.add_argument('--resblock', default=1, help="'1' selects ResBlock1 (string!), anything else ResBlock2 (reference default)")
    ap.add_argument('--sampling-rate', type=int, default=16000,
                    help="the MODEL's sampling rate (the generator is a 16 kHz model); written into the wav header unless --out-rate is given")
    ap.add_argument('--out-rate', type=int, default=None,
                    help='resample every utterance on the GPU from --sampling-rate to this rate and write it into the wav header (default: '
                         'absent, the audio is written at the model rate)')
    ap.add_argument('--remove-weight-norm', action='store_true')
    ap.add_argument('--seed', type=int, default=1234)
    ap.add_argument('--device', default='cuda:0')
    ap.add_argument('--precision', default='f32', choices=['f32', 'f16x3', 'bf16'],
                    help="Generator.precision: exact fp32 (default), split-f16 (fp32-level accuracy, faster) or bf16 operands")
    args = ap.parse_args(argv)
    if len(args.spk_emb) not in (1, len(args.feat)):
        ap.error('--spk-emb: one file for all --feat files or one per file')
    if args.batch < 1:
        ap.error('--batch must be >= 1')
    if args.out_rate is not None and args.out_rate < 1:
        ap.error('--out-rate must be >= 1')
    return args


def main(argv=None) -> int:
    args = parse_args(argv)
    feats = [load_latents(f) for f in args.feat]
    spk_files = args.spk_emb if len(args.spk_emb) == len(args.feat) else args.spk_emb * len(args.feat)
    spks = [load_speaker_embedding(s) for s in spk_files]
    resblock = '1' if str(args.resblock) == "'1'" or args.resblock == '1s' else args.resblock
    h = synthetic.make_hparams(num_wv_feat=args.num_wv_feat or feats[0].shape[1], resblock=resblock)
    g = build_generator(args.checkpoint, h, torch.device(args.device), args.remove_weight_norm)
    g.precision = args.precision
    outs = output_paths(args.feat, args.out)
    if len(outs) > 1:
        os.makedirs(args.out, exist_ok=True)
    ys = synthesize_many(g, feats, spks, seed=args.seed, batch=args.batch)
    rate = args.sampling_rate
    if args.out_rate is not None:
        ys, rate = resample_many(ys, args.sampling_rate, args.out_rate), args.out_rate
    for path, y, feat in zip(outs, ys, feats):
        write_wav(path, y, rate)
        print(f'{path}: {y.shape[-1]} samples ({y.shape[-1] / rate:.2f} s) from {feat.shape[-1]} frames')
    return 0


if __name__ == '__main__':
    raise SystemExit(main())
