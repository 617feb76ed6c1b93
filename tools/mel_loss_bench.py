#!/usr/bin/env python
"""Times the mel L1 training loss, forward + backward, at B = 32 x 81 920 (a training batch) for 1024 / 256 / 1024 with 80 mels:
  (a) mel.mel_loss without lengths (the L1 fused into the mel's last kernel);
  (b) the composition it replaces, F.l1_loss(y_mel, mel_spectrogram(y).permute(0, 2, 1)), in the same run on the same GPU;
  (c) mel.mel_loss with lengths uniform in [64, 256] frames of 320 samples (seed 0, as tools/ragged_bench.py draws them).

Device events around every iteration, warm-up first, the median reported; the three are timed in turn, twice (a b c a b c), and both
passes are printed so that a drift of the clock shows.  Prints one JSON line.  Needs the GPU: nothing here falls back."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from wavthruvec_pytorch_amd import mel_loss  # noqa: E402
from wavthruvec_pytorch_amd.mel import mel_frames, mel_spectrogram  # noqa: E402

CFG = (1024, 80, 16000, 256, 1024, 0, None)
B, T, HOP_TOTAL = 32, 256, 320


def median_ms(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return statistics.median(times)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--iters', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    args = ap.parse_args()
    if args.iters < 20 or args.warmup < 5:
        sys.exit('mel_loss_bench: at least 20 timed iterations after 5 warm-ups')
    if not torch.cuda.is_available():
        sys.exit('mel_loss_bench: needs a GPU')
    dev = torch.device('cuda:0')
    L = T * HOP_TOTAL
    F = mel_frames(L, CFG[0], CFG[3])
    g = torch.Generator(device=dev).manual_seed(0)
    y = (torch.rand((B, L), device=dev, generator=g) - 0.5).requires_grad_(True)
    y_mel = torch.randn((B, F, CFG[1]), device=dev, generator=g) * 2 - 5             # the range of log-mels, frames first as train.py's
    ns = torch.randint(64, T + 1, (B,), generator=torch.Generator().manual_seed(0)).tolist()
    lens = torch.tensor(ns, dtype=torch.int32, device=dev)

    def fused():
        y.grad = None
        mel_loss(y, y_mel, *CFG).backward()

    def composed():
        y.grad = None
        torch.nn.functional.l1_loss(y_mel, mel_spectrogram(y, *CFG).permute(0, 2, 1)).backward()

    def ragged():
        y.grad = None
        mel_loss(y, y_mel, *CFG, lengths=lens, len_mul=HOP_TOTAL).backward()

    out = dict(workload=f'mel L1 loss forward + backward, B={B} x {L}, 1024/256/1024, 80 mels; lengths uniform in [64, {T}] frames (seed 0), '
                        f'mean fill {sum(ns) / (B * T):.3f}', gpu=torch.cuda.get_device_name(dev), iters=args.iters, warmup=args.warmup)
    passes = []
    for _ in range(2):
        passes.append({name: round(median_ms(fn, args.warmup, args.iters), 4)
                       for name, fn in (('a_mel_loss_ms', fused), ('b_l1_of_mel_spectrogram_ms', composed), ('c_mel_loss_lengths_ms', ragged))})
    out['passes'] = passes
    for k in passes[0]:
        out[k] = min(p[k] for p in passes)
    fused()
    a = y.grad.clone()
    composed()
    with torch.no_grad():
        out['loss'] = [mel_loss(y, y_mel, *CFG).item(), torch.nn.functional.l1_loss(y_mel, mel_spectrogram(y, *CFG).permute(0, 2, 1)).item()]
        out['max_abs_grad_diff'] = (a - y.grad).abs().max().item()
    print(json.dumps(out), flush=True)


if __name__ == '__main__':
    main()
