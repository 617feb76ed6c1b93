#!/usr/bin/env python
"""Times audio.resample (one launch of resample_kernel, csrc/v2w_resample.hip) against the dense form of the same filter with stock torch ops on
the same GPU - torchaudio.functional.resample's formulation: one F.conv1d with stride M, L output channels and 2 * width + M taps, then a
transpose - at 44100 -> 16000 (B = 32 x 10 s; int16 and float32 input) and 16000 -> 48000 (B = 32 x 81 920).

Device events around every call, warm-up first, `--reps` repetitions of `--iters` calls each: the median over all calls and the range of the
repetitions' medians are reported.  GB/s is against the bytes the kernel must move: input + output + table.  The two forms' outputs are compared at
the timed size (max |difference|; the dense form adds its 475 products in another order).  Prints one JSON line per case.  Needs the GPU: nothing
here falls back."""
import argparse
import json
import math
import os
import statistics
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from wavthruvec_pytorch_amd import audio  # noqa: E402

CASES = (('44100->16000 int16', 44100, 16000, 32, 441000, torch.int16), ('44100->16000 float32', 44100, 16000, 32, 441000, torch.float32),
         ('16000->48000 float32', 16000, 48000, 32, 81920, torch.float32))


def dense_weights(orig, new, device, lpw=6, rolloff=0.99):
    """(L, 1, 2 * width + M) float32 and width: the strided-conv kernel of the same filter, zeros where the polyphase run has no tap."""
    t = audio.resample_table(orig, new, lpw, rolloff)
    M, L, NT = t['M'], t['L'], t['NT']
    width = int(math.ceil(lpw * M / (min(M, L) * rolloff)))
    w = np.zeros((L, 2 * width + M))
    for p in range(L):
        a = int(t['k0'][p]) + width
        w[p, a:a + NT] = t['h'][p][:max(0, min(NT, w.shape[1] - a))]
    return torch.from_numpy(w.astype(np.float32))[:, None, :].to(device), width, M, L


def dense_resample(x, w, width, M, L, N):
    y = F.conv1d(F.pad(x, (width, width + M))[:, None], w, stride=M)             # (B, L, Q)
    return y.transpose(1, 2).reshape(x.shape[0], -1)[:, :N].contiguous()


def times_ms(fn, warmup, iters, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    meds, every = [], []
    for _ in range(reps):
        ts = []
        for _ in range(iters):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ts.append(a.elapsed_time(b))
        meds.append(statistics.median(ts))
        every += ts
    return dict(median_ms=round(statistics.median(every), 4), rep_medians_ms=[round(min(meds), 4), round(max(meds), 4)], min_ms=round(min(every), 4))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('resample_bench: needs a GPU')
    dev = torch.device('cuda:0')
    for name, orig, new, B, n, dtype in CASES:
        g = torch.Generator(device=dev).manual_seed(n)
        xf = torch.rand((B, n), device=dev, generator=g) - 0.5
        x = (xf * 32768.0).round().clamp(-32768, 32767).to(torch.int16) if dtype == torch.int16 else xf
        xd = x.float() / 32768.0 if dtype == torch.int16 else x                 # the dense form's input (its conversion is not timed)
        N = audio.resampled_length(n, orig, new)
        w, width, M, L = dense_weights(orig, new, dev)
        c = audio._constants(orig, new, 6, 0.99, dev)
        moved = x.numel() * x.element_size() + B * N * 4 + c['h'].numel() * 4 + c['k0'].numel() * 4
        out = dict(case=name, B=B, n=n, N=N, M=M, L=L, NT=c['NT'], dense_taps=w.shape[-1], iters=args.iters, reps=args.reps, bytes=moved)
        hip = times_ms(lambda: audio.resample(x, orig, new), args.warmup, args.iters, args.reps)
        hip_peak = times_ms(lambda: audio.resample(x, orig, new, peak=0.95), args.warmup, args.iters, args.reps)
        dense = times_ms(lambda: dense_resample(xd, w, width, M, L, N), args.warmup, args.iters, args.reps)
        hip['GBps'] = round(moved / hip['median_ms'] / 1e6, 1)
        out.update(hip=hip, hip_with_peak=hip_peak, dense_conv1d=dense, speedup=round(dense['median_ms'] / hip['median_ms'], 2))
        a, b = audio.resample(x, orig, new), dense_resample(xd, w, width, M, L, N)
        out['max_abs_diff'] = float((a - b).abs().max())
        print(json.dumps(out), flush=True)


if __name__ == '__main__':
    main()
