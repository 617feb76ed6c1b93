#!/usr/bin/env python3
"""Batched validation (validate.mel_errors) against the reference's per-utterance loop (train.py:246-289) at the cfg2 shape, fp32, eval mode:

    (a) the loop: per utterance  g(x) -> mel_spectrogram -> F.l1_loss(...).item()  at B = 1, as the reference writes it,
    (b) validate.mel_errors with --batch utterances per forward (ragged forward, ragged mel, masked L1; one read-back at the end).

N utterances with lengths uniform in [64, 256] frames (seed 0: the set tools/ragged_bench.py uses), random target mels.  Reports wall ms per
utterance (median of --steps timed passes over the whole set after --warmup, --runs runs each, interleaved) and the largest difference
between the two sets of errors.  One JSON line.

    python tools/validate_bench.py [--n 32] [--batch 8 32] [--steps 5] [--warmup 2] [--runs 3]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from wavthruvec_pytorch_amd import Generator, synthetic, validate  # noqa: E402
from wavthruvec_pytorch_amd.mel import mel_frames, mel_spectrogram  # noqa: E402
from wavthruvec_pytorch_amd.synthesize import item_noise  # noqa: E402


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--n', type=int, default=32)
    ap.add_argument('--batch', type=int, nargs='+', default=[8, 32])
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--runs', type=int, default=3)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    T = 256
    h = synthetic.make_hparams(num_wv_feat=768)
    H = synthetic.total_upsample(h)
    g = Generator(h)
    g.load_state_dict(synthetic.make_state_dict(h, seed=0))
    g = g.to(dev).eval()
    x, spk, _nz = synthetic.make_inputs(h, args.n, T, seed=1234)
    ns = torch.randint(64, T + 1, (args.n,), generator=torch.Generator().manual_seed(0)).tolist()
    feats = [x[b:b + 1, :, :n].contiguous().to(dev) for b, n in enumerate(ns)]
    spks = [spk[b:b + 1].contiguous().to(dev) for b in range(args.n)]
    rng = np.random.default_rng(0)
    y_mels = [torch.from_numpy(rng.standard_normal((mel_frames(n * H, h.n_fft, h.hop_size) + 1, h.num_mels)).astype(np.float32) * 2 - 5)
              for n in ns]
    nz = item_noise(h.noise_dim, 1234).to(dev)
    last = {}

    def loop():
        errs = []
        with torch.no_grad():
            for f, s, m in zip(feats, spks, y_mels):
                y = g(f, s, nz)
                ym = mel_spectrogram(y.squeeze(1), h.n_fft, h.num_mels, h.sampling_rate, h.hop_size, h.win_size, h.fmin,
                                     h.fmax_for_loss).permute(0, 2, 1)
                t = m[None].to(dev, non_blocking=True)[:, :ym.shape[1], :]
                errs.append(torch.nn.functional.l1_loss(t, ym).item())
        last['loop'] = errs

    def batched(bs):
        def fn():
            last[bs] = validate.mel_errors(g, feats, spks, y_mels, h, seed=1234, batch=bs).tolist()
        return fn

    arms = [('loop', loop)] + [(f'batch{bs}', batched(bs)) for bs in args.batch]
    out = dict(workload=f'cfg2 f32 eval, {args.n} utterances, lengths uniform in [64, {T}] frames (seed 0), mean {sum(ns) / args.n:.1f}',
               lengths=ns)
    ms = {name: [] for name, _ in arms}
    for _ in range(args.runs):                          # interleaved: every arm once per run
        for name, fn in arms:
            ms[name].append(timed(fn, args.steps, args.warmup))
    for name, _ in arms:
        out[name] = dict(ms_per_pass=[round(v, 3) for v in ms[name]], ms_per_utterance=[round(v / args.n, 4) for v in ms[name]])
    for bs in args.batch:
        out[f'batch{bs}']['max_abs_diff_vs_loop'] = max(abs(a - b) for a, b in zip(last[bs], last['loop']))
        out[f'batch{bs}']['over_loop'] = round(statistics.median(ms[f'batch{bs}']) / statistics.median(ms['loop']), 4)
    out['val_err'] = dict(loop=sum(last['loop']) / args.n, **{f'batch{bs}': sum(last[bs]) / args.n for bs in args.batch})
    print(json.dumps(out))


if __name__ == '__main__':
    main()
