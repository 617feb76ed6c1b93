#!/usr/bin/env python3
"""Batched synthesis of utterances of unequal length (Generator.forward(lengths=...)) at the cfg2 shape, fp32, eval mode:

    (a) the padded B = 32 x T = 256 forward without lengths,
    (b) the same batch with per-item lengths (tiles past an item's end return at once),
    (c) the 32 single-item forwards on the trimmed inputs, one after the other (the reference's validation loop, train.py:246-291).

Lengths: 32 draws uniform in [64, 256] frames (fixed seed).  Reports ms per forward (median of --steps timed forwards after --warmup, three
runs each) and valid-audio samples/s (sum of n_b * 320 over the median time).  One JSON line.

    python tools/ragged_bench.py [--steps 20] [--warmup 3] [--runs 3]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from wavthruvec_pytorch_amd import Generator, synthetic  # noqa: E402


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--runs', type=int, default=3)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    B, T = 32, 256
    h = synthetic.make_hparams(num_wv_feat=768)
    H = synthetic.total_upsample(h)
    g = Generator(h)
    g.load_state_dict(synthetic.make_state_dict(h, seed=0))
    g = g.to(dev).eval()
    x, spk, nz = (t.to(dev) for t in synthetic.make_inputs(h, B, T, seed=1234))
    ns = torch.randint(64, T + 1, (B,), generator=torch.Generator().manual_seed(0)).tolist()
    singles = [(x[b:b + 1, :, :n].contiguous(), spk[b:b + 1].contiguous(), nz[b:b + 1].contiguous()) for b, n in enumerate(ns)]
    valid = sum(ns) * H

    def padded():
        g(x, spk, nz)

    def ragged():
        g(x, spk, nz, lengths=ns)

    def single():
        for xb, sb, nb in singles:
            g(xb, sb, nb)

    out = dict(workload=f'cfg2 f32 eval, B={B} x T={T}, lengths uniform in [64, {T}] (seed 0), mean fill {sum(ns) / (B * T):.3f}',
               lengths=ns, valid_samples=valid)
    with torch.no_grad():
        for name, fn in (('padded', padded), ('ragged', ragged), ('single', single)):
            ms = [timed(fn, args.steps if name != 'single' else max(3, args.steps // 4), args.warmup) for _ in range(args.runs)]
            out[name] = dict(ms=[round(v, 4) for v in ms], valid_samples_per_s=[round(valid / (v * 1e-3)) for v in ms])
    out['ragged_over_padded'] = round(statistics.median(out['ragged']['ms']) / statistics.median(out['padded']['ms']), 4)
    out['ragged_over_single'] = round(statistics.median(out['ragged']['ms']) / statistics.median(out['single']['ms']), 4)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
