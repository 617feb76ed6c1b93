#!/usr/bin/env python3
"""Forward + backward of the three GAN losses with and without `lengths=`, at the GAN benchmark's shape, on the real MPD / MSD maps.

    python tools/gan_loss_len_bench.py [--batch 32] [--samples 81920] [--iters 20] [--warmup 5]

The batch is B x samples of random audio; lengths are uniform in [64, 256] frames x 320 samples (seed 0), the generated batch goes through
`mask_tail`.  The discriminators run once; their maps are detached (the generated ones made leaves), so that a timed iteration is exactly
feature_loss + generator_loss + discriminator_loss and the gradients with respect to the generated maps and scores - the loss kernels'
forwards and backwards and torch's few scalar ops around them.  Dense and ragged iterations alternate in the same run; each is timed with
device events after a warm-up; the line printed last is one JSON record with the medians, the minima and the fill.
"""
import argparse
import json
import statistics
import sys
from pathlib import Path
from types import SimpleNamespace

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--samples', type=int, default=81920)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    a = ap.parse_args()
    from wavthruvec_pytorch_amd import discriminators as D
    from wavthruvec_pytorch_amd import mask_tail, synthetic
    dev = torch.device('cuda:0')
    g = torch.Generator().manual_seed(0)
    frames = torch.randint(64, 257, (a.batch,), generator=g)
    frames = frames.clamp(max=a.samples // 320)
    fill = float(frames.sum()) * 320 / (a.batch * a.samples)
    lens = frames.to(dev)
    mpd = D.MultiPeriodDiscriminator(SimpleNamespace(periods=synthetic.DEFAULT_PERIODS))
    mpd.load_state_dict(synthetic.make_disc_state_dict(synthetic.mpd_state_dict_spec(), seed=3))
    msd = D.MultiScaleDiscriminator()
    msd.load_state_dict(synthetic.make_disc_state_dict(synthetic.msd_state_dict_spec(), seed=3))
    y, y_hat = synthetic.make_audio_pair(a.batch, a.samples, seed=4)
    y, y_hat = mask_tail(y.to(dev), lens, 320), mask_tail(y_hat.to(dev), lens, 320)
    sets = []
    with torch.no_grad():
        for m in (mpd, msd):
            m = m.to(dev).train()
            y_r, y_g, f_r, f_g = m(y, y_hat)
            f_g = [[f.requires_grad_() for f in maps] for maps in f_g]
            y_g = [s.clone().requires_grad_() for s in y_g]
            sets.append((y_r, y_g, f_r, f_g, m.map_lengths(lens, 320, L=a.samples)))
    leaves = [t for _r, y_g, _f, f_g, _ml in sets for t in y_g + [f for maps in f_g for f in maps]]
    floats = sum(t.numel() for t in leaves)

    def step(ragged):
        loss = 0
        for y_r, y_g, f_r, f_g, ml in sets:
            ml = ml if ragged else None
            loss = loss + D.feature_loss(f_r, f_g, lengths=ml) + D.generator_loss(y_g, lengths=ml)[0]
            loss = loss + _disc_total(D, y_r, y_g, ml)
        torch.autograd.grad(loss, leaves)
        return loss

    times = {False: [], True: []}
    for it in range(a.warmup + a.iters):
        for ragged in (False, True):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            loss = step(ragged)
            t1.record()
            t1.synchronize()
            if it >= a.warmup:
                times[ragged].append(t0.elapsed_time(t1))
    rec = dict(bench='gan_loss_len', batch=a.batch, samples=a.samples, fill=round(fill, 4), generated_floats=floats, iters=a.iters,
               dense_ms_median=round(statistics.median(times[False]), 4), dense_ms_min=round(min(times[False]), 4),
               ragged_ms_median=round(statistics.median(times[True]), 4), ragged_ms_min=round(min(times[True]), 4),
               last_loss=float(loss.detach()))
    rec['ragged_over_dense'] = round(rec['ragged_ms_median'] / rec['dense_ms_median'], 4)
    print(json.dumps(rec))


def _disc_total(D, y_r, y_g, ml):
    """discriminator_loss's total without its device-to-host copy of the terms (the copy would serialise the timed region): the same
    autograd call on the same kernels."""
    nr = len(y_r)
    return D._lsgan(list(y_r) + list(y_g), (1.0,) * nr + (0.0,) * nr, None if ml is None else ml.scores_twice)[0]


if __name__ == '__main__':
    main()
