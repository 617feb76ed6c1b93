#!/usr/bin/env python
"""Times the multi-resolution STFT loss (wavthruvec_pytorch_amd.stft_loss) against the same loss written with torch.stft and stock torch ops
on the same GPU: forward and forward + backward at B = 32 x 81 920 (a training batch) and B = 2 x 8 192, the three default resolutions.
At B = 32 x 81 920 also the ragged call on the same padded batch: lengths uniform in [64, 256] frames of 320 samples (seed 0, the draw of
tools/mel_loss_bench.py), `lengths=` / `len_mul=320`, forward and forward + backward, and - for the spread of the run - the dense and the
ragged forward + backward measured in turn three more times (`dense_vs_ragged_fwd_bwd_ms`).

Device events around every iteration, warm-up first, the median reported.  For the two streaming kernels (the forward's sums launch with its
finishing launch, and the backward's d spec launch) it also prints the achieved bytes/s against their algorithmic bytes: the forward reads
Re and Im of both signals once (2 * B * 2 nb * F * 4 bytes per resolution), the backward reads the same and writes B * Cs * FP * 4.
Prints one JSON line per shape.  Needs the GPU: nothing here falls back."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from wavthruvec_pytorch_amd import MultiResolutionSTFTLoss, _hip, stft_loss  # noqa: E402

SHAPES = ((32, 81920), (2, 8192))
RAGGED = (32, 81920)                      # the shape that also gets the ragged line
HOP_TOTAL, T_MIN, T_MAX = 320, 64, 256    # samples per frame of the lengths (the generator's upsampling), frames per item


def torch_loss(x, y, resolutions, windows):
    """The same loss (the project's framing: reflect padding of (n_fft - hop) / 2, center=False) in stock torch ops."""
    sc = mag = 0.0
    for (n_fft, hop, win), w in zip(resolutions, windows):
        pad = int((n_fft - hop) / 2)
        m = []
        for s in (x, y):
            sp = torch.stft(torch.nn.functional.pad(s.unsqueeze(1), (pad, pad), mode='reflect').squeeze(1), n_fft, hop_length=hop,
                            win_length=win, window=w, center=False, return_complex=True)
            m.append(torch.sqrt(sp.real.pow(2) + sp.imag.pow(2) + 1e-9))
        X, Y = m
        sc = sc + torch.linalg.vector_norm(Y - X) / torch.linalg.vector_norm(Y)
        mag = mag + (torch.log(Y) - torch.log(X)).abs().mean()
    return sc / len(resolutions), mag / len(resolutions)


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
    if not torch.cuda.is_available():
        sys.exit('stft_loss_bench: needs a GPU')
    dev = torch.device('cuda:0')
    res = stft_loss.DEFAULT_RESOLUTIONS
    mod = MultiResolutionSTFTLoss(res)
    windows = [torch.hann_window(w, device=dev) for _n, _h, w in res]
    lib = _hip.load()
    for B, L in SHAPES:
        g = torch.Generator(device=dev).manual_seed(B)
        x = torch.rand((B, L), device=dev, generator=g) - 0.5
        y = torch.rand((B, L), device=dev, generator=g) - 0.5
        xg = x.clone().requires_grad_(True)

        def hip_fwd():
            with torch.no_grad():
                return mod(x, y)

        def hip_both():
            xg.grad = None
            sc, mag = mod(xg, y)
            (sc + mag).backward()

        def torch_fwd():
            with torch.no_grad():
                return torch_loss(x, y, res, windows)

        def torch_both():
            xg.grad = None
            sc, mag = torch_loss(xg, y, res, windows)
            (sc + mag).backward()

        out = dict(B=B, L=L, resolutions=res, iters=args.iters)
        for name, fn in (('hip_fwd_ms', hip_fwd), ('torch_fwd_ms', torch_fwd), ('hip_fwd_bwd_ms', hip_both), ('torch_fwd_bwd_ms', torch_both)):
            out[name] = round(median_ms(fn, args.warmup, args.iters), 4)
        a, b = hip_fwd(), torch_fwd()
        out['sc'], out['mag'] = [a[0].item(), b[0].item()], [a[1].item(), b[1].item()]          # (hip, torch)

        if (B, L) == RAGGED:
            ns = torch.randint(T_MIN, T_MAX + 1, (B,), generator=torch.Generator().manual_seed(0)).tolist()
            lens = torch.tensor(ns, dtype=torch.int32, device=dev)

            def len_fwd():
                with torch.no_grad():
                    return mod(x, y, lengths=lens, len_mul=HOP_TOTAL)

            def len_both():
                xg.grad = None
                sc, mag = mod(xg, y, lengths=lens, len_mul=HOP_TOTAL)
                (sc + mag).backward()

            out['lengths'] = 'uniform in [%d, %d] frames of %d samples (seed 0): %d of %d samples valid' % (T_MIN, T_MAX, HOP_TOTAL,
                                                                                                          sum(ns) * HOP_TOTAL, B * L)
            out['hip_fwd_ms_lengths'] = round(median_ms(len_fwd, args.warmup, args.iters), 4)
            out['hip_fwd_bwd_ms_lengths'] = round(median_ms(len_both, args.warmup, args.iters), 4)
            out['dense_vs_ragged_fwd_bwd_ms'] = [[round(median_ms(fn, 2, args.iters), 4) for fn in (hip_both, len_both)] for _ in range(3)]
            c = len_fwd()
            out['sc_lengths'], out['mag_lengths'] = c[0].item(), c[1].item()

        # the streaming kernels alone, on the specs of one forward
        st = torch.cuda.current_stream(dev).cuda_stream
        total, sums, specs, geoms = stft_loss._forward(x, y, res)
        cs = [stft_loss._constants(r, dev) for r in res]
        dspecs = [torch.empty((B, c['cs'], FP), device=dev) for c, (_F, FP) in zip(cs, geoms)]
        arr = stft_loss._items(cs, specs, B, geoms, dspecs)
        n = len(res)
        scratch = torch.empty((lib.v2w_stft_loss_scratch_bytes(arr, n) // 8,), dtype=torch.float64, device=dev)
        gout = torch.ones((2,), device=dev)
        fwd_bytes = sum(2 * B * 2 * c['nb'] * F * 4 for c, (F, _FP) in zip(cs, geoms))
        bwd_bytes = fwd_bytes + sum(B * c['cs'] * FP * 4 for c, (_F, FP) in zip(cs, geoms))
        t_f = median_ms(lambda: _hip.check(lib.v2w_stft_loss_multi(arr, n, None, None, total.data_ptr(), sums.data_ptr(), scratch.data_ptr(), st),
                                           'v2w_stft_loss_multi'), args.warmup, args.iters)
        t_b = median_ms(lambda: _hip.check(lib.v2w_stft_loss_multi_bwd(arr, n, sums.data_ptr(), gout.data_ptr(), gout[1:].data_ptr(), None, None, st),
                                           'v2w_stft_loss_multi_bwd'), args.warmup, args.iters)
        out['sums_launches'] = dict(ms=round(t_f, 4), bytes=fwd_bytes, GBps=round(fwd_bytes / t_f / 1e6, 1))
        out['dspec_launch'] = dict(ms=round(t_b, 4), bytes=bwd_bytes, GBps=round(bwd_bytes / t_b / 1e6, 1))
        print(json.dumps(out), flush=True)


if __name__ == '__main__':
    main()
