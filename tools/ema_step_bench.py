#!/usr/bin/env python3
"""GPU time and launch count of one optimizer step that also keeps an exponential moving average of the weights, on the generator's
parameter list (131 tensors, 8.58 M floats, random gradients):
    plain      wavthruvec_pytorch_amd.AdamW (the step as it was)
    lerp       the same step followed by torch._foreach_lerp_(averages, parameters, 1 - decay): what a user writes without this
    fused      wavthruvec_pytorch_amd.AdamW(ema_decay=0.999): the average updated by the step's own kernel
and the three again with max_grad_norm=1000.0 (`plain+clip`, `lerp+clip`, `fused+clip`: the clipped step, no clipping takes place).
argv: [steps=30] [warmup=5] [nocount].  The variants alternate in one process; every step is enqueued behind ~10 ms of other work, so the
event pair around it sees GPU time, not the host's issue time ("queued").  Median (min - max) in µs; launches counted by
torch.profiler over one step (kernels and copies; 'nocount' leaves that out, for a run under another profiler)."""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from wavthruvec_pytorch_amd import AdamW, Generator, synthetic  # noqa: E402

DECAY = 0.999


def main():
    steps = int(sys.argv[1]) if len(sys.argv) > 1 else 30
    warmup = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    dev = torch.device('cuda:0')
    h = synthetic.make_hparams(num_wv_feat=768)
    variants = {}
    for clip in ({}, dict(max_grad_norm=1000.0)):
        for kind in ('plain', 'lerp', 'fused'):
            g = Generator(h)
            g.load_state_dict(synthetic.make_state_dict(h, seed=0))
            params = list(g.to(dev).parameters())
            gen = torch.Generator(device=dev).manual_seed(7)
            for p in params:
                p.grad = torch.randn(p.shape, device=dev, generator=gen) * 1e-2
            opt = AdamW(params, 2e-4, betas=(0.8, 0.99), **clip, **(dict(ema_decay=DECAY) if kind == 'fused' else {}))
            if kind == 'lerp':
                emas = [p.detach().clone() for p in params]
                data = [p.detach() for p in params]
                post = lambda emas=emas, data=data: torch._foreach_lerp_(emas, data, 1.0 - DECAY)      # noqa: E731
            else:
                post = lambda: None                                                                       # noqa: E731
            variants[kind + ('+clip' if clip else '')] = (lambda opt=opt, post=post: (opt.step(), post()), [])
    a = torch.randn(4096, 4096, device=dev)
    for it in range(warmup + steps):
        for name, (fn, times) in variants.items():
            for _ in range(40):                       # ~10 ms of queued work: the host runs ahead of the GPU through fn()
                a @ a
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if it >= warmup:
                times.append(e0.elapsed_time(e1) * 1e3)
    launches = {}
    for name, (fn, _t) in variants.items():
        if 'nocount' in sys.argv[3:]:
            launches[name] = 'not counted'
            continue
        try:
            with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CPU, torch.profiler.ProfilerActivity.CUDA]) as prof:
                fn()
                torch.cuda.synchronize()
            launches[name] = sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)
        except Exception as e:                        # the count is a by-product: say so and keep the times
            launches[name] = f'n/a ({type(e).__name__})'
    for name, (_fn, times) in variants.items():
        print(f'{name:10s} {statistics.median(times):8.1f} us ({min(times):.1f} - {max(times):.1f}), n={len(times)}, GPU activities per step: {launches[name]}')


if __name__ == '__main__':
    main()
