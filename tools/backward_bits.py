#!/usr/bin/env python3
"""What the generator's backward computes and launches, as a JSON to compare between two commits: per case the sha256 of
every gradient after an ordinary `loss.backward()`, and the kernel names of one `generator_backward` - called directly on this thread under a
schedule.NameProbe, since the recorder of `_hip.set_recorder` is thread-local and autograd's backward thread does not see it.
argv: the output file."""
import hashlib
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from wavthruvec_pytorch_amd import Generator, _hip, schedule, synthetic  # noqa: E402
from wavthruvec_pytorch_amd.backward import generator_backward  # noqa: E402
from wavthruvec_pytorch_amd.models import ResBlock1, ResBlock2  # noqa: E402

DEV = torch.device('cuda:0')
WIDE_HALO = dict(resblock_dilation_sizes=[[1, 3, 5], [1, 3, 5], [1, 7, 5]])          # no tile configuration: per-branch ResBlock2 path
ONE_KERNEL_SIZE = dict(resblock_kernel_sizes=[7], resblock_dilation_sizes=[[1, 3, 5]])
SIX_STAGES = dict(upsample_rates=[5, 4, 4, 2, 2, 2], upsample_kernel_sizes=[11, 8, 8, 4, 4, 4])
# name: (hparams overrides, B, T, module switches; 'calibrated' / 'x_grad' / 'frozen' are read here, the rest are set on the Generator)
CASES = {
    'rb2_f32_b2_t8': ({}, 2, 8, {}),
    'rb2_f32_b3_t21': ({}, 3, 21, {}),
    'rb2_f32_eval_b2_t8': ({}, 2, 8, dict(calibrated=True)),
    'rb2_one_kernel_b2_t20': ({}, 2, 20, dict(fuse_stage_backward=True)),
    'rb1_f32_b2_t9': (dict(resblock='1'), 2, 9, {}),
    'rb2_wide_halo_b2_t8': (WIDE_HALO, 2, 8, {}),
    'rb2_nk1_b2_t8': (ONE_KERNEL_SIZE, 2, 8, {}),
    'rb2_f16x3_b2_t12': ({}, 2, 12, dict(precision='f16x3')),
    'rb2_bf16_b2_t16': ({}, 2, 16, dict(precision='bf16')),
    'rb1_bf16_b2_t16': (dict(resblock='1'), 2, 16, dict(precision='bf16')),
    'rb2_six_stages_b2_t9': (SIX_STAGES, 2, 9, {}),
    'rb2_x_grad_b2_t12': ({}, 2, 12, dict(x_grad=True)),
    'rb2_x_grad_frozen_b2_t12': ({}, 2, 12, dict(x_grad=True, frozen=True)),
}


def sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def generator_case(over, B, T, sw):
    sw = dict(sw)
    h = synthetic.make_hparams(num_wv_feat=768, **over)
    g = Generator(h)
    g.load_state_dict(synthetic.make_state_dict(h, seed=0))
    g = g.to(DEV).train()
    x, spk, nz = synthetic.make_inputs(h, B, T, seed=21, device=DEV)
    if sw.pop('calibrated', False):        # running statistics := this batch's (momentum 1, one train-mode forward), then eval mode
        for c in g.cbns:
            c.batch_nrom.momentum = 1.0
        with torch.no_grad():
            g(x, spk, nz)
        g.eval()
    x_grad, frozen = sw.pop('x_grad', False), sw.pop('frozen', False)
    for k, v in sw.items():
        setattr(g, k, v)
    g.requires_grad_(not frozen)
    x.requires_grad_(x_grad)
    dy = torch.from_numpy(np.random.default_rng(5).standard_normal((B, 1, T * synthetic.total_upsample(h))).astype(np.float32)).to(DEV)
    (g(x, spk, nz) * dy).sum().backward()
    hashes = {n: sha(t.grad) for n, t in [*g.named_parameters(), ('__x__', x)] if t.grad is not None}
    # the kernel names: a second forward that keeps what the backward reads, then the backward itself on this thread
    save, names = {}, []
    with torch.no_grad():
        g._forward_hip(x.detach(), spk, nz, save)
    prev = _hip.set_recorder(schedule.NameProbe(_hip.load(), names))
    generator_backward(g, save, dy, need_dx=x_grad)
    _hip.set_recorder(prev)
    return dict(hashes=hashes, kernels=names)


def resblock_case(cls, dil):
    """A stand-alone block, C 32, L 500, k 7: both forwards, input and parameter gradients (autograd drives ResBlockFunction: no kernel names)."""
    rng = np.random.default_rng(5)
    torch.manual_seed(0)
    rb = cls(synthetic.make_hparams(), 32, 7, dil).to(DEV)
    x, dy = (torch.from_numpy(rng.standard_normal((2, 32, 500)).astype(np.float32)).to(DEV) for _ in range(2))
    with torch.no_grad():
        hashes = dict(__out_no_grad__=sha(rb(x)))
    out = rb(x.requires_grad_(True))
    (out * dy).sum().backward()
    hashes.update({n: sha(t.grad) for n, t in [*rb.named_parameters(), ('__x__', x)]}, __out__=sha(out))
    return dict(hashes=hashes, kernels=[])


def main():
    res = {}
    runs = [(n, generator_case, c) for n, c in CASES.items()]
    runs += [('standalone_rb1', resblock_case, (ResBlock1, (1, 3, 5))), ('standalone_rb2', resblock_case, (ResBlock2, (1, 3)))]
    for name, fn, args in runs:
        res[name] = fn(*args)
        print(name, len(res[name]['hashes']), 'gradients,', len(res[name]['kernels']), 'kernels', flush=True)
        with open(sys.argv[1], 'w') as f:       # (after every case: a case that raises leaves the ones before it on disk)
            json.dump(res, f, indent=1, sort_keys=True)


if __name__ == '__main__':
    main()
