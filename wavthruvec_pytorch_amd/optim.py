"""`AdamW`: torch.optim.AdamW whose step runs in the library's multi-tensor kernel (include/vec2wav_hip.h, v2w_adamw_multi): one launch per
80 parameter tensors in place of the dozen passes torch's foreach implementation makes over the lists.

It is a subclass that overrides `step()` only, so the state layout (`step`: a CPU scalar tensor; `exp_avg`, `exp_avg_sq`: zeros_like(p),
created at the first step), `state_dict()` / `load_state_dict()`, `param_groups`, `zero_grad()` and the schedulers that rewrite
`group['lr']` (ExponentialLR, train.py:104-105) are torch's own: the `optim_g` / `optim_d` of a checkpoint load into either class."""
from __future__ import annotations

import torch

from . import hipops

__all__ = ['AdamW']

_UNSERVED = ('amsgrad', 'maximize', 'capturable', 'differentiable')


class AdamW(torch.optim.AdamW):
    """torch.optim.AdamW(params, lr, betas, eps, weight_decay) as the reference constructs it (train.py:96-99).  Parameter groups on a GPU
    are stepped by hipops.adamw_multi (one call per group); a group on another device is handed to torch's implementation unchanged.
    amsgrad, maximize, capturable, differentiable, sparse gradients and non-fp32 parameters raise ValueError: the kernel has no form of
    them and there is no quiet fall-back."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, **kw):
        for name in _UNSERVED:
            if kw.get(name):
                raise ValueError(f'wavthruvec_pytorch_amd.optim.AdamW does not serve {name}=True (use torch.optim.AdamW)')
        if isinstance(lr, torch.Tensor):
            raise ValueError('wavthruvec_pytorch_amd.optim.AdamW takes a Python float lr: the kernel never reads a device scalar')
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, **kw)
        for group in self.param_groups:
            for p in group['params']:
                if p.is_cuda and p.dtype != torch.float32:
                    raise ValueError(f'wavthruvec_pytorch_amd.optim.AdamW steps fp32 parameters on the GPU, got {p.dtype}')

    @staticmethod
    def _on_gpu(group):
        cuda = [p.is_cuda for p in group['params']]
        if any(cuda) and not all(cuda):
            raise ValueError('a parameter group must live on one kind of device')
        return bool(cuda) and cuda[0]

    def _hip_group(self, group):
        for name in _UNSERVED:                      # a loaded state dict can bring them back
            if group.get(name):
                raise ValueError(f'wavthruvec_pytorch_amd.optim.AdamW does not serve {name}=True')
        by_dev = {}
        for p in group['params']:
            if p.grad is None:
                continue
            g = p.grad
            if g.is_sparse:
                raise ValueError('wavthruvec_pytorch_amd.optim.AdamW does not serve sparse gradients')
            if p.dtype != torch.float32 or g.dtype != torch.float32:
                raise ValueError(f'wavthruvec_pytorch_amd.optim.AdamW steps fp32 parameters and gradients, got {p.dtype} / {g.dtype}')
            st = self.state[p]
            if len(st) == 0:
                st['step'] = torch.tensor(0.0, dtype=torch.get_default_dtype())
                st['exp_avg'] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st['exp_avg_sq'] = torch.zeros_like(p, memory_format=torch.preserve_format)
            elif not torch.is_tensor(st['step']):   # a state dict written by torch < 1.12 holds a Python int
                st['step'] = torch.tensor(float(st['step']), dtype=torch.get_default_dtype())
            by_dev.setdefault((p.device, int(st['step'].item()) + 1), []).append((p, g, st))
        for (_dev, t), rows in by_dev.items():      # one call per group (parameters that joined later carry another step count)
            ps = [r[0] for r in rows]
            hipops.adamw_multi(ps, [r[1] for r in rows], [r[2]['exp_avg'] for r in rows], [r[2]['exp_avg_sq'] for r in rows],
                               lr=group['lr'], betas=group['betas'], eps=group['eps'], weight_decay=group['weight_decay'], step=t)
            torch._foreach_add_([r[2]['step'] for r in rows], 1)
            # the kernel wrote through the raw pointers: the caches of folded / packed weights are keyed on the version counters
            torch.autograd.graph.increment_version(ps)

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        groups = self.param_groups
        mine = [self._on_gpu(g) for g in groups]
        # torch's own step WITHOUT the hook wrapper Optimizer.__init__ puts around a class's step: this method already runs inside one
        torch_step = getattr(torch.optim.AdamW.step, '__wrapped__', torch.optim.AdamW.step)
        if not any(mine):
            torch_step(self)
            return loss
        for g in (g for g, hip in zip(groups, mine) if hip):
            self._hip_group(g)
        rest = [g for g, hip in zip(groups, mine) if not hip]
        if rest:
            # torch's implementation walks self.param_groups: show it the other groups only (same dict objects, nothing is copied)
            self.param_groups = rest
            try:
                torch_step(self)
            finally:
                self.param_groups = groups
        return loss
