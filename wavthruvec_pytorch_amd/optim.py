"""`AdamW`: torch.optim.AdamW whose step runs in the library's multi-tensor kernel (include/vec2wav_hip.h, v2w_adamw_multi): one launch per
80 parameter tensors in place of the dozen passes torch's foreach implementation makes over the lists.

It is a subclass that overrides `step()` only, so the state layout (`step`: a CPU scalar tensor; `exp_avg`, `exp_avg_sq`: zeros_like(p),
created at the first step), `state_dict()` / `load_state_dict()`, `param_groups`, `zero_grad()` and the schedulers that rewrite
`group['lr']` (ExponentialLR, train.py:104-105) are torch's own: the `optim_g` / `optim_d` of a checkpoint load into either class.

`clip_grad_norm_`: torch.nn.utils.clip_grad_norm_ for fp32 GPU gradients and the 2-norm in one streaming launch per 80 tensors, one
finishing launch and one scaling launch per 80 tensors (v2w_grad_sumsq_multi / v2w_grad_norm_finish / v2w_scale_multi), without a host
sync.  `AdamW(max_grad_norm=..., skip_nonfinite=...)` goes one further: the step's kernel reads the clip coefficient from GPU memory, so
no gradient is rewritten at all.

`AdamW(ema_decay=...)` keeps an exponential moving average of every parameter in `state[p]['ema']`, updated by the step's own kernel
(v2w_adamw_ema_multi); `swap_ema()` exchanges weights and averages in place for validation or synthesis, `ema_state_dict` writes the
averaged checkpoint."""
from __future__ import annotations

import contextlib

import torch

from . import hipops

__all__ = ['AdamW', 'clip_grad_norm_', 'ema_state_dict']

_UNSERVED = ('amsgrad', 'maximize', 'capturable', 'differentiable')


class AdamW(torch.optim.AdamW):
    """torch.optim.AdamW(params, lr, betas, eps, weight_decay) as the reference constructs it (train.py:96-99).  Parameter groups on a GPU
    are stepped by hipops.adamw_multi (one call per group); a group on another device is handed to torch's implementation unchanged.
    amsgrad, maximize, capturable, differentiable, sparse gradients and non-fp32 parameters raise ValueError: the kernel has no form of
    them and there is no quiet fall-back.

    max_grad_norm (a float, or None): every step first computes ONE 2-norm over the gradients of all parameters of all groups - what
    clip_grad_norm_(all parameters, max_grad_norm) computes - and steps on g * min(1, max_grad_norm / (norm + 1e-6)); the coefficient
    stays on the GPU and the gradients are not written.  After a step `grad_norm` is the unclipped norm, a 0-d GPU tensor (a view of the
    optimizer's scratch: the next step overwrites it).  skip_nonfinite: a step whose norm is inf or NaN writes nothing to the parameters
    and the moments; `nonfinite_steps()` counts such steps (it reads the GPU: a sync, on request only).  The CPU `step` counters of the
    state advance on a skipped step too - whether the step was skipped is known on the GPU only, and reading it would be the host sync
    this path exists to avoid - so the bias corrections of later steps are those of the step count including skipped steps.
    skip_nonfinite without max_grad_norm computes the norm with max_norm = inf (coefficient 1).  Both are attributes of the optimizer,
    not entries of `param_groups`: `state_dict()` is torch's.  With either set, every group must live on ONE GPU (ValueError otherwise).
    Under DistributedDataParallel the gradients are all-reduced before step() runs: every rank computes the same norm, no collective
    is added.

    ema_decay (a float in [0, 1), or None): every step also moves an exponential moving average of each parameter it steps,
    e <- e + (1 - ema_decay) (p' - e), in the same launch (hipops.adamw_ema_multi; with max_grad_norm / skip_nonfinite the clipped form).
    `state[p]['ema']` is created at the parameter's first step as a clone of p before the update - and likewise when a loaded state has
    none - and travels in `state_dict()` / `load_state_dict()` like the moments.  A step skipped by skip_nonfinite leaves the averages
    alone.  There is no warm-up schedule of the decay, and buffers (BatchNorm running statistics, spectral-norm u / v) are not averaged:
    hipops.ema_multi serves those.  An attribute of the optimizer like max_grad_norm, not an entry of `param_groups`; with None nothing
    changes and `state_dict()` is torch's.  Every group must live on the GPU (ValueError otherwise).  `ema_parameters()`, `swap_ema()`
    and `ema_state_dict()` read the averages."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, **kw):
        ema_decay = kw.pop('ema_decay', None)
        if ema_decay is not None:
            ema_decay = float(ema_decay)
            if not 0.0 <= ema_decay < 1.0:
                raise ValueError(f'ema_decay must lie in [0, 1), got {ema_decay}')
        self.ema_decay = ema_decay
        self._ema_swapped = False
        max_grad_norm = kw.pop('max_grad_norm', None)
        self.skip_nonfinite = bool(kw.pop('skip_nonfinite', False))
        if max_grad_norm is not None:
            max_grad_norm = float(max_grad_norm)
            if not max_grad_norm >= 0.0:
                raise ValueError(f'max_grad_norm must be >= 0, got {max_grad_norm}')
        self.max_grad_norm = max_grad_norm
        self.grad_norm = None
        self._clip_scratch = {}                     # device -> [partials, out (norm, coefficient, finite, non-finite steps)]
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

    def _global_norm(self, groups):
        """The four floats of hipops.grad_norm_finish for the gradients of every parameter of `groups`, on their GPU (None: no gradient)."""
        grads = []
        for group in groups:
            for p in group['params']:
                if p.grad is None:
                    continue
                if p.grad.is_sparse or p.grad.dtype != torch.float32:
                    raise ValueError('wavthruvec_pytorch_amd.optim.AdamW clips dense fp32 gradients')
                grads.append(p.grad)
        if not grads:
            return None
        dev = grads[0].device
        if any(g.device != dev for g in grads):
            raise ValueError('max_grad_norm / skip_nonfinite serve parameters on one GPU')
        need = hipops.grad_sumsq_partials(grads)
        scratch = self._clip_scratch.get(dev)
        if scratch is None:
            scratch = self._clip_scratch[dev] = [None, torch.zeros(4, device=dev)]
        if scratch[0] is None or scratch[0].numel() < need:      # sized at the first step; grows only if more gradients turn up
            scratch[0] = torch.empty(need, device=dev)
        hipops.grad_sumsq_multi(grads, scratch[0])
        out = hipops.grad_norm_finish(scratch[0], need, float('inf') if self.max_grad_norm is None else self.max_grad_norm, scratch[1])
        self.grad_norm = out[0]
        return out

    def nonfinite_steps(self):
        """Steps so far whose gradient norm was inf or NaN.  Reads the GPU counter: a host sync."""
        return sum(int(s[1][3].item()) for s in self._clip_scratch.values())

    def _hip_group(self, group, clip=None):
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
            if self.ema_decay is not None and 'ema' not in st:      # the first step, or a loaded state without one: start from p
                st['ema'] = p.detach().clone(memory_format=torch.contiguous_format)
            by_dev.setdefault((p.device, int(st['step'].item()) + 1), []).append((p, g, st))
        for (_dev, t), rows in by_dev.items():      # one call per group (parameters that joined later carry another step count)
            ps = [r[0] for r in rows]
            lists = (ps, [r[1] for r in rows], [r[2]['exp_avg'] for r in rows], [r[2]['exp_avg_sq'] for r in rows])
            hyper = dict(lr=group['lr'], betas=group['betas'], eps=group['eps'], weight_decay=group['weight_decay'], step=t)
            if self.ema_decay is not None:
                hipops.adamw_ema_multi(*lists, [r[2]['ema'] for r in rows], clip, ema_decay=self.ema_decay,
                                       skip_nonfinite=self.skip_nonfinite, **hyper)
            elif clip is None:
                hipops.adamw_multi(*lists, **hyper)
            else:
                hipops.adamw_multi_clipped(*lists, clip, skip_nonfinite=self.skip_nonfinite, **hyper)
            torch._foreach_add_([r[2]['step'] for r in rows], 1)
            # the kernel wrote through the raw pointers: the caches of folded / packed weights are keyed on the version counters
            torch.autograd.graph.increment_version(ps)

    def ema_parameters(self):
        """[(p, e), ...]: every parameter that has state with its average, in the order of the parameter groups."""
        return [(p, self.state[p]['ema']) for group in self.param_groups for p in group['params']
                if p in self.state and 'ema' in self.state[p]]

    def _swap(self):
        by_dev = {}
        for p, e in self.ema_parameters():
            by_dev.setdefault(p.device, []).append((p, e))
        for rows in by_dev.values():
            ps = [r[0] for r in rows]
            hipops.swap_multi(ps, [r[1] for r in rows])
            # as after a step: the caches of folded / packed weights are keyed on the version counters
            torch.autograd.graph.increment_version(ps)

    @contextlib.contextmanager
    def swap_ema(self):
        """`with opt.swap_ema():` - inside, every parameter that has state holds its average and `state[p]['ema']` holds the weights: one
        hipops.swap_multi per list on entry and on exit (on exceptions too), the version counters bumped both times so that fold and pack
        caches refresh.  Storage pointers do not move: recorded launch plans stay valid.  Not re-entrant: nesting it, or step() inside it,
        raises RuntimeError."""
        if self.ema_decay is None:
            raise RuntimeError('wavthruvec_pytorch_amd.optim.AdamW.swap_ema needs ema_decay')
        if self._ema_swapped:
            raise RuntimeError('wavthruvec_pytorch_amd.optim.AdamW.swap_ema is not re-entrant')
        with torch.no_grad():
            self._swap()
        self._ema_swapped = True
        try:
            yield self
        finally:
            with torch.no_grad():
                self._swap()
            self._ema_swapped = False

    @torch.no_grad()
    def step(self, closure=None):
        if self._ema_swapped:
            raise RuntimeError('wavthruvec_pytorch_amd.optim.AdamW.step inside swap_ema(): the parameters hold the averages')
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        groups = self.param_groups
        mine = [self._on_gpu(g) for g in groups]
        # torch's own step WITHOUT the hook wrapper Optimizer.__init__ puts around a class's step: this method already runs inside one
        torch_step = getattr(torch.optim.AdamW.step, '__wrapped__', torch.optim.AdamW.step)
        guarded = self.max_grad_norm is not None or self.skip_nonfinite
        if guarded and not all(mine):
            raise ValueError('wavthruvec_pytorch_amd.optim.AdamW: max_grad_norm / skip_nonfinite need every parameter group on the GPU '
                             '(use torch.nn.utils.clip_grad_norm_ for CPU parameters)')
        if self.ema_decay is not None and not all(mine):
            raise ValueError('wavthruvec_pytorch_amd.optim.AdamW: ema_decay needs every parameter group on the GPU')
        if not any(mine):
            torch_step(self)
            return loss
        clip = self._global_norm(groups) if guarded else None
        for g in (g for g, hip in zip(groups, mine) if hip):
            self._hip_group(g, clip)
        rest = [g for g, hip in zip(groups, mine) if not hip]
        if rest:
            # torch's implementation walks self.param_groups: show it the other groups only (same dict objects, nothing is copied)
            self.param_groups = rest
            try:
                torch_step(self)
            finally:
                self.param_groups = groups
        return loss


def ema_state_dict(optimizer, module):
    """`module.state_dict()` with every parameter `optimizer` holds an average of replaced by a clone of that average (shaped like the
    parameter); buffers and parameters without one are taken as they are (detached clones).  Keys and order are those of
    `module.state_dict()`: torch.save({'generator': ema_state_dict(opt_g, generator)}, path) is a checkpoint of the averaged weights."""
    emas = {id(p): e for p, e in optimizer.ema_parameters()}
    params = dict(module.named_parameters(remove_duplicate=False))
    out = module.state_dict()
    for key in out:
        p = params.get(key)
        src = emas.get(id(p)) if p is not None else None
        out[key] = (src.view(p.shape) if src is not None else out[key]).detach().clone()
    return out


def clip_grad_norm_(parameters, max_norm, norm_type=2.0, error_if_nonfinite=False):
    """torch.nn.utils.clip_grad_norm_ for what the library serves: dense fp32 gradients on one GPU and norm_type 2.  Returns the total
    norm (a 0-d GPU tensor) and scales the gradients in place by min(1, max_norm / (norm + 1e-6)); the coefficient never leaves the GPU
    and a coefficient of 1 leaves every bit alone.  A non-finite norm propagates into the gradients as under torch, unless
    error_if_nonfinite - then RuntimeError, after the one host read this function can make.  Parameters without .grad are skipped; no
    gradient at all returns a zero tensor.  Anything else raises ValueError: there is no quiet fall-back."""
    if isinstance(parameters, torch.Tensor):
        parameters = [parameters]
    if float(norm_type) != 2.0:
        raise ValueError(f'wavthruvec_pytorch_amd.optim.clip_grad_norm_ serves norm_type 2, got {norm_type}')
    max_norm = float(max_norm)
    if not max_norm >= 0.0:
        raise ValueError(f'max_norm must be >= 0, got {max_norm}')
    grads = [p.grad for p in parameters if p.grad is not None]
    if not grads:
        return torch.tensor(0.0)
    for g in grads:
        if g.is_sparse or g.dtype != torch.float32:
            raise ValueError(f'wavthruvec_pytorch_amd.optim.clip_grad_norm_ serves dense fp32 gradients, got {g.dtype}'
                             + (' (sparse)' if g.is_sparse else ''))
        if not g.is_cuda or g.device != grads[0].device:
            raise ValueError('wavthruvec_pytorch_amd.optim.clip_grad_norm_ serves gradients on one GPU')
        if not g.is_contiguous():
            raise ValueError('wavthruvec_pytorch_amd.optim.clip_grad_norm_ scales in place: a gradient is not contiguous')
    grads = [g for g in grads if g.numel()]
    if not grads:
        return torch.tensor(0.0)
    partials, count = hipops.grad_sumsq_multi(grads)
    out = hipops.grad_norm_finish(partials, count, max_norm)
    if error_if_nonfinite and out[2].item() == 0.0:
        raise RuntimeError(f'The total norm of order {norm_type} for gradients from `parameters` is non-finite, so it cannot be clipped')
    hipops.scale_multi(grads, out[1:2])
    return out[0]
