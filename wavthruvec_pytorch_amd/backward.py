"""Backward pass of the Vec2Wav generator on the HIP path (`loss_gen_all.backward()` of
vec2wav/train.py:214 back-propagates through `generator(wv_feat, spk_emb, noise)`).

`GeneratorFunction` wraps `Generator._forward_hip(save=...)` for autograd.  The backward mirrors the forward schedule in
reverse - `_Walk`: tail, then per stage residual -> cbn -> upsample, then conv_pre - and runs entirely through `hipops`:

  conv / transposed-conv input gradients  conv1d / conv1d_multi / resblock2_stage(bwd=) / convt1d_dgrad: the forward tile kernel itself
                                          on the output gradient with transposed(-flipped) weights, the leaky_relu derivative as an epilogue mask
  weight gradients                        wgrad / wgrad_bf16 (MFMA, reduction over positions, deterministic slab reduce)
  bias gradients                          channel_sum, or bn_reduce_partials over the row sums a masked conv launch left
  Conditional BatchNorm                   cbn_backward (+ one all-reduce of 2C sums when data-parallel)
  tanh + conv_post                        tail_backward
  weight norm, spectral-norm Linear, fcs  wn_backward, cond_backward

Scope: ResBlock2 (the reference default) and ResBlock1 generators with up to 3 residual branches per stage.
"""
from __future__ import annotations

import contextlib
from collections import namedtuple
from functools import partial

import torch

from . import _hip, hipops
from .models import ResBlock2, _resblock_steps      # (models.py imports this module inside its functions only)

LRELU_SLOPE = 0.1


class GeneratorFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, gen, names, x, spk, nz, *params):
        if gen.num_kernels > 3:
            raise NotImplementedError('Generator (HIP) backward supports up to 3 residual branches per stage')
        save = {}
        y = gen._forward_hip(x, spk, nz, save)
        ctx.gen, ctx.names, ctx.saved = gen, names, save
        ctx.needs = [p.requires_grad for p in params]
        ctx.need_dx = x.requires_grad           # the latent as an autograd citizen (the reference's modules are: models.py:116-123)
        return y

    @staticmethod
    @_hip.on_tensor_device
    def backward(ctx, dy):
        grads = generator_backward(ctx.gen, ctx.saved, dy.contiguous().float(), need_dx=ctx.need_dx)
        ctx.saved = None
        out = [grads.get(n) if need else None for n, need in zip(ctx.names, ctx.needs)]
        return (None, None, grads.get('__x__'), None, None, *out)


def _dconv(gen, x, wT, out, *, k, **kw):
    """Input-gradient convolution with the transposed(-flipped) weights wT [k][C_out][C_in]: the forward conv kernel of the
    generator's precision mode (exact fp32 MFMA, or the split-f16 / bf16 kernel when the layer shape has one).  gen None: the exact kernel."""
    co = wT.shape[2]
    if gen is not None and gen.precision != 'f32' and (k & 1) and k >= 3 and hipops.split_supported(wT.shape[1], co) \
            and co >= gen.split_min_channels and kw.get('in_stride', 0) <= 1:
        bf = gen.precision == 'bf16'
        return hipops.conv1d(x, None, None, out, k=k, algo=hipops.ALGO_BF16 if bf else hipops.ALGO_SPLIT, wps=hipops.pack_split(wT, bf16=bf), **kw)
    return hipops.conv1d(x, wT, None, out, k=k, wp=hipops.pack_mfma(wT), **kw)


def _wgrad(gen, x, dy, *, k, dil, slope, x_affine=None):
    """Conv1d weight gradient in the generator's arithmetic: bf16 operands with fp32 accumulation when the generator computes in bf16 (what
    the reference's autocast backward does, train.py:167,214) and the layer shape has that kernel, the exact fp32 kernel otherwise or for gen None."""
    if gen is not None and gen.precision == 'bf16':
        dwf = hipops.wgrad_bf16(x, dy, k=k, dil=dil, slope=slope, x_affine=x_affine)
        if dwf is not None:
            return dwf
    return hipops.wgrad(x, dy, k=k, dil=dil, slope=slope, x_affine=x_affine)


def _wn_grads(grads, name, m, dwf):
    """dW in the [k][C_in][C_out] layout -> gradients of the layer's weight_v / weight_g (or plain weight)."""
    if m.weight_normed:
        dv, dg = hipops.wn_backward(dwf, m.weight_v.detach(), m.weight_g.detach(), m.transposed)
        grads[name + '.weight_v'], grads[name + '.weight_g'] = dv, dg
    else:
        dv, _ = hipops.wn_backward(dwf, m.weight.detach(), None, m.transposed)
        grads[name + '.weight'] = dv


# One residual step as its backward reads it:  out = x' + conv_a(lrelu x')  (cb None)  or  out = x' + conv_b(lrelu u), u = conv_a(lrelu x'), with
# x' = a * x + s when the input carries the CondBN affine `aff` = (a, s), else None.  na / nb: parameter-name prefixes; wfa / wfb: folded weights.
PairStep = namedtuple('PairStep', 'x aff u ca na wfa cb nb wfb', defaults=(None, None, None))


def pair_backward(steps, d, grads, dconv, wgrad, *, db_out=None, dst=None, accumulate=False):
    """Backward of a chain of residual steps, last to first, from d = dL/d(its output): weight / bias gradients into `grads`, returns dL/d(steps[0].x').
    dconv / wgrad: `_dconv` / `_wgrad` bound to a generator (its precision picks the kernels) or to None (exact).  db_out: the bias gradient
    of the outermost conv when the caller has it (the channel sums of d).  dst / accumulate: where the first step's input gradient lands.
      d(x') = d + lrelu'(x') * conv(du; Wa^T flipped),  du = d  or  lrelu'(u) * conv(d; Wb^T flipped)"""
    for n in reversed(range(len(steps))):
        s = steps[n]
        du = d
        if s.cb is not None:
            du = torch.empty_like(d)
            dconv(d, hipops.transpose_flip(s.wfb), du, k=s.cb.kernel_size, dil=s.cb.dilation, slope=1.0, mask=(s.u, None), mask_slope=LRELU_SLOPE)
            _wn_grads(grads, s.nb, s.cb, wgrad(s.u, d, k=s.cb.kernel_size, dil=s.cb.dilation, slope=LRELU_SLOPE))
            grads[s.nb + '.bias'] = hipops.channel_sum(d) if db_out is None else db_out
            db_out = None
        out = dst if n == 0 and dst is not None else torch.empty_like(d)
        dconv(du, hipops.transpose_flip(s.wfa), out, k=s.ca.kernel_size, dil=s.ca.dilation, slope=1.0, res=d, mask=(s.x, s.aff),
              mask_slope=LRELU_SLOPE, accumulate=accumulate and n == 0)
        _wn_grads(grads, s.na, s.ca, wgrad(s.x, du, k=s.ca.kernel_size, dil=s.ca.dilation, slope=LRELU_SLOPE, x_affine=s.aff))
        grads[s.na + '.bias'] = hipops.channel_sum(du) if db_out is None else db_out
        d, db_out = out, None
    return d


def _branch_steps(ws, wf, i, j, rb, name, xr, aff):
    """Branch j of stage i as PairSteps, from the buffers its forward kept (models.py:37-44, 65-70); the first input is x' = a * xr + s."""
    if isinstance(rb, ResBlock2):    # t1 = x' + conv0(lrelu x'), r = t1 + conv1(lrelu t1)
        ins = [xr, ws[f'act.t1_{i}_{j}']]
        return [PairStep(ins[n], aff if n == 0 else None, None, c, f'{name}.convs.{n}', wf[f'{name}.convs.{n}']) for n, c in enumerate(rb.convs)]
    ins = [xr, ws[f'act.xa_{i}_{j}'], ws[f'act.xb_{i}_{j}']]       # ResBlock1: x_{n+1} = x_n + convs2_n(lrelu(convs1_n(lrelu x_n)))
    return [PairStep(ins[n], aff if n == 0 else None, ws[f'act.t1_{i}_{j}_{n}'], rb.convs1[n], f'{name}.convs1.{n}', wf[f'{name}.convs1.{n}'],
                     rb.convs2[n], f'{name}.convs2.{n}', wf[f'{name}.convs2.{n}']) for n in range(3)]


@contextlib.contextmanager
def _beside(side, reads):
    """Work that nothing downstream waits for, on the side stream beside the main stream's next launches (joined at the end of the backward).
    `reads`: the main-stream tensors the work reads; the body appends every tensor it makes, which the main stream's consumers - the optimizer
    - use later, to the list it is handed.  Both lifetimes are told to the allocator here and nowhere else: a tensor left out is a
    use-after-free that shows only under allocator pressure."""
    main = torch.cuda.current_stream(reads[0].device)
    side.wait_stream(main)
    made = []
    with torch.cuda.stream(side):
        yield made
    for t in reads:
        t.record_stream(side)
    for t in made:
        t.record_stream(main)


# The merged ResBlock2 form of one stage, as its input-gradient launches and its weight-gradient step read and write it:
#   dxs, unit      dL/d(stage output); every branch receives dr = dxs / nk through the per-(b, c) affine `unit` = (1 / nk, 0)
#   stg            the stage's record (forward_plan.Stage): the branches, their parameter-name prefixes, the heaviest-first order
#   t1s, xr, aff   what the forward kept: t1_j, and the stage input x' = a * xr + s
#   w2s, w1s       kernel and weights of every branch's conv2 / conv1 input-gradient conv (`_dgrad_weights`)
#   dt1s, dx       written: dL/d(t1_j), and dL/dx' summed over the branches
_Rb2Stage = namedtuple('_Rb2Stage', 'dxs unit stg t1s xr aff w2s w1s dt1s dx')


def _dgrad_weights(sv, nm, use_bf):
    """Kernel and weights of the merged form's input-gradient conv of layer `nm`: the bf16 kernel the forward used on transposed, tap-reversed
    fragments packed here, or the exact fp32 tile kernel on a fragment stream made straight from the forward-layout weights (no transposed
    copy: C -> C layers) - the one the forward's batched weight fold built beside the forward streams, when it did."""
    wf = sv['wf'][nm]
    if use_bf:
        return dict(algo=hipops.ALGO_BF16, wps=hipops.pack_split(hipops.transpose_flip(wf), bf16=True))
    wp = sv.get('wpd', {}).get(nm)
    return dict(algo=hipops.ALGO_MFMA, wp=wp if wp is not None else hipops.pack_mfma_dgrad(wf))


def _rb2_dgrad_one_kernel(s):
    """Narrow stages (C = 32 / 16): both input-gradient convs of all branches in ONE kernel (v2w_stage_args::bwd_*) - dxs read once, every
    dt1_j written once and not read back, the branch sum in registers: 9 tensor passes instead of 18.  Returns what
    `_rb2_dgrad_three_launches` returns, or None (nothing launched) when the kernel does not take the stage."""
    B, C, Lo = s.dxs.shape
    p2, p1 = [q.get('wp') for q in s.w2s], [q.get('wp') for q in s.w1s]
    ks, dd2, dd1 = s.stg.ks, s.stg.dil2s, s.stg.dil1s          # (the kernel takes conv2's dilations first)
    ntile = hipops.resblock2_stage_bwd_rows(B, C, Lo, ks, dd2, dd1)
    if not ntile or any(q is None for q in p1 + p2):       # (the kernel reads fp32 fragment streams only)
        return None
    rsp = [torch.empty((ntile * C * 2,), device=s.dxs.device) for _ in s.stg.rbs]       # (tile, wave) channel sums of dt1_j
    branches = [dict(wp1=p2[j], b1=None, wp2=p1[j], b2=None, k=ks[j], dil1=dd2[j], dil2=dd1[j]) for j in range(len(s.stg.rbs))]
    ok = hipops.resblock2_stage(s.dxs, s.unit, branches, s.dx, slope=1.0, out_div=0.0, bwd=(s.t1s, s.dt1s, s.xr, s.aff, LRELU_SLOPE, rsp))
    return (ntile, rsp) if ok else None


def _rb2_dconv1(s, j, out, **extra):
    """t1 = x' + conv1(lrelu x') + b1, x' = a*xr + s   ->   dx' = sum_j dt1_j + lrelu'(x') * conv(dt1_j; W1^T flipped)"""
    return (s.dt1s[j], None, None, out, dict(k=s.stg.rbs[j].kernel_size, dil=s.stg.rbs[j].convs[0].dilation, slope=1.0, res=s.dt1s[j], mask=(s.xr, s.aff),
                                             mask_slope=LRELU_SLOPE, **s.w1s[j], **extra))


def _rb2_dgrad_three_launches(s, rowsum):
    """The forward's launch structure mirrored: the branches' conv2 input gradients in ONE launch, the conv1 input gradients of branches
    0 .. nk-2 in one launch and the last branch adding them (heaviest kernel size first), so the tile shape is chosen for three problems' worth
    of tiles instead of one.  Writes s.dt1s and s.dx; returns (ntile, [per branch: the per-tile channel sums of dt1_j - conv1_j's bias gradient,
    an epilogue of the f32 tile kernel - or None]), ntile 0 when the launch leaves none (`rowsum` False, or Lo % 4 != 0)."""
    (B, C, Lo), nk = s.dxs.shape, len(s.stg.rbs)
    # (the launch's tile shape follows its WIDEST halo - the wide-halo tile variants are other shapes: probe with that branch)
    kw, dw = max(((rb.kernel_size, rb.convs[1].dilation) for rb in s.stg.rbs), key=lambda kd: kd[1] * (kd[0] - 1))
    ntile = hipops.conv_rowsum_tiles(B, nk, C, C, Lo, kw, dw) if Lo % 4 == 0 and rowsum else 0
    rsp = [torch.empty((ntile * C * 2,), device=s.dxs.device) if ntile else None for _ in range(nk)]
    # r_j = t1 + conv2(lrelu(t1)) + b2   ->   dt1 = dr + lrelu'(t1) * conv(dr; W2^T flipped),  dr = dxs / nk
    hipops.conv1d_multi([(s.dxs, None, None, s.dt1s[j],
                          dict(k=s.stg.rbs[j].kernel_size, dil=s.stg.rbs[j].convs[1].dilation, slope=1.0, in_affine=s.unit, res=s.dxs, res_affine=s.unit,
                               mask=(s.t1s[j], None), mask_slope=LRELU_SLOPE, rowsum=rsp[j], **s.w2s[j])) for j in s.stg.heavy_first])
    parts = [torch.empty_like(s.dxs) for _ in range(nk - 1)]
    hipops.conv1d_multi([_rb2_dconv1(s, j, parts[j]) for j in s.stg.heavy_first if j < nk - 1])
    hipops.conv1d_multi([_rb2_dconv1(s, nk - 1, s.dx, add=parts)])
    return ntile, rsp


def _rb2_branch_grads(s, j, db2, ntile, rsp, wgrad):
    """{name: gradient} of branch j's parameters from what the input-gradient launches left.  dr = dxs / nk is never materialised: conv2's
    weight gradient, linear in dr, is scaled afterwards, and `db2` (shared by the branches) is handed in."""
    c1, c2 = s.stg.rbs[j].convs
    k, nm, nk = s.stg.rbs[j].kernel_size, s.stg.names[j], len(s.stg.rbs)
    B, C, Lo = s.dxs.shape
    g = {nm + '.convs.1.bias': db2}
    _wn_grads(g, nm + '.convs.1', c2, wgrad(s.t1s[j], s.dxs, k=k, dil=c2.dilation, slope=LRELU_SLOPE).mul_(1.0 / nk))
    _wn_grads(g, nm + '.convs.0', c1, wgrad(s.xr, s.dt1s[j], k=k, dil=c1.dilation, slope=LRELU_SLOPE, x_affine=s.aff))
    if ntile:
        st = torch.empty((2 * C + 1,), device=s.dxs.device, dtype=torch.float64)
        hipops.bn_reduce_partials(rsp[j], ntile, C, B * Lo, st)
        g[nm + '.convs.0.bias'] = st[:C].float()
    else:
        g[nm + '.convs.0.bias'] = hipops.channel_sum(s.dt1s[j])
    return g


class _Walk:
    """One backward of the generator as named steps, in the order of the module docstring.  `d` is the gradient that flows down (each step
    reads it and leaves its own input's gradient there); `grads` fills with {parameter name: gradient}."""

    def __init__(self, gen, sv, dy):
        self.gen, self.sv, self.ws, self.wf = gen, sv, sv['ws'], sv['wf']
        self.B, self.dev = sv['B'], sv['x'].device
        self.side = gen._side_stream(self.dev)
        self.dconv, self.wgrad = partial(_dconv, gen), partial(_wgrad, gen)
        self.d, self.grads = dy, {}

    def tail(self):
        """tanh + conv_post (models.py:143-145)"""
        xs_last = self.ws[f'act.rb{self.gen.num_upsamples - 1}']
        self.d, dwf_post, dp = hipops.tail_backward(self.d, self.sv['y'], xs_last, self.wf['conv_post'], k=7, slope=0.01)
        self.grads['conv_post.bias'] = hipops.channel_sum(dp)
        _wn_grads(self.grads, 'conv_post', self.gen.conv_post, dwf_post)

    def residual(self, i):
        """The mean over the nk residual branches of stage i: every branch receives dr = d / nk; leaves dL/dx', x' = a * xr + s."""
        gen, ws, B, nk, dxs = self.gen, self.ws, self.B, self.gen.num_kernels, self.d
        xr, aff = ws[f'act.up{i}'], (ws[f'bn.a{i}'], ws[f'bn.s{i}'])
        C, Lo = xr.shape[1:]
        stg = gen.stage_record(i)
        rbs, names = stg.rbs, stg.names
        unit = (torch.full((B, C), 1.0 / nk, device=self.dev), torch.zeros((B, C), device=self.dev))
        # the merged launches run on ALGO_MFMA, which has no direct-kernel fallback: every gradient conv of every branch must have a
        # tile configuration at ITS kernel size and dilation (a wide halo, e.g. k = 11 with dilation 7, has none: per-branch path)
        merged = gen.precision in ('f32', 'bf16') and gen.algo == hipops.ALGO_AUTO and 1 < nk <= 3 \
            and stg.is_rb2 \
            and all(hipops.conv_tile_config(B * nk, C, C, Lo, rb.kernel_size, c.dilation) is not None for rb in rbs for c in rb.convs)
        if merged:
            return self._residual_merged(stg, unit, xr, aff)
        dr = hipops.affine_apply(dxs, *unit, torch.empty_like(dxs))
        db2 = hipops.channel_sum(dr)
        dx = torch.empty_like(dxs)
        for j in range(nk):     # the branches' input gradients summed into the stage's dx
            pair_backward(_branch_steps(ws, self.wf, i, j, rbs[j], names[j], xr, aff), dr, self.grads, self.dconv, self.wgrad,
                          db_out=db2, dst=dx, accumulate=j > 0)
        self.d = dx

    def _residual_merged(self, stg, unit, xr, aff):
        """ResBlock2 with the branches' launches merged: the input gradients by one of two variants, then one weight / bias gradient step."""
        gen, dxs, i, rbs, names, nk = self.gen, self.d, stg.i, stg.rbs, stg.names, len(stg.rbs)
        B, C, Lo = dxs.shape
        # the generator's bf16 arithmetic (precision = 'bf16': the reference under torch.autocast): the wide stages' gradient convs on the bf16
        # kernel the forward used, the narrow stages' on the exact fp32 tile kernel
        use_bf = gen.precision == 'bf16' and ((C >= gen.split_min_channels and hipops.split_supported(C, C)) or (C == 32 and Lo % 4 == 0)) \
            and all(rb.kernel_size >= 3 and (rb.kernel_size & 1) for rb in rbs)
        s = _Rb2Stage(dxs, unit, stg, [self.ws[f'act.t1_{i}_{j}'] for j in range(nk)], xr, aff,
                      [_dgrad_weights(self.sv, nm + '.convs.1', use_bf) for nm in names], [_dgrad_weights(self.sv, nm + '.convs.0', use_bf) for nm in names],
                      [torch.empty_like(dxs) for _ in range(nk)], torch.empty_like(dxs))
        done = _rb2_dgrad_one_kernel(s) if C in gen.fuse_stage and C in (16, 32) and gen.fuse_stage_backward else None
        ntile, rsp = done if done is not None else _rb2_dgrad_three_launches(s, rowsum=not use_bf)
        # weight / bias gradients: nothing downstream waits for them - side stream, beside the next stage's gradient convs.  The LAST stage of
        # the walk (stage 0: the widest convs) leaves the side stream a backlog the main stream has nothing left to run beside (it waited
        # ~2.5 ms for it at the end of the backward): its heaviest branch's weight gradients go to the main stream
        on_main = [s.stg.heavy_first[0]] if i == 0 and nk > 1 else []
        with _beside(self.side, [s.dxs, s.xr, *s.aff, *s.dt1s, *s.t1s, *[r for r in rsp if r is not None]]) as made:
            db2 = hipops.channel_sum(s.dxs) * (1.0 / nk)        # (a memory-bound pass)
            made.append(db2)
            for j in range(nk):
                if j not in on_main:
                    g = _rb2_branch_grads(s, j, db2, ntile, rsp, self.wgrad)
                    self.grads.update(g)
                    made += g.values()
        for j in on_main:       # (db2 is only handed on as the bias gradient here: no kernel of the main stream reads it)
            self.grads.update(_rb2_branch_grads(s, j, db2, ntile, rsp, self.wgrad))
        self.d = s.dx

    def cbn(self, i):
        """Conditional BatchNorm (modules.py:20-30): through the affine, the batch statistics and into gamma / beta; leaves dL/d(ups[i] output)."""
        gen, ws, sv, grads = self.gen, self.ws, self.sv, self.grads
        bn, ly = gen.cbns[i].batch_nrom, gen.cbns[i].layer
        dxr, dgb = hipops.cbn_backward(self.d, ws[f'act.up{i}'], ws[f'gb.{i}'], ws.get(f'bn.stats{i}'), bn.running_mean, bn.running_var,
                                       training=sv['training'], eps=bn.eps, sync=gen.stat_sync)
        sn_u, sn_v = sv['sn_uv'][i]               # the vectors the forward of THIS graph used (ly.weight_u/_v may have moved on)
        z = ws['z_ws'].view(gen.num_upsamples, self.B, 128)[i].contiguous()
        # the conditioning branch (spectral-norm Linear + fcs[i]: five small latency-bound kernels per stage) hangs off dgb only, and the
        # upsampler's bias gradient is a memory-bound pass: both beside the gradient convs
        with _beside(self.side, [dgb, dxr]) as made:
            made += hipops.cond_backward(dgb, z, ly.weight_orig.detach(), sn_u, sn_v, ws['sigma_ws'][i:i + 1], sv['spk'], sv['nz'])
            made.append(hipops.channel_sum(dxr))
        grads.update(zip((f'cbns.{i}.layer.weight_orig', f'cbns.{i}.layer.bias', f'fcs.{i}.weight', f'fcs.{i}.bias', f'ups.{i}.bias'), made))
        self.d = dxr

    def upsample(self, i):
        """leaky_relu -> ConvTranspose1d (models.py:128-129); leaves the gradient of the stage's input."""
        up, dxr = self.gen.ups[i], self.d
        cur_in = self.ws['act.pre'] if i == 0 else self.ws[f'act.rb{i - 1}']
        _wn_grads(self.grads, f'ups.{i}', up, hipops.wgrad(cur_in, dxr, k=up.kernel_size, u=up.stride, slope=LRELU_SLOPE))
        self.d = torch.empty_like(cur_in)
        hipops.convt1d_dgrad(dxr, self.wf[f'ups.{i}'], self.d, k=up.kernel_size, u=up.stride, mask=(cur_in, None), mask_slope=LRELU_SLOPE)

    def conv_pre(self, need_dx):
        """conv_pre (models.py:123): no activation in front of it; its input gradient only on request."""
        x, dxs = self.sv['x'], self.d
        self.grads['conv_pre.bias'] = hipops.channel_sum(dxs)
        _wn_grads(self.grads, 'conv_pre', self.gen.conv_pre, hipops.wgrad(x, dxs, k=7, dil=1, slope=1.0))
        if need_dx:     # dL/dx = conv(dxs; W_pre^T, taps reversed) - no mask
            self.grads['__x__'] = self.dconv(dxs, hipops.transpose_flip(self.wf['conv_pre']), torch.empty_like(x), k=7, dil=1, slope=1.0)


@torch.no_grad()
def generator_backward(gen, sv, dy, need_dx=False):
    """dy (B, 1, L_out) -> {parameter name: gradient}.  `sv` is the dict filled by `Generator._forward_hip(save=...)`.
    need_dx: also the gradient w.r.t. the latent input x (key '__x__'): conv_pre's input-gradient conv, one more launch."""
    # the folded weights live in module-owned buffers that the NEXT forward's fold overwrites: harmless while the parameters are unchanged
    # (the same values again); parameters that changed in between - an optimizer step between this graph's forward and its backward -
    # are what autograd itself refuses ("modified by an inplace operation")
    # (`gen`: the fold generation - every fold, a replayed launch plan's included, bumps it.  Unchanged: the buffers are this forward's.  Changed:
    # they were folded again, from whatever the parameters held then - the same values unless a parameter's version moved since the forward)
    if sv.get('vers') is not None and gen._fold_key.get('gen') != sv.get('gen') and gen._param_versions() != sv['vers']:
        raise RuntimeError('Generator (HIP) backward: the generator\'s weights were modified and re-folded by a later forward before this '
                           'backward ran (the saved forward used the earlier weights)')
    w = _Walk(gen, sv, dy)
    w.tail()
    for i in reversed(range(gen.num_upsamples)):
        w.residual(i)
        w.cbn(i)
        w.upsample(i)
    w.conv_pre(need_dx)
    torch.cuda.current_stream(w.dev).wait_stream(w.side)
    return w.grads


class ResBlockFunction(torch.autograd.Function):
    """A stand-alone `ResBlock1` / `ResBlock2` as an autograd citizen (the reference's are: models.py:37-44, 65-70): the forward loop of
    models._resblock_steps with every step kept, the backward from `pair_backward` with the exact kernels.  `pairs`: [(conv_a, conv_b | None)]
    as in _resblock_steps; params: the parameters of every conv, in `names` order."""

    @staticmethod
    def forward(ctx, rb, pairs, names, x, *params):
        out, ctx.steps = _resblock_steps(rb, x, pairs, keep=True)
        ctx.names, ctx.needs, ctx.need_dx = names, [p.requires_grad for p in params], x.requires_grad
        return out

    @staticmethod
    @_hip.on_tensor_device
    @torch.no_grad()
    def backward(ctx, dout):
        grads = {}
        dx = pair_backward(ctx.steps, dout.contiguous().float(), grads, partial(_dconv, None), partial(_wgrad, None))
        ctx.steps = None
        out = [grads.get(n) if need else None for n, need in zip(ctx.names, ctx.needs)]
        return (None, None, None, dx if ctx.need_dx else None, *out)
