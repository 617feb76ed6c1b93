"""MPD / MSD discriminators on the MI355X, forward and backward.

Mirror of /root/reference/vec2wav/models.py:158-275 - `DiscriminatorP`, `MultiPeriodDiscriminator(hp)`, `DiscriminatorS`,
`MultiScaleDiscriminator()`, the same `forward(y, y_hat) -> (y_d_rs, y_d_gs, fmap_rs, fmap_gs)`, identical `state_dict` keys and
shapes (weight_norm: bias / weight_g / weight_v with Conv2d (k, 1) shapes for the period discriminators; legacy spectral_norm on
the first scale discriminator: bias / weight_orig / weight_u / weight_v) - so `do_%08d` checkpoints load.

Differentiable: each discriminator call is one `autograd.Function` (`_DiscFn`) whose backward runs on the same C ABI (input
gradients on the forward conv kernel with transposed tap-flipped weights, weight gradients on `v2w_wgrad_groups`, weight-norm
backward on `v2w_wn_bwd`), so both optimisation steps of train.py:188-215 work.  No PyTorch/CPU fallback: the convolutions run on
the f32 MFMA tile kernel through the C ABI as stride-1 problems (csrc/v2w_disc.hip explains the mapping):
  stride-s layers  -> `v2w_phase_split` + a conv over the s stacked phases (ceil(k/s)-ish taps),
  (k, 1) Conv2d    -> Conv1d with dilation = period on the flattened (H * period) axis, feature maps kept as (B, C, H, period),
  grouped Conv1d   -> one problem per group on channel slices (`in_ct` / `out_ct`), four groups per launch,
  C_in = 1 layers  -> `v2w_unfold1` (k shifted rows, padded to 16) + a 1-tap conv,
  leaky_relu       -> the conv epilogue (`out_slope`): feature maps are stored activated, as the reference returns them,
  row pitch        -> feature maps live in (B, C, roundup4(length)) buffers (the kernel's float4 staging) and are returned as
                      `[:, :, :length]` views: same shapes and values as the reference, strided when length % 4 != 0.
Weight preparation (weight-norm fold on the HIP kernel; the spectral-norm power iteration, sigma and W / sigma of all layers of a call in
one `hipops.sn_step` - `NATIVE_SN`; tap re-indexing for the stride / group forms with torch index ops on the weight tensors) is cached
per parameter version.

How the file is laid out: a `_DiscConv` decides its stride-1 form once, in `__init__` (`form`, `cs`, `kp`, `Q`); its
`kernel_weights()` returns a `_Weights` record (forward weights, the optional split-f16 set, input-gradient weights built on first
use); `_conv_split_or_exact` is the one place a conv is launched with the split-f16 fallback; `_DiscFn.backward` walks the layers
top down through `_dz_and_bias_grad`, `_weight_grad` and `_input_grad`.  Every kernel is reached through `hipops`.
"""
from __future__ import annotations

import math
import os
import threading
from typing import NamedTuple, Optional

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _hip, hipops, mel
from .synthetic import DISC_P_LAYERS, DISC_P_POST, DISC_S_LAYERS, DISC_S_POST

LRELU_SLOPE = 0.1   # models.py:9
_UNFOLD_ROWS = 16   # C_in = 1 layers: the k shifted copies padded to the MFMA kernel's smallest channel block

# the stride-1 form a layer's conv runs in:
_FIRST = 'first'    # C_in = 1: the k taps as 16 rows of a 1-tap conv (v2w_unfold1)
_TAPS = 'taps'      # optional (V2W_DISC_UNFOLD=1): the taps of a short strided conv as k * C_in channels of a 1-tap conv (v2w_unfold_taps)
_PHASES = 'phases'  # stride s > 1: the s phases of the input stacked along the channels (v2w_phase_split), ceil(k / s)-ish taps
_PLAIN = 'plain'    # stride 1: the input itself, its pitch tail zeroed (v2w_zero_tail)


def _mfma_packs(w4):
    """Per group the packed MFMA stream of w4 [G][k][C_in][C_out], or None where the tile kernel has no configuration for the shape."""
    G, _k, ci, co = w4.shape
    if ci % 16 == 0 and (co % 32 == 0 or co == 16):
        return list(hipops.pack_mfma_batch(w4).unbind(0))
    return [None] * G


class _Weights:
    """One layer's weights in kernel form, per group of its stride-1 conv (`_DiscConv.kernel_weights` builds it; the y and y_hat calls
    of one step share it):
      w4 [G][kp][cs / G][C_out / G], wp    the forward conv and its packed MFMA streams (`_mfma_packs`)
      ws4 [G][kps][..][..], wps            the same conv for the split-f16 kernel (precision 'f16x3'), or None: not eligible, or declined
      transposed(), transposed_split()     the input-gradient conv's weights in both forms, built on first use."""
    __slots__ = ('w4', 'wp', 'ws4', 'wps', 'wT4', 'wTp', 'wTs4', 'wTs')

    def __init__(self, w4, split):
        self.w4, self.wp = w4, _mfma_packs(w4)
        self.ws4 = self.wps = self.wT4 = self.wTp = self.wTs4 = self.wTs = None
        if split:
            # (hi, lo) f16 fragments + scale record of the forward conv, per group.  The kernel pipelines over an odd tap count: the
            # two-tap phase-stacked layers (k = 5, stride 3) get a zero third tap behind the others (same pad_left; 1.5 x the MFMAs at 2.2 x the rate)
            self.ws4 = w4 if w4.shape[1] % 2 == 1 else torch.cat([w4, torch.zeros_like(w4[:, :1])], 1)
            self.wps = [hipops.pack_split(self.ws4[g]) for g in range(w4.shape[0])]

    def __contains__(self, name):
        """`'wps' in rec`: the record carries that form at this point."""
        return getattr(self, name, None) is not None

    def split(self):
        """(ws4, wps) or None."""
        return None if self.wps is None else (self.ws4, self.wps)

    def transposed(self):
        """(wT4 [G][kp][C_out / G][cs / G] with the taps reversed, its packed MFMA streams)."""
        if self.wT4 is None:
            self.wT4 = self.w4.flip(1).transpose(2, 3).contiguous()
            self.wTp = _mfma_packs(self.wT4)
        return self.wT4, self.wTp

    def transposed_split(self, allowed):
        """(wTs4 [G][kps][C_out / G][cs / G] - the zero pad tap comes first - and its pack_split pairs), or None: the layer has no split set, the
        split kernel does not serve the transposed shape, or (`allowed` False) it has declined this problem before."""
        if self.wTs is None and self.wps is not None and allowed and hipops.split_supported(self.w4.shape[3], self.w4.shape[2]):
            self.wTs4 = self.ws4.flip(1).transpose(2, 3).contiguous()
            self.wTs = [hipops.pack_split(self.wTs4[g]) for g in range(self.wTs4.shape[0])]
        return None if self.wTs is None else (self.wTs4, self.wTs)

    def forget_split(self, transposed):
        """The split kernel declined the forward conv (or, `transposed`, the input-gradient conv): exact from here on."""
        if transposed:
            self.wTs4 = self.wTs = None
        else:
            self.ws4 = self.wps = None


class _DiscConv(nn.Module):
    """Parameter holder of one (weight- or spectral-)normed conv of a discriminator; `wshape` is the reference's weight shape
    (C_out, C_in / groups, k) or (C_out, C_in, k, 1)."""

    def __init__(self, c_in, c_out, k, stride, groups, padding, spectral, conv2d):
        super().__init__()
        self.c_in, self.c_out, self.k, self.stride, self.groups, self.padding = c_in, c_out, k, stride, groups, padding
        self.spectral = spectral
        wshape = (c_out, c_in // groups, k, 1) if conv2d else (c_out, c_in // groups, k)
        fan_in = c_in // groups * k
        bound = 1.0 / math.sqrt(fan_in)
        w = torch.empty(wshape).uniform_(-bound, bound)
        self.bias = nn.Parameter(torch.empty(c_out).uniform_(-bound, bound))
        if spectral:
            self.weight_orig = nn.Parameter(w)
            self.register_buffer('weight_u', F.normalize(torch.randn(c_out), dim=0, eps=1e-12))
            self.register_buffer('weight_v', F.normalize(torch.randn(fan_in), dim=0, eps=1e-12))
        else:
            self.weight_g = nn.Parameter(w.flatten(1).norm(dim=1).view(c_out, *([1] * (len(wshape) - 1))).clone())
            self.weight_v = nn.Parameter(w)
        self._cache = None
        self._pair_rec = None
        self._last_sn = None
        self._sn_ready = None           # (wf, _SnKept) of a spectral layer that `_sn_prepare` has stepped for the coming kernel_weights()
        self._wf_sn = None
        self._jmap = None
        self._wpad = None
        self._no_split_dgrad = None     # (C_out / G, cs / G, pitch) of the input-gradient conv the split-f16 kernel declined last
        # 'f32' (exact) or 'f16x3': the forward and input-gradient convs of the layers the split-f16 kernel serves - dense, stride 1, an odd
        # tap count: the 1024 -> 1024 five-tap convs that are 54 % of a period discriminator's and 30 % of a scale discriminator's FLOPs -
        # run as f16 hi + lo operands (three MFMAs per product, fp32 accumulate: ~1e-6 of the fp32 result); weight gradients stay exact.
        # Set through `set_precision(module, ...)`.
        self.precision = 'f32'
        # optional form of the short strided ungrouped convs (DiscriminatorP k = 5, stride 3): taps unfolded into channels of a
        # 1-tap conv (exact MAC count, no halo).  Measured equal to the phase-stacked default (40.6 vs 40.4 ms per MPD forward):
        # one tap per staged chunk makes the kernel staging-bound, which cancels the 6/5 tap-slot saving.
        self.unfolded = c_in > 1 and stride > 1 and groups == 1 and k <= 8 and os.environ.get('V2W_DISC_UNFOLD', '0') == '1'
        # the stride-1 form: `cs` stacked input channels, `kp` taps of which `Q` sit left of the output position.  With j - P = s*q + r, tap j
        # of the strided conv is tap q + Q on phase r of the stacked one
        if c_in == 1:
            self.form, self.cs = _FIRST, _UNFOLD_ROWS
        elif self.unfolded:
            self.form, self.cs = _TAPS, k * c_in
        elif stride > 1:
            self.form, self.cs = _PHASES, stride * c_in
        else:
            self.form, self.cs = _PLAIN, c_in
        self.Q, self.kp = 0, 1
        if self.form in (_PHASES, _PLAIN):
            self.Q = -(-padding // stride)
            self.kp = self.Q + (k - 1 - padding) // stride + 1

    def extra_repr(self):
        return f'{self.c_in}, {self.c_out}, k={self.k}, stride={self.stride}, groups={self.groups}, ' \
               f'{"spectral_norm" if self.spectral else "weight_norm"}'

    def rows_out(self, rows_in):
        """Output rows of the strided conv on `rows_in` input rows."""
        if self.form == _PHASES:
            return -(-rows_in // self.stride)
        return (rows_in + 2 * self.padding - self.k) // self.stride + 1 if self.form in (_FIRST, _TAPS) else rows_in

    def dil(self, inner):
        """Dilation of the stride-1 conv on feature maps of `inner` columns per row."""
        return 1 if self.kp == 1 else inner

    # -- weights in kernel form --------------------------------------------------------------------------------------
    def _folded(self, out=None):
        """-> wf [k][C_in / groups][C_out], normalisation applied (one power iteration first for spectral_norm in training)."""
        co, cig, k = self.c_out, self.c_in // self.groups, self.k
        if not self.spectral:
            return hipops.fold_conv_weight(self.weight_v.detach().reshape(co, cig, k), self.weight_g.detach().reshape(co, 1, 1), out=out)
        if NATIVE_SN:          # stepped with the discriminator's other layers (`_sn_prepare`), or - a layer used on its own - here, n = 1
            if self._sn_ready is None:
                _sn_prepare([self])
            (wf, self._last_sn), self._sn_ready = self._sn_ready, None
            assert out is None or wf.data_ptr() == out.data_ptr()
            return wf
        w = self.weight_orig.detach()
        wm = w.reshape(co, -1)
        if self.training:      # legacy torch.nn.utils.spectral_norm: v <- norm(W^T u), u <- norm(W v), in place, per forward
            self.weight_v.copy_(F.normalize(torch.mv(wm.t(), self.weight_u), dim=0, eps=1e-12))
            self.weight_u.copy_(F.normalize(torch.mv(wm, self.weight_v), dim=0, eps=1e-12))
        sigma = torch.dot(self.weight_u, torch.mv(wm, self.weight_v))
        self._last_sn = (sigma, self.weight_u.clone(), self.weight_v.clone())
        return hipops.fold_conv_weight((w / sigma).reshape(co, cig, k), None, out=out)

    def invalidate_weight_cache(self):
        self._cache = None

    def _key(self):
        return tuple((p.data_ptr(), p._version) for p in list(self.parameters()) + list(self.buffers()))

    def _reindex_constants(self):
        """Constants of the stacked forms' re-indexing, built once per device: the tap map j[q][r] (k = "no such tap" -> the zero row of wpad)."""
        dev = self.bias.device
        if self._wpad is None or self._wpad.device != dev:
            q = torch.arange(self.kp, device=dev).view(self.kp, 1) - self.Q
            r = torch.arange(self.stride, device=dev).view(1, self.stride)
            j = self.stride * q + r + self.padding
            self._jmap = torch.where((j >= 0) & (j < self.k), j, torch.full_like(j, self.k)).reshape(-1)
            self._wpad = torch.zeros((self.k + 1, self.c_in // self.groups, self.c_out), device=dev)

    def _sn_tensors(self):
        """(weight_orig as (C_out, C_in / groups, k), u, v, wf) of a spectral layer for hipops.sn_step: wf is where `kernel_weights` reads the
        folded weight - the first k rows of wpad for the stacked forms, a buffer of the layer's own otherwise."""
        co, cig, k = self.c_out, self.c_in // self.groups, self.k
        if self.form in (_PHASES, _PLAIN):
            self._reindex_constants()
            wf = self._wpad[:k]
        else:
            if self._wf_sn is None or self._wf_sn.device != self.bias.device:
                self._wf_sn = torch.empty((k, cig, co), device=self.bias.device)
            wf = self._wf_sn
        return self.weight_orig.detach().reshape(co, cig, k), self.weight_u, self.weight_v, wf

    def kernel_weights(self) -> _Weights:
        """The `_Weights` of the current parameters.  Phase-stacked / plain form, with j - P = s*q + r:
        w4[g][q + Q][r * cig + c][o] = wf[s*q + r + P][c][g * cog + o]  (0 where the tap does not exist)."""
        key = self._key()
        # train mode refolds every call, as the reference's weight-norm / spectral-norm hooks do (and as the generator does): a
        # `.data` mutation (EMA swap, re-initialisation) bumps neither the pointer nor the version counter, so the cache is an
        # eval-mode optimisation only (`invalidate_weight_cache()` after a `.data` edit in eval mode)
        if self._cache is not None and self._cache[0] == key and not self.training:
            return self._cache[1]
        # inside ONE forward(y, y_hat) of a multi-discriminator the weight-normed layers fold once for both inputs (`_pairwise`): nothing
        # can change a parameter between the two calls, and at the reference's batch_size = 2 the ten-odd small launches of this function
        # per layer and call are most of a discriminator forward's wall clock.  (Spectral norm iterates u, v on EVERY call, as the legacy
        # hook does: never shared.)
        if _PAIR.on and not self.spectral and self._pair_rec is not None and self._pair_rec[0] == key:
            return self._pair_rec[1]
        k, s, P, G = self.k, self.stride, self.padding, self.groups
        cig, cog = self.c_in // G, self.c_out // G
        stacked = self.form in (_PHASES, _PLAIN)
        dev = self.bias.device
        if stacked:
            self._reindex_constants()
        wf = self._folded(self._wpad[:k] if stacked else None)            # [k][cig][co]
        if self.form == _TAPS:                               # rows (j, c): the taps become channels of a 1-tap conv
            w4 = torch.stack([wf.reshape(1, k * cig, self.c_out)], 0)
        elif self.form == _FIRST:                            # rows = taps
            w2 = torch.zeros((1, _UNFOLD_ROWS, self.c_out), device=dev)
            w2[0, :k] = wf[:, 0, :]
            w4 = torch.stack([w2], 0)
        else:
            w5 = self._wpad[self._jmap].reshape(self.kp, s * cig, G, cog)  # rows (r, c), columns (g, o)
            w4 = w5.permute(2, 0, 1, 3).contiguous()                       # [G][kp][s * cig][cog]
        rec = _Weights(w4, split=self.split_eligible(w4.shape[2], w4.shape[3]))
        self._cache = (key, rec)
        if _PAIR.on and not self.spectral:
            self._pair_rec = (key, rec)
        return rec

    def split_eligible(self, cigp, cog):
        """The split-f16 kernel serves this layer's stride-1 form: `cigp` stacked input channels and `cog` output channels per group."""
        return (self.precision == 'f16x3' and self.form in (_PHASES, _PLAIN) and self.kp >= 2 and hipops.split_supported(cigp, cog))

    def folded_grad(self, dws):
        """dwf [k][C_in / groups][C_out], the gradient wrt the folded weight, from the per-group weight gradients of the stride-1 form,
        dws[g] [kp][cs / G][C_out / G] (the inverse of `kernel_weights`' re-indexing)."""
        k, s, G = self.k, self.stride, self.groups
        co, cig = self.c_out, self.c_in // G
        dev = dws[0].device
        if self.form == _FIRST:
            dwf = dws[0][0, :k, :].reshape(k, 1, co)
        elif self.form == _TAPS:
            dwf = dws[0].reshape(k, cig, co)
        else:
            d5 = torch.stack(dws, 2).reshape(self.kp * s, cig, co)       # rows (q, r), then c; columns (g, o)
            dwf = torch.zeros((k + 1, cig, co), device=dev).index_add_(0, self._jmap, d5)[:k]
        return dwf.contiguous()

    def param_grads(self, db, dws, sn):
        """Gradients of this layer's parameters (parameters() order) from the bias gradient and the per-group weight gradients of the
        stride-1 form."""
        co, cig, k = self.c_out, self.c_in // self.groups, self.k
        dwf = self.folded_grad(dws)
        if not self.spectral:
            v, g = self.weight_v.detach(), self.weight_g.detach()
            dv, dg = hipops.wn_backward(dwf, v.reshape(co, cig, k), g.reshape(co, 1, 1), False)
            return [db, dg.reshape(g.shape), dv.reshape(v.shape)]
        # W = weight_orig / sigma, sigma = u^T W v with u, v constants (the power iteration runs under no_grad)
        w = self.weight_orig.detach()
        if isinstance(sn, _SnKept):        # one layer of the step's set (the discriminator's backward hands all of them over at once)
            dwfs = [None] * sn.plan.n
            dwfs[sn.index] = dwf
            return [db, hipops.sn_backward(sn.plan, sn.keep, dwfs)[sn.index].reshape(w.shape)]
        sigma, u, vv = sn
        dW = dwf.permute(2, 1, 0).reshape(w.shape)
        dot = (dW * w).sum() / (sigma * sigma)
        return [db, dW / sigma - dot * torch.outer(u, vv).reshape(w.shape)]


class _SnKept(NamedTuple):
    """What one native spectral-norm step leaves for its backward: the layer set's plan, the call's keep slab (sigma, u, v of every layer as
    the forward used them - the next call overwrites the buffers before this call's backward runs) and the layer's index in the set."""
    plan: 'hipops.SnPlan'
    keep: torch.Tensor
    index: int

    def values(self):
        """(sigma, u, v) of the layer, views of the slab."""
        return self.plan.keep_views(self.keep, self.index)


def _sn_prepare(layers):
    """NATIVE_SN: the spectral layers among `layers` whose `kernel_weights()` is about to fold (train mode: every call, with one power iteration,
    as the legacy hook; eval mode: only when the cached record is stale, and without one) take their step in ONE hipops.sn_step per mode;
    each finds its folded weight and its `_SnKept` in `_sn_ready`."""
    todo = [l for l in layers if l.spectral and (l.training or l._cache is None or l._cache[0] != l._key())]
    for training in (True, False):
        grp = [l for l in todo if l.training == training]
        if not grp:
            continue
        _check_cuda(*[l.bias for l in grp])
        tensors = [l._sn_tensors() for l in grp]
        plan, keep = hipops.sn_step(tensors, training)
        for i, (l, t) in enumerate(zip(grp, tensors)):
            l._sn_ready = (t[3], _SnKept(plan, keep, i))


def _check_cuda(*xs):
    for x in xs:
        if not x.is_cuda:
            raise RuntimeError('the discriminators run on the MI355X HIP path only (no CPU fallback)')


def _stacked_input(layer: _DiscConv, x, L_in, inner):
    """The stride-1 form's input of a layer above the first: x (B, C_in, pitch) activated feature-map buffer (valid [:L_in * inner]) ->
    xs (B, layer.cs, roundup4(layer.rows_out(L_in) * inner)): phases stacked, taps unfolded, or x itself with its tail zeroed."""
    if layer.form == _TAPS:
        return hipops.unfold_taps(x, L=L_in, inner=inner, s=layer.stride, k=layer.k, pad=layer.padding)
    if layer.form == _PHASES:
        return hipops.phase_split(x, L=L_in, inner=inner, s=layer.stride, cg=layer.c_in // layer.groups)
    return hipops.zero_tail(x, valid=L_in * inner)


def _unfold_first(layer: _DiscConv, x, H, inner):
    """The first layer's stride-1 input: x (B, 1, T) -> (B, 16, roundup4(layer.rows_out(H) * inner))."""
    if layer.rows_out(H) < 1:
        raise RuntimeError('discriminator input is shorter than the first kernel')
    return hipops.unfold1(x, H=H, inner=inner, s=layer.stride, k=layer.k, pad=layer.padding, rows=_UNFOLD_ROWS)


def _conv_split_or_exact(layer: _DiscConv, rec: _Weights, x, bias, out, inner, out_slope, dgrad):
    """The layer's stride-1 conv x (B, cs, P) -> out (B, C_out, P), or (`dgrad`) its input-gradient conv x = dz (B, C_out, P) -> out
    (B, cs, P) on the transposed, tap-flipped weights.  On the split-f16 kernel where the record has that form; a problem that
    kernel declines (V2W_E_SHAPE: a halo beyond its staging slots, another channel count per group) runs on the exact fp32 kernel, which
    overwrites whatever groups the declined launches wrote, and the record forgets the split weights: no re-pack, no retry.  A declined
    input-gradient problem is also remembered ON THE LAYER - records are rebuilt whenever a parameter version moves, i.e. after every
    optimizer step - so that later steps do not even pack for it."""
    dil = layer.dil(inner)
    if dgrad:
        exact = rec.transposed()
        declined = (layer.c_out // layer.groups, layer.cs // layer.groups, x.shape[2])
        split = rec.transposed_split(allowed=layer._no_split_dgrad != declined)
    else:
        exact, split = (rec.w4, rec.wp), rec.split()

    def run(w4, packs, algo):
        taps_left = w4.shape[1] - 1 - layer.Q if dgrad else layer.Q
        hipops.conv1d_groups(x, w4, bias, out, packs, dil=dil, pad_left=taps_left * dil, out_slope=out_slope, algo=algo)

    if split is not None:
        try:
            return run(*split, hipops.ALGO_SPLIT)
        except _hip.HipLibraryError as e:
            if e.code != _hip.E_SHAPE:
                raise
        rec.forget_split(dgrad)
        if dgrad:
            layer._no_split_dgrad = declined
    run(*exact, hipops.ALGO_AUTO)


def _conv_layer(layer: _DiscConv, rec, x, L_in, inner, out_slope):
    """x (B, C_in, pitch(L_in * inner)) -> (out buffer (B, C_out, pitch(U * inner)), U), U = L_out of the strided conv.  The convs
    run at L = pitch: the tail columns are ordinary positions to the kernel, hold zeros on the input side (phase_split / unfold
    fill them; `v2w_zero_tail` before a stride-1 layer reads a conv output directly) and are never part of the returned views."""
    xs = _stacked_input(layer, x, L_in, inner)
    out = torch.empty((x.shape[0], layer.c_out, xs.shape[2]), device=x.device)
    _conv_split_or_exact(layer, rec, xs, layer.bias.detach(), out, inner, out_slope, dgrad=False)
    return out, layer.rows_out(L_in)


def _first_layer(layer: _DiscConv, rec, x, H, inner):
    """C_in = 1: x (B, 1, T) -> activated buffer (B, C_out, pitch(U * inner)) through the unfolded 1-tap form."""
    xu = _unfold_first(layer, x, H, inner)
    out = torch.empty((x.shape[0], layer.c_out, xu.shape[2]), device=x.device)
    hipops.conv1d(xu, rec.w4[0], layer.bias.detach(), out, k=1, dil=1, slope=1.0, wp=rec.wp[0], out_slope=LRELU_SLOPE)
    return out, layer.rows_out(H)


class _DiscBase(nn.Module):
    """Shared driver of DiscriminatorP / DiscriminatorS: `inner` columns per row (the period, or 1)."""

    def _layers(self):
        return list(self.convs) + [self.conv_post]

    def _geometry(self, t):
        raise NotImplementedError

    def _chain(self):
        """(period, [(k, stride, pad) of every layer]): what `map_extents` walks, read from the layers themselves."""
        return getattr(self, 'period', 1), [(l.k, l.stride, l.padding) for l in self._layers()]

    def map_extents(self, n, pools=0):
        """Rows of each returned map (the score's are the last map's) that exist for an utterance of n samples, pure integers: n ->
        ceil(n / period) (a partly filled last row counts: the trimmed utterance's own reflect pad would fill it), `pools` times
        m -> m // 2 + 1 (AvgPool1d(4, 2, padding=2) in front of a scale discriminator), then m -> (m + 2 pad - k) // stride + 1 per layer.
        0 stays 0.  A map holds extent * period valid floats at the head of each (b, c) row."""
        period, layers = self._chain()
        return _chain_extents(int(n), period, pools, layers)

    def _run(self, x):
        """x (B, 1, T) -> state for the views / the backward: per layer (buffer (B, C, pitch), rows U) + the weights used."""
        b, c, t = x.shape
        inner, H = self._geometry(t)
        layers = self._layers()
        if NATIVE_SN:
            _sn_prepare(layers)                                 # spectral norm: the power iteration of this call, all layers in one step
        recs = [l.kernel_weights() for l in layers]             # (NATIVE_SN off: the power iteration of this call happens here)
        sn = [l._last_sn for l in layers]
        bufs = [_first_layer(layers[0], recs[0], x, H, inner)]
        for i in range(1, len(layers)):
            f, U = bufs[-1]
            bufs.append(_conv_layer(layers[i], recs[i], f, U, inner, LRELU_SLOPE if i + 1 < len(layers) else 0.0))
        return dict(bufs=bufs, recs=recs, sn=sn, inner=inner, H=H, T=t)

    def _views(self, st, b):
        inner = st['inner']
        if inner == 1:
            return [f[:, :, :U] for f, U in st['bufs']]
        return [f[:, :, :U * inner].view(b, f.shape[1], U, inner) for f, U in st['bufs']]      # strided when U * inner % 4 != 0

    @_hip.on_tensor_device
    def forward(self, x):
        _check_cuda(x)
        params = [p for l in self._layers() for p in l.parameters()]
        if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in params)):
            fmap = list(_DiscFn.apply(self, x, *params))
        else:
            with torch.no_grad():
                x = x.detach().contiguous().float()
                fmap = self._views(self._run(x), x.shape[0])
        return torch.flatten(fmap[-1], 1, -1), fmap


# ---- the backward of one layer, in the order it runs: dz and the bias gradient, the weight gradient, the input gradient
class _Down(NamedTuple):
    """What a layer's backward hands to the layer below: the gradient wrt that layer's activated map, as the pitched buffer `d`
    (s == 1), or still in the phase-stacked form (B, s * C, pitch) of a stride-s layer with `cg` channels per group - un-stacked
    inside the next disc_dz."""
    d: torch.Tensor
    cg: int
    s: int


def _dz_and_bias_grad(f, U, inner, g, down: Optional[_Down], slope, need_db):
    """f (B, C, P): a layer's activated map (U rows of `inner` columns valid), g: the gradient that arrived on its returned view (dense)
    or None, down: the one from the layer above or None -> (dz (B, C, P), the gradient wrt the conv's output; db (C,) or None)."""
    B, Cc, P = f.shape
    dz = torch.empty((B, Cc, P), device=f.device)
    rowsum = torch.empty((B, Cc), device=f.device) if need_db else None      # bias gradient partials from the same pass
    if down is not None and down.s > 1:
        hipops.disc_dz_merge(f, g, down.d, cg=down.cg, L=U, inner=inner, s=down.s, slope=slope, out=dz, rowsum=rowsum)
    else:
        hipops.disc_dz(f, g, None if down is None else down.d, valid=U * inner, slope=slope, out=dz, rowsum=rowsum)
    return dz, (hipops.rowsum_reduce(rowsum) if need_db else None)


def _weight_grad(layer: _DiscConv, xs, dz, inner):
    """xs (B, cs, P): the layer's stride-1 input, dz (B, C_out, P) -> the weight gradient in the stride-1 form, per group:
    [G] of [kp][cs / G][C_out / G] (`_DiscConv.param_grads` takes it back to the reference's parameters)."""
    assert xs.shape[1] == layer.cs and xs.shape[2] == dz.shape[2]
    if layer.c_out == 1:
        return [hipops.cout1_wgrad(xs, dz, k=layer.kp, dil=layer.dil(inner), tap0=layer.Q)]
    return list(hipops.wgrad_groups(xs, dz, groups=layer.groups, k=layer.kp, dil=layer.dil(inner), tap0=layer.Q).unbind(0))


def _input_grad(layer: _DiscConv, rec: _Weights, dz, inner) -> _Down:
    """dz (B, C_out, P) -> the gradient wrt the layer's stride-1 input (B, cs, P) - the forward conv kernel with the transposed,
    tap-flipped weights - as what flows to the layer below (the first layer: to `fold1`)."""
    if layer.form == _TAPS:
        raise NotImplementedError('backward of the unfolded-tap form (V2W_DISC_UNFOLD=1) is not built')
    dxs = torch.empty((dz.shape[0], layer.cs, dz.shape[2]), device=dz.device)
    _conv_split_or_exact(layer, rec, dz, None, dxs, inner, 0.0, dgrad=True)
    return _Down(dxs, layer.c_in // layer.groups, layer.stride if layer.form == _PHASES else 1)


class _DiscFn(torch.autograd.Function):
    """One discriminator call under autograd: forward = `_DiscBase._run`, backward below (the D step and the G step of
    train.py:188-215 both differentiate through it).  Inputs: x and every parameter in `_layers()` order."""

    @staticmethod
    def forward(ctx, disc, x, *params):
        xd = x.detach().contiguous().float()
        st = disc._run(xd)        # (the stride-1 layer inputs are rebuilt in the backward from the maps below them: -11 GB)
        views = tuple(disc._views(st, xd.shape[0]))
        # the maps go through save_for_backward, not a ctx attribute: autograd then releases them when the backward has run (unless
        # retain_graph) - as a plain attribute they lived as long as ANY tensor downstream of this call (train.py keeps `loss_disc_*` and the
        # score lists until the next iteration assigns them: the D step's 19.5 GB of maps stayed allocated through the whole G step)
        ctx.save_for_backward(xd, *[f for f, _u in st['bufs']])
        ctx.rows = [u for _f, u in st['bufs']]
        st['bufs'] = None
        ctx.disc, ctx.st = disc, st
        ctx.need_dx = x.requires_grad
        ctx.need_dw = any(p.requires_grad for p in params)
        return views

    @staticmethod
    @_hip.on_tensor_device
    def backward(ctx, *gouts):
        x, *maps = ctx.saved_tensors
        st, rows = ctx.st, ctx.rows
        layers = ctx.disc._layers()
        inner, H, T = st['inner'], st['H'], st['T']
        n = len(layers)
        grads = [None] * n           # per layer: its parameter gradients in parameters() order
        down, dx = None, None        # what flows into layer l from layer l + 1; the gradient wrt the audio
        sn_todo = []                 # (l, db, dwf, _SnKept) of the natively spectral-normed layers: their backward is one call, after the loop
        for l in reversed(range(n)):
            layer, rec, g = layers[l], st['recs'][l], gouts[l]
            if g is None and down is None:
                continue                                     # nothing flows through this layer (nor, so far, below it)
            if g is not None:
                g = g.contiguous().float()
            dz, db = _dz_and_bias_grad(maps[l], rows[l], inner, g, down, LRELU_SLOPE if l + 1 < n else 1.0, ctx.need_dw)
            down = None
            if ctx.need_dw:                   # (frozen discriminators - `frozen()` around the G step - skip all of this)
                # the layer's stride-1 input: rebuilt here, one streaming pass, and only when a weight gradient reads it - the forward
                # keeps the feature maps alone
                xs = _unfold_first(layer, x, H, inner) if l == 0 else _stacked_input(layer, maps[l - 1], rows[l - 1], inner)
                dws = _weight_grad(layer, xs, dz, inner)
                if isinstance(st['sn'][l], _SnKept):
                    sn_todo.append((l, db, layer.folded_grad(dws), st['sn'][l]))
                else:
                    grads[l] = layer.param_grads(db, dws, st['sn'][l])
            if l > 0:
                down = _input_grad(layer, rec, dz, inner)
            elif ctx.need_dx:
                dx = hipops.fold1(_input_grad(layer, rec, dz, inner).d, T=T, H=H, inner=inner, s=layer.stride, k=layer.k, pad=layer.padding)
        while sn_todo:               # the layers that shared a step share its backward
            kept = sn_todo[0][3]
            grp = [e for e in sn_todo if e[3].keep is kept.keep]
            sn_todo = [e for e in sn_todo if e[3].keep is not kept.keep]
            dwfs = [None] * kept.plan.n
            for _l, _db, dwf, sk in grp:
                dwfs[sk.index] = dwf
            dw = hipops.sn_backward(kept.plan, kept.keep, dwfs)
            for l, db, _dwf, sk in grp:
                grads[l] = [db, dw[sk.index].reshape(layers[l].weight_orig.shape)]
        flat = []
        for l in range(n):
            npar = len(list(layers[l].parameters()))
            flat.extend(grads[l] if grads[l] is not None else [None] * npar)
        return (None, dx, *flat)


def _chain_extents(n, period, pools, layers):
    m = -(-max(n, 0) // period)
    for _ in range(pools):
        m = m // 2 + 1 if m > 0 else 0
    out = []
    for k, stride, pad in layers:
        num = m + 2 * pad - k
        m = num // stride + 1 if m > 0 and num >= 0 else 0
        out.append(m)
    return out


class MapLengths:
    """What `MultiPeriodDiscriminator.map_lengths` / `MultiScaleDiscriminator.map_lengths` return and the three losses take as `lengths=`:
    `table`, int32 (rows, B) on the discriminator's device - the floats at the head of each (b, c) row that exist for item b (rows of the
    map x period) - and `B`.  Rows: one per feature map in the order the forward returns them (discriminator by discriminator:
    `maps`), then one per score (`scores`), then the score rows once more (`scores_twice`: the real and the generated scores of
    discriminator_loss in one table).  `counts[d]`: maps of discriminator d."""
    __slots__ = ('table', 'B', 'counts')

    def __init__(self, table, counts):
        self.table, self.B, self.counts = table, int(table.shape[1]), tuple(counts)
        assert table.dtype == torch.int32 and table.shape[0] == sum(counts) + 2 * len(counts)

    @property
    def maps(self):
        return self.table[:sum(self.counts)]

    @property
    def scores(self):
        n = sum(self.counts)
        return self.table[n:n + len(self.counts)]

    @property
    def scores_twice(self):
        return self.table[sum(self.counts):]

    def __repr__(self):
        return f'MapLengths(B={self.B}, maps={sum(self.counts)}, scores={len(self.counts)}, device={self.table.device})'


def _map_lengths(module, discs, pools, lengths, len_mul, L):
    """The MapLengths of `discs` (discriminator d behind pools[d] mean pools).  Host lengths: the integers of `map_extents`, one upload.
    Device lengths: one launch of v2w_map_extents from the lengths and the constant chain table of the module (cached per device and L)
    - nothing comes to the host."""
    B = lengths.numel() if torch.is_tensor(lengths) else len(lengths)
    src = mel.check_lengths(lengths, B, L, len_mul)
    len_mul = int(len_mul)
    chains = [d._chain() for d in discs]
    layers = chains[0][1]
    if any(c[1] != layers for c in chains):
        raise NotImplementedError('map_lengths: the discriminators of one module share their layers\' (k, stride, pad)')
    counts = [len(layers)] * len(discs)
    # rows {period, pools, depth, size}: the maps, the scores, the scores again; size: the rows of the map of an L-sample batch (0: no clip)
    sizes = [d.map_extents(L, pl) if L is not None else [0] * len(layers) for d, pl in zip(discs, pools)]
    rows = [(c[0], pl, j + 1, sz[j]) for c, pl, sz in zip(chains, pools, sizes) for j in range(len(layers))]
    score_rows = [(c[0], pl, len(layers), sz[-1]) for c, pl, sz in zip(chains, pools, sizes)]
    rows += score_rows + score_rows
    dev = src.device if src.is_cuda else next(module.parameters()).device
    if not src.is_cuda:
        cap = 2 ** 31 - 1 if L is None else int(L)
        table = [[min(_chain_extents(min(n * len_mul, cap), per, pl, layers[:depth])[-1], size or 2 ** 31) * per
                  for n in src.tolist()] for per, pl, depth, size in rows]
        return MapLengths(torch.tensor(table, dtype=torch.int32).reshape(len(rows), B).to(dev), counts)
    cache = module.__dict__.setdefault('_chain_tables', {})
    key = (str(dev), L)
    if key not in cache:
        cache[key] = (torch.tensor(rows, dtype=torch.int32).to(dev), torch.tensor(layers, dtype=torch.int32).to(dev))
    with torch.cuda.device(dev):
        table = hipops.map_extents(src.to(torch.int32).contiguous(), len_mul, 2 ** 31 - 1 if L is None else int(L), *cache[key])
    return MapLengths(table, counts)


class DiscriminatorP(_DiscBase):
    """models.py:158-193."""

    def __init__(self, period, kernel_size=5, stride=3, use_spectral_norm=False):
        super().__init__()
        if kernel_size != 5 or stride != 3:
            raise NotImplementedError('DiscriminatorP (HIP): the reference configuration kernel_size=5, stride=3')
        self.period = period
        self.convs = nn.ModuleList([_DiscConv(ci, co, k, s, 1, p, use_spectral_norm, True) for ci, co, k, s, p in DISC_P_LAYERS])
        ci, co, k, s, p = DISC_P_POST
        self.conv_post = _DiscConv(ci, co, k, s, 1, p, use_spectral_norm, True)

    def _geometry(self, t):
        p = self.period
        H = -(-t // p)                   # the reflect pad to a multiple of the period (models.py:176-181) happens inside unfold1
        if H * p - t >= t:
            raise RuntimeError('reflect padding needs an input longer than the pad')
        return p, H


class _PairState(threading.local):
    """`on`: this THREAD is inside a multi-discriminator's (y, y_hat) pairs (see _DiscConv.kernel_weights).  Thread-local and counted: replicas
    driven from several threads (DataParallel) or a nested call do not switch the sharing off under each other."""
    depth = 0

    @property
    def on(self):
        return self.depth > 0


_PAIR = _PairState()


# (y, y_hat) of a weight-normed discriminator as ONE call on the batch [y; y_hat] (the stacks hold no batch statistics: every sample's
# result is what the two calls give; the spectral-normed discriminator iterates u, v once per call and keeps its two calls).  Half the
# launches of a discriminator step's forwards and backwards, and no gradient accumulation over the two calls: train.py's own batch_size = 2 is
# launch-bound.  Only when the parameters ask for gradients - with frozen parameters the real half of two calls needs no backward at all.
# 'auto': up to _BATCH_PAIRS_MAX_SAMPLES input samples per half (above, the autograd slices of the split feature maps cost more than the launches).
BATCH_PAIRS = 'auto'
_BATCH_PAIRS_MAX_SAMPLES = 1 << 20
# The spectral-norm arithmetic of the first scale discriminator on the C ABI (hipops.sn_step / sn_backward: all layers of a call in four
# launches, their backward in two).  False: the torch lines of `_DiscConv._folded` / `param_grads` (mv, normalize, dot, outer), kept as the
# benchmark's A/B partner and the tests' second implementation.  Either way u, v advance once per call and spectral layers are never pair-shared.
NATIVE_SN = True


def _batch_pair(d, y, y_hat):
    if BATCH_PAIRS is False or y.shape != y_hat.shape or any(l.spectral for l in d._layers()):
        return False
    if not (torch.is_grad_enabled() and any(p.requires_grad for p in d.parameters())):
        return False
    return BATCH_PAIRS is True or y.numel() <= _BATCH_PAIRS_MAX_SAMPLES


def _pairwise(discs, inputs):
    """Run every discriminator on its (y, y_hat) pair -> (scores_real, scores_generated, fmaps_real, fmaps_generated)."""
    _PAIR.depth += 1
    try:
        outs = []
        for d, (y, y_hat) in zip(discs, inputs):
            if _batch_pair(d, y, y_hat):
                nb = y.shape[0]
                score, fmap = d(torch.cat([y, y_hat], 0))
                outs.append(((score[:nb], [f[:nb] for f in fmap]), (score[nb:], [f[nb:] for f in fmap])))
            else:
                outs.append((d(y), d(y_hat)))
    finally:
        _PAIR.depth -= 1
        for d in discs:
            for l in d._layers():
                l._pair_rec = None
    return ([r[0] for r, _ in outs], [g[0] for _, g in outs], [r[1] for r, _ in outs], [g[1] for _, g in outs])


class MultiPeriodDiscriminator(nn.Module):
    """models.py:196-216: one DiscriminatorP per period of `hp.periods`, each applied to y then y_hat."""

    def __init__(self, hp):
        super().__init__()
        self.discriminators = nn.ModuleList([DiscriminatorP(prd) for prd in hp.periods])

    def forward(self, y, y_hat):
        return _pairwise(self.discriminators, [(y, y_hat)] * len(self.discriminators))

    def map_lengths(self, lengths, len_mul=1, L=None):
        """The `MapLengths` of this module's maps and scores for a padded batch whose item b holds n_b = min(lengths[b] * len_mul, L)
        samples (`mel.check_lengths`' conventions; lengths: a list or an integer tensor on any device; L: the batch's samples - given, every
        extent is also clipped to the map's size, which the loss kernels do anyway).  See `feature_loss` for what the extents mean."""
        return _map_lengths(self, list(self.discriminators), [0] * len(self.discriminators), lengths, len_mul, L)


class DiscriminatorS(_DiscBase):
    """models.py:219-243."""

    def __init__(self, use_spectral_norm=False):
        super().__init__()
        self.convs = nn.ModuleList([_DiscConv(ci, co, k, s, g, p, use_spectral_norm, False) for ci, co, k, s, g, p in DISC_S_LAYERS])
        ci, co, k, s, g, p = DISC_S_POST
        self.conv_post = _DiscConv(ci, co, k, s, g, p, use_spectral_norm, False)

    def _geometry(self, t):
        return 1, t


class _AvgPoolFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        ctx.L = x.shape[2]
        return hipops.avgpool4(x.detach().contiguous().float())

    @staticmethod
    @_hip.on_tensor_device
    def backward(ctx, g):
        return hipops.avgpool4_bwd(g.contiguous().float(), L=ctx.L)


@_hip.on_tensor_device
def avg_pool(x):
    """AvgPool1d(4, 2, padding=2) of models.py:255-258 on (B, 1, L); differentiable."""
    _check_cuda(x)
    if torch.is_grad_enabled() and x.requires_grad:
        return _AvgPoolFn.apply(x)
    with torch.no_grad():
        return hipops.avgpool4(x.detach().contiguous().float())


class _MeanPool(nn.Module):
    def forward(self, x):
        return avg_pool(x)


class MultiScaleDiscriminator(nn.Module):
    """models.py:246-275: a spectral-normed and two weight-normed DiscriminatorS on the 1x, 1/2x, 1/4x mean-pooled audio."""

    def __init__(self):
        super().__init__()
        self.discriminators = nn.ModuleList([DiscriminatorS(use_spectral_norm=True), DiscriminatorS(), DiscriminatorS()])
        self.meanpools = nn.ModuleList([_MeanPool(), _MeanPool()])

    def forward(self, y, y_hat):
        pyramid = [(y, y_hat)]
        for pool in self.meanpools:
            pyramid.append((pool(pyramid[-1][0]), pool(pyramid[-1][1])))
        return _pairwise(self.discriminators, pyramid)

    def map_lengths(self, lengths, len_mul=1, L=None):
        """`MultiPeriodDiscriminator.map_lengths` for the three scales: discriminator j sits behind j mean pools."""
        return _map_lengths(self, list(self.discriminators), list(range(len(self.discriminators))), lengths, len_mul, L)


class frozen:
    """Context manager: the parameters of the given discriminators do not require grad inside.  train.py's generator step
    (train.py:201-215) back-propagates through MPD / MSD only to reach `y_g_hat`; the discriminator parameter gradients it also
    produces are discarded by the next `optim_d.zero_grad()`.  Wrapping that step's discriminator forwards in
    `with frozen(mpd, msd):` gives the same training trajectory while the real-audio branch needs no backward at all and the
    generated branch only its input gradients."""

    def __init__(self, *modules):
        self.params = [p for m in modules for p in m.parameters()]

    def __enter__(self):
        self.state = [p.requires_grad for p in self.params]
        for p in self.params:
            p.requires_grad_(False)
        return self

    def __exit__(self, *exc):
        for p, r in zip(self.params, self.state):
            p.requires_grad_(r)
        return False


class _L1MeanFn(torch.autograd.Function):
    """mean |real - fake| of one feature-map pair.  torch's own graph for `torch.mean(torch.abs(real - fake))` keeps the difference and its
    absolute value alive until the backward - two more tensors per feature map, 18 GB over the 2 x 48 maps of a generator step at
    B = 32 x 81 920 samples; here nothing but the two maps (alive anyway: they are what the discriminators return) is saved, the sign is
    rebuilt in the backward."""

    @staticmethod
    def forward(ctx, real, fake):
        ctx.save_for_backward(real, fake)
        return (real - fake).abs_().mean()

    @staticmethod
    def backward(ctx, g):
        real, fake = ctx.saved_tensors
        d = torch.sign(real - fake).mul_(g / real.numel())
        return (d if ctx.needs_input_grad[0] else None), (d.neg() if ctx.needs_input_grad[1] else None)


def set_precision(module, precision):
    """precision of the discriminator convs under `module` (a DiscriminatorP / DiscriminatorS / MultiPeriodDiscriminator /
    MultiScaleDiscriminator): 'f32' (exact, default) or 'f16x3' (see _DiscConv.precision)."""
    if precision not in ('f32', 'f16x3'):
        raise ValueError(f"discriminator precision must be 'f32' or 'f16x3', got {precision!r}")
    for m in module.modules():
        if isinstance(m, _DiscConv):
            m.precision = precision
            m.invalidate_weight_cache()
    return module


class _L1MultiFn(torch.autograd.Function):
    """scale * sum_i mean |a_i - b_i| over n map pairs (inputs: a_0 .. a_{n-1}, b_0 .. b_{n-1}) on the multi-tensor L1 kernels: the forward
    is one streaming and one finishing launch for all pairs, the backward one launch that writes only the sides that ask for a gradient
    and reads the incoming gradient on the device.  Like `_L1MeanFn` it saves nothing but the maps (alive anyway), which are read in place
    - pitched views and batch halves included (hipops.loss_rows)."""

    @staticmethod
    def forward(ctx, scale, n, *maps):
        ctx.scale, ctx.n = scale, n
        ctx.save_for_backward(*maps)
        return hipops.l1_mean_multi(list(zip(maps[:n], maps[n:])), scale)[1]

    @staticmethod
    @_hip.on_tensor_device
    def backward(ctx, g):
        maps, n = ctx.saved_tensors, ctx.n
        need = ctx.needs_input_grad[2:]
        da, db = hipops.l1_mean_multi_bwd(list(zip(maps[:n], maps[n:])), ctx.scale, g.contiguous(), need[:n], need[n:])
        return (None, None, *da, *db)


class _L1MultiLenFn(torch.autograd.Function):
    """`_L1MultiFn` over the counted floats of a padded batch: `ext` (n, B) rows of a MapLengths table, kept by reference for the backward."""

    @staticmethod
    def forward(ctx, scale, n, ext, *maps):
        ctx.scale, ctx.n, ctx.ext = scale, n, ext
        ctx.save_for_backward(*maps)
        return hipops.l1_mean_multi(list(zip(maps[:n], maps[n:])), scale, ext=ext)[1]

    @staticmethod
    @_hip.on_tensor_device
    def backward(ctx, g):
        maps, n = ctx.saved_tensors, ctx.n
        need = ctx.needs_input_grad[3:]
        da, db = hipops.l1_mean_multi_bwd(list(zip(maps[:n], maps[n:])), ctx.scale, g.contiguous(), need[:n], need[n:], ext=ctx.ext)
        return (None, None, None, *da, *db)


class _LsganLenFn(torch.autograd.Function):
    """`_LsganFn` over the counted floats of a padded batch (`ext`: the score rows of a MapLengths table)."""

    @staticmethod
    def forward(ctx, targets, ext, *scores):
        ctx.targets, ctx.ext = targets, ext
        ctx.save_for_backward(*scores)
        ctx.set_materialize_grads(False)
        terms, total = hipops.lsgan_multi(scores, targets, ext=ext)
        return total, terms

    @staticmethod
    def backward(ctx, g_total, g_terms):
        scores = ctx.saved_tensors
        if g_total is None and g_terms is None:
            return (None,) * (2 + len(scores))
        with torch.cuda.device(scores[0].device):
            ds = hipops.lsgan_multi_bwd(scores, ctx.targets, None if g_total is None else g_total.contiguous(),
                                        None if g_terms is None else g_terms.contiguous(), ctx.needs_input_grad[2:], ext=ctx.ext)
        return (None, None, *ds)


class _LsganFn(torch.autograd.Function):
    """(sum_i mean (t_i - s_i)^2, the n terms) of n score tensors with targets t_i in {0, 1}: one launch forward, one backward (gradients
    that arrive on the total and on single terms are added inside the kernel)."""

    @staticmethod
    def forward(ctx, targets, *scores):
        ctx.targets = targets
        ctx.save_for_backward(*scores)
        ctx.set_materialize_grads(False)
        terms, total = hipops.lsgan_multi(scores, targets)
        return total, terms

    @staticmethod
    def backward(ctx, g_total, g_terms):
        scores = ctx.saved_tensors
        if g_total is None and g_terms is None:
            return (None,) * (1 + len(scores))
        with torch.cuda.device(scores[0].device):
            ds = hipops.lsgan_multi_bwd(scores, ctx.targets, None if g_total is None else g_total.contiguous(),
                                        None if g_terms is None else g_terms.contiguous(), ctx.needs_input_grad[1:])
        return (None, *ds)


def _any_cpu(tensors):
    return any(not t.is_cuda for t in tensors)


def _lsgan(scores, targets, ext=None):
    """(total, terms (n,)) of the LSGAN terms of GPU score tensors: one launch per hipops.LOSS_MAX_ITEMS tensors."""
    cap = _hip.LOSS_MAX_ITEMS
    if ext is None:
        outs = [_LsganFn.apply(tuple(targets[i:i + cap]), *scores[i:i + cap]) for i in range(0, len(scores), cap)]
    else:
        outs = [_LsganLenFn.apply(tuple(targets[i:i + cap]), ext[i:i + cap], *scores[i:i + cap]) for i in range(0, len(scores), cap)]
    if len(outs) == 1:
        return outs[0]
    return sum(t for t, _ in outs), torch.cat([x for _, x in outs])


def _ext_rows(lengths, which, tensors, what):
    """The rows `which` ('maps', 'scores', 'scores_twice') of a MapLengths table for `tensors` (one row each), checked before anything is
    launched."""
    if not isinstance(lengths, MapLengths):
        raise TypeError(f'{what}: lengths must be the MapLengths of the discriminator that made the maps (its map_lengths(...))')
    rows = getattr(lengths, which)
    if rows.shape[0] != len(tensors):
        raise ValueError(f'{what}: {len(tensors)} tensors, but the MapLengths holds {rows.shape[0]} rows for them')
    for t in tensors:
        if t.dim() < 2 or t.shape[0] != lengths.B:
            raise ValueError(f'{what}: the MapLengths is of a batch of {lengths.B}, a tensor is {tuple(t.shape)}')
    if tensors and rows.device != tensors[0].device:
        rows = rows.to(tensors[0].device)
    return rows


def _masked_term(x, ext_row):
    """sum of x over the counted floats / their count (0 when there are none), in torch: x (B, C, ...) or (B, N), row (b, c) counts its
    first ext_row[b] floats - the definition the HIP kernels implement, for CPU tensors."""
    B = x.shape[0]
    x3 = x.reshape(B, 1, -1) if x.dim() == 2 else x.flatten(2)
    v = ext_row.to(torch.int64).clamp(0, x3.shape[2])
    on = torch.arange(x3.shape[2], device=x.device).view(1, 1, -1) < v.view(B, 1, 1)
    den = x3.shape[1] * int(v.sum())
    s = torch.where(on, x3, torch.zeros((), dtype=x.dtype, device=x.device)).sum()
    return s / den if den > 0 else s * 0


def l1_mean_loss(a, b):
    """mean |a - b| (F.l1_loss with the default reduction: the mel term of train.py:204), differentiable in both arguments; GPU tensors run
    on the multi-tensor L1 kernels as one pair."""
    if _any_cpu((a, b)):
        return F.l1_loss(a, b)
    if a.shape != b.shape:
        raise ValueError(f'l1_mean_loss: shapes differ: {tuple(a.shape)} and {tuple(b.shape)}')
    return _L1MultiFn.apply(1.0, 1, a, b)


def feature_loss(fmap_r, fmap_g, lengths=None):
    """2 x the sum over every feature map of mean |real - generated| (models.py:278-284).  GPU maps: all pairs of the call in one
    autograd.Function (hipops.LOSS_MAX_ITEMS pairs per launch); CPU maps: the torch expressions.

    lengths: the `MapLengths` of the discriminator that made the maps (`mpd.map_lengths(lengths, len_mul)`), for a padded batch of
    utterances of unequal lengths: every mean is over exactly the positions the utterance's own maps would have, and no position past them
    receives a gradient (+0.0 there).  The VALUES at the last few of those positions are those of the padded batch: a deeper layer's
    window there reaches into what the layer below computed past the utterance's end, where the trimmed utterance would see the conv's zero
    padding - the call is not claimed to equal the loss of the trimmed signals (the discriminator convs are not masked).  Apply
    `audio.mask_tail` to the generated batch first: the train-mode generator writes non-zero audio in the padding."""
    pairs = [(real, fake) for maps_r, maps_g in zip(fmap_r, fmap_g) for real, fake in zip(maps_r, maps_g)]
    ext = None if lengths is None else _ext_rows(lengths, 'maps', [r for r, _ in pairs], 'feature_loss')
    if lengths is not None:
        for real, fake in pairs:
            if real.shape != fake.shape:
                raise ValueError(f'feature_loss: shapes differ: {tuple(real.shape)} and {tuple(fake.shape)}')
    if not pairs or _any_cpu(t for p in pairs for t in p):
        if ext is not None:
            return 2 * sum(_masked_term((real - fake).abs(), ext[i]) for i, (real, fake) in enumerate(pairs))
        terms = [_L1MeanFn.apply(real, fake) for real, fake in pairs]
        return 2 * sum(terms)
    cap = _hip.LOSS_MAX_ITEMS
    if ext is not None:
        parts = [_L1MultiLenFn.apply(2.0, len(grp), ext[i:i + cap], *[r for r, _ in grp], *[f for _, f in grp])
                 for i, grp in ((i, pairs[i:i + cap]) for i in range(0, len(pairs), cap))]
        return parts[0] if len(parts) == 1 else sum(parts)
    parts = [_L1MultiFn.apply(2.0, len(grp), *[r for r, _ in grp], *[f for _, f in grp])
             for grp in (pairs[i:i + cap] for i in range(0, len(pairs), cap))]
    return parts[0] if len(parts) == 1 else sum(parts)


def discriminator_loss(disc_real_outputs, disc_generated_outputs, lengths=None):
    """LSGAN discriminator loss: sum over discriminators of mean (1 - D(y))^2 + mean D(y_hat)^2; also the per-discriminator
    values as Python floats (models.py:287-299).  GPU scores: one launch, and one device-to-host copy for all the floats.
    lengths: the `MapLengths` of the discriminator that made the scores - the means are over the positions each utterance's own score
    would have (see `feature_loss`)."""
    nr = min(len(disc_real_outputs), len(disc_generated_outputs))
    scores = list(disc_real_outputs[:nr]) + list(disc_generated_outputs[:nr])
    ext = None if lengths is None else _ext_rows(lengths, 'scores_twice', scores, 'discriminator_loss')
    if not scores or _any_cpu(scores):
        if ext is not None:
            real_terms = [_masked_term((1 - score) ** 2, ext[i]) for i, score in enumerate(scores[:nr])]
            fake_terms = [_masked_term(score ** 2, ext[nr + i]) for i, score in enumerate(scores[nr:])]
        else:
            real_terms = [torch.mean((1 - score) ** 2) for score in disc_real_outputs]
            fake_terms = [torch.mean(score ** 2) for score in disc_generated_outputs]
        total = sum(r + f for r, f in zip(real_terms, fake_terms))
        return total, [t.item() for t in real_terms], [t.item() for t in fake_terms]
    total, terms = _lsgan(scores, (1.0,) * nr + (0.0,) * nr, ext)
    vals = terms.detach().tolist()
    return total, vals[:nr], vals[nr:]


def generator_loss(disc_outputs, lengths=None):
    """LSGAN generator loss: sum over discriminators of mean (1 - D(y_hat))^2, and the terms (models.py:302-310).  GPU scores: one launch.
    lengths: as in `discriminator_loss`."""
    scores = list(disc_outputs)
    ext = None if lengths is None else _ext_rows(lengths, 'scores', scores, 'generator_loss')
    if not scores or _any_cpu(scores):
        if ext is not None:
            terms = [_masked_term((1 - score) ** 2, ext[i]) for i, score in enumerate(scores)]
        else:
            terms = [torch.mean((1 - score) ** 2) for score in disc_outputs]
        return sum(terms), terms
    total, terms = _lsgan(scores, (1.0,) * len(scores), ext)
    return total, list(terms.unbind(0))
