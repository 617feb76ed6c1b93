"""The planner of `Generator.forward` (reference: vec2wav/models.py:116-147): which C-ABI call serves which step, in which order, on which
stream.  One `ForwardPlanner` plans - and, through the hipops wrappers, launches - ONE forward; under a `schedule.Recorder` the launches are
taped as they go out and every later forward of the same configuration replays the tape (schedule.py).

    begin            bf16 activation storage or fp32 tensors (asked of the library's shape queries), the side stream forked
    weights          weight-norm folds, fragment packs, the conditioning chain: side-stream work in order of first use, an event per step
    conv_pre         models.py:123
    stage(i)         upsample (models.py:128-129) -> statistics (modules.py:23: batch sums, [all-reduce], folded affine) -> residual
                     (models.py:133-141: the first candidate that takes the stage runs it - one kernel with the next upsampler behind it, one
                     kernel, merged branch launches, layer by layer)
    tail             models.py:143-145 unless the last stage's kernel already ran it

A forward that will be back-propagated (`save`) gets every intermediate in a fresh buffer and no stage fusion (backward.py reads them)."""
from __future__ import annotations

import contextlib
import functools
from collections import namedtuple

import torch

from . import hipops

LRELU_SLOPE = 0.1  # models.py:10
POST_SLOPE = 0.01  # models.py:143 (F.leaky_relu's default, in front of conv_post)
_Z_CHANNEL = 128   # models.py:110


class DirectStreams:
    """The stream operations of a plan, executed and not taped (schedule.Recorder offers the same five and tapes them)."""

    def __init__(self, main, side, side2=None):
        self.main, self.side, self.side2 = main, side, side if side2 is None else side2
        self.events = {}
        self.nfork = 1
        self.tag = None

    def stream(self, sid):
        return (self.main, self.side, self.side2)[sid]

    def fork(self, sides=1):
        self.nfork = sides
        for q in (self.side, self.side2)[:sides]:
            q.wait_stream(self.main)

    def join(self):
        for q in (self.side, self.side2)[:self.nfork]:
            self.main.wait_stream(q)

    def mark(self, name, sid=1):
        ev = torch.cuda.Event()
        ev.record(self.stream(sid))
        self.events[name] = ev

    def need(self, name):
        self.main.wait_event(self.events[name])

    def py(self, fn, tag=None):
        return fn()

    def keep(self, obj):
        pass


STAGE_WINO_BLOCKS = [(3, 1, 3), (7, 1, 3), (11, 1, 3)]     # (kernel size, dilation 1, dilation 2) of the reference's ResBlock2 triple


def stage_wino_selected(wino_stage, precision, algo, C, blocks) -> bool:
    """Does the fused stage kernel run in its Winograd F(2,3) form (hipops.resblock2_stage_wino)?  Exact fp32 on the MFMA path, the
    32-channel stage, the standard block set - the one shape that form was measured on; everything else keeps the direct-form kernel.
    Read by the planner (rb2_stage_f32) and by the fold (Generator._wino_stage_layers: which layers get a Winograd stream)."""
    return bool(wino_stage) and precision == 'f32' and algo != hipops.ALGO_DIRECT and C == 32 and list(blocks) == STAGE_WINO_BLOCKS


def wino_sum_selected(wino_sum, precision, algo, C, blocks) -> bool:
    """Do the second convs of a wide ResBlock2 stage run as ONE Winograd launch on one accumulator (hipops.conv1d_wino_sum)?  Exact fp32 on
    the MFMA path, C in `wino_sum` (Generator.wino_sum: the stages that form was measured faster on), 2 or 3 branches of odd k >= 3 and one
    dilation.  `blocks`: (kernel size, second dilation) per branch.  Read by the planner (rb2_layers; the plain forward only) and by the
    fold (Generator._wino_sum_layers: which layers get a Winograd stream)."""
    blocks = list(blocks)
    return (C in tuple(wino_sum or ()) and precision == 'f32' and algo != hipops.ALGO_DIRECT and C % 64 == 0 and 2 <= len(blocks) <= 3
            and all(k >= 3 and k % 2 == 1 and d == blocks[0][1] for k, d in blocks))


def wino_fan_selected(wino_fan, precision, algo, C, blocks, *, save=False, lengths=False, streams=True) -> bool:
    """Do the FIRST convs of a ResBlock2 stage run as ONE Winograd launch that stages their common input once (hipops.conv1d_wino_fan)?
    Exact fp32 on the MFMA path, C in `wino_fan` (Generator.wino_fan), 1 to 3 branches of odd k >= 3 and one dilation, the plain forward
    only (`save`: the forward is back-propagated), no per-item `lengths`, and `streams`: every branch's `convs.0` has the Winograd stream
    `Generator.wino` folds.  `blocks`: (kernel size, first dilation) per branch.  Read by the planner (rb2_layers); the fold is asked for
    nothing.  The same bits either way: each conv runs the one-conv kernel's operations in its order."""
    blocks = list(blocks)
    return (C in tuple(wino_fan or ()) and precision == 'f32' and algo != hipops.ALGO_DIRECT and not save and not lengths and bool(streams)
            and 1 <= len(blocks) <= 3 and all(k >= 3 and k % 2 == 1 and d == blocks[0][1] for k, d in blocks))


def wino_up_shape(c_in, c_out, k, u) -> bool:
    """The transposed convs the upsampler form of the Winograd kernel serves (v2w_convt1d_wino_fwd): k == 2 u, so every output phase is a
    two-tap conv, u in (2, 4), 32-channel chunks, 64-row tiles of the u * C_out virtual rows."""
    return u in (2, 4) and k == 2 * u and c_in % 32 == 0 and c_in >= 64 and (u * c_out) % 64 == 0


def wino_up_selected(wino_up, i, precision, algo, c_in, c_out, k, u, *, save=False, lengths=False, stream=True) -> bool:
    """Does upsampler `i` run as ONE two-tap Winograd conv over u * C_out rows with a pixel-shuffle store (hipops.convt1d_wino: 3 products
    per output pair where the direct tile issues 4)?  Exact fp32 on the MFMA path, i in `wino_up` (Generator.wino_up: the upsamplers that
    form was measured faster on), a shape the kernel serves, the plain forward only (`save`: the forward is back-propagated), no per-item
    `lengths`, and `stream`: the fold has built the layer's Winograd stream.  Read by the planner (upsample) and, without the last three, by
    the fold (Generator._wino_up_layers).  The values differ from the direct tile's in the last bits."""
    return (i in tuple(wino_up or ()) and precision == 'f32' and algo != hipops.ALGO_DIRECT and wino_up_shape(c_in, c_out, k, u)
            and not save and not lengths and bool(stream))


class Stage(namedtuple('Stage', 'i C rbs names')):
    """Residual stage `i` of a generator (Generator.stage_record): its width, its num_kernels residual blocks and their parameter-name
    prefixes - and what the planner, the weight fold and the backward derive from them.  Where a method takes `n`: None means the two convs
    of a ResBlock2 (`convs.0`, `convs.1`), 0 .. 2 pair n of a ResBlock1 (`convs1.n`, `convs2.n`); `c` is 0 / 1, the conv of the pair."""
    __slots__ = ()

    def convs(self, c, n=None):
        return [rb.convs[c] if n is None else (rb.convs1, rb.convs2)[c][n] for rb in self.rbs]

    def dils(self, c, n=None):
        return [m.dilation for m in self.convs(c, n)]

    def pairs(self, c):
        """(kernel size, dilation of conv c) per branch: what wino_fan_selected (c = 0) and wino_sum_selected (c = 1) take."""
        return list(zip(self.ks, self.dils(c)))

    def layer(self, j, c, n=None):
        return f'{self.names[j]}.convs.{c}' if n is None else f'{self.names[j]}.convs{c + 1}.{n}'

    def layers(self, cs=(0, 1), n=None):
        return {self.layer(j, c, n) for j in range(len(self.rbs)) for c in cs}

    is_rb2 = property(lambda self: all(hasattr(rb, 'convs') for rb in self.rbs))     # (ResBlock2: `convs`; ResBlock1: `convs1` / `convs2`)
    ks = property(lambda self: [rb.kernel_size for rb in self.rbs])
    dil1s = property(lambda self: self.dils(0))
    dil2s = property(lambda self: self.dils(1))
    blocks = property(lambda self: list(zip(self.ks, self.dil1s, self.dil2s)))       # (k, dil1, dil2) per branch: what stage_wino_selected takes
    is_std = property(lambda self: self.is_rb2 and self.blocks == STAGE_WINO_BLOCKS)
    # the branch indices, heaviest kernel size first: the order of the problems of a merged launch, forward and backward
    heavy_first = property(lambda self: sorted(range(len(self.rbs)), key=lambda j: -self.rbs[j].kernel_size))

    def branches(self, w, key1, key2, n=None):
        """The per-branch dicts the stage and pair wrappers of hipops take: the two convs' weights out of `w` under `key1` / `key2`, b1, b2, k, dil1, dil2."""
        return [{key1: w[self.layer(j, 0, n)], 'b1': c1.bias.detach(), key2: w[self.layer(j, 1, n)], 'b2': c2.bias.detach(),
                 'k': rb.kernel_size, 'dil1': c1.dilation, 'dil2': c2.dilation}
                for j, (rb, c1, c2) in enumerate(zip(self.rbs, self.convs(0, n), self.convs(1, n)))]


class ForwardPlanner:
    def __init__(self, g, x, spk, nz, save, S, lens=None):
        self.g, self.x, self.spk, self.nz, self.save, self.S = g, x, spk, nz, save, S
        self.lens = lens           # per-item valid lengths (B,) int32 on the device, or None (Generator.forward(lengths=...))
        self.lmul = 1              # product of the upsample rates in front of the current layer: its input rate's len_mul
        self.dev = x.device
        self.B, _, self.T = x.shape
        self.training = g.training
        self.algo = g.algo
        self.nk, self.ns = g.num_kernels, g.num_upsamples
        self.marked = set()        # side-stream steps with an event behind them ...
        self.order = []            # ... (name, stream) in the order they were recorded
        self.needed = set()        # ... and the ones the main stream has already waited for

    # ---------------------------------------------------------------------------------------------------------------------------
    def run(self):
        g = self.g
        keep_ws = None
        if self.save is not None:
            keep_ws, g._ws = g._ws, {}
        try:
            with torch.no_grad():
                self.begin()
                self.weights()
                self.conv_pre()
                for i in range(self.ns):
                    self.stage(i)
                y = self.tail()
            if self.save is not None:
                self.hand_over(y)
        finally:
            if keep_ws is not None:
                g._ws = keep_ws
        return y

    def timed(self, tag, fn, *args, **kw):
        """Launch `fn` under `tag`: bench.py's roofline brackets the launches of a tag with events on the launching stream."""
        g = self.g
        self.S.tag = tag
        try:
            if g._profile is None or not isinstance(self.S, DirectStreams):
                return fn(*args, **kw)          # (a recorded plan is profiled at replay)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            pn = g._profile_names                # Generator.profile_kernel_names: also ask every launch of the tag for its kernel names
            e0.record()
            if pn is not None:
                from . import _hip, schedule
                prev = _hip.set_recorder(schedule.NameProbe(_hip.load(), pn.setdefault(tag, [])))
                try:
                    r = fn(*args, **kw)
                finally:
                    _hip.set_recorder(prev)
            else:
                r = fn(*args, **kw)
            e1.record()
            g._profile.append((tag, e0, e1))
            return r
        finally:
            self.S.tag = None

    def on_side(self, sid=1):
        return torch.cuda.stream(self.S.stream(sid))

    def mark(self, name, sid=1):
        self.S.mark(name, sid)
        self.marked.add(name)
        self.order.append((name, sid))

    def need(self, *names):
        """The main stream waits for these steps of the side streams - for nothing more, and for each stream at most once per call: the event
        behind a step of an in-order stream stands for every earlier step of that stream (`post` is behind `ups.0`, `rest` behind `ups.1`), so
        the latest of `names` on a stream is the one waited for and the earlier ones count as met (a wait costs the main queue ~3 us even when
        long satisfied: eight per forward before, five now)."""
        want = [nm for nm in names if nm in self.marked and nm not in self.needed]
        if not self.g.merge_waits:
            for nm in want:
                self.needed.add(nm)
                self.S.need(nm)
            return
        for sid in sorted({s for n, s in self.order if n in want}):
            seq = [n for n, s in self.order if s == sid]
            last = max(seq.index(n) for n in want if n in seq)
            self.S.need(seq[last])
            self.needed.update(seq[:last + 1])

    def join_side(self):
        if not self.joined:
            self.S.join()
            self.joined = True

    # ---------------------------------------------------------------------------------------------------------------------------
    def begin(self):
        """bf16 activation STORAGE (BASELINE configs[2] priced at 2 bytes per activation): every layer of the no-grad bf16 forward reads and
        writes bf16 tensors when all of them run on the bf16 kernels - wide stages C % 64 == 0, narrow stages 32 / 16 fused.  fp32 accumulate,
        fp32 BatchNorm statistics from the accumulators, fp32 output."""
        g, x = self.g, self.x
        from .models import ResBlock1, ResBlock2
        self.fuse_stage = () if self.save is not None else g.fuse_stage
        self.fuse_pairs = () if self.save is not None else g.fuse_pairs
        self.adt = torch.float32
        rb1_net = all(isinstance(rb, ResBlock1) for rb in g.resblocks)
        if (g.precision == 'bf16' and g.bf16_storage and self.save is None and self.algo == hipops.ALGO_AUTO and self.nk <= 3
                and (all(isinstance(rb, ResBlock2) for rb in g.resblocks) or rb1_net) and x.shape[2] % 4 == 0 and g.h.num_wv_feat % 32 == 0
                and all((up.out_channels >= 64 and up.out_channels % 64 == 0) or up.out_channels in self.fuse_stage for up in g.ups)
                and all(up.in_channels % 32 == 0 and 2 <= up.stride <= 8 for up in g.ups)
                and g._bf16_storage_kernels_exist(self.B, self.T)):
            self.adt = torch.bfloat16
        self.st = self.adt == torch.bfloat16
        # the conditioning chain (fcs -> spectral-norm step -> gamma / beta: three latency-bound launches, 70 - 125 us beside conv_pre) on a queue of
        # its own in the bf16-storage train-mode plan: behind it on ONE side stream the residual convs' fragments reached the first stage kernel
        # 35 us late (B = 32 x T = 256, round 6 trace)
        cs = g.cond_stream if g.cond_stream is not None else 3072 <= self.B * self.T <= 10240
        self.cond_sid = 2 if (self.st and self.training and cs) else 1
        self.joined = False
        self.S.fork(self.cond_sid)
        self.slab = g._slab(self.dev)
        self.y = None
        self.wps32 = {}
        self.up_done = None        # rows of bn.part{i} when the kernel of stage i - 1 already ran ups[i] (fuse_up)

    @functools.cached_property
    def stg(self):      # the record of the stage being planned: `stage` sets it, a planner stood up at one step of a stage builds it on first use
        return self.g.stage_record(self.stage_i)

    def buf(self, name, shape, dtype=torch.float32):
        return self.g._buf(name, shape, dtype=dtype, device=self.dev)

    def lkw(self, mul=None):
        """Keyword arguments of a launch that serves per-item lengths: none without them, else the lengths and the launch's len_mul (the
        product of the rates in front of its input)."""
        if self.lens is None:
            return {}
        return dict(lengths=self.lens, len_mul=self.lmul if mul is None else mul)

    def lkw_out(self):       # `lkw` at the current stage's OUTPUT rate: the residual convs run behind its upsampler
        return self.lkw(self.lmul * self.g.ups[self.stage_i].stride)

    def wino_streams(self, kind='wpw'):     # {layer: Winograd stream} the weight fold left under 'wpw' (Generator.wino), 'wpw_stage', 'wpw_sum', 'wpw_up'
        return self.g._fold_key.get(kind, {})

    # ---------------------------------------------------------------------------------------------------------------------------
    def weights(self):
        """K0 + K3.  bf16 storage: the side stream's work - conv_post's fold, ups.0's fragments, the conditioning chain (train mode at mid sizes:
        on the second side stream), the other upsamplers' fragments, the Conv1d batch - with an event behind ups.0, the conditioning chain and
        the last step, and the main stream waits for exactly the event its next launch needs (`need`): three waits per forward.  fp32: the folds run in front of conv_pre (8.55 against 8.65 ms with them beside it), the conditioning chain on the
        side stream, joined as late as its first use."""
        g, st, dev = self.g, self.st, self.dev
        B, ns = self.B, self.ns
        self.gbs = [self.buf(f'gb.{i}', (B, 2 * g.cbns[i].num_features)) for i in range(ns)]
        self.z_ws = self.buf('z_ws', (ns * B * _Z_CHANNEL,))
        self.sigma_ws = self.buf('sigma_ws', (ns,))
        self.affs = None
        self.cond_ran = False
        if self.cond_sid == 2:
            self.cond()                # its own queue: issued first, it runs beside everything below
        with (self.on_side() if st else contextlib.nullcontext()):
            self.wf, self.wp = g._fold_weights(dev, need_wf=self.save is not None, bf16_only=st)
        # (no event of its own behind conv_post's fold: it is the first thing on the side stream, the event behind ups.0 stands for it)
        self.wps = g._split_weights(dev, all_ups=st, ups_stream=self.S.side, mark=self.mark if st else None,
                                    between=self.cond if st else None)
        self.cond()

    def cond(self):
        """gamma / beta of every stage (depend on spk / noise only); spectral-norm u / v updated in train mode.  Eval-mode inference: gamma /
        beta, the running statistics and the fold into (a, s) of EVERY stage are one launch (v2w_cond_affine_eval); sigma = u^T W v depends
        on the parameters alone and is kept with the fold cache."""
        if self.cond_ran:
            return
        self.cond_ran = True
        g, dev, ns, B = self.g, self.dev, self.ns, self.B
        with self.on_side(self.cond_sid):
            if not self.training and self.save is None:
                sn_p = [q for c in g.cbns for q in (c.layer.weight_orig, c.layer.weight_u, c.layer.weight_v)]
                skey = (tuple((q.data_ptr(), q._version) for q in sn_p), str(dev))
                if g._fold_key.get('sigma') != skey:
                    hipops.cond_sigma([c.layer.weight_orig.detach() for c in g.cbns], [c.layer.weight_u for c in g.cbns],
                                      [c.layer.weight_v for c in g.cbns], self.sigma_ws, training=False)
                    g._fold_key['sigma'] = skey
                self.affs = [(self.buf(f'bn.a{i}', (B, g.cbns[i].num_features)), self.buf(f'bn.s{i}', (B, g.cbns[i].num_features))) for i in range(ns)]
                hipops.cond_affine_eval(
                    self.spk, self.nz, [f.weight.detach() for f in g.fcs], [f.bias.detach() for f in g.fcs],
                    [c.layer.weight_orig.detach() for c in g.cbns], [c.layer.bias.detach() for c in g.cbns], self.sigma_ws,
                    [c.batch_nrom.running_mean for c in g.cbns], [c.batch_nrom.running_var for c in g.cbns],
                    [c.batch_nrom.eps for c in g.cbns], [q[0] for q in self.affs], [q[1] for q in self.affs])
            else:
                g._fold_key.pop('sigma', None)        # (sigma_ws is about to hold this forward's own values)
                hipops.cond_gamma_beta(
                    self.spk, self.nz, [f.weight.detach() for f in g.fcs], [f.bias.detach() for f in g.fcs],
                    [c.layer.weight_orig.detach() for c in g.cbns], [c.layer.bias.detach() for c in g.cbns],
                    [c.layer.weight_u for c in g.cbns], [c.layer.weight_v for c in g.cbns], self.gbs, self.z_ws, self.sigma_ws, self.training)
        if self.st:
            self.mark('cond', self.cond_sid)

    def ck(self, nm, io=3):
        """Kernel choice of one Conv1d layer: bf16 / split-f16 fragments when prepared, else the f32 MFMA stream."""
        g = self.g
        if nm in self.wps32:
            return dict(algo=hipops.ALGO_BF16, wps=self.wps32[nm])
        if nm in self.wps and nm in g._split_wide:
            if self.st:       # bf16 storage: io bit 0 = the input tensor is bf16, bit 1 = out / res / addends are bf16
                return dict(algo=hipops.ALGO_BF16, wps=self.wps[nm], io_bf16=io)
            return dict(algo=hipops.ALGO_BF16 if g.precision == 'bf16' else hipops.ALGO_SPLIT, wps=self.wps[nm])
        if self.st:
            raise RuntimeError(f'bf16 storage: layer {nm} has no bf16 kernel (set generator.bf16_storage = False)')
        wpw = self.wino_streams().get(nm)
        if wpw is not None:     # the Winograd F(2,3) kernel, with this f32 MFMA stream for a launch it declines (hipops.conv1d_wino_multi)
            return dict(algo=self.algo, wp=self.wp[nm], wpw=wpw)
        return dict(algo=self.algo, wp=self.wp[nm])

    # ---------------------------------------------------------------------------------------------------------------------------
    def conv_pre(self):
        g = self.g
        self.cur = self.buf('act.pre', (self.B, g.h.upsample_initial_channel, self.T), dtype=self.adt)
        self.timed('conv_pre', hipops.conv1d, self.x, self.wf['conv_pre'], g.conv_pre.bias.detach(), self.cur, k=7, dil=1,
                   slope=1.0, splitk_ws=self.slab, **self.ck('conv_pre', io=2), **self.lkw())        # (the latents arrive as fp32)
        self.L = self.T

    def stage(self, i):
        self.stage_i, self.stg = i, self.g.stage_record(i)
        up = self.g.ups[i]
        self.C, self.Lo = up.out_channels, self.L * up.stride
        self.xr = self.buf(f'act.up{i}', (self.B, self.C, self.Lo), dtype=self.adt)
        nt_stats, part = self.upsample(i)
        self.aff = self.statistics(i, nt_stats, part)
        # (bf16 storage: the fragments of the residual convs, of the upsampler a fused stage kernel runs, of the tail)
        self.need('rest', f'ups.{i + 1}' if i + 1 < self.ns else 'post')
        self.xs = self.buf(f'act.rb{i}', (self.B, self.C, self.Lo), dtype=self.adt)
        self.residual(i)
        self.cur, self.L = self.xs, self.Lo
        self.lmul *= self.g.ups[i].stride

    def upsample(self, i):
        """K2: leaky_relu(0.1) -> ConvTranspose1d (+ the per-tile BatchNorm sums of its output)."""
        g, st, up, C = self.g, self.st, self.g.ups[i], self.C
        B, L, dev = self.B, self.L, self.dev
        if st:
            if self.up_done is None:
                self.need(f'ups.{i}')                       # this upsampler's fragments (the side stream packed them)
        elif f'ups.{i}' in self.wps:                        # the side stream holds this upsampler's packed weights (bf16 / f16x3 modes)
            self.join_side()
        part, nt_stats = None, 0
        wpw, nt_wino = self.wino_up(i)
        if self.training:
            # fused statistics: the MFMA transposed conv emits per-tile (sum, sumsq) from its accumulators
            if self.up_done is not None:
                nt_stats = self.up_done
            elif nt_wino:
                nt_stats = nt_wino
            elif f'ups.{i}' in self.wps:
                nt_stats = hipops.convt_bf16_stats_tiles(self.cur, self.xr, up.kernel_size, up.stride, io_bf16=3 if st else 0)
            elif self.algo != hipops.ALGO_DIRECT and self.wp[f'ups.{i}'] is not None:
                nt_stats = hipops.convt_stats_tiles(B, up.in_channels, C, L, up.kernel_size, up.stride)
            if nt_stats:
                part = self.buf(f'bn.part{i}', (nt_stats * C * 2,))
        if self.up_done is not None:
            pass        # the previous stage's kernel has written xr (and the partial sums): models.py:128-129 ran fused behind it
        elif nt_wino and self.timed(f'ups.{i}', hipops.convt1d_wino, self.cur, wpw, up.bias.detach(), self.xr, k=up.kernel_size, u=up.stride,
                                    slope=LRELU_SLOPE, stats_part=part):
            pass        # the upsampler form of the Winograd kernel took it
        elif nt_wino:   # ... declined it after all: today's launch, with its own partial rows
            if self.training:
                nt_stats = hipops.convt_stats_tiles(B, up.in_channels, C, L, up.kernel_size, up.stride)
                part = self.buf(f'bn.part{i}', (nt_stats * C * 2,)) if nt_stats else None
            self.timed(f'ups.{i}', hipops.convt1d, self.cur, self.wf[f'ups.{i}'], up.bias.detach(), self.xr, k=up.kernel_size,
                       u=up.stride, slope=LRELU_SLOPE, algo=self.algo, wp=self.wp[f'ups.{i}'], stats_part=part, splitk_ws=self.slab)
        elif f'ups.{i}' in self.wps and (nt_stats or not self.training):
            self.timed(f'ups.{i}', hipops.convt1d_bf16, self.cur, self.wps[f'ups.{i}'], up.bias.detach(), self.xr, k=up.kernel_size,
                       u=up.stride, slope=LRELU_SLOPE, stats_part=part, io_bf16=3 if st else 0)
        elif st:
            raise RuntimeError(f'bf16 storage: ups.{i} has no bf16 kernel (set generator.bf16_storage = False)')
        else:
            self.timed(f'ups.{i}', hipops.convt1d, self.cur, self.wf[f'ups.{i}'], up.bias.detach(), self.xr, k=up.kernel_size,
                       u=up.stride, slope=LRELU_SLOPE, algo=self.algo, wp=self.wp[f'ups.{i}'], stats_part=part, splitk_ws=self.slab, **self.lkw())
        self.up_done = None
        return nt_stats, part

    def wino_up(self, i):
        """(Winograd stream, position tiles) when upsampler i runs in the upsampler form of the Winograd kernel (wino_up_selected, the library
        takes the shape, and - the one-conv kernel's rule - the launch has more than 128 workgroups), else (None, 0): today's launch."""
        g, up = self.g, self.g.ups[i]
        wpw = self.wino_streams('wpw_up').get(f'ups.{i}')
        if (self.st or self.up_done is not None or f'ups.{i}' in self.wps
                or not wino_up_selected(g.wino_up, i, g.precision, self.algo, up.in_channels, up.out_channels, up.kernel_size, up.stride,
                                        save=self.save is not None, lengths=self.lens is not None, stream=wpw is not None)):
            return None, 0
        tiles, wgs = hipops.convt_wino_tiles(self.B, up.in_channels, up.out_channels, self.L, up.kernel_size, up.stride)
        return (wpw, tiles) if tiles and wgs > 128 else (None, 0)

    def statistics(self, i, nt_stats, part):
        """K4: batch statistics (train) -> [all-reduce] -> folded per-sample affine a, s (modules.py:20-30)."""
        g, C, B, Lo = self.g, self.C, self.B, self.Lo
        bn = g.cbns[i].batch_nrom
        # many thousands of partial rows, nothing to all-reduce, no backward that reads the array: the two-level form (below that the one-level
        # kernels keep four row loads in flight: one launch)
        sliced = self.training and nt_stats >= 4096 and g.stat_sync is None and self.save is None
        stats = None
        # ... hundreds of rows, nothing to all-reduce: the reduction and the finalisation as one launch
        fused = g.fuse_bn_finalize and self.training and not sliced and nt_stats and g.stat_sync is None and self.affs is None
        if self.training and not sliced:
            stats = self.buf(f'bn.stats{i}', (2 * C + 1,), dtype=torch.float64)
            if fused:
                pass
            elif nt_stats:
                hipops.bn_reduce_partials(part, nt_stats, C, B * Lo, stats)
            else:
                hipops.bn_stats(self.xr, stats, self.buf('bn.partial', (2 * max(C, 256) * 64,), dtype=torch.float64))
            if g.stat_sync is not None:
                sync = g.stat_sync
                self.timed(f'stat_sync.{i}', self.S.py, lambda: sync(stats))
        a_t, s_t = self.buf(f'bn.a{i}', (B, C)), self.buf(f'bn.s{i}', (B, C))
        self.need('cond')              # (bf16 storage: gamma / beta - or the eval-mode affines - are the side stream's second step)
        if not self.st:                # (fp32: the side stream only carries gamma / beta - joined as late as their first use, which
            self.join_side()           # matters at B = 1, where conv_pre is shorter than the conditioning chain)
        if sliced:
            sl = self.buf(f'bn.slices{i}', (hipops.BN_SLICES * 2 * C,), dtype=torch.float64)
            hipops.bn_reduce_finalize_slices(part, nt_stats, B * Lo, sl, self.gbs[i], bn.running_mean, bn.running_var, bn.num_batches_tracked,
                                             a_t, s_t, momentum=bn.momentum, eps=bn.eps)
        elif fused:
            hipops.bn_reduce_finalize(part, nt_stats, B * Lo, stats, self.gbs[i], bn.running_mean, bn.running_var, bn.num_batches_tracked,
                                      a_t, s_t, momentum=bn.momentum, eps=bn.eps)
        elif self.affs is None:
            hipops.bn_finalize(stats, self.gbs[i], bn.running_mean, bn.running_var, bn.num_batches_tracked, a_t, s_t,
                               training=self.training, momentum=bn.momentum, eps=bn.eps)
        return a_t, s_t

    # ---------------------------------------------------------------------------------------------------------------------------
    def residual(self, i):
        """K6 / K7: the num_kernels residual blocks read the same x = a * xr + s; their mean is the next input (models.py:133-141)."""
        g, nk, stg = self.g, self.nk, self.stg
        # a back-propagated forward in the bf16 arithmetic (fp32 tensors): the 32-channel stage's convs layer by layer on the bf16 kernel too
        # (32 x 256 tiles; fragments packed here from the folded weights - the arena holds this stage's in the fused kernel's unit order)
        self.wps32 = {}
        if (self.save is not None and g.precision == 'bf16' and not self.st and self.C == 32 and self.Lo % 4 == 0 and self.algo == hipops.ALGO_AUTO
                and stg.is_rb2 and all(k >= 3 and k % 2 == 1 for k in stg.ks)):
            for nm in [stg.layer(j, c) for j in range(nk) for c in (0, 1)]:
                self.wps32[nm] = hipops.pack_split(self.wf[nm], bf16=True)
        if not (self.algo != hipops.ALGO_DIRECT and nk <= 3):
            return self.residual_serial(i)
        B, C, Lo = self.B, self.C, self.Lo
        # The branches are independent until the final sum: conv n of ALL branches goes out as one launch (heaviest kernel size first); the
        # first nk - 1 branches end in their own buffers o_j and the last branch's final conv adds them in the reference's order
        # ((r0 + r1) + r2) / nk.
        self.t1s = [self.buf(f'act.t1_{i}_{j}', (B, C, Lo), dtype=self.adt) for j in range(nk)]
        self.outs = [self.buf(f'act.o_{i}_{j}', (B, C, Lo), dtype=self.adt) for j in range(nk - 1)] + [self.xs]
        if not stg.is_rb2:
            return self.residual1(i)
        self.all_wps = all(nm in self.wps for nm in stg.layers())
        self.all_wp = all(self.wp.get(nm) is not None for nm in stg.layers())
        for cand in (self.rb2_stage_with_upsampler, self.rb2_narrow_stage_split, self.rb2_wide_stage_bf16, self.rb2_stage_f32,
                     self.rb2_stage_small, self.rb2_pairs, self.rb2_branch_convs_bf16, self.rb2_layers):
            if cand(i):
                return
            if self.st and cand is self.rb2_wide_stage_bf16 and C in (16, 32):
                raise RuntimeError('bf16 storage: the fused narrow-stage kernel did not take this shape (set generator.bf16_storage = False)')

    def launch(self, tag_sfx, probs):
        lk = self.lkw_out()
        probs = [(j, (*pr[:4], {**pr[4], **lk})) for j, pr in (probs[j] for j in self.stg.heavy_first if j in probs)]
        tag = '+'.join(f'{self.stg.names[j]}.{tag_sfx}' for j, _ in probs)
        self.timed(tag, hipops.conv1d_multi, [pr for _, pr in probs], splitk_ws=self.slab)

    def final_kw(self, j):
        if j < self.nk - 1:
            return {}
        return dict(add=self.outs[:self.nk - 1], out_div=float(self.nk))

    def stage_tag(self, sfx=''):
        return 'stage:' + '+'.join(f'{nm}.0&1' for nm in self.stg.names) + sfx

    def branch_tag(self, c):       # tag of the one launch that runs conv c of every branch
        return f'bconv{c}:' + '+'.join(f'{nm}.{c}' for nm in self.stg.names)

    def post_args(self):
        """The `post=` tuple of a stage kernel that runs the generator's tail (models.py:143-145) behind the last stage; y is allocated here."""
        y = torch.empty((self.B, 1, self.Lo), device=self.dev, dtype=torch.float32)
        return self.wf['conv_post'], self.g.conv_post.bias.detach(), y, self.g.conv_post.kernel_size, POST_SLOPE

    def rb2_stage_with_upsampler(self, i):
        """The stage with the NEXT stage's upsampler behind it in one kernel (bf16 tensors): xs is never written, the kernel stores
        act.up{i+1} and the BatchNorm partial sums of stage i + 1."""
        g, C, B, Lo, stg = self.g, self.C, self.B, self.Lo, self.stg
        if not (self.st and g.fuse_up and i + 1 < self.ns and C >= 32 and (C >= 64 and g.fuse_wide_stage or C in self.fuse_stage)
                and f'ups.{i + 1}' in self.wps and self.all_wps):
            return False
        nup = g.ups[i + 1]
        if not (nup.kernel_size == 2 * nup.stride and nup.stride in (2, 4) and nup.out_channels * 2 == C):
            return False
        ntn = hipops.resblock2_stage_up_tiles(B, C, Lo, stg.ks, stg.dil1s, stg.dil2s, slope=LRELU_SLOPE,
                                              up_k=nup.kernel_size, up_u=nup.stride, up_slope=LRELU_SLOPE)
        if not ntn:
            return False
        xr_n = self.buf(f'act.up{i + 1}', (B, nup.out_channels, Lo * nup.stride), dtype=self.adt)
        part_n = self.buf(f'bn.part{i + 1}', (ntn * nup.out_channels * 2,)) if self.training else None
        ok = self.timed(self.stage_tag(f'+ups.{i + 1}'), hipops.resblock2_stage_split, self.xr, self.aff, stg.branches(self.wps, 'wps1', 'wps2'), None,
                        slope=LRELU_SLOPE, out_div=float(self.nk), bf16=True, io_bf16=3,
                        up=(self.wps[f'ups.{i + 1}'], nup.bias.detach(), xr_n, part_n, nup.kernel_size, nup.stride, LRELU_SLOPE))
        if ok:
            self.up_done = ntn
        return ok

    def rb2_narrow_stage_split(self, i):
        """C = 32 / 16 on split / bf16 fragments: the whole residual section as one kernel - on bf16 tensors the last (16-channel) stage with
        the generator's tail behind it (models.py:143-145): the stage's output never leaves the chip, y is written instead."""
        g, C = self.g, self.C
        if not (C in (16, 32) and C in self.fuse_stage and self.all_wps):
            return False
        branches = self.stg.branches(self.wps, 'wps1', 'wps2')
        # (the reference's block set and 7-tap tail: the weights-in-registers kernel takes them; any other set / k <= 9 tail would run on the
        # resident-tile template, measured slower than the two kernels: only with fuse_post = 'any')
        kp = g.conv_post.kernel_size
        if self.st and g.fuse_post and i == self.ns - 1 and C == 16 and kp <= 9 and ((self.stg.is_std and kp == 7) or g.fuse_post == 'any'):
            post = self.post_args()
            if self.timed(self.stage_tag('+conv_post'), hipops.resblock2_stage_split, self.xr, self.aff, branches, None, slope=LRELU_SLOPE,
                          out_div=float(self.nk), bf16=True, io_bf16=3, post=post):
                self.y = post[2]
                return True
        return self.timed(self.stage_tag(), hipops.resblock2_stage_split, self.xr, self.aff, branches, self.xs, slope=LRELU_SLOPE,
                          out_div=float(self.nk), bf16=g.precision == 'bf16', io_bf16=3 if self.st else 0)

    def rb2_wide_stage_bf16(self, i):
        """A wide stage on bf16 tensors: the WHOLE residual section in one kernel (v2w_stage_bf16_wide.hip): x read once, t1_j on chip, one fp32
        accumulator over the branches."""
        g = self.g
        if not (self.st and g.fuse_wide_stage and self.C >= 64 and self.all_wps):
            return False
        return self.timed(self.stage_tag(), hipops.resblock2_stage_split, self.xr, self.aff, self.stg.branches(self.wps, 'wps1', 'wps2'), self.xs,
                          slope=LRELU_SLOPE, out_div=float(self.nk), bf16=True, io_bf16=3)

    def rb2_stage_f32(self, i):
        """The whole residual section of a narrow stage in ONE f32-MFMA kernel: x read once, t1_j in LDS, sum in registers - the last
        (16-channel) stage with the generator's tail behind it (models.py:143-145; round 5): its output is neither written nor read back."""
        g = self.g
        if self.st or not (self.C in self.fuse_stage and self.all_wp):
            return False
        lk, stg, wpw = self.lkw_out(), self.stg, self.wino_streams('wpw_stage')
        if all(nm in wpw for nm in stg.layers()) and stage_wino_selected(g.wino_stage, g.precision, self.algo, self.C, stg.blocks):
            # the Winograd F(2,3) form (its streams come from the same fold); a launch it declines runs on the direct form below
            if self.timed(self.stage_tag(), hipops.resblock2_stage_wino, self.xr, self.aff, stg.branches(wpw, 'wpw1', 'wpw2'), self.xs,
                          slope=LRELU_SLOPE, out_div=float(self.nk), **lk):
                return True
        branches = stg.branches(self.wp, 'wp1', 'wp2')
        kp = g.conv_post.kernel_size
        if g.fuse_post and i == self.ns - 1 and self.C == 16 and kp <= 9 and kp % 2 == 1 and g.conv_post.in_channels == 16:
            post = self.post_args()
            if self.timed(self.stage_tag('+conv_post'), hipops.resblock2_stage, self.xr, self.aff, branches, None, slope=LRELU_SLOPE,
                          out_div=float(self.nk), post=post, **lk):
                self.y = post[2]
                return True
        return self.timed(self.stage_tag(), hipops.resblock2_stage, self.xr, self.aff, branches, self.xs, slope=LRELU_SLOPE, out_div=float(self.nk),
                          **lk)

    def rb2_stage_small(self, i):
        """8 channels (the sixth stage of a x640 generator): below every MFMA tile - the whole section as one FMA kernel."""
        if not (self.C == 8 and 8 in self.fuse_stage and not self.st and self.nk <= 4
                and all(self.wf.get(nm) is not None for nm in self.stg.layers())):
            return False
        return self.timed(self.stage_tag(), hipops.resblock2_stage_small, self.xr, self.aff, self.stg.branches(self.wf, 'wf1', 'wf2'), self.xs,
                          slope=LRELU_SLOPE, out_div=float(self.nk))

    def launch_pairs(self, tag_sfx, probs):
        """probs: {j: dict}; the first nk - 1 branches in one launch, the summing branch after them."""
        nk, done = self.nk, True
        for js in ([j for j in self.stg.heavy_first if j in probs and j < nk - 1], [nk - 1] if nk - 1 in probs else []):
            if js and done:
                done = self.timed('+'.join(f'{self.stg.names[j]}.{tag_sfx}' for j in js), hipops.resblock_pair_multi, [probs[j] for j in js])
        return done

    def fused_pair_ok(self, n=None):
        return (self.lens is None and not self.st and self.C in self.fuse_pairs and self.C in (16, 32)
                and all(self.wp.get(nm) is not None for nm in self.stg.layers(n=n)))

    def pair_problems(self, srcs, src_aff, dsts, res_mode, n=None, last=True):
        """{j: problem dict of hipops.resblock_pair_multi}: both convs of a ResBlock2 branch (`n` None) or pair n of a ResBlock1 branch."""
        return {j: dict(br, x=srcs[j], in_affine=src_aff, out=dsts[j], res_mode=res_mode, slope=LRELU_SLOPE, **(self.final_kw(j) if last else {}))
                for j, br in enumerate(self.stg.branches(self.wp, 'wp1', 'wp2', n))}

    def rb2_pairs(self, i):
        """Narrow stages (C = 32 / 16): both convs of a pair in ONE kernel, the intermediate stays in LDS."""
        if not self.fused_pair_ok():
            return False
        return self.launch_pairs('0&1', self.pair_problems([self.xr] * self.nk, self.aff, self.outs, res_mode=0))

    def conv_problems(self, c, srcs, dsts, extra, n=None):
        """{j: (j, problem of hipops.conv1d_multi)}: conv c of every branch (`n`: of pair n of a ResBlock1); extra(j): the launch's other keywords."""
        stg = self.stg
        return {j: (j, (srcs[j], self.wf[stg.layer(j, c, n)], m.bias.detach(), dsts[j],
                        dict(k=stg.ks[j], dil=m.dilation, slope=LRELU_SLOPE, **extra(j), **self.ck(stg.layer(j, c, n)))))
                for j, m in enumerate(stg.convs(c, n))}

    def conv2_problems(self):
        return self.conv_problems(1, self.t1s, self.outs, lambda j: dict(res=self.t1s[j], **self.final_kw(j)))

    def launch_conv2(self, sfx, conv2):
        nk = self.nk
        if nk > 1:
            self.launch(sfx, {j: conv2[j] for j in range(nk - 1)})
        self.launch(sfx, {nk - 1: conv2[nk - 1]})

    def rb2_branch_convs_bf16(self, i):
        """A wide stage on bf16 tensors the one-kernel form declined: the first convs of all branches in ONE launch (x staged once), then the
        second convs in one launch on one accumulator (v2w_branch_convs_bf16_fwd; o_j never written)."""
        g, stg, nk = self.g, self.stg, self.nk
        if not (self.st and g.fuse_wide and self.C >= 64 and self.all_wps):
            return False
        frags, biases = ([[self.wps[stg.layer(j, c)][0] for j in range(nk)] for c in (0, 1)],
                         [[m.bias.detach() for m in stg.convs(c)] for c in (0, 1)])
        if not self.timed(self.branch_tag(0), hipops.branch_convs_bf16, 0, [self.xr], self.aff, frags[0], biases[0], self.t1s,
                          stg.ks, stg.dil1s, slope=LRELU_SLOPE):
            return False
        if not self.timed(self.branch_tag(1), hipops.branch_convs_bf16, 1, self.t1s, None, frags[1], biases[1], [self.xs],
                          stg.ks, stg.dil2s, slope=LRELU_SLOPE, out_div=float(nk)):
            self.launch_conv2('1', self.conv2_problems())
        return True

    def rb2_layers(self, i):
        """Layer by layer: conv1 of the three branches in ONE launch, conv2 of branches 0 .. nk - 2 in one, the last branch's conv2 adds them."""
        if not self.conv1_fan():
            self.launch('0', self.conv_problems(0, [self.xr] * self.nk, self.t1s, lambda j: dict(in_affine=self.aff, res=self.xr, res_affine=self.aff)))
        if not self.conv2_sum():
            self.launch_conv2('1', self.conv2_problems())
        return True

    def conv1_fan(self):
        """The first convs of all branches as one Winograd launch that stages x once per tile (each t1_j the bits of its own launch); False:
        not selected or declined - rb2_layers then issues the multi-problem launch."""
        g, stg, wpw = self.g, self.stg, self.wino_streams()
        if self.st or not wino_fan_selected(g.wino_fan, g.precision, self.algo, self.C, stg.pairs(0),
                                            save=self.save is not None, lengths=self.lens is not None,
                                            streams=all(nm in wpw for nm in stg.layers((0,)))):
            return False
        return self.timed(self.branch_tag(0), hipops.conv1d_wino_fan, self.xr,
                          [(wpw[stg.layer(j, 0)], c1.bias.detach(), self.t1s[j], stg.ks[j]) for j, c1 in enumerate(stg.convs(0))],
                          dil=stg.dil1s[0], slope=LRELU_SLOPE, in_affine=self.aff, res=self.xr, res_affine=self.aff,
                          only_if_multi_wino=True)

    def conv2_sum(self):
        """The second convs of all branches as one Winograd launch on one accumulator (o_j never written); False: not selected or declined."""
        g, stg = self.g, self.stg
        # (wino_sum: stages the fold gives streams of their own; wino_sum_wide: stages that reuse the streams `wino` folds - none without it)
        listed = tuple(g.wino_sum or ()) + tuple(g.wino_sum_wide or ())
        if self.save is not None or self.st or not wino_sum_selected(listed, g.precision, self.algo, self.C, stg.pairs(1)):
            return False
        wpw = {**self.wino_streams('wpw_sum'), **self.wino_streams()}
        if not all(nm in wpw for nm in stg.layers((1,))):
            return False
        return self.timed(self.branch_tag(1), hipops.conv1d_wino_sum,
                          [(self.t1s[j], wpw[stg.layer(j, 1)], c2.bias.detach(), stg.ks[j]) for j, c2 in enumerate(stg.convs(1))],
                          self.xs, dil=stg.dil2s[0], slope=LRELU_SLOPE, out_div=float(self.nk), **self.lkw_out())

    # ---------------------------------------------------------------------------------------------------------------------------
    def residual1(self, i):
        """ResBlock1 (models.py:37-44): three (dilated conv, conv) pairs per branch, merged over the branches."""
        nk, B, C, Lo, stg = self.nk, self.B, self.C, self.Lo, self.stg
        xas = [self.buf(f'act.xa_{i}_{j}', (B, C, Lo), dtype=self.adt) for j in range(nk)]
        xbs = [self.buf(f'act.xb_{i}_{j}', (B, C, Lo), dtype=self.adt) for j in range(nk)]
        srcs, src_aff, t1s = [self.xr] * nk, self.aff, self.t1s
        for n in range(3):
            dsts = [xas, xbs, self.outs][n]
            if self.save is not None:   # backward needs every sub-block's conv1 output: one buffer per n
                t1s = [self.buf(f'act.t1_{i}_{j}_{n}', (B, C, Lo)) for j in range(nk)]
            last_kw = (lambda j: self.final_kw(j)) if n == 2 else (lambda j: {})
            if self.st and hipops.resblock1_pairs_ok(B, C, Lo, stg.ks, stg.dils(0, n), stg.dils(1, n), slope=LRELU_SLOPE):
                # bf16 tensors: pair n of every branch as one resident-tile launch - the dilated conv's output stays in LDS, the pair's residual
                # joins the output - and the last pair of the last branch adds the other branches' results.  (A pair whose resident tiles do not
                # fit - 256 channels at dilation 5 - runs conv by conv on the chunked bf16 kernel below, still on bf16 tensors.)
                brs = stg.branches(self.wps, 'wps1', 'wps2', n)
                for js in ([list(range(nk))] if n < 2 or nk == 1 else [list(range(nk - 1)), [nk - 1]]):
                    last = n == 2 and js[-1] == nk - 1
                    tag = 'rb1:' + '+'.join(f'{stg.names[j]}.{2 * n}&{2 * n + 1}' for j in js)
                    if not self.timed(tag, hipops.resblock1_pairs_bf16, [srcs[j] for j in js], src_aff, [brs[j] for j in js], [dsts[j] for j in js],
                                      slope=LRELU_SLOPE, out_div=float(nk) if last else 0.0, add=self.outs[:nk - 1] if last and nk > 1 else None):
                        raise RuntimeError('bf16 storage: the ResBlock1 pair kernel declined a shape its query accepted')
                srcs, src_aff = dsts, None
                continue
            ok = False
            if self.fused_pair_ok(n):
                ok = self.launch_pairs(f'{2 * n}&{2 * n + 1}', self.pair_problems(srcs, src_aff, dsts, res_mode=1, n=n, last=n == 2))
            if not ok:
                self.launch(str(2 * n), self.conv_problems(0, srcs, t1s, lambda j: dict(in_affine=src_aff), n))
                conv2 = self.conv_problems(1, t1s, dsts, lambda j: dict(res=srcs[j], res_affine=src_aff, **last_kw(j)), n)
                if n < 2:
                    self.launch(str(2 * n + 1), conv2)
                else:
                    self.launch_conv2('5', conv2)
            srcs, src_aff = dsts, None

    def residual_serial(self, i):
        """Branch after branch, conv after conv (the scalar cross-check kernels, or more than three branches): `xs` accumulates."""
        from .models import ResBlock2
        g, nk, B, C, Lo = self.g, self.nk, self.B, self.C, self.Lo
        t1 = self.buf(f'act.t1_{i}', (B, C, Lo))
        for j, (rb, name) in enumerate(zip(self.stg.rbs, self.stg.names)):
            k = rb.kernel_size
            last = dict(accumulate=(j > 0), out_div=(float(nk) if j == nk - 1 else 0.0))
            if isinstance(rb, ResBlock2):
                c1, c2 = rb.convs[0], rb.convs[1]
                self.timed(name + '.0', hipops.conv1d, self.xr, self.wf[name + '.convs.0'], c1.bias.detach(), t1, k=k, dil=c1.dilation,
                           slope=LRELU_SLOPE, in_affine=self.aff, res=self.xr, res_affine=self.aff, splitk_ws=self.slab, **self.ck(name + '.convs.0'))
                self.timed(name + '.1', hipops.conv1d, t1, self.wf[name + '.convs.1'], c2.bias.detach(), self.xs, k=k, dil=c2.dilation,
                           slope=LRELU_SLOPE, res=t1, splitk_ws=self.slab, **self.ck(name + '.convs.1'), **last)
                continue
            xa, xb = self.buf(f'act.xa_{i}', (B, C, Lo)), self.buf(f'act.xb_{i}', (B, C, Lo))
            src, src_aff, dsts = self.xr, self.aff, [xa, xb, self.xs]
            for n in range(3):
                c1, c2 = rb.convs1[n], rb.convs2[n]
                self.timed(f'{name}.{2 * n}', hipops.conv1d, src, self.wf[f'{name}.convs1.{n}'], c1.bias.detach(), t1, k=k, dil=c1.dilation,
                           slope=LRELU_SLOPE, in_affine=src_aff, splitk_ws=self.slab, **self.ck(f'{name}.convs1.{n}'))
                self.timed(f'{name}.{2 * n + 1}', hipops.conv1d, t1, self.wf[f'{name}.convs2.{n}'], c2.bias.detach(), dsts[n], k=k, dil=1,
                           slope=LRELU_SLOPE, res=src, res_affine=src_aff, splitk_ws=self.slab, **self.ck(f'{name}.convs2.{n}'),
                           **(last if n == 2 else {}))
                src, src_aff = dsts[n], None

    # ---------------------------------------------------------------------------------------------------------------------------
    def tail(self):
        """K8: leaky_relu(0.01) -> conv_post -> tanh (unless the last stage's kernel has already done it)."""
        g = self.g
        if self.st:
            # bf16 storage: every launch on a side stream has an event behind it (weights(), cond()); when the main stream has waited for all of
            # them - and every forked stream has one, so each has rejoined - there is nothing left to join (two waits on the main queue less)
            forked = range(1, 1 + self.cond_sid)
            if not (self.g.merge_waits and self.marked <= self.needed and all(any(s == sid for _n, s in self.order) for sid in forked)):
                self.S.join()    # (whatever step nobody asked for; the side streams have long finished)
        elif not self.joined:
            self.S.join()
        if self.y is None:
            self.y = torch.empty((self.B, 1, self.L), device=self.dev, dtype=torch.float32)
            self.timed('conv_post', hipops.conv_post_tanh, self.cur, self.wf['conv_post'], g.conv_post.bias.detach(), self.y, k=7, slope=POST_SLOPE,
                       **self.lkw())
        return self.y

    def hand_over(self, y):
        """What backward.py reads: this forward's buffers, folded weights and the spectral-norm vectors AS THIS FORWARD LEFT THEM (the backward
        of sigma = u^T W v must not see a later forward's power-iteration step)."""
        g, save = self.g, self.save
        save['sn_uv'] = [(c.layer.weight_u.detach().clone(), c.layer.weight_v.detach().clone()) for c in g.cbns]
        save.update(ws=g._ws, wf=self.wf, wp=self.wp, wpd=g._fold_key.get('wpd', {}), vers=g._fold_key.get('vers'), gen=g._fold_key.get('gen'),
                    y=y, x=self.x, spk=self.spk, nz=self.nz, training=self.training, B=self.B, T=self.T)
        g._fold_key.pop('state', None)     # the cached fold pointed into the handed-over buffers
