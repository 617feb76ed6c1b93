"""Every record of tests/tile_cases.py on the device: the f32 tile kernel family (conv_tile_kernel's ten tile shapes, its four epilogues, the
vector and scalar paths, the split over C_in with splitk_reduce_kernel, the four upsamplers) against the fp64 statement of the call
(tests/tile_ref.py), per entry.  tests/test_tile_ref_cpu.py asserts which kernels each record launches.

A record fails when any entry's |got - want| / (n * 2^-24 * S) exceeds 1 (n: the chain length of the record's problem, S: the summed magnitudes of the
entry's terms, from the reference's data).  Every buffer a call may write is NaN-filled and larger than the region it may write - guard
floats on both sides, the other channel slices of a wider tensor, the tiles wholly past an item's length, a workspace the call must not use -
and everything outside that region must keep its bits.  Inputs past an item's length hold NaN, which no valid output may show.  Each test
prints its worst error / bound ratio (`-s` shows them; DESIGN.md 3e'' records them).

Row sums (rowsum_part, n = NT) and the upsamplers' statistics rows (stats_part, n = the NT * u positions of a row) are sums of the values the
launch stored: they are held to n * 2^-24 * sum |v| (sum v^2 for the squares) of the stored values themselves.
The mask source is drawn with |mask_a * m + mask_s| >= 2^-10 (offenders redrawn on the CPU), so the fp32 and fp64 arguments have one sign and
no entry is excluded; without the affine it also holds exact +0 and -0, which take the slope.

Worst ratios on an MI355X when these tests were written: tiles 0.091 forward (CK 16, k = 3) and 0.070 input gradient, lengths and offsets
0.080, epilogues 0.081 (row sums 0.036), per-item lengths 0.038, split over C_in 0.018, upsamplers 0.077 (statistics rows 0.014); the file
takes 6.4 s, its slowest record 0.41 s.  Value-only mutants of csrc/v2w_conv_mfma.hip these records fail on (DESIGN.md 3e'' has the table):
`add1` ignored (17 records), `res_s` read as 0 (20), `out_div` before the residual (20), the reduce starting at slab 2 (19), the mask compare
as `>=` (6: the exact zeros), one tap of one weight fragment zeroed in pack_mfma_kernel (252)."""
import numpy as np
import pytest
import torch

from tests import disc_ref as D
from tests import tile_cases as K
from tests import tile_ref as R
from tests.test_disc_kernels_gpu import NAN, _cases, _report, env  # noqa: F401  (env: the module-scoped fixture)
from wavthruvec_pytorch_amd import hipops

pytestmark = pytest.mark.gpu

GUARD = 64                      # floats on either side of every buffer a call may write (a multiple of 4: the base stays 16-byte aligned)
MASK_MIN = 2.0 ** -10


def _rng(c):
    return np.random.default_rng(sum(map(ord, c['id'])))          # a seed per record id


def _f32(rng, *shape, scale=1.0):
    return torch.from_numpy(rng.standard_normal(shape, dtype=np.float32) * np.float32(scale))


class Buf:
    """A flat device buffer [GUARD | lead | payload | GUARD]: `base` is the 16-byte aligned address the argument builder offsets from, the
    payload (the whole tensor the call's operand is a slice of) starts `lead` floats behind it."""

    def __init__(self, dev, payload, lead=0):
        n = payload.numel()
        flat = torch.full((2 * GUARD + lead + n,), NAN)
        flat[GUARD + lead:GUARD + lead + n] = payload.reshape(-1)
        self.flat, self.lo, self.n, self.shape = flat.to(dev), GUARD + lead, n, tuple(payload.shape)
        self.before = self.flat.clone()
        assert self.flat.data_ptr() % 16 == 0
        self.base = self.flat.data_ptr() + 4 * GUARD

    def payload(self):
        return self.flat[self.lo:self.lo + self.n].view(self.shape)

    def untouched_outside(self, written):
        """`written`: bool tensor of the payload's shape, True where the call may store.  Everything else keeps its bits."""
        w = torch.zeros(self.flat.numel(), dtype=torch.bool, device=self.flat.device)
        w[self.lo:self.lo + self.n] = written.reshape(-1).to(self.flat.device)
        same = self.flat.view(torch.int32) == self.before.view(torch.int32)
        return bool((same | w).all())


def _sync_or_stop(what):
    """A HIP error (a fault) ends the session: nothing more is launched on that device."""
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit('%s: %s' % (what, e), returncode=3)


def _nan_payload(*shape):
    return torch.full(shape, NAN)


def _ends(c):
    return None if c['lens'] is None else [min(c['L'], e * c['len_mul']) for e in c['lens']]


def _draw_mask(rng, B, Cc, L, a, s):
    """The mask source with |a * m + s| >= 2^-10 in fp64 everywhere; offenders are redrawn.  Without the affine: plus exact zeros."""
    m = _f32(rng, B, Cc, L)
    for _ in range(64):
        arg = D.f64(m) if a is None else D.f64(a)[:, :, None] * D.f64(m) + D.f64(s)[:, :, None]
        bad = arg.abs() < MASK_MIN
        if not bad.any():
            break
        m[bad] = _f32(rng, int(bad.sum()))
    assert not bad.any()
    if a is None:
        flat = m.view(-1)
        flat[:4] = torch.tensor([0.0, -0.0, 0.0, -0.0])
        flat[-2:] = torch.tensor([-0.0, 0.0])
    return m


def _problem(c, i, dev, rng):
    """Operands of problem i of a conv record: (buffers by operand name, keyword arguments of tile_ref.conv1d on the call's slices)."""
    B, ci, co, L, k, f = c['B'], c['ci'], c['co'], c['L'], c['ks'][i], c['flags']
    ict, oct_ = c['in_ct'] or ci, c['out_ct'] or co
    isl, osl = slice(c['in_g'] * ci, (c['in_g'] + 1) * ci), slice(c['out_g'] * co, (c['out_g'] + 1) * co)
    ends = _ends(c)
    bufs, ref = {}, dict(dil=c['dil'], pad_left=c['pad_left'], slope=c['slope'], in_stride=c['in_stride'], in_phase=c['in_phase'],
                         out_div=c['out_div'], out_slope=c['out_slope'], lengths=ends)
    x = _f32(rng, B, ict, L * c['in_stride'])
    if ends is not None:
        for b, e in enumerate(ends):
            x[b, :, e:] = NAN                                # whatever the tensor holds past the item's end
    bufs['in_'] = Buf(dev, x, c['in_off'])
    if c.get('wT'):                                          # the forward layer's weights [k][co][ci]; the stream of its input gradient
        w_fwd = _f32(rng, k, co, ci, scale=1.0 / np.sqrt(co * k)).to(dev)
        wf, wp = D.transpose_flip(w_fwd), hipops.pack_mfma_dgrad(w_fwd)
    else:
        wf = _f32(rng, k, ci, co, scale=1.0 / np.sqrt(ci * k)).to(dev)
        wp = hipops.pack_mfma(wf)
    assert wp is not None
    bufs['wp'] = wp
    wf = wf.cpu()

    def small(name, *shape, scale=1.0, shift=0.0):
        t = _f32(rng, *shape, scale=scale) + shift
        bufs[name] = t.to(dev)
        return t

    def wide(name):                                          # a (B, out_ct, L) operand; the reference gets the call's slice
        t = _f32(rng, B, oct_, L)
        bufs[name] = Buf(dev, t)
        return t[:, osl]

    if 'in_aff' in f:
        ref['in_a'], ref['in_s'] = small('in_a', B, ci, scale=0.5, shift=1.0), small('in_s', B, ci, scale=0.5)
    if 'bias' in f:
        ref['bias'] = small('bias', co)
    if 'res' in f:
        ref['res'] = wide('res')
    if 'res_aff' in f:
        ref['res_a'], ref['res_s'] = small('res_a', B, co, scale=0.5, shift=1.0), small('res_s', B, co, scale=0.5)
    if 'add0' in f:
        ref['add0'] = wide('add0')
    if 'add1' in f:
        ref['add1'] = wide('add1')
    if 'mask' in f:
        if 'mask_aff' in f:
            ref['mask_a'], ref['mask_s'] = small('mask_a', B, co, scale=0.5, shift=1.0), small('mask_s', B, co, scale=0.5)
        m = _draw_mask(rng, B, co, L, ref.get('mask_a'), ref.get('mask_s'))
        mw = _f32(rng, B, oct_, L)
        mw[:, osl] = m
        bufs['mask_src'] = Buf(dev, mw)
        ref['mask_src'], ref['mask_slope'] = m, c['mask_slope']
    out = _nan_payload(B, oct_, L)
    if 'acc' in f:
        ref['old'] = _f32(rng, B, co, L)
        out[:, osl] = ref['old']
    bufs['out'] = Buf(dev, out, c['out_off'])
    if 'rowsum' in f:
        bufs['rowsum_part'] = Buf(dev, _nan_payload(B * D.ceil_div(L, K.NT[c['tile']]), co, 2))
    return bufs, (x[:, isl], wf, ref), osl


def _addr(b):
    return b.base if isinstance(b, Buf) else b.data_ptr()


def _written(shape, osl, ends, NT, u=1):
    """Where the call may store: its channel slice; with lengths, the tiles that start before the item's end."""
    w = torch.zeros(shape, dtype=torch.bool)
    w[:, osl] = True
    if ends is not None:
        for b, e in enumerate(ends):
            w[b, :, D.ceil_div(e, NT) * NT * u:] = False
    return w


def _shared(c, dev, B):
    sh, keep = dict(ws=0, len=0, stats_part=0), {}
    if c['ws']:
        nbytes = K.ws_bytes(c)
        keep['ws'] = Buf(dev, _nan_payload(D.ceil_div(nbytes, 4)))
        sh['ws'] = keep['ws'].base
    if c['lens'] is not None:
        keep['len'] = torch.tensor(c['lens'], dtype=torch.int32).to(dev)
        sh['len'] = keep['len'].data_ptr()
    return sh, keep


def _sum_rows_ok(name, part, stored, NT, n, squares):
    """part (tiles, C, 2) against the fp64 sums of the stored values per tile and row."""
    tot, mag, sq = R.tile_sums(stored, NT)
    ratios = dict(rowsum=D.worst_ratio(part[..., 0], tot, D.sum_bound(n, mag)))
    if squares:
        ratios['sumsq'] = D.worst_ratio(part[..., 1], sq, D.sum_bound(n, sq))
    else:
        assert torch.equal(part[..., 1], torch.zeros_like(part[..., 1])), name
    return ratios


def run_conv(env, c):
    dev, _hip, lib, st = env
    rng = _rng(c)
    n, NT = len(c['ks']), K.NT[c['tile']]
    probs = [_problem(c, i, dev, rng) for i in range(n)]
    shared, keep = _shared(c, dev, c['B'])
    per = [{name: _addr(b) for name, b in bufs.items()} for bufs, _, _ in probs]
    torch.cuda.synchronize()
    rc, _ = K.call(c, per, shared, st)
    _sync_or_stop(c['id'])
    assert rc == c['rc'], (c['id'], rc)
    rd = dev if c['big'] else torch.device('cpu')
    ends = _ends(c)
    ratios = {}
    for i, (bufs, (x, wf, ref), osl) in enumerate(probs):
        out = bufs['out']
        if rc != K.OK:                                       # a refusal launches nothing: every buffer keeps its bits
            assert out.untouched_outside(torch.zeros(out.shape, dtype=torch.bool))
            continue
        assert out.untouched_outside(_written(out.shape, osl, ends, NT)), c['id'] + ': stored outside its region'
        for name in ('in_', 'res', 'add0', 'add1', 'mask_src'):
            if name in bufs:
                assert bufs[name].untouched_outside(torch.zeros(bufs[name].shape, dtype=torch.bool)), name
        ref = {k_: (v.to(rd) if isinstance(v, torch.Tensor) else v) for k_, v in ref.items()}
        want, S = R.conv1d(x.to(rd), wf.to(rd), **ref)
        got = out.payload()[:, osl].to(rd)
        if ends is None:
            ratios['out%d' % i] = D.worst_ratio(got, want, D.sum_bound(c['n'][i], S))
        else:
            r = 0.0
            for b, e in enumerate(ends):
                r = max(r, D.worst_ratio(got[b, :, :e], want[b, :, :e], D.sum_bound(c['n'][i], S[b, :, :e])))
            ratios['out%d' % i] = r
        if 'rowsum_part' in bufs:
            rs = bufs['rowsum_part']
            assert rs.untouched_outside(torch.ones(rs.shape, dtype=torch.bool))
            ratios.update({k_ + str(i): v for k_, v in _sum_rows_ok(c['id'], rs.payload().to(rd), got, NT, NT, False).items()})
    if 'ws' in keep:
        ws = keep['ws']
        splits = any(name.startswith('splitk_reduce') for name in c['kernels'])
        assert ws.untouched_outside(torch.full(ws.shape, splits, dtype=torch.bool)), c['id'] + ': workspace'
    _report('tile ' + c['id'] + ' n=' + '/'.join(map(str, c['n'])), **ratios)


def run_convt(env, c):
    dev, _hip, lib, st = env
    rng = _rng(c)
    B, ci, co, L, k, u, NT = c['B'], c['ci'], c['co'], c['L'], c['k'], c['u'], c['NT']
    ends = _ends(c)
    x = _f32(rng, B, ci, L)
    if ends is not None:
        for b, e in enumerate(ends):
            x[b, :, e:] = NAN
    wf = _f32(rng, k, ci, co, scale=1.0 / np.sqrt(ci * k / u))
    bias = _f32(rng, co)
    xb, out = Buf(dev, x), Buf(dev, _nan_payload(B, co, L * u))
    wfd, bd = wf.to(dev), bias.to(dev)
    wp = hipops.pack_mfma(wfd, u=u)
    assert wp is not None
    shared, keep = _shared(c, dev, B)
    stats = Buf(dev, _nan_payload(B * D.ceil_div(L, NT), co, 2)) if c['stats'] else None
    shared['stats_part'] = stats.base if stats else 0
    per = [dict(in_=xb.base, wp=wp.data_ptr(), bias=bd.data_ptr(), out=out.base)]
    torch.cuda.synchronize()
    rc, _ = K.call(c, per, shared, st)
    _sync_or_stop(c['id'])
    assert rc == c['rc'], (c['id'], rc)
    assert out.untouched_outside(_written(out.shape, slice(0, co), ends, NT, u)), c['id'] + ': stored outside its region'
    assert xb.untouched_outside(torch.zeros(xb.shape, dtype=torch.bool))
    want, S = R.convt1d(x, wf, u, slope=c['slope'], bias=bias, lengths=ends)
    got = out.payload().cpu()
    if ends is None:
        ratios = dict(out=D.worst_ratio(got, want, D.sum_bound(c['n'][0], S)))
    else:
        ratios = dict(out=max(D.worst_ratio(got[b, :, :e * u], want[b, :, :e * u], D.sum_bound(c['n'][0], S[b, :, :e * u])) for b, e in enumerate(ends)))
    if stats:
        assert stats.untouched_outside(torch.ones(stats.shape, dtype=torch.bool))
        ratios.update(_sum_rows_ok(c['id'], stats.payload().cpu(), got, NT * u, NT * u, True))
    if 'ws' in keep:
        ws = keep['ws']
        splits = any(name.startswith('splitk_reduce') for name in c['kernels'])
        assert ws.untouched_outside(torch.full(ws.shape, splits, dtype=torch.bool)), c['id'] + ': workspace'
    _report('tile ' + c['id'] + ' n=' + '/'.join(map(str, c['n'])), **ratios)


@_cases(K.TILES)
def test_tiles_forward_and_input_gradient(env, c):
    run_conv(env, c)


@_cases(K.LENGTHS)
def test_lengths_and_alignment_on_every_tile(env, c):
    run_conv(env, c)


@_cases(K.EPILOGUES)
def test_epilogues(env, c):
    run_conv(env, c)


@_cases(K.LENS)
def test_per_item_lengths(env, c):
    run_conv(env, c)


@_cases(K.SPLIT)
def test_split_over_c_in(env, c):
    run_conv(env, c)


@_cases(K.UPS)
def test_upsamplers(env, c):
    run_convt(env, c)


def test_the_short_workspace_gives_the_split_result_within_the_bound(env):
    """The same launch split (four slabs, the reduce) and whole (workspace one byte short): both within the bound of the same reference, hence
    within twice the bound of each other - checked directly, on the same operands."""
    dev = env[0]
    outs = []
    for id_ in ('split_vec', 'split_short_ws'):
        c = dict(next(r for r in K.SPLIT if r['id'] == id_), id='split_vec')          # the same seed: the same operands
        rng = _rng(c)
        bufs, (x, wf, ref), osl = _problem(c, 0, dev, rng)
        shared, keep = _shared(c, dev, c['B'])
        rc, _ = K.call(c, [{name: _addr(b) for name, b in bufs.items()}], shared, env[3])
        _sync_or_stop(c['id'])
        assert rc == K.OK
        outs.append(bufs['out'].payload().cpu())
        _, S = R.conv1d(x, wf, **ref)
    assert ((outs[0].double() - outs[1].double()).abs() <= 2 * D.sum_bound(c['n'][0], S)).all()
