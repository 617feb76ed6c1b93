"""Every record of tests/stage_cases.py on the device: the fused narrow-stage kernels (resblock2_stage_kernel's four tile shapes in their plain,
LEN, BWD, POST and POST + LEN forms, resblock2_stage_wino_kernel, resblock_pair_kernel, small_stage_kernel; the vector and the scalar
paths; the refusals) against the fp64 statement of the call (tests/stage_ref.py), per entry.  tests/test_stage_ref_cpu.py asserts which
kernel each record launches.

A record fails when any valid entry's |got - want| / bound exceeds 1 (the bound: stage_ref's first-order propagation, no tuned constant; no
entry is excluded).  Every buffer a call may write is NaN-filled and larger than the region it may write - guard floats on both sides, the
tiles wholly past an item's end, `out` behind the fused tail - and everything outside that region must keep its bits, inputs and masks
included; a refused call must leave every buffer as it was.  Inputs past an item's end hold NaN, which no valid output may show.  Each test
prints its worst error / bound ratio (`-s` shows them; DESIGN.md 3e''' records them).

The gradient form's row sums are held, per tile, to (W / 4) * 2^-24 * sum |v| of the dt1_j the launch stored (a row is one wave's sum over at
most W / 4 positions; the rows of a tile are added in fp64 here).  bwd_mask1 holds exact +0 and -0, which take the slope; bwd_mask2 with its
affine is drawn with |a * m + s| >= 2^-10 (test_tile_kernels_gpu._draw_mask; tests/test_stage_ref_cpu.py checks that the redraw ends)."""
import numpy as np
import pytest
import torch

from tests import disc_ref as D
from tests import stage_cases as K
from tests import stage_ref as R
from tests import tile_ref
from tests.test_disc_kernels_gpu import NAN, _cases, _report, env  # noqa: F401  (env: the module-scoped fixture)
from tests.test_tile_kernels_gpu import Buf, _draw_mask, _f32, _nan_payload, _rng, _sync_or_stop
from wavthruvec_pytorch_amd import hipops

pytestmark = pytest.mark.gpu

NONE = 'none'           # written-region marker: the call may store nowhere in this buffer


def _ends(c):
    return None if c['lens'] is None else [min(c['L'], e * c['len_mul']) for e in c['lens']]


def _untouched(buf, written=None):
    return buf.untouched_outside(torch.zeros(buf.shape, dtype=torch.bool) if written is None else written)


def _weights(c, rng, dev, k, ok):
    """One conv of a record: (the weights [k][C][C] as the conv applies them, the device stream the call gets)."""
    Cc = c['C']
    w = _f32(rng, k, Cc, Cc, scale=1.0 / np.sqrt(Cc * k))
    if not ok:
        return w, w.to(dev)                                      # a refused call reads no weights
    if c['op'] == 'stage' and c['bwd'] is not None:              # `w`: the forward layer's; the gradient conv applies them transposed, taps reversed
        return D.transpose_flip(w), hipops.pack_mfma_dgrad(w.to(dev))
    if c['form'] == 'small':
        return w, w.to(dev)
    wp = hipops.pack_wino(w.to(dev)) if c['form'] == 'wino' else hipops.pack_mfma(w.to(dev))
    assert wp is not None
    return w, wp


def _affine(c, rng, dev, bufs, ref, B, Cc):
    if 'in_aff' in c['flags']:
        ref['in_a'], ref['in_s'] = _f32(rng, B, Cc, scale=0.5) + 1.0, _f32(rng, B, Cc, scale=0.5)
        bufs['in_a'], bufs['in_s'] = Buf(dev, ref['in_a'], int('in_a' in c['offs'])), Buf(dev, ref['in_s'])


def _branch(c, rng, dev, k, d1, d2, ok, keep):
    w1, p1 = _weights(c, rng, dev, k, ok)
    w2, p2 = _weights(c, rng, dev, k, ok)
    b1 = b2 = None
    if 'bias' in c['flags']:
        b1, b2 = _f32(rng, c['C']), _f32(rng, c['C'])
    dv = [p1, p2, None if b1 is None else b1.to(dev), None if b2 is None else b2.to(dev)]
    keep.append(dv)
    return dict(w1=w1, b1=b1, w2=w2, b2=b2, d1=d1, d2=d2), dv


def _ptr(t):
    return 0 if t is None else (t.base if isinstance(t, Buf) else t.data_ptr())


def run_stage(env, c):
    dev, _hip, lib, st = env
    rng = _rng(c)
    B, Cc, L, ok, bwd = c['B'], c['C'], c['L'], c['rc'] == K.OK, c['bwd']
    g, ends, nk = c['geom'], _ends(c), len(c['br'])
    bufs, ref, keep = {}, {}, []
    x = _f32(rng, B, Cc, L)
    if ends is not None:
        for b, e in enumerate(ends):
            x[b, :, e:] = NAN                                    # whatever the tensor holds past the item's end
    bufs['in_'] = Buf(dev, x, int('in_' in c['offs']))
    _affine(c, rng, dev, bufs, ref, B, Cc)
    branches, dvs = zip(*[_branch(c, rng, dev, k, d1, d2, ok, keep) for k, d1, d2 in c['br']])
    bufs['out'] = Buf(dev, _nan_payload(B, Cc, L), int('out' in c['offs']))
    addr = {n: 0 for n in K.SCALARS}
    addr.update(wp1=[d[0].data_ptr() for d in dvs], wp2=[d[1].data_ptr() for d in dvs], b1=[_ptr(d[2]) for d in dvs], b2=[_ptr(d[3]) for d in dvs])
    if c['post_k']:
        post_w = _f32(rng, c['post_k'], Cc, 1, scale=1.0 / np.sqrt(Cc * c['post_k']))
        post_b = _f32(rng, 1) if c['post_b'] else None
        keep += [post_w.to(dev), None if post_b is None else post_b.to(dev)]
        addr['post_w'], addr['post_b'] = keep[-2].data_ptr(), _ptr(keep[-1])
        bufs['post_out'] = Buf(dev, _nan_payload(B, 1, L), int('post_out' in c['offs']))
    if bwd is not None:
        mask1 = []
        for j in range(nk):
            m = _draw_mask(rng, B, Cc, L, None, None)            # the forward's t1_j: exact +0 and -0 among its entries
            mask1.append(m)
            bufs['mask1_%d' % j], bufs['mid_%d' % j] = Buf(dev, m), Buf(dev, _nan_payload(B, Cc, L))
        m2a = m2s = None
        if bwd['aff']:
            m2a, m2s = _f32(rng, B, Cc, scale=0.5) + 1.0, _f32(rng, B, Cc, scale=0.5)
            bufs['mask2_a'], bufs['mask2_s'] = Buf(dev, m2a), Buf(dev, m2s)
        mask2 = _draw_mask(rng, B, Cc, L, m2a, m2s)
        bufs['mask2'] = Buf(dev, mask2)
        if bwd['rowsum']:
            rows = K.bwd_rows(c) if ok else 8
            assert rows == (B * g['ntl'] * 4 if ok else 8), rows
            for j in range(nk):
                bufs['rowsum_%d' % j] = Buf(dev, _nan_payload(rows, Cc, 2))
        for n in ('mask1', 'mid', 'rowsum'):
            addr[n] = [_ptr(bufs.get('%s_%d' % (n, j))) for j in range(nk)]
    if c['lens'] is not None:
        keep.append(torch.tensor(c['lens'], dtype=torch.int32).to(dev))
        addr['len'] = keep[-1].data_ptr()
    for n in ('in_', 'in_a', 'in_s', 'out', 'post_out', 'mask2', 'mask2_a', 'mask2_s'):
        addr[n] = _ptr(bufs.get(n))
    torch.cuda.synchronize()
    rc, _ = K.call(c, [addr], st)
    _sync_or_stop(c['id'])
    assert rc == c['rc'], (c['id'], rc)

    # ---- where the call may store
    written = {n: None for n in bufs}                            # None: nowhere
    if ok:
        full = torch.ones(B, Cc, L, dtype=torch.bool)
        if c['post_k']:
            written['post_out'] = torch.ones(B, 1, L, dtype=torch.bool)
        elif ends is None:
            written['out'] = full
        else:
            w = full.clone()
            for b, e in enumerate(ends):
                w[b, :, D.ceil_div(e, g['nto']) * g['nto']:] = False          # tiles that start at or past the item's end return at once
            written['out'] = w
        if bwd is not None:
            for j in range(nk):
                written['mid_%d' % j] = full
                if bwd['rowsum']:
                    written['rowsum_%d' % j] = torch.ones(bufs['rowsum_%d' % j].shape, dtype=torch.bool)
    for n, buf in bufs.items():
        assert _untouched(buf, written[n]), '%s: %s changed outside the region the call may write' % (c['id'], n)
    if not ok:
        return

    # ---- values
    ratios = {}
    if bwd is not None:
        want, E, mids = R.section_bwd(x, branches, mask1, c['n1'], c['n2'], mask2=mask2, mask2_a=m2a, mask2_s=m2s, bwd_slope=bwd['slope'],
                                      in_a=ref.get('in_a'), in_s=ref.get('in_s'))
        ratios['out'] = D.worst_ratio(bufs['out'].payload().cpu(), want, E)
        for j, (t1, E1) in enumerate(mids):
            got = bufs['mid_%d' % j].payload().cpu()
            ratios['mid%d' % j] = D.worst_ratio(got, t1, E1)
            if bwd['rowsum']:
                part = D.f64(bufs['rowsum_%d' % j].payload().cpu()).reshape(B * g['ntl'], 4, Cc, 2)
                assert torch.equal(part[..., 1], torch.zeros_like(part[..., 1])), c['id']
                tot, mag, _ = tile_ref.tile_sums(got, g['nto'])
                ratios['rows%d' % j] = D.worst_ratio(part[..., 0].sum(1), tot, D.sum_bound(g['W'] // 4, mag))
    else:
        want, E = R.section(x, branches, c['n1'], c['n2'], slope=c['slope'], in_a=ref.get('in_a'), in_s=ref.get('in_s'), out_div=c['out_div'],
                            ends=ends, wino=c['form'] == 'wino')
        if c['post_k']:
            want, E, _ = R.tail(want, E, post_w, post_b, c['n_p'], post_slope=c['post_slope'], ends=ends)
            ratios['post_out'] = D.worst_ratio(bufs['post_out'].payload().cpu(), want, E)         # (past an item's end: exactly 0)
        else:
            got = bufs['out'].payload().cpu()
            if ends is None:
                ratios['out'] = D.worst_ratio(got, want, E)
            else:
                ratios['out'] = max(D.worst_ratio(got[b, :, :e], want[b, :, :e], E[b, :, :e]) for b, e in enumerate(ends))
    _report('stage ' + c['id'], **ratios)


def run_pair(env, c):
    dev, _hip, lib, st = env
    rng = _rng(c)
    B, Cc, L, ok = c['B'], c['C'], c['L'], c['rc'] == K.OK
    probs, addrs, keep = [], [], []
    for k in c['ks']:
        bufs, ref = {}, {}
        x = _f32(rng, B, Cc, L)
        bufs['in_'] = Buf(dev, x, int('in_' in c['offs']))
        _affine(c, rng, dev, bufs, ref, B, Cc)
        br, dv = _branch(c, rng, dev, k, c['d1'], c['d2'], ok, keep)
        for n in ('add0', 'add1')[:c['adds']]:
            ref[n] = _f32(rng, B, Cc, L)
            bufs[n] = Buf(dev, ref[n])
        bufs['out'] = Buf(dev, _nan_payload(B, Cc, L))
        addr = {n: _ptr(bufs.get(n)) for n in K.SCALARS}
        addr.update(wp1=[dv[0].data_ptr()], wp2=[dv[1].data_ptr()], b1=[_ptr(dv[2])], b2=[_ptr(dv[3])])
        probs.append((bufs, x, br, ref))
        addrs.append(addr)
    torch.cuda.synchronize()
    rc, _ = K.call(c, addrs, st)
    _sync_or_stop(c['id'])
    assert rc == c['rc'], (c['id'], rc)
    ratios = {}
    for i, (bufs, x, br, ref) in enumerate(probs):
        for n, buf in bufs.items():
            w = torch.ones(buf.shape, dtype=torch.bool) if ok and n == 'out' else None
            assert _untouched(buf, w), '%s: %s of problem %d changed outside the region the call may write' % (c['id'], n, i)
        if ok:
            want, E = R.pair(x, br, c['n1'][i], c['n2'][i], c['n_add'], slope=c['slope'], res_mode=c['res_mode'], out_div=c['out_div'], **ref)
            ratios['out%d' % i] = D.worst_ratio(bufs['out'].payload().cpu(), want, E)
    if ok:
        _report('pair ' + c['id'], **ratios)


@_cases(K.LENGTHS)
def test_lengths_on_every_window(env, c):
    run_stage(env, c)


@_cases(K.ALIGN)
def test_unaligned_operands_take_the_scalar_path(env, c):
    run_stage(env, c)


@_cases(K.BRANCHES)
def test_branch_sets_and_optional_operands(env, c):
    run_stage(env, c)


@_cases(K.LENS)
def test_per_item_lengths(env, c):
    run_stage(env, c)


@_cases(K.GRAD)
def test_gradient_form(env, c):
    run_stage(env, c)


@_cases(K.PAIR)
def test_pair(env, c):
    run_pair(env, c)


@_cases(K.SMALL)
def test_eight_channel_kernel(env, c):
    run_stage(env, c)


@_cases(K.REFUSALS)
def test_refusals_write_nothing(env, c):
    run_stage(env, c)


def test_device_tanhf_error(env):
    """The tail's tanhf against fp64 tanh of the same fp32 argument, on a record whose pre-activation is exact: zero branch weights, no bias, no
    affine, slope 1 (out = x + 0), post_slope 1, a one-hot post_w of 1.0 on the centre tap of channel 0 - arg = x[b][0][l], swept over [-9, 9]
    (and the arguments a random draw adds near 0).  stage_ref.TANH_C is twice the worst error in units of 2^-24, rounded up."""
    dev, _hip, lib, st = env
    B, Cc, L = 8, 16, 14336
    x = torch.zeros(B, Cc, L)
    x[:, 0] = torch.linspace(-9.0, 9.0, B * L, dtype=torch.float64).to(torch.float32).reshape(B, L)
    x[0, 0, :4096] = _f32(np.random.default_rng(5), 4096)
    c = K.stage('tanh_sweep', 'direct', C=Cc, B=B, L=L, W=256, br=((3, 1, 1),), flags=(), slope=1.0, out_div=0.0, post_k=9, post_b=False,
                post_slope=1.0)
    zero = hipops.pack_mfma(torch.zeros(3, Cc, Cc, device=dev))
    post_w = torch.zeros(9, Cc, 1)
    post_w[4, 0, 0] = 1.0
    xin, out, pw = Buf(dev, x), Buf(dev, _nan_payload(B, 1, L)), post_w.to(dev)
    addr = {n: 0 for n in K.SCALARS}
    addr.update(in_=xin.base, post_out=out.base, post_w=pw.data_ptr(), wp1=[zero.data_ptr()], wp2=[zero.data_ptr()], b1=[0], b2=[0])
    rc, _ = K.call(c, [addr], st)
    _sync_or_stop(c['id'])
    assert rc == K.OK
    assert _untouched(out, torch.ones(out.shape, dtype=torch.bool)) and _untouched(xin)
    err = (D.f64(out.payload().cpu())[:, 0] - torch.tanh(D.f64(x[:, 0]))).abs() / D.U
    worst = err.max().item()
    print('[tanhf] worst |tanhf(a) - tanh(a)| = %.3f * 2^-24 at a = %r over %d arguments; TANH_C = %d'
          % (worst, x[:, 0].reshape(-1)[int(err.argmax())].item(), B * L, R.TANH_C))
    assert np.isfinite(worst) and 2 * worst <= R.TANH_C
