"""Every record of tests/split_cases.py on the device: the split-f16 conv kernel (conv_split_kernel's five tile forms, vector and scalar
staging and epilogue, its bf16-operand form where a call reaches it), the fused narrow-stage kernel (stage_split_kernel, C = 32 and 16) and
the packers, against the fp64 statement of the call and its derived bound (tests/split_ref.py, tests/stage_ref.py with split = True), per
entry.  tests/test_split_ref_cpu.py asserts which kernel each record launches and that the short-chain records can see a lost lo term.

A record fails when any entry's |got - want| / bound exceeds 1.  Every buffer a call may write is NaN-filled and larger than the region it
may write (guard floats on both sides, the other channel slices of a wider tensor) and everything outside that region must keep its bits;
a refusal must leave every buffer alone.  The packers are compared bit for bit (int16 view) with the layout documented above
pack_split_kernel, over all documented elements, on buffers pre-filled with a pattern that must survive everywhere else.  Each test prints
its worst error / bound ratio (`-s` shows them).

Worst ratios on an MI355X when these tests were written: tiles 0.036 dense (HM = 40, pad_left 37) and 0.37 short-chain (128 x 128, k = 3);
lengths and offsets 0.018; prologue / epilogue switches 0.032; forward / input-gradient pairs 0.0091; operand range 0.036 dense (the
subnormal lo halves) and 0.33 short-chain (on the clamp); bf16 operands 0.054 dense and 0.42 short-chain; stage 0.0033 dense and 0.036
short-chain (its second conv counts all C channels: t1 is dense); weight-norm batch pack 0.54 (split f16) and 0.996 (bf16 fragments: one rounding to 8 bits against its own unit roundoff).
The file takes 6 s, its slowest record 0.85 s.  No record failed on the unmodified kernels.

Value-only mutants these records fail on, one run each, (b) once more after the second conv's chain length was corrected, with the
same outcome (the letters are the issue's): (a) the x_lo * w_hi MFMA removed from
conv_split_kernel - 194 records: every split-f16 conv record of the tiles, lengths, switches, pairs and operand-range tests, dense ones
included, the bf16 records untouched; (b) the same MFMA removed from stage_split_kernel's second conv only - 11 stage records: the four
short-chain ones and the one-branch block set at C = 16 (and L = 1 at C = 32), the three- and four-branch dense records hide it; (c) hi
and lo swapped in pack_split_kernel - 212: the six non-zero layers of the bitwise packer test, every split-f16 conv record and 12 stage
records; (e) the +-65504 clamp removed - range_big and range_big_short; (f) res_s dropped from the element-wise epilogue - the ten scalar
records with a residual affine (res_res_aff, all_add, all_acc, mask_all, n4_all on both tiles); (d) channels j and j ^ 1 swapped in
pack_split_kernel's fragment elements and, as a shuffle of the signal operand's register in front of the MFMA, in conv_split_kernel and
stage_split_kernel together - the six non-zero layers of the bitwise packer test and nothing else: every value test passes, which is
what the layout test is for."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import disc_ref as D
from tests import split_cases as K
from tests import split_ref as R
from tests import stage_ref
from tests.test_disc_kernels_gpu import NAN, _cases, _report, env  # noqa: F401  (env: the module-scoped fixture)
from tests.test_tile_kernels_gpu import Buf, _addr, _nan_payload, _sync_or_stop
from wavthruvec_pytorch_amd import hipops

pytestmark = pytest.mark.gpu

WIDE = ('res', 'add0', 'add1', 'mask_src')
PATTERN = 0x5a5b                     # int16 pre-fill of every fragment buffer


def _problem(c, i, dev):
    """Device buffers of problem i of a conv record (by operand name) and its CPU operands (split_cases.operands)."""
    o = K.operands(c, i)
    t, osl = o['t'], o['osl']
    bufs = {'in_': Buf(dev, t['x'], c['in_off'])}
    if c['rc'] == K.OK:
        bufs['wps'], bufs['winv'] = hipops.pack_split(t['wf'].to(dev).contiguous(), bf16=c['bf'])
    else:                                                    # a refusal reads no weights (and some of its shapes have no fragments)
        bufs['wps'], bufs['winv'] = torch.zeros(2048, dtype=torch.float16, device=dev), torch.ones(4, device=dev)
    for name, v in t.items():
        if name in WIDE:
            bufs[name] = Buf(dev, v)
        elif name not in ('x', 'wf'):
            bufs[name] = v.to(dev)
    out = _nan_payload(c['B'], c['out_ct'] or c['co'], c['L'])
    if 'old' in o['ref']:
        out[:, osl] = o['ref']['old']
    bufs['out'] = Buf(dev, out, c['out_off'])
    return bufs, o


def run_conv(env, c):
    dev, _hip, lib, st = env
    n = len(c['ks'])
    probs = [_problem(c, i, dev) for i in range(n)]
    per = [{name: _addr(b) for name, b in bufs.items()} for bufs, _ in probs]
    torch.cuda.synchronize()
    rc, _ = K.call(c, per, st)
    _sync_or_stop(c['id'])
    assert rc == c['rc'], (c['id'], rc)
    rd = dev if c['big'] else torch.device('cpu')
    ratios = {}
    for i, (bufs, o) in enumerate(probs):
        out, osl = bufs['out'], o['osl']
        written = torch.zeros(out.shape, dtype=torch.bool)
        if rc == K.OK:
            written[:, osl] = True
        assert out.untouched_outside(written), c['id'] + ': stored outside its region'
        for name in ('in_',) + WIDE:
            if name in bufs:
                assert bufs[name].untouched_outside(torch.zeros(bufs[name].shape, dtype=torch.bool)), name
        if rc != K.OK:
            continue
        ref = {q: (v.to(rd) if isinstance(v, torch.Tensor) else v) for q, v in o['ref'].items()}
        x, wf = o['t']['x'][:, o['isl']].to(rd), o['t']['wf'].to(rd)
        if c['bf']:
            want, bound = R.conv1d_bf16(x, wf, c['n'][i], **{q: v for q, v in ref.items() if q not in ('in_stride', 'in_phase')})
        else:
            want, bound = R.conv1d(x, wf, c['n'][i], **ref)
        ratios['out%d' % i] = D.worst_ratio(out.payload()[:, osl].to(rd), want, bound)
    _report('split ' + c['id'] + ' n=' + '/'.join(map(str, c['n'])), **ratios)


@_cases(K.TILES)
def test_tiles_dense_and_short_chain(env, c):
    run_conv(env, c)


@_cases(K.LENGTHS)
def test_lengths_and_alignment_on_every_tile(env, c):
    run_conv(env, c)


@_cases(K.EPILOGUES)
def test_prologue_and_epilogue_switches(env, c):
    run_conv(env, c)


@_cases(K.DGRAD)
def test_forward_and_matching_input_gradient(env, c):
    run_conv(env, c)


@_cases(K.RANGE)
def test_operand_range(env, c):
    run_conv(env, c)


@_cases(K.BF16)
def test_bf16_operands_on_the_split_kernel(env, c):
    run_conv(env, c)


@_cases(K.REFUSALS)
def test_refusals(env, c):
    run_conv(env, c)


# ---------------------------------------------------------------------------------------------------------------
# the fused narrow stage
def _stage_buffers(c, dev):
    x, in_a, in_s, brs = K.stage_operands(c)
    Cc, nk = c['C'], len(c['blocks'])
    offs, total = K.stream_offsets(c)
    guard = 4096                                             # halves after the last stream: never read, never written
    wps = torch.full((total + guard,), NAN, dtype=torch.float16, device=dev)
    sc = torch.zeros(2 * nk, 4, device=dev)
    for j, br in enumerate(brs):
        for s, w in ((2 * j, br['w1']), (2 * j + 1, br['w2'])):
            n = K.stream_halves(c, j)
            assert n == hipops.split_units_halves(w.shape[0], Cc, Cc)
            hipops.pack_split(w.to(dev).contiguous(), out=wps[offs[s]:offs[s] + n], sc=sc[s])
    keep = dict(x=Buf(dev, x, c['in_off']), out=Buf(dev, _nan_payload(*x.shape)), wps=wps, sc=sc)
    if c['aff']:
        keep['in_a'], keep['in_s'] = in_a.to(dev), in_s.to(dev)
    if c['bias']:
        keep['b1'] = torch.stack([br['b1'] for br in brs]).to(dev).contiguous()
        keep['b2'] = torch.stack([br['b2'] for br in brs]).to(dev).contiguous()
    addr = dict(in_=keep['x'].base, out=keep['out'].base, wps=wps.data_ptr(), sc=sc.data_ptr())
    addr.update({q: keep[q].data_ptr() for q in ('in_a', 'in_s', 'b1', 'b2') if q in keep})
    return keep, addr, (x, in_a, in_s, brs), total


@_cases(K.STAGES)
def test_stage_split(env, c):
    dev, _hip, lib, st = env
    keep, addr, (x, in_a, in_s, brs), total = _stage_buffers(c, dev)
    wps_before = keep['wps'].clone()
    torch.cuda.synchronize()
    rc = lib.v2w_resblock2_stage_split_fwd(C.byref(K.stage_struct(c, addr)), st)
    _sync_or_stop(c['id'])
    assert rc == c['rc'], (c['id'], rc)
    out = keep['out']
    assert out.untouched_outside(torch.full(out.shape, rc == K.OK, dtype=torch.bool)), c['id'] + ': stored outside its region'
    assert keep['x'].untouched_outside(torch.zeros(keep['x'].shape, dtype=torch.bool))
    assert torch.equal(keep['wps'].view(torch.int16), wps_before.view(torch.int16)) and bool(torch.isnan(keep['wps'][total:]).all())
    if rc != K.OK:
        return
    kw = dict(slope=c['slope'], in_a=in_a, in_s=in_s, out_div=c['out_div'])
    want, bound = stage_ref.section(x, brs, c['n1'], c['n2'], split=True, **kw)
    got = out.payload().cpu()
    _report('stage ' + c['id'], out=D.worst_ratio(got, want, bound))


# ---------------------------------------------------------------------------------------------------------------
# packers against the documented layout, bit for bit
def _pack_weights(kind, k, ci, co):
    wf = (np.random.default_rng(k * 1000 + ci + co).standard_normal((k, ci, co)) / np.sqrt(k * ci)).astype(np.float32)
    if kind == 'zero':
        wf[:] = 0
    elif kind == 'pow2':
        wf = np.clip(wf, -0.2, 0.2)
        wf[0, 1, 2], wf[k - 1, ci - 1, co - 1] = 0.25, -0.25
    return wf


def _fragment_buffer(dev, n):
    """int16 buffer of n documented elements and the 1024-element padding unit, pre-filled."""
    return torch.full((n + 1024,), PATTERN, dtype=torch.int16, device=dev)


PACK_CASES = [('normal', 3, 16, 64), ('normal', 7, 48, 128), ('normal', 11, 32, 32), ('normal', 3, 16, 16), ('normal', 1, 16, 64),
              ('zero', 3, 16, 64), ('pow2', 3, 16, 64)]


@pytest.mark.parametrize('kind,k,ci,co', PACK_CASES, ids=['%s_k%d_ci%d_co%d' % q for q in PACK_CASES])
def test_pack_split_is_the_documented_layout_bit_for_bit(env, kind, k, ci, co):
    dev, _hip, lib, st = env
    wf = _pack_weights(kind, k, ci, co)
    want, (sc0, sc1) = R.pack_split(wf)
    n = R.fragment_count(k, ci, co)
    buf, sc = _fragment_buffer(dev, n), torch.full((4,), NAN, device=dev)
    wfd = torch.from_numpy(wf).to(dev)
    assert lib.v2w_pack_split(wfd.data_ptr(), buf.data_ptr(), sc.data_ptr(), k, ci, co, st) == 0
    _sync_or_stop('pack_split')
    got = buf.cpu().numpy()
    assert np.array_equal(got[:n], want.reshape(-1)) and (got[n:] == PATTERN).all()
    assert sc[0].item() == float(sc0) and sc[1].item() == float(sc1)
    if kind == 'pow2':
        assert sc1 * 0.25 == 8192.0
    if kind == 'zero':
        assert (sc0, sc1) == (1.0, 1.0) and not got[:n].any()


@pytest.mark.parametrize('kind,k,ci,co', PACK_CASES, ids=['%s_k%d_ci%d_co%d' % q for q in PACK_CASES])
def test_pack_bf16_fills_the_hi_slots_and_leaves_the_lo_slots(env, kind, k, ci, co):
    dev, _hip, lib, st = env
    wf = _pack_weights(kind, k, ci, co)
    n = R.fragment_count(k, ci, co)
    buf, sc = _fragment_buffer(dev, n), torch.full((4,), NAN, device=dev)
    wfd = torch.from_numpy(wf).to(dev)
    assert lib.v2w_pack_bf16(wfd.data_ptr(), buf.data_ptr(), sc.data_ptr(), k, ci, co, st) == 0
    _sync_or_stop('pack_bf16')
    got = buf.cpu().numpy()
    units = got[:n].reshape(-1, 2, 64, 8)                    # [mb][ch][K] units of (hi, lo) x 64 lanes x 8
    assert np.array_equal(units[:, 0], R.pack_bf16(wf).reshape(-1, 64, 8))
    assert (units[:, 1] == PATTERN).all() and (got[n:] == PATTERN).all()
    assert sc[0].item() == 1.0 and sc[1].item() == 1.0


class _Batch:
    """The device tables of one v2w_split_pack_batch call, a mode per layer (hipops.SplitPlan has one for all).  layers: (v (C_out, C_in,
    k) CPU, g (C_out) CPU | None, mode); v_off: floats between a 16-byte boundary and the base of every v."""

    def __init__(self, dev, layers, v_off=0):
        from wavthruvec_pytorch_amd import _hip
        n = len(layers)
        self.layers, self.n = layers, n
        self.rowscale = torch.zeros(sum(v.shape[0] for v, _, _ in layers), device=dev)
        self.v, self.g, self.wps, self.sc = [], [], [], []
        descs = (_hip.SplitDesc * n)()
        starts = [0] * (2 * (n + 1))
        off = blocks = 0
        for i, (d, (v, g, mode)) in enumerate(zip(descs, layers)):
            co, ci, k = v.shape
            flat = torch.zeros(v.numel() + 8, device=dev)
            flat[v_off:v_off + v.numel()] = v.reshape(-1).to(dev)
            self.v.append(flat)
            self.g.append(None if g is None else g.to(dev))
            self.wps.append(_fragment_buffer(dev, R.fragment_count(k, ci, co)))
            self.sc.append(torch.full((4,), NAN, device=dev))
            d.v, d.g, d.wps, d.sc = flat.data_ptr() + 4 * v_off, _hip.ptr(self.g[-1]), self.wps[-1].data_ptr(), self.sc[-1].data_ptr()
            d.rowscale = self.rowscale.data_ptr() + 4 * off
            d.c_in, d.c_out, d.k, d.mode = ci, co, k, mode
            starts[i], starts[n + 1 + i] = off, blocks
            off += co
            blocks += ((co + 31) // 32) * (ci // 16)
        starts[n], starts[2 * n + 1] = off, blocks
        self.rows, self.blocks, self.k_max = off, blocks, max(v.shape[2] for v, _, _ in layers)
        self.descs = torch.frombuffer(bytearray(bytes(descs)), dtype=torch.uint8).to(dev)
        self.starts = torch.tensor(starts, dtype=torch.int32, device=dev)

    def run(self, lib, st, all_bf16=0, k_max=None):
        rc = lib.v2w_split_pack_batch(self.descs.data_ptr(), self.starts.data_ptr(), self.n, self.rows, self.blocks,
                                      self.k_max if k_max is None else k_max, all_bf16, st)
        _sync_or_stop('split_pack_batch')
        return rc


def _layer(seed, co, ci, k, g=False, mode=0):
    rng = np.random.default_rng(seed)
    v = torch.from_numpy(rng.standard_normal((co, ci, k), dtype=np.float32) * np.float32(1.0 / np.sqrt(ci * k)))
    return v, (torch.from_numpy(rng.standard_normal(co, dtype=np.float32)) + 2.0 if g else None), mode


BATCHES = {
    'four_layers': ([_layer(1, 64, 16, 3), _layer(2, 128, 48, 7), _layer(3, 32, 32, 11), _layer(4, 16, 16, 5)], 0, 0),
    'v_plus4': ([_layer(5, 64, 16, 3), _layer(6, 16, 32, 7)], 1, 0),
    'mode_mix': ([_layer(7, 64, 16, 3), _layer(8, 64, 32, 7, mode=1), _layer(9, 16, 16, 11), _layer(10, 32, 16, 5, mode=1)], 0, 0),
    'all_bf16': ([_layer(11, 64, 16, 3, mode=1), _layer(12, 16, 32, 7, mode=1)], 0, 1),
    'all_bf16_flag_off': ([_layer(11, 64, 16, 3, mode=1), _layer(12, 16, 32, 7, mode=1)], 0, 0),
    'weight_norm': ([_layer(13, 64, 16, 3, g=True), _layer(14, 128, 48, 7, g=True), _layer(15, 16, 16, 11, g=True)], 0, 0),
    'weight_norm_v_plus4': ([_layer(16, 64, 16, 3, g=True), _layer(17, 32, 32, 7, g=True, mode=1)], 1, 0),
}


@pytest.mark.parametrize('name', list(BATCHES))
def test_split_pack_batch(env, name):
    dev, _hip, lib, st = env
    layers, v_off, all_bf16 = BATCHES[name]
    b = _Batch(dev, layers, v_off)
    assert b.run(lib, st, all_bf16) == 0
    worst = 0.0
    for (v, g, mode), wps, sc in zip(layers, b.wps, b.sc):
        co, ci, k = v.shape
        n = R.fragment_count(k, ci, co)
        got = wps.cpu().numpy()
        assert (got[n:] == PATTERN).all()
        if g is None:
            wf = v.permute(2, 1, 0).contiguous().numpy()                     # the conv layout [k][C_in][C_out]
            if mode == 1:
                units = got[:n].reshape(-1, 2, 64, 8)
                assert np.array_equal(units[:, 0], R.pack_bf16(wf).reshape(-1, 64, 8)) and (units[:, 1] == PATTERN).all()
                assert sc[0].item() == 1.0 and sc[1].item() == 1.0
            else:
                want, (sc0, sc1) = R.pack_split(wf)
                assert np.array_equal(got[:n], want.reshape(-1)), name
                assert sc[0].item() == float(sc0) and sc[1].item() == float(sc1)
            continue
        # weight norm: w = g * v / ||v|| per output row; the row scale is an fp32 rounding of a double sum whose order is not pinned
        v64 = v.double()
        w = (g.double()[:, None, None] * v64 / v64.flatten(1).norm(dim=1)[:, None, None]).permute(2, 1, 0).numpy()
        if mode == 1:                                                        # bf16(fp32(v * rowscale)): the row scale and the product round to fp32 (2 * 2^-24), then rne to 8 bits (2^-8)
            units = got[:n].reshape(-1, 2, 64, 8)
            hi = torch.from_numpy(np.ascontiguousarray(units[:, 0])).view(torch.bfloat16).double().numpy()
            ref = torch.from_numpy(np.ascontiguousarray(R._fragments(w))).numpy().reshape(-1, 64, 8)
            r = np.abs(hi - ref) / ((2.0 ** -8 + 2.0 ** -23) * np.abs(ref) + 1e-300)
            worst = max(worst, float(r.max()))
            continue
        sc0, sc1 = sc[0].item(), sc[1].item()
        frag = got[:n].reshape(-(-co // 32), ci // 16, k, 2, 64, 8)
        back = R.unpack_split(np.ascontiguousarray(frag), sc0, k, ci, co)
        bound = (2.0 ** -22 + 3 * 2.0 ** -24) * np.abs(w) + 2.0 ** -38 * np.abs(w).max()
        worst = max(worst, float((np.abs(back - w) / bound).max()))
        assert sc0 * sc1 == 1.0 and np.frexp(sc1)[0] == 0.5                 # a power of two and its exact inverse
        assert 8192 <= np.abs(back).max() * sc1 < 16384
    _report('split_pack_batch ' + name, decoded=worst)


def test_split_pack_batch_refuses_a_tap_count_past_the_lds(env):
    dev, _hip, lib, st = env
    b = _Batch(dev, [_layer(20, 32, 16, 3)])
    assert 32 * (16 * 31 + 1) * 4 <= 64 * 1024 < 32 * (16 * 32 + 1) * 4
    assert b.run(lib, st, k_max=32) == K.E_SHAPE
    assert (b.wps[0].cpu().numpy() == PATTERN).all()
