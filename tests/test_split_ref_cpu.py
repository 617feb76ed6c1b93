"""tests/split_ref.py pinned against independent statements (F.conv1d in fp64 on every record's operands, the packers decoded back to the
weights), the proof that the short-chain records can see a lost lo term, and the dispatch table of the split kernel tests
(tests/split_cases.py through the name sink: which kernel every GPU record launches, and its return code).  No GPU needed."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import disc_ref as D
from tests import split_cases as K
from tests import split_ref as R
from tests import stage_ref
from tests.test_disc_ref_cpu import _close

RUN = [c for c in K.CONV_ALL if c['rc'] == K.OK]


def _lr(v, slope):
    return v if slope == 1.0 else F.leaky_relu(v, float(np.float32(slope)))


def _independent(c, x, wf, ref):
    """The call's value from F.conv1d and the header's formula, in fp64."""
    k, dil = wf.shape[0], c['dil']
    left = c['pad_left'] if c['pad_left'] >= 0 else dil * (k - 1) // 2
    x = D.f64(x)[:, :, c['in_phase']::c['in_stride']]
    if 'in_a' in ref:
        x = D.f64(ref['in_a'])[:, :, None] * x + D.f64(ref['in_s'])[:, :, None]
    act = _lr(x, c['slope']).clamp(-65504.0, 65504.0)
    z = F.conv1d(F.pad(act, (left, (k - 1) * dil - left)), D.wf_to_w(D.f64(wf)), dilation=dil)
    if 'mask_src' in ref:
        arg = D.f64(ref['mask_src'])
        if 'mask_a' in ref:
            arg = D.f64(ref['mask_a'])[:, :, None] * arg + D.f64(ref['mask_s'])[:, :, None]
        z = torch.where(arg > 0, z, z * float(np.float32(ref['mask_slope'])))
    if 'bias' in ref:
        z = z + D.f64(ref['bias'])[None, :, None]
    if 'res' in ref:
        z = z + (D.f64(ref['res']) if 'res_a' not in ref else D.f64(ref['res_a'])[:, :, None] * D.f64(ref['res']) + D.f64(ref['res_s'])[:, :, None])
    if 'add0' in ref:
        z = (D.f64(ref['add0']) + (D.f64(ref['add1']) if 'add1' in ref else 0.0)) + z
    if 'old' in ref:
        z = D.f64(ref['old']) + z
    if c['out_div']:
        z = z / float(np.float32(c['out_div']))
    return _lr(z, c['out_slope']) if c['out_slope'] else z


@pytest.mark.parametrize('c', RUN, ids=K.ids(RUN))
def test_the_reference_is_f_conv1d_and_the_short_chain_records_see_a_lost_lo_term(c):
    for i in range(len(c['ks'])):
        o = K.operands(c, i)
        x, wf, ref = o['t']['x'][:, o['isl']], o['t']['wf'], o['ref']
        if c['bf']:
            continue                                                 # (the bf16 statement rounds its operands: pinned on its own below)
        want, bound = R.conv1d(x, wf, c['n'][i], **ref)
        _close(want, _independent(c, x, wf, ref), 1e-11)
        assert torch.isfinite(bound).all() and (bound >= 0).all()
        if c['short'] and c['data'] != 'zero_layer':
            # a kernel without the a_lo * w_hi products is short of `lost`: more than the bound on at least half of the live entries
            lost = R.without_a_lo(x[:, :, c['in_phase']::c['in_stride']], wf, dil=c['dil'], pad_left=c['pad_left'], slope=c['slope'])
            _, scale = R.epilogue_scale(lost, ref)
            lost = lost.abs() * scale
            live = R.conv1d(x, wf, c['n'][i], **{q: v for q, v in ref.items() if q in ('dil', 'pad_left', 'slope', 'in_stride', 'in_phase')})[0] != 0
            seen = (lost > bound) & live
            print('[power] %s: lost a_lo * w_hi exceeds the bound on %d of %d live entries, worst %.3g bounds'
                  % (c['id'], int(seen.sum()), int(live.sum()), float((lost / bound)[live].max())))
            # (every short-chain record but the all-zero layer, which has no live entry; the operand-range draws keep enough activations
            # with a non-zero lo half - off the clamp, the 0.1 of `tiny` - for one half of the entries)
            assert 2 * int(seen.sum()) >= int(live.sum()) > 0, c['id']


def test_the_bf16_statement_rounds_both_operands_once():
    c = next(q for q in K.BF16 if q['id'] == 'bf_t256_k3')
    o = K.operands(c)
    x, wf, ref = o['t']['x'], o['t']['wf'], o['ref']
    got, bound = R.conv1d_bf16(x, wf, c['n'][0], **{q: v for q, v in ref.items() if q not in ('in_stride', 'in_phase')})
    a = F.leaky_relu(x, float(np.float32(0.1))).bfloat16().double()
    want = F.conv1d(a, D.wf_to_w(wf.bfloat16().double()), ref['bias'].double(), padding=1)
    _close(got, want, 1e-11)
    # the statement without the rounding is 2^-8 away, not 2^-24: the emulation matters
    plain = F.conv1d(F.leaky_relu(x.double(), float(np.float32(0.1))), D.wf_to_w(wf.double()), ref['bias'].double(), padding=1)
    assert ((plain - want).abs() > bound).float().mean() > 0.5


@pytest.mark.parametrize('c', K.ALL, ids=K.ids(K.ALL))
def test_dispatch_of_every_gpu_record(c):
    rc, names = K.dispatch(c) if c['op'] == 'conv' else K.stage_dispatch(c)
    print(c['id'], rc, names)
    assert (rc, names) == (c['rc'], c['kernels']), (rc, names)


def test_the_table_reaches_every_instantiation_the_launchers_can_select():
    seen = {n for c in K.ALL for n in c['kernels']}
    need = [K.tile_name(t, v, False) for t in (K.T128, K.T64, K.T256, K.W128, K.W64) for v in (True, False)]
    need += [K.tile_name(t, True, True) for t in (K.T128, K.T64, K.T256)] + [K.tile_name(K.T256, False, True)]
    need += [K.stage_name(32), K.stage_name(16)]
    assert [n for n in need if n not in seen] == []
    # what the names cannot show
    for c in K.CONV_ALL:
        if c['rc'] == K.OK and c['tile'] in (K.T128, K.W128):
            assert 2 * c['B'] * D.ceil_div(c['L'], 256) * (c['co'] // 128) >= 384, c['id']
        if c['short']:
            assert c['B'] >= c['ci'] and 'in_aff' not in c['flags'], c['id']         # every channel live once; zero stays zero
        assert c['n'] == tuple((1 if c['bf'] else 3) * k * (1 if c['short'] else c['ci']) + c['ops'] for k in c['ks'])
    assert any(2 * c['B'] * D.ceil_div(c['L'], 256) == 384 for c in K.TILES) and any(2 * c['B'] * D.ceil_div(c['L'], 256) == 382 for c in K.TILES)
    for c in K.STAGES:
        nto = K.stage_nto(c['blocks'])
        assert nto >= 128 or c['rc'] == K.E_SHAPE
    assert K.stage_nto(K.BLOCKS['four']) == 128 and K.stage_nto(K.BLOCKS['past']) < 128


# ---------------------------------------------------------------------------------------------------------------
# the CPU packer
PACK_SHAPES = [(3, 16, 64), (7, 48, 128), (11, 32, 32), (3, 16, 16), (1, 16, 64)]


@pytest.mark.parametrize('k,ci,co', PACK_SHAPES)
def test_the_cpu_packer_decodes_back_to_the_weights(k, ci, co):
    wf = (np.random.default_rng(k * ci + co).standard_normal((k, ci, co)) / np.sqrt(k * ci)).astype(np.float32)
    frag, (sc0, sc1) = R.pack_split(wf)
    assert frag.size == R.fragment_count(k, ci, co) and sc0 * sc1 == 1.0
    assert 8192 <= np.abs(wf).max() * sc1 < 16384
    back = R.unpack_split(frag, sc0, k, ci, co)
    # hi + lo is within 2^-22 of a weight whose lo half is a normal f16 number; below that the f16 subnormal floor, in units of w
    tol = 2.0 ** -22 * np.abs(wf.astype(np.float64)) + 2.0 ** -25 * float(sc0)
    assert (np.abs(back - wf.astype(np.float64)) <= tol).all()
    assert (np.abs(back - wf.astype(np.float64)) <= 2.0 ** -22 * np.abs(wf).max()).all()
    # one slot, by the documented formula: element (((mb * nch + ch) * K + t) * 2 + hl) * 64 + lane, half j
    mb, ch, t, lane, j = (co - 1) // 32, ci // 16 - 1, k - 1, 37, 5
    hi, lo = R.halves(np.float32(wf[t, ch * 16 + 8 * (lane >> 5) + j, mb * 32 + (lane & 31)] * sc1) if mb * 32 + (lane & 31) < co else np.float32(0))
    flat = frag.reshape(-1, 8)
    base = ((mb * (ci // 16) + ch) * k + t) * 2 * 64 + lane
    assert flat[base, j] == hi.view(np.int16) and flat[base + 64, j] == lo.view(np.int16)
    if co == 16:
        assert (frag.reshape(1, ci // 16, k, 2, 2, 32, 8)[..., 16:, :] == 0).all()      # the padded rows


def test_the_scale_edges():
    assert R.split_scale(np.zeros((3, 16, 32), np.float32)) == 1.0
    assert R.split_scale(np.full((1,), np.inf, np.float32)) == 1.0 and R.split_scale(np.full((1,), np.nan, np.float32)) == 1.0
    assert R.split_scale(np.array([0.25, -0.1], np.float32)) * 0.25 == 8192.0           # a power of two lands on 8192 exactly
    assert 8192 <= R.split_scale(np.array([0.2499999], np.float32)) * np.float32(0.2499999) < 16384
    frag, sc = R.pack_split(np.zeros((3, 16, 32), np.float32))
    assert not frag.any() and sc == (1.0, 1.0)


def test_the_stage_statement_with_the_split_terms_only_widens_the_bound():
    c = next(q for q in K.STAGES if q['id'] == 'c16_ref_L4')
    x, in_a, in_s, brs = K.stage_operands(c)
    v0, e0 = stage_ref.section(x, brs, c['n1'], c['n2'], slope=c['slope'], in_a=in_a, in_s=in_s, out_div=c['out_div'])
    v1, e1 = stage_ref.section(x, brs, c['n1'], c['n2'], slope=c['slope'], in_a=in_a, in_s=in_s, out_div=c['out_div'], split=True)
    assert torch.equal(v0, v1) and (e1 > e0).all() and (e1 < 2 * e0).all()


def test_stage_streams():
    c = next(q for q in K.STAGES if q['id'] == 'c32_ref_L4')
    offs, total = K.stream_offsets(c)
    assert offs == [0, 6144, 12288, 26624, 40960, 63488] and total == 86016          # 2 K units of 1024 halves per stream
    c = next(q for q in K.STAGES if q['id'] == 'c16_streams_swapped')
    assert K.stream_offsets(c)[0][:2] == [3072, 0]
