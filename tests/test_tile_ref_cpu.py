"""tests/tile_ref.py pinned against independent statements of the same operations (F.conv1d, F.conv_transpose1d, autograd in fp64), and the
dispatch table of the tile kernel tests (tests/tile_cases.py through the name sink: which kernels every GPU record launches, and its return
code).  No GPU needed."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import disc_ref as D
from tests import tile_cases as K
from tests import tile_ref as R
from tests.test_disc_ref_cpu import _close, _rnd


def _lr(v, slope):
    return F.leaky_relu(v, float(np.float32(slope)))


@pytest.mark.parametrize('k,dil,pad_left', [(3, 1, -1), (7, 3, -1), (11, 5, -1), (5, 16, -1), (7, 5, 30), (4, 2, 1), (2, 13, 0)])
def test_conv1d_is_f_conv1d_with_the_fused_prologue_and_epilogue(k, dil, pad_left):
    B, ci, co, L = 2, 4, 6, 70
    x, wf = _rnd(1, B, ci, L), _rnd(2, k, ci, co)
    in_a, in_s, bias = _rnd(3, B, ci), _rnd(4, B, ci), _rnd(5, co)
    res, res_a, res_s, a0, a1 = _rnd(6, B, co, L), _rnd(7, B, co), _rnd(8, B, co), _rnd(9, B, co, L), _rnd(10, B, co, L)
    left = pad_left if pad_left >= 0 else dil * (k - 1) // 2
    act = _lr(in_a[:, :, None] * x + in_s[:, :, None], 0.1)
    z = F.conv1d(F.pad(act, (left, (k - 1) * dil - left)), D.wf_to_w(wf), bias, dilation=dil)
    want = _lr(((a0 + a1) + (z + (res_a[:, :, None] * res + res_s[:, :, None]))) / 3.0, 0.2)
    got, S = R.conv1d(x, wf, dil=dil, pad_left=pad_left, slope=0.1, in_a=in_a, in_s=in_s, bias=bias, res=res, res_a=res_a, res_s=res_s,
                      add0=a0, add1=a1, out_div=3.0, out_slope=0.2)
    _close(got, want)
    assert (S * (1 + 1e-12) >= ((a0 + a1) + (z + (res_a[:, :, None] * res + res_s[:, :, None]))).abs() / 3.0).all()
    # plain, and `accumulate` is add0 = the old contents
    _close(R.conv1d(x, wf, dil=dil, pad_left=pad_left)[0], F.conv1d(F.pad(x, (left, (k - 1) * dil - left)), D.wf_to_w(wf), dilation=dil))
    _close(R.conv1d(x, wf, dil=dil, pad_left=pad_left, old=a0)[0], R.conv1d(x, wf, dil=dil, pad_left=pad_left, add0=a0)[0], 0.0)


def test_in_stride_reads_one_phase_and_slices_are_plain_slices():
    x, wf = _rnd(11, 2, 4, 60), _rnd(12, 3, 4, 5)
    for ph in (0, 1):
        _close(R.conv1d(x, wf, in_stride=2, in_phase=ph, slope=0.1)[0], R.conv1d(x[:, :, ph::2].contiguous(), wf, slope=0.1)[0], 0.0)


def test_the_input_gradient_record_is_autograd_of_the_forward_record():
    """conv(dy; transposed tap-flipped weights, pad_left' = (k - 1) dil - pad_left) is d/dx of the forward conv, also for asymmetric padding."""
    for k, dil, pad_left in ((7, 3, -1), (7, 5, 30), (4, 2, 1)):
        B, ci, co, L = 2, 4, 6, 50
        x, wf, dy = _rnd(13, B, ci, L).requires_grad_(True), _rnd(14, k, ci, co), _rnd(15, B, co, L)
        left = pad_left if pad_left >= 0 else dil * (k - 1) // 2
        y = F.conv1d(F.pad(x, (left, (k - 1) * dil - left)), D.wf_to_w(wf), dilation=dil)
        y.backward(dy)
        got, S = R.conv1d(dy, D.transpose_flip(wf), dil=dil, pad_left=(k - 1) * dil - left)
        _close(got, x.grad)
        assert (S >= got.abs() - 1e-12).all()


def test_the_mask_epilogue_is_the_gradient_of_leaky_relu():
    """dx of y = conv(leaky_relu(a * m + s)) is lrelu'(a * m + s) * conv^T(dy) (times a, which the caller folds elsewhere): the mask epilogue
    with mask_src = m, before the bias / residual terms.  +0 and -0 take the slope."""
    B, ci, co, L, k = 2, 4, 6, 40, 3
    m, wf, dy = _rnd(16, B, ci, L), _rnd(17, k, ci, co), _rnd(18, B, co, L)
    a, s, res = _rnd(19, B, ci), _rnd(20, B, ci), _rnd(21, B, ci, L)
    pre = (a[:, :, None] * m + s[:, :, None]).requires_grad_(True)
    y = F.conv1d(_lr(pre, 0.1), D.wf_to_w(wf), padding=1)
    y.backward(dy)
    got, _ = R.conv1d(dy, D.transpose_flip(wf), mask_src=m, mask_a=a, mask_s=s, mask_slope=0.1, res=res)
    _close(got, pre.grad + res)
    f, arg = R.mask_factor(torch.tensor([[[0.0, -0.0, 1e-300, -1e-300]]], dtype=torch.float64), None, None, 0.5)
    assert f.flatten().tolist() == [0.5, 0.5, 1.0, 0.5] and arg.abs().max().item() == 1e-300


def test_lengths_are_each_items_own_unpadded_call():
    B, ci, co, L, k, dil = 3, 4, 5, 40, 7, 3
    x, wf, bias = _rnd(22, B, ci, L), _rnd(23, k, ci, co), _rnd(24, co)
    ends = [0, 13, 40]
    xn = x.clone()
    for b, e in enumerate(ends):
        xn[b, :, e:] = float('nan')                                   # whatever the tensor holds there
    got, S = R.conv1d(xn, wf, dil=dil, slope=0.1, bias=bias, lengths=ends)
    for b, e in enumerate(ends):
        assert torch.isnan(got[b, :, e:]).all() and torch.isnan(S[b, :, e:]).all()
        if e:
            _close(got[b:b + 1, :, :e], R.conv1d(x[b:b + 1, :, :e].contiguous(), wf, dil=dil, slope=0.1, bias=bias)[0])


@pytest.mark.parametrize('u', [2, 4, 5, 8])
@pytest.mark.parametrize('L', [1, 3, 20])
def test_convt1d_is_f_conv_transpose1d(u, L):
    k = 2 * u if u % 2 == 0 else 2 * u + 1
    B, ci, co = 2, 6, 3
    x, wf, bias = _rnd(25, B, ci, L), _rnd(26, k, ci, co), _rnd(27, co)
    want = F.conv_transpose1d(_lr(x, 0.1), wf.permute(1, 2, 0).contiguous(), bias, stride=u, padding=(k - u) // 2)
    got, S = R.convt1d(x, wf, u, slope=0.1, bias=bias)
    assert got.shape == (B, co, u * L)
    _close(got, want)
    assert (S >= got.abs() - 1e-12).all()
    ends = [0, L]
    gl, _ = R.convt1d(x, wf, u, slope=0.1, bias=bias, lengths=ends)
    assert torch.isnan(gl[0]).all()
    _close(gl[1], got[1], 0.0)


def test_tile_sums():
    v = _rnd(28, 2, 3, 10)
    s, a, q = R.tile_sums(v, 4)
    assert s.shape == (6, 3)
    _close(s[4], v[1, :, 4:8].sum(-1))
    _close(a[5], v[1, :, 8:].abs().sum(-1))
    _close(q[2], (v[0, :, 8:] ** 2).sum(-1))


# ---------------------------------------------------------------------------------------------------------------
# the dispatch table: one row per GPU record
ROWS = [(g, c) for g, cases in K.TABLE.items() for c in cases]


@pytest.mark.parametrize('group,c', ROWS, ids=['%s-%s' % (g, c['id']) for g, c in ROWS])
def test_dispatch_of_every_gpu_record(group, c):
    rc, names, no_device = K.dispatch(c)
    print(group, c['id'], rc, names)
    want = c['kernels'][:1] if no_device else c['kernels']           # (without a device the call ends in front of the reduce launch: its name is pinned only with one)
    assert (rc, names) == (c['rc'], want), (rc, names)


def test_the_split_records_ask_for_a_workspace_and_the_others_for_none():
    for c in K.ALL:
        if c['rc'] != K.OK:
            continue
        splits = any(n.startswith('splitk_reduce') for n in c['kernels'])
        if splits or c['id'] in ('split_short_ws', 'split_no_ws', 'ups0_stats_whole'):
            assert K.ws_bytes(c) > 0, c['id']
        elif c['ws']:
            assert K.ws_bytes(c) == 0, c['id']                        # the short chain


def test_the_table_reaches_every_branch():
    seen = {n for c in K.ALL for n in c['kernels']}
    tiles = (K.LAT, K.T128x64, K.T128, K.T64x128, K.CK16, K.R32, K.MF16)
    need = [K.tile_name(t, 0, v) for t in tiles for v in (True, False)]
    need += [K.tile_name(t, e, v) for t in (K.LAT, K.T128x64) for e in (1, 2, 3) for v in (True, False)]
    need += [K.tile_name(K.UP_TILE[co] % u, e, v) for u in (2, 4, 5, 8) for co in (64, 32, 16) for e in (0, 3) for v in (True, False)]
    need += [K.reduce_name(True), K.reduce_name(False)]
    assert [n for n in need if n not in seen] == []
    # what the names cannot show: the 128 x 128 record is exactly 1 024 tiles, the tile-edge lengths are on an edge
    big = next(c for c in K.TILES if c['id'] == 't128_k11_d5')
    assert big['B'] * D.ceil_div(big['L'], 128) * (big['co'] // 128) == 1024
    for c in K.LENGTHS:
        assert bool(c['in_off'] or c['out_off']) == c['id'].endswith('plus4')
    assert all(any(0 < e * c['len_mul'] < c['L'] and e * c['len_mul'] % K.NT[c['tile']] == 0 for e in c['lens']) for c in K.LENS)
    assert all(c['n'] == tuple(k * c['ci'] + c['ops'] for k in c['ks']) for c in K.ALL if c['op'] == 'conv')       # one n per problem
