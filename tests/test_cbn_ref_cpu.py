"""tests/cbn_ref.py pinned against independent statements of the same operations (F.linear, the oracle's spectral_norm_weight in both modes,
F.batch_norm with its running-statistics update, the oracle's batch_norm_no_affine), its bounds checked on a plain fp64 evaluation of the
kernels' own formulas, and the dispatch table of the conditional batch norm tests (tests/cbn_cases.py through the name sink: which kernels
every call of every GPU record launches, and its return code).  No GPU needed."""
from fractions import Fraction

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import vec2wav_oracle as O
from tests import cbn_cases as K
from tests import cbn_ref as R


def _t(a):
    return torch.from_numpy(np.asarray(a, dtype=np.float64))


def _close(a, b, tol=1e-12):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b.detach().numpy() if hasattr(b, 'detach') else b, dtype=np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    assert np.abs(a - b).max() <= tol * max(1.0, np.abs(b).max())


def test_linear_and_cond_z_are_f_linear():
    rng = np.random.default_rng(1)
    spk, noise, w, b = rng.standard_normal((3, 70)), rng.standard_normal((3, 33)), rng.standard_normal((128, 103)), rng.standard_normal(128)
    z, S = R.cond_z(spk, noise, w, b)
    _close(z, F.linear(torch.cat([_t(spk), _t(noise)], 1), _t(w), _t(b)))
    assert (S >= np.abs(z) - 1e-12).all()
    _close(R.cond_z(spk, None, w[:, :70], b)[0], F.linear(_t(spk), _t(w[:, :70]), _t(b)))
    z0, S0 = R.cond_z(spk, noise, None, None)
    assert np.array_equal(z0, np.concatenate([spk, noise], 1)) and not S0.any()


@pytest.mark.parametrize('R_', [16, 80, 2048])
def test_the_power_iteration_is_the_oracles_spectral_norm_weight(R_):
    rng = np.random.default_rng(R_)
    W = 1 + 0.02 * rng.standard_normal((R_, 128))
    u, v = rng.standard_normal(R_), rng.standard_normal(128)
    u, v = u / np.linalg.norm(u), v / np.linalg.norm(v)
    z, b = rng.standard_normal((2, 128)), rng.standard_normal(R_)
    # training: v, then u from that v, sigma from both
    w_sn, u2, v2 = O.spectral_norm_weight(_t(W), _t(u), _t(v), True)
    v_new, dv = R.sn_new_v(W, u, R_ // 8 + 8, 23)
    _close(v_new, v2)
    u_new, du, wv, dwv = R.sn_new_u(W, v_new, 8, 25)
    _close(u_new, u2)
    sigma, dsig = R.sn_sigma(u_new, du, wv, dwv, 25)
    _close(W / sigma, w_sn)
    gb, dgb = R.gamma_beta(W, b, z, sigma, 8)
    _close(gb, F.linear(_t(z), w_sn, _t(b)))
    assert (dv > 0).all() and (du > 0).all() and dsig > 0 and (dgb > 0).all()
    assert dv.max() < 1e-4 and du.max() < 1e-5 and dsig < 1e-4 * sigma          # tight: sigma is far from 0
    # eval: u, v as stored
    w_sn, u3, v3 = O.spectral_norm_weight(_t(W), _t(u), _t(v), False)
    wv, dwv = R.sn_wv(W, v, 8)
    sigma, _ = R.sn_sigma(u, 0.0, wv, dwv, 25)
    _close(W / sigma, w_sn)
    assert torch.equal(u3, _t(u)) and torch.equal(v3, _t(v))


def test_quotient_and_norm_bounds_hold_on_perturbed_operands():
    rng = np.random.default_rng(2)
    p, q = rng.standard_normal(1000), rng.uniform(1, 2, 1000) * rng.choice([-1, 1], 1000)
    dp, dq = 1e-6 * rng.uniform(0, 1, 1000), 1e-6 * rng.uniform(0, 1, 1000)
    r, dr = R.quotient(p, dp, q, dq)
    for sp in (-1, 1):
        for sq in (-1, 1):
            assert (np.abs((p + sp * dp) / (q + sq * dq) - r) <= dr * (1 + 1e-5)).all()
    nq, dnq = R.norm(p, dp, 0)
    assert abs(np.linalg.norm(p + dp) - nq) <= dnq and abs(np.linalg.norm(p - dp * np.sign(p)) - nq) <= dnq


def _signal(seed, B, C, L):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((B, C, L)) * rng.uniform(0.5, 2, C)[None, :, None] + rng.standard_normal(C)[None, :, None]
    return x, rng.standard_normal((B, 2 * C)), rng.standard_normal(C), rng.uniform(0.5, 1.5, C)


@pytest.mark.parametrize('B,L,momentum', [(3, 50, 0.25), (1, 1, 0.25), (2, 7, 1.0)])
def test_finalize_is_batch_norm_in_training_mode(B, L, momentum):
    """a x + s from the channel sums is gamma * F.batch_norm(x, training) + beta, and the running statistics are torch's update (unbiased
    variance, skipped at count 1) and the oracle's; eps 2^-10 and these momenta are exact in fp32."""
    C, eps = 5, 2.0 ** -10
    x, gb, rm, rv = _signal(3, B, C, L)
    s1, s2, mag = R.channel_sums(x)
    assert (mag >= np.abs(s1)).all()
    fin = R.finalize(s1, s2, B * L, gb, rm, rv, momentum, eps)
    trm, trv = _t(rm).clone(), _t(rv).clone()
    if B * L > 1:
        xhat = F.batch_norm(_t(x), trm, trv, training=True, momentum=momentum, eps=eps)
    else:                                   # torch refuses one value per channel in training mode: the definition
        xhat = torch.zeros(B, C, L, dtype=torch.float64)
        trm, trv = (1 - momentum) * trm + momentum * _t(x)[0, :, 0], (1 - momentum) * trv
    want = _t(gb[:, :C])[:, :, None] * xhat + _t(gb[:, C:])[:, :, None]
    got, bound = R.affine_apply(x, fin['a'][0], fin['s'][0])
    _close(got, want, 1e-9)
    assert (bound >= R.U * np.abs(got) * (1 - 1e-12)).all()
    _close(fin['rm'][0], trm, 1e-12)
    _close(fin['rv'][0], trv, 1e-9)
    if momentum == 0.25 and B * L > 1:                               # the oracle's momentum is 0.1, its eps 1e-5: the statistics alone
        fo = R.finalize(s1, s2, B * L, gb, rm, rv, O.BN_MOMENTUM, O.BN_EPS)
        xh, orm, orv = O.batch_norm_no_affine(_t(x), _t(rm), _t(rv), True)
        _close(fo['rm'][0], orm, 1e-7)                               # (float32(0.1) against 0.1)
        _close(fo['rv'][0], orv, 1e-7)
        _close(R.affine_apply(x, fo['a'][0], fo['s'][0])[0], _t(gb[:, :C])[:, :, None] * xh + _t(gb[:, C:])[:, :, None], 1e-7)


def test_finalize_eval_is_batch_norm_in_eval_mode():
    B, C, L, eps = 3, 5, 20, 2.0 ** -10
    x, gb, rm, rv = _signal(4, B, C, L)
    fin = R.finalize_eval(gb, rm, rv, eps)
    want = _t(gb[:, :C])[:, :, None] * F.batch_norm(_t(x), _t(rm), _t(rv), training=False, eps=eps) + _t(gb[:, C:])[:, :, None]
    _close(R.affine_apply(x, fin['a'][0], fin['s'][0])[0], want, 1e-10)
    xh, orm, orv = O.batch_norm_no_affine(_t(x), _t(rm), _t(rv), False)
    fo = R.finalize_eval(gb, rm, rv, O.BN_EPS)
    _close(R.affine_apply(x, fo['a'][0], fo['s'][0])[0], _t(gb[:, :C])[:, :, None] * xh + _t(gb[:, C:])[:, :, None], 1e-9)


def test_row_and_slice_sums():
    rng = np.random.default_rng(5)
    part = rng.standard_normal((37, 3, 2)).astype(np.float32)
    s, mag = R.row_sums(part)
    assert s.shape == (2, 3)
    _close(s, part.astype(np.float64).sum(0).T)
    _close(mag, np.abs(part.astype(np.float64)).sum(0).T)
    sl, _ = R.slice_sums(part, 128)                                   # 37 rows in 128 slices: 91 of them empty, each row in exactly one
    assert sl.shape == (128, 2, 3) and int((sl[:, 0, 0] == 0).sum()) == 91
    _close(sl.sum(0), s)
    _close(R.slice_sums(part, 1)[0][0], s)


# ---------------------------------------------------------------------------------------------------------------
# the rows are real tile partials, and the stated bound covers a plain fp64 evaluation of the kernels' formula on them
def _kernel_formula_fp64(part, count, gb, rm, rv, momentum, eps):
    """What the three finalising kernels compute, statement by statement, in numpy (fp64 sums in row order, the casts to float32 where the
    code has them)."""
    f32 = np.float32
    C = part.shape[1]
    t = part.astype(np.float64).sum(0)
    mean = t[:, 0] / count
    var = np.maximum(t[:, 1] / count - mean * mean, 0.0)
    rstd = (1.0 / np.sqrt(var + float(f32(eps)))).astype(f32)
    av = (gb[:, :C] * rstd).astype(f32)
    s = (gb[:, C:].astype(np.float64) - av.astype(np.float64) * mean.astype(f32).astype(np.float64)).astype(f32)
    unb = var * (count / (count - 1.0)) if count > 1 else var
    m, rm, rv = float(f32(momentum)), rm.astype(np.float64), rv.astype(np.float64)
    return dict(a=av, s=s, rm=((1 - m) * rm + m * mean).astype(f32), rv=((1 - m) * rv + m * unb).astype(f32), sums=t)


@pytest.mark.parametrize('c', K.COND + K.ONE_LEVEL[:3], ids=K.ids(K.COND + K.ONE_LEVEL[:3]))
def test_the_stated_bound_covers_the_formula_in_fp64_on_fp32_rows(c):
    d = K.draw_rows(c)
    part, count = d['part'], c['count']
    got = _kernel_formula_fp64(part, count, d['gb'], d['rm'], d['rv'], c['momentum'], c['eps'])
    exact, mag = R.row_sums(part)
    fin = R.finalize(got['sums'][:, 0], got['sums'][:, 1], count, d['gb'], d['rm'], d['rv'], c['momentum'], c['eps'])
    ratios = {k: R.worst_ratio(got[k], *fin[k]) for k in ('a', 's', 'rm', 'rv')}
    ratios['sums'] = R.worst_ratio(got['sums'].T, exact, c['ntiles'] * R.U64 * mag)
    print(c['id'], ratios, 'kappa up to %.3g: its term %.3g of 2^-24' % (fin['kappa'].max(), 2.5 * fin['kappa'].max() * R.U64 / R.U))
    assert max(ratios.values()) <= 1.0, ratios
    assert 2.5 * fin['kappa'].max() * R.U64 < 0.1 * R.U                 # the kappa term is never what fills the bound: far from vacuous
    if c['chan'] == 'cond':
        # the rows are a true batch norm: mean and variance from them match the signal's own to the rows' fp32 rounding times kappa
        assert np.abs(fin['mean'] - d['mean']).max() <= 2 * R.U * (np.abs(d['mean']).max() + 1)
        assert (np.abs(fin['var'] - d['var']) <= 8 * R.U * (d['mean'] ** 2 + d['var']) + 1e-12).all()
        k = fin['kappa']
        assert k[0] < 1.01 and 1.9 < k[1] < 2.1 and 60 < k[2] < 70 and 1000 < k[3] < 1050 and k[4] > 1e3 and k[5] == 0


def test_the_clamp_runs():
    """Some channel of the count-1 records, whose rows are (x, float(x^2)), has an exactly negative variance; the constant channel's is within
    the rows' rounding of 0 on either side."""
    neg = 0
    for c in K.COND:
        part = K.draw_rows(c)['part']
        for ch in range(c['C']):
            s1, s2 = (sum(Fraction(float(v)) for v in part[:, ch, j]) for j in (0, 1))
            var = s2 / c['count'] - (s1 / c['count']) ** 2
            neg += var < 0
            if c['chan'] == 'cond' and ch == 4:
                print(c['id'], 'constant channel: exact variance of the rows %.3g' % float(var))
                assert abs(float(var)) < 4 * R.U * 3.1 ** 2
    assert neg > 0


# ---------------------------------------------------------------------------------------------------------------
# the dispatch table: one row per call of every GPU record
ROWS = [(g, c, e) for g, c in K.ALL for e in K.entries(g, c)]


@pytest.mark.parametrize('group,c,e', ROWS, ids=['%s-%s-%s%d' % (g, c['id'], e[0], e[1]) for g, c, e in ROWS])
def test_dispatch_of_every_gpu_record(group, c, e):
    entry, training, rc_want, kernels = e
    rc, names = K.dispatch(entry, c, group, training)
    print(group, c['id'], entry, training, rc, names)
    assert (rc, names) == (rc_want, kernels), (rc, names)


def test_the_table_reaches_all_twelve_kernels_and_every_refusal():
    seen = {n for g, c, e in ROWS for n in e[3]}
    assert sorted(seen) == sorted(K.KERNELS) and len(K.KERNELS) == 12
    per_entry = {}
    for g, c, e in ROWS:
        if e[2] == K.OK:
            per_entry.setdefault(e[0], set()).add(len(e[3]))
    assert per_entry.pop('cond_gamma_beta') == {3} and per_entry.pop('bn_stats') == {2} and all(v == {1} for v in per_entry.values())
    refused = {(e[0], e[2]) for g, c, e in ROWS if e[2] != K.OK}
    assert refused >= {('cond_gamma_beta', K.E_SHAPE), ('cond_gamma_beta', K.E_ARG), ('cond_affine_eval', K.E_SHAPE), ('cond_affine_eval', K.E_ARG),
                       ('cond_sigma', K.E_ARG), ('reduce_slices', K.E_ARG), ('finalize_slices', K.E_ARG), ('affine_apply', K.E_SHAPE)}


def test_affine_apply_refuses_more_rows_than_the_grid_has():
    """gridDim.y ends at 65 535: B * C = 65 536 is V2W_E_SHAPE and launches nothing, 65 535 is served."""
    assert K.dispatch('affine_apply', dict(B=256, C=256, L=7), 'affine') == (K.E_SHAPE, [])
    assert K.dispatch('affine_apply', dict(B=65536, C=1, L=7), 'affine') == (K.E_SHAPE, [])
    assert K.dispatch('affine_apply', dict(B=46341, C=46341, L=7), 'affine') == (K.E_SHAPE, [])          # B * C past 2^31
    assert K.dispatch('affine_apply', dict(B=65535, C=1, L=7), 'affine') == (K.OK, ['affine_apply_kernel'])


def test_the_records_reach_the_loop_edges_they_name():
    nts = {c['ntiles'] for c in K.ONE_LEVEL}
    assert {1, 255, 256, 257, 768, 769, 1024, 1025, 1792, 1793, 4095} <= nts
    assert {K.stats_slice(c['L']) for c in K.BN_STATS} == {64, 128, 192, 320}
    assert [c['n'] for c in K.BN_STATS if c['id'] in ('B1_L4096', 'B1_L4097', 'B1_L8193', 'B1_L16500')] == [2, 2, 3, 4]
    assert {2 * c['C'] for c in K.TWO_LEVEL} >= {2, 48, 256, 272, 512, 40}
    assert all(c['n']['col'] == [2 * x // 8 + 8 for x in c['Cs']] for c in K.CONDS)
