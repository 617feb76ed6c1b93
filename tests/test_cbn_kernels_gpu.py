"""Every record of tests/cbn_cases.py on the device: the twelve kernels of csrc/v2w_cbn.hip behind their eleven entry points, each quantity a
call leaves in memory against the fp64 statement of its own step (tests/cbn_ref.py), per entry.  tests/test_cbn_ref_cpu.py asserts which
kernels each call launches.

The chain is cut at every buffer: z_ws against fp64 of the inputs, the new v against fp64 of (W, old u), the new u and sigma against fp64 of W
and the device's v, gb against fp64 of the device's z_ws and sigma_ws; sums against the extended-precision sum of the rows; (a, s) and the
running statistics against exact rationals of the device's own stats / slices.  A quantity fails when |got - want| exceeds its bound
(n * 2^-24 * S with n from cbn_cases.py, first-order propagation through quotients, the kappa * 2^-53 term of the one-pass variance carried from
the record's data).  Outputs start as NaN with sentinel guards on both sides, inputs lie between NaN guards, everything a call has no business
writing keeps its bits, every call runs twice from restored buffers and must give the same bits.  Each test prints its worst error / bound
ratio (`-s` shows them; DESIGN.md 3e'''' records them).

Worst ratios on an MI355X when these tests were written: every fp64 sum of rows and every slice 0 (exact: 224 positions of magnitude ~1 per
row leave fp64 room for thousands of rows); bn_stats sums 0.0023, squares 0.32; z 0.040, new v 0.074, new u 0.12, sigma 0.054 (0.0085 in eval
mode), gb 0.17, the one-launch eval (a, s) 0.11; (a, s) of the finalisers 0.82 / 0.93, running mean / variance 0.99 / 0.99, v2w_affine_apply 0.997.
The last three sit near 1 because their bounds are one or two roundings and nothing else: a running statistic is one cast of an fp64 value
(bound 2^-24 |value|, which a correctly rounded result attains), an output of v2w_affine_apply is one fma, a = gamma * (float)rstd is two
roundings against 2 * 2^-24 |a|.  The one-pass variance at mean / std 0, 1, 8, 32 (L = 4 097, n = 2) leaves a within 3.5e-8, 5.1e-8, 7.7e-8,
3.5e-8 of the two-pass fp64 value (relative), against 1.5 kappa n 2^-24 = 3.0e-7 .. 1.8e-4.  The file takes 5 s, its slowest record 0.38 s
(the first, which loads the library), the next 0.20 s (C = 256).

One-line mutants of csrc/v2w_cbn.hip, each built into a library of its own and run once (new records that fail / earlier tests that fail):
the unbiased factor dropped in bn_reduce_finalize_kernel: 19 one-level records (all but the two count-1) / 5 (the bit-for-bit test);
dropped in bn_finalize_slices_kernel: 21 two-level records / none; the two statistics swapped in bn_reduce_slices_kernel: all 23 two-level
records / 5; the single-element tail of bn_stats_kernel removed: 45 of the 49 bn_stats records (L = 8 192 fills every slice of 128: no
tail) / 5; sigma from the old u in cond_sn_kernel: 36 conditioning records / 2; the beta row read as the gamma row in
cond_affine_eval_kernel: 32 / 2; `fmaf(-av, mean, beta)` as `beta - av` in bn_finalize_kernel: 47 / 17; `count > 1.0` as `count > 0.0`
in bn_finalize_kernel: the 4 count-1 records / 1.  DESIGN.md 3e'''' has the table."""
import numpy as np
import pytest
import torch

from tests import cbn_cases as K
from tests import cbn_ref as R
from tests.test_disc_kernels_gpu import NAN, SENT, _cases, _report, env  # noqa: F401  (env: the module-scoped fixture)
from tests.test_tile_kernels_gpu import GUARD, _sync_or_stop

pytestmark = pytest.mark.gpu

_INT = {torch.float32: torch.int32, torch.float64: torch.int64, torch.int64: torch.int64}


class Arr:
    """A flat device buffer [GUARD | payload | GUARD]; `ptr` is the payload's address (GUARD elements in: 8-byte aligned at least)."""

    def __init__(self, dev, payload, guard):
        payload = torch.as_tensor(payload)
        n = payload.numel()
        flat = torch.full((2 * GUARD + n,), int(SENT) if payload.dtype == torch.int64 else guard, dtype=payload.dtype)
        flat[GUARD:GUARD + n] = payload.reshape(-1)
        self.flat, self.n, self.shape = flat.to(dev), n, tuple(payload.shape)
        self.first = self.flat.clone()
        self.ptr = self.flat.data_ptr() + GUARD * payload.element_size()
        assert self.ptr % 8 == 0

    def restore(self):
        self.flat.copy_(self.first)

    def bits(self):
        return self.flat.view(_INT[self.flat.dtype]).clone()

    def get(self):
        return self.flat[GUARD:GUARD + self.n].cpu().view(self.shape).numpy()

    def unchanged(self, keep=None):
        """The whole buffer (keep = None) or its guards and the payload elements where `keep` is True hold their first bits."""
        same = self.flat.view(_INT[self.flat.dtype]) == self.first.view(_INT[self.flat.dtype])
        if keep is not None:
            k = torch.ones(self.flat.numel(), dtype=torch.bool)
            k[GUARD:GUARD + self.n] = torch.as_tensor(keep).reshape(-1)
            same = same | ~k.to(same.device)
        return bool(same.all())


def _inp(dev, x):
    return Arr(dev, x, NAN)                                  # an input between NaN guards


def _out(dev, *shape, dtype=torch.float32):
    return Arr(dev, torch.full(shape, NAN, dtype=dtype), SENT)   # an output: NaN, sentinels on both sides


def _state(dev, x):
    return Arr(dev, x, SENT)                                 # updated in place


def _addr(A):
    return {k: ([a.ptr for a in v] if isinstance(v, list) else v.ptr) for k, v in A.items()}


def _all(A):
    return [a for v in A.values() for a in (v if isinstance(v, list) else [v])]


def _twice(A, what, run, before=None):
    """run() twice, each time from the buffers' first contents; the two runs must leave the same bits everywhere.  -> run()'s value."""
    snaps = []
    for _ in range(2):
        for a in _all(A):
            a.restore()
        if before:
            before()
        torch.cuda.synchronize()
        rv = run()
        _sync_or_stop(what)
        snaps.append([a.bits() for a in _all(A)])
    assert all(torch.equal(x, y) for x, y in zip(*snaps)), what + ': two runs differ'
    return rv


def _kept(A, written, what):
    """Guards everywhere; whole buffers outside `written`."""
    for k, v in A.items():
        for i, a in enumerate(v if isinstance(v, list) else [v]):
            if k in written:
                assert a.unchanged(keep=np.zeros(a.shape, dtype=bool)), '%s: %s[%d] guards' % (what, k, i)
            else:
                assert a.unchanged(), '%s: %s[%d] was written' % (what, k, i)


# ---------------------------------------------------------------------------------------------------------------
# partial rows: the one-level reduce, the three finalisers, the two-level pair
def _bn_arrs(dev, c, d):
    B, C = c['B'], c['C']
    return dict(part=_inp(dev, d['part']), gb=_inp(dev, d['gb']), rm=_state(dev, d['rm']), rv=_state(dev, d['rv']),
                nbt=_state(dev, torch.tensor([41], dtype=torch.int64)), a=_out(dev, B, C), s=_out(dev, B, C))


def _fin_ratios(A, fin, tag=''):
    return {tag + k: R.worst_ratio(A[k].get(), *fin[k]) for k in ('a', 's', 'rm', 'rv')}


def _check_sums(A, c, d, name):
    C = c['C']
    st = A['stats'].get()
    want, mag = R.row_sums(d['part'])
    assert st[2 * C] == c['count'], name
    return dict(sums=R.worst_ratio(st[:C], want[0], c['ntiles'] * R.U64 * mag[0]), sumsq=R.worst_ratio(st[C:2 * C], want[1], c['ntiles'] * R.U64 * mag[1]))


@_cases(K.ONE_LEVEL)
def test_one_level_reduce_and_both_finalisers(env, c):
    dev, _hip, lib, st = env
    d, C = K.draw_rows(c), c['C']
    A = dict(_bn_arrs(dev, c, d), stats=_out(dev, 2 * C + 1, dtype=torch.float64))
    t, name = _addr(A), 'one_level ' + c['id']

    def two_calls():
        return K.call('reduce_partials', c, t, st)[0], K.call('finalize', c, t, st, training=1)[0]

    assert _twice(A, name, two_calls) == (K.OK, K.OK)
    _kept(A, {'stats', 'rm', 'rv', 'nbt', 'a', 's'}, name)
    ratios = _check_sums(A, c, d, name)
    stats = A['stats'].get()
    fin = R.finalize(stats[:C], stats[C:2 * C], c['count'], d['gb'], d['rm'], d['rv'], c['momentum'], c['eps'])
    ratios.update(_fin_ratios(A, fin))
    assert A['nbt'].get()[0] == 42
    two = [a.bits() for a in _all(A)]
    # the one-launch form: the same bits everywhere, and (again) within the bounds
    assert _twice(A, name + ' fused', lambda: K.call('reduce_finalize', c, t, st)[0]) == K.OK
    _kept(A, {'stats', 'rm', 'rv', 'nbt', 'a', 's'}, name + ' fused')
    assert all(torch.equal(x, y.bits()) for x, y in zip(two, _all(A))), name + ': v2w_bn_reduce_finalize differs from the two calls'
    ratios.update({'f_' + k: v for k, v in _check_sums(A, c, d, name).items()})
    ratios.update(_fin_ratios(A, fin, 'f_'))
    assert A['nbt'].get()[0] == 42
    _report(name, **ratios)


@_cases(K.TWO_LEVEL + K.REFUSED_SLICES)
def test_two_level_reduce_and_finalize(env, c):
    dev, _hip, lib, st = env
    d, C, ns, nt = K.draw_rows(c), c['C'], c['nslices'], c['ntiles']
    nsb = max(1, min(ns, 1024))
    A = dict(_bn_arrs(dev, c, d), slices=_out(dev, nsb + 1, 2, C, dtype=torch.float64))        # one slice more than the call owns
    t, name = _addr(A), 'two_level ' + c['id']

    def two_calls():
        return K.call('reduce_slices', c, t, st)[0], K.call('finalize_slices', c, t, st)[0]

    assert _twice(A, name, two_calls) == (c['rc'], c['rc'])
    if c['rc'] != K.OK:
        _kept(A, set(), name)
        return
    _kept(A, {'slices', 'rm', 'rv', 'nbt', 'a', 's'}, name)
    own = np.zeros((nsb + 1, 2, C), dtype=bool)
    own[:ns] = True
    assert A['slices'].unchanged(keep=~own), name + ': wrote past nslices * 2 C'
    sl = A['slices'].get()[:ns]
    want, mag = R.slice_sums(d['part'], ns)
    rows_in = np.array([nt * (s + 1) // ns - nt * s // ns for s in range(ns)], dtype=np.float64)[:, None, None]
    ratios = dict(slices=R.worst_ratio(sl, want, rows_in * R.U64 * mag))
    assert (sl[rows_in[:, 0, 0] == 0] == 0).all()                                                  # empty slices: exact zeros
    # (a, s), the running statistics: from the device's slices, whose sum the kernel takes in fp64 (nslices additions)
    tot, tmag = sl.astype(np.longdouble).sum(0), np.abs(sl).astype(np.longdouble).sum(0)
    fin = R.finalize(tot[0].astype(np.float64), tot[1].astype(np.float64), c['count'], d['gb'], d['rm'], d['rv'], c['momentum'], c['eps'],
                     ds1=((ns + 1) * R.U64 * tmag[0]).astype(np.float64), ds2=((ns + 1) * R.U64 * tmag[1]).astype(np.float64))
    ratios.update(_fin_ratios(A, fin))
    assert A['nbt'].get()[0] == 42
    # against the one-level form: both within their bounds of the rows' own sums
    ex, emag = R.row_sums(d['part'])
    fx = R.finalize(ex[0].astype(np.float64), ex[1].astype(np.float64), c['count'], d['gb'], d['rm'], d['rv'], c['momentum'], c['eps'],
                    ds1=((nt + ns + 1) * R.U64 * emag[0]).astype(np.float64), ds2=((nt + ns + 1) * R.U64 * emag[1]).astype(np.float64))
    got2 = {k: A[k].get().copy() for k in ('a', 's', 'rm', 'rv')}
    ratios.update(_fin_ratios(A, fx, 'x2_'))
    A1 = dict(_bn_arrs(dev, c, d), stats=_out(dev, 2 * C + 1, dtype=torch.float64))
    t1 = _addr(A1)
    assert (K.call('reduce_partials', c, t1, st)[0], K.call('finalize', c, t1, st, training=1)[0]) == (K.OK, K.OK)
    _sync_or_stop(name + ' one level')
    ratios.update(_fin_ratios(A1, fx, 'x1_'))
    for k in got2:
        assert (np.abs(got2[k].astype(np.float64) - A1[k].get()) <= 2 * fx[k][1]).all(), name + ': the two forms differ in ' + k
    _report(name, **ratios)


@_cases(K.FIN_EVAL)
def test_finalize_in_eval_mode(env, c):
    dev, _hip, lib, st = env
    d, B, C = K.draw_eval(c), c['B'], c['C']
    A = dict(gb=_inp(dev, d['gb']), rm=_inp(dev, d['rm']), rv=_inp(dev, d['rv']), nbt=_state(dev, torch.tensor([41], dtype=torch.int64)),
             a=_out(dev, B, C), s=_out(dev, B, C))
    t, name = dict(_addr(A), stats=None), 'fin_eval ' + c['id']
    assert _twice(A, name, lambda: K.call('finalize', c, t, st, training=0)[0]) == K.OK
    _kept(A, {'a', 's'}, name)                                             # the running statistics and the counter keep their bits
    fin = R.finalize_eval(d['gb'], d['rm'], d['rv'], c['eps'])
    _report(name, a=R.worst_ratio(A['a'].get(), *fin['a']), s=R.worst_ratio(A['s'].get(), *fin['s']))


# ---------------------------------------------------------------------------------------------------------------
# v2w_bn_stats
@_cases(K.BN_STATS + K.BN_STATS_COND)
def test_bn_stats(env, c):
    dev, _hip, lib, st = env
    d, B, C, L = K.draw_stats(c), c['B'], c['C'], c['L']
    nws = 2 * C * K.BN_SPLITS
    A = dict(x=_inp(dev, d['x']), stats=_out(dev, 2 * C + 1, dtype=torch.float64), partial=_out(dev, nws + 128, dtype=torch.float64))
    t, name = _addr(A), 'bn_stats ' + c['id']
    assert _twice(A, name, lambda: K.call('bn_stats', c, t, st)[0]) == K.OK
    _kept(A, {'stats', 'partial'}, name)
    own = np.arange(nws + 128) < nws
    assert A['partial'].unchanged(keep=~own) and np.isfinite(A['partial'].get()[:nws]).all(), name + ': only the first 2 C 64 doubles of partial_ws'
    stats = A['stats'].get()
    s1, s2, mag = R.channel_sums(d['x'])
    assert stats[2 * C] == B * L
    ratios = dict(sums=R.worst_ratio(stats[:C], s1, R.stats_bound(c['n'], B, mag)), sumsq=R.worst_ratio(stats[C:2 * C], s2, R.stats_bound(c['n'], B, s2)))
    if c['chan'] == 'cond':
        # finalised by v2w_bn_finalize: within the bound of its own stats, and the one-pass formula's loss against the two-pass fp64 value
        F = dict(stats=A['stats'], gb=_inp(dev, d['gb']), rm=_state(dev, d['rm']), rv=_state(dev, d['rv']),
                 nbt=_state(dev, torch.tensor([41], dtype=torch.int64)), a=_out(dev, B, C), s=_out(dev, B, C))
        cf = dict(c, momentum=0.1, eps=1e-5)
        assert K.call('finalize', cf, _addr(F), st, training=1)[0] == K.OK
        _sync_or_stop(name + ' finalize')
        fin = R.finalize(stats[:C], stats[C:2 * C], B * L, d['gb'], d['rm'], d['rv'], 0.1, 1e-5)
        ratios.update(_fin_ratios(F, fin))
        x = d['x'].astype(np.float64)
        mean = x.mean((0, 2))
        var = ((x - mean[None, :, None]) ** 2).mean((0, 2))
        e = float(np.float32(1e-5))
        kappa = (var + mean ** 2) / (var + e)
        a2 = d['gb'][:, :C].astype(np.float64) / np.sqrt(var + e)
        rel = np.abs(F['a'].get() - a2) / np.abs(a2)
        allowed = R.one_pass_loss_bound(kappa, c['n']) + fin['a'][1] / np.abs(a2)
        for ch in range(C):
            print('[one-pass] mean/std %g: kappa %.4g, |a - two-pass| / |a| = %.3g, bound %.3g' % (K.RATIOS[ch % 4], kappa[ch], rel[:, ch].max(), allowed[:, ch].min()))
        ratios['one_pass'] = float((rel / allowed).max())
    _report(name + ' n=%d' % c['n'], **ratios)


# ---------------------------------------------------------------------------------------------------------------
# cond_*
def _cond_arrs(dev, c, d):
    n, B = len(d['stages']), c['B']
    per = lambda key, make: [make(dev, s[key]) for s in d['stages']]  # noqa: E731
    A = dict(spk=_inp(dev, d['spk']), sn_w=per('sn_w', _inp), sn_b=per('sn_b', _inp), sn_u=per('sn_u', _state), sn_v=per('sn_v', _state),
             rm=per('rm', _inp), rv=per('rv', _inp), gb=[_out(dev, B, 2 * Cs) for Cs in c['Cs'][:n]], a=[_out(dev, B, Cs) for Cs in c['Cs'][:n]],
             s=[_out(dev, B, Cs) for Cs in c['Cs'][:n]], z_ws=_out(dev, n, B, 128), sigma_ws=_out(dev, n))
    if d['noise'] is not None:
        A['noise'] = _inp(dev, d['noise'])
    if c['fc']:
        A['fc_w'] = per('fc_w', _inp)
    if c['fc_b']:
        A['fc_b'] = per('fc_b', _inp)
    return A


def _check_sn(c, d, A, training, name):
    """The new v, the new u and sigma of every stage (training), sigma alone with u and v untouched (eval)."""
    r = {}
    n = c['n']
    sig = A['sigma_ws'].get()
    for i, s in enumerate(d['stages']):
        W = s['sn_w']
        if training:
            v_dev, u_dev = A['sn_v'][i].get(), A['sn_u'][i].get()
            r['v'] = max(r.get('v', 0), R.worst_ratio(v_dev, *R.sn_new_v(W, s['sn_u'], n['col'][i], n['sq_v'])))
            u, du, wv, dwv = R.sn_new_u(W, v_dev, n['row'], n['sq_u'][i])
            r['u'] = max(r.get('u', 0), R.worst_ratio(u_dev, u, du))
        else:
            u, du = s['sn_u'], 0.0
            wv, dwv = R.sn_wv(W, s['sn_v'], n['row'])
        r['sigma'] = max(r.get('sigma', 0), R.worst_ratio(sig[i], *R.sn_sigma(u, du, wv, dwv, n['sq_u'][i])))
    return r


def _check_gb(c, d, A):
    r = dict(z=0.0, gb=0.0)
    z_dev, sig = A['z_ws'].get(), A['sigma_ws'].get()
    for i, s in enumerate(d['stages']):
        z, S = R.cond_z(d['spk'], d['noise'], s['fc_w'] if c['fc'] else None, s['fc_b'] if c['fc'] else None)
        r['z'] = max(r['z'], R.worst_ratio(z_dev[i], z, c['n']['z'] * R.U * S))
        r['gb'] = max(r['gb'], R.worst_ratio(A['gb'][i].get(), *R.gamma_beta(s['sn_w'], s['sn_b'], z_dev[i], sig[i], c['n']['row'])))
    return r


@_cases(K.CONDS + K.COND_REFUSED)
def test_conditioning(env, c):
    dev, _hip, lib, st = env
    d = K.draw_cond(c)
    A = _cond_arrs(dev, c, d)
    t, name = dict(noise=None, fc_w=[None] * 8, fc_b=[None] * 8), 'cond ' + c['id']
    t.update(_addr(A))
    ratios, bits = {}, {}
    for training in (1, 0):
        tag = 'train' if training else 'eval'
        # v2w_cond_gamma_beta
        assert _twice(A, name, lambda: K.call('cond_gamma_beta', c, t, st, training)[0]) == c['rc'], name
        if c['rc'] != K.OK:
            _kept(A, set(), name)
        else:
            _kept(A, {'z_ws', 'sigma_ws', 'gb'} | ({'sn_u', 'sn_v'} if training else set()), name)
            ratios.update({'%s_%s' % (tag, k): v for k, v in {**_check_sn(c, d, A, training, name), **_check_gb(c, d, A)}.items()})
            bits[training] = [A[k].bits() if k == 'sigma_ws' else [a.bits() for a in A[k]] for k in ('sigma_ws', 'sn_u', 'sn_v')]
        # v2w_cond_sigma: the same sigma, u and v, bit for bit, and nothing else
        assert _twice(A, name, lambda: K.call('cond_sigma', c, t, st, training)[0]) == c['rc_sigma'], name
        if c['rc_sigma'] != K.OK:
            _kept(A, set(), name)
            continue
        _kept(A, {'sigma_ws'} | ({'sn_u', 'sn_v'} if training else set()), name + ' sigma')
        ratios.update({'%s_sigma_%s' % (tag, k): v for k, v in _check_sn(c, d, A, training, name).items()})
        if training in bits:
            now = [A[k].bits() if k == 'sigma_ws' else [a.bits() for a in A[k]] for k in ('sigma_ws', 'sn_u', 'sn_v')]
            assert torch.equal(now[0], bits[training][0]) and all(torch.equal(x, y) for j in (1, 2) for x, y in zip(now[j], bits[training][j])), name
    # v2w_cond_affine_eval on the eval-mode sigma in memory: one launch, no intermediates
    have_sigma = c['rc_sigma'] == K.OK
    sigma = A['sigma_ws'].flat.clone()

    def put_sigma():
        if have_sigma:
            A['sigma_ws'].flat.copy_(sigma)

    assert _twice(A, name, lambda: K.call('cond_affine_eval', c, t, st)[0], before=put_sigma) == c['rc_eval'], name
    A['sigma_ws'].first = sigma if have_sigma else A['sigma_ws'].first
    _kept(A, {'a', 's'} if c['rc_eval'] == K.OK else set(), name + ' affine_eval')                  # gb, z_ws, u, v, sigma keep their bits
    if c['rc_eval'] == K.OK:
        sig = A['sigma_ws'].get()
        ra = rs = 0.0
        for i, s in enumerate(d['stages']):
            z, S = R.cond_z(d['spk'], d['noise'], s['fc_w'] if c['fc'] else None, s['fc_b'] if c['fc'] else None)
            gbv, dgb = R.gamma_beta(s['sn_w'], s['sn_b'], z, sig[i], c['n']['row'], dz=c['n']['z_eval'] * R.U * S)
            a, da, sv, ds = R.affine_eval(gbv, dgb, s['rm'], s['rv'], K.EVAL_EPS[i % 2])
            ra, rs = max(ra, R.worst_ratio(A['a'][i].get(), a, da)), max(rs, R.worst_ratio(A['s'][i].get(), sv, ds))
        ratios.update(affine_a=ra, affine_s=rs)
    _report(name, **ratios)


# ---------------------------------------------------------------------------------------------------------------
# v2w_affine_apply
@_cases(K.AFFINE + K.AFFINE_EDGE + K.AFFINE_REFUSED)
def test_affine_apply(env, c):
    dev, _hip, lib, st = env
    d, B, C, L = K.draw_affine(c), c['B'], c['C'], c['L']
    A = dict(x=_inp(dev, d['x']), a=_inp(dev, d['a']), s=_inp(dev, d['s']), out=_out(dev, B, C, L))
    t, name = _addr(A), 'affine ' + c['id']
    assert _twice(A, name, lambda: K.call('affine_apply', c, t, st)[0]) == c['rc']
    _kept(A, {'out'} if c['rc'] == K.OK else set(), name)
    if c['rc'] == K.OK:
        _report(name, out=R.worst_ratio(A['out'].get(), *R.affine_apply(d['x'], d['a'], d['s'])))
