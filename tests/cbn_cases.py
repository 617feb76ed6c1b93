"""The cases of tests/test_cbn_kernels_gpu.py: one record per call sequence on the conditional batch norm forward (csrc/v2w_cbn.hip: twelve
kernels behind eleven entry points), with the kernels each entry must launch, its return code, and the chain lengths n of its bounds.

tests/test_cbn_ref_cpu.py drives every record through the name sink (host-only, made-up addresses) and asserts kernels and return codes; the
GPU tests run the same records on real tensors.  `call` builds the arguments of both runs from one table of addresses.

n (the bound of a sum is n * 2^-24 * S, tests/cbn_ref.py) counts the fp32 roundings on an entry's longest chain, as the kernel's code has them:
  z            cond_fc_kernel: D fmas in a row, the bias add                                                   D + 1      (0: no fcs layer, a copy)
  W^T u        cond_sn_kernel: ceil(R / 8) fmas per thread, eight partial columns added in order               ceil(R / 8) + 8
  |col|^2      one product, six shuffle adds, sixteen wave totals                                              23
  W v, W z     two products (the second fused with their add), six shuffle adds                                8
  |W v|^2, u . (W v)   ceil(R / 1024) products and adds per thread, 6 + 16 for the block, one product rounding ceil(R / 1024) + 23
  z (eval)     cond_affine_eval_kernel: ceil(D / 64) fmas per lane, six shuffle adds, the bias add             ceil(D / 64) + 7
  bn_stats     a lane's chain per batch item, ceil(slice / 128) terms, the pair's add                          ceil(slice / 128) + 1
col * (1 / norm) is two roundings where a quotient is one (cbn_ref.quotient's `roundings`)."""
import ctypes as C
import functools

import numpy as np

from wavthruvec_pytorch_amd import _hip

from tests.disc_cases import OK, _case, ids  # noqa: F401  (ids: re-exported for the parametrisations)
from tests.disc_ref import ceil_div

E_ARG, E_SHAPE = -1, -2
BN_SPLITS, BN_SLICES, MAX_STAGES = 64, 128, 8
TILE = 224                                  # positions per partial row, as the fused stage kernels write them


# ---------------------------------------------------------------------------------------------------------------
# partial rows [ntiles][C][2] and what reduces and finalises them.  chan: how the rows are drawn (draw_rows below)
#   'std'    per channel mean 0.5 randn, std in [0.5, 1.5]
#   'cond'   channel c: mean / std = (0, 1, 8, 32)[c % 4], except channel 4 constant at 3.1 and channel 5 all zeros
#   'count1' one row (x, x^2), count = 1
ONE = ['bn_reduce_partials_kernel']
FIN = ['bn_finalize_kernel']
FUSED = ['bn_reduce_finalize_kernel']
SLICES = ['bn_reduce_slices_kernel']
FIN_SLICES = ['bn_finalize_slices_kernel']


def rows(id, *, C, B, ntiles, chan='std', momentum=0.1, eps=1e-5, nslices=BN_SLICES, rc=OK):
    count = 1 if chan == 'count1' else TILE * ntiles
    return _case(id, ONE + FIN + FUSED, rc, C=C, B=B, ntiles=ntiles, chan=chan, momentum=momentum, eps=eps, nslices=nslices, count=count)


# the edges of bn_rows_of_channel's two loops (t + 768 < ntiles, step 1024; t < ntiles, step 256), one and odd channel counts, B past the
# block's 256 threads, B = 1
ONE_LEVEL = [rows('nt%d' % _n, C=16, B=3, ntiles=_n) for _n in (1, 255, 256, 257, 768, 769, 1024, 1025, 1792, 1793, 4095)]
ONE_LEVEL += [rows('C1', C=1, B=3, ntiles=300), rows('C24', C=24, B=3, ntiles=300), rows('B300', C=16, B=300, ntiles=300),
              rows('B1', C=16, B=1, ntiles=300)]

# two-level: empty slices below 128 rows, one and 1024 slices, the column passes of bn_reduce_slices_kernel (W = 2 C against 256), the partly
# empty second block of bn_finalize_slices_kernel (C = 20), its trips of 16 samples
TWO_LEVEL = [rows('s128_nt%d' % _n, C=16, B=3, ntiles=_n) for _n in (1, 127, 128, 129, 4096, 4100)]
TWO_LEVEL += [rows('s1_nt1500', C=16, B=3, ntiles=1500, nslices=1), rows('s1024_nt1500', C=16, B=3, ntiles=1500, nslices=1024)]
TWO_LEVEL += [rows('s128_C%d' % _c, C=_c, B=3, ntiles=300) for _c in (1, 24, 128, 136, 256, 20)]
TWO_LEVEL += [rows('s128_B%d' % _b, C=16, B=_b, ntiles=300) for _b in (1, 16, 17)]
REFUSED_SLICES = [rows('s0_refused', C=16, B=3, ntiles=300, nslices=0, rc=E_ARG), rows('s1025_refused', C=16, B=3, ntiles=300, nslices=1025, rc=E_ARG)]

# conditioning of the variance, on each of the three finalising kernels
COND = [rows('cond_m%g_eps%g' % (_m, _e), C=16, B=3, ntiles=300, chan='cond', momentum=_m, eps=_e) for _m in (0.1, 1.0) for _e in (1e-5, 1e-3)]
COND += [rows('count1_m%g_eps%g' % (_m, _e), C=16, B=3, ntiles=1, chan='count1', momentum=_m, eps=_e) for _m, _e in ((0.1, 1e-5), (1.0, 1e-3))]
ONE_LEVEL += COND
TWO_LEVEL += COND

# v2w_bn_finalize in eval mode: the running statistics as they are, nothing but (a, s) written
FIN_EVAL = [_case('eval_C16_B3', FIN, C=16, B=3, eps=1e-5), _case('eval_C20_B17', FIN, C=20, B=17, eps=1e-3)]


# ---------------------------------------------------------------------------------------------------------------
# v2w_bn_stats: slice = roundup64(ceil(L / 64)): 64 up to L = 4096 (splits past ceil(L / 64) are empty), 128 from 4097, 192 at 8 193, 320 at 16 500;
# the paired loop (l + 64 < hi) runs from slice 128 on, once at 128 and twice (with a single-element tail trip) at 320; B < 4 leaves waves idle,
# B = 5 gives wave 0 two items
def stats_slice(L):
    return (ceil_div(L, BN_SPLITS) + 63) // 64 * 64


def stats(id, *, B, C, L, chan='std'):
    return _case(id, ['bn_stats_kernel', 'bn_reduce_kernel'], B=B, C=C, L=L, chan=chan, slice=stats_slice(L), n=ceil_div(stats_slice(L), 128) + 1)


BN_STATS = [stats('B%d_L%d' % (_b, _l), B=_b, C=2, L=_l) for _b in (1, 3, 4, 5) for _l in (1, 63, 64, 65, 127, 128, 129, 4096, 4097, 8192, 8193, 16500)]
BN_STATS_COND = [stats('ratios_L4097', B=3, C=4, L=4097, chan='cond')]                     # channel c: mean / std = (0, 1, 8, 32)[c]


# ---------------------------------------------------------------------------------------------------------------
# cond_*: one record = v2w_cond_gamma_beta and v2w_cond_sigma in both modes, v2w_cond_affine_eval
COND_KERNELS = ['cond_fc_kernel', 'cond_sn_kernel', 'cond_linear_kernel']
STAGES = dict(gen=[256, 128, 64, 32, 16], c8=[8], c40=[40], c1024=[1024], eight=[16] * 8)


def cond(id, Cs, B, spk_dim, noise_dim, *, fc=True, fc_b=None, rc=OK, rc_eval=None, rc_sigma=OK):
    """fc: the stages have an fcs layer.  fc_b: None as fc; else whether fc_b is given (one of the two: refused)."""
    D = spk_dim + noise_dim
    n = dict(z=D + 1 if fc else 0, z_eval=ceil_div(D, 64) + 7 if fc else 0, row=8, sq_v=23,
             col=[ceil_div(2 * c, 8) + 8 for c in Cs], sq_u=[ceil_div(2 * c, 1024) + 23 for c in Cs])
    return _case(id, COND_KERNELS if rc == OK else [], rc, Cs=list(Cs), B=B, spk_dim=spk_dim, noise_dim=noise_dim, fc=fc, fc_b=fc if fc_b is None else fc_b,
                 rc_eval=rc if rc_eval is None else rc_eval, rc_sigma=rc_sigma, n=n)


CONDS = [cond('%s_B%d_d%d_%d' % (_s, _b, _sd, _nd), STAGES[_s], _b, _sd, _nd)
         for _s in STAGES for _b in (1, 5) for _sd, _nd in ((192, 192), (100, 0), (70, 33))]
CONDS += [cond('gen_B5_nofc_64_64', STAGES['gen'], 5, 64, 64, fc=False), cond('gen_B5_nofc_128_0', STAGES['gen'], 5, 128, 0, fc=False)]
COND_REFUSED = [
    cond('nofc_dim127_refused', [16], 2, 64, 63, fc=False, rc=E_SHAPE),
    cond('fc_w_without_fc_b_refused', [16], 2, 64, 64, fc=True, fc_b=False, rc=E_ARG),
    cond('fc_b_without_fc_w_refused', [16], 2, 64, 64, fc=False, fc_b=True, rc=E_ARG),
    cond('nine_stages_refused', [16] * 9, 2, 64, 64, rc=E_ARG, rc_sigma=E_ARG),
    cond('eval_lds_48k_refused', [16], 1, 12289, 0, rc=OK, rc_eval=E_SHAPE),           # D * 4 = 49 156 bytes: only the one-launch form refuses
]


# ---------------------------------------------------------------------------------------------------------------
# v2w_affine_apply: the grid caps at 64 blocks of 256, so 16 384 positions take one grid-stride trip and 16 385 two
def affine(id, *, B, C, L, rc=OK):
    return _case(id, ['affine_apply_kernel'] if rc == OK else [], rc, B=B, C=C, L=L)


AFFINE = [affine('L%d' % _l, B=2, C=3, L=_l) for _l in (1, 255, 256, 257, 16384, 16385)]
AFFINE_REFUSED = [affine('rows_65536_refused', B=256, C=256, L=1, rc=E_SHAPE)]          # gridDim.y ends at 65 535
AFFINE_EDGE = [affine('rows_65535', B=255, C=257, L=1)]                                 # the largest grid the launch takes

TABLE = dict(one_level=ONE_LEVEL, two_level=TWO_LEVEL + REFUSED_SLICES, fin_eval=FIN_EVAL, bn_stats=BN_STATS + BN_STATS_COND,
             cond=CONDS + COND_REFUSED, affine=AFFINE + AFFINE_EDGE + AFFINE_REFUSED)
KERNELS = ['cond_fc_kernel', 'cond_sn_kernel', 'cond_linear_kernel', 'cond_affine_eval_kernel', 'bn_stats_kernel', 'bn_reduce_kernel',
           'bn_reduce_partials_kernel', 'bn_reduce_slices_kernel', 'bn_finalize_slices_kernel', 'bn_finalize_kernel', 'bn_reduce_finalize_kernel',
           'affine_apply_kernel']


# ---------------------------------------------------------------------------------------------------------------
# the calls, from a table of addresses (made up here, real ones in the GPU tests)
def fake(c, group):
    """8-byte aligned addresses nothing reads, by operand name; per-stage operands as lists."""
    names = ('part', 'stats', 'slices', 'gb', 'rm', 'rv', 'nbt', 'a', 's', 'x', 'partial', 'out', 'spk', 'noise', 'z_ws', 'sigma_ws')
    t = {name: 0x10000000 + 0x1000000 * i for i, name in enumerate(names)}
    if group == 'cond':
        for j, name in enumerate(('fc_w', 'fc_b', 'sn_w', 'sn_b', 'sn_u', 'sn_v', 'gb', 'rm', 'rv', 'a', 's')):
            t[name] = [0x40000000 + 0x8000000 * j + 0x100000 * i for i in range(len(c['Cs']))]
    return t


def cond_struct(c, t, training):
    """v2w_cond_eval_args (its `.c` is the v2w_cond_args of the other two entry points).  More than V2W_MAX_STAGES stages: the arrays hold
    the first eight and n_stages says nine."""
    e = _hip.CondEvalArgs()
    a = e.c
    a.spk, a.noise = t['spk'], (t['noise'] if c['noise_dim'] > 0 else None)
    for i in range(min(len(c['Cs']), MAX_STAGES)):
        a.fc_w[i], a.fc_b[i] = (t['fc_w'][i] if c['fc'] else None), (t['fc_b'][i] if c['fc_b'] else None)
        a.sn_w[i], a.sn_b[i], a.sn_u[i], a.sn_v[i], a.gb[i], a.C[i] = t['sn_w'][i], t['sn_b'][i], t['sn_u'][i], t['sn_v'][i], t['gb'][i], c['Cs'][i]
        e.running_mean[i], e.running_var[i], e.a_out[i], e.s_out[i], e.eps[i] = t['rm'][i], t['rv'][i], t['a'][i], t['s'][i], EVAL_EPS[i % 2]
    a.z_ws, a.sigma_ws = t['z_ws'], t['sigma_ws']
    a.n_stages, a.B, a.spk_dim, a.noise_dim, a.training = len(c['Cs']), c['B'], c['spk_dim'], c['noise_dim'], int(training)
    return e


EVAL_EPS = (1e-5, 1e-3)             # eps of stage i in v2w_cond_affine_eval: EVAL_EPS[i % 2]


def call(entry, c, t, stream=None, training=1):
    """Run `entry` of record c on the addresses t: with a stream for real, without one through the name sink -> (rc, kernel names or None)."""
    lib = _hip.load()
    f32 = C.c_float
    if entry == 'reduce_partials':
        fn, args = lib.v2w_bn_reduce_partials, (t['part'], c['ntiles'], c['C'], float(c['count']), t['stats'])
    elif entry == 'finalize':
        fn, args = lib.v2w_bn_finalize, (t['stats'] if training else None, t['gb'], t['rm'], t['rv'], t['nbt'], t['a'], t['s'], c['B'], c['C'], int(training),
                                         f32(c.get('momentum', 0.1)), f32(c['eps']))
    elif entry == 'reduce_finalize':
        fn, args = lib.v2w_bn_reduce_finalize, (t['part'], c['ntiles'], float(c['count']), t['gb'], t['rm'], t['rv'], t['nbt'], t['stats'], t['a'], t['s'],
                                                c['B'], c['C'], f32(c['momentum']), f32(c['eps']))
    elif entry == 'reduce_slices':
        fn, args = lib.v2w_bn_reduce_slices, (t['part'], c['ntiles'], c['C'], t['slices'], c['nslices'])
    elif entry == 'finalize_slices':
        fn, args = lib.v2w_bn_finalize_slices, (t['slices'], c['nslices'], float(c['count']), t['gb'], t['rm'], t['rv'], t['nbt'], t['a'], t['s'],
                                                c['B'], c['C'], f32(c['momentum']), f32(c['eps']))
    elif entry == 'bn_stats':
        fn, args = lib.v2w_bn_stats, (t['x'], t['stats'], t['partial'], c['B'], c['C'], c['L'])
    elif entry == 'affine_apply':
        fn, args = lib.v2w_affine_apply, (t['x'], t['a'], t['s'], t['out'], c['B'], c['C'], c['L'])
    elif entry in ('cond_gamma_beta', 'cond_sigma'):
        e = cond_struct(c, t, training)
        fn, args = getattr(lib, 'v2w_' + entry), (C.byref(e.c),)
    elif entry == 'cond_affine_eval':
        e = cond_struct(c, t, 0)
        fn, args = lib.v2w_cond_affine_eval, (C.byref(e),)
    else:
        raise KeyError(entry)
    if stream is None:
        return _hip.kernel_names(fn, *args)
    return fn(*args, stream), None


def dispatch(entry, c, group, training=1):
    """Host-only: (return code, kernels) of one call of the record.  A process without a GPU reports hipErrorNoDevice (100) from the launch
    status that ends every entry point, after all its launch sites were passed: it counts as OK here."""
    rc, names = call(entry, c, fake(c, group), training=training)
    return (OK if rc == 100 else rc), names


def entries(group, c):
    """(entry, training, expected return code, expected kernels) of every call the record's GPU test makes."""
    ok = c['rc'] == OK
    if group == 'one_level':
        return [('reduce_partials', 1, OK, ONE), ('finalize', 1, OK, FIN), ('reduce_finalize', 1, OK, FUSED)]
    if group == 'two_level':
        return [('reduce_slices', 1, c['rc'], SLICES if ok else []), ('finalize_slices', 1, c['rc'], FIN_SLICES if ok else [])]
    if group == 'fin_eval':
        return [('finalize', 0, OK, FIN)]
    if group == 'bn_stats':
        return [('bn_stats', 1, OK, c['kernels'])]
    if group == 'affine':
        return [('affine_apply', 1, c['rc'], c['kernels'])]
    sn = ['cond_sn_kernel'] if c['rc_sigma'] == OK else []
    return [('cond_gamma_beta', 1, c['rc'], c['kernels']), ('cond_gamma_beta', 0, c['rc'], c['kernels']),
            ('cond_sigma', 1, c['rc_sigma'], sn), ('cond_sigma', 0, c['rc_sigma'], sn),
            ('cond_affine_eval', 0, c['rc_eval'], ['cond_affine_eval_kernel'] if c['rc_eval'] == OK else [])]


ALL = [(g, c) for g, cases in TABLE.items() for c in cases]
assert len({(g, c['id']) for g, c in ALL}) == len(ALL)


# ---------------------------------------------------------------------------------------------------------------
# the records' data (numpy, a seed per record id): drawn once per record and shared by the CPU and GPU suites
RATIOS = (0.0, 1.0, 8.0, 32.0)              # per-channel mean / std of the 'cond' records


def _rng(c):
    return np.random.default_rng(sum(map(ord, c['id'])))


def _f32(rng, *shape, scale=1.0, shift=0.0):
    return (rng.standard_normal(shape) * scale + shift).astype(np.float32)


def _channels(rng, C, chan):
    if chan == 'cond':
        return np.array([RATIOS[c % 4] for c in range(C)]), np.ones(C)
    return 0.5 * rng.standard_normal(C), rng.uniform(0.5, 1.5, C)


def _bn_operands(rng, B, C):
    return dict(gb=_f32(rng, B, 2 * C), rm=_f32(rng, C, scale=0.3), rv=rng.uniform(0.5, 1.5, C).astype(np.float32))


@functools.lru_cache(maxsize=4)
def _draw_rows(id, C, B, ntiles, chan):
    rng = _rng(dict(id=id))
    d = _bn_operands(rng, B, C)
    if chan == 'count1':
        x = _f32(rng, 1, C, scale=2.0)
        d['part'] = np.stack([x, (x.astype(np.float64) ** 2).astype(np.float32)], -1)
        d['mean'], d['var'] = x[0].astype(np.float64), np.zeros(C)
        return d
    mu, sd = _channels(rng, C, chan)
    part = np.empty((ntiles, C, 2), dtype=np.float32)
    s1, s2 = np.zeros(C), np.zeros(C)
    for t0 in range(0, ntiles, 256):                 # x in fp64, a tile of 224 positions per row
        x = rng.standard_normal((min(256, ntiles - t0), C, TILE)) * sd[None, :, None] + mu[None, :, None]
        if chan == 'cond' and C > 5:
            x[:, 4], x[:, 5] = 3.1, 0.0
        a, q = x.sum(-1), (x * x).sum(-1)
        part[t0:t0 + len(x), :, 0], part[t0:t0 + len(x), :, 1] = a, q
        s1 += a.sum(0)
        s2 += q.sum(0)
    n = ntiles * TILE
    d['part'], d['mean'] = part, s1 / n
    d['var'] = s2 / n - (s1 / n) ** 2                # of the signal itself (one pass in fp64: good to kappa * 2^-53)
    return d


def draw_rows(c):
    """part (ntiles, C, 2) float32 = (float(sum x), float(sum x^2)) per tile of a known fp64 signal, gb (B, 2C), the old running statistics,
    and the signal's own mean and variance.  The arrays are shared: leave them unchanged."""
    return _draw_rows(c['id'], c['C'], c['B'], c['ntiles'], c['chan'])


def draw_stats(c):
    rng = _rng(c)
    mu, sd = _channels(rng, c['C'], c['chan'])
    x = (rng.standard_normal((c['B'], c['C'], c['L'])) * sd[None, :, None] + mu[None, :, None]).astype(np.float32)
    return dict(x=x, **_bn_operands(rng, c['B'], c['C']))


def draw_eval(c):
    rng = _rng(c)
    return _bn_operands(rng, c['B'], c['C'])


def draw_affine(c):
    rng = _rng(c)
    return dict(x=_f32(rng, c['B'], c['C'], c['L']), a=_f32(rng, c['B'], c['C'], shift=1.0), s=_f32(rng, c['B'], c['C']))


def draw_cond(c):
    """W = 1 + 0.02 randn as the earlier test draws it: sigma is about sqrt(128 R), far from 0, and the quotient bounds stay tight."""
    rng = _rng(c)
    B, D = c['B'], c['spk_dim'] + c['noise_dim']
    d = dict(spk=_f32(rng, B, c['spk_dim']), noise=_f32(rng, B, c['noise_dim']) if c['noise_dim'] else None, stages=[])
    for Cs in c['Cs'][:MAX_STAGES]:
        R = 2 * Cs
        u, v = rng.standard_normal(R), rng.standard_normal(128)
        d['stages'].append(dict(fc_w=_f32(rng, 128, D, scale=D ** -0.5), fc_b=_f32(rng, 128, scale=0.1), sn_w=_f32(rng, R, 128, scale=0.02, shift=1.0),
                                sn_b=_f32(rng, R, scale=0.1), sn_u=(u / np.linalg.norm(u)).astype(np.float32), sn_v=(v / np.linalg.norm(v)).astype(np.float32),
                                rm=_f32(rng, Cs, scale=0.3), rv=rng.uniform(0.3, 2.0, Cs).astype(np.float32)))
    return d
