"""The cases of tests/test_mel_kernels_gpu.py: one record per geometry of the mel-spectrogram ends (csrc/v2w_mel.hip: the six kernels its seven first
entry points launch, each an instantiation of a device template that the v2w_mel_*_geo calls run too), with the kernel each entry must launch, its return code and its seeded data.

tests/test_mel_ref_cpu.py drives every record through the name sink (host-only, made-up addresses) and asserts kernels and return codes; the
GPU tests run the same records on guarded buffers.  `call` builds the arguments of both runs from one table of addresses.  The shapes are
generic and small: the kernels take hop, pad, FP, Cs, nb, n_mels as arguments and mel.py reaches one value of each.

  phase records   one geometry (B, L, hop, pad, FP) -> v2w_mel_phases and v2w_mel_phases_bwd.  FP_min = ceil((L + 2 pad) / hop) columns hold
                  the whole padded signal; FP_min + 3 adds a zero tail (forward) that the backward must not read.
  len records     v2w_mel_phases_len: (2 pad) % hop == 0, lengths that give every F_b class, NaN in y[b, Lb:].
  finish records  (B, nb, n_mels, F, FP, Cs) and a data class -> v2w_mel_finish, v2w_mel_finish_len (the record's own lengths, hop 4,
                  n_fft 8) and v2w_mel_finish_bwd.
The chain lengths n of the bounds are the shapes themselves (nb fmas per acc, n_mels per dm): tests/mel_ref.py reads them off the operands."""
import functools
import os

import numpy as np

from wavthruvec_pytorch_amd import _hip

from tests import mel_ref as R
from tests.disc_cases import OK, _case, ids  # noqa: F401  (ids: re-exported for the parametrisations)
from tests.disc_ref import ceil_div

E_ARG, E_SHAPE = -1, -2
KERNELS = ['mel_phase_kernel', 'mel_phase_len_kernel', 'mel_finish_kernel', 'mel_finish_len_kernel', 'mel_finish_bwd_kernel', 'mel_phase_bwd_kernel']
LOOP = 1024 * 256                              # the grids end at 1024 blocks of 256: past this many elements a thread takes a second trip
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'mel_filterbank.npz')


# ---------------------------------------------------------------------------------------------------------------
# v2w_mel_phases / v2w_mel_phases_bwd
def phase(id, *, B, L, hop, pad, FP, rc=OK, null=(), host_only=False):
    """null: operands passed as NULL.  host_only: a refusal whose shape no buffer could back; never run on a device."""
    return _case(id, ['mel_phase_kernel'] if rc == OK else [], rc, kernels_bwd=['mel_phase_bwd_kernel'] if rc == OK else [],
                 B=B, L=L, hop=hop, pad=pad, FP=FP, null=tuple(null), host_only=host_only)


def fp_min(L, hop, pad):
    return ceil_div(L + 2 * pad, hop)


PHASES = []
for _hop in (1, 3, 32):
    for _pad in sorted({0, 1, 5, _hop, 2 * _hop}):
        for _L in sorted({2, _pad + 1, _pad + 2, 2 * _pad, 2 * _pad + 1, 2 * _pad + 2, 100}):
            if _L <= 1 or _pad >= _L:
                continue
            _j = len(PHASES)                 # FP at its minimum and three columns past it, B = 1 and 3: alternating, out of step
            PHASES.append(phase('hop%d_pad%d_L%d' % (_hop, _pad, _L), B=(1, 3, 3)[_j % 3], L=_L, hop=_hop, pad=_pad,
                                FP=fp_min(_L, _hop, _pad) + 3 * (_j % 2)))
# fewer columns than the padded signal has: the forward stops early, the backward treats the rest as zero
PHASES.append(phase('hop3_pad5_L100_FP20', B=3, L=100, hop=3, pad=5, FP=20))
# the grid-stride loops: hop * FP = 264 192 > 262 144 (forward; L = 262 000 stays below), then L = 262 200 (backward; hop * FP = 262 304)
PHASES_LOOP = [phase('loop_hop512_FP516', B=1, L=262000, hop=512, pad=768, FP=516),
               phase('loop_L262200', B=1, L=262200, hop=32, pad=48, FP=fp_min(262200, 32, 48))]
assert PHASES_LOOP[0]['hop'] * PHASES_LOOP[0]['FP'] > LOOP > PHASES_LOOP[0]['L'] and PHASES_LOOP[1]['L'] > LOOP

_P = dict(B=2, L=100, hop=3, pad=5, FP=40)
PHASES_REFUSED = [
    phase('null_in_refused', **_P, rc=E_ARG, null=('in',)), phase('null_out_refused', **_P, rc=E_ARG, null=('out',)),
    phase('B0_refused', **dict(_P, B=0), rc=E_ARG), phase('L1_refused', **dict(_P, L=1, pad=0), rc=E_ARG),
    phase('L0_refused', **dict(_P, L=0, pad=0), rc=E_ARG), phase('pad_eq_L_refused', **dict(_P, L=5), rc=E_ARG),
    phase('pad_gt_L_refused', **dict(_P, L=4), rc=E_ARG), phase('pad_negative_refused', **dict(_P, pad=-1), rc=E_ARG),
    phase('hop0_refused', **dict(_P, hop=0), rc=E_ARG), phase('hop_negative_refused', **dict(_P, hop=-3), rc=E_ARG),
    phase('FP0_refused', **dict(_P, FP=0), rc=E_ARG), phase('FP_negative_refused', **dict(_P, FP=-4), rc=E_ARG),
    # the kernels' int arithmetic: hop * FP = 2^31, L + 2 pad = 2^31 (the largest each call takes is one below)
    phase('hopFP_2p31_refused', B=1, L=100, hop=1 << 16, pad=5, FP=1 << 15, rc=E_SHAPE, host_only=True),
    phase('L2pad_2p31_refused', B=1, L=(1 << 30) + 2, pad=(1 << 29) - 1, hop=32, FP=64, rc=E_SHAPE, host_only=True),
]
PHASES_EDGE = [phase('hopFP_2p31_minus_1', B=1, L=100, hop=(1 << 31) - 1, pad=5, FP=1, host_only=True),
               phase('L2pad_2p31_minus_1', B=1, L=(1 << 30) + 1, pad=(1 << 29) - 1, hop=32, FP=64, host_only=True)]


# ---------------------------------------------------------------------------------------------------------------
# v2w_mel_phases_len.  F_b = frames(Lb): 0 for Lb <= pad and for Lb < hop (Lb + 2 pad < n_fft; needs pad < hop), 1 for hop <= Lb < 2 hop
def plen(id, *, L, hop, pad, lens, len_mul=1, extra=0, rc=OK, null=(), host_only=False, FP=None):
    k = (2 * pad + hop) // max(hop, 1)
    F = R.frames(L, hop, pad) if hop > 0 else 0
    return _case(id, ['mel_phase_len_kernel'] if rc == OK else [], rc, B=len(lens), L=L, hop=hop, pad=pad, FP=FP or R.roundup4(F + k - 1) + extra,
                 lens=tuple(lens), len_mul=len_mul, null=tuple(null), host_only=host_only)


PHASES_LEN = [
    # n_fft 128 (k = 4): Lb = 40, 48 <= pad; 49, 63 one frame; the interior; L itself; past L (clamped); negative
    plen('n128_hop32', L=400, hop=32, pad=48, lens=(40, 48, 49, 63, 64, 200, 399, 400, 401, 100000, -5, 0)),
    plen('n128_hop32_wide', L=400, hop=32, pad=48, lens=(49, 400, 130), extra=4),
    # n_fft 64 (k = 2), pad < hop: 16 <= pad; 17 .. 31 have the padding but no frame
    plen('n64_hop32', L=300, hop=32, pad=16, lens=(16, 17, 31, 32, 33, 64, 300)),
    # len_mul: 7 * 13 = 91, 23 * 13 = 299 <= L, 24 * 13 > L; the product past 2^31 (clamped in 64 bits)
    plen('n12_hop4_mul13', L=301, hop=4, pad=4, lens=(7, 23, 24, 1, 0, 400000000), len_mul=13),
    plen('n2_hop2_pad0', L=33, hop=2, pad=0, lens=(1, 2, 3, 33)),
    plen('one_item_hop1', L=50, hop=1, pad=3, lens=(20,)),
]
_PL = dict(L=400, hop=32, pad=48, lens=(49, 400))
PHASES_LEN_REFUSED = [
    plen('pad_not_half_hops_refused', **dict(_PL, pad=40), rc=E_ARG), plen('null_len_refused', **_PL, rc=E_ARG, null=('len',)),
    plen('len_mul0_refused', **_PL, len_mul=0, rc=E_ARG), plen('null_in_refused', **_PL, rc=E_ARG, null=('in',)),
    plen('hop0_refused', **dict(_PL, hop=0, pad=0), rc=E_ARG, FP=16), plen('pad_eq_L_refused', **dict(_PL, L=48), rc=E_ARG, FP=16),
    plen('hopFP_2p31_refused', L=100, hop=1 << 16, pad=0, lens=(50,), rc=E_SHAPE, host_only=True, FP=1 << 15),
    plen('L2pad_2p31_refused', L=(1 << 30) + 2, hop=2, pad=(1 << 29) - 1, lens=(50,), rc=E_SHAPE, host_only=True, FP=64),
]


# ---------------------------------------------------------------------------------------------------------------
# v2w_mel_finish / _len / _bwd.  One workgroup = 16 frames; its 256 threads take nb * 16 magnitudes and n_mels * 16 outputs in trips of 256:
# nb, n_mels = 15, 16, 17 lie below, on and above one trip
FIN_HOP, FIN_NFFT = 4, 8                      # of the records' v2w_mel_finish_len calls: pad 2, F_b = Lb / 4 for Lb >= 4
DATA = ('loud', 'silence', 'mixed', 'tiny')


def fin(id, *, B, nb, n_mels, F, FP=None, Cs=None, data='loud', lens=None, len_mul=1, rc=OK, rc_bwd=None, rc_len=None, null=(), hop=FIN_HOP,
        n_fft=FIN_NFFT, host_only=False):
    """lens: the samples of each item for the _len call (default: F_b = F)."""
    lens = tuple(lens) if lens is not None else (F * FIN_HOP,) * B
    rc_bwd, rc_len = rc if rc_bwd is None else rc_bwd, rc if rc_len is None else rc_len
    return _case(id, ['mel_finish_kernel'] if rc == OK else [], rc, kernels_len=['mel_finish_len_kernel'] if rc_len == OK else [],
                 kernels_bwd=['mel_finish_bwd_kernel'] if rc_bwd == OK else [], rc_bwd=rc_bwd, rc_len=rc_len, B=B, nb=nb, n_mels=n_mels, F=F,
                 FP=F if FP is None else FP, Cs=2 * nb if Cs is None else Cs, data=data, lens=lens, len_mul=len_mul, null=tuple(null), hop=hop,
                 n_fft=n_fft, host_only=host_only)


SHAPES = ((1, 1), (15, 17), (16, 16), (17, 15), (40, 80), (1, 80), (40, 1))          # (nb, n_mels)
FRAMES = (1, 15, 16, 17, 33)


def _lens(F, B, j):
    """F_b of 0, mid-block, on a block edge, F and beyond F, three at a time (in samples: 4 per frame, 3 samples are no frame)."""
    pool = (3, 4 * 7, 4 * 16, 4 * F, 4 * F + 40, 0, 4 * 20, -9, 4 * F - 4)
    return tuple(pool[(j + i) % len(pool)] for i in range(B))


FINISH = []
for _d in DATA:
    for _nb, _nm in SHAPES:
        _j = len(FINISH)
        _F, _B = FRAMES[_j % 5], (1, 3)[_j % 2]
        FINISH.append(fin('%s_nb%d_m%d_F%d' % (_d, _nb, _nm, _F), B=_B, nb=_nb, n_mels=_nm, F=_F, FP=_F + (0, 3, 8)[_j % 3],
                          Cs=2 * _nb + (0, 5)[(_j // 2) % 2], data=_d, lens=_lens(_F, _B, _j)))
# every F on every data class at one middling shape, F_b in every position
FINISH += [fin('%s_nb17_m17_F%d_B3' % (_d, _F), B=3, nb=17, n_mels=17, F=_F, FP=_F + 1, Cs=37, data=_d, lens=_lens(_F, 3, _i + 2 * _k))
           for _k, _d in enumerate(DATA) for _i, _F in enumerate(FRAMES) if (_i + _k) % 2 == 0]
FINISH.append(fin('len_mul5_nb16_m15_F33', B=3, nb=16, n_mels=15, F=33, FP=36, Cs=40, data='mixed', lens=(13, 26, 6), len_mul=5))
# the committed reference filterbank (80 x 513): silent, quiet and loud frames side by side
FINISH_GOLDEN = [fin('golden_80x513_F17', B=1, nb=513, n_mels=80, F=17, FP=20, Cs=1088, data='golden', lens=(4 * 9,))]

_F0 = dict(B=2, nb=16, n_mels=15, F=17, FP=20, Cs=40)
FINISH_REFUSED = [
    fin('FP_lt_F_refused', **dict(_F0, FP=16), rc=E_ARG), fin('Cs_lt_2nb_refused', **dict(_F0, Cs=31), rc=E_ARG),
    fin('F0_refused', **dict(_F0, F=0), rc=E_ARG), fin('null_spec_refused', **_F0, rc=E_ARG, null=('spec',)),
    fin('null_basis_refused', **_F0, rc=E_ARG, null=('basis',)), fin('null_out_refused', **_F0, rc=E_ARG, null=('out',)),
    # 64 KiB of LDS: 16 floats per bin forward, per bin and per mel backward
    fin('nb1025_refused', B=1, nb=1025, n_mels=2, F=3, FP=4, rc=E_SHAPE, host_only=True),
    fin('nb1024', B=1, nb=1024, n_mels=2, F=3, FP=4, rc=OK, rc_bwd=E_SHAPE, host_only=True),
    fin('nb_plus_mels_1025_refused', B=1, nb=513, n_mels=512, F=3, FP=4, rc=OK, rc_bwd=E_SHAPE, host_only=True),
    fin('nb_plus_mels_1024', B=1, nb=512, n_mels=512, F=3, FP=4, host_only=True),
    fin('mels_2p27_refused', B=1, nb=4, n_mels=1 << 27, F=3, FP=4, rc=E_SHAPE, host_only=True),            # n_mels * 16 = 2^31
    # the _len arguments: the plain calls take the same record
    fin('null_len_refused', **_F0, rc_len=E_ARG, null=('len',)), fin('len_mul0_refused', **_F0, len_mul=0, rc_len=E_ARG),
    fin('len_hop0_refused', **_F0, hop=0, rc_len=E_ARG), fin('n_fft_lt_hop_refused', **_F0, hop=8, n_fft=4, rc_len=E_ARG),
    fin('n_fft_no_multiple_refused', **_F0, hop=4, n_fft=10, rc_len=E_ARG), fin('n_fft_minus_hop_odd_refused', **_F0, hop=1, n_fft=2, rc_len=E_ARG),
    fin('F_hop_2p31_refused', **dict(_F0, F=1 << 20, FP=1 << 20), hop=1 << 11, n_fft=1 << 12, rc_len=E_SHAPE, host_only=True),
]

TABLE = dict(phases=PHASES + PHASES_LOOP + PHASES_REFUSED + PHASES_EDGE, phases_len=PHASES_LEN + PHASES_LEN_REFUSED,
             finish=FINISH + FINISH_GOLDEN + FINISH_REFUSED)
ALL = [(g, c) for g, cases in TABLE.items() for c in cases]
assert len({(g, c['id']) for g, c in ALL}) == len(ALL)


def on_device(cases):
    return [c for c in cases if not c['host_only']]


# ---------------------------------------------------------------------------------------------------------------
# the calls, from a table of addresses (made up here, real ones in the GPU tests)
def fake(c):
    names = ('y', 'xp', 'dxp', 'dy', 'len', 'spec', 'basis', 'basisT', 'out', 'gout', 'dspec')
    return {name: 0x10000000 + 0x1000000 * i for i, name in enumerate(names)}


def call(entry, c, t, stream=None):
    """Run `entry` of record c on the addresses t: with a stream for real, without one through the name sink -> (rc, kernel names or None).
    The record's `null` names operands by role: 'in' / 'out' of the phase calls, 'len', 'spec', 'basis', 'out' of the finish calls."""
    lib = _hip.load()
    z = lambda role, name: None if role in c['null'] else t[name]  # noqa: E731
    if entry == 'phases':
        fn, args = lib.v2w_mel_phases, (z('in', 'y'), z('out', 'xp'), c['B'], c['L'], c['hop'], c['pad'], c['FP'])
    elif entry == 'phases_bwd':
        fn, args = lib.v2w_mel_phases_bwd, (z('in', 'dxp'), z('out', 'dy'), c['B'], c['L'], c['hop'], c['pad'], c['FP'])
    elif entry == 'phases_len':
        fn, args = lib.v2w_mel_phases_len, (z('in', 'y'), z('out', 'xp'), c['B'], c['L'], c['hop'], c['pad'], c['FP'], z('len', 'len'), c['len_mul'])
    elif entry == 'finish':
        fn, args = lib.v2w_mel_finish, (z('spec', 'spec'), z('basis', 'basis'), z('out', 'out'), c['B'], c['Cs'], c['FP'], c['F'], c['nb'], c['n_mels'])
    elif entry == 'finish_len':
        fn, args = lib.v2w_mel_finish_len, (z('spec', 'spec'), z('basis', 'basis'), z('out', 'out'), c['B'], c['Cs'], c['FP'], c['F'], c['nb'], c['n_mels'],
                                            z('len', 'len'), c['len_mul'], c['hop'], c['n_fft'])
    elif entry == 'finish_bwd':
        fn, args = lib.v2w_mel_finish_bwd, (z('spec', 'spec'), z('basis', 'basis'), t['basisT'], t['gout'], z('out', 'dspec'), c['B'], c['Cs'], c['FP'],
                                            c['F'], c['nb'], c['n_mels'])
    else:
        raise KeyError(entry)
    if stream is None:
        return _hip.kernel_names(fn, *args)
    return fn(*args, stream), None


def dispatch(entry, c):
    """Host-only: (return code, kernels) of one call of the record.  A process without a GPU reports hipErrorNoDevice (100) from the launch
    status that ends every entry point, after all its launch sites were passed: it counts as OK here."""
    rc, names = call(entry, c, fake(c))
    return (OK if rc == 100 else rc), names


def entries(group, c):
    """(entry, expected return code, expected kernels) of every call the record's GPU test makes."""
    if group == 'phases':
        return [('phases', c['rc'], c['kernels']), ('phases_bwd', c['rc'], c['kernels_bwd'])]
    if group == 'phases_len':
        return [('phases_len', c['rc'], c['kernels'])]
    return [('finish', c['rc'], c['kernels']), ('finish_len', c['rc_len'], c['kernels_len']), ('finish_bwd', c['rc_bwd'], c['kernels_bwd'])]


# ---------------------------------------------------------------------------------------------------------------
# the records' data (numpy, a seed per record id): drawn once per record and shared by the CPU and GPU suites
def _rng(c):
    return np.random.default_rng(sum(map(ord, c['id'])))


def _f32(rng, *shape, scale=1.0):
    return (rng.standard_normal(shape) * scale).astype(np.float32)


def draw_phase(c):
    """y (B, L); dxp (B, hop, FP) with NaN wherever the forward reads nothing (past the padded signal)."""
    rng = _rng(c)
    if c['rc'] != OK:
        return dict(y=_f32(rng, 64), dxp=_f32(rng, 64), n_out=64)
    B, L, hop, FP = c['B'], c['L'], c['hop'], c['FP']
    dxp = _f32(rng, B, hop, FP)
    src, _ = R.gather_map(L, hop, c['pad'], FP)
    dxp[:, src < 0] = np.nan
    return dict(y=_f32(rng, B, L), dxp=dxp)


def draw_phase_len(c):
    """y (B, L) with NaN at and past every item's own length."""
    rng = _rng(c)
    if c['rc'] != OK:
        return dict(y=_f32(rng, 64), lens=np.asarray(c['lens'], dtype=np.int32), n_out=64)
    y = _f32(rng, c['B'], c['L'])
    for b, n in enumerate(R.item_samples(c['lens'], c['len_mul'], c['L'])):
        y[b, n:] = np.nan
    return dict(y=y, lens=np.asarray(c['lens'], dtype=np.int32))


M0 = float(np.sqrt(R.C9))                    # the magnitude of a silent bin, 3.16e-5


def _positive_rows(rng, n_mels, nb):
    """A filterbank-like basis: non-negative, three weights in ten exactly zero, no empty row."""
    w = rng.uniform(0.05, 1.0, (n_mels, nb)) * (rng.uniform(0, 1, (n_mels, nb)) < 0.7)
    w[np.arange(n_mels), rng.integers(0, nb, n_mels)] += 0.5
    return w


def _acc(spec, basis, nb):
    s = spec.astype(np.float64)
    return np.einsum('mc,bcf->bmf', basis.astype(np.float64), np.sqrt(s[:, :nb] ** 2 + s[:, nb:2 * nb] ** 2 + R.C9))


def _keep_the_gap(spec, basis, nb):
    """Frames with an acc closer than 2^-9 (relative) to the clamp are scaled up by 5/4 until none is left (2^-9: twice what the suite asserts)."""
    for _ in range(64):
        bad = (np.abs(_acc(spec, basis, nb) / R.C5 - 1) < 2 * R.GAP).any(1)            # (B, F)
        if not bad.any():
            return spec
        spec = np.where(bad[:, None, :], spec * np.float32(1.25), spec).astype(np.float32)
    raise AssertionError('no gap')


TAUS = (1 - 2.0 ** -8, 1 + 2.0 ** -8, 1 - 2.0 ** -7, 1 + 2.0 ** -7, 0.7, 1.5)       # of frame f: acc = 1e-5f * tau[f % 6] * row[m % 3]
ROWS = (1.0, 1 + 2.0 ** -5, 1 - 2.0 ** -5)


def _mixed(rng, B, nb, n_mels, F):
    """Quiet frames whose acc straddles the clamp: proportional basis rows (row m = w * ROWS[m % 3], sum(w) m0 = 0.5e-5), each frame's spec
    scaled in fp64 (bisection: sqrt(. + 1e-9) is not linear) until w @ mag = 1e-5f * TAUS[f % 6]."""
    w = rng.uniform(0.2, 1.0, nb)
    w *= 0.5 * R.C5 / M0 / w.sum()
    shape = rng.standard_normal((B, 2 * nb, F)) + 0.1
    target = R.C5 * np.array([TAUS[f % 6] for f in range(F)])[None, :]
    lo, hi = np.zeros((B, F)), np.full((B, F), 1.0)
    for _ in range(80):
        mid = 0.5 * (lo + hi)
        s = shape * mid[:, None, :]
        a = np.einsum('c,bcf->bf', w, np.sqrt(s[:, :nb] ** 2 + s[:, nb:] ** 2 + R.C9))
        lo, hi = np.where(a < target, mid, lo), np.where(a < target, hi, mid)
    basis = w[None, :] * np.array([ROWS[m % 3] for m in range(n_mels)])[:, None]
    return (shape * hi[:, None, :]).astype(np.float32), basis.astype(np.float32)


@functools.lru_cache(maxsize=8)
def _draw_finish(id, B, nb, n_mels, F, FP, Cs, data):
    rng = _rng(dict(id=id))
    if data == 'golden':
        basis = np.load(GOLDEN)['basis.ref_16k_1024_80_0_8000']
        assert basis.shape == (n_mels, nb) and basis.dtype == np.float32
        spec = _f32(rng, B, 2 * nb, F, scale=4.0)
        spec[:, :, 0::3] = 0.0                                                  # silent frames: every acc below the clamp (test_mel_ref_cpu pins it)
        spec[:, :, 1::3] *= np.float32(2.0 ** -12)                               # quiet ones: about 1e-3
        spec = _keep_the_gap(spec, basis, nb)
    elif data == 'loud':
        basis = (_positive_rows(rng, n_mels, nb) / nb).astype(np.float32)
        spec = _keep_the_gap(_f32(rng, B, 2 * nb, F, scale=3.0), basis, nb)
    elif data == 'silence':                                                       # acc = rowsum * m0 = 1e-5f * (0.2 .. 1 - 2^-8): all clamped
        w = _positive_rows(rng, n_mels, nb)
        factor = np.where(np.arange(n_mels) % 2 == 0, 1 - 2.0 ** -8, rng.uniform(0.2, 0.9, n_mels))
        basis = (w * (factor * R.C5 / M0 / w.sum(1))[:, None]).astype(np.float32)
        spec = np.zeros((B, 2 * nb, F), dtype=np.float32)
    elif data == 'mixed':
        spec, basis = _mixed(rng, B, nb, n_mels, F)
    elif data == 'tiny':                                                          # |re|, |im| in [1e-6, 1e-4] (where the 1e-9 governs re / mag) next to loud bins
        basis = (_positive_rows(rng, n_mels, nb) * (4.0 / nb)).astype(np.float32)
        spec = (10.0 ** rng.uniform(-6, -4, (B, 2 * nb, F)) * rng.choice([-1.0, 1.0], (B, 2 * nb, F))).astype(np.float32)
        loud = np.arange(nb) % 2 == 1
        spec[:, np.concatenate([loud, loud])] = _f32(rng, B, 2 * int(loud.sum()), F)
        spec = _keep_the_gap(spec, basis, nb)
    else:
        raise KeyError(data)
    full = np.full((B, Cs, FP), np.nan, dtype=np.float32)                         # pad rows and the columns >= F hold NaN
    full[:, :2 * nb, :F] = spec
    return dict(spec=full, basis=basis, gout=_f32(rng, B, n_mels, F))


def draw_finish(c):
    """spec (B, Cs, FP) with NaN in the pad rows and in the columns >= F, basis (n_mels, nb) >= 0, gout (B, n_mels, F) signed.  A record all of
    whose calls are refused gets small stand-ins (nothing reads them).  The arrays are shared: leave them unchanged."""
    if c['rc'] != OK or c['host_only']:
        rng = _rng(c)
        return dict(spec=_f32(rng, 64), basis=_f32(rng, 64), gout=_f32(rng, 64), n_out=64)
    return _draw_finish(c['id'], c['B'], c['nb'], c['n_mels'], c['F'], c['FP'], c['Cs'], c['data'])


def spec_for_len(c, d):
    """The record's spec with NaN in every frame at and past the item's F_b: v2w_mel_finish_len must not let them through."""
    spec = d['spec'].copy()
    for b, Fb in enumerate(R.item_frames(c['lens'], c['len_mul'], c['hop'], c['n_fft'], c['F'])):
        spec[b, :, Fb:] = np.nan
    return spec
