"""mel_spectrogram at any STFT frame geometry (win_size <= n_fft, 1 <= hop_size <= n_fft) on the device: the v2w_mel_*_geo entry points of
csrc/v2w_mel.hip one by one, then mel.py end to end against oracle/mel_oracle.py in fp64.  The geometries, lengths and signals are
tests/stft_ref.py's (tests/test_stft_geometry_cpu.py holds their host-only half).

  1. the phase kernels (forward, per-item lengths, backward): bit for bit against tests/stft_ref.py's gather map and its transpose, on guarded
     buffers, NaN wherever a call has no business reading; the padding channels and the columns past the signal are +0.0.
  2. the finish calls at nb = 1025 (8 frames per workgroup) against tests/mel_ref.py's fp64 statements under that module's own bounds; at an
     nb the first kernels serve, the _geo calls give the bits of v2w_mel_finish, _len and _bwd.
  3. end to end, forward and d y, against the oracle in fp64 and torch autograd through it.  The bar is measured, not fixed: the oracle's own
     float32-against-float64 gap on the same input (max over the entries, CPU), times 4 - the MFMA tile and torch.stft's FFT add in different
     orders.  Entries whose fp64 filterbank sum lies within mel_ref.GAP of the clamp are left out (at most 1 %; the seeded noise has none:
     test_stft_geometry_cpu.py::test_oracle_alone_excludes_no_entry) and get no upstream gradient.
  4. lengths=: out[b, :, :F_b] is the item's own B = 1 call bit for bit, out[b, :, F_b:] is +0.0, NaN in y[b, Lb:] reaches nothing; mel_l1 of
     such a batch is F.l1_loss of the trimmed pairs (fp64, 1e-6 relative).
128 / 32 / 128 is a geometry the first entry points serve: mel.py's result there is theirs, called one by one through ctypes, bit for bit.
Measured on an MI355X (error against fp64 / the oracle's own float32 gap; bar 4): the six 128-point geometries at their listed lengths
out 1.2 - 3.1, d y 0.7 - 2.7; 512 / 50 / 240 out 1.45, d y 1.99; 1024 / 120 / 600 out 2.47, d y 2.40 (8.11e-6 against a gap of 3.39e-6);
2048 / 240 / 1200 out 2.13, d y 1.63.  With the input-gradient conv in one launch (one chain of 5 x 1088 / 2112 fp32 terms) the last two
d y figures were 7.70 and 4.80 and missed the bar; mel.py adds the rows 128 at a time since (mel._dft_conv_bwd).
Every test here fails without the feature (NotImplementedError from mel.py, no v2w_mel_*_geo symbol in the library).  DESIGN.md 3d''' has the
measured gaps and ratios."""
import numpy as np
import pytest
import torch

from tests import mel_ref as R
from tests import stft_ref as S
from tests.test_cbn_kernels_gpu import _addr, _inp, _kept, _out, _state, _twice
from tests.test_disc_kernels_gpu import _report, env  # noqa: F401  (env: the module-scoped fixture)
from tests.test_mel_kernels_gpu import _bits_equal
from tests.test_tile_kernels_gpu import _sync_or_stop

pytestmark = pytest.mark.gpu
OK = 0


def _geo_ints(g, B, L, FP):
    return B, L, g['n_fft'], g['win'], g['hop'], g['cp'], g['pad'], g['left'], g['k'], FP


def _lens3(L, pad):
    """One item at full L, one at pad + 1 (no frame or the fewest), one in between."""
    return [L, pad + 1, (L + pad + 1) // 2]


def _runs(geo):
    """(g, the listed lengths that give a frame)."""
    from wavthruvec_pytorch_amd import mel
    g = mel.stft_geometry(*geo)
    return g, [L for L in S.lengths_of(geo[0], geo[1], g['pad']) if S.frames(L, g) and L > 1]


# ---------------------------------------------------------------------------------------------------------------
# 1. the phase kernels
@pytest.mark.parametrize('geo', S.SMALL, ids=S.gid)
def test_phase_kernels(env, geo):
    dev, _hip, lib, st = env
    g, lengths = _runs(geo)
    hop, cp = g['hop'], g['cp']
    for j, L in enumerate(lengths):
        B, FP = 2, S.columns(L, g) + 4 * (j % 2)                 # (every other length: a zero tail of four columns)
        rng = np.random.default_rng(L)
        y = rng.standard_normal((B, L)).astype(np.float32)
        src, _ = S.gather_map(L, g, FP)
        dxp = rng.standard_normal((B, cp, FP)).astype(np.float32)
        dxp[:, src < 0] = np.nan                                # what the forward never reads must not reach dy
        A = dict(y=_inp(dev, y), dxp=_inp(dev, dxp), xp=_out(dev, B, cp, FP), dy=_out(dev, B, L))
        t, name = _addr(A), 'phases_geo %s L=%d' % (S.gid(geo), L)
        ints = _geo_ints(g, B, L, FP)
        assert _twice(A, name, lambda: (lib.v2w_mel_phases_geo(t['y'], t['xp'], *ints, st),
                                        lib.v2w_mel_phases_geo_bwd(t['dxp'], t['dy'], *ints, st))) == (OK, OK)
        _kept(A, {'xp', 'dy'}, name)
        xp = A['xp'].get()
        assert _bits_equal(xp, S.phases(y, g, FP)), name + ': xp'
        assert _bits_equal(xp[:, hop:], np.zeros((B, cp - hop, FP))), name + ': padding channels'
        assert _bits_equal(A['dy'].get(), S.phases_bwd(dxp, L, g)), name + ': dy'
    # per-item lengths at the longest length: NaN at and past every item's own end
    L = lengths[-1]
    lens = _lens3(L, g['pad']) + [1]
    B, FP = len(lens), S.columns(L, g)
    y = np.random.default_rng(L + 1).standard_normal((B, L)).astype(np.float32)
    for b, n in enumerate(lens):
        y[b, n:] = np.nan
    A = dict(y=_inp(dev, y), xp=_out(dev, B, cp, FP))
    ld = torch.tensor(lens, dtype=torch.int32, device=dev)
    t, name = _addr(A), 'phases_geo_len %s' % S.gid(geo)
    assert _twice(A, name, lambda: lib.v2w_mel_phases_geo_len(t['y'], t['xp'], *_geo_ints(g, B, L, FP), ld.data_ptr(), 1, st)) == OK
    _kept(A, {'xp'}, name)
    assert ld.cpu().tolist() == lens
    assert _bits_equal(A['xp'].get(), S.phases_len(y, g, FP, lens)), name


def test_first_phase_entry_points_are_the_geo_calls_at_their_geometry(env):
    """128 / 32 / 128 (pad 48, CP 32, k 4): the four first phase entry points hand their hop, pad, FP to the kernels of the _geo calls as
    left = 0, CP = hop, k = n_fft / hop, n_fft = 2 pad + hop.  Each pair bit for bit on guarded buffers; the lengths are full, pad + 1 and
    between, NaN at and past every item's own end and, in dxp, wherever the forward reads nothing."""
    dev, _hip, lib, st = env
    from wavthruvec_pytorch_amd import mel
    g = mel.stft_geometry(128, 32, 128)
    assert (g['pad'], g['cp'], g['k'], g['left']) == (48, 32, 4, 0)
    B, L, lens = 3, 200, [200, 49, 124]
    FP = S.columns(L, g)
    rng = np.random.default_rng(128)
    y = rng.standard_normal((B, L)).astype(np.float32)
    y_len = y.copy()
    for b, n in enumerate(lens):
        y_len[b, n:] = np.nan
    dxp = rng.standard_normal((B, 32, FP)).astype(np.float32)
    dxp[:, S.gather_map(L, g, FP)[0] < 0] = np.nan
    ld = torch.tensor(lens, dtype=torch.int32, device=dev)
    first, geo, tail = (B, L, 32, 48, FP), _geo_ints(g, B, L, FP), (ld.data_ptr(), 1)

    def pair(what, src, out_shape, f_first, f_geo, *more):
        A = dict(src=_inp(dev, src), a=_out(dev, *out_shape), b=_out(dev, *out_shape))
        t = _addr(A)
        assert _twice(A, what, lambda: (f_first(t['src'], t['a'], *first, *more, st), f_geo(t['src'], t['b'], *geo, *more, st))) == (OK, OK)
        _kept(A, {'a', 'b'}, what)
        assert _bits_equal(A['a'].get(), A['b'].get()), what
        return A['a'].get()

    xp = pair('phases', y, (B, 32, FP), lib.v2w_mel_phases, lib.v2w_mel_phases_geo)
    assert _bits_equal(xp, S.phases(y, g, FP))
    xp = pair('phases_len', y_len, (B, 32, FP), lib.v2w_mel_phases_len, lib.v2w_mel_phases_geo_len, *tail)
    assert _bits_equal(xp, S.phases_len(y_len, g, FP, lens))
    dy = pair('phases_bwd', dxp, (B, L), lib.v2w_mel_phases_bwd, lib.v2w_mel_phases_geo_bwd)
    assert _bits_equal(dy, S.phases_bwd(dxp, L, g))
    dy = pair('phases_len_bwd', dxp, (B, L), lib.v2w_mel_phases_len_bwd, lib.v2w_mel_phases_geo_len_bwd, *tail)
    assert np.isfinite(dy).all() and _bits_equal(dy[0], S.phases_bwd(dxp, L, g)[0]) and not dy[1, 49:].any() and not dy[2, 124:].any()
    assert ld.cpu().tolist() == lens


# ---------------------------------------------------------------------------------------------------------------
# 2. the finish calls
def _finish_data(seed, B, nb, n_mels, F, FP, Cs):
    """A loud spectrum (|re|, |im| ~ 3) under a non-negative basis of row sum ~ 0.4: every acc far above the clamp.  NaN in the pad rows and
    in the columns >= F."""
    rng = np.random.default_rng(seed)
    basis = (rng.uniform(0.05, 1.0, (n_mels, nb)) * (rng.uniform(0, 1, (n_mels, nb)) < 0.7) / nb).astype(np.float32)
    spec = np.full((B, Cs, FP), np.nan, dtype=np.float32)
    spec[:, :2 * nb, :F] = (3.0 * rng.standard_normal((B, 2 * nb, F))).astype(np.float32)
    return spec, basis, rng.standard_normal((B, n_mels, F)).astype(np.float32)


def _finish_calls(env, spec, basis, gout, F, nb, lens, hop, n_fft, family):
    """The three finish calls of one family ('' or '_geo') -> (out, out_len, dspec, F_b); lens in samples, spec for the _len call carries NaN in the
    frames at and past each item's own."""
    dev, _hip, lib, st = env
    B, Cs, FP = spec.shape
    n_mels = basis.shape[0]
    fn = lambda tail: getattr(lib, 'v2w_mel_finish' + family + tail)  # noqa: E731
    shape = (B, Cs, FP, F, nb, n_mels)
    A = dict(spec=_inp(dev, spec), basis=_inp(dev, basis), out=_out(dev, B, n_mels, F))
    t, name = _addr(A), 'finish%s nb=%d' % (family, nb)
    assert _twice(A, name, lambda: fn('')(t['spec'], t['basis'], t['out'], *shape, st)) == OK
    _kept(A, {'out'}, name)
    out = A['out'].get().copy()
    pad = (n_fft - hop) // 2
    Fb = [min(S.frames(n, dict(pad=pad, n_fft=n_fft, hop=hop)), F) for n in lens]
    spec_len = spec.copy()
    for b, f in enumerate(Fb):
        spec_len[b, :, f:] = np.nan
    ld = torch.tensor(lens, dtype=torch.int32, device=dev)
    A = dict(spec=_inp(dev, spec_len), basis=_inp(dev, basis), out=_out(dev, B, n_mels, F))
    t = _addr(A)
    assert _twice(A, name + ' len', lambda: fn('_len')(t['spec'], t['basis'], t['out'], *shape, ld.data_ptr(), 1, hop, n_fft, st)) == OK
    _kept(A, {'out'}, name + ' len')
    out_len = A['out'].get().copy()
    A = dict(spec=_inp(dev, spec), basis=_inp(dev, basis), basisT=_inp(dev, np.ascontiguousarray(basis.T)), gout=_inp(dev, gout),
             dspec=_state(dev, np.full(spec.shape, 555.0, dtype=np.float32)))
    t = _addr(A)
    assert _twice(A, name + ' bwd', lambda: fn('_bwd')(t['spec'], t['basis'], t['basisT'], t['gout'], t['dspec'], *shape, st)) == OK
    _kept(A, {'dspec'}, name + ' bwd')
    own = np.zeros(spec.shape, dtype=bool)
    own[:, :2 * nb, :F] = True
    assert A['dspec'].unchanged(keep=~own), name + ': pad rows or columns >= F were written'
    return out, out_len, A['dspec'].get()[:, :2 * nb, :F].copy(), Fb


def test_finish_at_nb_1025(env):
    """n_fft 2048: 1025 bins x 16 frames pass 64 KiB of LDS, the 8-frame kernels take them.  F = 19: two whole blocks and a ragged third; the
    items' own frames end inside a block, on a block's edge, at 0 and at F.  hop 25 / n_fft 128: n_fft - hop odd, n_fft % hop != 0."""
    B, nb, n_mels, F, FP, Cs = 4, 1025, 5, 19, 20, 2 * 1025 + 6
    spec, basis, gout = _finish_data(1025, B, nb, n_mels, F, FP, Cs)
    gap, frac = R.clamp_gap(spec, basis, F, nb)
    assert gap >= R.GAP and frac < 1
    hop, n_fft, pad = 25, 128, 51
    lens = [n_fft - 2 * pad + hop * (fb - 1) for fb in (5, 8, 19)] + [pad]
    out, out_len, dspec, Fb = _finish_calls(env, spec, basis, gout, F, nb, lens, hop, n_fft, '_geo')
    assert Fb == [5, 8, 19, 0]
    keep = np.arange(F)[None, :] < np.asarray(Fb)[:, None]
    value, bound = R._finish(R._parts(spec, basis, F, nb, keep))
    ratios = dict(out=R.worst_ratio(out, *R.finish(spec, basis, F, nb)),
                  out_len=R.worst_ratio(out_len, np.where(keep[:, None, :], value, 0.0), np.where(keep[:, None, :], bound, 0.0)),
                  dspec=R.worst_ratio(dspec, *R.finish_bwd(spec, basis, gout, F, nb)))
    for b, f in enumerate(Fb):
        assert _bits_equal(out_len[b, :, :f], out[b, :, :f]) and _bits_equal(out_len[b, :, f:], np.zeros((n_mels, F - f))), b
    _report('finish_geo nb=1025', **ratios)


def test_finish_geo_gives_the_first_kernels_bits_where_they_serve(env):
    """nb = 40, 80 mels, F = 33: both families run the 16-frame kernels (hop 4, n_fft 8 is a geometry v2w_mel_finish_len takes)."""
    B, nb, n_mels, F, FP, Cs = 3, 40, 80, 33, 36, 85
    spec, basis, gout = _finish_data(40, B, nb, n_mels, F, FP, Cs)
    lens = [4 * 7, 4 * 33, 3]
    a = _finish_calls(env, spec, basis, gout, F, nb, lens, 4, 8, '')
    b = _finish_calls(env, spec, basis, gout, F, nb, lens, 4, 8, '_geo')
    assert a[3] == b[3] == [7, 33, 0]
    for x, y, what in zip(a[:3], b[:3], ('out', 'out_len', 'dspec')):
        assert _bits_equal(x, y), what


# ---------------------------------------------------------------------------------------------------------------
# 3. end to end against the oracle
def _end_to_end(dev, geo, mels, B, L, seed):
    """-> (out, dy, figures): mel.py forward and backward at one geometry and length, held to 4 x the oracle's own float32 gap."""
    from wavthruvec_pytorch_amd import mel
    cfg = S.cfg_of(geo, mels)
    y0 = S.signal(B, L, seed)
    near = S.near_clamp(y0, cfg)
    assert near.mean() <= 0.01
    G = np.random.default_rng(seed + 1).standard_normal(near.shape).astype(np.float32)
    G[near] = 0.0
    want, dwant, gap_out, gap_dy = S.oracle_gaps(y0, cfg, G)
    yd = torch.from_numpy(y0).to(dev).requires_grad_(True)
    out = mel.mel_spectrogram(yd, *cfg)
    assert tuple(out.shape) == want.shape == (B, mels, mel.mel_frames(L, geo[0], geo[1]))
    (out * torch.from_numpy(G).to(dev)).sum().backward()
    _sync_or_stop('mel_spectrogram %s L=%d' % (S.gid(geo), L))
    got, dy = out.detach().cpu().numpy(), yd.grad.cpu().numpy()
    assert np.isfinite(got).all() and np.isfinite(dy).all()
    e_out, e_dy = float(np.abs(got - want)[~near].max()), float(np.abs(dy - dwant).max())
    print('[stft geometry] %s L=%d F=%d: oracle f32 - f64 gap out %.3e dy %.3e; HIP - f64 out %.3e dy %.3e; ratios %.3f %.3f (bar 4); left out %d'
          % (S.gid(geo), L, want.shape[2], gap_out, gap_dy, e_out, e_dy, e_out / gap_out, e_dy / gap_dy, int(near.sum())))
    return got, dy, (e_out, 4 * gap_out, e_dy, 4 * gap_dy)


@pytest.mark.parametrize('geo', S.SMALL, ids=S.gid)
def test_end_to_end_at_the_listed_lengths(env, geo):
    dev = env[0]
    from wavthruvec_pytorch_amd import mel
    g, lengths = _runs(geo)
    figures = [_end_to_end(dev, geo, S.SMALL_MELS, 2, L, L)[2] for L in lengths]
    for L in S.lengths_of(geo[0], geo[1], g['pad']):
        if L not in lengths:                                     # pad + 1 samples that are no frame: the reference raises there too
            with pytest.raises(RuntimeError):
                mel.mel_spectrogram(torch.zeros(2, L, device=dev), *S.cfg_of(geo, S.SMALL_MELS))
    for L, (e_out, bar_out, e_dy, bar_dy) in zip(lengths, figures):
        assert e_out <= bar_out and e_dy <= bar_dy, (L, e_out, bar_out, e_dy, bar_dy)


@pytest.mark.parametrize('geo', S.LARGE, ids=S.gid)
def test_end_to_end_at_a_multi_resolution_setting(env, geo):
    e_out, bar_out, e_dy, bar_dy = _end_to_end(env[0], geo, S.LARGE_MELS, S.LARGE_B, S.LARGE_L, geo[0])[2]
    assert e_out <= bar_out and e_dy <= bar_dy, (e_out, bar_out, e_dy, bar_dy)


def test_the_first_entry_points_geometry_keeps_their_bits(env):
    """128 / 32 / 128: mel.py's forward and backward are v2w_mel_phases -> conv -> v2w_mel_finish and v2w_mel_finish_bwd -> conv ->
    v2w_mel_phases_bwd, called here one by one."""
    dev, _hip, lib, st = env
    from wavthruvec_pytorch_amd import hipops, mel
    geo, B, L = S.SMALL[0], 2, 200
    cfg = S.cfg_of(geo, S.SMALL_MELS)
    y0 = S.signal(B, L, 7)
    G = torch.from_numpy(np.random.default_rng(8).standard_normal((B, S.SMALL_MELS, mel.mel_frames(L, 128, 32))).astype(np.float32)).to(dev)
    yd = torch.from_numpy(y0).to(dev).requires_grad_(True)
    out = mel.mel_spectrogram(yd, *cfg)
    (out * G).sum().backward()
    c = mel._constants(*cfg, dev)
    assert c['old'] and c['cp'] == 32 and c['k'] == 4
    F, pad, k, nb, cs = out.shape[2], 48, 4, 65, c['cs']
    FP = R.roundup4(F + k - 1)
    y = torch.from_numpy(y0).to(dev)
    xp, spec, ref = torch.empty((B, 32, FP), device=dev), torch.empty((B, cs, FP), device=dev), torch.empty((B, S.SMALL_MELS, F), device=dev)
    assert lib.v2w_mel_phases(y.data_ptr(), xp.data_ptr(), B, L, 32, pad, FP, st) == OK
    hipops.conv1d(xp, c['wf'], None, spec, k=k, dil=1, slope=1.0, pad_left=0, wp=c['wp'])
    assert lib.v2w_mel_finish(spec.data_ptr(), c['basis'].data_ptr(), ref.data_ptr(), B, cs, FP, F, nb, S.SMALL_MELS, st) == OK
    dspec, dxp, dy = torch.zeros_like(spec), torch.empty_like(xp), torch.empty((B, L), device=dev)
    assert lib.v2w_mel_finish_bwd(spec.data_ptr(), c['basis'].data_ptr(), c['basisT'].data_ptr(), G.data_ptr(), dspec.data_ptr(), B, cs, FP, F, nb,
                                  S.SMALL_MELS, st) == OK
    hipops.conv1d(dspec, c['wT'], None, dxp, k=k, dil=1, slope=1.0, pad_left=k - 1, wp=c['wTp'])
    assert lib.v2w_mel_phases_bwd(dxp.data_ptr(), dy.data_ptr(), B, L, 32, pad, FP, st) == OK
    _sync_or_stop('the first entry points')
    assert _bits_equal(out.detach().cpu().numpy(), ref.cpu().numpy()) and _bits_equal(yd.grad.cpu().numpy(), dy.cpu().numpy())


# ---------------------------------------------------------------------------------------------------------------
# 4. lengths=
@pytest.mark.parametrize('geo', S.SMALL + S.LARGE[2:], ids=S.gid)
def test_lengths(env, geo):
    dev = env[0]
    from wavthruvec_pytorch_amd import mel
    large = geo in S.LARGE
    mels = S.LARGE_MELS if large else S.SMALL_MELS
    cfg = S.cfg_of(geo, mels)
    g = mel.stft_geometry(*geo)
    L = 4096 if large else _runs(geo)[1][-1]
    lens = _lens3(L, g['pad'])
    y0 = S.signal(3, L, L + 2)
    for b, n in enumerate(lens):
        y0[b, n:] = np.nan
    out = mel.mel_spectrogram(torch.from_numpy(y0).to(dev), *cfg, lengths=lens)
    _sync_or_stop('lengths ' + S.gid(geo))
    F = mel.mel_frames(L, geo[0], geo[1])
    Fb = [mel.mel_frames(n, geo[0], geo[1]) for n in lens]
    assert tuple(out.shape) == (3, mels, F) and Fb[0] == F and Fb == [S.frames(n, g) for n in lens]
    got = out.cpu().numpy()
    for b, (n, f) in enumerate(zip(lens, Fb)):
        assert _bits_equal(got[b, :, f:], np.zeros((mels, F - f))), (b, 'frames past F_b are not +0.0')
        if f:
            own = mel.mel_spectrogram(torch.from_numpy(y0[b:b + 1, :n].copy()).to(dev), *cfg)
            assert _bits_equal(got[b, :, :f], own.cpu().numpy()[0]), (b, "the item's own call")
    # the masked L1 against F.l1_loss of the trimmed pairs, fp64
    tgt = np.random.default_rng(L + 3).standard_normal(got.shape).astype(np.float32)
    for b, f in enumerate(Fb):
        tgt[b, :, f:] = np.nan
    total, per = mel.mel_l1(out, torch.from_numpy(tgt).to(dev), lens, n_fft=geo[0], hop_size=geo[1])
    _sync_or_stop('mel_l1 ' + S.gid(geo))
    want = [torch.nn.functional.l1_loss(torch.from_numpy(got[b, :, :f]).double(), torch.from_numpy(tgt[b, :, :f]).double()).item() if f else 0.0
            for b, f in enumerate(Fb)]
    whole = sum(w * f for w, f in zip(want, Fb)) / sum(Fb)
    for b in range(3):
        assert abs(per[b].item() - want[b]) <= 1e-6 * abs(want[b]), (b, per[b].item(), want[b])
    assert abs(total.item() - whole) <= 1e-6 * abs(whole)
