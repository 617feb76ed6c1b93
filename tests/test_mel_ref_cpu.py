"""tests/mel_ref.py pinned against independent statements of the same operations (F.pad(mode='reflect') + unfold, torch.stft + the oracle's
mel_spectrogram, torch fp64 autograd, the trimmed B = 1 call), the clamp-gap condition of every record, the bounds checked on a float32
emulation of the kernels' own operation order (and found too tight for a basis weight changed by 2^-12), and the dispatch table of the mel
tests (tests/mel_cases.py through the name sink: which kernel every call of every record launches, and its return code).  No GPU needed."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import mel_oracle as M
from tests import mel_cases as K
from tests import mel_ref as R

SMALL = [c for c in K.PHASES if c['L'] <= 100]


def _padded(y, pad):
    y = torch.as_tensor(y)
    return F.pad(y[:, None], (pad, pad), mode='reflect')[:, 0] if pad else y


def _xp_torch(y, hop, pad, FP):
    """xp from torch: the reflect-padded rows cut or zero-extended to hop * FP samples, de-interleaved by phase."""
    yp = _padded(y, pad)
    n = hop * FP
    yp = yp[:, :n] if yp.shape[1] >= n else F.pad(yp, (0, n - yp.shape[1]))
    return yp.reshape(-1, FP, hop).transpose(1, 2)


@pytest.mark.parametrize('c', SMALL + K.PHASES_LOOP[1:], ids=K.ids(SMALL + K.PHASES_LOOP[1:]))
def test_phases_is_reflect_pad_and_unfold(c):
    d = K.draw_phase(c)
    hop, pad, FP, L = c['hop'], c['pad'], c['FP'], c['L']
    xp, bound = R.phases(d['y'], hop, pad, FP)
    assert bound is None and xp.dtype == np.float32
    assert torch.equal(torch.from_numpy(xp), _xp_torch(d['y'], hop, pad, FP))
    n_fft = 2 * pad + hop
    if n_fft % hop == 0 and L + 2 * pad >= n_fft and FP * hop >= L + 2 * pad:          # frame f = the columns f .. f + k - 1, phase-minor
        k = n_fft // hop
        fr = _padded(d['y'], pad).unfold(1, n_fft, hop)                                  # (B, frames, n_fft)
        t = torch.from_numpy(xp)
        mine = torch.stack([t[:, :, j:j + fr.shape[1]] for j in range(k)], 1)            # (B, k, hop, frames)
        assert torch.equal(mine.permute(0, 3, 1, 2).reshape(fr.shape), fr)
        assert fr.shape[1] == R.frames(L, hop, pad)


@pytest.mark.parametrize('c', SMALL, ids=K.ids(SMALL))
def test_phases_bwd_is_the_autograd_of_phases(c):
    d = K.draw_phase(c)
    hop, pad, FP, L = c['hop'], c['pad'], c['FP'], c['L']
    dy, bound = R.phases_bwd(d['dxp'], L, hop, pad)
    assert bound is None and dy.dtype == np.float32 and np.isfinite(dy).all()              # the NaN of the unread positions stay out
    g = torch.from_numpy(np.nan_to_num(d['dxp'], nan=0.0)).double()
    y = torch.from_numpy(d['y']).double().requires_grad_(True)
    (_xp_torch(y, hop, pad, FP) * g).sum().backward()
    src, _ = R.gather_map(L, hop, pad, FP)
    S = np.zeros((c['B'], L))
    np.add.at(S, (slice(None), src[src >= 0]), np.abs(g.numpy()[:, src >= 0]))
    assert (np.abs(dy - y.grad.numpy()) <= 2 * R.U * S).all()                              # three terms at most: two float32 additions


def test_phases_bwd_adds_in_the_documented_order():
    """L = 3, pad = 2, hop = 1: sample 1 is read at padded positions 3 (itself), 1 (left reflection) and 5 (right reflection).  With
    2^24, 1, -2^24 there the three orders of a float32 sum differ: (2^24 + 1) - 2^24 = 0."""
    dxp = np.zeros((1, 1, 7), dtype=np.float32)
    dxp[0, 0, [3, 1, 5]] = [2.0 ** 24, 1.0, -2.0 ** 24]
    assert R.phases_bwd(dxp, 3, 1, 2)[0][0, 1] == 0.0
    dxp[0, 0, [3, 1, 5]] = [2.0 ** 24, -2.0 ** 24, 1.0]
    assert R.phases_bwd(dxp, 3, 1, 2)[0][0, 1] == 1.0


@pytest.mark.parametrize('c', K.PHASES_LEN, ids=K.ids(K.PHASES_LEN))
def test_phases_len_is_the_trimmed_single_call(c):
    d = K.draw_phase_len(c)
    hop, pad, FP, L = c['hop'], c['pad'], c['FP'], c['L']
    xp, _ = R.phases_len(d['y'], hop, pad, FP, c['lens'], c['len_mul'])
    assert np.isfinite(xp).all()
    k, seen = (2 * pad + hop) // hop, set()
    for b, Lb in enumerate(R.item_samples(c['lens'], c['len_mul'], L)):
        Fb = R.frames(int(Lb), hop, pad)
        seen.add(0 if Fb == 0 else 1 if Fb == 1 else 3 if Lb == L else 2)
        if Fb == 0:
            assert not xp[b].any()
            continue
        FPb = R.roundup4(Fb + k - 1)
        own = _xp_torch(d['y'][b:b + 1, :Lb], hop, pad, FPb)[0].numpy()
        assert np.array_equal(xp[b, :, :FPb], own[:, :FP]) and not xp[b, :, FPb:].any()
        fr = _padded(d['y'][b:b + 1, :Lb], pad).unfold(1, 2 * pad + hop, hop)
        assert fr.shape[1] == Fb <= R.frames(L, hop, pad)
    if c['id'].startswith('n128_hop32') or c['id'] == 'n64_hop32':
        assert seen >= {1, 2, 3}
    assert R.frames(20, 32, 16) == 0 and R.frames(16, 32, 16) == 0 and R.frames(32, 32, 16) == 1      # Lb + 2 pad < n_fft; Lb <= pad; one frame


# ---------------------------------------------------------------------------------------------------------------
# finish and its backward
def test_finish_is_the_oracles_mel_spectrogram_given_torch_stft():
    n_fft, hop, mels, L = 128, 32, 8, 1000
    y = torch.from_numpy(0.9 * np.tanh(np.random.default_rng(3).standard_normal((2, L))))
    want = M.mel_spectrogram(y, n_fft, mels, 16000, hop, n_fft, 0, None, dtype=torch.float64).numpy()
    pad = (n_fft - hop) // 2
    st = torch.stft(_padded(y, pad), n_fft, hop_length=hop, win_length=n_fft, window=torch.hann_window(n_fft, dtype=torch.float64),
                    center=False, onesided=True, return_complex=True)
    nb, Fr = st.shape[1], st.shape[2]
    spec = np.concatenate([st.real.numpy(), st.imag.numpy(), np.full((2, 5, Fr), np.nan)], 1)        # pad rows: NaN
    value, bound = R.finish(spec, M.mel_filterbank(16000, n_fft, mels, 0, 8000), Fr, nb)
    assert value.shape == want.shape == (2, mels, R.frames(L, hop, pad))
    assert np.abs(value - want).max() <= 1e-7                         # 1e-9f and 1e-5f against the oracle's doubles
    assert np.isfinite(bound).all() and (bound > 0).all() and bound.max() < 1e-4


def _clamp_records():
    return [c for c in K.on_device(K.FINISH + K.FINISH_GOLDEN)]


@pytest.mark.parametrize('c', _clamp_records(), ids=K.ids(_clamp_records()))
def test_every_record_keeps_the_clamp_gap_and_has_finite_bounds(c):
    d, F_, nb = K.draw_finish(c), c['F'], c['nb']
    gap, rel = R.clamp_gap(d['spec'], d['basis'], F_, nb)
    assert gap >= R.GAP and rel < 2.0 ** -6, (gap, rel)              # |d acc| is no more than 1/64 of the distance to the clamp
    assert (d['basis'] >= 0).all() and np.isnan(d['spec'][:, 2 * nb:]).all() and np.isnan(d['spec'][:, :, F_:]).all()
    value, bound = R.finish(d['spec'], d['basis'], F_, nb)
    assert np.isfinite(value).all() and np.isfinite(bound).all() and (bound > 0).all()
    assert bound.max() <= (nb + 4 + 12 * R.LOG_C) * R.U * 1.01          # nb + 3.5 roundings relative, and |log| <= log(1e5) = 11.6 here
    p = R._parts(d['spec'], d['basis'], F_, nb)
    shut = p['acc'] < R.C5
    assert {'loud': not shut.any(), 'silence': shut.all(), 'mixed': (shut.any() and not shut.all()) or shut.size < 4, 'tiny': True,
            'golden': shut.any() and not shut.all()}[c['data']]
    # the per-item form: within F_b the plain value, 0.0 behind it, NaN in the spec there
    vl, bl = R.finish_len(K.spec_for_len(c, d), d['basis'], F_, nb, c['lens'], c['len_mul'], c['hop'], c['n_fft'])
    for b, Fb in enumerate(R.item_frames(c['lens'], c['len_mul'], c['hop'], c['n_fft'], F_)):
        one = R.finish(d['spec'][b:b + 1, :, :Fb], d['basis'], Fb, nb) if Fb else (np.zeros((1, c['n_mels'], 0)),) * 2
        assert np.array_equal(vl[b, :, :Fb], one[0][0]) and np.array_equal(bl[b, :, :Fb], one[1][0])
        assert not vl[b, :, Fb:].any() and not bl[b, :, Fb:].any()
    # the backward
    gv, gb = R.finish_bwd(d['spec'], d['basis'], d['gout'], F_, nb)
    assert np.isfinite(gv).all() and np.isfinite(gb).all() and (gb >= 0).all() and (gb[gv != 0] > 0).all()
    assert not gv.transpose(0, 2, 1)[shut.all(1)].any()                 # a frame on the clamped side: exactly 0.0 in every bin
    if c['data'] == 'golden' or (c['data'] == 'mixed' and shut.size >= 4):
        assert gv.transpose(0, 2, 1)[~shut.all(1)].any()


def test_the_item_frames_reach_every_position():
    kinds = set()
    for c in K.FINISH:
        for Fb in R.item_frames(c['lens'], c['len_mul'], c['hop'], c['n_fft'], 10 ** 9):
            kinds.add('zero' if Fb == 0 else 'edge' if Fb % 16 == 0 and Fb < c['F'] else 'F' if Fb == c['F'] else 'beyond' if Fb > c['F'] else 'mid')
    assert kinds == {'zero', 'edge', 'F', 'beyond', 'mid'}


def test_a_silent_frame_of_the_reference_filterbank_is_clamped():
    """mag = sqrt(1e-9f) = 3.1623e-5 in every bin, and the largest row sum of the committed 80 x 513 filterbank is 0.0654 (row 1; the
    area-normalised triangles: about one bin width, 1 / 15.625 Hz): acc <= 2.07e-6, a fifth of the clamp.  Silence trains through it."""
    basis = np.load(K.GOLDEN)['basis.ref_16k_1024_80_0_8000'].astype(np.float64)
    top = basis.sum(1).max() * K.M0
    print('largest acc of a silent frame: %.4g (row sums %.4g .. %.4g)' % (top, basis.sum(1).min(), basis.sum(1).max()))
    assert 1.5e-6 < top < 2.5e-6 < R.C5 and abs(K.M0 - 3.1623e-5) < 1e-9


@pytest.mark.parametrize('data', ['loud', 'mixed', 'tiny'])
def test_finish_bwd_is_torch_autograd_through_the_clamp(data):
    c = next(c for c in K.FINISH if c['data'] == data and c['nb'] == 17)
    d, F_, nb = K.draw_finish(c), c['F'], c['nb']
    value, _ = R.finish_bwd(d['spec'], d['basis'], d['gout'], F_, nb)
    t = torch.from_numpy(d['spec'][:, :2 * nb, :F_].astype(np.float64)).requires_grad_(True)
    mag = torch.sqrt(t[:, :nb] ** 2 + t[:, nb:] ** 2 + R.C9)
    out = torch.log(torch.clamp(torch.matmul(torch.from_numpy(d['basis'].astype(np.float64)), mag), min=R.C5))
    assert np.array_equal(out.detach().numpy(), R.finish(d['spec'], d['basis'], F_, nb)[0]) or \
        np.abs(out.detach().numpy() - R.finish(d['spec'], d['basis'], F_, nb)[0]).max() < 1e-13
    (out * torch.from_numpy(d['gout'].astype(np.float64))).sum().backward()
    assert np.abs(value - t.grad.numpy()).max() <= 1e-12 * max(1.0, np.abs(value).max())


def test_the_clamp_passes_the_gradient_on_its_closed_side():
    acc = torch.tensor([R.C5 * (1 - 2.0 ** -30), R.C5, R.C5 * (1 + 2.0 ** -30)], dtype=torch.float64, requires_grad=True)
    torch.log(torch.where(acc >= R.C5, acc, torch.full_like(acc, R.C5))).sum().backward()
    assert acc.grad[0] == 0 and acc.grad[1] == 1 / R.C5 and acc.grad[2] > 0


# ---------------------------------------------------------------------------------------------------------------
# the bounds on the kernels' own operation order in float32, and on a basis with one weight off by 2^-12
@pytest.mark.parametrize('id', ['loud_nb17_m17_F1_B3', 'mixed_nb17_m17_F16_B3', 'loud_nb40_m80_F33', 'len_mul5_nb16_m15_F33'])
def test_the_bound_holds_on_the_emulation_and_not_on_a_perturbed_weight(id):
    c = next(c for c in K.FINISH if c['id'] == id)
    d, F_, nb = K.draw_finish(c), c['F'], c['nb']
    value, bound = R.finish(d['spec'], d['basis'], F_, nb)
    gvalue, gbound = R.finish_bwd(d['spec'], d['basis'], d['gout'], F_, nb)
    got, acc, _ = R.finish_emulated(d['spec'], d['basis'], F_, nb)
    assert np.array_equal(acc >= np.float32(1e-5), R._parts(d['spec'], d['basis'], F_, nb)['acc'] >= R.C5)       # every entry on its side
    r = R.worst_ratio(got, value, bound), R.worst_ratio(R.finish_bwd_emulated(d['spec'], d['basis'], d['gout'], F_, nb), gvalue, gbound)
    off = d['basis'].copy()
    m, col = 0, int(np.argmax(off[0]))
    off[m, col] *= np.float32(1 + 2.0 ** -12)
    ro = (R.worst_ratio(R.finish_emulated(d['spec'], off, F_, nb)[0], value, bound),
          R.worst_ratio(R.finish_bwd_emulated(d['spec'], off, d['gout'], F_, nb), gvalue, gbound))
    print(id, 'emulation: error / bound %.3g (finish) %.3g (finish_bwd); one weight off by 2^-12: %.3g, %.3g' % (r + ro))
    assert max(r) <= 1.0 and min(ro) > 1.0


# ---------------------------------------------------------------------------------------------------------------
# the dispatch table: one row per call of every record
ROWS = [(g, c, e) for g, c in K.ALL for e in K.entries(g, c)]


@pytest.mark.parametrize('group,c,e', ROWS, ids=['%s-%s-%s' % (g, c['id'], e[0]) for g, c, e in ROWS])
def test_dispatch_of_every_record(group, c, e):
    entry, rc_want, kernels = e
    rc, names = K.dispatch(entry, c)
    assert (rc, names) == (rc_want, kernels), (rc, names)


def test_the_table_reaches_all_six_kernels_and_every_refusal():
    seen = {n for g, c, e in ROWS for n in e[2]}
    assert sorted(seen) == sorted(K.KERNELS) and len(K.KERNELS) == 6
    assert all(len(e[2]) == (1 if e[1] == K.OK else 0) for g, c, e in ROWS)                      # one launch per call, none after a refusal
    refused = {(e[0], e[1]) for g, c, e in ROWS if e[1] != K.OK}
    assert refused == {(n, r) for n in ('phases', 'phases_bwd', 'phases_len', 'finish', 'finish_len', 'finish_bwd') for r in (K.E_ARG, K.E_SHAPE)}
    assert all(c['rc'] != K.OK or c['id'].endswith(('minus_1', '1024', '1025_refused', 'F_hop_2p31_refused')) for g, c in K.ALL if c['host_only'])


def test_the_records_reach_the_edges_they_name():
    P = K.PHASES
    assert {c['hop'] for c in P} == {1, 3, 32} and {0, 1, 5} <= {c['pad'] for c in P} and {c['B'] for c in P} == {1, 3}
    assert any(c['L'] - 1 <= 2 * c['pad'] and c['pad'] > 0 for c in P) and any(c['L'] == c['pad'] + 1 and c['pad'] > 1 for c in P)
    assert any(c['L'] == 2 for c in P) and any(c['FP'] == K.fp_min(c['L'], c['hop'], c['pad']) for c in P) and any(c['FP'] > K.fp_min(c['L'], c['hop'], c['pad']) for c in P)
    Fi = K.FINISH
    assert {c['nb'] for c in Fi} >= {1, 15, 16, 17, 40} and {c['n_mels'] for c in Fi} >= {1, 15, 16, 17, 80} and {c['F'] for c in Fi} == {1, 15, 16, 17, 33}
    assert {c['FP'] > c['F'] for c in Fi} == {True, False} == {c['Cs'] > 2 * c['nb'] for c in Fi} and {c['B'] for c in Fi} == {1, 3}
    assert {c['data'] for c in Fi} == set(K.DATA) and K.FINISH_GOLDEN[0]['F'] == 17
    assert all(np.isnan(K.draw_phase_len(c)['y']).any() for c in K.PHASES_LEN[:4])
