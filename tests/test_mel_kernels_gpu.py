"""Every record of tests/mel_cases.py on the device: the six kernels of csrc/v2w_mel.hip that its seven first entry points launch, each against the fp64
statement of its own operation (tests/mel_ref.py), per entry.  tests/test_mel_ref_cpu.py asserts which kernel each call launches.

The two phase kernels and their adjoint move or add floats in a fixed order and are held bit for bit; the finish kernels and their backward
are held to |got - want| <= bound with the bound of tests/mel_ref.py (no entry is excluded: the records keep every acc 2^-10 away from the
clamp).  Outputs start as NaN (dspec: as a sentinel, the caller's zero fill stands in it) between sentinel guards, inputs lie between NaN
guards, pad rows, columns >= F and y[b, Lb:] hold NaN, everything a call has no business writing keeps its bits - after a refusal,
everything - and every call runs twice from restored buffers and must give the same bits.  Each test prints its worst error / bound ratio
(`-s` shows them; DESIGN.md 3d'' records them).

test_mel_spectrogram_at_a_second_configuration runs mel.py itself at n_fft 128 / hop 32 / 8 mels, forward and backward, and cuts the chain
at every buffer the five launches leave in memory (the DFT conv against tests/tile_ref.py on the device's own xp / dspec), then compares the
ends with oracle/mel_oracle.py in fp64.

Worst ratios on an MI355X when these tests were written: v2w_mel_finish and _len 0.40 (mixed_nb1_m80_F33), v2w_mel_finish_bwd 0.31
(tiny_nb1_m1_F15); the chain's spec 0.023, out 0.12, dspec 0.066, dxp 0.0087, the output against the oracle 0.011 of the propagated bound,
the gradient against the oracle 0.058 / 0.099 / 0.115 * 2^-24 * n_fft * max|grad| at L = 49 / 200 / 1000 (bar: 0.46).  Division 0.9901,
sqrtf 0.9910, logf 3.0495 units of 2^-24.  The file takes 4 s after the library is loaded.  One-line mutants of csrc/v2w_mel.hip (values only,
each built into a library of its own and run once): DESIGN.md 3d'' has the table; the 1e-9f, both sides of the clamp and the left-reflection
edge of the phase backward failed no earlier test."""
import numpy as np
import pytest
import torch

from tests import mel_cases as K
from tests import mel_ref as R
from tests import tile_ref as T
from tests.test_cbn_kernels_gpu import _addr, _inp, _kept, _out, _state, _twice
from tests.test_disc_kernels_gpu import _cases, _report, env  # noqa: F401  (env: the module-scoped fixture)
from tests.test_tile_kernels_gpu import _sync_or_stop

pytestmark = pytest.mark.gpu


def _bits_equal(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


def _lens(dev, d):
    return torch.from_numpy(d['lens']).to(dev)


# ---------------------------------------------------------------------------------------------------------------
# v2w_mel_phases, v2w_mel_phases_bwd: bit for bit
@_cases(K.on_device(K.PHASES + K.PHASES_LOOP + K.PHASES_REFUSED))
def test_phases_and_their_adjoint(env, c):
    dev, _hip, lib, st = env
    d, ok = K.draw_phase(c), c['rc'] == K.OK
    A = dict(y=_inp(dev, d['y']), dxp=_inp(dev, d['dxp']),
             xp=_out(dev, c['B'], c['hop'], c['FP']) if ok else _out(dev, 64), dy=_out(dev, c['B'], c['L']) if ok else _out(dev, 64))
    t, name = _addr(A), 'phases ' + c['id']
    assert _twice(A, name, lambda: (K.call('phases', c, t, st)[0], K.call('phases_bwd', c, t, st)[0])) == (c['rc'], c['rc'])
    if not ok:
        _kept(A, set(), name)
        return
    _kept(A, {'xp', 'dy'}, name)
    assert _bits_equal(A['xp'].get(), R.phases(d['y'], c['hop'], c['pad'], c['FP'])[0]), name + ': xp'
    assert _bits_equal(A['dy'].get(), R.phases_bwd(d['dxp'], c['L'], c['hop'], c['pad'])[0]), name + ': dy'


@_cases(K.on_device(K.PHASES_LEN + K.PHASES_LEN_REFUSED))
def test_phases_len(env, c):
    dev, _hip, lib, st = env
    d, ok = K.draw_phase_len(c), c['rc'] == K.OK
    A = dict(y=_inp(dev, d['y']), xp=_out(dev, c['B'], c['hop'], c['FP']) if ok else _out(dev, 64))
    lens = _lens(dev, d)
    t, name = dict(_addr(A), len=lens.data_ptr()), 'phases_len ' + c['id']
    assert _twice(A, name, lambda: K.call('phases_len', c, t, st)[0]) == c['rc']
    assert torch.equal(lens.cpu(), torch.from_numpy(d['lens']))
    if not ok:
        _kept(A, set(), name)
        return
    _kept(A, {'xp'}, name)
    assert _bits_equal(A['xp'].get(), R.phases_len(d['y'], c['hop'], c['pad'], c['FP'], c['lens'], c['len_mul'])[0]), name


# ---------------------------------------------------------------------------------------------------------------
# v2w_mel_finish, v2w_mel_finish_len, v2w_mel_finish_bwd
def _fin_out(dev, c, ok):
    return _out(dev, c['B'], c['n_mels'], c['F']) if ok else _out(dev, 64)


@_cases(K.on_device(K.FINISH + K.FINISH_GOLDEN + K.FINISH_REFUSED))
def test_finish_and_finish_len(env, c):
    dev, _hip, lib, st = env
    d, name = K.draw_finish(c), 'finish ' + c['id']
    F, nb = c['F'], c['nb']
    ratios = {}
    # the plain call
    ok = c['rc'] == K.OK
    A = dict(spec=_inp(dev, d['spec']), basis=_inp(dev, d['basis']), out=_fin_out(dev, c, ok))
    assert _twice(A, name, lambda: K.call('finish', c, _addr(A), st)[0]) == c['rc']
    _kept(A, {'out'} if ok else set(), name)
    if ok:
        plain = A['out'].get().copy()
        ratios['out'] = R.worst_ratio(plain, *R.finish(d['spec'], d['basis'], F, nb))
    # per-item lengths: NaN in every frame past the item's own
    ok_len = c['rc_len'] == K.OK
    lens_np = np.asarray(c['lens'], dtype=np.int32)
    lens = torch.from_numpy(lens_np).to(dev)
    A = dict(spec=_inp(dev, K.spec_for_len(c, d) if ok_len else d['spec']), basis=_inp(dev, d['basis']), out=_fin_out(dev, c, ok_len))
    t = dict(_addr(A), len=lens.data_ptr())
    assert _twice(A, name + ' len', lambda: K.call('finish_len', c, t, st)[0]) == c['rc_len']
    _kept(A, {'out'} if ok_len else set(), name + ' len')
    assert torch.equal(lens.cpu(), torch.from_numpy(lens_np))
    if ok_len:
        got = A['out'].get()
        ratios['out_len'] = R.worst_ratio(got, *R.finish_len(d['spec'], d['basis'], F, nb, c['lens'], c['len_mul'], c['hop'], c['n_fft']))
        for b, Fb in enumerate(R.item_frames(c['lens'], c['len_mul'], c['hop'], c['n_fft'], F)):
            assert _bits_equal(got[b, :, :Fb], plain[b, :, :Fb]), name + ': the item frames differ from the plain call'
            assert _bits_equal(got[b, :, Fb:], np.zeros((c['n_mels'], F - Fb))), name + ': frames past F_b are not +0.0'
    _report(name, **ratios)


@_cases(K.on_device(K.FINISH + K.FINISH_GOLDEN + K.FINISH_REFUSED))
def test_finish_bwd(env, c):
    dev, _hip, lib, st = env
    d, name = K.draw_finish(c), 'finish_bwd ' + c['id']
    F, nb, ok = c['F'], c['nb'], c['rc_bwd'] == K.OK
    A = dict(spec=_inp(dev, d['spec']), basis=_inp(dev, d['basis']), basisT=_inp(dev, np.ascontiguousarray(d['basis'].T) if ok else d['basis']),
             gout=_inp(dev, d['gout']), dspec=_state(dev, np.full(d['spec'].shape, 555.0, dtype=np.float32)))
    assert _twice(A, name, lambda: K.call('finish_bwd', c, _addr(A), st)[0]) == c['rc_bwd']
    if not ok:
        _kept(A, set(), name)
        return
    _kept(A, {'dspec'}, name)
    own = np.zeros(d['spec'].shape, dtype=bool)
    own[:, :2 * nb, :F] = True
    assert A['dspec'].unchanged(keep=~own), name + ': pad rows or columns >= F were written'
    got = A['dspec'].get()[:, :2 * nb, :F]
    value, bound = R.finish_bwd(d['spec'], d['basis'], d['gout'], F, nb)
    shut = (R._parts(d['spec'], d['basis'], F, nb)['acc'] < R.C5).all(1)                       # (B, F): every mel of the frame is clamped
    assert (got.transpose(0, 2, 1)[shut] == 0).all(), name + ': a frame on the clamped side has a gradient'
    _report(name + ' clamped frames %d / %d' % (shut.sum(), shut.size), dspec=R.worst_ratio(got, value, bound))


# ---------------------------------------------------------------------------------------------------------------
# the device's fp32 division, sqrtf and logf on arguments the kernels compute exactly
def test_device_function_errors(env):
    """mel_ref.DIV_C, SQRT_C, LOG_C are twice the worst error seen here in units of 2^-24 (relative), rounded up.
    division: N bins of magnitude 1 (re = 1: 1 + 1e-9f rounds to 1), basis = diag(b), basisT = the identity: dspec[c][f] = fl(g[c][f] / b[c]).
    sqrtf: bins (1, im) with im a multiple of 2^-11 below sqrt(3) (t = 1 + im^2 < 4 is exact in 24 bits), one more bin (1, 0) that alone has a basis
           weight (1.0), gout = 1, basisT = ones: dspec[c][f] = fl(1 / sqrtf(t)).  Where that is the correctly rounded quotient of the correctly
           rounded root - expected everywhere - sqrtf's error is that root's; elsewhere the whole difference is charged to sqrtf.
    logf: re = x in [1, 2) on 11 fractional bits (x^2 + 1e-9f rounds to x^2, whose root is x), basis = diag(b), b on 11 fractional bits times
          2^e: out = logf(b x), the product exact."""
    dev, _hip, lib, st = env
    rng = np.random.default_rng(11)
    N, F, B = 64, 64, 4
    f32 = np.float32

    def run(entry, c, **arrs):
        A = {k: _inp(dev, v) for k, v in arrs.items()}
        A['out' if entry == 'finish' else 'dspec'] = _out(dev, c['B'], c['n_mels'], c['F']) if entry == 'finish' else _out(dev, c['B'], c['Cs'], c['FP'])
        assert K.call(entry, c, _addr(A), st)[0] == K.OK
        _sync_or_stop('device functions ' + entry)
        return A['out' if entry == 'finish' else 'dspec'].get()

    # division
    c = K.fin('probe_div', B=B, nb=N, n_mels=N, F=F)
    spec = np.zeros((B, 2 * N, F), dtype=f32)
    spec[:, :N] = 1.0
    b = (2.0 ** rng.uniform(-13, 10, N)).astype(f32)
    g = (2.0 ** rng.uniform(-10, 10, (B, N, F)) * rng.choice([-1.0, 1.0], (B, N, F))).astype(f32)
    q = run('finish_bwd', c, spec=spec, basis=np.diag(b), basisT=np.eye(N, dtype=f32), gout=g)[:, :N]
    want = g.astype(np.float64) / b.astype(np.float64)[None, :, None]
    div = float((np.abs(q - want) / (R.U * np.abs(want))).max())
    div_exact = float((q == (g / b[None, :, None]).astype(f32)).mean())
    # sqrtf
    c = K.fin('probe_sqrt', B=B, nb=N + 1, n_mels=1, F=F)
    spec = np.zeros((B, 2 * (N + 1), F), dtype=f32)
    spec[:, :N + 1] = 1.0
    im = (rng.integers(1, 3548, (B, N, F)) * 2.0 ** -11).astype(f32)
    spec[:, N + 1:2 * N + 1] = im
    basis = np.zeros((1, N + 1), dtype=f32)
    basis[0, N] = 1.0
    r = run('finish_bwd', c, spec=spec, basis=basis, basisT=np.ones((N + 1, 1), dtype=f32), gout=np.ones((B, 1, F), dtype=f32))[:, :N]
    tt = 1.0 + im.astype(np.float64) ** 2
    assert (tt.astype(f32) == tt).all()
    root = np.sqrt(tt.astype(f32)).astype(f32)                                      # numpy's float32 sqrt is correctly rounded
    same = r == (f32(1) / root).astype(f32)
    e_root = np.abs(root - np.sqrt(tt)) / (R.U * np.sqrt(tt))
    e_whole = np.abs(r - 1 / np.sqrt(tt)) * np.sqrt(tt) / R.U
    sq = float(np.where(same, e_root, e_whole).max())
    # logf
    c = K.fin('probe_log', B=B, nb=N, n_mels=N, F=F)
    x = (1 + rng.integers(0, 2048, (B, N, F)) * 2.0 ** -11).astype(f32)
    spec = np.zeros((B, 2 * N, F), dtype=f32)
    spec[:, :N] = x
    b = ((1 + rng.integers(0, 2048, N) * 2.0 ** -11) * 2.0 ** rng.integers(-17, 11, N)).astype(f32)
    b[:8] = (1 + rng.integers(0, 64, 8) * 2.0 ** -11) * 0.5                          # b x within a few percent of 1
    lg = run('finish', c, spec=spec, basis=np.diag(b))
    a = b.astype(np.float64)[None, :, None] * x
    assert (a.astype(f32) == a).all()
    use = a >= R.C5 * (1 + R.GAP)
    with np.errstate(divide='ignore', invalid='ignore'):
        rel = np.where(use & (a != 1), np.abs(lg - np.log(a)) / (R.U * np.abs(np.log(a))), 0.0)
    absolute = float(np.where(use, np.abs(lg - np.log(a)) / R.U, 0.0).max())
    lo = float(rel.max())
    print('[device functions] division %.4f u (%d probes, %.4f of them the correctly rounded quotient), sqrtf %.4f u (%d probes, %.4f of the quotients '
          'as from the correctly rounded root; whole 1 / sqrtf %.4f u), logf %.4f u relative at a = %r (%d probes; %.3f u absolute)'
          % (div, q.size, div_exact, sq, r.size, float(same.mean()), float(e_whole.max()), lo, float(a.reshape(-1)[int(rel.argmax())]), int(use.sum()),
             absolute))
    assert np.isfinite([div, sq, lo]).all()
    assert 2 * div <= R.DIV_C and 2 * sq <= R.SQRT_C and 2 * lo <= R.LOG_C


# ---------------------------------------------------------------------------------------------------------------
# mel.py away from 1024 / 256 / 80
N_FFT, HOP, MELS, SR = 128, 32, 8, 16000
GRAD_C = 0.46         # 4 x the largest figure measured on an MI355X (0.058, 0.099, 0.115 at L = 49, 200, 1000): room for other seeds


@pytest.mark.parametrize('L', [48 + 1, 200, 1000])
def test_mel_spectrogram_at_a_second_configuration(env, monkeypatch, L):
    dev, _hip, lib, st = env
    from oracle import mel_oracle as M
    from wavthruvec_pytorch_amd import mel
    B, pad, k, nb = 2, (N_FFT - HOP) // 2, N_FFT // HOP, N_FFT // 2 + 1
    rng = np.random.default_rng(L)
    y0 = (0.9 * np.tanh(rng.standard_normal((B, L)))).astype(np.float32)
    seen, conv = [], mel.hipops.conv1d

    def spy(x, wf, bias, out, **kw):
        r = conv(x, wf, bias, out, **kw)
        seen.append((x.detach().clone(), wf, out.detach().clone(), dict(kw)))
        return r

    monkeypatch.setattr(mel.hipops, 'conv1d', spy)
    cfg = (N_FFT, MELS, SR, HOP, N_FFT, 0, None)
    yd = torch.from_numpy(y0).to(dev).requires_grad_(True)
    out = mel.mel_spectrogram(yd, *cfg)
    F = mel.mel_frames(L, N_FFT, HOP)
    FP = R.roundup4(F + k - 1)
    assert tuple(out.shape) == (B, MELS, F) and F == (L + 2 * pad - N_FFT) // HOP + 1 >= 1
    G = rng.standard_normal((B, MELS, F)).astype(np.float32)
    (out * torch.from_numpy(G).to(dev)).sum().backward()
    _sync_or_stop('mel chain')
    assert len(seen) == 2
    (xp, wf, spec, kw_f), (dspec, wT, dxp, kw_b) = seen
    consts = mel._constants(*cfg, dev)
    basis = consts['basis'].cpu().numpy()
    assert np.array_equal(basis, M.mel_filterbank(SR, N_FFT, MELS, 0, SR / 2)) and basis.shape == (MELS, nb)
    assert tuple(xp.shape) == (B, HOP, FP) and tuple(spec.shape) == (B, consts['cs'], FP) and kw_f['pad_left'] == 0 and kw_b['pad_left'] == k - 1
    ratios = {}
    # forward, cut at xp and spec
    assert _bits_equal(xp.cpu().numpy(), R.phases(y0, HOP, pad, FP)[0]), 'xp'
    n_f, n_b = k * HOP, k * consts['cs']
    value, S = T.conv1d(xp.cpu(), wf.cpu(), dil=1, pad_left=0)
    ratios['spec'] = R.worst_ratio(spec.cpu(), value.numpy(), n_f * R.U * S.numpy())
    got = out.detach().cpu().numpy()
    ratios['out'] = R.worst_ratio(got, *R.finish(spec.cpu().numpy(), basis, F, nb))
    # the whole forward against the oracle: the conv's bound (plus one rounding of every fp32 DFT weight) through the magnitude and the log
    want = M.mel_spectrogram(torch.from_numpy(y0), *cfg, dtype=torch.float64).numpy()
    v, Sv = value.numpy(), (n_f + 1) * R.U * S.numpy()
    end_value, end_bound = R.through_finish(v[:, :nb, :F], v[:, nb:2 * nb, :F], Sv[:, :nb, :F], Sv[:, nb:2 * nb, :F], basis, nb)
    assert np.abs(end_value - want).max() <= 1e-6                                     # the DFT rows in fp32 against torch.stft in fp64
    ratios['out_oracle'] = R.worst_ratio(got, want, end_bound)
    # backward, cut at dspec and dxp
    ds = dspec.cpu().numpy()
    own = np.zeros(ds.shape, dtype=bool)
    own[:, :2 * nb, :F] = True
    assert (ds[~own] == 0).all(), 'dspec outside the bins and frames'
    ratios['dspec'] = R.worst_ratio(ds[:, :2 * nb, :F], *R.finish_bwd(spec.cpu().numpy(), basis, G, F, nb))
    bvalue, bS = T.conv1d(dspec.cpu(), wT.cpu(), dil=1, pad_left=k - 1)
    ratios['dxp'] = R.worst_ratio(dxp.cpu().numpy(), bvalue.numpy(), n_b * R.U * bS.numpy())
    dy = yd.grad.cpu().numpy()
    assert _bits_equal(dy, R.phases_bwd(dxp.cpu().numpy(), L, HOP, pad)[0]), 'dy'
    # whole against whole: fp64 autograd through the oracle
    yo = torch.from_numpy(y0).double().requires_grad_(True)
    (M.mel_spectrogram(yo, *cfg, dtype=torch.float64) * torch.from_numpy(G).double()).sum().backward()
    go = yo.grad.numpy()
    whole = np.abs(dy - go).max() / (R.U * N_FFT * np.abs(go).max())
    print('[mel chain] L=%d: max |dy - oracle| = %.3f * 2^-24 * n_fft * max|grad| (bar %g)' % (L, whole, GRAD_C))
    ratios['dy_oracle'] = whole / GRAD_C
    _report('mel chain L=%d' % L, **ratios)
