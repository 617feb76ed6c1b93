"""The resampler on the device: resample_kernel and peak_scale_kernel (csrc/v2w_resample.hip) behind v2w_resample and v2w_peak_scale, then
audio.py and `synthesize --out-rate` end to end.  tests/test_resample_cpu.py holds the host-only half.

  1. kernel level, on guarded buffers (NaN-filled outputs between sentinels, inputs between NaN guards, NaN - or, in int16 PCM, full-scale
     junk - in x[b, n_b:]), every call twice from restored buffers with equal bits.  For EVERY output entry, nothing left out:
       (a) against fp64 arithmetic on the kernel's own fp32 table and input:  |got - want| <= (NT + 1) 2^-24 sum_j |h32[p][j] x[s_j]|
       (b) against the restatement of tests/resample_ref.py (fp64 coefficients from t(p, k), no table, no k0): the same with NT + 2
     both the standard bound for NT rounded products and NT - 1 additions in any order (one more rounding per product for the table's cast);
     an entry whose bound is 0 must be exactly 0; out[b, N_b:] is +0.0 bit for bit; a tile's peak partial is the maximum of its |out|.
     Ratios 1:3, 2:3, 3:1, 2:1, 160:441, 441:160, 8:3, 7:5; per ratio n = 1, NT - 1, n whose N is tile - 1, tile, tile + 1, 2 tiles + 3 (the
     first N some n gives from there on), and an Lin that is no multiple of 4; B = 3 with lengths [n, 1, n // 2]; float32 and int16 input.
  2. peak: |got - y 0.95 / max|y|| <= 4 * 2^-24 |want| per entry (one division of at most 1 ulp and one multiply), the maximum equal to
     numpy's, an all-zero item and an item below FLT_MIN keep their bits, the zeros past N_b stay +0.0; peak_normalize alone on (3, 1000).
  3. `synthesize --out-rate 48000` on the synthetic checkpoint of the existing end-to-end test.
Every test here fails without the feature (no wavthruvec_pytorch_amd.audio, no v2w_resample symbol).  Each kernel test prints its worst
error / bound ratio (`-s` shows them).

Measured on an MI355X: worst error / bound 0.36 against the fp32 table and 0.34 against the restatement (both at 1:3, int16 input; 0.16 at
441:160), the peak scaling 0.50 of its bar; the file takes 4.4 s, its slowest test 1.0 s (the first, which loads the library)."""
import os
import wave

import numpy as np
import pytest
import torch

from tests import mel_ref as R
from tests import resample_ref as RR
from tests.test_cbn_kernels_gpu import _addr, _inp, _kept, _out, _twice
from tests.test_disc_kernels_gpu import SENT, _report, env  # noqa: F401  (env: the module-scoped fixture)
from tests.test_mel_kernels_gpu import _bits_equal
from tests.test_tile_kernels_gpu import GUARD, _sync_or_stop

pytestmark = pytest.mark.gpu
OK = 0
FLT_MIN = float(np.finfo(np.float32).tiny)


class Ints:
    """test_cbn_kernels_gpu.Arr for an int16 or int32 payload: [GUARD | payload | GUARD] with `guard` in the guards."""

    def __init__(self, dev, payload, guard):
        payload = torch.as_tensor(payload)
        n = payload.numel()
        flat = torch.full((2 * GUARD + n,), guard, dtype=payload.dtype)
        flat[GUARD:GUARD + n] = payload.reshape(-1)
        self.flat, self.n, self.shape = flat.to(dev), n, tuple(payload.shape)
        self.first = self.flat.clone()
        self.ptr = self.flat.data_ptr() + GUARD * payload.element_size()

    def restore(self):
        self.flat.copy_(self.first)

    def bits(self):
        return self.flat.clone()

    def get(self):
        return self.flat[GUARD:GUARD + self.n].cpu().view(self.shape).numpy()

    def unchanged(self, keep=None):
        return bool((self.flat == self.first).all())


def _table(M, L):
    """The kernel's operands for M : L: (NT, h32 (L, NT), k0 int32) - the identity for 1 : 1."""
    from wavthruvec_pytorch_amd import resample_table
    if M == L:
        return 1, np.ones((1, 1), np.float32), np.zeros(1, np.int32)
    t = resample_table(M, L)
    assert (t['M'], t['L']) == (M, L)
    return t['NT'], t['h'].astype(np.float32), t['k0'].astype(np.int32)


def _plan(env, M, L, NT, B, Lout):
    _dev, _hip, lib, _st = env
    import ctypes as C
    g = _hip.ResampleGrids()
    assert lib.v2w_resample_plan(M, L, NT, B, Lout, C.byref(g)) == OK
    return g


def _x_buffer(dev, x, ns):
    """x (B, Lin) with what lies past n_b made poisonous: NaN for float32, full-scale junk for int16."""
    x = x.copy()
    for b, n in enumerate(ns):
        x[b, max(n, 0):] = np.nan if x.dtype == np.float32 else (32767 if b % 2 else -32768)
    t = torch.from_numpy(x)
    return _inp(dev, t) if x.dtype == np.float32 else Ints(dev, t, 32767)


def _run(env, M, L, x, lens, extra=5, peak=None, with_part=True, with_len=True):
    """v2w_resample (and, with `peak`, v2w_peak_scale) on guarded buffers, twice -> (buffers, plan, NT, h32, k0, n_b list, Lout)."""
    dev, _hip, lib, st = env
    B, Lin = x.shape
    NT, h32, k0 = _table(M, L)
    ns = [min(max(int(v), 0), Lin) for v in lens] if with_len else [Lin] * B
    Lout = -(-Lin * L // M) + extra
    g = _plan(env, M, L, NT, B, Lout)
    A = dict(x=_x_buffer(dev, x, ns), y=_out(dev, B, Lout), h=_inp(dev, torch.from_numpy(h32)), k0=Ints(dev, torch.from_numpy(k0), 1 << 28),
             len=Ints(dev, torch.tensor(lens, dtype=torch.int32), 1 << 28), part=_out(dev, B, g.tiles))
    t = _addr(A)
    i16 = int(x.dtype == np.int16)

    def run():
        rc = lib.v2w_resample(t['x'], i16, t['y'], B, Lin, Lout, t['h'], t['k0'], M, L, NT, t['len'] if with_len else None,
                              t['part'] if with_part else None, st)
        if peak is None or rc != OK:
            return rc
        return lib.v2w_peak_scale(t['y'], B, Lout, t['part'], g.tiles, peak, st)

    what = 'resample %d:%d B=%d Lin=%d %s' % (M, L, B, Lin, x.dtype)
    assert _twice(A, what, run) == OK
    _kept(A, {'y', 'part'} if with_part else {'y'}, what)
    return A, g, NT, h32, k0, ns, Lout


def _check(env, M, L, x, lens, **kw):
    """One call against both references, every entry -> the two worst error / bound ratios."""
    A, g, NT, h32, k0, ns, Lout = _run(env, M, L, x, lens, **kw)
    got, part = A['y'].get(), A['part'].get()
    x64 = RR.f64_of(x)
    worst_a = worst_b = 0.0
    for b, n in enumerate(ns):
        N = -(-n * L // M)
        assert _bits_equal(got[b, N:], np.zeros(Lout - N)), 'out[%d, N_b:] is not +0.0' % b
        if n == 0:
            continue
        want, S = RR.apply_table(x64[b, :n], h32, k0, M, L)
        assert want.shape == (N,)
        worst_a = max(worst_a, R.worst_ratio(got[b, :N], want, RR.bound(NT + 1, S)))
        if M != L:
            want, S = RR.resample(x64[b, :n], M, L)
            worst_b = max(worst_b, R.worst_ratio(got[b, :N], want, RR.bound(NT + 2, S)))
    if kw.get('with_part', True):
        pad = np.zeros((got.shape[0], g.tiles * g.tile), np.float32)
        pad[:, :Lout] = np.abs(got)
        assert _bits_equal(part, pad.reshape(got.shape[0], g.tiles, g.tile).max(axis=2)), 'peak partials'
    return worst_a, worst_b, g


# ---------------------------------------------------------------------------------------------------------------
# 1. kernel level
@pytest.mark.parametrize('i16', [False, True], ids=['f32', 'i16'])
@pytest.mark.parametrize('ratio', RR.RATIOS, ids=RR.rid)
def test_every_entry_within_its_bound(env, ratio, i16):
    M, L = ratio
    NT = _table(M, L)[0]
    tile = _plan(env, M, L, NT, 1, 1).tile
    ratios, seen = {}, set()
    for n in RR.lengths_for(M, L, NT, tile):
        x = np.stack([RR.signal(11 * b + n, n, i16) for b in range(3)])
        a, c, g = _check(env, M, L, x, [n, 1, max(n // 2, 1)], extra=5 if RR.length(n, M, L) % tile else 0)      # (a last tile that is full)
        ratios['n%d' % n], ratios['n%d_chain' % n] = a, c
        seen.add(g.tiles)
    assert seen >= {1, 2, 3}                                       # one tile, the boundary, more than two
    _report('resample %d:%d %s tile %d' % (M, L, 'i16' if i16 else 'f32', tile), **ratios)


def test_lengths_are_clamped_and_optional(env):
    """len[b] past Lin counts as Lin, len[b] <= 0 as an empty item (all +0.0), len == NULL as Lin everywhere; no peak partials asked."""
    M, L = 441, 160
    x = np.stack([RR.signal(b, 3001) for b in range(4)])
    a, c, _g = _check(env, M, L, x, [3001 + 9, 0, -5, 2999], with_part=False)
    a2, c2, _g = _check(env, M, L, x, [7, 7, 7, 7], with_len=False)
    _report('resample 441:160 clamped lengths', table=a, chain=c, nolen_table=a2, nolen_chain=c2)


def test_an_item_in_a_batch_has_the_bits_of_its_own_call(env):
    M, L = 160, 441
    n = 1700
    x = np.stack([RR.signal(b, n) for b in range(3)])
    lens = [n, 613, 1]
    A = _run(env, M, L, x, lens)[0]
    got = A['y'].get()
    for b, nb in enumerate(lens):
        own = _run(env, M, L, x[b:b + 1, :nb], [nb], extra=0)[0]['y'].get()
        assert _bits_equal(got[b, :own.shape[1]], own[0]), b


def test_identity_table_is_the_float32_copy(env):
    """M = L = NT = 1, h = {1}: what audio.resample runs at orig == new.  int16 comes out as x / 32768 exactly, float32 with its bits."""
    x = np.stack([RR.signal(b, 5003) for b in range(2)])
    got = _run(env, 1, 1, x, [5003, 77], extra=0)[0]['y'].get()
    assert _bits_equal(got[0], x[0]) and _bits_equal(got[1, :77], x[1, :77]) and _bits_equal(got[1, 77:], np.zeros(5003 - 77))
    xi = np.stack([RR.signal(b, 5003, True) for b in range(2)])
    got = _run(env, 1, 1, xi, [5003, 5003], extra=0)[0]['y'].get()
    assert _bits_equal(got, xi.astype(np.float32) / np.float32(32768.0))


# ---------------------------------------------------------------------------------------------------------------
# 2. peak
def _peak_inputs(n):
    """Four items: noise, all zeros, below FLT_MIN (denormal samples), noise of half the length."""
    x = np.stack([RR.signal(b, n) for b in range(4)])
    x[1] = 0.0
    x[2] = (x[2] * np.float32(1e-39)).astype(np.float32)
    return x, [n, n, n, n // 2]


@pytest.mark.parametrize('ratio', [(441, 160), (1, 3), (1, 1)], ids=RR.rid)
def test_peak_scale_per_entry(env, ratio):
    M, L = ratio
    x, lens = _peak_inputs(6007)
    plain = _run(env, M, L, x, lens)
    y0, part = plain[0]['y'].get(), plain[0]['part'].get()
    ns, Lout = plain[5], plain[6]
    y1 = _run(env, M, L, x, lens, peak=0.95)[0]['y'].get()
    m = np.abs(y0).max(axis=1)
    assert _bits_equal(part.max(axis=1), m)                       # the maximum itself: numpy's
    assert m[0] >= FLT_MIN and m[1] == 0 and m[2] < FLT_MIN and m[3] >= FLT_MIN
    ratios = {}
    for b in (0, 3):
        want = y0[b].astype(np.float64) * 0.95 / float(m[b])
        ratios['item%d' % b] = R.worst_ratio(y1[b], want, 4 * RR.U * np.abs(want))
        assert abs(float(np.abs(y1[b]).max()) - 0.95) <= 4 * RR.U
        N = -(-ns[b] * L // M)
        assert _bits_equal(y1[b, N:], np.zeros(Lout - N))
    assert _bits_equal(y1[1], y0[1]) and _bits_equal(y1[2], y0[2]) and not y1[1].any()
    _report('peak_scale %d:%d' % ratio, **ratios)


def test_peak_normalize_alone(env):
    from wavthruvec_pytorch_amd import peak_normalize
    dev = env[0]
    x, _ = _peak_inputs(1000)
    x, lens = x[[0, 1, 3]], [1000, 1000, 333]
    xd = torch.from_numpy(x).to(dev)
    xd[2, 333:] = float('nan')
    got = peak_normalize(xd, 0.95, lengths=lens)
    same = peak_normalize(xd, peak=0.95, lengths=torch.tensor(lens, device=dev))
    one = peak_normalize(xd[0])
    _sync_or_stop('peak_normalize')
    got, same, one = got.cpu().numpy(), same.cpu().numpy(), one.cpu().numpy()
    assert got.shape == (3, 1000) and got.dtype == np.float32 and one.shape == (1, 1000)
    assert _bits_equal(got, same) and _bits_equal(got[0], one[0])
    ratios = {}
    for b, n in enumerate(lens):
        v = x[b, :n].astype(np.float64)
        want = v * 0.95 / np.abs(v).max() if v.any() else v
        ratios['item%d' % b] = R.worst_ratio(got[b, :n], want, 4 * RR.U * np.abs(want))
        assert _bits_equal(got[b, n:], np.zeros(1000 - n))
    _report('peak_normalize', **ratios)


# ---------------------------------------------------------------------------------------------------------------
# audio.resample
@pytest.mark.parametrize('rate', [(44100, 16000), (16000, 48000), (16000, 16000)], ids=RR.rid)
def test_python_resample(env, rate):
    from wavthruvec_pytorch_amd import audio
    dev = env[0]
    M, L = RR.ratio(*rate)
    n, lens = 4411, [4411, 1, 2205]
    xi = np.stack([RR.signal(b + 5, n, True) for b in range(3)])
    xf = (xi.astype(np.float32) / np.float32(32768.0))
    xd = torch.from_numpy(xi).to(dev)
    out_i = audio.resample(xd, *rate, lengths=lens)
    fd = torch.from_numpy(xf).to(dev)
    for b, nb in enumerate(lens):
        fd[b, nb:] = float('nan')
    out_f = audio.resample(fd, *rate, lengths=torch.tensor(lens))
    out_p = audio.resample(fd, *rate, lengths=lens, peak=0.95)
    one = audio.resample(fd[2, :2205], *rate)
    again = audio.resample(xd, *rate, lengths=lens)
    _sync_or_stop('audio.resample %s' % (rate,))
    N = audio.resampled_length(n, *rate)
    assert out_i.shape == (3, N) and out_i.dtype == torch.float32 and out_i.device == dev and not out_i.requires_grad
    out_i, out_f, out_p, one, again = (t.cpu().numpy() for t in (out_i, out_f, out_p, one, again))
    assert _bits_equal(out_i, out_f) and _bits_equal(out_i, again)                 # x / 32768 is exact; the cached table; run to run
    assert _bits_equal(one[0], out_i[2, :one.shape[1]]) and one.shape == (1, audio.resampled_length(2205, *rate))
    ratios = {}
    for b, nb in enumerate(lens):
        Nb = audio.resampled_length(nb, *rate)
        assert _bits_equal(out_i[b, Nb:], np.zeros(N - Nb)) and _bits_equal(out_p[b, Nb:], np.zeros(N - Nb))
        if M == L:
            assert _bits_equal(out_i[b, :Nb], xf[b, :nb])
        else:
            want, S = RR.resample(RR.f64_of(xi[b, :nb]), *rate)
            ratios['item%d' % b] = R.worst_ratio(out_i[b, :Nb], want, RR.bound(_table(M, L)[0] + 2, S))
        m = float(np.abs(out_i[b]).max())
        assert m >= FLT_MIN
        want = out_i[b].astype(np.float64) * 0.95 / m
        ratios['peak%d' % b] = R.worst_ratio(out_p[b], want, 4 * RR.U * np.abs(want))
    _report('audio.resample %d -> %d' % rate, **ratios)
    with pytest.raises(ValueError, match='64 KiB of LDS'):
        audio.resample(fd, 16000, 44101)
    with pytest.raises(NotImplementedError):
        audio.resample(fd.clone().requires_grad_(True), *rate)


# ---------------------------------------------------------------------------------------------------------------
# 3. synthesize --out-rate
def test_synthesize_out_rate(env, tmp_path):
    """The wav header carries 48000, the frame count is 3 T 320, the samples are the int16 quantisation of resample(plain output) to 1 LSB;
    without the flag the file is today's, byte for byte.  One file, then two files of unequal length in one --batch 2 forward."""
    from oracle import vec2wav_oracle as O
    from wavthruvec_pytorch_amd import audio, synthesize as S, synthetic, utils
    dev = env[0]
    h = synthetic.make_hparams(num_wv_feat=768)
    sd = synthetic.make_state_dict(h, seed=0)
    x, spk, nz = synthetic.make_inputs(h, 1, 20, seed=3)
    O.calibrate_running_stats(sd, h, x, spk, nz)
    d = str(tmp_path)
    utils.save_checkpoint(os.path.join(d, 'g_00000042'), {'generator': sd})
    feats = {'a': x, 'b': x[:, :, :13].contiguous()}
    for k, v in feats.items():
        np.save(os.path.join(d, k + '.npy'), v.permute(0, 2, 1).numpy())
    torch.save(spk.reshape(1, 1, -1), os.path.join(d, 'spk.pth'))
    common = ['--checkpoint', d, '--spk-emb', os.path.join(d, 'spk.pth'), '--seed', '7']
    g = S.build_generator(d, h, dev)
    spk1 = S.load_speaker_embedding(os.path.join(d, 'spk.pth'))

    def frames(path):
        with wave.open(path) as w:
            return w.getframerate(), w.getnframes(), np.frombuffer(w.readframes(w.getnframes()), dtype='<i2')

    def check(names, batch):
        paths = [os.path.join(d, k + '.npy') for k in names]
        out = os.path.join(d, 'o.wav') if len(names) == 1 else os.path.join(d, 'wavs_%d' % batch)
        plain = out + '.plain.wav'
        assert S.main(common + ['--feat'] + paths + ['--out', out, '--batch', str(batch), '--out-rate', '48000']) == 0
        if len(names) == 1:
            assert S.main(common + ['--feat'] + paths + ['--out', plain, '--batch', str(batch)]) == 0
        ys = S.synthesize_many(g, [S.load_latents(p) for p in paths], [spk1] * len(paths), seed=7, batch=batch)
        for k, y, o48 in zip(names, ys, S.output_paths(paths, out)):
            T = feats[k].shape[-1]
            if len(names) == 1:                                   # the same command without the flag: today's file
                today = os.path.join(d, 'today_%s.wav' % k)
                S.write_wav(today, y, 16000)
                assert open(plain, 'rb').read() == open(today, 'rb').read(), k
            rate, nframes, pcm = frames(o48)
            assert rate == 48000 and nframes == 3 * T * 320, (k, rate, nframes)
            up = audio.resample(y.reshape(1, -1), 16000, 48000)
            want = (up.reshape(-1).clamp(-1.0, 1.0).cpu().numpy() * 32767.0).round()
            assert np.abs(pcm.astype(np.float64) - want).max() <= 1, k

    check(['a'], 1)
    check(['a', 'b'], 2)
