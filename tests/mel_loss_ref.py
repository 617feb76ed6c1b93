"""What `mel.mel_loss` computes, restated in fp64 on the CPU with oracle/mel_oracle.py and torch autograd, and the cases, signals and targets
that tests/test_mel_loss_cpu.py and tests/test_mel_loss_gpu.py share.  Geometries, signals and the oracle's own float32 gap are
tests/stft_ref.py's.

The loss.  Item b holds n_b = min(lengths[b] * len_mul, L) samples and counts F_b = min(mel_frames(n_b), F, F_t) frames of the mel that
y[b:b+1, :n_b] alone gives (the oracle on the TRIMMED signal: the reflection is about the item's own last sample):
    loss = scale * sum_b sum_{m, f < F_b} |mel_b[m][f] - t[b][f][m]| / (num_mels * sum_b F_b),      0 when no entry is valid
    per_item[b] = the mean of the same entries of item b alone, 0 for F_b = 0.
Without lengths every item holds L samples.

The targets are t = m64 + s * (0.05 + u), m64 the fp64 oracle mel, s a random sign, u uniform in [0, 1): |m64 - t| >= 0.05 on every valid
entry, so the sign of mel - t is the same in float32 and in fp64, and d loss / d y is the gradient of sum(mel * G) for the FIXED cotangent
G = scale * sign(m64 - t) / (num_mels * sum_b F_b): stft_ref.oracle_gaps(y_item, cfg, G_item) applies per item as it stands."""
import numpy as np
import torch

from tests import stft_ref as S

MARGIN = 0.05
EXTRA_FRAMES = 2          # the loader's targets run past the generated frames (dataset.py:194-218): F_t = F + 2
REF_GEO = (1024, 256, 1024)


def _geometry(geo):
    from wavthruvec_pytorch_amd import mel
    return mel.stft_geometry(*geo)


def _last_length(geo):
    g = _geometry(geo)
    return [L for L in S.lengths_of(geo[0], geo[1], g['pad']) if S.frames(L, g) and L > 1][-1]


def _lens3(L, pad):
    return [L, pad + 1, (L + pad + 1) // 2]


def _case(name, geo, mels, L, len_mul, lens, scale, seed):
    return dict(name=name, geo=tuple(geo), mels=mels, L=L, len_mul=len_mul, lens=list(lens), scale=scale, seed=seed, cfg=S.cfg_of(geo, mels))


def _build_cases():
    out = [_case('samples', REF_GEO, 80, 4100, 1, [4100, 385, 640, 1023, 2049, 4099], 45.0, 41),     # (45: the weight of train.py:204)
           _case('frames', REF_GEO, 80, 3840, 320, [12, 2, 5, 11], 45.0, 42)]
    for i, geo in enumerate(S.SMALL):
        L = _last_length(geo)
        out.append(_case(S.gid(geo), geo, S.SMALL_MELS, L, 1, _lens3(L, _geometry(geo)['pad']), 1.0, 50 + i))
    for i, geo in enumerate(S.LARGE[1:]):
        out.append(_case(S.gid(geo), geo, S.LARGE_MELS, 4096, 1, _lens3(4096, _geometry(geo)['pad']), 1.0, 60 + i))
    return out


CASES = _build_cases()
IDS = [c['name'] for c in CASES]


def samples_of(c):
    """n_b per item."""
    return [min(n * c['len_mul'], c['L']) for n in c['lens']]


def frames_of(c, Ft=None):
    """(F, F_t, [F_b])."""
    g = _geometry(c['geo'])
    F = S.frames(c['L'], g)
    Ft = F + EXTRA_FRAMES if Ft is None else Ft
    return F, Ft, [min(S.frames(n, g), F, Ft) for n in samples_of(c)]


def oracle_mel(y_item, cfg):
    """(num_mels, F_b) fp64: the oracle on one trimmed item y_item (1, n_b)."""
    from oracle import mel_oracle as M
    return M.mel_spectrogram(torch.as_tensor(y_item), *cfg, dtype=torch.float64)[0].numpy()


def make_inputs(c):
    """-> (y (B, L) float32, tgt (B, F_t, num_mels) float32 frames first, zeros past F_b, [m64 per item or None])."""
    B = len(c['lens'])
    y = S.signal(B, c['L'], c['seed'])
    F, Ft, Fb = frames_of(c)
    rng = np.random.default_rng(c['seed'] + 1000)
    tgt = np.zeros((B, Ft, c['mels']), dtype=np.float32)
    m64 = []
    for b, (n, f) in enumerate(zip(samples_of(c), Fb)):
        if not f:
            m64.append(None)
            continue
        m = oracle_mel(y[b:b + 1, :n], c['cfg'])[:, :f]
        sgn = np.where(rng.uniform(size=m.shape) < 0.5, -1.0, 1.0)
        t = (m + sgn * (MARGIN + rng.uniform(size=m.shape))).astype(np.float32)
        t = np.where(np.abs(m - t) >= MARGIN, t, (m + sgn * (2 * MARGIN)).astype(np.float32))     # (the float32 rounding of t at u = 0)
        tgt[b, :f] = t.T
        m64.append(m)
    return y, tgt, m64


def loss_torch(y, tgt, cfg, ns, Fb, scale):
    """The loss in torch fp64 through the oracle, item by item on the trimmed signals -> (loss, [per-item mean or 0.], d loss / d y (B, L))."""
    from oracle import mel_oracle as M
    mels = cfg[1]
    yt = torch.from_numpy(np.asarray(y, dtype=np.float32)).double().requires_grad_(True)
    tt = torch.from_numpy(np.asarray(tgt, dtype=np.float32)).double()
    sums = []
    for b, (n, f) in enumerate(zip(ns, Fb)):
        if f:
            m = M.mel_spectrogram(yt[b:b + 1, :n], *cfg, dtype=torch.float64)[0][:, :f]
            sums.append((m - tt[b, :f].t()).abs().sum())
        else:
            sums.append(yt.new_zeros(()))
    count = mels * sum(Fb)
    loss = scale * torch.stack(sums).sum() / count if count else yt.sum() * 0
    loss.backward()
    per = [float(s.detach()) / (mels * f) if f else 0.0 for s, f in zip(sums, Fb)]
    return float(loss.detach()), per, yt.grad.numpy()


_REF = {}


def reference(c):
    """Everything the GPU tests hold one case to, computed once: y, tgt, ns, F, Ft, Fb, want (the loss), per (per-item means), dy (B, L) fp64
    with zeros past n_b, gap_out / gap_dy per item (the oracle's own float32 gap on the trimmed item, stft_ref.oracle_gaps), m64."""
    r = _REF.get(c['name'])
    if r is not None:
        return r
    y, tgt, m64 = make_inputs(c)
    ns = samples_of(c)
    F, Ft, Fb = frames_of(c)
    mels, scale = c['mels'], c['scale']
    coef = scale / (mels * sum(Fb))
    dy = np.zeros(y.shape, dtype=np.float64)
    gap_out, gap_dy, S_b = [], [], []
    for b, (n, f) in enumerate(zip(ns, Fb)):
        if not f:
            gap_out.append(0.0), gap_dy.append(0.0), S_b.append(0.0)
            continue
        t = tgt[b, :f].T.astype(np.float64)
        G = (coef * np.sign(m64[b] - t)).astype(np.float32)[None]
        o64, d64, go, gd = S.oracle_gaps(y[b:b + 1, :n], c['cfg'], G)
        assert np.array_equal(o64[0], m64[b])
        dy[b, :n] = d64[0] * (coef / float(np.float32(coef)))            # (G went through float32)
        gap_out.append(go), gap_dy.append(gd)
        S_b.append(float(np.abs(o64[0] - t).sum()))
    r = dict(y=y, tgt=tgt, ns=ns, F=F, Ft=Ft, Fb=Fb, want=coef * sum(S_b), per=[s / (mels * f) if f else 0.0 for s, f in zip(S_b, Fb)],
             dy=dy, gap_out=gap_out, gap_dy=gap_dy, m64=m64)
    _REF[c['name']] = r
    return r
