"""GPU tests of batched validation: mel_spectrogram(lengths=...), mel_l1 and validate.mel_errors (reference configuration 1024 / 256 / 1024, 80
mels).  The reference of every mel check is oracle/mel_oracle.py on each item's TRIMMED signal; the kernels with lengths are also held, item
by item, to the B = 1 launches on the trimmed item.

The masked L1's bound (`_l1_bound`).  include/vec2wav_hip.h lists the roundings on the way to one stored value:
    [1] fp32 for each a - b: fl(a - b) = (a - b)(1 + d), |d| <= 2^-24 (a difference in the subnormal range is exact); |.| is exact;
    every sum is fp64: n64 = 4 ceil(units / (256 G)) additions in a thread's chain, rounded up to the kernel's four units in flight
        (16 ceil(units / (1024 G))) + [6 + 4] in the workgroup's reduction + [G] over the item's partials
        (total: + [ceil(B / 256) + 6 + 4] over the items) + [1] the fp64 quotient, each within 2^-53 relative of sums of non-negative terms;
    [1] fp32 for the stored value.
With S the exact sum of |a - b| over the N valid elements and want = S / N, the stored value is within
    want * (2 * 2^-24 + (n64 + 1) * 2^-53 + 4 * 2^-48)        (the last term: the second-order products of the above)
of want.  Nothing here was read off the kernel's output."""
import math

import numpy as np
import pytest
import torch

from oracle import mel_oracle as M
from oracle import vec2wav_oracle as O
from wavthruvec_pytorch_amd import _hip, mel, synthetic, validate
from wavthruvec_pytorch_amd.mel import mel_frames, mel_l1, mel_spectrogram

pytestmark = pytest.mark.gpu
N_FFT, HOP, MELS, PAD, K = 1024, 256, 80, 384, 4
CFG = (N_FFT, MELS, 16000, HOP, 1024, 0, None)
MEL_BAR = 2e-4        # tests/test_hip_ops.py::test_mel_spectrogram_matches_oracle: "log of fp32 sums of 513 magnitudes"
U24, U53 = 2.0 ** -24, 2.0 ** -53
# (L, len_mul, lengths): every residue of Lb mod 4 and mod 256, the smallest legal length (385 = pad + 1), reflections that cross a
# 256-sample phase boundary; then the generator's form, lengths in frames of 320 samples
CASES = {'samples': (4100, 1, [4100, 385, 640, 1023, 2049, 4099]), 'frames': (3840, 320, [12, 2, 5, 11])}


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a MI355X'
    return torch.device('cuda:0')


def _signal(B, L, seed=16):
    return torch.from_numpy(np.tanh(np.random.default_rng(seed).standard_normal((B, L))).astype(np.float32) * 0.9)


def _poisoned(y, ns, val):
    y = y.clone()
    for b, n in enumerate(ns):
        y[b, n:] = val
    return y


def _roundup4(n):
    return (n + 3) // 4 * 4


def _phases(y, FP, lens=None, mul=1):
    B, L = y.shape
    lib, st = _hip.load(), torch.cuda.current_stream(y.device).cuda_stream
    xp = torch.full((B, HOP, FP), 7.0, device=y.device)
    if lens is None:
        _hip.check(lib.v2w_mel_phases(y.data_ptr(), xp.data_ptr(), B, L, HOP, PAD, FP, st), 'v2w_mel_phases')
    else:
        _hip.check(lib.v2w_mel_phases_len(y.data_ptr(), xp.data_ptr(), B, L, HOP, PAD, FP, lens.data_ptr(), mul, st), 'v2w_mel_phases_len')
    return xp


# ---- 1. the phases kernel
@pytest.mark.parametrize('case', list(CASES))
@pytest.mark.parametrize('val', [float('nan'), 1e30])
def test_phases_with_lengths_are_the_bits_of_the_trimmed_launches(dev, case, val):
    L, mul, lens = CASES[case]
    ns = [n * mul for n in lens]
    y = _signal(len(ns), L)
    FP = _roundup4(mel_frames(L, N_FFT, HOP) + K - 1)
    xp = _phases(_poisoned(y, ns, val).to(dev), FP, torch.tensor(lens, dtype=torch.int32, device=dev), mul)
    assert torch.isfinite(xp).all()
    for b, n in enumerate(ns):
        FPb = _roundup4(mel_frames(n, N_FFT, HOP) + K - 1)
        want = _phases(y[b:b + 1, :n].contiguous().to(dev), FPb)
        assert torch.equal(xp[b, :, :FPb], want[0]), (b, n)
        assert (xp[b, :, FPb:] == 0).all(), (b, n)


# ---- 2. the whole mel
_REF = {}


def _reference(case):
    """(y, per item: fp64 oracle mel of the trimmed signal), computed once"""
    if case not in _REF:
        L, mul, lens = CASES[case]
        y = _signal(len(lens), L)
        _REF[case] = (y, [M.mel_spectrogram(y[b:b + 1, :n * mul], *CFG, dtype=torch.float64)[0] for b, n in enumerate(lens)])
    return _REF[case]


@pytest.mark.parametrize('case', list(CASES))
def test_mel_with_lengths_matches_trimmed_items_and_oracle(dev, case):
    L, mul, lens = CASES[case]
    y, oracle = _reference(case)
    ns = [n * mul for n in lens]
    F = mel_frames(L, N_FFT, HOP)
    outs = {}
    for name, val in (('clean', 0.0), ('nan', float('nan')), ('big', 1e30)):
        outs[name] = mel_spectrogram(_poisoned(y, ns, val).to(dev), *CFG, lengths=lens, len_mul=mul)
        assert outs[name].shape == (len(ns), MELS, F) and torch.isfinite(outs[name]).all()
    assert torch.equal(outs['clean'], outs['nan']) and torch.equal(outs['clean'], outs['big'])
    got = outs['nan'].cpu()
    for b, n in enumerate(ns):
        Fb = mel_frames(n, N_FFT, HOP)
        assert oracle[b].shape == (MELS, Fb)
        single = mel_spectrogram(y[b:b + 1, :n].contiguous().to(dev), *CFG).cpu()
        d_single = (got[b, :, :Fb] - single[0]).abs().max().item()
        d_oracle = (got[b, :, :Fb].double() - oracle[b]).abs().max().item()
        print(f'{case} item {b} (n = {n}, {Fb} frames): max |d| vs B = 1 {d_single:.3e}, vs oracle {d_oracle:.3e}')
        assert d_single <= MEL_BAR and d_oracle <= MEL_BAR, (b, n)
        assert (got[b, :, Fb:] == 0).all(), (b, n)                 # exactly 0, not log(1e-5)


def test_mel_lengths_on_the_device_are_used_without_validation(dev):
    """A device tensor is taken as it is (no sync): values past L are clamped by the kernels, a length of at most pad gives an all-zero item."""
    L, mul, lens = CASES['samples']
    y, _ = _reference('samples')
    a = mel_spectrogram(y.to(dev), *CFG, lengths=lens)
    odd = torch.tensor([L + 1000] + lens[1:-1] + [PAD], dtype=torch.int64, device=dev)
    b = mel_spectrogram(y.to(dev), *CFG, lengths=odd)
    assert torch.equal(a[:-1], b[:-1]) and (b[-1] == 0).all()


# ---- 3. full lengths
@pytest.mark.parametrize('L', [4096, 4100])
def test_full_lengths_are_bit_identical_to_no_lengths(dev, L):
    y = _signal(3, L, seed=L).to(dev)
    plain = mel_spectrogram(y, *CFG)
    assert plain.shape == (3, MELS, L // HOP)
    assert torch.equal(plain, mel_spectrogram(y, *CFG, lengths=[L] * 3))
    assert torch.equal(plain, mel_spectrogram(y, *CFG, lengths=torch.full((3,), L, dtype=torch.int32, device=dev)))


# ---- 4. the masked L1
def _l1_bound(want, C, F, B=None):
    units = (C * F + 3) // 4
    G = min(max(-(-units // 1024), 1), 256)
    n64 = 16 * -(-units // (1024 * G)) + 10 + G + 1
    if B is not None:
        n64 += -(-B // 256) + 10
    return want * (2 * U24 + (n64 + 1) * U53 + 4 * U24 * U24)


@pytest.mark.parametrize('shape,mul,lens,frames', [
    ((5, MELS, 17), 1, [4352, 300, 400, 2307, 4096], [17, 0, 1, 9, 16]),        # F % 4 != 0: the element path
    ((3, MELS, 16), 100, [41, 4, 3], [16, 1, 0]),                                # the 16-byte path
])
def test_masked_l1_against_fp64_sums(dev, shape, mul, lens, frames):
    B, C, F = shape
    assert [min(mel_frames(n * mul, N_FFT, HOP), F) for n in lens] == frames
    rng = np.random.default_rng(F)
    a = torch.from_numpy(rng.standard_normal(shape).astype(np.float32) * 3 - 4)            # the range of log-mels
    b = torch.from_numpy(rng.standard_normal(shape).astype(np.float32) * 3 - 4)
    ap, bp = a.clone(), b.clone()
    for i, f in enumerate(frames):                                                         # what must be selected away
        ap[i, :, f:] = float('nan')
        bp[i, :, f:] = 1e30
    total, per = mel_l1(ap.to(dev), bp.to(dev), lens, mul, n_fft=N_FFT, hop_size=HOP)
    total2, per2 = mel_l1(ap.to(dev), bp.to(dev), torch.tensor(lens, device=dev), mul, n_fft=N_FFT, hop_size=HOP)
    assert per.shape == (B,) and total.shape == () and torch.equal(per, per2) and torch.equal(total, total2)   # two runs: the same bits
    assert torch.isfinite(per).all() and torch.isfinite(total)
    S = [(a[i, :, :f].double() - b[i, :, :f].double()).abs().sum().item() for i, f in enumerate(frames)]
    for i, f in enumerate(frames):
        want = S[i] / (C * f) if f else 0.0
        d, bound = abs(per[i].item() - want), _l1_bound(want, C, F)
        print(f'item {i} ({f} frames): |d| = {d:.3e}, bound {bound:.3e}')
        assert d <= bound, (i, f)
    want = sum(S) / (C * sum(frames))
    d, bound = abs(total.item() - want), _l1_bound(want, C, F, B)
    print(f'total: |d| = {d:.3e}, bound {bound:.3e}')
    assert d <= bound
    # an item's bits do not depend on its neighbours: permute the items
    perm = list(range(B))[::-1] if B == 3 else [3, 0, 4, 2, 1]
    _t, per3 = mel_l1(ap[perm].to(dev), bp[perm].to(dev), [lens[i] for i in perm], mul, n_fft=N_FFT, hop_size=HOP)
    assert torch.equal(per3, per[torch.tensor(perm, device=dev)])
    # clean padding: the same bits
    _t, per4 = mel_l1(a.to(dev), b.to(dev), lens, mul, n_fft=N_FFT, hop_size=HOP)
    assert torch.equal(per4, per)


# ---- 5. end to end
def test_mel_errors_batched_is_the_per_utterance_loop(dev):
    """cfg2 generator as tests/test_ragged_gpu.py::_setup.  ns holds no 1 on purpose: one frame is 320 samples <= pad, and the reference
    itself raises there.

    batch = 5 against batch = 1: an utterance's error is a mean of |mel - target| over its elements, and | |x - t| - |x' - t| | <= |x - x'|,
    so two mels that agree within MEL_BAR in every entry give errors within MEL_BAR - the bar of test 2 goes through the L1 unchanged (the
    fp64 sums add 1e-7 relative, see _l1_bound).
    batch = 1 against the written-out loop: lengths = [T] is the plain forward and the plain mel bit for bit (the full-lengths tests), so
    only the L1 differs - the masked kernel's fp64 sum against F.l1_loss's fp32 reduction of N elements, which is within N * 2^-24
    relative of the exact mean whatever its order."""
    T, ns = 16, [16, 2, 7, 13, 5]
    h = synthetic.make_hparams(num_wv_feat=768)
    sd = synthetic.make_state_dict(h, seed=5)
    O.calibrate_running_stats(sd, h, *synthetic.make_inputs(h, 3, 16, seed=1))
    from wavthruvec_pytorch_amd import Generator
    from wavthruvec_pytorch_amd.synthesize import item_noise
    g = Generator(h)
    g.load_state_dict(sd)
    g = g.to(dev).eval()
    x, spk, _nz = synthetic.make_inputs(h, 5, T, seed=9)
    H = synthetic.total_upsample(h)
    feats = [x[b:b + 1, :, :n].contiguous() for b, n in enumerate(ns)]
    spks = [spk[b:b + 1] for b in range(5)]
    frames = [mel_frames(n * H, N_FFT, HOP) for n in ns]
    rng = np.random.default_rng(5)
    y_mels = [torch.from_numpy(rng.standard_normal((f + 2, h.num_mels)).astype(np.float32) * 2 - 5) for f in frames]
    batched = validate.mel_errors(g, feats, spks, y_mels, h, seed=1234, batch=5)
    single = validate.mel_errors(g, feats, spks, y_mels, h, seed=1234, batch=1)
    assert batched.shape == single.shape == (5,)
    nz = item_noise(h.noise_dim, 1234).to(dev)
    for i in range(5):
        with torch.no_grad():
            y_g_hat = g(feats[i].to(dev), spks[i].to(dev), nz)
            y_g_hat_mel = mel_spectrogram(y_g_hat.squeeze(1), h.n_fft, h.num_mels, h.sampling_rate, h.hop_size, h.win_size, h.fmin,
                                          h.fmax_for_loss).permute(0, 2, 1)
            y_mel = y_mels[i][None].to(dev)[:, :y_g_hat_mel.shape[1], :]
            loop = torch.nn.functional.l1_loss(y_mel, y_g_hat_mel).item()
        n_el = y_g_hat_mel.numel()
        print(f'utterance {i} ({ns[i]} frames): batch 5 {batched[i].item():.7f}, batch 1 {single[i].item():.7f}, loop {loop:.7f}')
        assert y_g_hat_mel.shape[1] == frames[i]
        assert abs(batched[i].item() - single[i].item()) <= MEL_BAR, i
        assert abs(single[i].item() - loop) <= (n_el + 3) * U24 * loop, i


# ---- 6. refusals
def test_refusals(dev):
    y = _signal(2, 4100).to(dev)
    with pytest.raises(NotImplementedError):
        mel_spectrogram(y, *CFG, center=True, lengths=[4100, 400])
    with pytest.raises(NotImplementedError):
        mel_spectrogram(y.clone().requires_grad_(), *CFG, lengths=[4100, 400])
    with torch.no_grad():                                   # no-grad: a y that asks for a gradient is served
        assert mel_spectrogram(y.clone().requires_grad_(), *CFG, lengths=[4100, 400]).shape == (2, MELS, 16)
    with pytest.raises(ValueError):
        mel_spectrogram(y, *CFG, lengths=[4100, 0])
    with pytest.raises(ValueError):
        mel_l1(torch.zeros(2, MELS, 16, device=dev), torch.zeros(2, MELS, 15, device=dev), [4100, 400], n_fft=N_FFT, hop_size=HOP)
    with pytest.raises(ValueError):
        mel_l1(torch.zeros(2, MELS, 16, device=dev), torch.zeros(2, MELS, 16, device=dev), [4100], n_fft=N_FFT, hop_size=HOP)
