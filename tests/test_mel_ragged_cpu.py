"""CPU tests of batched validation (mel_spectrogram(lengths=...), mel_l1, validate.mel_errors): the C ABI surface of the new entry points, the
frame-count formula against torch.stft, the host validation of `lengths`, the refusals that need no GPU, and the batching / ordering of
validate.mel_errors with stubs in place of the generator and the two GPU steps.  Nothing is launched."""
import ctypes as C
import os
import re
import types

import pytest
import torch

from wavthruvec_pytorch_amd import _hip, mel, validate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('v2w_mel_phases_len', 'v2w_mel_finish_len', 'v2w_l1_masked')
FAKE = 0x7f0000100000          # 16-byte aligned "device" pointers: the name sink never dereferences them
N_FFT, HOP, MELS = 1024, 256, 80
CFG = (N_FFT, MELS, 16000, HOP, 1024, 0, None)


def test_entry_points_are_declared_bound_and_additive():
    hdr = open(os.path.join(ROOT, 'include', 'vec2wav_hip.h')).read()
    lib = _hip.load()
    assert int(re.search(r'#define V2W_ABI_VERSION (\d+)', hdr).group(1)) == _hip.ABI_VERSION == 35 == lib.v2w_abi_version()
    text = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    for name in NAMES + ('v2w_l1_masked_plan',):
        assert name in _hip.SIGNATURES and re.search(r'\b%s\s*\(' % name, hdr) and hasattr(lib, name) and name in text, name
    assert set(NAMES) <= _hip.LAUNCHERS and 'v2w_l1_masked_plan' not in _hip.LAUNCHERS
    # the plain entry points keep their signatures
    assert len(_hip.SIGNATURES['v2w_mel_phases'][1]) == 8 and len(_hip.SIGNATURES['v2w_mel_finish'][1]) == 10


def test_name_sink_reports_the_kernels_and_the_entry_points_refuse_bad_arguments():
    lib = _hip.load()
    ph = (FAKE, FAKE + (1 << 28), 6, 4100, HOP, 384, 20)
    rc, names = _hip.kernel_names(lib.v2w_mel_phases_len, *ph, FAKE + (2 << 28), 1)
    assert rc in (0, 100) and names == ['mel_phase_len_kernel'], names
    assert _hip.kernel_names(lib.v2w_mel_phases_len, *ph, None, 1) == (_hip.E_ARG, [])
    assert _hip.kernel_names(lib.v2w_mel_phases_len, *ph, FAKE, 0) == (_hip.E_ARG, [])
    assert _hip.kernel_names(lib.v2w_mel_phases_len, FAKE, FAKE, 6, 4100, HOP, 100, 20, FAKE, 1) == (_hip.E_ARG, [])     # 2 pad % hop != 0
    fi = (FAKE, FAKE + (1 << 28), FAKE + (2 << 28), 6, 1088, 20, 16, 513, MELS)
    rc, names = _hip.kernel_names(lib.v2w_mel_finish_len, *fi, FAKE + (3 << 28), 320, HOP, N_FFT)
    assert rc in (0, 100) and names == ['mel_finish_len_kernel'], names
    assert _hip.kernel_names(lib.v2w_mel_finish_len, *fi, None, 1, HOP, N_FFT) == (_hip.E_ARG, [])
    assert _hip.kernel_names(lib.v2w_mel_finish_len, *fi, FAKE, 0, HOP, N_FFT) == (_hip.E_ARG, [])
    assert _hip.kernel_names(lib.v2w_mel_finish_len, *fi, FAKE, 1, HOP, 1000) == (_hip.E_ARG, [])                         # n_fft % hop != 0
    # the masked L1: the 16-byte kernel where F % 4 == 0 on 16-byte aligned pointers, else the element kernel; one finishing launch
    tail = (FAKE + (3 << 28), 1, HOP, N_FFT, FAKE + (4 << 28), FAKE + (5 << 28), FAKE + (6 << 28))
    for F, a, kern in ((16, FAKE, 'l1_masked_kernel<true>'), (17, FAKE, 'l1_masked_kernel<false>'), (16, FAKE + 4, 'l1_masked_kernel<false>')):
        rc, names = _hip.kernel_names(lib.v2w_l1_masked, a, FAKE + (1 << 28), 5, MELS, F, *tail)
        assert rc in (0, 100) and names == [kern, 'l1_masked_finish_kernel'], names
    assert _hip.kernel_names(lib.v2w_l1_masked, FAKE, FAKE, 5, MELS, 16, None, *tail[1:]) == (_hip.E_ARG, [])
    assert _hip.kernel_names(lib.v2w_l1_masked, FAKE, FAKE, 5, MELS, 16, FAKE, 0, *tail[2:]) == (_hip.E_ARG, [])
    assert _hip.kernel_names(lib.v2w_l1_masked, FAKE, FAKE, 5, MELS, 16, *tail[:4], None, None, tail[6]) == (_hip.E_ARG, [])   # nothing to write
    assert _hip.kernel_names(lib.v2w_l1_masked, FAKE, FAKE, 5, MELS, 16, *tail[:6], FAKE + 4) == (_hip.E_ARG, [])             # ws not 8-byte aligned
    assert _hip.kernel_names(lib.v2w_l1_masked, FAKE, FAKE, 5, MELS, 16, *tail[:6], None) == (_hip.E_ARG, [])
    # the plan depends on the shape only: clamp(ceil(ceil(C F / 4) / 1024), 1, 256)
    assert lib.v2w_l1_masked_plan(MELS, 17) == 1 and lib.v2w_l1_masked_plan(MELS, 320) == 7 and lib.v2w_l1_masked_plan(4096, 4096) == 256
    assert lib.v2w_l1_masked_plan(0, 16) == _hip.E_ARG and lib.v2w_l1_masked_plan(1 << 16, 1 << 15) == _hip.E_SHAPE


@pytest.mark.parametrize('n', [385, 640, 1023, 1024, 1025, 4100])
def test_mel_frames_is_torch_stfts_frame_count(n):
    pad = (N_FFT - HOP) // 2
    y = torch.nn.functional.pad(torch.randn(1, 1, n), (pad, pad), mode='reflect').squeeze(1)
    spec = torch.stft(y, N_FFT, hop_length=HOP, win_length=N_FFT, window=torch.hann_window(N_FFT), center=False, return_complex=True)
    assert mel.mel_frames(n, N_FFT, HOP) == spec.shape[-1] == (n + 2 * pad - N_FFT) // HOP + 1 >= 1


def test_mel_frames_is_zero_where_the_reference_raises():
    pad = (N_FFT - HOP) // 2
    assert mel.mel_frames(pad, N_FFT, HOP) == 0 and mel.mel_frames(1, N_FFT, HOP) == 0 and mel.mel_frames(pad + 1, N_FFT, HOP) == 1
    with pytest.raises(RuntimeError):
        torch.nn.functional.pad(torch.randn(1, 1, pad), (pad, pad), mode='reflect')
    # n_fft = 2 hop: more than pad samples, but fewer than one frame needs
    assert mel.mel_frames(200, 512, 256) == 0 and mel.mel_frames(256, 512, 256) == 1


def test_host_validation_of_lengths():
    assert mel.check_lengths([4100, 385, 1], 3, 4100).tolist() == [4100, 385, 1]
    assert mel.check_lengths(torch.tensor([12, 2]), 2, 3840, 320).tolist() == [12, 2]
    for bad in ([4100, 0, 7], [4100, -1, 7], [4101, 5, 7], [5, 7], [1, 2, 3, 4]):
        with pytest.raises(ValueError):
            mel.check_lengths(bad, 3, 4100)
    with pytest.raises(ValueError):
        mel.check_lengths([13, 2], 2, 3840, 320)               # 13 * 320 > L
    with pytest.raises(ValueError):
        mel.check_lengths([12, 2], 2, 3840, 0)
    with pytest.raises(ValueError):
        mel.check_lengths(torch.tensor([1.0, 2.0]), 2, 100)
    with pytest.raises(ValueError):
        mel.check_lengths(torch.tensor([[1, 2]]), 2, 100)
    # through the public call, before anything touches a device
    y = torch.zeros(3, 4100)
    for bad in ([4100, 0, 7], [4101, 5, 7], [5, 7]):
        with pytest.raises(ValueError):
            mel.mel_spectrogram(y, *CFG, lengths=bad)


def test_refusals_that_need_no_gpu():
    y = torch.zeros(2, 4100)
    with pytest.raises(NotImplementedError):
        mel.mel_spectrogram(y, *CFG, center=True, lengths=[4100, 400])
    with pytest.raises(NotImplementedError):
        mel.mel_spectrogram(y.clone().requires_grad_(), *CFG, lengths=[4100, 400])
    with pytest.raises(RuntimeError, match='HIP path only'):
        mel.mel_spectrogram(y, *CFG, lengths=[4100, 400])
    with pytest.raises(RuntimeError, match='HIP path only'):
        mel.mel_l1(torch.zeros(2, 80, 16), torch.zeros(2, 80, 16), [4100, 400], n_fft=N_FFT, hop_size=HOP)
    with pytest.raises(TypeError):
        mel.mel_spectrogram(y, *CFG, False, [4100, 400])       # lengths is keyword-only: the positional signature is the reference's


# ---- validate.mel_errors with stubs
H = types.SimpleNamespace(upsample_rates=(5, 4, 4, 2, 2), noise_dim=4, n_fft=N_FFT, num_mels=3, sampling_rate=16000, hop_size=HOP, win_size=1024,
                          fmin=0, fmax_for_loss=None)
HOP_TOTAL = 320


class _StubGen:
    """y[b, 0, s] = (mean of x[b] over its channels at frame s // 320) + spk[b, 0]; zero past lengths[b] * 320.  Records each call's lengths."""

    def __init__(self):
        self.calls = []
        self._p = torch.nn.Parameter(torch.zeros(1))

    def parameters(self):
        yield self._p

    def __call__(self, x, spk, nz, lengths=None):
        self.calls.append(list(lengths))
        assert nz.shape == (x.shape[0], 4) and torch.equal(nz[0], nz[-1])
        y = x.mean(1, keepdim=True).repeat_interleave(HOP_TOTAL, dim=2) + spk[:, :1, None]
        for b, n in enumerate(lengths):
            y[b, :, n * HOP_TOTAL:] = 0
        return y


def _stub_mel(calls):
    def f(y, n_fft, num_mels, sampling_rate, hop_size, win_size, fmin, fmax, center=False, *, lengths=None, len_mul=1):
        """mel[b, m, f] = (m + 1) * mean of frame f's hop samples; zero past the item's frames."""
        calls.append((list(lengths), len_mul, (n_fft, num_mels, sampling_rate, hop_size, win_size, fmin, fmax)))
        F = mel.mel_frames(y.shape[1], n_fft, hop_size)
        fr = y[:, :F * hop_size].reshape(y.shape[0], F, hop_size).mean(2)
        out = fr[:, None, :] * torch.arange(1, num_mels + 1, dtype=y.dtype)[None, :, None]
        for b, n in enumerate(lengths):
            out[b, :, mel.mel_frames(n * len_mul, n_fft, hop_size):] = 0
        return out
    return f


def _stub_l1(a, b, lengths, len_mul=1, *, n_fft, hop_size):
    fr = [min(mel.mel_frames(n * len_mul, n_fft, hop_size), a.shape[2]) for n in lengths]
    per = torch.stack([(a[i, :, :f] - b[i, :, :f]).abs().mean() for i, f in enumerate(fr)])
    return per.mean(), per


@pytest.mark.parametrize('batch', [1, 2, 8])
def test_mel_errors_batches_by_length_and_answers_in_input_order(monkeypatch, batch):
    calls = []
    monkeypatch.setattr(validate, 'mel_spectrogram', _stub_mel(calls))
    monkeypatch.setattr(validate, 'mel_l1', _stub_l1)
    g = _StubGen()
    ts = [4, 9, 2, 9, 6]
    gen = torch.Generator().manual_seed(3)
    feats = [torch.randn(1, 6, t, generator=gen) for t in ts]
    spks = [torch.randn(1, 5, generator=gen) for _ in ts]
    frames = [t * HOP_TOTAL // HOP for t in ts]
    y_mels = [torch.randn(f + 2, 3, generator=gen) for f in frames]               # the loader's targets run past the generated frames
    errs = validate.mel_errors(g, feats, spks, y_mels, H, seed=7, batch=batch)
    assert errs.shape == (5,) and errs.dtype == torch.float32 and not errs.is_cuda
    # longest first, ties in input order, at most `batch` per forward; a lone item goes through lengths=[T] too
    order = [1, 3, 4, 0, 2]
    want_calls = [[ts[i] for i in order[k:k + batch]] for k in range(0, 5, batch)]
    assert g.calls == want_calls and [c[0] for c in calls] == want_calls
    assert all(c[1] == HOP_TOTAL and c[2] == (N_FFT, 3, 16000, HOP, 1024, 0, None) for c in calls)
    # every utterance's own single run: the target cropped to the generated frames (train.py:273)
    for i, t in enumerate(ts):
        y = feats[i].mean(1).repeat_interleave(HOP_TOTAL, dim=1) + spks[i][:, :1]
        fr = y[:, :frames[i] * HOP].reshape(frames[i], HOP).mean(1)
        m = fr[None, :] * torch.arange(1, 4, dtype=y.dtype)[:, None]
        want = torch.nn.functional.l1_loss(y_mels[i][:frames[i]].t(), m)
        assert abs(errs[i].item() - want.item()) <= 1e-6 * max(1.0, want.item()), i


def test_mel_errors_refuses_mismatched_inputs(monkeypatch):
    monkeypatch.setattr(validate, 'mel_spectrogram', _stub_mel([]))
    monkeypatch.setattr(validate, 'mel_l1', _stub_l1)
    g = _StubGen()
    feats, spks = [torch.randn(1, 6, 4)], [torch.randn(1, 5)]
    with pytest.raises(ValueError):
        validate.mel_errors(g, feats, spks, [], H)
    with pytest.raises(ValueError):
        validate.mel_errors(g, feats, spks, [torch.randn(4, 3)], H)                 # 4 target frames, 5 generated
    with pytest.raises(ValueError):
        validate.mel_errors(g, [torch.randn(1, 6, 1)], spks, [torch.randn(4, 3)], H)  # one latent frame: 320 samples <= pad


def test_pad_targets_crops_transposes_and_zero_pads():
    y_mels = [torch.randn(7, 3), torch.randn(4, 3)]
    tgt = validate.pad_targets(y_mels, [1, 0], [3, 5], 6)
    assert tgt.shape == (2, 3, 6)
    assert torch.equal(tgt[0, :, :3], y_mels[1][:3].t()) and (tgt[0, :, 3:] == 0).all()
    assert torch.equal(tgt[1, :, :5], y_mels[0][:5].t()) and (tgt[1, :, 5:] == 0).all()
