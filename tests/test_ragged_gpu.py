"""GPU tests of per-item valid lengths (ABI v36; Generator.forward(lengths=...)): every length-aware kernel against B = 1 launches on the
trimmed input, the generator against its own B = 1 forward and the oracle, poisoned padding, the launch plan, the refusals and synthesize."""
import os

import numpy as np
import pytest
import torch

from oracle import vec2wav_oracle as O
from wavthruvec_pytorch_amd import hipops, synthetic

pytestmark = pytest.mark.gpu
LRELU = 0.1


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a MI355X'
    return torch.device('cuda:0')


def _lens(ns, dev):
    return torch.tensor(ns, dtype=torch.int32, device=dev)


def _poisoned(x, ns, val=float('nan')):
    x = x.clone()
    for b, n in enumerate(ns):
        x[b, :, n:] = val
    return x


def _close(got, want, tol=1e-5):
    assert torch.isfinite(got).all()
    d = (got - want).abs().max().item()
    assert d <= tol * max(1.0, want.abs().max().item()), d


# ---- kernel level -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('B,ci,co,L,k,dil,ns,split', [
    (6, 64, 128, 67, 7, 1, [67, 1, 5, 14, 27, 66], False),        # conv_tile, unaligned L (element-wise staging)
    (6, 128, 128, 96, 11, 3, [96, 1, 6, 15, 29, 95], False),     # float4 staging, every residue mod 4, residual
    (2, 512, 512, 64, 7, 1, [64, 13], True),                     # small grid: split over C_in (partial + reduce)
])
def test_conv1d_with_lengths_matches_trimmed_launches(dev, B, ci, co, L, k, dil, ns, split):
    g = torch.Generator().manual_seed(L + k)
    x = torch.randn((B, ci, L), generator=g).to(dev)
    wf = (torch.randn((k, ci, co), generator=g) / (ci * k) ** 0.5).to(dev)
    bias = torch.randn((co,), generator=g).to(dev)
    aff = (torch.rand((B, ci), generator=g).to(dev) + 0.5, torch.randn((B, ci), generator=g).to(dev))
    wp = hipops.pack_mfma(wf)
    slab = hipops.SplitKSlab()
    out = torch.full((B, co, L), 7.0, device=dev)
    res = ci == co                       # (the residual: C_in == C_out only)
    hipops.conv1d(_poisoned(x, ns), wf, bias, out, k=k, dil=dil, slope=LRELU, in_affine=aff, res=x if res else None,
                  res_affine=aff if res else None, wp=wp, splitk_ws=slab if split else None, lengths=_lens(ns, dev), len_mul=1)
    if split:
        assert slab.t is not None            # the split over C_in ran
    for b, n in enumerate(ns):
        xb = x[b:b + 1, :, :n].contiguous()
        ob = torch.empty((1, co, n), device=dev)
        ab = (aff[0][b:b + 1], aff[1][b:b + 1])
        hipops.conv1d(xb, wf, bias, ob, k=k, dil=dil, slope=LRELU, in_affine=ab, res=xb if res else None, res_affine=ab if res else None, wp=wp)
        _close(out[b:b + 1, :, :n], ob)


def test_wino_with_lengths_matches_trimmed_launches(dev):
    B, C, L, k, dil = 8, 256, 520, 7, 3              # (160 workgroups: the Winograd kernel takes launches of more than 128)
    ns = [520, 1, 6, 13, 36, 71, 128, 519]            # every residue mod 4 and mod 6
    g = torch.Generator().manual_seed(3)
    x = torch.randn((B, C, L), generator=g).to(dev)
    wf = (torch.randn((k, C, C), generator=g) / (C * k) ** 0.5).to(dev)
    bias = torch.randn((C,), generator=g).to(dev)
    wp, wpw = hipops.pack_mfma(wf), hipops.pack_wino(wf)
    out = torch.full((B, C, L), 7.0, device=dev)
    hipops.conv1d(_poisoned(x, ns), wf, bias, out, k=k, dil=dil, slope=LRELU, res=x, algo=hipops.ALGO_WINO, wp=wpw,
                  lengths=_lens(ns, dev))
    for b, n in enumerate(ns):
        xb = x[b:b + 1, :, :n].contiguous()
        ob = torch.empty((1, C, n), device=dev)
        hipops.conv1d(xb, wf, bias, ob, k=k, dil=dil, slope=LRELU, res=xb, wp=wp)
        _close(out[b:b + 1, :, :n], ob)


@pytest.mark.parametrize('ci,co,k,u,mul', [(512, 256, 11, 5, 1), (256, 128, 8, 4, 5), (64, 32, 4, 2, 3)])
def test_convt_with_lengths_matches_trimmed_launches(dev, ci, co, k, u, mul):
    B, L = 5, 40 * mul
    ns = [40, 1, 7, 14, 39]
    g = torch.Generator().manual_seed(u)
    x = torch.randn((B, ci, L), generator=g).to(dev)
    wf = (torch.randn((k, ci, co), generator=g) / ci ** 0.5).to(dev)
    bias = torch.randn((co,), generator=g).to(dev)
    wp = hipops.pack_mfma(wf, u=u)
    out = torch.full((B, co, L * u), 7.0, device=dev)
    hipops.convt1d(_poisoned(x, [n * mul for n in ns]), wf, bias, out, k=k, u=u, slope=LRELU, wp=wp, lengths=_lens(ns, dev), len_mul=mul)
    for b, n in enumerate(ns):
        xb = x[b:b + 1, :, :n * mul].contiguous()
        ob = torch.empty((1, co, n * mul * u), device=dev)
        hipops.convt1d(xb, wf, bias, ob, k=k, u=u, slope=LRELU, wp=wp)
        _close(out[b:b + 1, :, :n * mul * u], ob)


@pytest.mark.parametrize('C,post', [(32, False), (16, False), (16, True)])
def test_stage_with_lengths_matches_trimmed_launches(dev, C, post):
    B, mul = 5, 4
    ns = [96, 1, 7, 13, 93]
    L = 96 * mul
    g = torch.Generator().manual_seed(C + post)
    x = torch.randn((B, C, L), generator=g).to(dev)
    aff = (torch.rand((B, C), generator=g).to(dev) + 0.5, torch.randn((B, C), generator=g).to(dev))
    brs = []
    for k in (3, 7, 11):
        w1, w2 = [(torch.randn((k, C, C), generator=g) / (C * k) ** 0.5).to(dev) for _ in range(2)]
        brs.append(dict(wp1=hipops.pack_mfma(w1), b1=torch.randn((C,), generator=g).to(dev), wp2=hipops.pack_mfma(w2),
                        b2=torch.randn((C,), generator=g).to(dev), k=k, dil1=1, dil2=3))
    pw = torch.randn((7, C, 1), generator=g).to(dev) / C ** 0.5
    pb = torch.randn((1,), generator=g).to(dev)

    def run(xx, a, n_len, Lx):
        Bx = xx.shape[0]
        y = torch.full((Bx, 1, Lx), 7.0, device=dev) if post else None
        o = None if post else torch.full((Bx, C, Lx), 7.0, device=dev)
        assert hipops.resblock2_stage(xx, a, brs, o, slope=LRELU, out_div=3.0, post=(pw, pb, y, 7, 0.01) if post else None,
                                      **(dict(lengths=_lens(n_len, dev), len_mul=mul) if n_len is not None else {}))
        return y if post else o

    got = run(_poisoned(x, [n * mul for n in ns]), aff, ns, L)
    for b, n in enumerate(ns):
        want = run(x[b:b + 1, :, :n * mul].contiguous(), (aff[0][b:b + 1], aff[1][b:b + 1]), None, n * mul)
        _close(got[b:b + 1, :, :n * mul], want)
        if post:
            assert (got[b, :, n * mul:] == 0).all()


def test_conv_post_with_lengths(dev):
    B, C, L = 4, 16, 203
    ns = [203, 1, 50, 101]
    g = torch.Generator().manual_seed(11)
    x = torch.randn((B, C, L), generator=g).to(dev)
    wf = torch.randn((7, C, 1), generator=g).to(dev) / 4
    bias = torch.randn((1,), generator=g).to(dev)
    y = torch.full((B, 1, L), 7.0, device=dev)
    hipops.conv_post_tanh(_poisoned(x, ns), wf, bias, y, k=7, slope=0.01, lengths=_lens(ns, dev))
    for b, n in enumerate(ns):
        yb = torch.empty((1, 1, n), device=dev)
        hipops.conv_post_tanh(x[b:b + 1, :, :n].contiguous(), wf, bias, yb, k=7, slope=0.01)
        _close(y[b:b + 1, :, :n], yb)
        assert (y[b, :, n:] == 0).all()


# ---- generator level ----------------------------------------------------------------------------------------------------------------
_CFG = {'cfg2': dict(num_wv_feat=768), 'cfg5': dict(num_wv_feat=1024, upsample_rates=[8, 5, 4, 2, 2], upsample_kernel_sizes=[16, 11, 8, 4, 4])}
_GEN = {}


def _setup(name, dev, T=16):
    if name not in _GEN:
        h = synthetic.make_hparams(**_CFG[name])
        sd = synthetic.make_state_dict(h, seed=5)
        O.calibrate_running_stats(sd, h, *synthetic.make_inputs(h, 3, 16, seed=1))
        from wavthruvec_pytorch_amd import Generator
        g = Generator(h)
        g.load_state_dict(sd)
        g = g.to(dev).eval()
        _GEN[name] = (h, sd, g)
    h, sd, g = _GEN[name]
    x, spk, nz = synthetic.make_inputs(h, 5, T, seed=9)
    return h, sd, g, x, spk, nz


@pytest.mark.parametrize('name,wino,fuse_post', [('cfg2', True, True), ('cfg2', False, True), ('cfg2', True, False), ('cfg5', True, True),
                                                 ('cfg5', False, True)])
def test_generator_ragged_batch_matches_single_forwards_and_oracle(dev, name, wino, fuse_post):
    T = 16
    h, sd, g, x, spk, nz = _setup(name, dev, T)
    H = synthetic.total_upsample(h)
    ns = [T, 1, 7, 13, T - 3]
    g.wino, g.fuse_post = wino, fuse_post
    try:
        with torch.no_grad():
            y = g(_poisoned(x, ns).to(dev), spk.to(dev), nz.to(dev), lengths=ns).cpu()
            assert y.shape == (5, 1, T * H)
            for b, n in enumerate(ns):
                xb, sb, nb = x[b:b + 1, :, :n].contiguous(), spk[b:b + 1], nz[b:b + 1]
                yb = g(xb.to(dev), sb.to(dev), nb.to(dev)).cpu()
                _close(y[b:b + 1, :, :n * H], yb, 1e-5)
                assert (y[b, :, n * H:] == 0).all()
                if wino and fuse_post or b == 2:
                    want, _ = O.generator_forward({k: v.clone() for k, v in sd.items()}, h, xb, sb, nb, training=False)
                    assert (y[b:b + 1, :, :n * H] - want).abs().max().item() <= 1e-4
    finally:
        g.wino, g.fuse_post = True, True


@pytest.mark.parametrize('val', [float('nan'), 1e30])
def test_generator_poisoned_padding_has_no_effect(dev, val):
    h, sd, g, x, spk, nz = _setup('cfg2', dev)
    H = synthetic.total_upsample(h)
    ns = [16, 3, 9, 12, 5]
    with torch.no_grad():
        clean = g(_poisoned(x, ns, 0.0).to(dev), spk.to(dev), nz.to(dev), lengths=ns)
        dirty = g(_poisoned(x, ns, val).to(dev), spk.to(dev), nz.to(dev), lengths=ns)
    assert torch.isfinite(dirty).all() and torch.equal(clean, dirty)
    for b, n in enumerate(ns):
        assert (dirty[b, :, n * H:] == 0).all()


def test_generator_full_lengths_are_bit_identical_to_no_lengths(dev):
    h, sd, g, x, spk, nz = _setup('cfg2', dev)
    with torch.no_grad():
        y0 = g(x.to(dev), spk.to(dev), nz.to(dev))
        y1 = g(x.to(dev), spk.to(dev), nz.to(dev), lengths=torch.full((5,), x.shape[2], dtype=torch.int64, device=dev))
    assert torch.equal(y0, y1)


def test_generator_lengths_replay_one_tape(dev):
    h, sd, g, x, spk, nz = _setup('cfg2', dev, T=20)
    H = synthetic.total_upsample(h)
    g._tapes.clear()
    outs = []
    with torch.no_grad():
        for ns in ([20, 4, 11, 17, 2], [3, 20, 9, 1, 14]):
            outs.append((ns, g(_poisoned(x, ns).to(dev), spk.to(dev), nz.to(dev), lengths=ns).cpu()))
        assert len([k for k in g._tapes if k[-1] == 'lengths']) == 1
        for ns, y in outs:
            for b, n in enumerate(ns):
                yb = g(x[b:b + 1, :, :n].to(dev), spk[b:b + 1].to(dev), nz[b:b + 1].to(dev)).cpu()
                _close(y[b:b + 1, :, :n * H], yb)
                assert (y[b, :, n * H:] == 0).all()


def test_generator_lengths_refusals(dev):
    h, sd, g, x, spk, nz = _setup('cfg2', dev)
    args = (x.to(dev), spk.to(dev), nz.to(dev))
    ns = [16, 3, 9, 12, 5]
    g.train()
    try:
        with pytest.raises(ValueError), torch.no_grad():
            g(*args, lengths=ns)
    finally:
        g.eval()
    with pytest.raises(NotImplementedError):
        g(x.to(dev).requires_grad_(), spk.to(dev), nz.to(dev), lengths=ns)
    for prec in ('bf16', 'f16x3'):
        g.precision = prec
        try:
            with pytest.raises(NotImplementedError), torch.no_grad():
                g(*args, lengths=ns)
        finally:
            g.precision = 'f32'
    g.algo = hipops.ALGO_DIRECT
    try:
        with pytest.raises(NotImplementedError), torch.no_grad():
            g(*args, lengths=ns)
    finally:
        g.algo = hipops.ALGO_AUTO
    with pytest.raises(ValueError), torch.no_grad():
        g(*args, lengths=[16, 0, 9, 12, 5])
    from wavthruvec_pytorch_amd import Generator
    h1 = synthetic.make_hparams(num_wv_feat=64, resblock='1')
    g1 = Generator(h1).to(dev).eval()
    x1, s1, n1 = synthetic.make_inputs(h1, 2, 8, seed=1)
    with pytest.raises(NotImplementedError), torch.no_grad():
        g1(x1.to(dev), s1.to(dev), n1.to(dev), lengths=[8, 3])


def test_synthesize_batched_run_writes_the_single_runs(dev, tmp_path):
    import wave
    from wavthruvec_pytorch_amd import synthesize
    h, sd, g, x, spk, nz = _setup('cfg2', dev)
    ck = tmp_path / 'g_00000001'
    torch.save({'generator': {k: v.clone() for k, v in sd.items()}}, ck)
    feats = []
    for i, t in enumerate((9, 16, 5)):
        f = tmp_path / f'u{i}.npy'
        np.save(f, x[i, :, :t].T.numpy()[None])
        feats.append(str(f))
    se = tmp_path / 's.pth'
    torch.save(spk[0].reshape(1, 1, -1).clone(), se)
    base = ['--checkpoint', str(ck), '--spk-emb', str(se), '--device', str(dev)]
    assert synthesize.main(base + ['--feat'] + feats + ['--out', str(tmp_path / 'batched'), '--batch', '3']) == 0
    for i, f in enumerate(feats):
        assert synthesize.main(base + ['--feat', f, '--out', str(tmp_path / f'single{i}.wav')]) == 0

    def read(p):
        with wave.open(str(p)) as w:
            return np.frombuffer(w.readframes(w.getnframes()), dtype='<i2').astype(np.int32)
    for i in range(3):
        a, b = read(tmp_path / 'batched' / f'u{i}.wav'), read(tmp_path / f'single{i}.wav')
        assert a.shape == b.shape and np.abs(a - b).max() <= 1       # 16-bit PCM of samples within 1e-5
    # the samples themselves, before the PCM rounding
    feats_t = [synthesize.load_latents(f) for f in feats]
    spk_t = [spk[0:1]] * 3
    ys = synthesize.synthesize_many(g, feats_t, spk_t, seed=1234, batch=3)
    for f, yb in zip(feats_t, ys):
        ref = synthesize.synthesize(g, f, spk[0:1], seed=1234)
        assert yb.shape == ref.shape
        _close(yb.cpu(), ref.cpu())
