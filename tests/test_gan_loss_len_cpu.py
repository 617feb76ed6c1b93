"""CPU tests of the GAN losses' `lengths=` form: the extent arithmetic of `map_lengths` against real conv shapes, the torch (CPU) path of the
three losses against the fp64 oracle tests/gan_loss_len_ref.py, the argument checks, the C-ABI surface, and `lengths=None` unchanged.

Real shapes.  The 1024-channel CPU discriminators (oracle/disc_oracle.py) are run at a few lengths; for every n in 1 .. 700, 4100 and 8192 the
same torch ops (reflect pad + view, avg_pool1d(4, 2, 2), conv with the layers' k / stride / padding) are run with ONE channel - the sizes
do not depend on the channel count - with the geometry read from the modules' own layers."""
import re
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import gan_loss_len_ref as R
from wavthruvec_pytorch_amd import synthetic

ROOT = Path(__file__).resolve().parents[1]
NS = list(range(1, 701)) + [4100, 8192]


@pytest.fixture(scope='module')
def mods():
    from wavthruvec_pytorch_amd.discriminators import MultiPeriodDiscriminator, MultiScaleDiscriminator
    return SimpleNamespace(mpd=MultiPeriodDiscriminator(SimpleNamespace(periods=synthetic.DEFAULT_PERIODS)), msd=MultiScaleDiscriminator())


def _p_sizes(d, n):
    """Rows of DiscriminatorP's maps on n samples by running one-channel convs, or None when the reflect pad does not fit."""
    p = d.period
    x = torch.zeros(1, 1, n)
    if n % p:
        if p - n % p >= n:
            return None
        x = F.pad(x, (0, p - n % p), 'reflect')
    x = x.view(1, 1, -1, p)
    out = []
    for l in d._layers():
        x = F.conv2d(x, torch.zeros(1, 1, l.k, 1), stride=(l.stride, 1), padding=(l.padding, 0))
        out.append(x.shape[2])
    return out


def _s_sizes(d, n, pools):
    x = torch.zeros(1, 1, n)
    for _ in range(pools):
        x = F.avg_pool1d(x, 4, 2, padding=2)
    out = []
    for l in d._layers():
        x = F.conv1d(x, torch.zeros(1, 1, l.k), stride=l.stride, padding=l.padding)
        out.append(x.shape[2])
    return out


def test_extents_equal_real_conv_shapes(mods):
    unpadded = 0
    for n in NS:
        for d in mods.mpd.discriminators:
            got = d.map_extents(n)
            want = _p_sizes(d, n)
            if want is None:                         # too short for the period's reflect pad: the arithmetic alone
                unpadded += 1
                H = -(-n // d.period)
                chain = [H]
                for _ in range(4):
                    chain.append((chain[-1] - 1) // 3 + 1)
                want = chain[1:] + [chain[-1], chain[-1]]
            assert got == want, (n, d.period)
        for j, d in enumerate(mods.msd.discriminators):
            assert d.map_extents(n, j) == _s_sizes(d, n, j), (n, j)
    assert unpadded > 0


def test_layer_geometry_is_the_issue_statement(mods):
    assert mods.msd.discriminators[0]._chain() == (1, [(15, 1, 7), (41, 2, 20), (41, 2, 20), (41, 4, 20), (41, 4, 20), (41, 1, 20), (5, 1, 2), (3, 1, 1)])
    for d in mods.mpd.discriminators:
        assert d._chain() == (d.period, [(5, 3, 2)] * 4 + [(5, 1, 2), (3, 1, 1)])


@pytest.mark.parametrize('n', [50, 699])
def test_extents_equal_the_oracle_discriminators(mods, n):
    from oracle import disc_oracle as O
    g = torch.Generator().manual_seed(n)
    y = torch.randn(1, 1, n, generator=g)
    sd = synthetic.make_disc_state_dict(synthetic.mpd_state_dict_spec(), seed=3)
    ml = mods.mpd.map_lengths([n])
    rows = ml.maps.tolist()
    i = 0
    with torch.no_grad():
        for k, d in enumerate(mods.mpd.discriminators):
            if d.period - n % d.period >= n and n % d.period:
                i += 6
                continue
            score, fmap = O.disc_p(y, sd, f'discriminators.{k}', d.period)
            for f in fmap:
                assert rows[i] == [f.shape[2] * f.shape[3]], (k, i)
                i += 1
            assert ml.scores.tolist()[k] == [score.shape[1]]
        sd = synthetic.make_disc_state_dict(synthetic.msd_state_dict_spec(), seed=3)
        y_r, _g, f_r, _fg = O.msd_forward(sd, y, y, training=False)
    ml = mods.msd.map_lengths([n])
    assert ml.maps.tolist() == [[f.shape[2]] for maps in f_r for f in maps]
    assert ml.scores.tolist() == [[s.shape[1]] for s in y_r]
    assert ml.scores_twice.tolist() == ml.scores.tolist() * 2 and ml.B == 1 and ml.table.dtype == torch.int32


def test_zero_monotone_clip_and_len_mul(mods):
    for d in mods.mpd.discriminators:
        assert d.map_extents(0) == [0] * 6
    for j, d in enumerate(mods.msd.discriminators):
        assert d.map_extents(0, j) == [0] * 8
    prev = None
    for n in range(0, 1200):
        cur = [d.map_extents(n) for d in mods.mpd.discriminators] + [d.map_extents(n, j) for j, d in enumerate(mods.msd.discriminators)]
        if prev is not None:
            assert all(c >= p for cs, ps in zip(cur, prev) for c, p in zip(cs, ps)), n
        prev = cur
    for m in (mods.mpd, mods.msd):
        assert torch.equal(m.map_lengths([13, 7], len_mul=320).table, m.map_lengths([13 * 320, 7 * 320]).table)
        full = m.map_lengths([4100], L=4100).table
        assert int(m.map_lengths([9000]).table.min()) >= int(full.max() >= 0) and (m.map_lengths([9000]).table >= full).all()
        assert torch.equal(m.map_lengths(torch.tensor([4100])).table, full)
        with pytest.raises(ValueError):
            m.map_lengths([4101], L=4100)                                                     # a list is validated (mel.check_lengths)
        with pytest.raises(ValueError):
            m.map_lengths([0])
    # the period is folded into the table: floats per row
    d = mods.mpd.discriminators[2]
    assert mods.mpd.map_lengths([501]).maps[12:18, 0].tolist() == [e * d.period for e in d.map_extents(501)]


def _fake_outputs(B, seed, sizes):
    """Random (scores, fmaps) shaped like a discriminator's, with a few channels: sizes[d] = (inner, [rows of each map])."""
    g = torch.Generator().manual_seed(seed)
    scores, fmaps = [], []
    for inner, rows in sizes:
        maps = [torch.randn((B, 3, r, inner) if inner > 1 else (B, 3, r), generator=g) for r in rows[:-1]]
        maps.append(torch.randn((B, 1, rows[-1], inner) if inner > 1 else (B, 1, rows[-1]), generator=g))
        fmaps.append(maps)
        scores.append(torch.flatten(maps[-1], 1, -1))
    return scores, fmaps


@pytest.mark.parametrize('kind', ['mpd', 'msd'])
def test_cpu_losses_equal_the_oracle(mods, kind):
    from wavthruvec_pytorch_amd import discriminators as D
    m = getattr(mods, kind)
    L, lens = 1000, [1000, 613, 40]
    discs = list(m.discriminators)
    sizes = [(getattr(d, 'period', 1), d.map_extents(L, j if kind == 'msd' else 0)) for j, d in enumerate(discs)]
    s_r, f_r = _fake_outputs(3, 1, sizes)
    s_g, f_g = _fake_outputs(3, 2, sizes)
    f_g = [[f.requires_grad_() for f in maps] for maps in f_g]
    ml = m.map_lengths(lens, L=L)
    assert ml.table.device.type == 'cpu' and int(ml.maps.max()) <= L
    ext = ml.maps.numpy()
    feat = D.feature_loss(f_r, f_g, lengths=ml)
    pairs = [(r, f) for mr, mg in zip(f_r, f_g) for r, f in zip(mr, mg)]
    want = 2 * sum(R.l1_term(r.detach().numpy(), f.detach().numpy(), ext[i]) for i, (r, f) in enumerate(pairs))
    assert abs(feat.item() - want) <= 1e-6 * want
    feat.backward()
    for i, (r, f) in enumerate(pairs):
        wd, on = R.l1_grad(f.detach().numpy(), r.numpy(), ext[i], 2.0)
        assert np.abs(f.grad.numpy() - wd).max() <= 1e-6 * np.abs(wd).max()
        assert (f.grad.numpy()[~on] == 0).all()
    assert not R.counted(ext[0], *R.as_rows(pairs[0][0].numpy(), 3).shape)[0].all()
    sext = ml.scores.numpy()
    s_g = [s.detach() for s in s_g]
    gen, gterms = D.generator_loss(s_g, lengths=ml)
    wterms = [R.lsgan_term(s.numpy(), 1.0, sext[i]) for i, s in enumerate(s_g)]
    assert all(abs(t.item() - w) <= 1e-6 * w for t, w in zip(gterms, wterms)) and abs(gen.item() - sum(wterms)) <= 1e-6 * sum(wterms)
    disc, rt, ft = D.discriminator_loss(s_r, s_g, lengths=ml)
    wr = [R.lsgan_term(s.numpy(), 1.0, sext[i]) for i, s in enumerate(s_r)]
    wf = [R.lsgan_term(s.numpy(), 0.0, sext[i]) for i, s in enumerate(s_g)]
    assert all(isinstance(t, float) and abs(t - w) <= 1e-6 * w for t, w in zip(rt + ft, wr + wf))
    assert abs(disc.item() - sum(wr + wf)) <= 1e-6 * sum(wr + wf)
    # the masked means differ from the dense ones: the lengths are seen
    assert abs(D.feature_loss(f_r, f_g).item() - feat.item()) > 1e-4


def test_mismatched_map_lengths_raise(mods):
    from wavthruvec_pytorch_amd import discriminators as D
    sizes = [(getattr(d, 'period', 1), d.map_extents(600)) for d in mods.mpd.discriminators]
    s, f = _fake_outputs(2, 5, sizes)
    good, wrong_b, other = mods.mpd.map_lengths([600, 300]), mods.mpd.map_lengths([600, 300, 200]), mods.msd.map_lengths([600, 300])
    D.feature_loss(f, f, lengths=good)
    for bad in (wrong_b, other):                     # another batch; another number of maps (MSD: 24 for MPD's 18)
        with pytest.raises(ValueError):
            D.feature_loss(f, f, lengths=bad)
    with pytest.raises(ValueError):
        D.generator_loss(s, lengths=wrong_b)
    with pytest.raises(ValueError):
        D.discriminator_loss(s, s, lengths=wrong_b)
    with pytest.raises(ValueError):
        D.generator_loss(s[:2], lengths=good)
    with pytest.raises(ValueError):
        D.discriminator_loss(s[:2], s, lengths=good)
    with pytest.raises(ValueError):
        D.feature_loss(f[:2], f[:2], lengths=good)
    with pytest.raises(TypeError):
        D.generator_loss(s, lengths=[600, 300])


def test_lengths_none_is_the_torch_expression(mods):
    from wavthruvec_pytorch_amd import discriminators as D
    sizes = [(1, d.map_extents(500, j)) for j, d in enumerate(mods.msd.discriminators)]
    s_r, f_r = _fake_outputs(2, 7, sizes)
    s_g, f_g = _fake_outputs(2, 8, sizes)
    assert torch.equal(D.feature_loss(f_r, f_g), 2 * sum(torch.mean(torch.abs(r - f)) for mr, mg in zip(f_r, f_g) for r, f in zip(mr, mg)))
    assert torch.equal(D.feature_loss(f_r, f_g, None), D.feature_loss(f_r, f_g))
    over = mods.msd.map_lengths([9000, 9000])                    # extents past the maps' sizes are clipped to them: the dense value
    assert abs(D.feature_loss(f_r, f_g, lengths=over).item() - D.feature_loss(f_r, f_g).item()) <= 1e-6 * D.feature_loss(f_r, f_g).item()
    gen, terms = D.generator_loss(s_g)
    assert torch.equal(gen, sum(torch.mean((1 - s) ** 2) for s in s_g)) and len(terms) == 3
    disc, rt, ft = D.discriminator_loss(s_r, s_g, lengths=None)
    assert torch.equal(disc, sum(torch.mean((1 - r) ** 2) + torch.mean(g ** 2) for r, g in zip(s_r, s_g)))
    assert rt == [torch.mean((1 - r) ** 2).item() for r in s_r] and ft == [torch.mean(g ** 2).item() for g in s_g]


def test_mask_tail_cpu():
    from wavthruvec_pytorch_amd import mask_tail
    y = torch.randn(2, 1, 10, generator=torch.Generator().manual_seed(0))
    y[1, 0, 7] = float('nan')
    out = mask_tail(y, [5, 3], len_mul=2)
    assert torch.equal(out[0], y[0]) and torch.equal(out[1, 0, :6], y[1, 0, :6]) and (out[1, 0, 6:] == 0).all()
    assert not torch.signbit(out[1, 0, 6:]).any()


def test_len_symbols_and_header():
    from wavthruvec_pytorch_amd import _hip
    lib = _hip.load()
    hdr = (ROOT / 'include' / 'vec2wav_hip.h').read_text()
    integ = (ROOT / 'INTEGRATION.md').read_text()
    for name in ('v2w_l1_mean_multi_len', 'v2w_l1_mean_multi_len_bwd', 'v2w_lsgan_multi_len', 'v2w_lsgan_multi_len_bwd', 'v2w_map_extents',
                 'v2w_mask_tail'):
        assert name in _hip.SIGNATURES and getattr(lib, name) is not None
        assert re.search(r'\b%s\(' % name, hdr) and name in integ, name
    # argument checks that need no GPU: nothing is launched before they fail
    import ctypes as C
    pairs = (_hip.L1Pair * 1)()
    pairs[0].a = pairs[0].b = 64
    pairs[0].rows, pairs[0].valid = 6, 5
    assert lib.v2w_l1_mean_multi_len(pairs, 1, None, 3, 1.0, 64, 64, 64, None) == _hip.E_ARG           # no table
    assert lib.v2w_l1_mean_multi_len(pairs, 1, 64, 4, 1.0, 64, 64, 64, None) == _hip.E_ARG             # rows % B
    assert lib.v2w_l1_mean_multi_len(pairs, 1, 64, 0, 1.0, 64, 64, 64, None) == _hip.E_ARG
    items = (_hip.LsganItem * 1)()
    items[0].s, items[0].rows, items[0].valid, items[0].target = 64, 6, 5, 1.0
    assert lib.v2w_lsgan_multi_len(items, 1, 64, 4, 64, 64, None) == _hip.E_ARG
    assert lib.v2w_mask_tail(64, 64, 6, 4, 8, 64, 1, None) == _hip.E_ARG
    assert lib.v2w_map_extents(64, 0, 8, 2, 64, 1, 64, 1, 64, None) == _hip.E_ARG
    starts = (C.c_int32 * 2)()
    assert lib.v2w_l1_multi_plan(pairs, 1, starts) == 1                                                # the plan of the _len call is the dense one
