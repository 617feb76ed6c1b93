"""GPU tests of the GAN loss kernels over a padded batch (v2w_l1_mean_multi_len / v2w_lsgan_multi_len and their backwards, v2w_map_extents,
v2w_mask_tail) and of `feature_loss` / `discriminator_loss` / `generator_loss` with `lengths=`, against the fp64 oracle
tests/gan_loss_len_ref.py on the same float32 inputs.

Bounds: those of tests/test_losses_gpu.py - the per-element arithmetic is the dense kernels', only the count differs.  Terms and totals
1e-6 relative (a few fp32 roundings per summand, fp64 sums, one rounding to fp32); the L1 gradient is sgn(a - b) times the correctly rounded
fp32 quotient (scale * gout) / den and is compared bit for bit; the LSGAN gradient 1e-6 of its largest entry.  A B = 1 call on one item
against the same item inside a batch whose other extents are 0 adds the same fp64 summands in another order before the one rounding to
fp32: one fp32 ulp (2^-23 relative)."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import gan_loss_len_ref as R
from wavthruvec_pytorch_amd import synthetic

pytestmark = pytest.mark.gpu
RTOL = 1e-6
B = 3
VALIDS = (1, 3, 4, 5, 37, 2051)
NAN, INF = float('nan'), float('inf')


@pytest.fixture(scope='module')
def dev():
    from wavthruvec_pytorch_amd import _hip
    _hip.load()
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def _rel(got, want):
    got, want = (float(v.detach()) if torch.is_tensor(v) else float(v) for v in (got, want))
    return abs(got - want) / max(abs(want), 1e-30)


def _tensor(shape, view, g, dev):
    """A float32 GPU tensor of `shape` (B, C, U[, inner]): 'dense'; 'pitched' - a view of (B, C, roundup4(V) + 4) rows whose tails are NaN;
    'off1' .. 'off3' - dense, its first float 1 - 3 floats past a 16-byte line; 'lo' / 'hi' - a leading-dim half of a pitched 2B tensor."""
    V = int(np.prod(shape[2:]))
    if view == 'dense':
        return torch.randn(shape, generator=g).to(dev)
    if view.startswith('off'):
        k = int(view[3])
        return torch.randn(int(np.prod(shape)) + k, generator=g).to(dev)[k:].view(shape)
    lead = shape[0] * (2 if view in ('lo', 'hi') else 1)
    pitch = (V + 3) // 4 * 4 + 4
    buf = torch.full((lead, shape[1], pitch), NAN)
    buf[:, :, :V] = torch.randn((lead, shape[1], V), generator=g)
    t = buf.to(dev)[:, :, :V]
    t = t.view(lead, shape[1], *shape[2:]) if len(shape) == 4 else t
    return t[:shape[0]] if view == 'lo' else (t[shape[0]:] if view == 'hi' else t)


def _extents(i, U):
    """Rows that count per item, cycling: 0 and 1 and all; one item at 0; all full; all 0; past the map (clamped); a middle value."""
    return [[0, 1, U], [U, 0, max(U // 2, 1)], [U, U, U], [0, 0, 0], [U + 5, 1, 0], [max(U - 1, 0), U, 1]][i % 6]


@pytest.fixture(scope='module')
def case(dev):
    """64 descriptors: every valid x C in {1, 4} x a view, inner 1 or 3, the extent patterns cycling; fp64 copies; computed once."""
    g = torch.Generator().manual_seed(4321)
    views = ['dense', 'pitched', 'off1', 'lo', 'off2', 'hi', 'off3', 'pitched']
    pairs, ext, inner = [], [], []
    i = 0
    for U in VALIDS:
        for C in (1, 4):
            for rep in range(5 if U < 37 else 6):
                if len(pairs) == 64:
                    break
                inn = 3 if i % 4 == 3 else 1
                shape = (B, C, U, inn) if inn == 3 else (B, C, U)
                va, vb = views[i % 8], views[(i + (3 if rep % 2 else 0)) % 8]       # the two sides in the same or in different forms
                a, b = _tensor(shape, va, g, dev), _tensor(shape, vb, g, dev)
                a[..., ::7] = b[..., ::7]                                           # planted ties
                pairs.append((a, b))
                ext.append([e * inn for e in _extents(i, U)])
                inner.append(inn)
                i += 1
    assert len(pairs) == 64
    ext_t = torch.tensor(ext, dtype=torch.int32, device=dev)
    ref = [(a.cpu().numpy(), b.cpu().numpy()) for a, b in pairs]
    assert all(np.isfinite(a).all() and np.isfinite(b).all() for a, b in ref)
    terms = [R.l1_term(a, b, e) for (a, b), e in zip(ref, ext)]
    return SimpleNamespace(pairs=pairs, ext=ext, ext_t=ext_t, ref=ref, terms=terms, inner=inner)


def _copy(t):
    """A copy of t with t's strides (a pitched view stays pitched)."""
    p = torch.empty_strided(t.shape, t.stride(), dtype=t.dtype, device=t.device)
    p.copy_(t)
    return p


def _rows(t):
    """(B, C, V) view of a (B, C, ...) map or a (B, N) score."""
    flat = t.reshape(t.shape[0], 1, -1) if t.dim() == 2 else t.flatten(2)
    assert flat.data_ptr() == t.data_ptr() and flat.numel() == t.numel()
    return flat


def _poisoned(t, e, value):
    """A copy of t (same strides) with `value` on every float that does not count."""
    p = _copy(t)
    flat = _rows(p)
    for b in range(t.shape[0]):
        flat[b, :, max(min(e[b], flat.shape[2]), 0):] = value
    return p


def test_l1_len_matches_fp64_and_is_deterministic(dev, case):
    from wavthruvec_pytorch_amd import hipops
    for a, b in case.pairs:                                           # every view goes through without a copy
        assert hipops.loss_rows_len(a, B) is not None and hipops.loss_rows_len(b, B) is not None
    terms, total = hipops.l1_mean_multi(case.pairs, 2.0, ext=case.ext_t)
    terms2, total2 = hipops.l1_mean_multi(case.pairs, 2.0, ext=case.ext_t)
    torch.cuda.synchronize()
    assert torch.isfinite(terms).all() and torch.isfinite(total)
    worst = 0.0
    for i, (got, want) in enumerate(zip(terms.tolist(), case.terms)):
        if want == 0.0:
            assert got == 0.0, i
            continue
        worst = max(worst, _rel(got, want))
        assert _rel(got, want) <= RTOL, (i, got, want)
    print(f'[l1 len] 64 terms: worst rel {worst:.2e}; total rel {_rel(total, 2.0 * sum(case.terms)):.2e}')
    assert _rel(total, 2.0 * sum(case.terms)) <= RTOL
    assert sum(t == 0.0 for t in case.terms) >= 5                     # the all-zero descriptors are there
    assert torch.equal(terms, terms2) and torch.equal(total, total2)


def test_l1_len_poison_past_the_extents(dev, case):
    from wavthruvec_pytorch_amd import hipops
    gout = torch.tensor(0.37, device=dev)
    want = hipops.l1_mean_multi(case.pairs, 2.0, ext=case.ext_t)
    want_d = hipops.l1_mean_multi_bwd(case.pairs, 2.0, gout, ext=case.ext_t)
    for value in (NAN, INF):
        pois = [(_poisoned(a, e, value), _poisoned(b, e, -value)) for (a, b), e in zip(case.pairs, case.ext)]
        assert sum(int((~torch.isfinite(a)).sum()) for a, _ in pois) > 10000
        got = hipops.l1_mean_multi(pois, 2.0, ext=case.ext_t)
        got_d = hipops.l1_mean_multi_bwd(pois, 2.0, gout, ext=case.ext_t)
        torch.cuda.synchronize()
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and torch.isfinite(got[0]).all()
        for side in (0, 1):
            for x, y in zip(got_d[side], want_d[side]):
                assert torch.isfinite(x).all() and torch.equal(x.view(torch.int32), y.view(torch.int32))


def test_l1_len_bwd_is_exact_and_plus_zero_past(dev, case):
    from wavthruvec_pytorch_amd import hipops
    scale = 2.0
    gout = torch.tensor(0.37, device=dev)
    da, db = hipops.l1_mean_multi_bwd(case.pairs, scale, gout, ext=case.ext_t)
    need_a = [i % 2 == 0 for i in range(64)]
    da1, db1 = hipops.l1_mean_multi_bwd(case.pairs, scale, gout, need_a, [not w for w in need_a], ext=case.ext_t)
    torch.cuda.synchronize()
    g32 = torch.tensor(0.37, dtype=torch.float32)
    past = 0
    for i, ((a, b), e) in enumerate(zip(case.ref, case.ext)):
        a3 = R.as_rows(a, B)
        on, den = R.counted(e, *a3.shape)
        on = torch.from_numpy(np.array(on)).view(case.pairs[i][0].shape)
        a32, b32 = torch.from_numpy(a), torch.from_numpy(b)
        coef = (scale * g32) / den if den else torch.tensor(0.0)
        want = torch.where(on, torch.sign(a32 - b32) * coef, torch.zeros(()))
        got_a, got_b = da[i].cpu(), db[i].cpu()
        assert got_a.shape == a32.shape and da[i].is_contiguous() and db[i].is_contiguous()
        assert torch.equal(got_a, want) and torch.equal(got_b, -want), i
        # every float that does not count is +0.0 on both sides: the sign bit is clear
        assert (got_a[~on].view(torch.int32) == 0).all() and (got_b[~on].view(torch.int32) == 0).all(), i
        past += int((~on).sum())
        if den == 0:
            assert (got_a.view(torch.int32) == 0).all() and (got_b.view(torch.int32) == 0).all()
        wd, _ = R.l1_grad(a, b, e, scale * float(g32))
        assert np.abs(got_a.numpy() - wd).max() <= RTOL * max(np.abs(wd).max(), 1e-30)
        if need_a[i]:
            assert db1[i] is None and torch.equal(da1[i], da[i])
        else:
            assert da1[i] is None and torch.equal(db1[i], db[i])
    assert past > 10000


def test_full_extents_give_the_dense_bits(dev, case):
    from wavthruvec_pytorch_amd import hipops
    full = torch.tensor([[int(np.prod(a.shape[2:]))] * B for a, _ in case.pairs], dtype=torch.int32, device=dev)
    gout = torch.tensor(0.37, device=dev)
    d_terms, d_total = hipops.l1_mean_multi(case.pairs, 2.0)
    l_terms, l_total = hipops.l1_mean_multi(case.pairs, 2.0, ext=full)
    d_da, d_db = hipops.l1_mean_multi_bwd(case.pairs, 2.0, gout)
    l_da, l_db = hipops.l1_mean_multi_bwd(case.pairs, 2.0, gout, ext=full)
    scores = [a.flatten(1) if a.is_contiguous() else a[:, 0] for a, _ in case.pairs]
    s_full = torch.tensor([[int(np.prod(s.shape[1:]))] * B for s in scores], dtype=torch.int32, device=dev)
    targets = [float(i % 2) for i in range(64)]
    gterms = torch.linspace(-1, 1, 64).to(dev)
    d_ls = hipops.lsgan_multi(scores, targets)
    l_ls = hipops.lsgan_multi(scores, targets, ext=s_full)
    d_ds = hipops.lsgan_multi_bwd(scores, targets, gout, gterms)
    l_ds = hipops.lsgan_multi_bwd(scores, targets, gout, gterms, ext=s_full)
    torch.cuda.synchronize()
    assert torch.equal(d_terms, l_terms) and torch.equal(d_total, l_total)
    for x, y in zip(d_da + d_db + d_ds, l_da + l_db + l_ds):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    assert torch.equal(d_ls[0], l_ls[0]) and torch.equal(d_ls[1], l_ls[1])


def test_items_are_independent(dev):
    from wavthruvec_pytorch_amd import hipops
    g = torch.Generator().manual_seed(77)
    shapes = [(B, 4, 2051), (B, 2, 700, 3), (B, 1, 37)]
    pairs = [(_tensor(s, v, g, dev), _tensor(s, v, g, dev)) for s, v in zip(shapes, ('pitched', 'dense', 'off1'))]
    ext = torch.tensor([[1500, 900, 2051], [1800, 3 * 100, 0], [20, 10, 37]], dtype=torch.int32, device=dev)
    base = hipops.l1_mean_multi(pairs, 2.0, ext=ext)
    moved = [(_copy(a), b) for a, b in pairs]
    for (a, _b), e in zip(moved, ext.tolist()):
        _rows(a)[1, :, e[1]:] += 3.0                                  # item 1 past its extent
    got = hipops.l1_mean_multi(moved, 2.0, ext=ext)
    torch.cuda.synchronize()
    assert torch.equal(got[0], base[0]) and torch.equal(got[1], base[1])
    # items 1 and 2 at extent 0: whatever they hold, the terms are item 0's alone - the B = 1 call on item 0 (same denominators)
    only0 = ext.clone()
    only0[:, 1:] = 0
    t3 = hipops.l1_mean_multi(pairs, 2.0, ext=only0)[0]
    changed = [(torch.where(torch.arange(B, device=dev).view(B, *([1] * (a.dim() - 1))) > 0, a * 5 + 1, a), b) for a, b in pairs]
    t3c = hipops.l1_mean_multi(changed, 2.0, ext=only0)[0]
    t1 = hipops.l1_mean_multi([(a[:1], b[:1]) for a, b in pairs], 2.0, ext=only0[:, :1].contiguous())[0]
    torch.cuda.synchronize()
    assert torch.equal(t3, t3c)
    for x, y in zip(t3.tolist(), t1.tolist()):
        assert _rel(x, y) <= 2.0 ** -23, (x, y)


@pytest.fixture(scope='module')
def ls_case(dev):
    g = torch.Generator().manual_seed(99)
    scores, ext = [], []
    for i, U in enumerate(VALIDS):
        for inn in (1, 3):
            s = _tensor((B, 1, U, inn) if inn == 3 else (B, 1, U), ['dense', 'pitched', 'lo', 'off1', 'hi'][(i + inn) % 5], g, dev)
            scores.append(torch.flatten(s, 1, -1))                                  # (B, U * inner), as the discriminators return it
            ext.append([e * inn for e in _extents(i + inn, U)])
    targets = [float(i % 2) for i in range(len(scores))]
    ref = [s.cpu().numpy() for s in scores]
    return SimpleNamespace(scores=scores, ext=ext, ext_t=torch.tensor(ext, dtype=torch.int32, device=dev), targets=targets, ref=ref)


def test_lsgan_len_forward_backward_poison(dev, ls_case):
    from wavthruvec_pytorch_amd import hipops
    c = ls_case
    n = len(c.scores)
    gout = torch.tensor(0.37, device=dev)
    gterms = torch.linspace(-1, 1, n).to(dev)
    terms, total = hipops.lsgan_multi(c.scores, c.targets, ext=c.ext_t)
    terms2, total2 = hipops.lsgan_multi(c.scores, c.targets, ext=c.ext_t)
    ds = hipops.lsgan_multi_bwd(c.scores, c.targets, gout, gterms, ext=c.ext_t)
    pois = [_poisoned(s, e, NAN if i % 2 else INF) for i, (s, e) in enumerate(zip(c.scores, c.ext))]
    p_terms, p_total = hipops.lsgan_multi(pois, c.targets, ext=c.ext_t)
    p_ds = hipops.lsgan_multi_bwd(pois, c.targets, gout, gterms, ext=c.ext_t)
    torch.cuda.synchronize()
    want = [R.lsgan_term(s, t, e) for s, t, e in zip(c.ref, c.targets, c.ext)]
    for i, (got, w) in enumerate(zip(terms.tolist(), want)):
        assert (got == 0.0) if w == 0.0 else _rel(got, w) <= RTOL, (i, got, w)
    assert _rel(total, sum(want)) <= RTOL and sum(w == 0.0 for w in want) >= 1
    assert torch.equal(terms, terms2) and torch.equal(total, total2)
    assert torch.equal(terms, p_terms) and torch.equal(total, p_total) and torch.isfinite(p_terms).all()
    g64 = float(torch.tensor(0.37, dtype=torch.float32))
    for i, (s, t, e) in enumerate(zip(c.ref, c.targets, c.ext)):
        wd, on = R.lsgan_grad(s, t, e, g64 + float(gterms[i]))
        got = ds[i].cpu()
        assert got.shape == s.shape and ds[i].is_contiguous()
        assert np.abs(got.numpy() - wd).max() <= RTOL * max(np.abs(wd).max(), 1e-30), i
        assert (got.view(torch.int32).numpy()[~on] == 0).all(), i                     # +0.0 past the extents
        assert torch.equal(ds[i].view(torch.int32), p_ds[i].view(torch.int32)) and torch.isfinite(p_ds[i]).all()


def test_65_maps_through_the_python_chunking(dev):
    from wavthruvec_pytorch_amd import discriminators as D
    g = torch.Generator().manual_seed(7)
    f_r = [[torch.randn(B, 2, 5 + i, generator=g).to(dev) for i in range(65)]]
    f_g = [[torch.randn(B, 2, 5 + i, generator=g).to(dev).requires_grad_() for i in range(65)]]
    ext = [[(i + b) % (6 + i) for b in range(B)] for i in range(65)]
    table = torch.tensor(ext + [[1] * B] * 2, dtype=torch.int32, device=dev)
    ml = D.MapLengths(table, [65])
    loss = D.feature_loss(f_r, f_g, lengths=ml)
    loss.backward()
    torch.cuda.synchronize()
    want = 2 * sum(R.l1_term(r.cpu().numpy(), f.detach().cpu().numpy(), e) for r, f, e in zip(f_r[0], f_g[0], ext))
    assert _rel(loss, want) <= RTOL
    wd, on = R.l1_grad(f_g[0][64].detach().cpu().numpy(), f_r[0][64].cpu().numpy(), ext[64], 2.0)
    assert np.abs(f_g[0][64].grad.cpu().numpy() - wd).max() <= RTOL * np.abs(wd).max()
    assert (f_g[0][64].grad.cpu().numpy()[~on] == 0).all()


def test_map_extents_kernel_equals_the_host_integers(dev):
    from wavthruvec_pytorch_amd.discriminators import MultiPeriodDiscriminator, MultiScaleDiscriminator
    lens = [4100, 2500, 1, 0, -3, 9000, 13, 700]
    for m in (MultiPeriodDiscriminator(SimpleNamespace(periods=synthetic.DEFAULT_PERIODS)), MultiScaleDiscriminator()):
        m = m.to(dev)
        for L in (4100, None):
            got = m.map_lengths(torch.tensor(lens, device=dev), L=L)
            cap = 2 ** 31 - 1 if L is None else L
            want = []
            for j, d in enumerate(m.discriminators):
                pools = j if isinstance(m, MultiScaleDiscriminator) else 0
                per = getattr(d, 'period', 1)
                size = d.map_extents(L, pools) if L else None
                cols = [d.map_extents(min(max(n, 0), cap), pools) for n in lens]
                want += [[min(c[k], size[k] if size else c[k]) * per for c in cols] for k in range(len(cols[0]))]
            assert got.maps.tolist() == want and got.B == len(lens)
            assert got.scores.tolist() == [want[i] for i in range(len(want)) if (i + 1) % got.counts[0] == 0]
            assert got.table.dtype == torch.int32 and got.table.device.type == 'cuda'
        host = m.map_lengths([4100, 2500, 1, 700], L=4100)
        assert torch.equal(host.table, m.map_lengths(torch.tensor([4100, 2500, 1, 700], device=dev, dtype=torch.int64), L=4100).table)
        assert torch.equal(m.map_lengths([13, 7], len_mul=320).table, m.map_lengths(torch.tensor([13, 7], device=dev), len_mul=320).table)


@pytest.mark.parametrize('shape,lens', [((2, 1, 4100), [4100, 2500]), ((3, 2, 37), [37, 1, 36]), ((2, 8), [3, 8])])
def test_mask_tail(dev, shape, lens):
    from wavthruvec_pytorch_amd import mask_tail
    g = torch.Generator().manual_seed(3)
    y0 = torch.randn(shape, generator=g)
    L = shape[-1]
    on = torch.arange(L).view(*([1] * (len(shape) - 1)), L) < torch.tensor(lens).view(-1, *([1] * (len(shape) - 1)))
    yp = torch.where(on, y0, torch.full((), NAN))                               # NaN past every end
    y = yp.to(dev).requires_grad_()
    out = mask_tail(y, lens)
    out_dev = mask_tail(y.detach(), torch.tensor(lens, device=dev))
    gr = torch.randn(shape, generator=g)
    out.backward(gr.to(dev))
    torch.cuda.synchronize()
    want = torch.where(on, y0, torch.zeros(()))
    assert torch.equal(out.detach().cpu().view(torch.int32), want.view(torch.int32))           # +0.0 past the end, y's bits before
    assert torch.equal(out_dev, out.detach())
    assert torch.equal(y.grad.cpu().view(torch.int32), torch.where(on, gr, torch.zeros(())).view(torch.int32))
    full = mask_tail(y0.to(dev), [L] * shape[0])
    assert torch.equal(full.cpu().view(torch.int32), y0.view(torch.int32))                     # n_b = L: y's bits (a -0.0 would stay)
    half = mask_tail(y0.to(dev), [max(n // 2, 1) for n in lens], len_mul=2)
    assert (half.cpu()[~(torch.arange(L).expand(shape) < torch.tensor([max(n // 2, 1) * 2 for n in lens]).view(-1, *([1] * (len(shape) - 1))))] == 0).all()


def _build(kind, dev):
    from wavthruvec_pytorch_amd.discriminators import MultiPeriodDiscriminator, MultiScaleDiscriminator
    spec = synthetic.mpd_state_dict_spec() if kind == 'mpd' else synthetic.msd_state_dict_spec()
    m = MultiPeriodDiscriminator(SimpleNamespace(periods=synthetic.DEFAULT_PERIODS)) if kind == 'mpd' else MultiScaleDiscriminator()
    m.load_state_dict(synthetic.make_disc_state_dict(spec, seed=3))
    return m.to(dev).train()


@pytest.mark.parametrize('kind', ['mpd', 'msd'])
def test_end_to_end_through_the_discriminators(dev, kind):
    from wavthruvec_pytorch_amd import discriminators as D
    from wavthruvec_pytorch_amd import mask_tail
    m = _build(kind, dev)
    L, lens = 4100, [4100, 2500]
    y, y_hat = synthetic.make_audio_pair(2, L, seed=4)
    y = mask_tail(y.to(dev), lens)
    yh = y_hat.to(dev).requires_grad_()
    y_r, y_g, f_r, f_g = m(y, mask_tail(yh, lens))
    ml = m.map_lengths(lens, L=L)
    lens_dev = torch.tensor(lens, device=dev)
    m.map_lengths(lens_dev, L=L)                            # (the module's constant chain table goes to the device once)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')                 # a device tensor of lengths: no host sync from the table to the loss values
    try:
        ml_dev = m.map_lengths(lens_dev, L=L)
        feat_dev = D.feature_loss(f_r, f_g, lengths=ml_dev)
        gen_dev, _ = D.generator_loss(y_g, lengths=ml_dev)
    finally:
        torch.cuda.set_sync_debug_mode('default')
    assert torch.equal(ml_dev.table, ml.table)
    feat = D.feature_loss(f_r, f_g, lengths=ml)
    gen, gen_terms = D.generator_loss(y_g, lengths=ml)
    disc, real_terms, fake_terms = D.discriminator_loss(y_r, y_g, lengths=ml)
    assert torch.equal(feat, feat_dev) and torch.equal(gen, gen_dev)
    # the torch expression of the definition (the CPU path) on the library's own maps
    cpu = lambda xs: [x.detach().cpu().double() for x in xs]
    w_feat = D.feature_loss([cpu(ms) for ms in f_r], [cpu(ms) for ms in f_g], lengths=ml)
    w_gen, w_gen_terms = D.generator_loss(cpu(y_g), lengths=ml)
    w_disc, w_real, w_fake = D.discriminator_loss(cpu(y_r), cpu(y_g), lengths=ml)
    for name, got, want in (('feature', feat, w_feat), ('generator', gen, w_gen), ('discriminator', disc, w_disc)):
        print(f'[{kind}] {name}: {got.item()!r} vs torch {want.item()!r}: rel {_rel(got, want):.2e}')
        assert got.dim() == 0 and _rel(got, want) <= RTOL, name
    assert all(_rel(t, w) <= RTOL for t, w in zip(gen_terms, w_gen_terms))
    assert all(isinstance(t, float) and _rel(t, w) <= RTOL for t, w in zip(real_terms + fake_terms, w_real + w_fake))
    dense = D.feature_loss(f_r, f_g)
    assert _rel(dense, feat) > 1e-4                         # the lengths are seen
    (feat + gen + disc).backward()
    torch.cuda.synchronize()
    assert torch.isfinite(yh.grad).all() and (yh.grad[1, :, 2500:] == 0).all() and yh.grad[1, :, :2500].abs().max() > 0
    assert yh.grad[0].abs().max() > 0
