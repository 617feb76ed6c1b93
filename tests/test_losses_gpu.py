"""GPU tests of the GAN loss kernels (v2w_l1_mean_multi / v2w_lsgan_multi and their backwards) and of the loss helpers built on them
(discriminators.feature_loss / discriminator_loss / generator_loss / l1_mean_loss), against fp64 torch on the CPU.

Bounds.  Forward values, 1e-6 relative: every |a - b| (and every (t - s)^2 factor) carries at most a few fp32 roundings of 2^-24, the
summands are non-negative, the accumulation is fp64 and the result is rounded once to fp32 - about 1.2e-7 to 2.4e-7 in all.  The L1
gradient is exact: sgn(a - b) times the fp32 quotient (scale * gout) / numel, so it is compared bit for bit."""
import copy
from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as F

from wavthruvec_pytorch_amd import synthetic

pytestmark = pytest.mark.gpu
RTOL = 1e-6


@pytest.fixture(scope='module')
def dev():
    from wavthruvec_pytorch_amd import _hip
    _hip.load()
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def _rel(got, want):
    got, want = (float(v.detach()) if torch.is_tensor(v) else float(v) for v in (got, want))
    return abs(got - want) / max(abs(want), 1e-30)


def _pitched(shape, pitch, g, dev, lead=None):
    """A (..., valid) view of a (..., pitch) GPU buffer whose [valid, pitch) tail is NaN; `lead`: a slice of the first dim."""
    buf = torch.full(shape[:-1] + (pitch,), float('nan'))
    buf[..., :shape[-1]] = torch.randn(shape, generator=g)
    view = buf.to(dev)[..., :shape[-1]]
    return view if lead is None else view[lead]


@pytest.fixture(scope='module')
def l1_case(dev):
    """The pairs of one call (GPU views), their fp64 CPU copies, and the fp64 terms - computed once."""
    g = torch.Generator().manual_seed(1234)
    pairs = []

    def dense(*shape):
        pairs.append(tuple(torch.randn(shape, generator=g).to(dev) for _ in range(2)))

    dense(1)                                                                    # numel = 1
    odd = [torch.randn(4100, generator=g).to(dev)[1:] for _ in range(2)]        # 4 099 floats, off the 16-byte lines, with a tail
    pairs.append(tuple(odd))
    pairs.append((_pitched((2, 3, 13), 16, g, dev), _pitched((2, 3, 13), 16, g, dev)))
    dense(4, 8, 20)                                                             # valid == pitch
    big = [_pitched((6, 5, 22), 24, g, dev) for _ in range(2)]                  # both halves of a real-plus-generated batch
    pairs.append((big[0][:3], big[1][:3]))
    pairs.append((big[0][3:], big[1][3:]))
    v4 = [_pitched((2, 4, 21), 24, g, dev).view(2, 4, 7, 3) for _ in range(2)]   # (b, C, U, inner) view of a (b, C, 24) buffer
    pairs.append(tuple(v4))
    dense(3, 64, 1000)                                                          # several workgroups
    pairs.append((torch.randn(2, 5, 12, generator=g).to(dev), _pitched((2, 5, 12), 16, g, dev)))      # dense against pitched
    # planted ties: a == b must give a zero gradient
    pairs[1][0][::5] = pairs[1][1][::5]
    pairs[2][0][:, :, 3] = pairs[2][1][:, :, 3]
    pairs[7][0][:, :, ::9] = pairs[7][1][:, :, ::9]
    ref = [(a.detach().cpu().double(), b.detach().cpu().double()) for a, b in pairs]
    assert all(torch.isfinite(a).all() and torch.isfinite(b).all() for a, b in ref)
    terms = [(a - b).abs().mean().item() for a, b in ref]
    return SimpleNamespace(pairs=pairs, ref=ref, terms=terms)


def test_l1_mean_multi_matches_fp64_and_is_deterministic(dev, l1_case):
    from wavthruvec_pytorch_amd import hipops
    for a, b in l1_case.pairs:                       # every view goes through without a copy
        assert hipops.loss_rows(a, b) is not None and hipops.loss_rows(b, a) is not None
    scale = 2.0
    terms, total = hipops.l1_mean_multi(l1_case.pairs, scale)
    terms2, total2 = hipops.l1_mean_multi(l1_case.pairs, scale)
    torch.cuda.synchronize()
    assert terms.shape == (len(l1_case.pairs),) and total.shape == ()
    assert torch.isfinite(terms).all() and torch.isfinite(total)          # the NaN padding was not read
    for i, (got, want) in enumerate(zip(terms.tolist(), l1_case.terms)):
        print(f'pair {i}: {got!r} vs fp64 {want!r}: rel {_rel(got, want):.2e}')
        assert _rel(got, want) <= RTOL, i
    want_total = scale * sum(l1_case.terms)
    print(f'total: {total.item()!r} vs {want_total!r}: rel {_rel(total, want_total):.2e}')
    assert _rel(total, want_total) <= RTOL
    assert torch.equal(terms, terms2) and torch.equal(total, total2)     # bit-identical


def test_l1_mean_multi_takes_64_pairs_and_refuses_65(dev):
    from wavthruvec_pytorch_amd import _hip, hipops
    g = torch.Generator().manual_seed(7)
    pairs = [(torch.randn(3, 5 + i, generator=g).to(dev), torch.randn(3, 5 + i, generator=g).to(dev)) for i in range(65)]
    terms, total = hipops.l1_mean_multi(pairs[:64])
    want = [(a.cpu().double() - b.cpu().double()).abs().mean().item() for a, b in pairs[:64]]
    for got, w in zip(terms.tolist(), want):
        assert _rel(got, w) <= RTOL
    assert _rel(total, sum(want)) <= RTOL
    with pytest.raises(_hip.HipLibraryError) as e:
        hipops.l1_mean_multi(pairs)
    assert e.value.code == _hip.E_ARG
    torch.cuda.synchronize()


def test_l1_mean_multi_bwd_is_exact_and_dense(dev, l1_case):
    from wavthruvec_pytorch_amd import hipops
    scale = 2.0
    gout = torch.tensor(0.37, device=dev)
    n = len(l1_case.pairs)
    da, db = hipops.l1_mean_multi_bwd(l1_case.pairs, scale, gout)
    # one side only: a on the even pairs, b on the odd ones
    need_a = [i % 2 == 0 for i in range(n)]
    da1, db1 = hipops.l1_mean_multi_bwd(l1_case.pairs, scale, gout, need_a, [not w for w in need_a])
    torch.cuda.synchronize()
    g32 = torch.tensor(0.37, dtype=torch.float32)
    zeros = 0
    for i, (a, b) in enumerate(l1_case.pairs):
        a32, b32 = a.cpu(), b.cpu()
        want = torch.sign(a32 - b32) * ((scale * g32) / a32.numel())
        assert want.dtype == torch.float32
        assert da[i].shape == a.shape and da[i].is_contiguous() and db[i].is_contiguous()
        assert torch.equal(da[i].cpu(), want), i
        assert torch.equal(db[i].cpu(), -want), i
        ties = a32 == b32
        zeros += int(ties.sum())
        assert (da[i].cpu()[ties] == 0).all()
        if need_a[i]:
            assert db1[i] is None and torch.equal(da1[i], da[i])
        else:
            assert da1[i] is None and torch.equal(db1[i], db[i])
    assert zeros > 100          # the planted ties are there


@pytest.fixture(scope='module')
def lsgan_case(dev):
    g = torch.Generator().manual_seed(99)
    shapes = [(1,), (7,), (77,), (1000,), (4099,), (2, 2731)]
    targets = [1.0, 0.0, 1.0, 0.0, 1.0, 0.0]
    scores = [torch.randn(s, generator=g).to(dev) for s in shapes]
    # a pitched score, as `flatten(fmap[-1], 1, -1)[:nb]` of a (B, 1, roundup4(U)) buffer is
    scores.append(torch.flatten(_pitched((4, 1, 13), 16, g, dev), 1, -1)[2:])
    targets.append(1.0)
    ref = [s.detach().cpu().double() for s in scores]
    return SimpleNamespace(scores=scores, targets=targets, ref=ref)


def test_lsgan_multi_forward_and_backward(dev, lsgan_case):
    from wavthruvec_pytorch_amd import hipops
    c = lsgan_case
    terms, total = hipops.lsgan_multi(c.scores, c.targets)
    terms2, total2 = hipops.lsgan_multi(c.scores, c.targets)
    gout = torch.tensor(0.37, device=dev)
    ds = hipops.lsgan_multi_bwd(c.scores, c.targets, gout)
    ds2 = hipops.lsgan_multi_bwd(c.scores, c.targets, gout)
    gterms = torch.linspace(-1, 1, len(c.scores)).to(dev)
    ds3 = hipops.lsgan_multi_bwd(c.scores, c.targets, gout, gterms)
    torch.cuda.synchronize()
    assert torch.isfinite(terms).all()
    want = [((t - s) ** 2).mean().item() for s, t in zip(c.ref, c.targets)]
    for i, (got, w) in enumerate(zip(terms.tolist(), want)):
        print(f'term {i}: {got!r} vs fp64 {w!r}: rel {_rel(got, w):.2e}')
        assert _rel(got, w) <= RTOL, i
    assert _rel(total, sum(want)) <= RTOL
    assert torch.equal(terms, terms2) and torch.equal(total, total2)
    g64 = float(torch.tensor(0.37, dtype=torch.float32))
    for i, (s, t) in enumerate(zip(c.ref, c.targets)):
        wd = 2 * (s - t) * g64 / s.numel()
        assert ds[i].shape == s.shape and ds[i].is_contiguous()
        err = (ds[i].cpu().double() - wd).abs().max().item()
        print(f'ds {i}: max err {err:.2e} of max {wd.abs().max().item():.2e}')
        assert err <= RTOL * wd.abs().max().item(), i
        assert torch.equal(ds[i], ds2[i])
        wd3 = 2 * (s - t) * (g64 + float(gterms[i])) / s.numel()
        assert (ds3[i].cpu().double() - wd3).abs().max().item() <= RTOL * max(wd3.abs().max().item(), wd.abs().max().item()), i


def _build(kind, dev):
    from wavthruvec_pytorch_amd.discriminators import MultiPeriodDiscriminator, MultiScaleDiscriminator
    spec = synthetic.mpd_state_dict_spec() if kind == 'mpd' else synthetic.msd_state_dict_spec()
    m = MultiPeriodDiscriminator(SimpleNamespace(periods=synthetic.DEFAULT_PERIODS)) if kind == 'mpd' else MultiScaleDiscriminator()
    m.load_state_dict(synthetic.make_disc_state_dict(spec, seed=3))
    return m.to(dev).train()


def _torch_losses(outs):
    """Today's torch expressions (models.py:278-310) on the returned scores and maps."""
    y_r, y_g, f_r, f_g = outs
    feat = 2 * sum(torch.mean(torch.abs(r - f)) for mr, mg in zip(f_r, f_g) for r, f in zip(mr, mg))
    gen_terms = [torch.mean((1 - s) ** 2) for s in y_g]
    real_terms = [torch.mean((1 - s) ** 2) for s in y_r]
    fake_terms = [torch.mean(s ** 2) for s in y_g]
    return feat, sum(gen_terms), gen_terms, sum(r + f for r, f in zip(real_terms, fake_terms)), real_terms, fake_terms


def _torch_terms_hip(scores, target):
    """The single LSGAN terms as the kernel gives them (the Python floats of discriminator_loss are exactly these)."""
    from wavthruvec_pytorch_amd import hipops
    return hipops.lsgan_multi(scores, [target] * len(scores))[0]


@pytest.mark.parametrize('freeze', [False, True])
@pytest.mark.parametrize('kind', ['mpd', 'msd'])
def test_losses_through_the_discriminators(dev, kind, freeze):
    import contextlib
    from wavthruvec_pytorch_amd import discriminators as D
    m = _build(kind, dev)
    y, y_hat = synthetic.make_audio_pair(1, 1000, seed=4)
    y = y.to(dev)

    yh = y_hat.to(dev).requires_grad_()
    with (D.frozen(m) if freeze else contextlib.nullcontext()):
        outs = m(y, yh)
    y_r, y_g, f_r, f_g = outs
    before = copy.deepcopy([[t.detach() for t in maps] for maps in f_r + f_g])
    feat = D.feature_loss(f_r, f_g)
    gen, gen_terms = D.generator_loss(y_g)
    disc, real_terms, fake_terms = D.discriminator_loss(y_r, y_g)
    got = (feat, gen, gen_terms, disc, real_terms, fake_terms)
    for maps, saved in zip(f_r + f_g, before):               # the maps are read, not used as scratch
        for t, sv in zip(maps, saved):
            assert torch.equal(t.detach(), sv)
    want = _torch_losses(outs)                               # the same quantities on the same returned scores and maps
    grad_g, = torch.autograd.grad(got[0] + got[1] + got[3], yh, retain_graph=True)
    grad_w, = torch.autograd.grad(want[0] + want[1] + want[3], yh)
    torch.cuda.synchronize()
    for name, i in (('feature', 0), ('generator', 1), ('discriminator', 3)):
        print(f'{kind} frozen={freeze} {name}: {got[i].item()!r} vs {want[i].item()!r}: rel {_rel(got[i], want[i]):.2e}')
        assert got[i].dim() == 0 and _rel(got[i], want[i]) <= RTOL, name
    assert len(got[2]) == len(want[2]) and all(t.dim() == 0 and _rel(t, w) <= RTOL for t, w in zip(got[2], want[2]))
    for terms_g, terms_w in ((got[4], want[4]), (got[5], want[5])):
        assert len(terms_g) == len(terms_w) and all(isinstance(t, float) for t in terms_g)
        assert all(_rel(t, w) <= RTOL for t, w in zip(terms_g, terms_w))
    assert got[4] == [t.item() for t in _torch_terms_hip(y_r, 1.0)] and got[5] == [t.item() for t in _torch_terms_hip(y_g, 0.0)]
    err = (grad_g - grad_w).abs().max().item()
    print(f'{kind} frozen={freeze} y_hat.grad: max err {err:.3e} of max {grad_w.abs().max().item():.3e}, equal bits: {torch.equal(grad_g, grad_w)}')
    assert err <= RTOL * grad_w.abs().max().item()


def test_l1_mean_loss_on_mels(dev):
    from wavthruvec_pytorch_amd import discriminators as D
    g = torch.Generator().manual_seed(5)
    a0, b0 = torch.randn(2, 80, 32, generator=g), torch.randn(2, 80, 32, generator=g)
    a0[:, :, 5] = b0[:, :, 5]
    a, b = a0.to(dev).requires_grad_(), b0.to(dev).requires_grad_()
    loss = D.l1_mean_loss(a, b)
    (loss * 0.37).backward()
    torch.cuda.synchronize()
    a64, b64 = a0.double().requires_grad_(), b0.double().requires_grad_()
    want = F.l1_loss(a64, b64)
    (want * 0.37).backward()
    assert loss.dim() == 0 and _rel(loss, want) <= RTOL
    coef = (1.0 * torch.tensor(0.37, dtype=torch.float32)) / a0.numel()
    assert torch.equal(a.grad.cpu(), torch.sign(a0 - b0) * coef) and torch.equal(b.grad.cpu(), -a.grad.cpu())
    assert (a.grad.cpu().double() - a64.grad).abs().max().item() <= RTOL * a64.grad.abs().max().item()
    # only the generated side asks for a gradient (train.py:204: y_mel is data)
    b2 = b0.to(dev).requires_grad_()
    D.l1_mean_loss(a0.to(dev), b2).backward()
    assert torch.equal(b2.grad.cpu(), -torch.sign(a0 - b0) * (torch.tensor(1.0) / a0.numel()))
