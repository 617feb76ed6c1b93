"""CPU tests of the multi-resolution STFT loss (csrc/v2w_stft_loss.hip, wavthruvec_pytorch_amd/stft_loss.py): the C ABI surface, the host-only
work split against its restatement, what the entry points refuse (through the dry-run stream) and what the name sink reports, the two
references of tests/stft_loss_ref.py against each other, and the Python errors.  No GPU needed: nothing is launched."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from tests import mel_ref as R
from tests import stft_loss_ref as SL
from tests import stft_ref as S
from wavthruvec_pytorch_amd import _hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('v2w_stft_loss_plan', 'v2w_stft_loss_scratch_bytes', 'v2w_stft_loss_multi', 'v2w_stft_loss_multi_bwd')
FAKE = 0x7f0000100000       # 16-byte aligned "device" pointers: the plan, the dry run and the name sink never dereference them
DRY = C.c_void_p(-1)


def _items(shapes, off=0):
    """shapes: (nb, F, FP, Cs, B) -> descriptor array on fake pointers (`off`: bytes added to every spec_x)."""
    arr = (_hip.StftLossItem * max(len(shapes), 1))()
    for d, (nb, F, FP, Cs, B) in zip(arr, shapes):
        d.spec_x, d.spec_y, d.dspec_x = FAKE + off, FAKE + 0x40000000, FAKE + 0x80000000
        d.B, d.Cs, d.FP, d.F, d.nb = B, Cs, FP, F, nb
    return arr


def _fwd(lib, arr, n, stream=DRY, **kw):
    a = dict(sc=FAKE, mag=FAKE + 0x100, total=FAKE + 0x200, sums=FAKE + 0x300, scratch=FAKE + 0x1000)
    a.update(kw)
    return lib.v2w_stft_loss_multi(arr, n, a['sc'], a['mag'], a['total'], a['sums'], a['scratch'], stream)


def _bwd(lib, arr, n, sums=FAKE, g=(FAKE, FAKE, None, None), stream=DRY):
    return lib.v2w_stft_loss_multi_bwd(arr, n, sums, *g, stream)


def test_entry_points_are_declared_bound_and_additive():
    hdr = open(os.path.join(ROOT, 'include', 'vec2wav_hip.h')).read()
    assert int(re.search(r'#define V2W_ABI_VERSION (\d+)', hdr).group(1)) == _hip.ABI_VERSION == 35 == _hip.load().v2w_abi_version()
    for name in NAMES:
        assert name in _hip.SIGNATURES and re.search(r'\b%s\s*\(' % name, hdr), name
        assert (name in _hip.LAUNCHERS) == name.startswith('v2w_stft_loss_multi'), name
    body = hdr[:hdr.index('} v2w_stft_loss_item;')]
    body = re.sub(r'/\*.*?\*/', '', body[body.rindex('typedef struct {'):], flags=re.S)
    assert re.findall(r'\b(\w+)\s*[;,]', body) == [n for n, _ in _hip.StftLossItem._fields_]
    assert C.sizeof(_hip.StftLossItem) == 48
    assert int(re.search(r'#define V2W_STFT_LOSS_MAX_ITEMS\s+(\d+)', hdr).group(1)) == _hip.STFT_LOSS_MAX_ITEMS == 8
    assert int(re.search(r'#define V2W_STFT_LOSS_TARGET_WGS\s+(\d+)', hdr).group(1)) == _hip.STFT_LOSS_TARGET_WGS


def _plan_restated(shapes):
    """include/vec2wav_hip.h: B * nb * ceil(F / 4) units, ceil(units / max(2048, ceil(units / TARGET))) workgroups, each resolution alone."""
    starts = [0]
    for nb, F, FP, Cs, B in shapes:
        units = B * nb * ((F + 3) // 4)
        chunk = max(2048, -(-units // _hip.STFT_LOSS_TARGET_WGS))
        starts.append(starts[-1] + max(1, -(-units // chunk)))
    return starts


def _shape_of(geo, B, L):
    from wavthruvec_pytorch_amd import mel
    g = mel.stft_geometry(*geo)
    F = mel.mel_frames(L, geo[0], geo[1])
    return g['nb'], F, (F + g['k'] - 1 + 3) // 4 * 4, g['cs'], B


PLANS = dict(tiny=[SL.SHAPES['one_frame']], kernel_cases=list(SL.SHAPES.values()),
             train=[_shape_of(g, 32, 81920) for g in ((1024, 120, 600), (2048, 240, 1200), (512, 50, 240))],
             small=[_shape_of(g, 2, 8192) for g in S.LARGE], eight=[SL.SHAPES['tail3']] * 8)


@pytest.mark.parametrize('case', sorted(PLANS))
def test_plan_is_deterministic_and_matches_its_restatement(case):
    lib = _hip.load()
    shapes = PLANS[case]
    n = len(shapes)
    got = []
    for _ in range(2):
        starts = (C.c_int32 * (n + 1))()
        nwg = lib.v2w_stft_loss_plan(_items(shapes), n, starts)
        got.append((nwg, list(starts)))
    assert got[0] == got[1]
    nwg, starts = got[0]
    assert starts == _plan_restated(shapes) and nwg == starts[-1]
    assert starts[0] == 0 and all(1 <= b - a <= _hip.STFT_LOSS_TARGET_WGS for a, b in zip(starts, starts[1:]))
    assert lib.v2w_stft_loss_scratch_bytes(_items(shapes), n) == 24 * nwg
    # a resolution's workgroups depend on its own descriptor only
    for i, s in enumerate(shapes):
        one = (C.c_int32 * 2)()
        assert lib.v2w_stft_loss_plan(_items([s]), 1, one) == starts[i + 1] - starts[i]
    assert _fwd(lib, _items(shapes), n) == 0 and _bwd(lib, _items(shapes), n) == 0          # the dry run takes what the plan takes


def test_training_shapes_fill_the_gpu():
    lib = _hip.load()
    starts = (C.c_int32 * 4)()
    assert lib.v2w_stft_loss_plan(_items(PLANS['train']), 3, starts) >= 3 * 512


def test_entry_points_refuse_bad_descriptors_with_an_error_code():
    lib = _hip.load()
    ok = SL.SHAPES['tail3']
    nb, F, FP, Cs, B = ok
    E_ARG, E_SHAPE = _hip.E_ARG, _hip.E_SHAPE

    def both(shapes, n=None, **kw):
        arr = _items(shapes, **kw)
        n = len(shapes) if n is None else n
        starts = (C.c_int32 * 9)()
        r = {_fwd(lib, arr, n), _bwd(lib, arr, n), min(lib.v2w_stft_loss_plan(arr, n, starts), 0), min(lib.v2w_stft_loss_scratch_bytes(arr, n), 0)}
        assert len(r) == 1, r
        return r.pop()

    assert both([ok] * 8) == 0
    assert both([ok] * 8, n=9) == E_ARG and both([ok], n=0) == E_ARG
    assert _fwd(lib, None, 1) == E_ARG and _bwd(lib, None, 1) == E_ARG
    for bad in ((0, F, FP, Cs, B), (nb, 0, FP, Cs, B), (nb, F, FP, Cs, 0), (nb, F, FP, Cs, -1)):        # B / F / nb <= 0
        assert both([bad]) == E_ARG, bad
    assert both([(nb, 9, 8, Cs, B)]) == E_ARG                       # FP < F
    assert both([(nb, F, FP, 2 * nb - 1, B)]) == E_ARG              # Cs < 2 nb
    assert both([(nb, F, FP, 2 * nb, B)]) == 0
    assert both([(nb, F, 10, Cs, B)]) == E_ARG                      # FP % 4
    assert both([ok], off=4) == E_ARG                               # rows off the 16-byte lines
    assert both([(nb, 1 << 21, 1 << 21, 2 * nb + 1000, 1)]) == E_SHAPE                       # Cs * FP past 2^31 - 1
    assert both([(1025, 1000, 1000, 2112, 1017)]) == E_SHAPE and both([(1025, 1000, 1000, 2112, 1016)]) == 0     # B * Cs * FP
    arr = _items([ok])
    for null in ('spec_x', 'spec_y'):
        a = _items([ok])
        setattr(a[0], null, None)
        assert _fwd(lib, a, 1) == E_ARG and _bwd(lib, a, 1) == E_ARG, null
    a = _items([ok])
    a[0].dspec_x = None
    assert _fwd(lib, a, 1) == 0 and _bwd(lib, a, 1) == E_ARG        # the forward ignores dspec_x
    assert _fwd(lib, arr, 1, scratch=None) == E_ARG and _fwd(lib, arr, 1, scratch=FAKE + 4) == E_ARG
    assert _fwd(lib, arr, 1, sc=None, mag=None, total=None, sums=None) == E_ARG
    assert _fwd(lib, arr, 1, sc=None, mag=None, total=None) == 0 and _fwd(lib, arr, 1, sums=FAKE + 4) == E_ARG
    assert _bwd(lib, arr, 1, sums=None) == E_ARG and _bwd(lib, arr, 1, g=(None, None, None, None)) == E_ARG
    assert _bwd(lib, arr, 1, g=(None, None, FAKE, None)) == 0 and _bwd(lib, arr, 1, g=(FAKE + 2, None, None, None)) == E_ARG


def test_name_sink_lists_the_three_kernels():
    lib = _hip.load()
    shapes = [SL.SHAPES[s] for s in SL.KERNEL_CASES['mixed']]
    arr = _items(shapes)
    rc, names = _hip.kernel_names(lib.v2w_stft_loss_multi, arr, 3, FAKE, FAKE, FAKE, FAKE, FAKE)
    assert rc in (0, 100) and names == ['stft_loss_sums_kernel', 'stft_loss_finish_kernel'], names
    rc, names = _hip.kernel_names(lib.v2w_stft_loss_multi_bwd, arr, 3, FAKE, FAKE, FAKE, None, None)
    assert rc in (0, 100) and names == ['stft_loss_bwd_kernel'], names
    assert _hip.kernel_names(lib.v2w_stft_loss_multi, arr, 9, FAKE, FAKE, FAKE, FAKE, FAKE) == (-1, [])


@pytest.mark.parametrize('case', sorted(SL.KERNEL_CASES))
def test_the_kernels_statement_is_autograd_through_the_oracles_formulas(case):
    """Reference (a) against (b)'s loss_of_spectra in fp64, fed the same spectra; both gradient inputs at once.  And the share of entries the
    device test leaves unchecked stays under its cap at every random-spec case."""
    specs = SL.case_specs(case)
    n = len(specs)
    g_sc, g_mag = SL.g_of(0.75, 0.5, n), SL.g_of(-1.25, None, n)
    for (nb, F, FP, Cs, B), sx, sy in specs:
        v, b = SL.sums(sx, sy, F, nb)
        assert all(0 < b[k] < 1e-4 * v[k] for k in ('Sy', 'Sl', 'sc', 'mag')) and 0 < b['Sd'] < 1e-4 * v['Sd']
        t = [torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)) for a in
             (sx[:, :nb, :F], sx[:, nb:2 * nb, :F], sy[:, :nb, :F], sy[:, nb:2 * nb, :F])]
        t[0].requires_grad_(True)
        t[1].requires_grad_(True)
        sc, mag = SL.loss_of_spectra(*t)
        assert abs(sc.item() - v['sc']) <= 1e-12 * v['sc'] and abs(mag.item() - v['mag']) <= 1e-12 * v['mag']
        (g_sc * sc + g_mag * mag).backward()
        dre, dim, bre, bim, unsure = SL.dspec(sx, sy, F, nb, v['Sd'], v['Sy'], g_sc, g_mag)
        scale = np.abs(dre).max()
        assert np.abs(dre - t[0].grad.numpy()).max() <= 1e-12 * scale and np.abs(dim - t[1].grad.numpy()).max() <= 1e-12 * scale
        assert (bre >= 0).all() and np.isfinite(bre).all() and bre.max() < 1e-4 * scale
        assert unsure.mean() <= SL.MAX_UNSURE, (case, unsure.mean())


def test_equal_signals_have_zero_loss_and_zero_gradient_in_the_reference():
    (nb, F, FP, Cs, B), sx, sy = SL.case_specs('tail3', same=True)[0]
    v, _ = SL.sums(sx, sy, F, nb)
    assert v['Sd'] == 0 and v['sc'] == 0 and v['mag'] == 0
    dre, dim, *_ = SL.dspec(sx, sy, F, nb, v['Sd'], v['Sy'], 1.0, 1.0)
    assert not dre.any() and not dim.any()
    x = torch.from_numpy(S.signal(1, 300, 1)).double().requires_grad_(True)
    sc, mag = SL.loss_of_spectra(*SL.spectrum(x, (128, 32, 96), torch.float64), *SL.spectrum(x.detach(), (128, 32, 96), torch.float64))
    (sc + mag).backward()
    assert sc.item() == 0 and mag.item() == 0 and not x.grad.any()


def test_real_spectra_leave_few_entries_unchecked():
    """Through real STFTs of the independent signals the share of |X / Y - 1| < GAP is far below the cap."""
    x, y = SL.signals(2, 8192)
    for geo in S.LARGE:
        X = torch.sqrt(sum(p.pow(2) for p in SL.spectrum(torch.from_numpy(x).double(), geo, torch.float64)) + 1e-9)
        Y = torch.sqrt(sum(p.pow(2) for p in SL.spectrum(torch.from_numpy(y).double(), geo, torch.float64)) + 1e-9)
        assert ((X / Y - 1).abs() < R.GAP).double().mean().item() <= SL.MAX_UNSURE


def test_python_errors():
    from wavthruvec_pytorch_amd import MultiResolutionSTFTLoss, mel, stft_loss
    assert stft_loss.MultiResolutionSTFTLoss is MultiResolutionSTFTLoss
    assert MultiResolutionSTFTLoss().resolutions == ((1024, 120, 600), (2048, 240, 1200), (512, 50, 240))
    a, b = torch.zeros(2, 4096), torch.zeros(2, 4096)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        MultiResolutionSTFTLoss()(a, b)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        stft_loss.stft_loss(a.unsqueeze(1), b, 512, 50, 240)
    with pytest.raises(ValueError, match='must not require grad'):
        stft_loss.stft_loss(a, b.clone().requires_grad_(True), 512, 50, 240)
    for bad in (torch.zeros(2, 4095), torch.zeros(3, 4096), torch.zeros(2, 2, 4096), torch.zeros(4096)):
        with pytest.raises(ValueError, match='one shape'):
            stft_loss.stft_loss(a, bad, 512, 50, 240)
    for geo in ((4096, 256, 1024), (512, 0, 240), (512, 513, 240), (512, 50, 600)):
        with pytest.raises(ValueError) as e1:
            mel.stft_geometry(*geo)
        with pytest.raises(ValueError) as e2:
            stft_loss.stft_loss(a, b, *geo)
        with pytest.raises(ValueError) as e3:
            MultiResolutionSTFTLoss(resolutions=[(512, 50, 240), geo])
        assert str(e1.value) == str(e2.value) == str(e3.value)
    with pytest.raises(ValueError):
        MultiResolutionSTFTLoss(resolutions=[(128, 32, 128)] * 9)
    with pytest.raises(ValueError):
        MultiResolutionSTFTLoss(resolutions=[])
