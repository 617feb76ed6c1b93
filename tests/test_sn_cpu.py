"""CPU tests of the spectral-norm entry points (v2w_sn_plan / v2w_sn_step / v2w_sn_bwd): the fp64 restatement (tests/sn_ref.py) against legacy
torch.nn.utils.spectral_norm and against the reference's recorded buffers, the C ABI surface, the host plan against the header's work
split, what the name sink reports for every case, the launch-count caps and what the entry points refuse.  Nothing is launched."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from tests import golden_util, sn_ref as R
from wavthruvec_pytorch_amd import _hip, hipops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('v2w_sn_plan', 'v2w_sn_step', 'v2w_sn_bwd')
FAKE = 0x7f0000100000       # 16-byte aligned "device" pointers: the plan, the dry run and the name sink never dereference them
DRY = C.c_void_p(-1)
STEP_KERNELS = ['sn_wtu_kernel', 'sn_v_kernel', 'sn_wv_kernel', 'sn_scale_kernel']
BWD_KERNELS = ['sn_bwd_dot_kernel', 'sn_bwd_apply_kernel']


def _header():
    return open(os.path.join(ROOT, 'include', 'vec2wav_hip.h')).read()


def _struct_fields(hdr, name):
    body = hdr[:hdr.index('} %s;' % name)]
    body = body[body.rindex('typedef struct {'):]
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    return re.findall(r'\b(\w+)(?:\[\d+\])?\s*[;,]', body)


def _descs(shapes):
    arr = (_hip.SnDesc * max(len(shapes), 1))()
    for i, (d, (co, ci, k)) in enumerate(zip(arr, shapes)):
        base = FAKE + i * (1 << 32)
        d.w, d.u, d.v, d.wf = base, base + (1 << 28), base + (2 << 28), base + (3 << 28)
        d.c_out, d.c_in, d.k = co, ci, k
    return arr


def _planned(shapes):
    arr, g = _descs(shapes), _hip.SnGrids()
    rc = _hip.load().v2w_sn_plan(arr, len(shapes), C.byref(g))
    return arr, g, rc


def test_entry_points_are_declared_bound_and_additive():
    hdr = _header()
    assert int(re.search(r'#define V2W_ABI_VERSION (\d+)', hdr).group(1)) == _hip.ABI_VERSION == 35 == _hip.load().v2w_abi_version()
    for name in NAMES:
        assert name in _hip.SIGNATURES and re.search(r'\b%s\s*\(' % name, hdr), name
    assert {'v2w_sn_step', 'v2w_sn_bwd'} <= _hip.LAUNCHERS and 'v2w_sn_plan' not in _hip.LAUNCHERS
    assert _struct_fields(hdr, 'v2w_sn_desc') == [n for n, _ in _hip.SnDesc._fields_]
    assert _struct_fields(hdr, 'v2w_sn_grids') == [n for n, _ in _hip.SnGrids._fields_]
    assert C.sizeof(_hip.SnDesc) == 72 and C.sizeof(_hip.SnGrids) == 32
    assert int(re.search(r'#define V2W_SN_MAX_LAYERS\s+(\d+)', hdr).group(1)) == _hip.SN_MAX_LAYERS >= 8
    text = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    assert all(name in text for name in NAMES)
    # the rounding counts the bounds rest on are the ones the header states
    for frag in ('[16 + 3 + nb - 1]', '[ceil(N / 1024) + 22]', '[ceil(N / 256) + 8]', '[ceil(N / 64) + 6]', '[ceil(R / 256) + 10]',
                 '[26 + ceil(tiles / 256) + 10]'):
        assert frag in hdr, frag
    c = R.counts(1024, 5120)
    assert (c['a'], c['q'], c['t'], c['p'], c['dot']) == (34, 27, 28, 14, 41) and R.counts(128, 15)['t'] == 7


def test_the_case_list_holds_the_workloads_shapes_and_the_edges():
    assert [(co, ci * k) for co, ci, k in R.real_shapes()] == [(128, 15), (128, 1312), (256, 328), (512, 656), (1024, 1312), (1024, 2624),
                                                               (1024, 5120), (1, 3072)]
    assert [(co, ci * k) for co, ci, k in R.EDGE_SHAPES] == [(1, 3), (3, 7), (17, 15), (130, 33), (64, 4)]


@pytest.mark.parametrize('which', ['all', 'real', 'each'])
def test_plan_matches_the_headers_work_split_and_its_workspace_covers_every_block(which):
    sets = dict(all=[R.cases()], real=[R.real_shapes()], each=[[s] for s in R.cases()])[which]
    for shapes in sets:
        n = len(shapes)
        arr, g, rc = _planned(shapes)
        rows, totals = R.plan_ref(shapes)
        assert rc == g.ws_bytes == totals[3] > 0 and g.n == n
        assert (g.grid_t, g.grid_r, g.grid_s, g.ws_bytes, g.keep_bytes) == totals
        assert [(d.blk_t, d.blk_r, d.blk_s, d.ws_off, d.keep_off) for d in arr[:n]] == rows
        ends = rows[1:] + [(totals[0], totals[1], totals[2], totals[3] // 4, totals[4] // 4)]
        for (co, ci, k), a, b in zip(shapes, rows, ends):
            N, c = ci * k, R.counts(co, ci * k)
            assert b[0] - a[0] == c['nb'] * R.cdiv(N, 256) >= 1 and b[1] - a[1] == R.cdiv(co, 4) >= 1 and b[2] - a[2] == c['tiles'] >= 1
            # every float a workgroup of this layer writes lies inside the layer's part of ws: band partials [nb][N], t [R] behind them, one
            # float per tile in the backward; and of keep: sigma, u, v
            assert c['nb'] * 64 >= co and a[3] + c['nb'] * N + co <= b[3] and a[3] + c['tiles'] <= b[3] and a[3] % 4 == 0
            assert a[4] + 4 + R.cdiv(co, 4) * 4 + N <= b[4] and a[4] % 4 == 0
        # the large layers are spread over the machine: the 1024 x 5120 matrix takes hundreds of workgroups in every launch
    rows, totals = R.plan_ref(R.real_shapes())
    assert rows[7][0] - rows[6][0] >= 256 and rows[7][1] - rows[6][1] >= 256 and rows[7][2] - rows[6][2] >= 256


def _step(lib, arr, n, training, g, keep=FAKE, ws=FAKE + (1 << 30), ws_bytes=None, stream=DRY):
    return lib.v2w_sn_step(C.addressof(arr) if arr is not None else None, n, training, C.byref(g) if g is not None else None, keep, ws,
                           g.ws_bytes if ws_bytes is None else ws_bytes, stream)


def _ptrs(n, every=True):
    a, b = (_hip._fp * n)(), (_hip._fp * n)()
    for i in range(n):
        if every or i == 0:
            a[i], b[i] = FAKE + (4 << 30) + i * (1 << 28), FAKE + (8 << 30) + i * (1 << 28)
    return a, b


def test_name_sink_reports_the_kernels_and_the_launch_counts_do_not_grow_with_the_layers():
    lib = _hip.load()
    for shapes in [R.cases(), R.real_shapes()] + [[s] for s in R.cases()]:
        n = len(shapes)
        arr, g, rc = _planned(shapes)
        assert rc > 0
        dev = C.addressof(arr)
        rc, names = _hip.kernel_names(lib.v2w_sn_step, dev, n, 1, C.byref(g), FAKE, FAKE + (1 << 30), g.ws_bytes)
        assert rc in (0, 100) and names == STEP_KERNELS and len(names) <= 4, names
        rc, names = _hip.kernel_names(lib.v2w_sn_step, dev, n, 0, C.byref(g), FAKE, FAKE + (1 << 30), g.ws_bytes)
        assert rc in (0, 100) and names == STEP_KERNELS[2:], names
        a, b = _ptrs(n)
        rc, names = _hip.kernel_names(lib.v2w_sn_bwd, dev, n, C.byref(g), FAKE, a, b, FAKE + (1 << 30), g.ws_bytes)
        assert rc in (0, 100) and names == BWD_KERNELS and len(names) <= 2, names
        assert _step(lib, arr, n, 1, g) == 0 and lib.v2w_sn_bwd(dev, n, C.byref(g), FAKE, a, b, FAKE + (1 << 30), g.ws_bytes, DRY) == 0


def test_entry_points_refuse_bad_arguments_with_an_error_code():
    lib = _hip.load()
    M = _hip.SN_MAX_LAYERS
    g = _hip.SnGrids()
    assert lib.v2w_sn_plan(_descs([(3, 2, 5)] * M), M, C.byref(g)) > 0
    assert lib.v2w_sn_plan(_descs([(3, 2, 5)] * (M + 1)), M + 1, C.byref(g)) == _hip.E_ARG
    assert lib.v2w_sn_plan(_descs([(3, 2, 5)]), 0, C.byref(g)) == _hip.E_ARG
    assert lib.v2w_sn_plan(None, 1, C.byref(g)) == _hip.E_ARG and lib.v2w_sn_plan(_descs([(3, 2, 5)]), 1, None) == _hip.E_ARG
    for bad in ((0, 2, 5), (3, 0, 5), (3, 2, 0), (-1, 2, 5)):
        assert lib.v2w_sn_plan(_descs([(3, 2, 5), bad]), 2, C.byref(g)) == _hip.E_ARG, bad
    assert lib.v2w_sn_plan(_descs([(1 << 16, 1 << 15, 1)]), 1, C.byref(g)) == _hip.E_SHAPE
    for field in ('w', 'u', 'v', 'wf'):
        arr = _descs([(3, 2, 5), (4, 1, 3)])
        setattr(arr[1], field, None)
        assert lib.v2w_sn_plan(arr, 2, C.byref(g)) == _hip.E_ARG, field
        arr = _descs([(3, 2, 5), (4, 1, 3)])
        setattr(arr[1], field, getattr(arr[1], field) + 2)
        assert lib.v2w_sn_plan(arr, 2, C.byref(g)) == _hip.E_ARG, field
    shapes = [(17, 3, 5), (64, 2, 2)]
    arr, g, rc = _planned(shapes)
    assert rc > 0 and _step(lib, arr, 2, 1, g) == 0
    assert _step(lib, None, 2, 1, g) == _hip.E_ARG and _step(lib, arr, 2, 1, g, keep=None) == _hip.E_ARG
    assert _step(lib, arr, 2, 1, g, ws=None) == _hip.E_ARG
    assert lib.v2w_sn_step(C.addressof(arr), 2, 1, None, FAKE, FAKE, 1 << 20, DRY) == _hip.E_ARG
    assert _step(lib, arr, M + 1, 1, g) == _hip.E_ARG and _step(lib, arr, 0, 1, g) == _hip.E_ARG and _step(lib, arr, 1, 1, g) == _hip.E_ARG
    assert _step(lib, arr, 2, 1, g, ws=FAKE + 4) == _hip.E_ARG and _step(lib, arr, 2, 1, g, keep=FAKE + 8) == _hip.E_ARG
    assert _step(lib, arr, 2, 1, g, ws_bytes=g.ws_bytes - 4) == _hip.E_ARG
    dev = C.addressof(arr)
    a, b = _ptrs(2)
    ws = FAKE + (1 << 30)
    assert lib.v2w_sn_bwd(dev, 2, C.byref(g), FAKE, a, b, ws, g.ws_bytes, DRY) == 0
    assert lib.v2w_sn_bwd(dev, 2, C.byref(g), FAKE, *_ptrs(2, every=False), ws, g.ws_bytes, DRY) == 0           # a skipped layer
    assert lib.v2w_sn_bwd(None, 2, C.byref(g), FAKE, a, b, ws, g.ws_bytes, DRY) == _hip.E_ARG
    assert lib.v2w_sn_bwd(dev, 2, C.byref(g), None, a, b, ws, g.ws_bytes, DRY) == _hip.E_ARG
    assert lib.v2w_sn_bwd(dev, 2, C.byref(g), FAKE, None, b, ws, g.ws_bytes, DRY) == _hip.E_ARG
    assert lib.v2w_sn_bwd(dev, 2, C.byref(g), FAKE, a, None, ws, g.ws_bytes, DRY) == _hip.E_ARG
    assert lib.v2w_sn_bwd(dev, M + 1, C.byref(g), FAKE, a, b, ws, g.ws_bytes, DRY) == _hip.E_ARG
    none = ((_hip._fp * 2)(), (_hip._fp * 2)())
    assert lib.v2w_sn_bwd(dev, 2, C.byref(g), FAKE, *none, ws, g.ws_bytes, DRY) == _hip.E_ARG                      # nothing to do
    half = _ptrs(2)
    half[1][1] = None
    assert lib.v2w_sn_bwd(dev, 2, C.byref(g), FAKE, *half, ws, g.ws_bytes, DRY) == _hip.E_ARG                      # dwf without dw
    # a refused call reports no kernel
    assert _hip.kernel_names(lib.v2w_sn_step, dev, 2, 1, C.byref(g), None, ws, g.ws_bytes) == (_hip.E_ARG, [])


def test_wrappers_refuse_what_they_cannot_hand_to_the_kernels():
    w, u, v, wf = torch.zeros(3, 2, 5), torch.zeros(3), torch.zeros(10), torch.zeros(5, 2, 3)
    with pytest.raises(RuntimeError, match='must live on a GPU'):
        hipops.sn_step([(w, u, v, wf)], True)
    with pytest.raises(ValueError):
        hipops.sn_step([], True)


# ---- the restatement against torch
def _sn_module(conv2d, dtype=torch.float64):
    torch.manual_seed(5 + conv2d)
    m = torch.nn.Conv2d(6, 7, (5, 1), groups=1) if conv2d else torch.nn.Conv1d(6, 8, 5, groups=2)
    return torch.nn.utils.spectral_norm(m.to(dtype))


@pytest.mark.parametrize('conv2d', [False, True])
def test_restatement_is_pinned_to_legacy_spectral_norm(conv2d):
    """Two consecutive training forwards, then two eval forwards, of torch.nn.utils.spectral_norm in fp64 on a grouped Conv1d and a Conv2d
    (k, 1) weight: u, v, the normalised weight and autograd's gradient of weight_orig after each, against sn_ref from the same state."""
    m = _sn_module(conv2d)
    x = torch.randn(2, 6, 40, 3, dtype=torch.float64) if conv2d else torch.randn(2, 6, 40, dtype=torch.float64)
    gen = torch.Generator().manual_seed(9)
    for training in (True, True, False, False):
        m.train(training)
        w0 = m.weight_orig.detach().numpy().copy()
        w3 = w0.reshape(w0.shape[0], w0.shape[1], w0.shape[2])
        u0, v0 = m.weight_u.numpy().copy(), m.weight_v.numpy().copy()
        m.weight_orig.grad = None
        m(x)
        G = torch.randn(m.weight.shape, generator=gen, dtype=torch.float64)
        (m.weight * G).sum().backward()
        r = R.step_ref(w3, u0, v0, training)
        if not training:
            assert np.array_equal(m.weight_u.numpy(), u0) and np.array_equal(m.weight_v.numpy(), v0)
        assert np.abs(m.weight_u.numpy() - r['u']).max() <= 1e-13 and np.abs(m.weight_v.numpy() - r['v']).max() <= 1e-13
        got_wf = m.weight.detach().numpy().reshape(w3.shape).transpose(2, 1, 0)
        assert np.abs(got_wf - r['wf']).max() <= 1e-12 * np.abs(r['wf']).max()
        dwf = G.numpy().reshape(w3.shape).transpose(2, 1, 0)
        dw, _E = R.bwd_ref(dwf, w3, r['u'], r['v'], r['sigma'])
        want = m.weight_orig.grad.numpy().reshape(w3.shape)
        assert np.abs(dw - want).max() <= 1e-11 * np.abs(want).max()


def test_restatement_reproduces_the_references_recorded_buffers():
    """tests/golden/disc_msd_b2_t8192_train.npz: weight_u / weight_v of the reference's spectral-normed DiscriminatorS after one training
    forward(y, y_hat) - two power iterations from the state dict's buffers."""
    z, meta = golden_util.load_golden('disc_msd_b2_t8192_train')
    sd, _y, _yh = golden_util.disc_case_setup(meta)
    keys = [k[4:] for k in z.files if k.startswith('buf_') and k.endswith('weight_u')]
    assert len(keys) == 8
    for ku in keys:
        base = ku[:-len('weight_u')]
        w = sd[base + 'weight_orig'].numpy()
        u, v = sd[ku].numpy(), sd[base + 'weight_v'].numpy()
        for _ in range(2):
            r = R.step_ref(w, u, v, True)
            u, v = r['u'], r['v']
        assert np.abs(u - z['buf_' + ku]).max() <= 1e-5 and np.abs(v - z['buf_' + base + 'weight_v']).max() <= 1e-5, base


def test_the_bound_holds_for_a_numpy_fp32_evaluation_and_sees_a_wrong_step():
    """The step evaluated with numpy float32 matrix products (another summation order, the same number of terms) stays inside the bounds on
    the small cases; a step that skips the u update, or divides by sigma^2, misses them by far."""
    rng = np.random.default_rng(R.SEED)
    f = np.float32
    for shape in R.EDGE_SHAPES + R.real_shapes()[:3]:
        w, u, v, dwf = R.make_case(shape, rng)
        W = w.reshape(shape[0], -1)
        r = R.step_ref(w, u, v, True)
        a = W.T @ u
        v1 = a / max(np.sqrt((a * a).sum(dtype=f)), f(R.EPS))
        t = W @ v1
        u1 = t / max(np.sqrt((t * t).sum(dtype=f)), f(R.EPS))
        sigma = (u1 * t).sum(dtype=f)
        assert a.dtype == v1.dtype == t.dtype == u1.dtype == sigma.dtype == f
        assert R.worst_ratio(v1, r['v'], r['E']['v']) <= 1.0 and R.worst_ratio(u1, r['u'], r['E']['u']) <= 1.0
        assert R.worst_ratio(sigma, r['sigma'], r['E']['sigma']) <= 1.0
        assert R.worst_ratio((w.transpose(2, 1, 0) / sigma).astype(f), r['wf'], r['E']['wf']) <= 1.0
        if shape[0] > 1:
            assert R.worst_ratio(u, r['u'], r['E']['u']) >= 100.0                      # u not updated
        assert R.worst_ratio(w.transpose(2, 1, 0) / (sigma * sigma), r['wf'], r['E']['wf']) >= 100.0
        along = np.ascontiguousarray(w.transpose(2, 1, 0))                            # a gradient along W itself: sum(dwf . w) = ||W||^2
        dw, E = R.bwd_ref(along, w, u1, v1, sigma)
        assert R.worst_ratio(w.astype(np.float64) / sigma, dw, E) >= 100.0             # the projection term left out
        dw, E = R.bwd_ref(dwf, w, u1, v1, sigma)
        assert R.worst_ratio(dwf.transpose(2, 1, 0).astype(np.float64) / (sigma * sigma), dw, E) >= 100.0 or abs(sigma - 1) < 1e-3


def test_eps_branch_case_stays_finite_in_fp64_and_in_torchs_fp32():
    """The GPU test's eps case: a 17 x 15 matrix of entries ~1e-14, so that ||W^T u|| < 1e-12 takes max(., eps).  For its seed both the
    restatement and torch's own fp32 lines give finite, non-zero u, v, sigma."""
    rng = np.random.default_rng(R.SEED + 1)
    w, u, v, _ = R.make_case((17, 3, 5), rng, scale=1e-14)
    r = R.step_ref(w, u, v, True)
    W = w.reshape(17, 15).astype(np.float64)
    assert np.linalg.norm(W.T @ u) < R.EPS and np.linalg.norm(W @ r['v']) < R.EPS
    assert all(np.isfinite(r[k]).all() for k in ('u', 'v', 'sigma')) and r['sigma'] > 0 and np.abs(r['u']).max() > 0
    wt, ut = torch.from_numpy(w).reshape(17, 15), torch.from_numpy(u)
    vt = torch.nn.functional.normalize(torch.mv(wt.t(), ut), dim=0, eps=1e-12)
    ut = torch.nn.functional.normalize(torch.mv(wt, vt), dim=0, eps=1e-12)
    st = torch.dot(ut, torch.mv(wt, vt))
    assert torch.isfinite(vt).all() and torch.isfinite(ut).all() and torch.isfinite(st) and st.item() > 0
    assert R.worst_ratio(vt.numpy(), r['v'], r['E']['v']) <= 1.0 and R.worst_ratio(ut.numpy(), r['u'], r['E']['u']) <= 1.0


def test_discriminators_carry_the_switch_and_no_raw_abi_call():
    from wavthruvec_pytorch_amd import discriminators as D
    assert D.NATIVE_SN is True
    src = open(os.path.join(ROOT, 'wavthruvec_pytorch_amd', 'discriminators.py')).read()
    assert src.index('NATIVE_SN = True') > src.index("BATCH_PAIRS = 'auto'")
    assert not re.search(r'_hip\.load\(\)|\.v2w_', src)
    msd = D.MultiScaleDiscriminator()
    from wavthruvec_pytorch_amd import synthetic
    assert list(msd.state_dict().keys()) == [k for k, _, _ in synthetic.msd_state_dict_spec()]
