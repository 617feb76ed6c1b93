"""GPU tests of the spectral-norm entry points (v2w_sn_step / v2w_sn_bwd) and of discriminators.NATIVE_SN.

Kernel level: every case of tests/sn_ref.py (the eight weight_orig shapes of the spectral-normed DiscriminatorS and the edge shapes) runs
through the C ABI on NaN-filled buffers with guards on both sides of every tensor, in ONE 13-layer launch and again layer by layer.  v, u,
sigma, wf and dw are held per entry to 2^-24 * E against the fp64 restatement, E built in sn_ref from the rounding counts the header lists
(a sum with n roundings on its longest path: n * S, S the summed magnitudes of its terms; quotients, norms and the chained sums propagate
these to first order - sn_ref's docstring has the rules).  The second step's bound chains the first's.  Nothing here was fitted to what
the kernels give; the worst ratios are printed.

End to end: MultiScaleDiscriminator with NATIVE_SN on against off, and a run with torch.mv / dot / outer / normalize patched to raise.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import disc_oracle as D
from tests import sn_ref as R
from wavthruvec_pytorch_amd import _hip, synthetic

pytestmark = pytest.mark.gpu
TOL = 1e-4      # tests/test_hip_discriminators.py: the bar on O(1) feature maps
GUARD = 64      # floats on both sides of every tensor (keeps 16-byte alignment)


@pytest.fixture(scope='module')
def dev():
    _hip.load()
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


class Guarded:
    """A NaN-filled device buffer with `n` payload floats between two guards."""

    def __init__(self, n, dev, data=None):
        self.n = n
        self.buf = torch.full((n + 2 * GUARD,), float('nan'), device=dev)
        self.t = self.buf[GUARD:GUARD + n]
        if data is not None:
            self.t.copy_(torch.from_numpy(np.ascontiguousarray(data).reshape(-1)))

    def ptr(self):
        return self.t.data_ptr()

    def guards_intact(self):
        g = torch.cat([self.buf[:GUARD], self.buf[GUARD + self.n:]]).view(torch.int32)
        return bool((g == g[0]).all()) and bool(torch.isnan(self.buf[0]))

    def bits(self):
        return self.buf.view(torch.int32).clone()

    def np(self):
        return self.t.cpu().numpy()


class Launch:
    """One planned layer set on the device: fresh guarded u, v, wf, dw, keep, ws; w and dwf are shared (read-only)."""

    def __init__(self, shapes, ws_in, dwf_in, us, vs, dev):
        self.shapes, self.n, self.dev = shapes, len(shapes), dev
        self.w, self.dwf = ws_in, dwf_in
        self.u = [Guarded(co, dev, u) for (co, ci, k), u in zip(shapes, us)]
        self.v = [Guarded(ci * k, dev, v) for (co, ci, k), v in zip(shapes, vs)]
        self.wf = [Guarded(co * ci * k, dev) for co, ci, k in shapes]
        self.dw = [Guarded(co * ci * k, dev) for co, ci, k in shapes]
        descs = (_hip.SnDesc * self.n)()
        for i, (d, (co, ci, k)) in enumerate(zip(descs, shapes)):
            d.w, d.u, d.v, d.wf = self.w[i].ptr(), self.u[i].ptr(), self.v[i].ptr(), self.wf[i].ptr()
            d.c_out, d.c_in, d.k = co, ci, k
        self.g = _hip.SnGrids()
        assert _hip.load().v2w_sn_plan(descs, self.n, C.byref(self.g)) == self.g.ws_bytes > 0
        self.keep_off = [int(d.keep_off) for d in descs]
        self.descs_dev = torch.frombuffer(bytearray(bytes(descs)), dtype=torch.uint8).to(dev)
        self.ws = Guarded(self.g.ws_bytes // 4, dev)
        self.keep = Guarded(self.g.keep_bytes // 4, dev)
        self.stream = torch.cuda.current_stream(dev).cuda_stream

    def step(self, training):
        _hip.check(_hip.load().v2w_sn_step(self.descs_dev.data_ptr(), self.n, int(training), C.byref(self.g), self.keep.ptr(), self.ws.ptr(),
                                           self.g.ws_bytes, self.stream), 'v2w_sn_step')

    def bwd(self):
        a, b = (_hip._fp * self.n)(), (_hip._fp * self.n)()
        for i in range(self.n):
            a[i], b[i] = self.dwf[i].ptr(), self.dw[i].ptr()
        _hip.check(_hip.load().v2w_sn_bwd(self.descs_dev.data_ptr(), self.n, C.byref(self.g), self.keep.ptr(), a, b, self.ws.ptr(),
                                          self.g.ws_bytes, self.stream), 'v2w_sn_bwd')

    def kept(self, i):
        co, ci, k = self.shapes[i]
        o = self.keep_off[i]
        kp = self.keep.t
        ou, ov = o + 4, o + 4 + R.cdiv(co, 4) * 4
        return kp[o].item(), kp[ou:ou + co].cpu().numpy(), kp[ov:ov + ci * k].cpu().numpy()

    def keep_padding_is_nan(self):
        """The floats of the keep slab that belong to no sigma, u or v stay as they were."""
        used = torch.zeros(self.keep.n, dtype=torch.bool)
        for (co, ci, k), o in zip(self.shapes, self.keep_off):
            ov = o + 4 + R.cdiv(co, 4) * 4
            used[o] = True
            used[o + 4:o + 4 + co] = True
            used[ov:ov + ci * k] = True
        kp = self.keep.t.cpu()
        return bool(torch.isnan(kp[~used]).all()) and not bool(torch.isnan(kp[used]).any())

    def all_guards_intact(self):
        return all(x.guards_intact() for x in self.u + self.v + self.wf + self.dw + self.w + self.dwf + [self.ws, self.keep])


@pytest.fixture(scope='module')
def run(dev):
    """Everything the kernel-level tests look at, computed once: the inputs, the 13-layer launch through two training steps, an eval step
    and the backward, and the fp64 references."""
    rng = np.random.default_rng(R.SEED)
    shapes = R.cases()
    inputs = [R.make_case(s, rng) for s in shapes]
    w = [Guarded(x[0].size, dev, x[0]) for x in inputs]
    dwf = [Guarded(x[3].size, dev, x[3]) for x in inputs]
    us, vs = [x[1] for x in inputs], [x[2] for x in inputs]
    out = dict(shapes=shapes, inputs=inputs, w=w, dwf=dwf, us=us, vs=vs)
    L = Launch(shapes, w, dwf, us, vs, dev)
    L.step(True)
    torch.cuda.synchronize()
    out['step1'] = dict(u=[x.np() for x in L.u], v=[x.np() for x in L.v], wf=[x.np() for x in L.wf], kept=[L.kept(i) for i in range(L.n)],
                        guards=L.all_guards_intact(), keep_pad=L.keep_padding_is_nan())
    L.bwd()
    torch.cuda.synchronize()
    out['bwd1'] = dict(dw=[x.np() for x in L.dw], guards=L.all_guards_intact())
    L.step(True)
    torch.cuda.synchronize()
    out['step2'] = dict(u=[x.np() for x in L.u], v=[x.np() for x in L.v], wf=[x.np() for x in L.wf], kept=[L.kept(i) for i in range(L.n)])
    ubits, vbits = [x.bits() for x in L.u], [x.bits() for x in L.v]
    L.step(False)
    torch.cuda.synchronize()
    out['eval'] = dict(u_same=all(torch.equal(a, x.bits()) for a, x in zip(ubits, L.u)), v_same=all(torch.equal(a, x.bits()) for a, x in zip(vbits, L.v)),
                       wf=[x.np() for x in L.wf], kept=[L.kept(i) for i in range(L.n)], guards=L.all_guards_intact())
    out['L'] = L
    refs = []
    for (wi, ui, vi, _d) in inputs:
        r1 = R.step_ref(wi, ui, vi, True)
        r2 = R.step_ref(wi, r1['u'], r1['v'], True, Eu=r1['E']['u'], Ev=r1['E']['v'])
        refs.append((r1, r2))
    out['refs'] = refs
    return out


def _worst(run, key, ref_index):
    worst = {}
    for i, shape in enumerate(run['shapes']):
        r = run['refs'][i][ref_index]
        got = run[key]
        sigma = got['kept'][i][0]
        ratios = dict(v=R.worst_ratio(got['v'][i], r['v'], r['E']['v']), u=R.worst_ratio(got['u'][i], r['u'], r['E']['u']),
                      sigma=R.worst_ratio(sigma, r['sigma'], r['E']['sigma']),
                      wf=R.worst_ratio(got['wf'][i].reshape(r['wf'].shape), r['wf'], r['E']['wf']))
        assert all(np.isfinite(x) for x in ratios.values()), (shape, ratios)
        worst[shape] = ratios
    return worst


def test_training_step_matches_fp64_per_entry_and_writes_nothing_else(run):
    worst = _worst(run, 'step1', 0)
    print('step 1 worst |err| / bound:', {k: max(w[k] for w in worst.values()) for k in ('v', 'u', 'sigma', 'wf')})
    for shape, ratios in worst.items():
        assert max(ratios.values()) <= 1.0, (shape, ratios)
    assert run['step1']['guards'] and run['step1']['keep_pad']
    for i in range(len(run['shapes'])):            # the kept copies are the in-place results, bit for bit
        _s, uk, vk = run['step1']['kept'][i]
        assert np.array_equal(uk.view(np.int32), run['step1']['u'][i].view(np.int32))
        assert np.array_equal(vk.view(np.int32), run['step1']['v'][i].view(np.int32))


def test_two_training_steps_equal_two_fp64_iterations(run):
    worst = _worst(run, 'step2', 1)
    print('step 2 worst |err| / bound:', {k: max(w[k] for w in worst.values()) for k in ('v', 'u', 'sigma', 'wf')})
    for shape, ratios in worst.items():
        assert max(ratios.values()) <= 1.0, (shape, ratios)
    for i in range(len(run['shapes'])):            # the second step did move u and v
        if run['shapes'][i][0] > 1:
            assert not np.array_equal(run['step2']['u'][i], run['step1']['u'][i])


def test_eval_step_leaves_u_v_untouched_and_matches_fp64(run):
    assert run['eval']['u_same'] and run['eval']['v_same'] and run['eval']['guards']
    worst = 0.0
    for i, (wi, _u, _v, _d) in enumerate(run['inputs']):
        u, v = run['step2']['u'][i], run['step2']['v'][i]
        r = R.step_ref(wi, u, v, False)
        sigma, uk, vk = run['eval']['kept'][i]
        assert np.array_equal(uk.view(np.int32), u.view(np.int32)) and np.array_equal(vk.view(np.int32), v.view(np.int32))
        worst = max(worst, R.worst_ratio(sigma, r['sigma'], r['E']['sigma']),
                    R.worst_ratio(run['eval']['wf'][i].reshape(r['wf'].shape), r['wf'], r['E']['wf']))
    print('eval worst |err| / bound:', worst)
    assert worst <= 1.0


def test_backward_matches_fp64_per_entry(run):
    worst = 0.0
    for i, (wi, _u, _v, dwf) in enumerate(run['inputs']):
        sigma, uk, vk = run['step1']['kept'][i]
        dw, E = R.bwd_ref(dwf, wi, uk, vk, sigma)
        got = run['bwd1']['dw'][i].reshape(dw.shape)
        assert np.isfinite(got).all()
        ratio = R.worst_ratio(got, dw, E)
        assert ratio <= 1.0, (run['shapes'][i], ratio)
        worst = max(worst, ratio)
    print('backward worst |err| / bound:', worst)
    assert run['bwd1']['guards']


def test_one_launch_equals_single_layer_launches_and_repeats_bit_for_bit(run, dev):
    """Each layer alone (n = 1) gives the bits it gave inside the 13-layer launch; the eight real layers as one 8-layer launch too; a second
    run of the same launch repeats the first."""
    shapes = run['shapes']

    def same(L, idx):
        L.step(True)
        L.bwd()
        torch.cuda.synchronize()
        for j, i in enumerate(idx):
            s1 = run['step1']
            for got, want in ((L.u[j].np(), s1['u'][i]), (L.v[j].np(), s1['v'][i]), (L.wf[j].np(), s1['wf'][i]), (L.dw[j].np(), run['bwd1']['dw'][i])):
                assert np.array_equal(got.view(np.int32), want.view(np.int32)), (shapes[i], idx)
            assert np.float32(L.kept(j)[0]).view(np.int32) == np.float32(s1['kept'][i][0]).view(np.int32)
        assert L.all_guards_intact()

    for i in range(len(shapes)):
        same(Launch([shapes[i]], [run['w'][i]], [run['dwf'][i]], [run['us'][i]], [run['vs'][i]], dev), [i])
    real = list(range(len(R.real_shapes())))
    pick = lambda xs: [xs[i] for i in real]          # noqa: E731
    same(Launch(pick(shapes), pick(run['w']), pick(run['dwf']), pick(run['us']), pick(run['vs']), dev), real)
    every = list(range(len(shapes)))
    same(Launch(shapes, run['w'], run['dwf'], run['us'], run['vs'], dev), every)


def test_eps_branch(dev):
    """A 17 x 15 matrix of entries ~1e-14: ||W^T u|| and ||W v|| are below 1e-12, both divisions take max(., eps).  u, v, sigma only."""
    rng = np.random.default_rng(R.SEED + 1)
    shape = (17, 3, 5)
    w, u, v, dwf = R.make_case(shape, rng, scale=1e-14)
    r = R.step_ref(w, u, v, True)
    assert np.linalg.norm(w.reshape(17, 15).astype(np.float64).T @ u) < R.EPS
    L = Launch([shape], [Guarded(w.size, dev, w)], [Guarded(dwf.size, dev, dwf)], [u], [v], dev)
    L.step(True)
    torch.cuda.synchronize()
    sigma = L.kept(0)[0]
    ratios = (R.worst_ratio(L.v[0].np(), r['v'], r['E']['v']), R.worst_ratio(L.u[0].np(), r['u'], r['E']['u']), R.worst_ratio(sigma, r['sigma'], r['E']['sigma']))
    print('eps case |err| / bound:', ratios)
    assert np.isfinite(L.u[0].np()).all() and np.isfinite(L.v[0].np()).all() and np.isfinite(sigma) and sigma > 0
    assert max(ratios) <= 1.0 and L.all_guards_intact()


# ---- end to end
def _msd(dev, training=True):
    from wavthruvec_pytorch_amd.discriminators import MultiScaleDiscriminator
    m = MultiScaleDiscriminator()
    m.load_state_dict(synthetic.make_disc_state_dict(synthetic.msd_state_dict_spec(), seed=21))
    m = m.to(dev)
    return m.train() if training else m.eval()


def _msd_run(dev, native, monkeypatch):
    from wavthruvec_pytorch_amd import discriminators
    monkeypatch.setattr(discriminators, 'NATIVE_SN', native)
    y, y_hat = synthetic.make_audio_pair(2, 3001, seed=6)
    m = _msd(dev)
    outs = m(y.to(dev), y_hat.to(dev).requires_grad_(True))
    D.mixed_loss(outs).backward()
    torch.cuda.synchronize()
    return m, outs


def test_msd_native_spectral_norm_equals_the_torch_lines(dev, monkeypatch):
    (m1, o1), (m0, o0) = _msd_run(dev, True, monkeypatch), _msd_run(dev, False, monkeypatch)
    for a, b in zip(o1[0] + o1[1], o0[0] + o0[1]):
        assert a.shape == b.shape and (a - b).abs().max().item() <= TOL
    for fa, fb in zip(o1[2] + o1[3], o0[2] + o0[3]):
        for a, b in zip(fa, fb):
            assert a.shape == b.shape and (a - b).abs().max().item() <= TOL
    sd1, sd0 = m1.state_dict(), m0.state_dict()
    assert list(sd1) == list(sd0) == [k for k, _, _ in synthetic.msd_state_dict_spec()]
    moved = 0
    for k in sd1:
        if k.endswith('weight_u') or (k.endswith('weight_v') and k.replace('weight_v', 'weight_orig') in sd1):
            assert (sd1[k] - sd0[k]).abs().max().item() <= 1e-5, k
            moved += 1
    assert moved == 16
    g0 = dict(m0.named_parameters())
    for k, p in m1.named_parameters():
        ref = g0[k].grad
        assert p.grad is not None and ref is not None and p.grad.shape == ref.shape, k
        # the bar of test_discriminator_backward_matches_oracle_autograd
        assert (p.grad - ref).abs().max().item() / max(ref.abs().max().item(), 1e-9) <= 5e-4, k


def test_msd_runs_without_torchs_mv_dot_outer_normalize(dev, monkeypatch):
    """With NATIVE_SN on, no spectral-norm arithmetic is left to torch: a train-mode forward + backward and an eval forward complete with
    torch.mv, torch.dot, torch.outer and F.normalize patched to raise, and the forward's launches include the new kernels."""
    from wavthruvec_pytorch_amd import discriminators, hipops
    assert discriminators.NATIVE_SN is True

    def refuse(name):
        def fn(*a, **k):
            raise AssertionError(f'torch.{name} called: the spectral norm is meant to run on the C ABI')
        return fn

    m, me = _msd(dev), _msd(dev, training=False)
    for name in ('mv', 'dot', 'outer'):
        monkeypatch.setattr(torch, name, refuse(name))
    monkeypatch.setattr(torch.nn.functional, 'normalize', refuse('nn.functional.normalize'))
    steps = []
    real_step = hipops.sn_step

    def spy(layers, training):
        plan, keep = real_step(layers, training)
        lib = _hip.load()
        rc, names = _hip.kernel_names(lib.v2w_sn_step, plan.descs_dev.data_ptr(), plan.n, int(training), C.byref(plan.grids), keep.data_ptr(),
                                      plan.ws.data_ptr(), plan.grids.ws_bytes)
        steps.append((plan.n, bool(training), rc, names))
        return plan, keep

    monkeypatch.setattr(hipops, 'sn_step', spy)
    y, y_hat = synthetic.make_audio_pair(2, 3001, seed=6)
    outs = m(y.to(dev), y_hat.to(dev).requires_grad_(True))
    D.mixed_loss(outs).backward()
    with torch.no_grad():
        me(y.to(dev), y_hat.to(dev))
        me(y.to(dev), y_hat.to(dev))
    torch.cuda.synchronize()
    assert all(torch.isfinite(p.grad).all() for p in m.parameters())
    # train: one 8-layer step per call (y, y_hat); eval: one step at the first call, the cached weights afterwards
    assert [(n, tr) for n, tr, _rc, _names in steps] == [(8, True), (8, True), (8, False)], steps
    assert steps[0][3] == ['sn_wtu_kernel', 'sn_v_kernel', 'sn_wv_kernel', 'sn_scale_kernel'] and steps[2][3] == ['sn_wv_kernel', 'sn_scale_kernel']
    assert all(rc == 0 for _n, _t, rc, _names in steps)
