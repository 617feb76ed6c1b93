"""CPU tests of the GAN loss entry points (v2w_l1_mean_multi / v2w_lsgan_multi and their backwards): the C ABI surface, the host-only work
split against a restatement in Python, what the name sink reports, what the entry points refuse, and the stride -> (rows, valid, pitch)
derivation of hipops.loss_rows.  No GPU needed: nothing is launched."""
import ctypes as C
import os
import re

import pytest
import torch

from wavthruvec_pytorch_amd import _hip, hipops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('v2w_l1_multi_plan', 'v2w_l1_multi_scratch_bytes', 'v2w_l1_mean_multi', 'v2w_l1_mean_multi_bwd', 'v2w_lsgan_multi', 'v2w_lsgan_multi_bwd')
FAKE = 0x7f0000100000       # 16-byte aligned "device" pointers: the plan and the name sink never dereference them


def _header():
    return open(os.path.join(ROOT, 'include', 'vec2wav_hip.h')).read()


def _struct_fields(hdr, name):
    body = hdr[:hdr.index('} %s;' % name)]
    body = body[body.rindex('typedef struct {'):]
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    return re.findall(r'\b(\w+)(?:\[\d+\])?\s*[;,]', body)


def test_loss_entry_points_are_declared_bound_and_additive():
    hdr = _header()
    assert int(re.search(r'#define V2W_ABI_VERSION (\d+)', hdr).group(1)) == _hip.ABI_VERSION == 35 == _hip.load().v2w_abi_version()
    for name in NAMES:
        assert name in _hip.SIGNATURES and re.search(r'\b%s\s*\(' % name, hdr), name
        assert (name in _hip.LAUNCHERS) == (name not in ('v2w_l1_multi_plan', 'v2w_l1_multi_scratch_bytes')), name
    assert _struct_fields(hdr, 'v2w_l1_pair') == [n for n, _ in _hip.L1Pair._fields_]
    assert _struct_fields(hdr, 'v2w_lsgan_item') == [n for n, _ in _hip.LsganItem._fields_]
    assert C.sizeof(_hip.L1Pair) == 56 and C.sizeof(_hip.LsganItem) == 40
    assert int(re.search(r'#define V2W_LOSS_MAX_ITEMS\s+(\d+)', hdr).group(1)) == _hip.LOSS_MAX_ITEMS >= 64
    assert int(re.search(r'#define V2W_L1_TARGET_WGS\s+(\d+)', hdr).group(1)) == _hip.L1_TARGET_WGS


def _pairs(shapes, base=FAKE, off_a=0):
    """shapes: (rows, valid, pitch_a, pitch_b) -> descriptor array on fake pointers (`off_a`: bytes added to every a)."""
    arr = (_hip.L1Pair * len(shapes))()
    for d, (rows, valid, pa, pb) in zip(arr, shapes):
        d.a, d.b, d.da, d.db = base + off_a, base + 0x40000000, base + 0x80000000, base + 0xc0000000
        d.rows, d.valid, d.pitch_a, d.pitch_b = rows, valid, pa, pb
    return arr


def _plan_restated(shapes, shift=0):
    """include/vec2wav_hip.h, v2w_l1_multi_plan: units of four floats, a chunk that deals about L1_TARGET_WGS workgroups, >= 1 per pair."""
    units = []
    for rows, valid, pa, pb in shapes:
        dense = (pa in (0, valid) and pb in (0, valid)) or rows == 1
        units.append((rows * valid + shift + 3) // 4 if dense else rows * ((valid + 3) // 4))
    chunk = max(2048, -(-sum(units) // _hip.L1_TARGET_WGS))
    starts = [0]
    for u in units:
        starts.append(starts[-1] + max(1, -(-u // chunk)))
    return starts


# the element counts of one feature-loss call: four orders of magnitude; numel = 1; pitched rows with a tail; a >2^31-float dense pair
CASES = {
    'tiny': [(1, 1, 0, 0)],
    'test_shapes': [(1, 1, 0, 0), (1, 4099, 4099, 0), (6, 13, 16, 16), (32, 20, 20, 20), (15, 22, 24, 24), (8, 21, 24, 24), (192, 1000, 0, 1000)],
    'b32_mpd': [(32 * c, u, -(-u // 4) * 4, -(-u // 4) * 4) for c, u in ((32, 27307 * 3), (128, 9103 * 3), (512, 3035 * 3), (1024, 1012 * 3),
                                                                          (1024, 1012 * 3), (1, 1012 * 3))],
    'mixed': [(32 * 1024, 81920, 0, 81920), (7, 5, 8, 5), (3, 9, 9, 12), (1, 7, 0, 0)] + [(2, 3, 4, 4)] * 60,
}


@pytest.mark.parametrize('case', sorted(CASES))
def test_plan_matches_its_restatement(case):
    lib = _hip.load()
    shapes = CASES[case]
    n = len(shapes)
    arr = _pairs(shapes)
    starts = (C.c_int32 * (n + 1))()
    nwg = lib.v2w_l1_multi_plan(arr, n, starts)
    starts = list(starts)
    assert starts == _plan_restated(shapes) and nwg == starts[-1]
    assert starts[0] == 0 and all(b - a >= 1 for a, b in zip(starts, starts[1:]))             # monotone, every pair has a workgroup
    assert nwg <= _hip.L1_TARGET_WGS + n
    assert lib.v2w_l1_multi_scratch_bytes(arr, n) == 8 * nwg
    assert hipops.l1_plan(arr, n) == (starts, nwg)


def test_plan_counts_the_floats_before_an_unaligned_dense_pair():
    lib = _hip.load()
    shapes = [(1, 4 * 2048 * 3, 0, 0)]
    for off in (0, 4, 8, 12):
        starts = (C.c_int32 * 2)()
        assert lib.v2w_l1_multi_plan(_pairs(shapes, off_a=off), 1, starts) == _plan_restated(shapes, shift=off // 4)[-1] == (3 if off == 0 else 4)


def test_name_sink_lists_the_loss_kernels():
    lib = _hip.load()
    arr = _pairs(CASES['test_shapes'])
    n = len(arr)
    rc, names = _hip.kernel_names(lib.v2w_l1_mean_multi, arr, n, 2.0, FAKE, FAKE + 0x1000, FAKE + 0x2000)
    assert rc in (0, 100) and names == ['l1_multi_kernel<false>', 'l1_finish_kernel'], names
    rc, names = _hip.kernel_names(lib.v2w_l1_mean_multi_bwd, arr, n, 2.0, FAKE)
    assert rc in (0, 100) and names == ['l1_multi_kernel<true>'], names
    items = (_hip.LsganItem * 3)()
    for d, (rows, valid, pitch, t) in zip(items, ((1, 7, 0, 1.0), (2, 77, 80, 0.0), (2, 2731, 2731, 1.0))):
        d.s, d.ds, d.rows, d.valid, d.pitch, d.target = FAKE, FAKE + 0x100000, rows, valid, pitch, t
    rc, names = _hip.kernel_names(lib.v2w_lsgan_multi, items, 3, FAKE, FAKE + 0x100)
    assert rc in (0, 100) and names == ['lsgan_multi_kernel'], names
    rc, names = _hip.kernel_names(lib.v2w_lsgan_multi_bwd, items, 3, FAKE, None)
    assert rc in (0, 100) and names == ['lsgan_multi_bwd_kernel'], names


def test_entry_points_refuse_bad_descriptors_with_an_error_code():
    lib = _hip.load()
    ok = (6, 13, 16, 16)

    def fwd(shapes, n=None, **kw):
        arr = _pairs(shapes, **kw)
        return _hip.kernel_names(lib.v2w_l1_mean_multi, arr, len(shapes) if n is None else n, 1.0, FAKE, FAKE, FAKE)

    assert fwd([ok] * 64)[0] in (0, 100)
    assert fwd([ok] * 65) == (-1, [])                         # more than V2W_LOSS_MAX_ITEMS
    assert fwd([ok], n=0) == (-1, [])
    assert fwd([(6, 13, 14, 16)]) == (-1, [])                 # pitch % 4
    assert fwd([(6, 13, 12, 16)]) == (-1, [])                 # pitch < valid
    assert fwd([(6, 13, 16, 16)], off_a=4) == (-1, [])        # pitched rows off the 16-byte lines
    assert fwd([(6, 13, 13, 13)], off_a=4)[0] in (0, 100)     # dense: any alignment
    assert fwd([(0, 13, 16, 16)]) == (-1, []) and fwd([(6, 0, 16, 16)]) == (-1, [])
    arr = _pairs([ok])
    assert _hip.kernel_names(lib.v2w_l1_mean_multi, arr, 1, 1.0, FAKE, FAKE, None) == (-1, [])       # no scratch
    assert _hip.kernel_names(lib.v2w_l1_mean_multi_bwd, arr, 1, 1.0, None) == (-1, [])               # no gout
    arr[0].da = arr[0].db = None
    assert _hip.kernel_names(lib.v2w_l1_mean_multi_bwd, arr, 1, 1.0, FAKE) == (-1, [])               # nothing to write
    assert lib.v2w_l1_multi_scratch_bytes(_pairs([ok] * 65), 65) == -1
    item = (_hip.LsganItem * 1)()
    item[0].s, item[0].rows, item[0].valid, item[0].target = FAKE, 1, 7, 0.5
    assert _hip.kernel_names(lib.v2w_lsgan_multi, item, 1, FAKE, FAKE) == (-1, [])                   # targets are 0 or 1
    item[0].target = 1.0
    assert _hip.kernel_names(lib.v2w_lsgan_multi_bwd, item, 1, None, None) == (-1, [])
    assert _hip.kernel_names(lib.v2w_lsgan_multi, item, 65, FAKE, FAKE) == (-1, [])


def test_loss_rows_reads_the_discriminator_views_in_place():
    """Every form the discriminators return has a descriptor (no copy); what has none is reported as None (the wrappers then copy)."""
    assert hipops.loss_rows(torch.zeros(())) == (1, 1, 1)
    assert hipops.loss_rows(torch.zeros(4099)) == (1, 4099, 4099)
    buf = torch.zeros(2, 3, 16)
    assert hipops.loss_rows(buf[:, :, :13]) == (6, 13, 16)
    assert hipops.loss_rows(torch.zeros(4, 8, 20)) == (1, 640, 640)                        # valid == pitch: dense
    big = torch.zeros(6, 5, 24)[:, :, :22]
    assert hipops.loss_rows(big[:3]) == hipops.loss_rows(big[3:]) == (15, 22, 24)
    assert big[3:].data_ptr() - big.data_ptr() == 3 * 5 * 24 * 4
    v4 = torch.zeros(2, 4, 24)[:, :, :21].view(2, 4, 7, 3)
    assert hipops.loss_rows(v4) == (8, 21, 24) and hipops.loss_rows(v4[1:]) == (4, 21, 24)
    assert hipops.loss_rows(torch.zeros(3, 64, 1000)) == (1, 192000, 192000)
    # a pair is cut into the same rows on both sides: dense against pitched
    dense, pitched = torch.zeros(4, 8, 20), torch.zeros(4, 8, 24)[:, :, :20]
    assert hipops.loss_rows(dense, like=pitched) == (32, 20, 20) and hipops.loss_rows(pitched, like=dense) == (32, 20, 24)
    # size-1 dims carry no stride information: (B, 1, U) scores of a one-item half
    assert hipops.loss_rows(torch.zeros(2, 1, 16)[:, :, :5][:1]) == (1, 5, 5)
    assert hipops.loss_rows(torch.flatten(torch.zeros(4, 1, 16)[:, :, :5], 1, -1)[2:], aligned=False) == (2, 5, 16)
    # no row form: transposed, strided last dim, rows that are not one pitch apart, an expanded dim
    assert hipops.loss_rows(torch.zeros(4, 6).t()) is None
    assert hipops.loss_rows(torch.zeros(4, 6)[:, ::2]) is None
    assert hipops.loss_rows(torch.zeros(4, 6, 8)[:, :3, :5]) is None
    assert hipops.loss_rows(torch.zeros(1, 8).expand(4, 8)) is None
    # pitched rows the 16-byte loads cannot take: pitch % 4 != 0, or a base off the 16-byte lines; the LSGAN kernels take them
    odd = torch.zeros(2, 3, 15)[:, :, :13]
    assert hipops.loss_rows(odd) is None and hipops.loss_rows(odd, aligned=False) == (6, 13, 15)
    shifted = torch.zeros(2 * 3 * 16 + 1)[1:].view(2, 3, 16)[:, :, :13]
    assert hipops.loss_rows(shifted) is None and hipops.loss_rows(shifted, aligned=False) == (6, 13, 16)
    with pytest.raises(ValueError):
        hipops.loss_rows(torch.zeros(0, 3))
    with pytest.raises(ValueError):
        hipops.loss_rows(torch.zeros(2, 3), like=torch.zeros(3, 2))


def test_cpu_arguments_keep_the_torch_expressions():
    """CPU tensors never reach the library: same values and gradients as the expressions of models.py:278-310."""
    from wavthruvec_pytorch_amd import discriminators as D
    g = torch.Generator().manual_seed(0)
    fr = [[torch.randn(2, 3, 5, generator=g), torch.randn(2, 1, 4, generator=g)]]
    fg = [[torch.randn(2, 3, 5, generator=g).requires_grad_(), torch.randn(2, 1, 4, generator=g).requires_grad_()]]
    loss = D.feature_loss(fr, fg)
    want = 2 * sum(torch.mean(torch.abs(r - f)) for r, f in zip(fr[0], fg[0]))
    assert torch.equal(loss, want)
    loss.backward()
    assert torch.equal(fg[0][0].grad, torch.sign(fg[0][0].detach() - fr[0][0]) * (2 / 30))
    s = [torch.randn(2, 7, generator=g), torch.randn(2, 5, generator=g)]
    total, real, fake = D.discriminator_loss(s, s[::-1])
    assert isinstance(real[0], float) and len(real) == len(fake) == 2
    assert abs(total.item() - sum(real) - sum(fake)) < 1e-6
    total, terms = D.generator_loss(s)
    assert torch.equal(total, sum(terms)) and terms[0].dim() == 0
    a, b = torch.randn(2, 80, 32, generator=g), torch.randn(2, 80, 32, generator=g)
    assert torch.equal(D.l1_mean_loss(a, b), torch.nn.functional.l1_loss(a, b))
