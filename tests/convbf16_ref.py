"""fp64 CPU statement of what csrc/v2w_conv_bf16.hip computes (conv_bf16_kernel behind v2w_conv1d_fwd / _fwd_multi with V2W_ALGO_BF16 and
behind v2w_convt1d_bf16_fwd where the resident-tile kernel does not take the call; pack_bf16_convt_kernel behind v2w_pack_bf16_convt), as
include/vec2wav_hip.h documents the calls, and what each entry may differ by.  Sums, epilogue and magnitude sum S are tests/tile_ref.py's.

The value.  The kernel rounds both operands to bf16 (rne) and the products of two bf16 numbers are exact in fp32, so the statement is on
the ROUNDED operands and the rounding itself is emulated, not bounded:
  weights   rne_bf16(wf)
  signal    rne_bf16(lrelu(fmaf(in_a, x, in_s))) in fp32, the leaky-relu one fp32 multiply (`operand`); with bf16-stored input
            (io_bf16 bit 0) x is a bf16 number to begin with.
Without an input affine that is exact (one fp32 multiply, one rounding).  With one, t = in_a * x + in_s is formed in fp64 (the product is
exact there) and cast to fp32; that is the fma's result up to a double rounding one fp32 ulp away, so an element is ACCEPTED only when t and
both its fp32 neighbours, after the slope multiply, round to the same bf16 (`ambiguous`), and the offenders are redrawn on the CPU
(`redraw`, at most 64 rounds, none may be left).  The rejection window is a few fp32 ulps against the 2^16 ulps between bf16 rounding
boundaries: about 2^-14 of the elements per round.  No entry is excluded and no entry's bound is widened.

The bound, fp32-stored output (eps = 2^-24):   n * eps * S,   n = k * C_in + ops (a short-chain record: k + ops), ops counted per switch as
tests/tile_cases.OPS counts them (the input affine's fma once: its rounding is in the emulation, not counted a second time), S the summed
magnitudes of the entry's terms on the rounded operands, scaled by the epilogue as tile_ref.epilogue scales them.

bf16-stored output (io_bf16 bit 1).  Adding 2^-9 |value| would swamp everything the bound is for.  Rounding is monotone: the fp32 value g
the kernel holds before its store lies in [want - b, want + b], so g >= the smallest fp32 number at or above want - b, g <= the largest at
or below want + b, and the stored rne_bf16(g) lies between the rne_bf16 of those two (`store_interval`) - one or two bf16 numbers, rarely
more.  The reported ratio is the distance from `want` to the nearest real that rounds to what was stored, over b (`store_ratio`): <= 1
exactly when the stored value is inside the interval, 0 when it is rne_bf16(want) itself.  res / add0 / add1 / an accumulated `out` read
as bf16 are exact inputs.

stats_part of the transposed conv: sums of the values the launch itself stored, held to n * eps * sum |v| (sum v^2 for the squares), n the
NT * u output positions of a row - the rule of the tile suite's statistics rows (tests/test_tile_kernels_gpu._sum_rows_ok).

v2w_pack_bf16_convt is stated bit for bit from the comment above pack_bf16_convt_kernel (`pack_bf16_convt`)."""
import numpy as np
import torch

from tests import split_ref
from tests import tile_ref as R
from tests.disc_ref import U, f64

FRAG_UNIT = 2048                 # bytes of one (hi, lo) fragment unit: 2 x 64 lanes x 16 bytes; the bf16 packers fill the hi half


def rne_bf16(t):
    """fp32 tensor -> the same values rounded to bf16 (nearest even), as fp32."""
    return torch.as_tensor(t, dtype=torch.float32).bfloat16().float()


def trunc_bf16(t):
    """fp32 -> bf16 by dropping the low 16 bits (what a kernel without the rounding would feed the matrix pipe)."""
    t = torch.as_tensor(t, dtype=torch.float32).contiguous()
    return (t.view(torch.int32) & -65536).view(torch.float32)


def _lrelu32(t, slope):
    """The kernel's leaky-relu on an fp32 tensor: one fp32 multiply."""
    return t if slope == 1.0 else torch.where(t > 0, t, t * float(np.float32(slope)))


def _affine32(x, in_a, in_s):
    """fmaf(in_a, x, in_s) per (b, c): the fp64 result (exact product, one rounded add) cast to fp32."""
    return (f64(in_a)[:, :, None] * f64(x) + f64(in_s)[:, :, None]).float()


def operand(x, slope=1.0, in_a=None, in_s=None, rnd=rne_bf16):
    """The staged signal as the kernel rounds it: fp32 (B, C_in, L) holding bf16 numbers."""
    t = torch.as_tensor(x, dtype=torch.float32)
    if in_a is not None:
        t = _affine32(t, in_a, in_s)
    return rnd(_lrelu32(t, slope))


def ambiguous(x, slope, in_a, in_s):
    """True where the emulation of `operand` could differ from the kernel's fma: t or one of its fp32 neighbours rounds to another bf16."""
    t = _affine32(torch.as_tensor(x, dtype=torch.float32), in_a, in_s)
    inf = torch.full_like(t, float('inf'))
    r = [rne_bf16(_lrelu32(v, slope)) for v in (t, torch.nextafter(t, -inf), torch.nextafter(t, inf))]
    return (r[0] != r[1]) | (r[0] != r[2])


def redraw(x, slope, in_a, in_s, draw, rounds=64):
    """x with every ambiguous element redrawn (`draw(n)` -> n fresh fp32 values, already in the tensor's storage format); -> (x, rounds used).
    Asserts that none is left."""
    x = x.clone()
    for r in range(rounds + 1):
        bad = ambiguous(x, slope, in_a, in_s)
        if not bad.any():
            return x, r
        assert r < rounds, 'redraw did not terminate'
        x[bad] = draw(int(bad.sum()))
    raise AssertionError('unreachable')


def _left(k, dil, pad_left):
    return split_ref._left(k, dil, pad_left)


def conv1d(x, wf, n, *, dil=1, pad_left=-1, slope=1.0, in_a=None, in_s=None, rnd=rne_bf16, **epi):
    """v2w_conv1d_fwd with V2W_ALGO_BF16 on conv_bf16_kernel (one problem of _fwd_multi): x (B, C_in, L) fp32 values (bf16 numbers where the
    tensor is stored in bf16), wf [k][C_in][C_out] -> (value, bound) (B, C_out, L) in fp64; the bound is for the fp32 value in front of the
    store.  rnd: the operand rounding (the wrong-kernel statements of the CPU test pass another)."""
    a = f64(operand(x, slope, in_a, in_s, rnd))
    w = f64(rne_bf16(wf))
    z, S = R.taps_sum(a, w, dil, _left(wf.shape[0], dil, pad_left))
    value, S = R.epilogue(z, S, **epi)
    return value, n * U * S


def convt1d(x, wf, u, n, *, slope=1.0, bias=None):
    """v2w_convt1d_bf16_fwd: leaky_relu -> ConvTranspose1d(k, stride u, padding (k - u) / 2) -> + bias on bf16 operands: (value, bound)."""
    a = operand(x, slope)
    value, S = R.convt1d(a, rne_bf16(wf), u, slope=1.0, bias=bias)
    return value, n * U * S


# ---------------------------------------------------------------------------------------------------------------
# the bf16 store
def _f32_at_or_above(v):
    f = v.float()
    return torch.where(f.double() < v, torch.nextafter(f, torch.full_like(f, float('inf'))), f)


def _f32_at_or_below(v):
    f = v.float()
    return torch.where(f.double() > v, torch.nextafter(f, torch.full_like(f, -float('inf'))), f)


def store_interval(want, b):
    """(lo, hi) fp32 tensors holding bf16 numbers: what rne_bf16 can store of an fp32 value within b of want."""
    return rne_bf16(_f32_at_or_above(want - b)), rne_bf16(_f32_at_or_below(want + b))


def bf16_cell(g):
    """g: fp32 tensor of bf16 numbers -> (lo, hi) fp64: the closed interval of reals whose nearest bf16 is g (ties on both ends)."""
    bits = g.bfloat16().contiguous().view(torch.int16).to(torch.int32) & 0xffff
    mag, neg = bits & 0x7fff, (bits & 0x8000) != 0

    def val(m):
        return m.to(torch.int16).view(torch.bfloat16).double()
    me, up, dn = val(mag), val((mag + 1).clamp(max=0x7f80)), val((mag - 1).clamp(min=0))
    hi = (me + up) / 2
    lo = torch.where(mag > 0, (me + dn) / 2, -val(torch.ones_like(mag)) / 2)
    return torch.where(neg, -hi, lo), torch.where(neg, -lo, hi)


def _next_bf16(g):
    """The next bf16 number above g (fp32 tensors of bf16 numbers)."""
    bits = g.bfloat16().contiguous().view(torch.int16).to(torch.int32) & 0xffff
    mag, neg = bits & 0x7fff, (bits & 0x8000) != 0
    nb = torch.where(neg, torch.where(mag > 1, bits - 1, torch.zeros_like(bits)), bits + 1)      # (-min subnormal -> +0)
    nb = torch.where(nb >= 0x8000, nb - 0x10000, nb)
    return nb.to(torch.int16).view(torch.bfloat16).float()


def store_ratio(got, want, b):
    """Per entry: the distance from want to the nearest real that rounds to the stored bf16 `got`, over b (0 / 0 = 0; non-finite got: inf)."""
    got = torch.as_tensor(got).float()
    lo, hi = bf16_cell(got)
    d = torch.clamp(lo - want, min=0) + torch.clamp(want - hi, min=0)
    r = torch.where(d == 0, torch.zeros_like(d), d / b)
    return torch.where(torch.isfinite(got), r, torch.full_like(r, float('inf')))


def check_store(got, want, b):
    """The bf16-store check -> dict: `ratio` (worst store_ratio), `outside` (entries outside their interval: must be 0), and where the
    value landed: `single` (one-member intervals, with the worst |got - want| / b among them: `single_err`), `lower` / `upper` (two members),
    `wider` (more than two)."""
    got, want, b = torch.as_tensor(got).float(), f64(want), f64(b)
    lo, hi = store_interval(want, b)
    inside = (got >= lo) & (got <= hi) & torch.isfinite(got)
    one = lo == hi
    two = ~one & (_next_bf16(lo) == hi)
    err = torch.where(b > 0, (got.double() - want).abs() / b, torch.zeros_like(b))
    return dict(ratio=float(store_ratio(got, want, b).max()) if got.numel() else 0.0, outside=int((~inside).sum()),
                single=int(one.sum()), single_err=float(err[one & inside].max()) if bool((one & inside).any()) else 0.0,
                lower=int((two & (got == lo)).sum()), upper=int((two & (got == hi)).sum()), wider=int((~one & ~two).sum()))


# ---------------------------------------------------------------------------------------------------------------
# v2w_pack_bf16_convt
def convt_geom(k, u):
    """(UP, hl, hr, KV) of the virtual conv: UP = u rounded up to a power of two; output phase r of position q reads the inputs
    q - hl .. q + hr (KV = hl + hr + 1 virtual taps)."""
    UP = 1
    while UP < u:
        UP *= 2
    pad, hl, hr = (k - u) // 2, 0, 0
    for r in range(u):
        t0, c = (r + pad) % u, (r + pad) // u
        nt = (k - t0 + u - 1) // u
        hr, hl = max(hr, c), max(hl, nt - 1 - c)
    return UP, hl, hr, hl + hr + 1


def virtual_weights(wf, u, rows_per):
    """Wv[tv][ci][co * rows_per + r] = wf[t0_r + m * u][ci][co], m = c_r - (tv - hl), t0_r = (r + pad) % u, c_r = (r + pad) / u; zero where
    the phase has no such tap and for the padding phases r >= u."""
    wf = np.asarray(wf, dtype=np.float32)
    k, ci, co = wf.shape
    _, hl, _, KV = convt_geom(k, u)
    pad = (k - u) // 2
    wv = np.zeros((KV, ci, co * rows_per), dtype=np.float32)
    for r in range(min(u, rows_per)):
        t0, cr = (r + pad) % u, (r + pad) // u
        for tv in range(KV):
            m = cr - (tv - hl)
            t = t0 + m * u
            if m >= 0 and t < k:
                wv[tv, :, r::rows_per] = wf[t]
    return wv


def exact_region(co, u):
    UP = convt_geom(u, u)[0]
    return UP != u and (co * u) % 32 == 0


def pack_bf16_convt_bytes(k, ci, co, u):
    UP, _, _, KV = convt_geom(k, u)
    return (co * UP // 32 + (co * u // 32 if exact_region(co, u) else 0)) * (ci // 16) * KV * FRAG_UNIT


def pack_bf16_convt(wf, u):
    """-> list of int16 arrays [mb][ch][KV][64][8], one per region (the padded rows co * UP + r; then, for a stride that is no power of
    two with C_out * u % 32 == 0, the exact rows co * u + r): the hi halves of the buffer's fragment units, in order.  The lo halves are
    not written."""
    co = np.asarray(wf).shape[2]
    UP = convt_geom(np.asarray(wf).shape[0], u)[0]
    return [split_ref.pack_bf16(virtual_weights(wf, u, rp)) for rp in ((UP, u) if exact_region(co, u) else (UP,))]
