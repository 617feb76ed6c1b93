"""fp64 CPU statement of what the two resident-tile kernels of the bf16-storage pipeline compute - conv_bf16_res_kernel
(csrc/v2w_conv_bf16_res.hip behind v2w_branch_convs_bf16_fwd, modes 0 and 1) and convt_bf16_res_kernel (csrc/v2w_convt_bf16_res.hip behind
v2w_convt1d_bf16_fwd with io_bf16 == 3) - and what each entry may differ by.  Operand rounding, redraw, the bf16 store criterion and the
transposed conv's value are tests/convbf16_ref.py's; this file adds the residual the kernel rebuilds, the two branch-conv forms and the
statistics rows of a kernel that sums BEFORE it rounds.

Operands (eps = 2^-24): weights rne_bf16(wf); signal xs = rne_bf16(lrelu32(fma32(in_a, x, in_s))) with x a bf16 number (the affine in mode 0
only; ambiguous elements redrawn, convbf16_ref.redraw); the padding of the activated signal is exactly 0.  Products of two bf16 numbers are
exact in fp32, so the statement is on the rounded operands.

Residual: the kernel's, not the tensor's - r = xs where xs > 0, else xs * fl32(1 / slope), the product formed here in fp64 from the fp32
reciprocal (its one fp32 rounding is counted in n); +-0 stays +-0.

mode 0, branch j:  want = bias_j + r + conv_{k_j, dil_j}(xs),  b = n eps S,  n = k_j C + 3 (the accumulator's k_j C additions behind the
bias, the residual's multiply and its addition, the store's input),  S = |bias_j| + |r| + sum |w| |xs|.
mode 1:  want = (sum_j bias_j + sum_j r_j + sum_j conv_j(xs_j)) / out_div (no division when out_div == 0),
n = sum_j k_j C + 3 nbr + (out_div != 0), S over every term, scaled by 1 / |out_div|.
A short-chain record has one live input channel per batch item: k_j in place of k_j C.

The outputs are bf16: the criterion is convbf16_ref.check_store - the stored number must be one rne_bf16 can make of an fp32 value within b
of want.

Transposed conv: value and bound are convbf16_ref.convt1d (n = ceil(k / u) C_in + 2).  Its statistics rows hold the sums of the fp32 values
BEFORE the store rounds them, so they are held to the sums of `want`, not of what was stored: row (tile, channel), N live output entries,
  |sum - sum want|  <= sum b_e + N eps sum |want_e|,      |squares - sum want^2|  <= sum (2 |want_e| b_e + b_e^2) + N eps sum want_e^2
(every value is within b_e of want_e; N additions - fmas for the squares - of N values, each rounding at most eps of the running sum, which
the sums of magnitudes bound to first order; the kernel's trees are far shallower than N).  Entries past L contribute nothing."""
import numpy as np
import torch

from tests import convbf16_ref as R
from tests import tile_ref as T
from tests.disc_ref import U, ceil_div, f64


def inv_slope(slope):
    """fl32(1 / slope) as the launcher forms it."""
    return float(np.float32(1.0) / np.float32(slope))


def residual(xs, slope):
    """The residual the kernel rebuilds from the staged operand xs (fp32 tensor of bf16 numbers), in fp64."""
    v = f64(xs)
    return torch.where(v > 0, v, v * inv_slope(slope))


def _branch(xs, wf, dil, bias, slope):
    """(bias + r + conv(xs), the same sum of magnitudes) of one branch on the staged operand."""
    k = wf.shape[0]
    z, S = T.taps_sum(f64(xs), f64(R.rne_bf16(wf)), dil, dil * (k - 1) // 2)
    r = residual(xs, slope)
    z, S = z + r, S + r.abs()
    if bias is not None:
        z, S = z + f64(bias)[None, :, None], S + f64(bias).abs()[None, :, None]
    return z, S


def first_convs(x, wfs, dils, ns, *, slope, in_a=None, in_s=None, biases=None):
    """mode 0: x (B, C, L) bf16 numbers, wfs[j] [k_j][C][C] -> [(want_j, b_j)] in fp64, one per branch."""
    xs = R.operand(x, slope, in_a, in_s)
    out = []
    for j, wf in enumerate(wfs):
        z, S = _branch(xs, wf, dils[j], None if biases is None else biases[j], slope)
        out.append((z, ns[j] * U * S))
    return out


def second_convs(xs, wfs, dils, n, *, slope, biases=None, out_div=0.0):
    """mode 1: xs[j] (B, C, L) bf16 numbers -> (want, b) in fp64."""
    tot = mag = 0.0
    for j, wf in enumerate(wfs):
        z, S = _branch(R.operand(xs[j], slope), wf, dils[j], None if biases is None else biases[j], slope)
        tot, mag = tot + z, mag + S
    if out_div:
        d = float(np.float32(out_div))
        tot, mag = tot / d, mag / abs(d)
    return tot, n * U * mag


def convt_rows(want, b, NT, u):
    """The statistics rows of the transposed conv from (want, b) (B, C_out, L u): -> (sums, their bound, squares, their bound), each
    (B * ceil(L / NT), C_out): row = item * tiles + tile, as the launch numbers its tiles."""
    B, co, Lo = want.shape
    ntl = ceil_div(Lo, NT * u)

    def rows(t):
        p = torch.zeros(B, co, ntl * NT * u, dtype=torch.float64, device=t.device)
        p[:, :, :Lo] = t
        return p.view(B, co, ntl, NT * u).sum(3).permute(0, 2, 1).reshape(B * ntl, co)
    N = torch.tensor([min(NT * u, Lo - t * NT * u) for t in range(ntl)], dtype=torch.float64, device=want.device).repeat(B)[:, None]
    w = want.abs()
    return (rows(want), rows(b) + N * U * rows(w), rows(want * want), rows(2 * w * b + b * b) + N * U * rows(want * want))
