"""float64 statement of the summed Winograd launch (hipops.conv1d_wino_sum, v2w_conv1d_wino_sum_fwd): the second convs of a ResBlock2 stage's
branches on one accumulator.  Stated from the UNPACKED weights wf_j [k_j][C][C] through tests/tile_ref.py, no Winograd transform."""
import torch

from tests import tile_ref


def wino_sum(xs, wfs, biases, *, dil, slope, out_div=0.0, lengths=None):
    """out = (sum_j x_j + sum_j conv_j(lrelu(x_j)) + sum_j b_j) [/ out_div]; x_j (B, C, L), wf_j [k_j][C][C], symmetric padding.  With `lengths`
    (B end positions) every x_j counts as zero at and past its item's end; the outputs there are unspecified (not masked here)."""
    total = None
    for x, wf, b in zip(xs, wfs, biases):
        k = wf.shape[0]
        act = tile_ref.activate(x, slope, lengths=lengths)
        r = tile_ref.f64(x) + tile_ref.taps_sum(act, wf, dil, dil * (k - 1) // 2)[0] + tile_ref.f64(b)[None, :, None]
        total = r if total is None else total + r
    return total / out_div if out_div else total
