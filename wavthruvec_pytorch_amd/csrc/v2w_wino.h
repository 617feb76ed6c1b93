// Winograd F(2,3) form of an odd-k dilated Conv1d (v2w_conv_wino.hip): the taps split into segments of at most 3 consecutive taps
// (k = 3 -> 3, 7 -> 3+3+1, 11 -> 3+3+3+2); every segment adds into the same four accumulator classes M0..M3 of an output PAIR
// (t, t + dil), and y(t) = M0 + M1 + M2, y(t + dil) = M1 - M2 - M3.  With x_j = act(x)[t + o + j*dil] (o: the segment's first tap):
//   3 taps: M0 += g0 (x0 - x2)   M1 += (g0+g1+g2)/2 (x1 + x2)   M2 += (g0-g1+g2)/2 (x2 - x1)   M3 += g2 (x1 - x3)
//   2 taps: M0 += g0 (x0 - x1)   M1 += (g0+g1) x1               M3 += g1 (x1 - x2)
//   1 tap : M0 += g0 x0          M3 += -g0 x1
// Shared by the kernel and by the two packers of its weight stream (v2w_pack_wino, the batched fold).
#pragma once

namespace {

__host__ __device__ constexpr int wino_seg_terms(int ntap) { return ntap == 3 ? 4 : (ntap == 2 ? 3 : 2); }
// terms (weight matrices) of a k-tap conv; 0 when k is not served (even, or < 3)
__host__ __device__ constexpr int wino_terms(int k) {
    return (k < 3 || (k & 1) == 0) ? 0 : 4 * (k / 3) + (k % 3 == 2 ? 3 : (k % 3 == 1 ? 2 : 0));
}

// Fragment fi (< wino_terms(k) * gpc) of one (row block, channel chunk) in consumption order [segment][unit gg][term]:
// the segment's first tap, its tap count, the unit and the term.
__host__ __device__ inline void wino_frag(int k, int gpc, int fi, int& s0, int& ntap, int& gg, int& term) {
    s0 = 0;
    for (;;) {
        ntap = k - s0 >= 3 ? 3 : k - s0;
        const int nt = wino_seg_terms(ntap);
        if (fi < nt * gpc) { gg = fi / nt; term = fi - gg * nt; return; }
        fi -= nt * gpc;
        s0 += ntap;
    }
}

// Transformed weight of `term` of a segment from its taps g0, g1, g2 (unused ones ignored).
__host__ __device__ inline float wino_weight(int ntap, int term, float g0, float g1, float g2) {
    if (ntap == 3) {
        switch (term) {
            case 0: return g0;
            case 1: return ((g0 + g2) + g1) * 0.5f;
            case 2: return ((g0 + g2) - g1) * 0.5f;
            default: return g2;
        }
    }
    if (ntap == 2) return term == 0 ? g0 : (term == 1 ? g0 + g1 : g1);
    return term == 0 ? g0 : -g0;
}

}  // namespace
