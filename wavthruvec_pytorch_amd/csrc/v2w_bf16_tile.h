// Device steps the bf16 kernels (v2w_stage_bf16*.hip, v2w_conv_bf16_res.hip, v2w_convt_bf16_res.hip, v2w_conv_bf16.hip) share: pieces of
// the staging ITEM, and the bf16 MFMA.  An item = 4 consecutive channels x 4 consecutive positions of a (B, C, L) tensor on its way into
// an LDS tile of position-major rows: four loads of 4 positions of one channel each, at the offset of v2w_item_off, then per position
// the 8 bytes of its 4 channels: unpack, optional per-(b, c) affine y = a x + s, lrelu, repack to bf16, exact 0 outside the sequence.
// L % 4 == 0 and an item's first position is a multiple of 4, so a position quad lies inside or outside the sequence as a whole (`ok`).
// Where the rows go (tile, row stride, swizzle, raw and mirror copies) is the kernel's own.
#pragma once
#include "v2w_tile.h"

// Byte offset of an item inside its batch item's block of channel rows: `first` = the element index of (first channel, position 0),
// ESIZE bytes per element.  The loads are UNCONDITIONAL: outside the sequence the offset is clamped to position 0 (always a legal address)
// and v2w_item_row returns zeros instead of what came back.  The empty asm makes the result opaque: the address of every load stays
// (uniform 64-bit base) + (this 32-bit per-lane offset), one register for the whole kernel - left transparent, hipcc folds the offset
// into 64-bit per-lane pointers (two registers and a 64-bit add per load) and re-derives the clamp at each use.
template <int ESIZE = 2>
__device__ __forceinline__ unsigned v2w_item_off(int first, bool ok, int pos) {
    unsigned vo = (unsigned)(first + (ok ? pos : 0)) * ESIZE;
    asm volatile("" : "+v"(vo));
    return vo;
}
// The four loads of an item of a bf16 tensor: pf[i] = the 4 positions of channel i.  base = the (uniform) byte address of the first
// channel, L = elements between channels, vo = v2w_item_off().
__device__ __forceinline__ void v2w_item_load(u32x2 (&pf)[4], const unsigned char* base, int L, unsigned vo) {
#pragma unroll
    for (int i = 0; i < 4; ++i) pf[i] = *gptr<const u32x2>(base + (size_t)i * L * 2 + vo);
}

// Position row e (0 .. 3) of an item: the activated operand of its 4 channels as 8 bytes of bf16, exactly 0 outside the sequence (the
// convs zero-pad the ACTIVATED signal).  AFFINE: y = av[i] * x + sv[i] first (else av / sv are not read).  The activation is the
// select form v2w_lrelu; the kernels tuned with max(y, slope y) spell their rows out themselves.
template <bool AFFINE, typename AV>
__device__ __forceinline__ u32x2 v2w_item_row(int e, const u32x2 (&pf)[4], const AV& av, const AV& sv, float slope, bool ok) {
    float v[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float xv = (e & 1) ? v2w_bf16_hi(pf[i][e >> 1]) : v2w_bf16_lo(pf[i][e >> 1]);
        v[i] = v2w_lrelu(AFFINE ? fmaf(av[i], xv, sv[i]) : xv, slope);
    }
    u32x2 w = {v2w_bf16x2(v[0], v[1]), v2w_bf16x2(v[2], v[3])};
    if (!ok) w = u32x2{0u, 0u};
    return w;
}

// ---- acc += A x B on the bf16 matrix pipe, operands as the 16 bytes a lane holds (8 bf16 k-values)
__device__ __forceinline__ f32x16 v2w_mfma_bf16_32(f32x16 c, u32x4 av, u32x4 bv) {     // v_mfma_f32_32x32x16_bf16
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(b8, av), __builtin_bit_cast(b8, bv), c, 0, 0, 0);
}
__device__ __forceinline__ f32x4 v2w_mfma_bf16_16(f32x4 c, u32x4 av, u32x4 bv) {       // v_mfma_f32_16x16x32_bf16
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(b8, av), __builtin_bit_cast(b8, bv), c, 0, 0, 0);
}
