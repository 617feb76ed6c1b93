// Launchers that one source file defines and another calls: each declared once, default arguments included.  Definers and callers
// both include this header, so a changed signature is a compile error and not a link-time surprise.
#pragma once
#include "v2w_common.h"

// ---- Conv1d / ConvTranspose1d (called by v2w_api.hip unless noted).  V2W_E_SHAPE: the kernel does not take the shape.
// v2w_conv_mfma.hip: cfg_out / ws_query turn the call into the host-only tile-configuration / split-workspace query; len: per-item lengths
int v2w_conv1d_mfma(const v2w_conv1d_args* a, int n, hipStream_t stream, int* cfg_out, long long* ws_query = nullptr,
                    const int32_t* len = nullptr, int len_mul = 1);
int v2w_convt1d_mfma(const v2w_convt1d_args* a, hipStream_t stream, int* cfg_out, long long* ws_query = nullptr,
                     const int32_t* len = nullptr, int len_mul = 1);
int v2w_conv1d_wino(const v2w_conv1d_args* a, int n, hipStream_t stream, const int32_t* len = nullptr, int len_mul = 1);   // v2w_conv_wino.hip
int v2w_conv1d_split(const v2w_conv1d_args* a, int n, hipStream_t stream, bool bf16);                                      // v2w_conv_split.hip
int v2w_conv1d_bf16(const v2w_conv1d_args* a, int n, hipStream_t stream, int32_t* cfg);             // v2w_conv_bf16.hip, for v2w_conv1d_split
int v2w_conv1d_direct(const v2w_conv1d_args* a, hipStream_t stream);                                // v2w_direct.hip
int v2w_convt1d_direct(const v2w_convt1d_args* a, hipStream_t stream);                              // v2w_direct.hip
// v2w_convt_bf16_res.hip, for v2w_conv_bf16.hip's transposed-conv dispatch
int v2w_convt1d_bf16_res(const v2w_convt1d_args* a, int UP, int hl, int KV, hipStream_t stream, int* ntiles_out, int32_t* cfg);
// v2w_conv_post_bf16.hip, for v2w_direct.hip's conv_post + tanh on a bf16 input
int v2w_conv_post_tanh_bf16_mfma(const unsigned short* in, const float* wf, const float* bias, float* out,
                                 int B, int C_in, int L, int k, float slope, hipStream_t stream);

// ---- residual stages in the bf16 arithmetic: v2w_stage_split.hip -> v2w_stage_bf16.hip -> the kernels by channel count
int v2w_resblock2_stage_bf16(const v2w_stage_split_args* a, hipStream_t stream, int* up_tiles_out = nullptr);        // v2w_stage_bf16.hip
int v2w_resblock2_stage_bf16_wide(const v2w_stage_split_args* a, hipStream_t stream, int* up_tiles_out = nullptr);   // v2w_stage_bf16_wide.hip
int v2w_resblock2_stage_bf16_n32s(const v2w_stage_split_args* a, hipStream_t stream, int* up_tiles_out);             // v2w_stage_bf16_n32s.hip
int v2w_resblock2_stage_bf16_n16(const v2w_stage_split_args* a, hipStream_t stream);                                 // v2w_stage_bf16_n16.hip
int v2w_resblock1_pairs_bf16_n16(const v2w_stage_split_args* a, hipStream_t stream);                                 // v2w_stage_bf16_n16.hip
int v2w_resblock2_stage_bf16_n16s(const v2w_stage_split_args* a, hipStream_t stream);        // v2w_stage_bf16_n16s.hip: the streaming form, stage + tail

// The branches of a stage as those launchers read them from v2w_stage_split_args: packed bf16 fragments and biases of both convs, taps and
// dilations, and the halos of the widest branch (h = dilation * (k - 1) / 2).  The kernels' argument structs keep their own field order (it
// is their argument segment); v2w_put_branch_ptrs copies the first N branches into one.
#define V2W_BF_MAXB 4
struct StageBfBranches {
    const unsigned char* w1[V2W_BF_MAXB]; const float* bias1[V2W_BF_MAXB];
    const unsigned char* w2[V2W_BF_MAXB]; const float* bias2[V2W_BF_MAXB];
    int K[V2W_BF_MAXB], d1[V2W_BF_MAXB], d2[V2W_BF_MAXB];
    int nk, h1max, h2max;
};
static inline StageBfBranches v2w_stage_bf_branches(const v2w_stage_split_args* q) {
    StageBfBranches r{};
    r.nk = q->nk;
    for (int j = 0; j < q->nk && j < V2W_BF_MAXB; ++j) {
        r.w1[j] = static_cast<const unsigned char*>(q->wps1[j]); r.bias1[j] = q->bias1[j];
        r.w2[j] = static_cast<const unsigned char*>(q->wps2[j]); r.bias2[j] = q->bias2[j];
        r.K[j] = q->k[j]; r.d1[j] = q->dil1[j]; r.d2[j] = q->dil2[j];
        const int h1 = r.d1[j] * (r.K[j] - 1) / 2, h2 = r.d2[j] * (r.K[j] - 1) / 2;
        if (h1 > r.h1max) r.h1max = h1;
        if (h2 > r.h2max) r.h2max = h2;
    }
    return r;
}
template <int N, typename P> static inline void v2w_put_branch_ptrs(P& p, const StageBfBranches& r) {
    static_assert(N <= V2W_BF_MAXB && sizeof(p.w1) == N * sizeof(p.w1[0]), "branches of the record / of the argument struct");
    for (int j = 0; j < N; ++j) { p.w1[j] = r.w1[j]; p.bias1[j] = r.bias1[j]; p.w2[j] = r.w2[j]; p.bias2[j] = r.bias2[j]; }
}
// ... and their taps, dilations and halos (the kernels that take the block set at run time)
template <typename P> static inline void v2w_put_branch_geom(P& p, const StageBfBranches& r) {
    static_assert(sizeof(p.K) == sizeof(r.K) && sizeof(p.d1) == sizeof(r.d1) && sizeof(p.d2) == sizeof(r.d2), "V2W_BF_MAXB branches");
    for (int j = 0; j < V2W_BF_MAXB; ++j) { p.K[j] = r.K[j]; p.d1[j] = r.d1[j]; p.d2[j] = r.d2[j]; }
    p.nk = r.nk; p.h1max = r.h1max; p.h2max = r.h2max;
}
// The reference's block set (hparams: resblock_kernel_sizes (3, 7, 11), dilations (1, 3), ResBlock2) with both packed weights of every
// branch present: what the kernels with compile-time taps are built for
static inline bool v2w_is_reference_block_set(const v2w_stage_split_args* q) {
    if (q->nk != 3) return false;
    for (int j = 0; j < 3; ++j)
        if (q->k[j] != 3 + 4 * j || q->dil1[j] != 1 || q->dil2[j] != 3 || !q->wps1[j] || !q->wps2[j]) return false;
    return true;
}
