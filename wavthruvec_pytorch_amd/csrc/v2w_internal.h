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
