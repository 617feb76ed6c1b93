// Spectral norm of the discriminators' conv weights (legacy torch.nn.utils.spectral_norm on the first DiscriminatorS, reference
// models.py:219-258): one power iteration, sigma, the division and the relayout into the conv kernels' [k][C_in][C_out] form for up to
// V2W_SN_MAX_LAYERS weight matrices in four launches (two without the iteration), and the backward through W / sigma in two.  The
// arithmetic, its order and its fp32 roundings are stated in include/vec2wav_hip.h.
//
// W is R = C_out rows of N = C_in * k floats.  The phases a grid-wide sum separates are the launches:
//   sn_wtu_kernel    W^T u: a workgroup owns kBand rows x kCols columns, its four waves take every fourth row, a lane four columns (one
//                    16-byte load per row when rows are 16-byte aligned, else four coalesced 4-byte loads); the waves' sums meet in LDS
//                    and one partial row per band goes to the workspace
//   sn_v_kernel      one workgroup per layer adds the bands in index order, takes the norm and writes v (and its kept copy)
//   sn_wv_kernel     W v: one wave per row, lanes stride along the row, a butterfly sum; t[o] goes to the workspace
//   sn_scale_kernel  every workgroup forms ||t||, u = t / max(||t||, eps) and sigma = u . t from the same R floats in the same order (so all
//                    agree bit for bit), the layer's first one stores u, sigma and the kept copies; then its kTile x kTile tile of W
//                    goes through LDS - read along rows, written along C_out - divided by sigma
//   sn_bwd_dot_kernel / sn_bwd_apply_kernel   the same tiles: sum dwf . w per tile to the workspace; every workgroup adds the layer's tile sums
//                    in index order, then writes its tile of dw
// Workgroups are dealt to the layers by the host plan (v2w_sn_plan: blk_t / blk_r / blk_s = a layer's first workgroup in the three grid
// shapes); a workgroup finds its layer by a search over the device descriptors that every lane makes alike, and everything it computes is
// indexed from its layer's first workgroup: a layer's bits do not depend on its neighbours in the launch.  No atomics.
#include "v2w_common.h"

namespace {

constexpr int kBand = 64;      // rows per W^T u partial
constexpr int kCols = 256;     // columns per sn_wtu_kernel workgroup: 64 lanes x 4
constexpr int kTile = 64;      // the relayout tile
constexpr float kEps = 1e-12f;

struct BwdPtrs {
    const float* dwf[V2W_SN_MAX_LAYERS];
    float* dw[V2W_SN_MAX_LAYERS];
};
static_assert(sizeof(v2w_sn_desc) == 72 && sizeof(v2w_sn_grids) == 32, "include/vec2wav_hip.h states these sizes");
static_assert(sizeof(BwdPtrs) <= 3072, "kernel arguments travel by value");

__host__ __device__ inline int cdiv(int a, int b) { return (a + b - 1) / b; }
__device__ inline bool al16(const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; }

// which: 0 blk_t, 1 blk_r, 2 blk_s.  The layer whose workgroups include wg.
__device__ inline int find_layer(const v2w_sn_desc* __restrict__ D, int n, int wg, int which) {
    int lo = 0, hi = n;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        const int s = which == 0 ? D[mid].blk_t : which == 1 ? D[mid].blk_r : D[mid].blk_s;
        if (s <= wg) lo = mid; else hi = mid;
    }
    return lo;
}

__device__ inline float* keep_sigma(float* keep, const v2w_sn_desc& d) { return keep + d.keep_off; }
__device__ inline float* keep_u(float* keep, const v2w_sn_desc& d) { return keep + d.keep_off + 4; }
__device__ inline float* keep_v(float* keep, const v2w_sn_desc& d) { return keep + d.keep_off + 4 + ((d.c_out + 3) & ~3); }

__global__ void __launch_bounds__(256)
sn_wtu_kernel(const v2w_sn_desc* __restrict__ D, int n, float* __restrict__ ws) {
    __shared__ float red[3][kCols];
    const v2w_sn_desc d = D[find_layer(D, n, blockIdx.x, 0)];
    const int R = d.c_out, N = d.c_in * d.k;
    const int nct = cdiv(N, kCols);
    const int b = blockIdx.x - d.blk_t;
    const int band = b / nct, c0 = (b % nct) * kCols;
    const int lane = threadIdx.x & 63, wave = v2w_uni(threadIdx.x >> 6);
    const bool vec = (N & 3) == 0 && al16(d.w) && al16(ws);
    const float* __restrict__ w = d.w;
    const float* __restrict__ u = d.u;
    const int o0 = band * kBand + wave;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    if (vec) {
        const int c = c0 + 4 * lane;
        if (c < N) {
#pragma unroll 8
            for (int i = 0; i < kBand / 4; ++i) {
                const int o = o0 + 4 * i;
                if (o < R) {
                    const f32x4 x = *reinterpret_cast<const f32x4*>(w + (size_t)o * N + c);
                    const float uo = u[o];
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc[j] = __fmaf_rn(x[j], uo, acc[j]);
                }
            }
        }
    } else {
#pragma unroll 4
        for (int i = 0; i < kBand / 4; ++i) {
            const int o = o0 + 4 * i;
            if (o < R) {
                const float uo = u[o];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int c = c0 + lane + 64 * j;
                    if (c < N) acc[j] = __fmaf_rn(w[(size_t)o * N + c], uo, acc[j]);
                }
            }
        }
    }
    if (wave > 0) {
#pragma unroll
        for (int j = 0; j < 4; ++j) red[wave - 1][j * 64 + lane] = acc[j];
    }
    __syncthreads();
    if (wave == 0) {
        float* part = ws + d.ws_off + (size_t)band * N;
        f32x4 r;
#pragma unroll
        for (int j = 0; j < 4; ++j)
            r[j] = __fadd_rn(__fadd_rn(__fadd_rn(acc[j], red[0][j * 64 + lane]), red[1][j * 64 + lane]), red[2][j * 64 + lane]);
        if (vec) {
            const int c = c0 + 4 * lane;
            if (c < N) *reinterpret_cast<f32x4*>(part + c) = r;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int c = c0 + lane + 64 * j;
                if (c < N) part[c] = r[j];
            }
        }
    }
}

__global__ void __launch_bounds__(1024)
sn_v_kernel(const v2w_sn_desc* __restrict__ D, float* ws, float* keep) {
    __shared__ float red[16];
    const v2w_sn_desc d = D[blockIdx.x];
    const int R = d.c_out, N = d.c_in * d.k;
    const int nb = cdiv(R, kBand);
    float* part = ws + d.ws_off;
    float q = 0.f;
    for (int j = threadIdx.x; j < N; j += 1024) {
        float a = part[j];
        for (int b = 1; b < nb; ++b) a = __fadd_rn(a, part[(size_t)b * N + j]);
        part[j] = a;                                   // read back below by this same thread
        q = __fmaf_rn(a, a, q);
    }
    q = v2w_block_sum(q, red);
    const float dn = fmaxf(__fsqrt_rn(q), kEps);
    float* vk = keep_v(keep, d);
    for (int j = threadIdx.x; j < N; j += 1024) {
        const float x = __fdiv_rn(part[j], dn);
        d.v[j] = x;
        vk[j] = x;
    }
}

__global__ void __launch_bounds__(256)
sn_wv_kernel(const v2w_sn_desc* __restrict__ D, int n, float* __restrict__ ws) {
    const v2w_sn_desc d = D[find_layer(D, n, blockIdx.x, 1)];
    const int R = d.c_out, N = d.c_in * d.k;
    const int lane = threadIdx.x & 63, wave = v2w_uni(threadIdx.x >> 6);
    const int o = (blockIdx.x - d.blk_r) * 4 + wave;
    if (o >= R) return;
    const float* __restrict__ row = d.w + (size_t)o * N;
    const float* __restrict__ v = d.v;
    float s;
    if ((N & 3) == 0 && al16(d.w) && al16(v)) {
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
        for (int j = 4 * lane; j < N; j += 256) {
            const f32x4 x = *reinterpret_cast<const f32x4*>(row + j);
            const f32x4 y = *reinterpret_cast<const f32x4*>(v + j);
#pragma unroll
            for (int i = 0; i < 4; ++i) acc[i] = __fmaf_rn(x[i], y[i], acc[i]);
        }
        s = __fadd_rn(__fadd_rn(acc[0], acc[1]), __fadd_rn(acc[2], acc[3]));
    } else {
        s = 0.f;
#pragma unroll 4
        for (int j = lane; j < N; j += 64) s = __fmaf_rn(row[j], v[j], s);
    }
    s = v2w_wave_sum(s);
    if (lane == 0) ws[d.ws_off + (size_t)cdiv(R, kBand) * N + o] = s;
}

// rows [o0, o0 + kTile) x columns [c0, c0 + kTile) of the R x N matrix `src` into tile[row][column], 0 outside; 16-byte loads when vec
__device__ __forceinline__ void load_rows_tile(float (*tile)[kTile + 1], const float* __restrict__ src, int R, int N, int o0, int c0, bool vec) {
    const int cl = (threadIdx.x & 15) * 4, ol = threadIdx.x >> 4;
#pragma unroll
    for (int p = 0; p < kTile / 16; ++p) {
        const int r = ol + 16 * p, o = o0 + r, c = c0 + cl;
        f32x4 x = {0.f, 0.f, 0.f, 0.f};
        if (o < R) {
            if (vec) {
                if (c < N) x = *reinterpret_cast<const f32x4*>(src + (size_t)o * N + c);
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (c + i < N) x[i] = src[(size_t)o * N + c + i];
            }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) tile[r][cl + i] = x[i];
    }
}

// column c = ci * K + t of W is row t * Cin + ci of the [k][C_in][C_out] layout
__device__ __forceinline__ size_t fold_index(int c, int K, int Cin, int R, int o) {
    const int ci = c / K, t = c - ci * K;
    return ((size_t)t * Cin + ci) * R + o;
}

__global__ void __launch_bounds__(256)
sn_scale_kernel(const v2w_sn_desc* __restrict__ D, int n, int training, const float* __restrict__ ws, float* keep) {
    __shared__ float tile[kTile][kTile + 1];
    __shared__ float red[16];
    const v2w_sn_desc d = D[find_layer(D, n, blockIdx.x, 2)];
    const int R = d.c_out, N = d.c_in * d.k, K = d.k;
    const float* __restrict__ t = ws + d.ws_off + (size_t)cdiv(R, kBand) * N;
    const int b = blockIdx.x - d.blk_s;
    const int nct = cdiv(N, kTile);
    const int o0 = (b / nct) * kTile, c0 = (b % nct) * kTile;
    const int tid = threadIdx.x;

    float du = 1.f;
    if (training) {
        float p = 0.f;
        for (int o = tid; o < R; o += 256) p = __fmaf_rn(t[o], t[o], p);
        p = v2w_block_sum(p, red);
        du = fmaxf(__fsqrt_rn(p), kEps);
    }
    float s = 0.f;
    for (int o = tid; o < R; o += 256) {
        const float uo = training ? __fdiv_rn(t[o], du) : d.u[o];
        s = __fmaf_rn(uo, t[o], s);
    }
    const float sigma = v2w_block_sum(s, red);
    if (b == 0) {                                         // the layer's first workgroup stores what all of them computed
        float* uk = keep_u(keep, d);
        for (int o = tid; o < R; o += 256) {
            const float uo = training ? __fdiv_rn(t[o], du) : d.u[o];
            if (training) d.u[o] = uo;
            uk[o] = uo;
        }
        if (!training) {
            float* vk = keep_v(keep, d);
            for (int j = tid; j < N; j += 256) vk[j] = d.v[j];
        }
        if (tid == 0) *keep_sigma(keep, d) = sigma;
    }

    load_rows_tile(tile, d.w, R, N, o0, c0, (N & 3) == 0 && al16(d.w));
    __syncthreads();
    const int ol = tid & 63, o = o0 + ol;
    if (o < R) {
#pragma unroll 4
        for (int cc = tid >> 6; cc < kTile; cc += 4) {
            const int c = c0 + cc;
            if (c < N) d.wf[fold_index(c, K, d.c_in, R, o)] = __fdiv_rn(tile[ol][cc], sigma);
        }
    }
}

__global__ void __launch_bounds__(256)
sn_bwd_dot_kernel(const v2w_sn_desc* __restrict__ D, int n, const BwdPtrs P, float* __restrict__ ws) {
    __shared__ float tile[kTile][kTile + 1];
    __shared__ float red[16];
    const int li = find_layer(D, n, blockIdx.x, 2);
    const float* __restrict__ dwf = P.dwf[li];
    if (!dwf || !P.dw[li]) return;
    const v2w_sn_desc d = D[li];
    const int R = d.c_out, N = d.c_in * d.k, K = d.k;
    const int b = blockIdx.x - d.blk_s;
    const int nct = cdiv(N, kTile);
    const int o0 = (b / nct) * kTile, c0 = (b % nct) * kTile;
    load_rows_tile(tile, d.w, R, N, o0, c0, (N & 3) == 0 && al16(d.w));
    __syncthreads();
    const int ol = threadIdx.x & 63, o = o0 + ol;
    float acc = 0.f;
    if (o < R) {
#pragma unroll 4
        for (int cc = threadIdx.x >> 6; cc < kTile; cc += 4) {
            const int c = c0 + cc;
            if (c < N) acc = __fmaf_rn(dwf[fold_index(c, K, d.c_in, R, o)], tile[ol][cc], acc);
        }
    }
    acc = v2w_block_sum(acc, red);
    if (threadIdx.x == 0) ws[d.ws_off + b] = acc;
}

__global__ void __launch_bounds__(256)
sn_bwd_apply_kernel(const v2w_sn_desc* __restrict__ D, int n, const BwdPtrs P, const float* __restrict__ ws, const float* __restrict__ keep) {
    __shared__ float tile[kTile][kTile + 1];
    __shared__ float red[16];
    const int li = find_layer(D, n, blockIdx.x, 2);
    const float* __restrict__ dwf = P.dwf[li];
    float* __restrict__ dw = P.dw[li];
    if (!dwf || !dw) return;
    const v2w_sn_desc d = D[li];
    const int R = d.c_out, N = d.c_in * d.k, K = d.k;
    const int b = blockIdx.x - d.blk_s;
    const int nct = cdiv(N, kTile), ntile = nct * cdiv(R, kTile);
    const int o0 = (b / nct) * kTile, c0 = (b % nct) * kTile;
    const float* part = ws + d.ws_off;
    float p = 0.f;
    for (int i = threadIdx.x; i < ntile; i += 256) p = __fadd_rn(p, part[i]);
    const float dot = v2w_block_sum(p, red);
    const float* kp = keep + d.keep_off;
    const float sigma = kp[0];
    const float* __restrict__ u = kp + 4;
    const float* __restrict__ v = kp + 4 + ((R + 3) & ~3);
    const float coef = __fdiv_rn(dot, __fmul_rn(sigma, sigma));

    {   // dwf tile, read along C_out: tile[row][column] = dwf[column's fold row][row]
        const int ol = threadIdx.x & 63, o = o0 + ol;
#pragma unroll 4
        for (int cc = threadIdx.x >> 6; cc < kTile; cc += 4) {
            const int c = c0 + cc;
            tile[ol][cc] = (o < R && c < N) ? dwf[fold_index(c, K, d.c_in, R, o)] : 0.f;
        }
    }
    __syncthreads();
    const bool vec = (N & 3) == 0 && al16(dw);
    const int cl = (threadIdx.x & 15) * 4, orow = threadIdx.x >> 4;
#pragma unroll
    for (int q = 0; q < kTile / 16; ++q) {
        const int r = orow + 16 * q, o = o0 + r, c = c0 + cl;
        if (o >= R || c >= N) continue;
        const float uo = u[o];
        f32x4 x;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float vv = c + i < N ? v[c + i] : 0.f;
            x[i] = __fmaf_rn(-coef, __fmul_rn(uo, vv), __fdiv_rn(tile[r][cl + i], sigma));
        }
        if (vec) {
            *reinterpret_cast<f32x4*>(dw + (size_t)o * N + c) = x;
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (c + i < N) dw[(size_t)o * N + c + i] = x[i];
        }
    }
}

inline bool ptr4(const void* p) { return p && (reinterpret_cast<uintptr_t>(p) & 3) == 0; }

int check_call(const void* descs_dev, int n, const v2w_sn_grids* g, const void* keep, const void* ws, long long ws_bytes) {
    if (!descs_dev || !g || !keep || !ws || n < 1 || n > V2W_SN_MAX_LAYERS) return V2W_E_ARG;
    if (g->n != n || g->grid_t < 1 || g->grid_r < 1 || g->grid_s < 1 || g->ws_bytes < 16 || ws_bytes < g->ws_bytes) return V2W_E_ARG;
    if (!v2w_al16(ws) || !v2w_al16(keep) || (reinterpret_cast<uintptr_t>(descs_dev) & 7)) return V2W_E_ARG;
    return 0;
}

}  // namespace

extern "C" long long v2w_sn_plan(v2w_sn_desc* descs, int n, v2w_sn_grids* g) {
    if (!descs || !g || n < 1 || n > V2W_SN_MAX_LAYERS) return V2W_E_ARG;
    long long bt = 0, br = 0, bs = 0, ws = 0, keep = 0;
    for (int i = 0; i < n; ++i) {
        v2w_sn_desc& d = descs[i];
        if (d.c_out <= 0 || d.c_in <= 0 || d.k <= 0) return V2W_E_ARG;
        if (!ptr4(d.w) || !ptr4(d.u) || !ptr4(d.v) || !ptr4(d.wf)) return V2W_E_ARG;
        const long long R = d.c_out, N = (long long)d.c_in * d.k;
        if (R * N > 0x7fffffffll) return V2W_E_SHAPE;                      // element indices stay below 2^31
        const long long nb = (R + kBand - 1) / kBand, tiles = ((R + kTile - 1) / kTile) * ((N + kTile - 1) / kTile);
        d.blk_t = (int32_t)bt; d.blk_r = (int32_t)br; d.blk_s = (int32_t)bs;
        d.ws_off = ws; d.keep_off = keep;
        bt += nb * ((N + kCols - 1) / kCols);
        br += (R + 3) / 4;
        bs += tiles;
        const long long need = nb * N + R > tiles ? nb * N + R : tiles;
        ws += (need + 3) & ~3ll;
        keep += 4 + ((R + 3) & ~3ll) + ((N + 3) & ~3ll);
        if (bt > 0x7fffffffll || bs > 0x7fffffffll) return V2W_E_SHAPE;
    }
    g->n = n; g->grid_t = (int32_t)bt; g->grid_r = (int32_t)br; g->grid_s = (int32_t)bs;
    g->ws_bytes = ws * 4; g->keep_bytes = keep * 4;
    return g->ws_bytes;
}

extern "C" int v2w_sn_step(const v2w_sn_desc* descs_dev, int n, int training, const v2w_sn_grids* g, float* keep, void* ws, long long ws_bytes,
                           void* stream) {
    if (const int rc = check_call(descs_dev, n, g, keep, ws, ws_bytes)) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (v2w_dry(st)) return 0;
    float* wsf = static_cast<float*>(ws);
    if (training) {
        V2W_LAUNCH(sn_wtu_kernel, dim3(g->grid_t), dim3(256), 0, st, descs_dev, n, wsf);
        V2W_LAUNCH(sn_v_kernel, dim3(n), dim3(1024), 0, st, descs_dev, wsf, keep);
    }
    V2W_LAUNCH(sn_wv_kernel, dim3(g->grid_r), dim3(256), 0, st, descs_dev, n, wsf);
    V2W_LAUNCH(sn_scale_kernel, dim3(g->grid_s), dim3(256), 0, st, descs_dev, n, training ? 1 : 0, (const float*)wsf, keep);
    return v2w_launch_status();
}

extern "C" int v2w_sn_bwd(const v2w_sn_desc* descs_dev, int n, const v2w_sn_grids* g, const float* keep, const float* const* dwf,
                          float* const* dw, void* ws, long long ws_bytes, void* stream) {
    if (const int rc = check_call(descs_dev, n, g, keep, ws, ws_bytes)) return rc;
    if (!dwf || !dw) return V2W_E_ARG;
    BwdPtrs P;
    int any = 0;
    for (int i = 0; i < V2W_SN_MAX_LAYERS; ++i) {
        P.dwf[i] = i < n ? dwf[i] : nullptr;
        P.dw[i] = i < n ? dw[i] : nullptr;
        if (i < n) {
            if ((P.dwf[i] == nullptr) != (P.dw[i] == nullptr)) return V2W_E_ARG;
            if (P.dwf[i] && (!ptr4(P.dwf[i]) || !ptr4(P.dw[i]))) return V2W_E_ARG;
            any |= P.dwf[i] != nullptr;
        }
    }
    if (!any) return V2W_E_ARG;
    hipStream_t st = (hipStream_t)stream;
    if (v2w_dry(st)) return 0;
    float* wsf = static_cast<float*>(ws);
    V2W_LAUNCH(sn_bwd_dot_kernel, dim3(g->grid_s), dim3(256), 0, st, descs_dev, n, P, wsf);
    V2W_LAUNCH(sn_bwd_apply_kernel, dim3(g->grid_s), dim3(256), 0, st, descs_dev, n, P, (const float*)wsf, keep);
    return v2w_launch_status();
}
