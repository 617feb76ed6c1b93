// Band-limited rational-ratio sample-rate conversion (the polyphase form of torchaudio.functional.resample's Hann-windowed sinc) and peak
// normalisation (librosa.util.normalize(y) * peak), per item of a batch of unequal lengths.  include/vec2wav_hip.h states the arithmetic;
// audio.py builds the table.
//
//   y[b][q L + p] = sum_{j < NT} h[p][j] * x[b][q M + k0[p] + j]        x = 0 outside [0, n_b), fp32, fma in tap order j = 0 .. NT - 1
//
// resample_kernel: workgroup (b, tile) owns the outputs [tile * T, (tile + 1) * T) of item b.  It copies the (L, NT) table and k0 to LDS, the
// table's rows NT | 1 floats apart (an odd pitch: the lanes of a wave hold consecutive phases p, and 32 rows an odd number of words apart
// lie on 32 banks; at NT = 34 the plain pitch would put them two to a bank), and stages the input window of its outputs once, as float -
// int16 PCM times 2^-15, exact - with zeros for the samples outside [0, n_b): x[b][n_b ..] is never loaded.  The window of the outputs
// [o0, oe] starts at (o0 / L) M + k0[0] and ends at (oe / L) M + k0[L - 1] + NT - 1, because k0 does not decrease with p.  Each thread then
// walks outputs 256 apart: one division by L, NT times (two LDS reads, one fma).  Outputs at or past N_b = ceil(L n_b / M) are stored as +0.0
// by the workgroup that owns them, and a tile with none below N_b loads nothing.  With peak_part the workgroup stores the maximum of |y| over
// its tile (a max of floats is exact in any order).
//
// peak_scale_kernel: every workgroup of an item takes the maximum of the item's partials for itself and multiplies its 4096 floats of the row
// by peak / max: one division, one multiplication per entry.  A maximum below FLT_MIN (or NaN) leaves the row as it is.
#include <float.h>
#include "v2w_common.h"

namespace {

constexpr int kRsThreads = 256;
constexpr int kRsTileMax = 4096, kRsTileMin = 256;       // outputs per workgroup: the largest power of two between them whose LDS fits
constexpr long long kRsLdsLimit = 64 * 1024;
constexpr int kPsChunk = 4096;                           // floats of a row per workgroup of peak_scale_kernel

struct RsArgs {
    const void* x; float* y; const float* h; const int* k0; const int* len; float* peak_part;
    int in_i16, Lin, Lout, M, L, NT, tile, tiles, wcap;
};

__host__ __device__ inline int rs_pitch(int NT) { return NT | 1; }
// floats of the staged window a tile of T outputs can need: its outputs span at most (T - 1) / L + 1 steps of M, k0 at most one more
inline long long rs_window(int M, int L, int NT, int T) { return ((long long)((T - 1) / L) + 2) * M + NT; }
inline long long rs_lds_bytes(int M, int L, int NT, int T) {
    return 4 * ((long long)L * rs_pitch(NT) + L + rs_window(M, L, NT, T) + 4);
}

__device__ __forceinline__ float rs_block_max(float v, float* red) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

__global__ void __launch_bounds__(kRsThreads)
resample_kernel(const RsArgs A) {
    extern __shared__ __align__(16) float rs_lds[];
    const int M = A.M, L = A.L, NT = A.NT, P = rs_pitch(NT);
    float* hs = rs_lds;                                         // [L][P]
    int* ks = reinterpret_cast<int*>(hs + (size_t)L * P);       // [L]
    float* xs = reinterpret_cast<float*>(ks + L);               // [wcap]
    float* red = xs + A.wcap;                                   // [4]
    const unsigned b = blockIdx.x / (unsigned)A.tiles, tile = blockIdx.x - b * (unsigned)A.tiles;
    const unsigned o0 = tile * (unsigned)A.tile;                // (< Lout)
    const unsigned left = (unsigned)A.Lout - o0;
    const unsigned o1 = o0 + (left < (unsigned)A.tile ? left : (unsigned)A.tile);
    long long n = A.Lin;
    if (A.len) {
        const int v = A.len[b];
        n = v < 0 ? 0 : (v < A.Lin ? v : A.Lin);
    }
    const long long N = (n * L + M - 1) / M;                    // (<= Lout: the host checked Lout >= ceil(L Lin / M))
    float* yb = A.y + (size_t)b * (size_t)A.Lout;
    float mx = 0.f;
    if ((long long)o0 < N) {                                    // uniform over the workgroup
        for (int i = threadIdx.x; i < L * NT; i += kRsThreads) {
            const int p = i / NT;
            hs[p * P + (i - p * NT)] = A.h[i];
        }
        for (int i = threadIdx.x; i < L; i += kRsThreads) ks[i] = A.k0[i];
        const int kfirst = A.k0[0], klast = A.k0[L - 1];
        const unsigned oe = ((long long)o1 < N ? o1 : (unsigned)N) - 1;        // the last output below N_b
        const unsigned q0 = o0 / (unsigned)L, q1 = oe / (unsigned)L;
        const long long s0 = (long long)q0 * M + kfirst;
        long long wl = (long long)(q1 - q0) * M + ((long long)klast - kfirst) + NT;
        wl = wl < 0 ? 0 : (wl < A.wcap ? wl : A.wcap);          // (a table whose k0 decreases, or spans more than M, is cut to the buffer)
        const size_t xo = (size_t)b * (size_t)A.Lin;
        for (int w = threadIdx.x; w < (int)wl; w += kRsThreads) {
            const long long s = s0 + w;
            float v = 0.f;
            if (s >= 0 && s < n)
                v = A.in_i16 ? (float)static_cast<const int16_t*>(A.x)[xo + s] * 0.000030517578125f : static_cast<const float*>(A.x)[xo + s];
            xs[w] = v;
        }
        __syncthreads();
        for (unsigned o = o0 + threadIdx.x; o < o1; o += kRsThreads) {
            float acc = 0.f;
            if ((long long)o < N) {
                const unsigned q = o / (unsigned)L, p = o - q * (unsigned)L;
                const long long st = (long long)(q - q0) * M + ((long long)ks[p] - kfirst);      // tap 0 in the window
                const float* hp = hs + p * P;
                if (st >= 0 && st + NT <= wl) {
                    const float* xp = xs + st;
                    for (int j = 0; j < NT; ++j) acc = fmaf(hp[j], xp[j], acc);
                } else {                                        // (only under a table that breaks the header's condition on k0)
                    for (int j = 0; j < NT; ++j) {
                        const long long w = st + j;
                        acc = fmaf(hp[j], w >= 0 && w < wl ? xs[w] : 0.f, acc);
                    }
                }
            }
            yb[o] = acc;
            mx = fmaxf(mx, fabsf(acc));
        }
    } else {
        for (unsigned o = o0 + threadIdx.x; o < o1; o += kRsThreads) yb[o] = 0.f;
    }
    if (A.peak_part) {                                          // uniform
        mx = rs_block_max(mx, red);
        if (threadIdx.x == 0) A.peak_part[(size_t)b * A.tiles + tile] = mx;
    }
}

__global__ void __launch_bounds__(kRsThreads)
peak_scale_kernel(float* __restrict__ y, int Lout, const float* __restrict__ part, int parts, int chunks, float peak) {
    __shared__ float red[4];
    const unsigned b = blockIdx.x / (unsigned)chunks, c = blockIdx.x - b * (unsigned)chunks;
    float m = 0.f;
    for (int i = threadIdx.x; i < parts; i += kRsThreads) m = fmaxf(m, part[(size_t)b * parts + i]);
    m = rs_block_max(m, red);
    if (!(m >= FLT_MIN)) return;                                // uniform: the row keeps its bits
    const float s = peak / m;
    float* yb = y + (size_t)b * (size_t)Lout;
    const unsigned i0 = c * (unsigned)kPsChunk, left = (unsigned)Lout - i0;
    const unsigned i1 = i0 + (left < (unsigned)kPsChunk ? left : (unsigned)kPsChunk);
    for (unsigned i = i0 + threadIdx.x; i < i1; i += kRsThreads) yb[i] = yb[i] * s;
}

inline bool rs_ptr(const void* p, unsigned mask) { return p && (reinterpret_cast<uintptr_t>(p) & mask) == 0; }

int rs_plan(int M, int L, int NT, int B, int Lout, v2w_resample_grids* g) {
    if (!g || M <= 0 || L <= 0 || NT <= 0 || B <= 0 || Lout <= 0) return V2W_E_ARG;
    int T = kRsTileMax;
    while (T > kRsTileMin && rs_lds_bytes(M, L, NT, T) > kRsLdsLimit) T >>= 1;
    if (rs_lds_bytes(M, L, NT, T) > kRsLdsLimit) return V2W_E_SHAPE;
    const long long tiles = ((long long)Lout + T - 1) / T;
    if (tiles * B > 0x7fffffffll) return V2W_E_SHAPE;
    g->tile = T;
    g->tiles = (int32_t)tiles;
    g->grid = (int32_t)(tiles * B);
    g->lds_bytes = (int32_t)rs_lds_bytes(M, L, NT, T);
    return 0;
}

}  // namespace

extern "C" int v2w_resample_plan(int M, int L, int NT, int B, int Lout, v2w_resample_grids* g) { return rs_plan(M, L, NT, B, Lout, g); }

extern "C" int v2w_resample(const void* x, int in_i16, float* y, int B, int Lin, int Lout, const float* h, const int32_t* k0, int M, int L,
                            int NT, const int32_t* len, float* peak_part, void* stream) {
    if (!rs_ptr(x, in_i16 ? 1 : 3) || !rs_ptr(y, 3) || !rs_ptr(h, 3) || !rs_ptr(k0, 3)) return V2W_E_ARG;
    if ((len && !rs_ptr(len, 3)) || (peak_part && !rs_ptr(peak_part, 3))) return V2W_E_ARG;
    if (B <= 0 || Lin <= 0 || Lout <= 0 || M <= 0 || L <= 0 || NT <= 0) return V2W_E_ARG;
    if ((long long)Lout < ((long long)L * Lin + M - 1) / M) return V2W_E_ARG;
    v2w_resample_grids g;
    if (const int rc = rs_plan(M, L, NT, B, Lout, &g)) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (v2w_dry(st)) return 0;
    const RsArgs A = {x, y, h, k0, len, peak_part, in_i16 != 0, Lin, Lout, M, L, NT, g.tile, g.tiles, (int)rs_window(M, L, NT, g.tile)};
    return v2w_launch_lds(resample_kernel, dim3(g.grid), dim3(kRsThreads), (size_t)g.lds_bytes, st, A);
}

extern "C" int v2w_peak_scale(float* y, int B, int Lout, const float* peak_part, int parts, float peak, void* stream) {
    if (!rs_ptr(y, 3) || !rs_ptr(peak_part, 3) || B <= 0 || Lout <= 0 || parts <= 0) return V2W_E_ARG;
    if (!(peak > 0.f) || !(peak <= FLT_MAX)) return V2W_E_ARG;
    const long long chunks = ((long long)Lout + kPsChunk - 1) / kPsChunk;
    if (chunks * B > 0x7fffffffll) return V2W_E_SHAPE;
    hipStream_t st = (hipStream_t)stream;
    if (v2w_dry(st)) return 0;
    V2W_LAUNCH(peak_scale_kernel, dim3((unsigned)(chunks * B)), dim3(kRsThreads), 0, st, y, Lout, peak_part, parts, (int)chunks, peak);
    return v2w_launch_status();
}
