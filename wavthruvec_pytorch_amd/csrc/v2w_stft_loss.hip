// Multi-resolution STFT loss (Yamamoto et al., Parallel WaveGAN: spectral convergence + log-magnitude L1 over several STFT resolutions) on
// the DFT conv's output as mel.py's forward leaves it: spec (B, Cs, FP), rows [0, nb) Re, rows [nb, 2 nb) Im, the rows [2 nb, Cs) and the
// columns [F, FP) not part of the spectrum (the columns hold finite junk).  Every resolution of a call in one launch per step, in the
// style of v2w_loss.hip: the table of up to V2W_STFT_LOSS_MAX_ITEMS descriptors travels by value, workgroups are dealt by v2w_multi.h's plan
// - here one resolution at a time, so that a resolution's workgroups, and with them its bits, depend on its own descriptor only - and a
// workgroup finds its resolution with find_item and its share with chunk_of.
//
// A UNIT is four consecutive frames of one (item, bin): four 16-byte loads (Re and Im of both signals; FP % 4 == 0 and 16-byte aligned bases
// keep every row on a 16-byte line, and 4 q + 3 < FP keeps the whole load inside the row).  Frames at or past F are SELECTED away after the
// arithmetic (never multiplied by a mask): Inf or NaN made from the junk there reaches nothing.  The forward counts B * nb * ceil(F / 4) units.
// The backward writes EVERY float of dspec_x once: its units are B * (nb + P) * (FP / 4), P = ceil((Cs - 2 nb) / 2) pairs of pad rows that get
// +0.0 like the columns [F, FP) of the other rows, so the caller's buffer needs no zero fill.
//
// Per-item lengths (v2w_stft_loss_multi_len, _len_bwd): the same three device bodies with LEN = true.  Item b of resolution i counts
// F_b = v2w_item_frames(len, b, len_mul, hop[i], n_fft[i], F) frames - F above becomes F_b, nothing else changes: the units, the grids and the
// chunks are the dense call's (they depend on the shapes only), a unit at or past F_b loads nothing, and with every F_b == F every value has
// the dense call's bits.  The finishing launch counts N = nb * sum_b F_b once and leaves it in sums[4 i + 3] for the backward.
#include "v2w_multi.h"

namespace {

constexpr int kUnroll = 2;                       // units in flight per thread: 2 x 4 x 16 B of loads before the first use

struct SlItem { const float* x; const float* y; float* dx; int B, Cs, FP, F, nb; };
struct SlArgs {
    SlItem it[V2W_STFT_LOSS_MAX_ITEMS];
    int starts[V2W_STFT_LOSS_MAX_ITEMS + 1];
    int n;
};
struct SlGrads { const float* g_sc; const float* g_mag; const float* gterm_sc; const float* gterm_mag; };
struct SlLen {                                   // LEN: the items' lengths (device) and every resolution's frame geometry
    const int32_t* len;
    int len_mul;
    int hop[V2W_STFT_LOSS_MAX_ITEMS], n_fft[V2W_STFT_LOSS_MAX_ITEMS];
};

// LEN: the frames item b counts, kept from unit to unit (a thread's units change their item every nb * Q units or more, and the count
// costs a 64-bit division)
struct SlFrames {
    unsigned b = ~0u;
    int Fb = 0;
    __device__ __forceinline__ int of(const SlLen& Ln, int i, unsigned item, int F) {
        if (item != b) {
            b = item;
            Fb = v2w_item_frames(Ln.len, (int)item, Ln.len_mul, Ln.hop[i], Ln.n_fft[i], F);
        }
        return Fb;
    }
};

// v2w_mel_finish's magnitude with the three operations under the root spelled out (no contraction left to the compiler): the two signals'
// magnitudes are then the same function of their operands, and equal spectra give X == Y bit for bit
__device__ __forceinline__ float sl_mag(float re, float im) {
    return sqrtf(__fadd_rn(__fmaf_rn(im, im, __fmul_rn(re, re)), 1e-9f));
}

// part[3 wg + {0, 1, 2}] = the workgroup's sums of (Y - X)^2, Y^2 and |log Y - log X| (fp64)
template <bool LEN>
__device__ __forceinline__ void sl_sums(const SlArgs& A, const SlLen& Ln, double* __restrict__ part) {
    __shared__ double red[16];
    const int wg = blockIdx.x;
    const int i = find_item(A.starts, A.n, wg);
    const SlItem& it = A.it[i];
    const unsigned nb = it.nb, FP = it.FP, Q = (unsigned)(it.F + 3) >> 2;
    const int F = it.F;
    const size_t plane = (size_t)it.Cs * FP, im_off = (size_t)nb * FP;
    long long u0;
    unsigned cnt;
    chunk_of(A.starts, i, wg, (long long)it.B * nb * Q, u0, cnt);
    const unsigned base = (unsigned)u0;                       // (units < 2^31: B * Cs * FP is)

    double sd = 0.0, sy = 0.0, sl = 0.0;
    SlFrames fr;
    for (unsigned t0 = threadIdx.x; t0 < cnt; t0 += kThreads * kUnroll) {
        f32x4 xr[kUnroll], xi[kUnroll], yr[kUnroll], yi[kUnroll];
        int e1[kUnroll];                                      // frames of the unit that count
#pragma unroll
        for (int k = 0; k < kUnroll; ++k) {
            const unsigned t = t0 + k * kThreads;
            xr[k] = xi[k] = yr[k] = yi[k] = f32x4{0.f, 0.f, 0.f, 0.f};
            e1[k] = 0;
            if (t >= cnt) continue;
            const unsigned u = base + t, row = u / Q, q = u - row * Q, b = row / nb, c = row - b * nb;
            const int Fb = LEN ? fr.of(Ln, i, b, F) : F;
            const int left = Fb - (int)(q << 2);
            if (LEN && left <= 0) continue;                   // the unit lies at or past the item's frames: no load, nothing added
            const size_t o = (size_t)b * plane + (size_t)c * FP + (q << 2);
            xr[k] = *reinterpret_cast<const f32x4*>(it.x + o);
            xi[k] = *reinterpret_cast<const f32x4*>(it.x + o + im_off);
            yr[k] = *reinterpret_cast<const f32x4*>(it.y + o);
            yi[k] = *reinterpret_cast<const f32x4*>(it.y + o + im_off);
            e1[k] = left < 4 ? left : 4;
        }
#pragma unroll
        for (int k = 0; k < kUnroll; ++k)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float X = sl_mag(xr[k][j], xi[k][j]), Y = sl_mag(yr[k][j], yi[k][j]);
                const float d = Y - X, l = fabsf(logf(Y) - logf(X));
                const bool in = j < e1[k];
                sd += in ? (double)d * (double)d : 0.0;
                sy += in ? (double)Y * (double)Y : 0.0;
                sl += in ? (double)l : 0.0;
            }
    }
    sd = v2w_block_sum(sd, red);
    sy = v2w_block_sum(sy, red);
    sl = v2w_block_sum(sl, red);
    if (threadIdx.x == 0) {
        part[3 * (size_t)wg] = sd;
        part[3 * (size_t)wg + 1] = sy;
        part[3 * (size_t)wg + 2] = sl;
    }
}
__global__ void __launch_bounds__(kThreads) stft_loss_sums_kernel(const SlArgs A, double* __restrict__ part) {
    sl_sums<false>(A, SlLen{}, part);
}
__global__ void __launch_bounds__(kThreads) stft_loss_sums_len_kernel(const SlArgs A, const SlLen Ln, double* __restrict__ part) {
    sl_sums<true>(A, Ln, part);
}

// sums[3 r + s] = resolution r's partials of sum s: thread t adds the partials t, t + 256, ... in index order, the 256 sums go through the
// fixed-order block reduction; sc[r] = sqrt(Sd) / sqrt(Sy), mag[r] = Sl / N, total = the means over r in list order; all in fp64.
// LEN: N = nb * sum_b F_b (the counts added as fp64 integers: exact), sums[4 r + {0, 1, 2, 3}] = (Sd, Sy, Sl, N), sc = mag = 0 for N == 0
template <bool LEN>
__device__ __forceinline__ void sl_finish(const SlArgs& A, const SlLen& Ln, const double* __restrict__ part, float* __restrict__ sc,
                                          float* __restrict__ mag, float* __restrict__ total, double* __restrict__ sums) {
    __shared__ double red[16];
    double tsc = 0.0, tmag = 0.0;
    for (int i = 0; i < A.n; ++i) {
        double s[3] = {0.0, 0.0, 0.0};
        for (int k = A.starts[i] + threadIdx.x; k < A.starts[i + 1]; k += kThreads) {
            s[0] += part[3 * (size_t)k];
            s[1] += part[3 * (size_t)k + 1];
            s[2] += part[3 * (size_t)k + 2];
        }
#pragma unroll
        for (int j = 0; j < 3; ++j) s[j] = v2w_block_sum(s[j], red);
        const SlItem& it = A.it[i];
        double N = (double)it.B * (double)it.nb * (double)it.F;
        if (LEN) {
            double fr = 0.0;
            for (int b = threadIdx.x; b < it.B; b += kThreads)
                fr += (double)v2w_item_frames(Ln.len, b, Ln.len_mul, Ln.hop[i], Ln.n_fft[i], it.F);
            N = (double)it.nb * v2w_block_sum(fr, red);
        }
        const bool any = !LEN || N > 0.0;
        const double vsc = any ? sqrt(s[0]) / sqrt(s[1]) : 0.0, vmag = any ? s[2] / N : 0.0;             // (Sy >= N * 1e-9 > 0)
        if (threadIdx.x == 0) {
            constexpr int S = LEN ? 4 : 3;
            if (sums) { sums[S * i] = s[0]; sums[S * i + 1] = s[1]; sums[S * i + 2] = s[2]; }
            if (LEN && sums) sums[S * i + 3] = N;
            if (sc) sc[i] = (float)vsc;
            if (mag) mag[i] = (float)vmag;
        }
        tsc += vsc;
        tmag += vmag;
    }
    if (threadIdx.x == 0 && total) {
        total[0] = (float)(tsc / (double)A.n);
        total[1] = (float)(tmag / (double)A.n);
    }
}
__global__ void __launch_bounds__(kThreads)
stft_loss_finish_kernel(const SlArgs A, const double* __restrict__ part, float* __restrict__ sc, float* __restrict__ mag,
                        float* __restrict__ total, double* __restrict__ sums) {
    sl_finish<false>(A, SlLen{}, part, sc, mag, total, sums);
}
__global__ void __launch_bounds__(kThreads)
stft_loss_finish_len_kernel(const SlArgs A, const SlLen Ln, const double* __restrict__ part, float* __restrict__ sc, float* __restrict__ mag,
                            float* __restrict__ total, double* __restrict__ sums) {
    sl_finish<true>(A, Ln, part, sc, mag, total, sums);
}

// dspec_x: see the head of this file and include/vec2wav_hip.h for the arithmetic, one fp32 operation per line there.
// LEN: sums holds four doubles per resolution, the fourth the forward's N (c_mag = 0 for N == 0)
template <bool LEN>
__device__ __forceinline__ void sl_bwd(const SlArgs& A, const SlLen& Ln, const SlGrads& G, const double* __restrict__ sums) {
    const int wg = blockIdx.x;
    const int i = find_item(A.starts, A.n, wg);
    const SlItem& it = A.it[i];
    const unsigned nb = it.nb, FP = it.FP, QP = FP >> 2, Cs = it.Cs;
    const unsigned rp = nb + ((Cs - 2 * nb + 1) >> 1);       // row pairs per item: the bins, then the pad rows two at a time
    const int F = it.F;
    const size_t plane = (size_t)Cs * FP, im_off = (size_t)nb * FP;
    long long u0;
    unsigned cnt;
    chunk_of(A.starts, i, wg, (long long)it.B * rp * QP, u0, cnt);
    const unsigned base = (unsigned)u0;

    const float fn = (float)A.n;
    const float gs = (G.g_sc ? G.g_sc[0] / fn : 0.f) + (G.gterm_sc ? G.gterm_sc[i] : 0.f);
    const float gm = (G.g_mag ? G.g_mag[0] / fn : 0.f) + (G.gterm_mag ? G.gterm_mag[i] : 0.f);
    constexpr int S = LEN ? 4 : 3;
    const double Sd = sums[S * i], Sy = sums[S * i + 1];
    const double N = LEN ? sums[S * i + 3] : (double)it.B * (double)nb * (double)F;
    const float csc = Sd > 0.0 ? (float)((double)gs / (sqrt(Sd) * sqrt(Sy))) : 0.f;          // torch's subgradient of a norm at 0
    const float cmag = !LEN || N > 0.0 ? (float)((double)gm / N) : 0.f;

    SlFrames fr;
    for (unsigned t0 = threadIdx.x; t0 < cnt; t0 += kThreads * kUnroll) {
        f32x4 xr[kUnroll], xi[kUnroll], yr[kUnroll], yi[kUnroll];
        size_t oo[kUnroll];
        int e1[kUnroll];                                      // frames of the unit that count; -1: a pair of pad rows, -2: no unit
        bool two[kUnroll];
#pragma unroll
        for (int k = 0; k < kUnroll; ++k) {
            const unsigned t = t0 + k * kThreads;
            xr[k] = xi[k] = yr[k] = yi[k] = f32x4{0.f, 0.f, 0.f, 0.f};
            e1[k] = -2; oo[k] = 0; two[k] = false;
            if (t >= cnt) continue;
            const unsigned u = base + t, row = u / QP, q = u - row * QP, b = row / rp, c = row - b * rp;
            if (c >= nb) {                                    // pad rows 2 nb + 2 (c - nb) and, below Cs, the next one
                const unsigned r0 = 2 * nb + 2 * (c - nb);
                oo[k] = (size_t)b * plane + (size_t)r0 * FP + (q << 2);
                two[k] = r0 + 1 < Cs;
                e1[k] = -1;
                continue;
            }
            oo[k] = (size_t)b * plane + (size_t)c * FP + (q << 2);
            const int Fb = LEN ? fr.of(Ln, i, b, F) : F;
            const int left = Fb - (int)(q << 2);
            e1[k] = left < 0 ? 0 : (left < 4 ? left : 4);
            if (e1[k] > 0) {
                xr[k] = *reinterpret_cast<const f32x4*>(it.x + oo[k]);
                xi[k] = *reinterpret_cast<const f32x4*>(it.x + oo[k] + im_off);
                yr[k] = *reinterpret_cast<const f32x4*>(it.y + oo[k]);
                yi[k] = *reinterpret_cast<const f32x4*>(it.y + oo[k] + im_off);
            }
        }
#pragma unroll
        for (int k = 0; k < kUnroll; ++k) {
            if (e1[k] == -2) continue;
            f32x4 dre = {0.f, 0.f, 0.f, 0.f}, dim = {0.f, 0.f, 0.f, 0.f};
            if (e1[k] == -1) {
                *reinterpret_cast<f32x4*>(it.dx + oo[k]) = dre;
                if (two[k]) *reinterpret_cast<f32x4*>(it.dx + oo[k] + FP) = dre;
                continue;
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float X = sl_mag(xr[k][j], xi[k][j]), Y = sl_mag(yr[k][j], yi[k][j]);
                const float d = X - Y;
                const float r = 1.f / X;
                const float m = cmag * r;
                const float ms = d > 0.f ? m : (d < 0.f ? -m : 0.f);
                const float dX = fmaf(csc, d, ms);
                const float w = dX * r;
                const bool in = j < e1[k];
                dre[j] = in ? w * xr[k][j] : 0.f;
                dim[j] = in ? w * xi[k][j] : 0.f;
            }
            *reinterpret_cast<f32x4*>(it.dx + oo[k]) = dre;
            *reinterpret_cast<f32x4*>(it.dx + oo[k] + im_off) = dim;
        }
    }
}
__global__ void __launch_bounds__(kThreads) stft_loss_bwd_kernel(const SlArgs A, const SlGrads G, const double* __restrict__ sums) {
    sl_bwd<false>(A, SlLen{}, G, sums);
}
__global__ void __launch_bounds__(kThreads)
stft_loss_bwd_len_kernel(const SlArgs A, const SlLen Ln, const SlGrads G, const double* __restrict__ sums) {
    sl_bwd<true>(A, Ln, G, sums);
}

// checks every descriptor and counts its units (four frames of one row pair; see the head of this file)
int sl_items(const v2w_stft_loss_item* items, int n, bool bwd, SlItem* out, long long* units) {
    if (!items || n < 1 || n > V2W_STFT_LOSS_MAX_ITEMS) return V2W_E_ARG;
    for (int i = 0; i < n; ++i) {
        const v2w_stft_loss_item& p = items[i];
        if (!p.spec_x || !p.spec_y || (bwd && !p.dspec_x)) return V2W_E_ARG;
        if (p.B <= 0 || p.F <= 0 || p.nb <= 0 || p.FP < p.F || (long long)p.Cs < 2ll * p.nb) return V2W_E_ARG;
        if ((p.FP & 3) || !aligned16(p.spec_x) || !aligned16(p.spec_y) || (bwd && !aligned16(p.dspec_x))) return V2W_E_ARG;
        const long long plane = (long long)p.Cs * p.FP;
        if (plane > 0x7fffffffll || plane * p.B > 0x7fffffffll) return V2W_E_SHAPE;
        SlItem& it = out[i];
        it.x = p.spec_x; it.y = p.spec_y; it.dx = p.dspec_x;
        it.B = p.B; it.Cs = p.Cs; it.FP = p.FP; it.F = p.F; it.nb = p.nb;
        const long long pairs = bwd ? p.nb + (p.Cs - 2ll * p.nb + 1) / 2 : p.nb;
        units[i] = (long long)p.B * pairs * (bwd ? p.FP >> 2 : (p.F + 3) >> 2);
    }
    return 0;
}

// one resolution at a time: its workgroups depend on its own descriptor only
int sl_deal(const long long* units, int n, int32_t* starts) {
    int w = 0;
    for (int i = 0; i < n; ++i) {
        int32_t one[2];
        starts[i] = w;
        w += deal_workgroups(units + i, 1, V2W_STFT_LOSS_TARGET_WGS, one);
    }
    starts[n] = w;
    return w;
}

int sl_args(const v2w_stft_loss_item* items, int n, bool bwd, SlArgs* A) {
    long long units[V2W_STFT_LOSS_MAX_ITEMS];
    if (const int rc = sl_items(items, n, bwd, A->it, units)) return rc;
    sl_deal(units, n, A->starts);
    A->n = n;
    return 0;
}

// the lengths and the frame geometries of a _len call, after the descriptors passed sl_items
int sl_len(const v2w_stft_loss_item* items, int n, const int32_t* hop, const int32_t* n_fft, const int32_t* len, int len_mul, SlLen* Ln) {
    if (!hop || !n_fft || !len || len_mul < 1) return V2W_E_ARG;
    for (int i = 0; i < n; ++i)
        if (hop[i] < 1 || n_fft[i] < hop[i]) return V2W_E_ARG;
    for (int i = 0; i < n; ++i) {
        if (items[i].B > 65535 || (long long)items[i].F * hop[i] + n_fft[i] > 0x7fffffffll) return V2W_E_SHAPE;
        Ln->hop[i] = hop[i]; Ln->n_fft[i] = n_fft[i];
    }
    Ln->len = len; Ln->len_mul = len_mul;
    return 0;
}

int sl_fwd_ptrs(const float* sc, const float* mag, const float* total, const double* sums, const void* scratch) {
    if (!scratch || (!sc && !mag && !total && !sums)) return V2W_E_ARG;
    if ((reinterpret_cast<uintptr_t>(scratch) & 7) || (reinterpret_cast<uintptr_t>(sums) & 7)) return V2W_E_ARG;
    if ((sc && !ptr4(sc)) || (mag && !ptr4(mag)) || (total && !ptr4(total))) return V2W_E_ARG;
    return 0;
}

int sl_bwd_ptrs(const double* sums, const SlGrads& G) {
    if (!sums || (reinterpret_cast<uintptr_t>(sums) & 7) || (!G.g_sc && !G.g_mag && !G.gterm_sc && !G.gterm_mag)) return V2W_E_ARG;
    if ((G.g_sc && !ptr4(G.g_sc)) || (G.g_mag && !ptr4(G.g_mag)) || (G.gterm_sc && !ptr4(G.gterm_sc)) || (G.gterm_mag && !ptr4(G.gterm_mag)))
        return V2W_E_ARG;
    return 0;
}

}  // namespace

extern "C" int v2w_stft_loss_plan(const v2w_stft_loss_item* items, int n, int32_t* starts) {
    if (!starts) return V2W_E_ARG;
    SlItem its[V2W_STFT_LOSS_MAX_ITEMS];
    long long units[V2W_STFT_LOSS_MAX_ITEMS];
    if (const int rc = sl_items(items, n, false, its, units)) return rc;
    return sl_deal(units, n, starts);
}

extern "C" long long v2w_stft_loss_scratch_bytes(const v2w_stft_loss_item* items, int n) {
    int32_t starts[V2W_STFT_LOSS_MAX_ITEMS + 1];
    const int w = v2w_stft_loss_plan(items, n, starts);
    return w < 0 ? (long long)w : (long long)w * 3 * (long long)sizeof(double);
}

extern "C" int v2w_stft_loss_multi(const v2w_stft_loss_item* items, int n, float* sc, float* mag, float* total, double* sums,
                                   void* scratch, void* stream) {
    if (const int rc = sl_fwd_ptrs(sc, mag, total, sums, scratch)) return rc;
    SlArgs A;
    if (const int rc = sl_args(items, n, false, &A)) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (v2w_dry(st)) return 0;
    double* part = static_cast<double*>(scratch);
    V2W_LAUNCH(stft_loss_sums_kernel, dim3(A.starts[n]), dim3(kThreads), 0, st, A, part);
    V2W_LAUNCH(stft_loss_finish_kernel, dim3(1), dim3(kThreads), 0, st, A, part, sc, mag, total, sums);
    return v2w_launch_status();
}

extern "C" int v2w_stft_loss_multi_bwd(const v2w_stft_loss_item* items, int n, const double* sums, const float* g_sc, const float* g_mag,
                                       const float* gterm_sc, const float* gterm_mag, void* stream) {
    const SlGrads G = {g_sc, g_mag, gterm_sc, gterm_mag};
    if (const int rc = sl_bwd_ptrs(sums, G)) return rc;
    SlArgs A;
    if (const int rc = sl_args(items, n, true, &A)) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (v2w_dry(st)) return 0;
    V2W_LAUNCH(stft_loss_bwd_kernel, dim3(A.starts[n]), dim3(kThreads), 0, st, A, G, sums);
    return v2w_launch_status();
}

extern "C" int v2w_stft_loss_multi_len(const v2w_stft_loss_item* items, int n, const int32_t* hop, const int32_t* n_fft, const int32_t* len,
                                       int len_mul, float* sc, float* mag, float* total, double* sums, void* scratch, void* stream) {
    if (const int rc = sl_fwd_ptrs(sc, mag, total, sums, scratch)) return rc;
    SlArgs A;
    SlLen Ln;
    if (const int rc = sl_args(items, n, false, &A)) return rc;
    if (const int rc = sl_len(items, n, hop, n_fft, len, len_mul, &Ln)) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (v2w_dry(st)) return 0;
    double* part = static_cast<double*>(scratch);
    V2W_LAUNCH(stft_loss_sums_len_kernel, dim3(A.starts[n]), dim3(kThreads), 0, st, A, Ln, part);
    V2W_LAUNCH(stft_loss_finish_len_kernel, dim3(1), dim3(kThreads), 0, st, A, Ln, part, sc, mag, total, sums);
    return v2w_launch_status();
}

extern "C" int v2w_stft_loss_multi_len_bwd(const v2w_stft_loss_item* items, int n, const int32_t* hop, const int32_t* n_fft,
                                           const int32_t* len, int len_mul, const double* sums, const float* g_sc, const float* g_mag,
                                           const float* gterm_sc, const float* gterm_mag, void* stream) {
    const SlGrads G = {g_sc, g_mag, gterm_sc, gterm_mag};
    if (const int rc = sl_bwd_ptrs(sums, G)) return rc;
    SlArgs A;
    SlLen Ln;
    if (const int rc = sl_args(items, n, true, &A)) return rc;
    if (const int rc = sl_len(items, n, hop, n_fft, len, len_mul, &Ln)) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (v2w_dry(st)) return 0;
    V2W_LAUNCH(stft_loss_bwd_len_kernel, dim3(A.starts[n]), dim3(kThreads), 0, st, A, Ln, G, sums);
    return v2w_launch_status();
}
