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

// v2w_mel_finish's magnitude with the three operations under the root spelled out (no contraction left to the compiler): the two signals'
// magnitudes are then the same function of their operands, and equal spectra give X == Y bit for bit
__device__ __forceinline__ float sl_mag(float re, float im) {
    return sqrtf(__fadd_rn(__fmaf_rn(im, im, __fmul_rn(re, re)), 1e-9f));
}

// part[3 wg + {0, 1, 2}] = the workgroup's sums of (Y - X)^2, Y^2 and |log Y - log X| (fp64)
__global__ void __launch_bounds__(kThreads)
stft_loss_sums_kernel(const SlArgs A, double* __restrict__ part) {
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
            const size_t o = (size_t)b * plane + (size_t)c * FP + (q << 2);
            xr[k] = *reinterpret_cast<const f32x4*>(it.x + o);
            xi[k] = *reinterpret_cast<const f32x4*>(it.x + o + im_off);
            yr[k] = *reinterpret_cast<const f32x4*>(it.y + o);
            yi[k] = *reinterpret_cast<const f32x4*>(it.y + o + im_off);
            const int left = F - (int)(q << 2);
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

// sums[3 r + s] = resolution r's partials of sum s: thread t adds the partials t, t + 256, ... in index order, the 256 sums go through the
// fixed-order block reduction; sc[r] = sqrt(Sd) / sqrt(Sy), mag[r] = Sl / N, total = the means over r in list order; all in fp64
__global__ void __launch_bounds__(kThreads)
stft_loss_finish_kernel(const SlArgs A, const double* __restrict__ part, float* __restrict__ sc, float* __restrict__ mag,
                        float* __restrict__ total, double* __restrict__ sums) {
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
        const double N = (double)it.B * (double)it.nb * (double)it.F;
        const double vsc = sqrt(s[0]) / sqrt(s[1]), vmag = s[2] / N;             // (Sy >= N * 1e-9 > 0)
        if (threadIdx.x == 0) {
            if (sums) { sums[3 * i] = s[0]; sums[3 * i + 1] = s[1]; sums[3 * i + 2] = s[2]; }
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

// dspec_x: see the head of this file and include/vec2wav_hip.h for the arithmetic, one fp32 operation per line there
__global__ void __launch_bounds__(kThreads)
stft_loss_bwd_kernel(const SlArgs A, const SlGrads G, const double* __restrict__ sums) {
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
    const double Sd = sums[3 * i], Sy = sums[3 * i + 1];
    const float csc = Sd > 0.0 ? (float)((double)gs / (sqrt(Sd) * sqrt(Sy))) : 0.f;          // torch's subgradient of a norm at 0
    const float cmag = (float)((double)gm / ((double)it.B * (double)nb * (double)F));

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
            const int left = F - (int)(q << 2);
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
    if (!scratch || (!sc && !mag && !total && !sums)) return V2W_E_ARG;
    if ((reinterpret_cast<uintptr_t>(scratch) & 7) || (reinterpret_cast<uintptr_t>(sums) & 7)) return V2W_E_ARG;
    if ((sc && !ptr4(sc)) || (mag && !ptr4(mag)) || (total && !ptr4(total))) return V2W_E_ARG;
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
    if (!sums || (reinterpret_cast<uintptr_t>(sums) & 7) || (!g_sc && !g_mag && !gterm_sc && !gterm_mag)) return V2W_E_ARG;
    if ((g_sc && !ptr4(g_sc)) || (g_mag && !ptr4(g_mag)) || (gterm_sc && !ptr4(gterm_sc)) || (gterm_mag && !ptr4(gterm_mag))) return V2W_E_ARG;
    SlArgs A;
    if (const int rc = sl_args(items, n, true, &A)) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (v2w_dry(st)) return 0;
    const SlGrads G = {g_sc, g_mag, gterm_sc, gterm_mag};
    V2W_LAUNCH(stft_loss_bwd_kernel, dim3(A.starts[n]), dim3(kThreads), 0, st, A, G, sums);
    return v2w_launch_status();
}
