// AdamW (torch.optim.AdamW as the reference calls it, train.py:96-99,198,215: decoupled weight decay, no amsgrad, no maximize): the step of
// up to V2W_ADAMW_MAX_ITEMS parameter tensors in ONE streaming launch.  One pass reads p, g, m, v and writes p, m, v (28 bytes per
// parameter); the arithmetic, its order and its fp32 roundings are stated in include/vec2wav_hip.h.
//
// Work split (host, v2w_adamw_multi_plan; the shape of v2w_l1_multi_plan): a tensor is cut into UNITS of four floats.  When the four
// pointers of an item share their 16-byte phase (s floats past a 16-byte line) the units are cut at the 16-byte lines - the first and the
// last one partial - and every whole unit is one 16-byte load / store per lane and tensor; otherwise the units start at element 0 and the
// item takes float-by-float accesses, chosen by a branch that is uniform over the workgroup.  Workgroups are dealt in proportion to the
// units (the parameter sizes of one call span six orders of magnitude), at least one per tensor, about V2W_ADAMW_TARGET_WGS in all:
// starts[i] is the first workgroup of tensor i, found from blockIdx.x by a search every lane makes alike.  The plan depends on the
// descriptors only.  Every element of p, m and v is written exactly once, nothing else is written; no atomics, no LDS, no scratch.
//
// Global-norm clipping and the non-finite guard (include/vec2wav_hip.h, v2w_grad_sumsq_multi and its neighbours) ride on the same table and
// plan: grad_sumsq_kernel writes one fp32 sum of squares per workgroup (fixed order, no atomics), grad_norm_finish_kernel adds them in fp64
// and leaves norm, clip coefficient, finite flag and a running count in four floats of the caller's, grad_scale_kernel is g *= coef[0], and
// adamw_multi_clipped_kernel is the step's body compiled with g * clip[1] for g - the coefficient never visits the host.
//
// The exponential moving average of the weights (include/vec2wav_hip.h, v2w_adamw_ema_multi and its neighbours): the step's body compiled
// twice more with a fifth tensor e per item - e' = fma(ema_omd, p' - e, e) while p' is in registers, 36 bytes per parameter - on a table of
// 48-byte items (AdamWEmaArgs, at most V2W_ADAMW_EMA_MAX_ITEMS), and two kernels on a table of {p, e, numel} items (PairArgs): the two lines
// alone and the exchange of p and e.  find_span and the plan are shared: they are written over the table's type.
#include "v2w_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kUnroll = 2;                       // units in flight per thread: 2 x 4 tensors x 16 B of loads before the first use
constexpr long long kMinChunk = kThreads * 8;    // units: no workgroup for less than 4 x 32 KB of reads unless the tensor is smaller
constexpr long long kMaxUnits = 1ll << 40;

// the launch's constants, each derived from the v2w_adamw_hyper in double and rounded ONCE to fp32 (host)
struct Coef { float decay, omb1, beta2, omb2, rbc2, eps, step; };

struct AdamWArgs {
    v2w_adamw_item it[V2W_ADAMW_MAX_ITEMS];
    int starts[V2W_ADAMW_MAX_ITEMS + 1];
    Coef c;
    int n;
};
static_assert(sizeof(v2w_adamw_item) == 40 && sizeof(v2w_adamw_hyper) == 32, "include/vec2wav_hip.h states these sizes");
static_assert(sizeof(AdamWArgs) <= 3584, "kernel arguments travel by value: 4 KB with the hidden ones");

// the step with the average: 48-byte items, the same constants and ema_omd = 1 - decay
struct AdamWEmaArgs {
    v2w_adamw_ema_item it[V2W_ADAMW_EMA_MAX_ITEMS];
    int starts[V2W_ADAMW_EMA_MAX_ITEMS + 1];
    Coef c;
    float omd;
    int n;
};
static_assert(sizeof(v2w_adamw_ema_item) == 48 && sizeof(v2w_ema_item) == 24 && sizeof(v2w_swap_item) == 24, "include/vec2wav_hip.h states these sizes");
static_assert(V2W_ADAMW_EMA_MAX_ITEMS * 48 + (V2W_ADAMW_EMA_MAX_ITEMS + 1) * 4 + sizeof(Coef) + 4 + 4 == sizeof(AdamWEmaArgs), "no padding");
static_assert(sizeof(AdamWEmaArgs) <= 3584, "kernel arguments travel by value: 4 KB with the hidden ones");

// {p, e, numel} items: Item is v2w_ema_item (p only read) or v2w_swap_item (both written)
template <class Item>
struct PairArgs {
    Item it[V2W_ADAMW_MAX_ITEMS];
    int starts[V2W_ADAMW_MAX_ITEMS + 1];
    int n;
};
static_assert(sizeof(PairArgs<v2w_ema_item>) <= 3584 && sizeof(PairArgs<v2w_swap_item>) == sizeof(PairArgs<v2w_ema_item>), "by-value table");

__host__ __device__ inline int phase16(const void* p) { return (int)((reinterpret_cast<uintptr_t>(p) >> 2) & 3); }
__host__ __device__ inline bool same_phase(const v2w_adamw_item& it) {
    const int ph = phase16(it.p);
    return phase16(it.g) == ph && phase16(it.m) == ph && phase16(it.v) == ph;
}
__host__ __device__ inline bool same_phase(const v2w_adamw_ema_item& it) {
    const int ph = phase16(it.p);
    return phase16(it.g) == ph && phase16(it.m) == ph && phase16(it.v) == ph && phase16(it.e) == ph;
}
__host__ __device__ inline bool same_phase(const v2w_ema_item& it) { return phase16(it.p) == phase16(it.e); }
__host__ __device__ inline bool same_phase(const v2w_swap_item& it) { return phase16(it.p) == phase16(it.e); }
template <class Item>
__host__ __device__ inline long long item_units(const Item& it) {
    return (it.numel + (same_phase(it) ? phase16(it.p) : 0) + 3) >> 2;
}

// elements [e0, e1) of the four floats at q (the others read as 0 and are never touched); one 16-byte access when all four are wanted
// and the item's pointers allow it (`vec`: q is then on a 16-byte line)
__device__ __forceinline__ f32x4 load_unit(const float* q, int e0, int e1, bool vec) {
    f32x4 x = {0.f, 0.f, 0.f, 0.f};
    if (vec && e0 == 0 && e1 == 4) return *reinterpret_cast<const f32x4*>(q);
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (j >= e0 && j < e1) x[j] = q[j];
    return x;
}
__device__ __forceinline__ void store_unit(float* q, f32x4 x, int e0, int e1, bool vec) {
    if (vec && e0 == 0 && e1 == 4) { *reinterpret_cast<f32x4*>(q) = x; return; }
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (j >= e0 && j < e1) q[j] = x[j];
}

// the chunk of workgroup wg: its tensor, and units [u0, u0 + cnt) of it
struct Span {
    int item;
    long long numel, base;      // base: element index of the first float of unit u0 (negative inside a partial first unit)
    unsigned cnt;
    bool vec;
};
template <class Args>
__device__ __forceinline__ Span find_span(const Args& A, int wg) {
    int lo = 0, hi = A.n;
    while (hi - lo > 1) {                                 // the tensor of this workgroup: starts[lo] <= wg < starts[lo + 1]
        const int mid = (lo + hi) >> 1;
        if (A.starts[mid] <= wg) lo = mid; else hi = mid;
    }
    const auto& it = A.it[lo];
    Span s;
    s.item = lo;
    s.numel = it.numel;
    s.vec = same_phase(it);
    const int shift = s.vec ? phase16(it.p) : 0;
    const long long units = (s.numel + shift + 3) >> 2;
    const int nwg = A.starts[lo + 1] - A.starts[lo];
    const long long chunk = (units + nwg - 1) / nwg;
    const long long u0 = (long long)(wg - A.starts[lo]) * chunk;
    const long long u1 = u0 + chunk < units ? u0 + chunk : units;
    s.cnt = u1 > u0 ? (unsigned)(u1 - u0) : 0u;
    // unit u holds elements [4u - shift, 4u - shift + 4) of the tensor; the floats before element 0 and past numel are masked
    s.base = (u0 << 2) - shift;
    return s;
}
// the floats [e0, e1) of unit t of the span that belong to the tensor (none for t >= cnt)
__device__ __forceinline__ void unit_mask(const Span& s, unsigned t, size_t off, int& e0, int& e1) {
    const long long pos = s.base + (long long)off;                    // element index of the unit's first float
    e0 = pos < 0 ? (int)-pos : 0;
    e1 = s.numel - pos < 4 ? (int)(s.numel - pos) : 4;
    if (t >= s.cnt) e0 = e1 = 0;
}

// CLIP: the step on g * coef (include/vec2wav_hip.h, v2w_adamw_multi_clipped); otherwise coef is not looked at.  EMA: the table is an
// AdamWEmaArgs and e' = fma(omd, p' - e, e) rides along (v2w_adamw_ema_multi); otherwise neither e nor omd exists
template <bool CLIP, bool EMA, class Args>
__device__ __forceinline__ void adamw_body(const Args& A, float coef) {
    const Span s = find_span(A, blockIdx.x);
    const auto& it = A.it[s.item];
    const bool vec = s.vec;
    float* p = it.p + s.base;
    const float* g = it.g + s.base;
    float* m = it.m + s.base;
    float* v = it.v + s.base;
    float* e = nullptr;
    float omd = 0.f;
    if constexpr (EMA) { e = it.e + s.base; omd = A.omd; }
    const Coef c = A.c;

    for (unsigned t0 = threadIdx.x; t0 < s.cnt; t0 += kThreads * kUnroll) {
        f32x4 xp[kUnroll], xg[kUnroll], xm[kUnroll], xv[kUnroll], xe[kUnroll];
        size_t off[kUnroll];
        int e0[kUnroll], e1[kUnroll];
#pragma unroll
        for (int k = 0; k < kUnroll; ++k) {
            const unsigned t = t0 + k * kThreads;
            off[k] = (size_t)t << 2;
            unit_mask(s, t, off[k], e0[k], e1[k]);
            xp[k] = load_unit(p + off[k], e0[k], e1[k], vec);
            xg[k] = load_unit(g + off[k], e0[k], e1[k], vec);
            xm[k] = load_unit(m + off[k], e0[k], e1[k], vec);
            xv[k] = load_unit(v + off[k], e0[k], e1[k], vec);
            if constexpr (EMA) xe[k] = load_unit(e + off[k], e0[k], e1[k], vec);
        }
#pragma unroll
        for (int k = 0; k < kUnroll; ++k) {
            f32x4 np, nm, nv, ne;
#pragma unroll
            for (int j = 0; j < 4; ++j) {                              // include/vec2wav_hip.h: one fp32 rounding per line
                const float gj = CLIP ? __fmul_rn(xg[k][j], coef) : xg[k][j];
                const float pd = __fmul_rn(xp[k][j], c.decay);
                const float d = __fsub_rn(gj, xm[k][j]);
                nm[j] = __fmaf_rn(c.omb1, d, xm[k][j]);
                const float gg = __fmul_rn(gj, gj);
                const float tg = __fmul_rn(c.omb2, gg);
                nv[j] = __fmaf_rn(c.beta2, xv[k][j], tg);
                const float den = __fmaf_rn(__fsqrt_rn(nv[j]), c.rbc2, c.eps);
                const float q = __fdiv_rn(nm[j], den);
                np[j] = __fmaf_rn(-c.step, q, pd);
                if constexpr (EMA) {
                    const float de = __fsub_rn(np[j], xe[k][j]);
                    ne[j] = __fmaf_rn(omd, de, xe[k][j]);
                }
            }
            store_unit(p + off[k], np, e0[k], e1[k], vec);
            store_unit(m + off[k], nm, e0[k], e1[k], vec);
            store_unit(v + off[k], nv, e0[k], e1[k], vec);
            if constexpr (EMA) store_unit(e + off[k], ne, e0[k], e1[k], vec);
        }
    }
}

__global__ void __launch_bounds__(kThreads)
adamw_multi_kernel(const AdamWArgs A) { adamw_body<false, false>(A, 1.f); }

// clip: the four floats of v2w_grad_norm_finish; a skipped step returns before the first load (the branch is uniform over the launch)
__global__ void __launch_bounds__(kThreads)
adamw_multi_clipped_kernel(const AdamWArgs A, const float* __restrict__ clip, int skip_nonfinite) {
    if (skip_nonfinite && clip[2] == 0.f) return;
    adamw_body<true, false>(A, clip[1]);
}

__global__ void __launch_bounds__(kThreads)
adamw_ema_multi_kernel(const AdamWEmaArgs A) { adamw_body<false, true>(A, 1.f); }

// a skipped step leaves the average alone too
__global__ void __launch_bounds__(kThreads)
adamw_ema_multi_clipped_kernel(const AdamWEmaArgs A, const float* __restrict__ clip, int skip_nonfinite) {
    if (skip_nonfinite && clip[2] == 0.f) return;
    adamw_body<true, true>(A, clip[1]);
}

// e' = fma(omd, p - e, e), every element of e once; p is only read
__global__ void __launch_bounds__(kThreads)
ema_multi_kernel(const PairArgs<v2w_ema_item> A, float omd) {
    const Span s = find_span(A, blockIdx.x);
    const float* p = A.it[s.item].p + s.base;
    float* e = A.it[s.item].e + s.base;
    for (unsigned t0 = threadIdx.x; t0 < s.cnt; t0 += kThreads * kUnroll) {
        f32x4 xp[kUnroll], xe[kUnroll];
        size_t off[kUnroll];
        int e0[kUnroll], e1[kUnroll];
#pragma unroll
        for (int k = 0; k < kUnroll; ++k) {
            const unsigned t = t0 + k * kThreads;
            off[k] = (size_t)t << 2;
            unit_mask(s, t, off[k], e0[k], e1[k]);
            xp[k] = load_unit(p + off[k], e0[k], e1[k], s.vec);
            xe[k] = load_unit(e + off[k], e0[k], e1[k], s.vec);
        }
#pragma unroll
        for (int k = 0; k < kUnroll; ++k) {
#pragma unroll
            for (int j = 0; j < 4; ++j) xe[k][j] = __fmaf_rn(omd, __fsub_rn(xp[k][j], xe[k][j]), xe[k][j]);
            store_unit(e + off[k], xe[k], e0[k], e1[k], s.vec);
        }
    }
}

// p <-> e: a thread loads both values of its units, then stores both; no element belongs to two threads
__global__ void __launch_bounds__(kThreads)
swap_multi_kernel(const PairArgs<v2w_swap_item> A) {
    const Span s = find_span(A, blockIdx.x);
    float* p = A.it[s.item].p + s.base;
    float* e = A.it[s.item].e + s.base;
    for (unsigned t0 = threadIdx.x; t0 < s.cnt; t0 += kThreads * kUnroll) {
        f32x4 xp[kUnroll], xe[kUnroll];
        size_t off[kUnroll];
        int e0[kUnroll], e1[kUnroll];
#pragma unroll
        for (int k = 0; k < kUnroll; ++k) {
            const unsigned t = t0 + k * kThreads;
            off[k] = (size_t)t << 2;
            unit_mask(s, t, off[k], e0[k], e1[k]);
            xp[k] = load_unit(p + off[k], e0[k], e1[k], s.vec);
            xe[k] = load_unit(e + off[k], e0[k], e1[k], s.vec);
        }
#pragma unroll
        for (int k = 0; k < kUnroll; ++k) {
            store_unit(p + off[k], xe[k], e0[k], e1[k], s.vec);
            store_unit(e + off[k], xp[k], e0[k], e1[k], s.vec);
        }
    }
}

// partials[wg] = sum of g^2 over the workgroup's chunk: per thread one fma chain over its units in order, then the fixed block sum.
// The items arrive with p = m = v = g: every span takes the 16-byte path.
__global__ void __launch_bounds__(kThreads)
grad_sumsq_kernel(const AdamWArgs A, float* __restrict__ partials) {
    __shared__ float red[16];
    const Span s = find_span(A, blockIdx.x);
    const float* g = A.it[s.item].g + s.base;
    float acc = 0.f;
    for (unsigned t0 = threadIdx.x; t0 < s.cnt; t0 += kThreads * kUnroll) {
        f32x4 x[kUnroll];
#pragma unroll
        for (int k = 0; k < kUnroll; ++k) {
            const unsigned t = t0 + k * kThreads;
            const size_t off = (size_t)t << 2;
            int e0, e1;
            unit_mask(s, t, off, e0, e1);
            x[k] = load_unit(g + off, e0, e1, s.vec);
        }
#pragma unroll
        for (int k = 0; k < kUnroll; ++k)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc = __fmaf_rn(x[k][j], x[k][j], acc);
    }
    const float sum = v2w_block_sum(acc, red);
    if (threadIdx.x == 0) partials[blockIdx.x] = sum;
}

// g *= coef[0], every element once
__global__ void __launch_bounds__(kThreads)
grad_scale_kernel(const AdamWArgs A, const float* __restrict__ coef) {
    const Span s = find_span(A, blockIdx.x);
    float* g = const_cast<float*>(A.it[s.item].g) + s.base;
    const float c = coef[0];
    for (unsigned t0 = threadIdx.x; t0 < s.cnt; t0 += kThreads * kUnroll) {
        f32x4 x[kUnroll];
        size_t off[kUnroll];
        int e0[kUnroll], e1[kUnroll];
#pragma unroll
        for (int k = 0; k < kUnroll; ++k) {
            const unsigned t = t0 + k * kThreads;
            off[k] = (size_t)t << 2;
            unit_mask(s, t, off[k], e0[k], e1[k]);
            x[k] = load_unit(g + off[k], e0[k], e1[k], s.vec);
        }
#pragma unroll
        for (int k = 0; k < kUnroll; ++k) {
#pragma unroll
            for (int j = 0; j < 4; ++j) x[k][j] = __fmul_rn(x[k][j], c);
            store_unit(g + off[k], x[k], e0[k], e1[k], s.vec);
        }
    }
}

// include/vec2wav_hip.h, v2w_grad_norm_finish: thread t adds its run of partials in index order, the 256 sums take the fixed block sum
__global__ void __launch_bounds__(kThreads)
grad_norm_finish_kernel(const float* __restrict__ partials, int n, float max_norm, float* out) {
    __shared__ double red[16];
    const int per = (n + kThreads - 1) / kThreads;
    const int k0 = threadIdx.x * per, k1 = k0 + per < n ? k0 + per : n;
    double acc = 0.0;
    for (int k = k0; k < k1; ++k) acc += (double)partials[k];
    const double S = v2w_block_sum(acc, red);
    if (threadIdx.x == 0) {
        const double nrm = sqrt(S);
        const float nf = (float)nrm;
        double c = (double)max_norm / (nrm + 1e-6);
        c = c > 1.0 ? 1.0 : c;                                         // a NaN stays one, as under torch.clamp
        const float fin = __builtin_isfinite(nf) ? 1.f : 0.f;
        const float count = out[3];
        out[0] = nf;
        out[1] = (float)c;
        out[2] = fin;
        out[3] = count + (1.f - fin);
    }
}

inline bool ptr4(const void* p) { return p && (reinterpret_cast<uintptr_t>(p) & 3) == 0; }
inline bool overlap(const void* a, const void* b, long long numel) {
    const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b), bytes = (uintptr_t)numel * 4;
    return x < y ? y - x < bytes : x - y < bytes;
}

// checks every descriptor and counts its units (four floats; see the head of this file)
int adamw_items(const v2w_adamw_item* items, int n, long long* units) {
    if (!items || n < 1 || n > V2W_ADAMW_MAX_ITEMS) return V2W_E_ARG;
    for (int i = 0; i < n; ++i) {
        const v2w_adamw_item& it = items[i];
        if (!ptr4(it.p) || !ptr4(it.g) || !ptr4(it.m) || !ptr4(it.v) || it.numel <= 0) return V2W_E_ARG;
        if (it.numel > (kMaxUnits << 2)) return V2W_E_SHAPE;
        units[i] = item_units(it);
        if (units[i] > kMaxUnits) return V2W_E_SHAPE;
        if (overlap(it.p, it.m, it.numel) || overlap(it.p, it.v, it.numel) || overlap(it.m, it.v, it.numel)) return V2W_E_ARG;
    }
    return 0;
}

// v2w_adamw_ema_item: the checks above, and e against p, m and v
int adamw_ema_items(const v2w_adamw_ema_item* items, int n, long long* units) {
    if (!items || n < 1 || n > V2W_ADAMW_EMA_MAX_ITEMS) return V2W_E_ARG;
    for (int i = 0; i < n; ++i) {
        const v2w_adamw_ema_item& it = items[i];
        if (!ptr4(it.p) || !ptr4(it.g) || !ptr4(it.m) || !ptr4(it.v) || !ptr4(it.e) || it.numel <= 0) return V2W_E_ARG;
        if (it.numel > (kMaxUnits << 2)) return V2W_E_SHAPE;
        units[i] = item_units(it);
        if (units[i] > kMaxUnits) return V2W_E_SHAPE;
        if (overlap(it.p, it.m, it.numel) || overlap(it.p, it.v, it.numel) || overlap(it.m, it.v, it.numel)) return V2W_E_ARG;
        if (overlap(it.e, it.p, it.numel) || overlap(it.e, it.m, it.numel) || overlap(it.e, it.v, it.numel)) return V2W_E_ARG;
    }
    return 0;
}

// v2w_ema_item / v2w_swap_item
template <class Item>
int pair_items(const Item* items, int n, long long* units) {
    if (!items || n < 1 || n > V2W_ADAMW_MAX_ITEMS) return V2W_E_ARG;
    for (int i = 0; i < n; ++i) {
        const Item& it = items[i];
        if (!ptr4(it.p) || !ptr4(it.e) || it.numel <= 0) return V2W_E_ARG;
        if (it.numel > (kMaxUnits << 2)) return V2W_E_SHAPE;
        units[i] = item_units(it);
        if (units[i] > kMaxUnits) return V2W_E_SHAPE;
        if (overlap(it.p, it.e, it.numel)) return V2W_E_ARG;
    }
    return 0;
}

// ema_omd = 1 - decay in [0, 1]; a NaN is refused
inline bool omd_ok(float omd) { return omd >= 0.f && omd <= 1.f; }

// starts[i] = first workgroup of tensor i, starts[n] = workgroups of the launch (returned)
int adamw_plan(const long long* units, int n, int32_t* starts) {
    long long total = 0;
    for (int i = 0; i < n; ++i) total += units[i];
    long long chunk = (total + V2W_ADAMW_TARGET_WGS - 1) / V2W_ADAMW_TARGET_WGS;
    if (chunk < kMinChunk) chunk = kMinChunk;
    int w = 0;
    for (int i = 0; i < n; ++i) {
        starts[i] = w;
        const long long k = (units[i] + chunk - 1) / chunk;
        w += k < 1 ? 1 : (int)k;
    }
    starts[n] = w;
    return w;
}

// the comparisons are written so that a NaN is refused
int adamw_coef(const v2w_adamw_hyper* h, Coef* c) {
    if (!h) return V2W_E_ARG;
    if (!(h->beta1 >= 0.f && h->beta1 < 1.f) || !(h->beta2 >= 0.f && h->beta2 < 1.f)) return V2W_E_ARG;
    if (!(h->eps >= 0.f) || !(h->lr >= 0.f) || !(h->bias_corr1 > 0.f) || !(h->bias_corr2_sqrt > 0.f)) return V2W_E_ARG;
    c->decay = (float)(1.0 - (double)h->lr * (double)h->weight_decay);
    c->omb1 = (float)(1.0 - (double)h->beta1);
    c->beta2 = h->beta2;
    c->omb2 = (float)(1.0 - (double)h->beta2);
    c->rbc2 = (float)(1.0 / (double)h->bias_corr2_sqrt);
    c->eps = h->eps;
    c->step = (float)((double)h->lr / (double)h->bias_corr1);
    return 0;
}

// the table of the launches that touch g only: every item with p = m = v = g (the plan then counts g's own phase and every span takes
// 16-byte accesses); only g and numel of the caller's items are looked at
int grad_args(const v2w_adamw_item* items, int n, AdamWArgs* A) {
    if (!items || n < 1 || n > V2W_ADAMW_MAX_ITEMS) return V2W_E_ARG;
    long long units[V2W_ADAMW_MAX_ITEMS];
    for (int i = 0; i < n; ++i) {
        if (!ptr4(items[i].g) || items[i].numel <= 0) return V2W_E_ARG;
        if (items[i].numel > (kMaxUnits << 2)) return V2W_E_SHAPE;
        float* g = const_cast<float*>(items[i].g);
        A->it[i] = v2w_adamw_item{g, g, g, g, items[i].numel};
        units[i] = item_units(A->it[i]);
        if (units[i] > kMaxUnits) return V2W_E_SHAPE;
    }
    adamw_plan(units, n, A->starts);
    A->c = Coef{};
    A->n = n;
    return 0;
}

}  // namespace

extern "C" int v2w_adamw_multi_plan(const v2w_adamw_item* items, int n, int32_t* starts) {
    if (!starts) return V2W_E_ARG;
    long long units[V2W_ADAMW_MAX_ITEMS];
    if (const int rc = adamw_items(items, n, units)) return rc;
    return adamw_plan(units, n, starts);
}

extern "C" int v2w_adamw_multi(const v2w_adamw_item* items, int n, const v2w_adamw_hyper* h, void* stream) {
    AdamWArgs A;
    long long units[V2W_ADAMW_MAX_ITEMS];
    if (const int rc = adamw_items(items, n, units)) return rc;
    if (const int rc = adamw_coef(h, &A.c)) return rc;
    for (int i = 0; i < n; ++i) A.it[i] = items[i];
    adamw_plan(units, n, A.starts);
    A.n = n;
    hipStream_t st = (hipStream_t)stream;
    if (v2w_dry(st)) return 0;
    V2W_LAUNCH(adamw_multi_kernel, dim3(A.starts[n]), dim3(kThreads), 0, st, A);
    return v2w_launch_status();
}

extern "C" int v2w_adamw_multi_clipped(const v2w_adamw_item* items, int n, const v2w_adamw_hyper* h, const float* clip, int skip_nonfinite,
                                       void* stream) {
    AdamWArgs A;
    long long units[V2W_ADAMW_MAX_ITEMS];
    if (const int rc = adamw_items(items, n, units)) return rc;
    if (const int rc = adamw_coef(h, &A.c)) return rc;
    if (!ptr4(clip)) return V2W_E_ARG;
    for (int i = 0; i < n; ++i) A.it[i] = items[i];
    adamw_plan(units, n, A.starts);
    A.n = n;
    hipStream_t st = (hipStream_t)stream;
    if (v2w_dry(st)) return 0;
    V2W_LAUNCH(adamw_multi_clipped_kernel, dim3(A.starts[n]), dim3(kThreads), 0, st, A, clip, skip_nonfinite);
    return v2w_launch_status();
}

extern "C" int v2w_grad_sumsq_partials(const v2w_adamw_item* items, int n) {
    AdamWArgs A;
    if (const int rc = grad_args(items, n, &A)) return rc;
    return A.starts[n];
}

extern "C" int v2w_grad_sumsq_multi(const v2w_adamw_item* items, int n, float* partials, void* stream) {
    AdamWArgs A;
    if (const int rc = grad_args(items, n, &A)) return rc;
    if (!ptr4(partials)) return V2W_E_ARG;
    hipStream_t st = (hipStream_t)stream;
    if (v2w_dry(st)) return 0;
    V2W_LAUNCH(grad_sumsq_kernel, dim3(A.starts[n]), dim3(kThreads), 0, st, A, partials);
    return v2w_launch_status();
}

extern "C" int v2w_grad_norm_finish(const float* partials, int n_partials, float max_norm, float* out, void* stream) {
    if (!ptr4(partials) || !ptr4(out) || n_partials < 1 || !(max_norm >= 0.f)) return V2W_E_ARG;
    hipStream_t st = (hipStream_t)stream;
    if (v2w_dry(st)) return 0;
    V2W_LAUNCH(grad_norm_finish_kernel, dim3(1), dim3(kThreads), 0, st, partials, n_partials, max_norm, out);
    return v2w_launch_status();
}

extern "C" int v2w_scale_multi(const v2w_adamw_item* items, int n, const float* coef, void* stream) {
    AdamWArgs A;
    if (const int rc = grad_args(items, n, &A)) return rc;
    if (!ptr4(coef)) return V2W_E_ARG;
    hipStream_t st = (hipStream_t)stream;
    if (v2w_dry(st)) return 0;
    V2W_LAUNCH(grad_scale_kernel, dim3(A.starts[n]), dim3(kThreads), 0, st, A, coef);
    return v2w_launch_status();
}

extern "C" int v2w_adamw_ema_multi_plan(const v2w_adamw_ema_item* items, int n, int32_t* starts) {
    if (!starts) return V2W_E_ARG;
    long long units[V2W_ADAMW_EMA_MAX_ITEMS];
    if (const int rc = adamw_ema_items(items, n, units)) return rc;
    return adamw_plan(units, n, starts);
}

extern "C" int v2w_adamw_ema_multi(const v2w_adamw_ema_item* items, int n, const v2w_adamw_hyper* h, const float* clip, int skip_nonfinite,
                                   float ema_omd, void* stream) {
    AdamWEmaArgs A;
    long long units[V2W_ADAMW_EMA_MAX_ITEMS];
    if (const int rc = adamw_ema_items(items, n, units)) return rc;
    if (const int rc = adamw_coef(h, &A.c)) return rc;
    if (!omd_ok(ema_omd) || (clip && !ptr4(clip))) return V2W_E_ARG;
    for (int i = 0; i < n; ++i) A.it[i] = items[i];
    adamw_plan(units, n, A.starts);
    A.omd = ema_omd;
    A.n = n;
    hipStream_t st = (hipStream_t)stream;
    if (v2w_dry(st)) return 0;
    if (clip) V2W_LAUNCH(adamw_ema_multi_clipped_kernel, dim3(A.starts[n]), dim3(kThreads), 0, st, A, clip, skip_nonfinite);
    else V2W_LAUNCH(adamw_ema_multi_kernel, dim3(A.starts[n]), dim3(kThreads), 0, st, A);
    return v2w_launch_status();
}

extern "C" int v2w_ema_multi_plan(const v2w_ema_item* items, int n, int32_t* starts) {
    if (!starts) return V2W_E_ARG;
    long long units[V2W_ADAMW_MAX_ITEMS];
    if (const int rc = pair_items(items, n, units)) return rc;
    return adamw_plan(units, n, starts);
}

extern "C" int v2w_ema_multi(const v2w_ema_item* items, int n, float ema_omd, void* stream) {
    PairArgs<v2w_ema_item> A;
    long long units[V2W_ADAMW_MAX_ITEMS];
    if (const int rc = pair_items(items, n, units)) return rc;
    if (!omd_ok(ema_omd)) return V2W_E_ARG;
    for (int i = 0; i < n; ++i) A.it[i] = items[i];
    adamw_plan(units, n, A.starts);
    A.n = n;
    hipStream_t st = (hipStream_t)stream;
    if (v2w_dry(st)) return 0;
    V2W_LAUNCH(ema_multi_kernel, dim3(A.starts[n]), dim3(kThreads), 0, st, A, ema_omd);
    return v2w_launch_status();
}

extern "C" int v2w_swap_multi(const v2w_swap_item* items, int n, void* stream) {
    PairArgs<v2w_swap_item> A;
    long long units[V2W_ADAMW_MAX_ITEMS];
    if (const int rc = pair_items(items, n, units)) return rc;
    for (int i = 0; i < n; ++i) A.it[i] = items[i];
    adamw_plan(units, n, A.starts);
    A.n = n;
    hipStream_t st = (hipStream_t)stream;
    if (v2w_dry(st)) return 0;
    V2W_LAUNCH(swap_multi_kernel, dim3(A.starts[n]), dim3(kThreads), 0, st, A);
    return v2w_launch_status();
}
