// AdamW (torch.optim.AdamW as the reference calls it, train.py:96-99,198,215: decoupled weight decay, no amsgrad, no maximize): the step of
// up to V2W_ADAMW_MAX_ITEMS parameter tensors in ONE streaming launch, and the launches that ride on the same mechanism.  The arithmetic,
// its order and its fp32 roundings are stated in include/vec2wav_hip.h; the units of four floats, the plan, the search for a workgroup's
// tensor and its Span are in v2w_multi.h.  What this file adds to them:
//   - ItemPtrs of its item types: which pointers an item has and which must not overlap;
//   - the kernels: the step (adamw_body: p, g, m, v [, e], 28 or 36 bytes per parameter; compiled with and without the clip coefficient
//     and the average), the average alone, the exchange of p and e, the sum of squares of g (one fp32 partial per workgroup, fixed
//     order), g *= coef.  Each writes out the same loop - the masks and all loads of kUnroll units, then the arithmetic and the stores -
//     ON PURPOSE: behind one loop template taking the arithmetic as a functor the compiler laid the masked paths out of line, and the
//     step measured 2 % slower on the generator's list (same bits); the small kernels follow the step.  Every element of a written
//     tensor is written exactly once, nothing else is written; no atomics, no scratch;
//   - check_items and fill_table, the host side of every entry point: check, extras, fill, dry-run return, V2W_LAUNCH, status.
// Global-norm clipping never visits the host: grad_norm_finish_kernel adds the partials in fp64 and leaves norm, clip coefficient, finite
// flag and a running count in four floats of the caller's, which the clipped step reads.
#include "v2w_multi.h"

namespace {

constexpr int kUnroll = 2;                       // units in flight per thread: 2 x 4 tensors x 16 B of loads before the first use

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

// the launches that touch g only read g and numel of the caller's v2w_adamw_item: one pointer, so every span takes the 16-byte path
struct GradItem {
    float* g;
    long long numel;
    GradItem() = default;
    GradItem(const v2w_adamw_item& it) : g(const_cast<float*>(it.g)), numel(it.numel) {}
};

// a table without constants: Item is v2w_ema_item (p only read), v2w_swap_item (both written) or GradItem
template <class Item>
struct ItemArgs {
    Item it[V2W_ADAMW_MAX_ITEMS];
    int starts[V2W_ADAMW_MAX_ITEMS + 1];
    int n;
};
static_assert(sizeof(ItemArgs<v2w_ema_item>) <= 3584 && sizeof(ItemArgs<v2w_swap_item>) == sizeof(ItemArgs<v2w_ema_item>), "by-value table");

template <int N_, int W_, int MAX_>
struct PtrList { static constexpr int N = N_, W = W_, MAX = MAX_; };
template <> struct ItemPtrs<v2w_adamw_item> : PtrList<4, 3, V2W_ADAMW_MAX_ITEMS> {
    __host__ __device__ static void get(const v2w_adamw_item& it, const void** q) { q[0] = it.p; q[1] = it.m; q[2] = it.v; q[3] = it.g; }
};
template <> struct ItemPtrs<v2w_adamw_ema_item> : PtrList<5, 4, V2W_ADAMW_EMA_MAX_ITEMS> {
    __host__ __device__ static void get(const v2w_adamw_ema_item& it, const void** q) { q[0] = it.p; q[1] = it.m; q[2] = it.v; q[3] = it.e; q[4] = it.g; }
};
template <> struct ItemPtrs<v2w_ema_item> : PtrList<2, 2, V2W_ADAMW_MAX_ITEMS> {      // (p is only read, and still kept off e)
    __host__ __device__ static void get(const v2w_ema_item& it, const void** q) { q[0] = it.p; q[1] = it.e; }
};
template <> struct ItemPtrs<v2w_swap_item> : PtrList<2, 2, V2W_ADAMW_MAX_ITEMS> {
    __host__ __device__ static void get(const v2w_swap_item& it, const void** q) { q[0] = it.p; q[1] = it.e; }
};
template <> struct ItemPtrs<GradItem> : PtrList<1, 0, V2W_ADAMW_MAX_ITEMS> {
    __host__ __device__ static void get(const GradItem& it, const void** q) { q[0] = it.g; }
};

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
ema_multi_kernel(const ItemArgs<v2w_ema_item> A, float omd) {
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
swap_multi_kernel(const ItemArgs<v2w_swap_item> A) {
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

// partials[wg] = sum of g^2 over the workgroup's chunk: per thread one fma chain over its units in order, then the fixed block sum
__global__ void __launch_bounds__(kThreads)
grad_sumsq_kernel(const ItemArgs<GradItem> A, float* __restrict__ partials) {
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
grad_scale_kernel(const ItemArgs<GradItem> A, const float* __restrict__ coef) {
    const Span s = find_span(A, blockIdx.x);
    float* g = A.it[s.item].g + s.base;
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

inline bool overlap(const void* a, const void* b, long long numel) {
    const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b), bytes = (uintptr_t)numel * 4;
    return x < y ? y - x < bytes : x - y < bytes;
}

// checks every descriptor - read as the table's Item - and counts its units: all pointers of ItemPtrs<Item> 4-byte aligned and not NULL,
// the written ones apart from one another
template <class Item, class Src>
int check_items(const Src* items, int n, long long* units) {
    typedef ItemPtrs<Item> P;
    if (!items || n < 1 || n > P::MAX) return V2W_E_ARG;
    for (int i = 0; i < n; ++i) {
        const Item it(items[i]);
        const void* q[P::N];
        P::get(it, q);
        bool ok = it.numel > 0;
        for (int k = 0; k < P::N; ++k) ok = ok && ptr4(q[k]);
        if (!ok) return V2W_E_ARG;
        if (it.numel > (kMaxUnits << 2)) return V2W_E_SHAPE;
        units[i] = item_units(it);
        if (units[i] > kMaxUnits) return V2W_E_SHAPE;
        for (int k = 1; k < P::W; ++k)
            for (int l = 0; l < k; ++l)
                if (overlap(q[k], q[l], it.numel)) return V2W_E_ARG;
    }
    return 0;
}

// it[], starts[] and n of a by-value table from checked items; returns the workgroups of the launch
template <class Args, class Src>
int fill_table(Args& A, const Src* items, int n, const long long* units) {
    for (int i = 0; i < n; ++i) A.it[i] = items[i];
    A.n = n;
    return deal_workgroups(units, n, V2W_ADAMW_TARGET_WGS, A.starts);
}

// ema_omd = 1 - decay in [0, 1]; a NaN is refused
inline bool omd_ok(float omd) { return omd >= 0.f && omd <= 1.f; }

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

// the host-only plan queries: the items' checks, then the deal
template <class Item>
int plan_of(const Item* items, int n, int32_t* starts) {
    if (!starts) return V2W_E_ARG;
    long long units[ItemPtrs<Item>::MAX];
    if (const int rc = check_items<Item>(items, n, units)) return rc;
    return deal_workgroups(units, n, V2W_ADAMW_TARGET_WGS, starts);
}

}  // namespace

extern "C" int v2w_adamw_multi_plan(const v2w_adamw_item* items, int n, int32_t* starts) { return plan_of(items, n, starts); }
extern "C" int v2w_adamw_ema_multi_plan(const v2w_adamw_ema_item* items, int n, int32_t* starts) { return plan_of(items, n, starts); }
extern "C" int v2w_ema_multi_plan(const v2w_ema_item* items, int n, int32_t* starts) { return plan_of(items, n, starts); }

extern "C" int v2w_adamw_multi(const v2w_adamw_item* items, int n, const v2w_adamw_hyper* h, void* stream) {
    AdamWArgs A;
    long long units[V2W_ADAMW_MAX_ITEMS];
    if (const int rc = check_items<v2w_adamw_item>(items, n, units)) return rc;
    if (const int rc = adamw_coef(h, &A.c)) return rc;
    const int wgs = fill_table(A, items, n, units);
    hipStream_t st = (hipStream_t)stream;
    if (v2w_dry(st)) return 0;
    V2W_LAUNCH(adamw_multi_kernel, dim3(wgs), dim3(kThreads), 0, st, A);
    return v2w_launch_status();
}

extern "C" int v2w_adamw_multi_clipped(const v2w_adamw_item* items, int n, const v2w_adamw_hyper* h, const float* clip, int skip_nonfinite,
                                       void* stream) {
    AdamWArgs A;
    long long units[V2W_ADAMW_MAX_ITEMS];
    if (const int rc = check_items<v2w_adamw_item>(items, n, units)) return rc;
    if (const int rc = adamw_coef(h, &A.c)) return rc;
    if (!ptr4(clip)) return V2W_E_ARG;
    const int wgs = fill_table(A, items, n, units);
    hipStream_t st = (hipStream_t)stream;
    if (v2w_dry(st)) return 0;
    V2W_LAUNCH(adamw_multi_clipped_kernel, dim3(wgs), dim3(kThreads), 0, st, A, clip, skip_nonfinite);
    return v2w_launch_status();
}

extern "C" int v2w_grad_sumsq_partials(const v2w_adamw_item* items, int n) {
    ItemArgs<GradItem> A;
    long long units[V2W_ADAMW_MAX_ITEMS];
    if (const int rc = check_items<GradItem>(items, n, units)) return rc;
    return fill_table(A, items, n, units);
}

extern "C" int v2w_grad_sumsq_multi(const v2w_adamw_item* items, int n, float* partials, void* stream) {
    ItemArgs<GradItem> A;
    long long units[V2W_ADAMW_MAX_ITEMS];
    if (const int rc = check_items<GradItem>(items, n, units)) return rc;
    if (!ptr4(partials)) return V2W_E_ARG;
    const int wgs = fill_table(A, items, n, units);
    hipStream_t st = (hipStream_t)stream;
    if (v2w_dry(st)) return 0;
    V2W_LAUNCH(grad_sumsq_kernel, dim3(wgs), dim3(kThreads), 0, st, A, partials);
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
    ItemArgs<GradItem> A;
    long long units[V2W_ADAMW_MAX_ITEMS];
    if (const int rc = check_items<GradItem>(items, n, units)) return rc;
    if (!ptr4(coef)) return V2W_E_ARG;
    const int wgs = fill_table(A, items, n, units);
    hipStream_t st = (hipStream_t)stream;
    if (v2w_dry(st)) return 0;
    V2W_LAUNCH(grad_scale_kernel, dim3(wgs), dim3(kThreads), 0, st, A, coef);
    return v2w_launch_status();
}

extern "C" int v2w_adamw_ema_multi(const v2w_adamw_ema_item* items, int n, const v2w_adamw_hyper* h, const float* clip, int skip_nonfinite,
                                   float ema_omd, void* stream) {
    AdamWEmaArgs A;
    long long units[V2W_ADAMW_EMA_MAX_ITEMS];
    if (const int rc = check_items<v2w_adamw_ema_item>(items, n, units)) return rc;
    if (const int rc = adamw_coef(h, &A.c)) return rc;
    if (!omd_ok(ema_omd) || (clip && !ptr4(clip))) return V2W_E_ARG;
    const int wgs = fill_table(A, items, n, units);
    A.omd = ema_omd;
    hipStream_t st = (hipStream_t)stream;
    if (v2w_dry(st)) return 0;
    if (clip) V2W_LAUNCH(adamw_ema_multi_clipped_kernel, dim3(wgs), dim3(kThreads), 0, st, A, clip, skip_nonfinite);
    else V2W_LAUNCH(adamw_ema_multi_kernel, dim3(wgs), dim3(kThreads), 0, st, A);
    return v2w_launch_status();
}

extern "C" int v2w_ema_multi(const v2w_ema_item* items, int n, float ema_omd, void* stream) {
    ItemArgs<v2w_ema_item> A;
    long long units[V2W_ADAMW_MAX_ITEMS];
    if (const int rc = check_items<v2w_ema_item>(items, n, units)) return rc;
    if (!omd_ok(ema_omd)) return V2W_E_ARG;
    const int wgs = fill_table(A, items, n, units);
    hipStream_t st = (hipStream_t)stream;
    if (v2w_dry(st)) return 0;
    V2W_LAUNCH(ema_multi_kernel, dim3(wgs), dim3(kThreads), 0, st, A, ema_omd);
    return v2w_launch_status();
}

extern "C" int v2w_swap_multi(const v2w_swap_item* items, int n, void* stream) {
    ItemArgs<v2w_swap_item> A;
    long long units[V2W_ADAMW_MAX_ITEMS];
    if (const int rc = check_items<v2w_swap_item>(items, n, units)) return rc;
    const int wgs = fill_table(A, items, n, units);
    hipStream_t st = (hipStream_t)stream;
    if (v2w_dry(st)) return 0;
    V2W_LAUNCH(swap_multi_kernel, dim3(wgs), dim3(kThreads), 0, st, A);
    return v2w_launch_status();
}
