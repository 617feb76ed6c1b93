// The multi-tensor streaming launches (optimizer: v2w_optim.hip, L1 losses: v2w_loss.hip) and the code they share.  A new multi-tensor kernel
// starts from here.
//
// A launch carries up to a few dozen tensors ("items") in a table that travels by value in the kernel arguments: it[] (the descriptors),
// starts[] and n.  A tensor is cut into UNITS of four floats; workgroups of kThreads are dealt in proportion to the units, at least one per
// tensor (host, deal_workgroups): starts[i] is the first workgroup of tensor i.  A workgroup finds its tensor from blockIdx.x by a search
// every lane makes alike (find_item) and takes an equal share of its units (chunk_of).  The plan depends on the descriptors only.
//
// Flat tensors (Span, find_span, unit_mask): when all pointers of an item share their 16-byte phase (s floats past a 16-byte line) the
// units are cut at the 16-byte lines - the first and the last one partial - and every whole unit is one 16-byte access per lane and tensor;
// otherwise the units start at element 0 and the item takes float-by-float accesses, chosen by a branch that is uniform over the
// workgroup.  A file says which pointers an item type has by specialising ItemPtrs.  (The pitched rows of the L1 pairs keep their own
// arithmetic in v2w_loss.hip: they share the search, the chunk and the unit access.)
#pragma once
#include "v2w_common.h"

namespace {

constexpr int kThreads = 256;
constexpr long long kMinChunk = kThreads * 8;    // units: no workgroup for less than 32 KB of reads per tensor unless the tensor is smaller
constexpr long long kMaxUnits = 1ll << 40;

__host__ __device__ inline int phase16(const void* p) { return (int)((reinterpret_cast<uintptr_t>(p) >> 2) & 3); }   // floats past a 16-byte line
__host__ __device__ inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
inline bool ptr4(const void* p) { return p && (reinterpret_cast<uintptr_t>(p) & 3) == 0; }

// elements [e0, e1) of the four floats at q (the others read as 0 and are never touched); one 16-byte access when all four are wanted
// and `vec` says that q is on a 16-byte line
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

// host: starts[i] = first workgroup of tensor i, starts[n] = workgroups of the launch (returned), about target_wgs of them
inline int deal_workgroups(const long long* units, int n, int target_wgs, int32_t* starts) {
    long long total = 0;
    for (int i = 0; i < n; ++i) total += units[i];
    long long chunk = (total + target_wgs - 1) / target_wgs;
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

// the tensor of workgroup wg: starts[i] <= wg < starts[i + 1]
__device__ __forceinline__ int find_item(const int* starts, int n, int wg) {
    int lo = 0, hi = n;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (starts[mid] <= wg) lo = mid; else hi = mid;
    }
    return lo;
}
// the share of workgroup wg of tensor i's units: [u0, u0 + cnt)
__device__ __forceinline__ void chunk_of(const int* starts, int i, int wg, long long units, long long& u0, unsigned& cnt) {
    const int nwg = starts[i + 1] - starts[i];
    const long long chunk = (units + nwg - 1) / nwg;
    u0 = (long long)(wg - starts[i]) * chunk;
    const long long u1 = u0 + chunk < units ? u0 + chunk : units;
    cnt = u1 > u0 ? (unsigned)(u1 - u0) : 0u;
}

// What a file says of each item type of its flat tables: N pointers, listed by get() with the WRITTEN ones first - those W must not overlap
// one another, the others are only read - and q[0] the one whose phase places the units; at most MAX items per launch.
template <class Item> struct ItemPtrs;

template <class Item>
__host__ __device__ inline bool same_phase(const Item& it) {
    const void* q[ItemPtrs<Item>::N];
    ItemPtrs<Item>::get(it, q);
    bool same = true;
    for (int k = 1; k < ItemPtrs<Item>::N; ++k) same = same && phase16(q[k]) == phase16(q[0]);
    return same;
}
template <class Item>
__host__ __device__ inline int item_shift(const Item& it) {
    const void* q[ItemPtrs<Item>::N];
    ItemPtrs<Item>::get(it, q);
    return same_phase(it) ? phase16(q[0]) : 0;
}
template <class Item>
__host__ __device__ inline long long item_units(const Item& it) { return (it.numel + item_shift(it) + 3) >> 2; }

// the chunk of workgroup wg: its tensor, and units [u0, u0 + cnt) of it
struct Span {
    int item;
    long long numel, base;      // base: element index of the first float of unit u0 (negative inside a partial first unit)
    unsigned cnt;
    bool vec;
};
template <class Args>
__device__ __forceinline__ Span find_span(const Args& A, int wg) {
    Span s;
    s.item = find_item(A.starts, A.n, wg);
    const auto& it = A.it[s.item];
    s.numel = it.numel;
    s.vec = same_phase(it);
    const int shift = item_shift(it);
    long long u0;
    chunk_of(A.starts, s.item, wg, (s.numel + shift + 3) >> 2, u0, s.cnt);
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

}  // namespace
