// GAN training losses (reference models.py:278-310 feature_loss / discriminator_loss / generator_loss, train.py:204 the mel L1 term):
// every map pair of a feature loss in ONE streaming launch (+ one finishing launch), every LSGAN term of a call in one launch, and
// their backwards in one launch each.  The maps are read where the discriminators left them: `rows` rows of `valid` floats `pitch`
// floats apart ([valid, pitch) is never read), so the [:, :, :U] views of the pitched feature-map buffers need no copy.
//
// The multi-tensor L1 launches are built from v2w_multi.h: its units of four floats, its plan (about V2W_L1_TARGET_WGS workgroups, at least
// one per pair), its search for a workgroup's pair and its unit access.  Their own here is the row arithmetic: a pair has per row
// ceil(valid / 4) units, the last one of a row partial; a pair whose two sides are dense is one row of rows * valid floats whose units are
// cut at the 16-byte boundaries of `a`.  The plan depends on the descriptors only (not on the device), every workgroup writes ONE fp64
// partial and the finishing launch adds them in index order: the same call gives the same bits.
// The masked L1, the LSGAN kernels and both finishing kernels do not share that skeleton: of v2w_multi.h they use the constants only.
// The *_len kernels are the same terms over a padded batch of items of unequal lengths: the dense kernels' descriptors, units, plan and order
// of sums with a per-float mask from a device table of extents; v2w_map_extents writes that table, v2w_mask_tail zeroes a batch's padding.
#include "v2w_multi.h"

namespace {

constexpr int kUnroll = 4;                       // units in flight per thread: 2 x 4 x 16 B of loads before the first use

struct L1Item {
    const float* a; const float* b; float* da; float* db;
    long long shape;               // pa == 0 (one dense run): its floats; else rows << 32 | floats per row
    int pa, pb;                    // row pitches in floats
    __host__ __device__ bool flat() const { return pa == 0; }
    __host__ __device__ int rows() const { return flat() ? 1 : (int)(shape >> 32); }
    __host__ __device__ long long len() const { return flat() ? shape : (shape & 0xffffffffll); }      // floats per row
};
struct L1Args {
    L1Item it[V2W_LOSS_MAX_ITEMS];
    int starts[V2W_LOSS_MAX_ITEMS + 1];
    int n;
    float scale;
    const float* gout;
};
static_assert(sizeof(L1Args) <= 3584, "kernel arguments travel by value: 4 KB with the hidden ones");

struct LsItem { const float* s; float* ds; unsigned numel, valid, pitch; float target; };
struct LsArgs {
    LsItem it[V2W_LOSS_MAX_ITEMS];
    int n;
    const float* gout; const float* gterm;
};

// BWD = false: part[workgroup] = sum |a - b| over the workgroup's units (fp64).
// BWD = true:  da = sgn(a - b) * (scale * gout / numel), db = -da, dense (rows x len); sgn = (a > b) - (a < b).
template <bool BWD>
__global__ void __launch_bounds__(kThreads)
l1_multi_kernel(const L1Args A, double* __restrict__ part) {
    __shared__ double red[16];
    const int wg = blockIdx.x;
    const int lo = find_item(A.starts, A.n, wg);
    const L1Item& it = A.it[lo];
    const float* a = it.a;
    const float* b = it.b;
    const long long len = it.len();
    const bool flat = it.flat();
    const int rows = it.rows();
    const int shift = flat ? phase16(a) : 0;              // units of a flat pair start at a's 16-byte lines
    const long long upr = (len + shift + 3) >> 2;         // units per row
    long long u0;
    unsigned cnt;
    chunk_of(A.starts, lo, wg, upr * rows, u0, cnt);
    const long long r0 = flat ? 0 : u0 / upr;
    const long long q0 = u0 - r0 * upr;
    const unsigned upr32 = flat ? 1u : (unsigned)upr, q032 = flat ? 0u : (unsigned)q0;
    a += r0 * it.pa - shift;                              // the first unit of row r0 (it may begin before the row: those floats are masked)
    b += r0 * it.pb - shift;

    float coef = 0.f;
    float* da = nullptr;
    float* db = nullptr;
    if (BWD) {
        const float numel = (float)(len * rows);
        // (scale * gout) / numel, correctly rounded: the fp64 quotient of two floats rounds to the fp32 quotient
        coef = (float)((double)(A.scale * A.gout[0]) / (double)numel);
        da = it.da ? it.da + r0 * len - shift : nullptr;
        db = it.db ? it.db + r0 * len - shift : nullptr;
    }

    double acc = 0.0;
    for (unsigned t0 = threadIdx.x; t0 < cnt; t0 += kThreads * kUnroll) {
        f32x4 va[kUnroll], vb[kUnroll];
        long long oo[kUnroll];
        int e0[kUnroll], e1[kUnroll];
#pragma unroll
        for (int k = 0; k < kUnroll; ++k) {
            const unsigned t = t0 + k * kThreads;
            long long p;             // position in its row of the unit's first float (negative: the floats before a flat pair's start)
            size_t oa, ob;
            if (flat) {
                p = ((q0 + t) << 2) - shift;
                oa = ob = ((size_t)q0 + t) << 2;
                oo[k] = (long long)oa;
            } else {
                const unsigned tt = q032 + t, r = tt / upr32, q = tt - r * upr32;
                p = (long long)q << 2;
                oa = (size_t)r * it.pa + (q << 2);
                ob = (size_t)r * it.pb + (q << 2);
                oo[k] = (long long)r * len + (q << 2);
            }
            e0[k] = p < 0 ? (int)-p : 0;
            e1[k] = len - p < 4 ? (int)(len - p) : 4;
            if (t >= cnt) e0[k] = e1[k] = 0;
            va[k] = load_unit(a + oa, e0[k], e1[k], aligned16(a + oa));
            vb[k] = load_unit(b + ob, e0[k], e1[k], aligned16(b + ob));
        }
#pragma unroll
        for (int k = 0; k < kUnroll; ++k) {
            if (!BWD) {
#pragma unroll
                for (int j = 0; j < 4; ++j) acc += (double)fabsf(va[k][j] - vb[k][j]);     // masked floats are 0 on both sides
            } else {
                f32x4 d, nd;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    d[j] = va[k][j] > vb[k][j] ? coef : (va[k][j] < vb[k][j] ? -coef : 0.f);
                    nd[j] = -d[j];
                }
                if (da) store_unit(da + oo[k], d, e0[k], e1[k], aligned16(da + oo[k]));
                if (db) store_unit(db + oo[k], nd, e0[k], e1[k], aligned16(db + oo[k]));
            }
        }
    }
    if (!BWD) {
        const double s = v2w_block_sum(acc, red);
        if (threadIdx.x == 0) part[wg] = s;
    }
}

// term[i] = (sum of pair i's partials, in workgroup order) / numel_i;  total = scale * sum_i term[i], in list order; all in fp64
__global__ void __launch_bounds__(kThreads)
l1_finish_kernel(const L1Args A, const double* __restrict__ part, float* __restrict__ term, float* __restrict__ total) {
    __shared__ double red[16];
    double tot = 0.0;
    for (int i = 0; i < A.n; ++i) {
        double s = 0.0;
        for (int k = A.starts[i] + threadIdx.x; k < A.starts[i + 1]; k += kThreads) s += part[k];
        const double mean = v2w_block_sum(s, red) / (double)(A.it[i].len() * A.it[i].rows());
        if (threadIdx.x == 0 && term) term[i] = (float)mean;
        tot += mean;
    }
    if (threadIdx.x == 0 && total) total[0] = (float)((double)A.scale * tot);
}

// term[i] = mean (t_i - s_i)^2, total = sum_i term[i] (list order); one workgroup: the scores of a call are a few thousand floats
__global__ void __launch_bounds__(1024)
lsgan_multi_kernel(const LsArgs A, float* __restrict__ term, float* __restrict__ total) {
    __shared__ double red[16];
    double tot = 0.0;
    for (int i = 0; i < A.n; ++i) {
        const LsItem& it = A.it[i];
        const double t = (double)it.target;
        double acc = 0.0;
        for (unsigned e = threadIdx.x; e < it.numel; e += 1024) {
            const unsigned r = e / it.valid, j = e - r * it.valid;
            const double d = t - (double)it.s[(size_t)r * it.pitch + j];
            acc += d * d;
        }
        const double mean = v2w_block_sum(acc, red) / (double)it.numel;
        if (threadIdx.x == 0 && term) term[i] = (float)mean;
        tot += mean;
    }
    if (threadIdx.x == 0 && total) total[0] = (float)tot;
}

// ds_i = 2 (s_i - t_i) * g_i / numel_i, dense; g_i = gout[0] + gterm[i] (either may be absent); grid (blocks, items)
__global__ void __launch_bounds__(kThreads)
lsgan_multi_bwd_kernel(const LsArgs A) {
    const int i = blockIdx.y;
    const LsItem& it = A.it[i];
    if (!it.ds) return;
    const float g = (A.gout ? A.gout[0] : 0.f) + (A.gterm ? A.gterm[i] : 0.f);
    const float c = g / (float)it.numel;
    for (unsigned e = blockIdx.x * kThreads + threadIdx.x; e < it.numel; e += gridDim.x * kThreads) {
        const unsigned r = e / it.valid, j = e - r * it.valid;
        it.ds[e] = 2.f * (it.s[(size_t)r * it.pitch + j] - it.target) * c;
    }
}

// ---- the multi-tensor terms over a padded batch (v2w_*_multi_len): B items, ext[i * B + b] = the floats at the head of each row of item b
// of descriptor i that count.  Same descriptors, same units, same plan and same order of every sum as the dense kernels above (full
// extents give their bits); a float that does not count is selected away, a unit without a counted float is not loaded.  A flat item
// (one dense run) keeps its row length in `pb`, which the dense kernel never reads for it.
struct L1LenArgs { L1Args A; const int32_t* ext; int B; };
static_assert(sizeof(L1LenArgs) <= 3584, "kernel arguments travel by value: 4 KB with the hidden ones");
struct LsLenArgs { LsArgs A; const int32_t* ext; int B; };

// the counted floats of a row of `rowlen`: ext clamped to [0, rowlen]
__device__ __forceinline__ int ext_clamp(int e, int rowlen) { return e < 0 ? 0 : (e < rowlen ? e : rowlen); }

// rpi * sum_b v_b of one descriptor (ext: its B entries): an integer below 2^53, exact in fp64.  Every thread of the workgroup calls it.
__device__ __forceinline__ double len_denominator(const int32_t* __restrict__ ext, int B, int rpi, int rowlen, double* red) {
    double s = 0.0;
    for (int b = threadIdx.x; b < B; b += blockDim.x) s += (double)ext_clamp(ext[b], rowlen);
    return v2w_block_sum(s, red) * (double)rpi;
}

// BWD = false: part[workgroup] = sum |a - b| over the counted floats of the workgroup's units (fp64).
// BWD = true:  da = sgn(a - b) * (scale * gout / den) on the counted floats, +0.0 on the others; db = -da, +0.0 on the others; dense.
template <bool BWD>
__global__ void __launch_bounds__(kThreads)
l1_multi_len_kernel(const L1LenArgs L, double* __restrict__ part) {
    __shared__ double red[16];
    const L1Args& A = L.A;
    const int wg = blockIdx.x;
    const int lo = find_item(A.starts, A.n, wg);
    const L1Item& it = A.it[lo];
    const float* a = it.a;
    const float* b = it.b;
    const long long len = it.len();
    const bool flat = it.flat();
    const int rowlen = flat ? it.pb : (int)len;           // floats per row of the descriptor (a flat item is rows * rowlen floats in one run)
    const int rows = flat ? (int)(it.shape / rowlen) : it.rows();
    const unsigned rpi = (unsigned)(rows / L.B);
    const int32_t* __restrict__ ext = L.ext + (size_t)lo * L.B;
    const int shift = flat ? phase16(a) : 0;
    const long long upr = (len + shift + 3) >> 2;
    long long u0;
    unsigned cnt;
    chunk_of(A.starts, lo, wg, upr * (flat ? 1 : rows), u0, cnt);
    const long long r0 = flat ? 0 : u0 / upr;
    const long long q0 = u0 - r0 * upr;
    const unsigned upr32 = flat ? 1u : (unsigned)upr, q032 = flat ? 0u : (unsigned)q0;
    a += r0 * it.pa - shift;
    b += r0 * it.pb - shift;                              // (r0 == 0 for a flat item, whose pb is its row length)

    // where the chunk begins: descriptor row R0 (RB0 rows into item B0), float C0 of it (negative: the floats before a flat pair's start)
    long long R0 = r0, C0 = q0 << 2;
    if (flat) {
        const long long E0 = (q0 << 2) - shift;
        R0 = E0 > 0 ? E0 / rowlen : 0;
        C0 = E0 - R0 * rowlen;
    }
    const int B0 = (int)(R0 / rpi);
    const unsigned RB0 = (unsigned)(R0 - (long long)B0 * rpi);

    if (!BWD) {
        // nothing to count in the whole chunk: it lies in one row past that row's extent, or every item it touches has extent 0
        const long long last = C0 + ((long long)cnt << 2) - 1;                 // last float of the chunk, counted from row R0's start
        const long long R1 = flat ? R0 + (last > 0 ? last / rowlen : 0) : (u0 + cnt - 1) / upr;
        bool dead = cnt == 0;
        if (!dead && R1 == R0) dead = C0 >= ext_clamp(ext[B0], rowlen);
        else if (!dead) {
            const long long B1l = R1 / rpi;
            const int B1 = B1l < L.B ? (int)B1l : L.B - 1;
            dead = true;
            for (int bb = B0; bb <= B1; ++bb) dead = dead && ext_clamp(ext[bb], rowlen) == 0;
        }
        if (dead) {
            if (threadIdx.x == 0) part[wg] = 0.0;
            return;
        }
    }

    float coef = 0.f;
    float* da = nullptr;
    float* db = nullptr;
    if (BWD) {
        const double den = len_denominator(ext, L.B, (int)rpi, rowlen, red);
        // the dense kernel's coefficient with den for numel: (scale * gout) / (float)den, correctly rounded
        coef = den > 0.0 ? (float)((double)(A.scale * A.gout[0]) / (double)(float)den) : 0.f;
        da = it.da ? it.da + r0 * len - shift : nullptr;
        db = it.db ? it.db + r0 * len - shift : nullptr;
    }

    double acc = 0.0;
    for (unsigned t0 = threadIdx.x; t0 < cnt; t0 += kThreads * kUnroll) {
        f32x4 va[kUnroll], vb[kUnroll];
        long long oo[kUnroll];
        int e0[kUnroll], e1[kUnroll];
        unsigned m[kUnroll];                             // bit j: float j of the unit counts
#pragma unroll
        for (int k = 0; k < kUnroll; ++k) {
            const unsigned t = t0 + k * kThreads;
            long long p;
            size_t oa, ob;
            unsigned r = 0, q = 0;
            if (flat) {
                p = ((q0 + t) << 2) - shift;
                oa = ob = ((size_t)q0 + t) << 2;
                oo[k] = (long long)oa;
            } else {
                const unsigned tt = q032 + t;
                r = tt / upr32; q = tt - r * upr32;
                p = (long long)q << 2;
                oa = (size_t)r * it.pa + (q << 2);
                ob = (size_t)r * it.pb + (q << 2);
                oo[k] = (long long)r * len + (q << 2);
            }
            e0[k] = p < 0 ? (int)-p : 0;
            e1[k] = len - p < 4 ? (int)(len - p) : 4;
            if (t >= cnt) e0[k] = e1[k] = 0;
            m[k] = 0;
            if (e1[k] > e0[k]) {
                if (flat) {
                    // the unit's first float: x floats past row R0's start -> (row, column, item), then float by float
                    const unsigned x = (unsigned)(C0 + ((long long)t << 2) + e0[k]);
                    const unsigned dr = x / (unsigned)rowlen;
                    unsigned c = x - dr * (unsigned)rowlen;
                    unsigned rb = RB0 + dr;
                    const unsigned dbi = rb / rpi;
                    rb -= dbi * rpi;
                    int item = B0 + (int)dbi;
                    int v = ext_clamp(ext[item], rowlen);
                    for (int j = e0[k]; j < e1[k]; ++j) {
                        if ((int)c < v) m[k] |= 1u << j;
                        if (++c == (unsigned)rowlen && j + 1 < e1[k]) {
                            c = 0;
                            if (++rb == rpi) { rb = 0; ++item; }
                            v = ext_clamp(ext[item], rowlen);
                        }
                    }
                } else {
                    const int v = ext_clamp(ext[(r0 + r) / rpi], rowlen);
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (j >= e0[k] && j < e1[k] && (int)(q << 2) + j < v) m[k] |= 1u << j;
                }
            }
            const int l0 = m[k] ? e0[k] : 0, l1 = m[k] ? e1[k] : 0;          // no counted float: no load
            va[k] = load_unit(a + oa, l0, l1, aligned16(a + oa));
            vb[k] = load_unit(b + ob, l0, l1, aligned16(b + ob));
        }
#pragma unroll
        for (int k = 0; k < kUnroll; ++k) {
            if (!BWD) {
#pragma unroll
                for (int j = 0; j < 4; ++j) acc += (m[k] >> j) & 1 ? (double)fabsf(va[k][j] - vb[k][j]) : 0.0;
            } else {
                f32x4 d, nd;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const bool on = (m[k] >> j) & 1;
                    d[j] = on ? (va[k][j] > vb[k][j] ? coef : (va[k][j] < vb[k][j] ? -coef : 0.f)) : 0.f;
                    nd[j] = on ? -d[j] : 0.f;
                }
                if (da) store_unit(da + oo[k], d, e0[k], e1[k], aligned16(da + oo[k]));
                if (db) store_unit(db + oo[k], nd, e0[k], e1[k], aligned16(db + oo[k]));
            }
        }
    }
    if (!BWD) {
        const double s = v2w_block_sum(acc, red);
        if (threadIdx.x == 0) part[wg] = s;
    }
}

// l1_finish_kernel with den_i for numel_i; term 0 when den_i == 0
__global__ void __launch_bounds__(kThreads)
l1_finish_len_kernel(const L1LenArgs L, const double* __restrict__ part, float* __restrict__ term, float* __restrict__ total) {
    __shared__ double red[16];
    const L1Args& A = L.A;
    double tot = 0.0;
    for (int i = 0; i < A.n; ++i) {
        const L1Item& it = A.it[i];
        const int rowlen = it.flat() ? it.pb : (int)it.len();
        const int rows = it.flat() ? (int)(it.shape / rowlen) : it.rows();
        double s = 0.0;
        for (int k = A.starts[i] + threadIdx.x; k < A.starts[i + 1]; k += kThreads) s += part[k];
        s = v2w_block_sum(s, red);
        const double den = len_denominator(L.ext + (size_t)i * L.B, L.B, rows / L.B, rowlen, red);
        const double mean = den > 0.0 ? s / den : 0.0;
        if (threadIdx.x == 0 && term) term[i] = (float)mean;
        tot += mean;
    }
    if (threadIdx.x == 0 && total) total[0] = (float)((double)A.scale * tot);
}

// lsgan_multi_kernel over the counted floats: row r = e / valid of item r / rpi counts its first v floats
__global__ void __launch_bounds__(1024)
lsgan_multi_len_kernel(const LsLenArgs L, float* __restrict__ term, float* __restrict__ total) {
    __shared__ double red[16];
    double tot = 0.0;
    for (int i = 0; i < L.A.n; ++i) {
        const LsItem& it = L.A.it[i];
        const int32_t* __restrict__ ext = L.ext + (size_t)i * L.B;
        const unsigned rpi = it.numel / it.valid / (unsigned)L.B;
        const double t = (double)it.target;
        double acc = 0.0;
        for (unsigned e = threadIdx.x; e < it.numel; e += 1024) {
            const unsigned r = e / it.valid, j = e - r * it.valid;
            if ((int)j < ext_clamp(ext[r / rpi], (int)it.valid)) {
                const double d = t - (double)it.s[(size_t)r * it.pitch + j];
                acc += d * d;
            }
        }
        acc = v2w_block_sum(acc, red);
        const double den = len_denominator(ext, L.B, (int)rpi, (int)it.valid, red);
        const double mean = den > 0.0 ? acc / den : 0.0;
        if (threadIdx.x == 0 && term) term[i] = (float)mean;
        tot += mean;
    }
    if (threadIdx.x == 0 && total) total[0] = (float)tot;
}

// ds = 2 (s - t) * g / den on the counted floats, +0.0 on the others, dense; grid (blocks, items)
__global__ void __launch_bounds__(kThreads)
lsgan_multi_len_bwd_kernel(const LsLenArgs L) {
    __shared__ double red[16];
    const int i = blockIdx.y;
    const LsItem& it = L.A.it[i];
    if (!it.ds) return;
    const int32_t* __restrict__ ext = L.ext + (size_t)i * L.B;
    const unsigned rpi = it.numel / it.valid / (unsigned)L.B;
    const double den = len_denominator(ext, L.B, (int)rpi, (int)it.valid, red);
    const float g = (L.A.gout ? L.A.gout[0] : 0.f) + (L.A.gterm ? L.A.gterm[i] : 0.f);
    const float c = den > 0.0 ? g / (float)den : 0.f;
    for (unsigned e = blockIdx.x * kThreads + threadIdx.x; e < it.numel; e += gridDim.x * kThreads) {
        const unsigned r = e / it.valid, j = e - r * it.valid;
        const bool on = (int)j < ext_clamp(ext[r / rpi], (int)it.valid);
        it.ds[e] = on ? 2.f * (it.s[(size_t)r * it.pitch + j] - it.target) * c : 0.f;
    }
}

// ---- v2w_map_extents: thread (i, b) walks row i's chain from item b's samples
__global__ void __launch_bounds__(kThreads)
map_extents_kernel(const int32_t* __restrict__ len, int len_mul, int L, int B, const int32_t* __restrict__ chains, int n,
                   const int32_t* __restrict__ layers, int32_t* __restrict__ ext) {
    const int idx = blockIdx.x * kThreads + threadIdx.x;
    if (idx >= n * B) return;
    const int i = idx / B, b = idx - i * B;
    const int period = chains[4 * i], pools = chains[4 * i + 1], depth = chains[4 * i + 2], size = chains[4 * i + 3];
    long long m = (long long)len[b] * len_mul;
    m = m < 0 ? 0 : (m < L ? m : L);
    m = (m + period - 1) / period;
    for (int k = 0; k < pools; ++k) m = m > 0 ? m / 2 + 1 : 0;
    for (int l = 0; l < depth; ++l) {
        const long long num = m + 2 * layers[3 * l + 2] - layers[3 * l];
        m = m > 0 && num >= 0 ? num / layers[3 * l + 1] + 1 : 0;
    }
    if (size > 0 && m > size) m = size;
    ext[idx] = (int32_t)(m * period);
}

// ---- v2w_mask_tail: grid (blocks over a row's units, rows); VEC: L % 4 == 0 and both pointers on 16-byte lines
template <bool VEC>
__global__ void __launch_bounds__(kThreads)
mask_tail_kernel(const float* __restrict__ x, float* __restrict__ out, long long rows, int rpi, int L, const int32_t* __restrict__ len,
                 int len_mul) {
    const int units = (L + 3) >> 2;
    for (long long r = blockIdx.y; r < rows; r += gridDim.y) {
        long long mm = (long long)len[r / rpi] * len_mul;
        const int m = mm < 0 ? 0 : (mm < L ? (int)mm : L);
        const float* xr = x + r * L;
        float* orow = out + r * L;
        for (int u = blockIdx.x * kThreads + threadIdx.x; u < units; u += gridDim.x * kThreads) {
            const int p = u << 2;
            if (VEC) {
                f32x4 v = {0.f, 0.f, 0.f, 0.f};
                if (p < m) {
                    const f32x4 w = *reinterpret_cast<const f32x4*>(xr + p);
#pragma unroll
                    for (int j = 0; j < 4; ++j) v[j] = p + j < m ? w[j] : 0.f;
                }
                *reinterpret_cast<f32x4*>(orow + p) = v;
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (p + j < L) orow[p + j] = p + j < m ? xr[p + j] : 0.f;
            }
        }
    }
}

// ---- masked mel L1 of a batch of unequal lengths (v2w_l1_masked): a, b (B, C, F) dense; item b counts its first Fb = v2w_item_frames frames.  An item is
// ceil(C * F / 4) units of four floats, shared out over the gridDim.x workgroups of its grid row; workgroup (g, b) writes part[b * G + g].
constexpr int kMaskedUnitsPerWg = kThreads * kUnroll;
constexpr int kMaskedMaxWgs = 256;

// VEC: F % 4 == 0 and both pointers 16-byte aligned - a unit lies in one row and is one 16-byte load per side.  A masked element is
// selected away (its load, where a unit straddles Fb, is discarded): nothing at or past Fb reaches the sum.
template <bool VEC>
__global__ void __launch_bounds__(kThreads)
l1_masked_kernel(const float* __restrict__ a, const float* __restrict__ b, const int32_t* __restrict__ len, int len_mul, int hop, int n_fft,
                 int C, int F, double* __restrict__ part) {
    __shared__ double red[16];
    const int item = blockIdx.y, G = gridDim.x;
    const int Fb = v2w_item_frames(len, item, len_mul, hop, n_fft, F);
    const int n = C * F;
    const int units = (n + 3) >> 2;
    const int chunk = (units + G - 1) / G;
    const int u0 = blockIdx.x * chunk;
    const int u1 = u0 + chunk < units ? u0 + chunk : units;
    const float* ai = a + (size_t)item * n;
    const float* bi = b + (size_t)item * n;
    double acc = 0.0;
    if (Fb > 0) {
        for (int t0 = u0 + threadIdx.x; t0 < u1; t0 += kThreads * kUnroll) {
            f32x4 va[kUnroll], vb[kUnroll];
            int col[kUnroll][4];                              // column of each of the unit's floats; F: masked or not there
#pragma unroll
            for (int k = 0; k < kUnroll; ++k) {
                const int u = t0 + k * kThreads;
                va[k] = vb[k] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int j = 0; j < 4; ++j) col[k][j] = F;
                if (u >= u1) continue;
                const int e = u << 2;
                if (VEC) {
                    const int c = e % F;
                    if (c < Fb) {
                        va[k] = *reinterpret_cast<const f32x4*>(ai + e);
                        vb[k] = *reinterpret_cast<const f32x4*>(bi + e);
#pragma unroll
                        for (int j = 0; j < 4; ++j) col[k][j] = c + j;
                    }
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int c = (e + j) % F;
                        if (e + j < n && c < Fb) { va[k][j] = ai[e + j]; vb[k][j] = bi[e + j]; col[k][j] = c; }
                    }
                }
            }
#pragma unroll
            for (int k = 0; k < kUnroll; ++k)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc += col[k][j] < Fb ? (double)fabsf(va[k][j] - vb[k][j]) : 0.0;
        }
    }
    const double s = v2w_block_sum(acc, red);
    if (threadIdx.x == 0) part[(size_t)item * G + blockIdx.x] = s;
}

// per_item[b] = (the item's G partials, added in index order) / (C * Fb); total = (the items' sums) / (C * sum Fb): one workgroup, thread t
// takes the items t, t + 256, ...; the sums over the items go through the fixed-order block reduction
__global__ void __launch_bounds__(kThreads)
l1_masked_finish_kernel(const double* __restrict__ part, const int32_t* __restrict__ len, int len_mul, int hop, int n_fft,
                        int B, int C, int F, int G, float* __restrict__ per_item, float* __restrict__ total) {
    __shared__ double red[16];
    double tot = 0.0, cnt = 0.0;
    for (int b = threadIdx.x; b < B; b += kThreads) {
        const int Fb = v2w_item_frames(len, b, len_mul, hop, n_fft, F);
        double s = 0.0;
        for (int g = 0; g < G; ++g) s += part[(size_t)b * G + g];
        const double ne = (double)C * (double)Fb;
        if (per_item) per_item[b] = Fb > 0 ? (float)(s / ne) : 0.f;
        tot += s;                                             // (an item without frames wrote zeros)
        cnt += ne;
    }
    tot = v2w_block_sum(tot, red);
    cnt = v2w_block_sum(cnt, red);
    if (threadIdx.x == 0 && total) total[0] = cnt > 0.0 ? (float)(tot / cnt) : 0.f;
}


// checks every descriptor, normalises it into the kernel's form and counts its units (four floats; see the head of this file)
int l1_items(const v2w_l1_pair* pairs, int n, L1Item* items, long long* units) {
    if (!pairs || n < 1 || n > V2W_LOSS_MAX_ITEMS) return V2W_E_ARG;
    for (int i = 0; i < n; ++i) {
        const v2w_l1_pair& p = pairs[i];
        if (!ptr4(p.a) || !ptr4(p.b) || p.rows <= 0 || p.valid <= 0 || p.pitch_a < 0 || p.pitch_b < 0) return V2W_E_ARG;
        const int pa = p.pitch_a ? p.pitch_a : p.valid, pb = p.pitch_b ? p.pitch_b : p.valid;
        if (pa < p.valid || pb < p.valid) return V2W_E_ARG;
        if (pa != p.valid && ((pa & 3) || !aligned16(p.a))) return V2W_E_ARG;       // pitched rows begin on 16-byte lines
        if (pb != p.valid && ((pb & 3) || !aligned16(p.b))) return V2W_E_ARG;
        if ((p.da && !ptr4(p.da)) || (p.db && !ptr4(p.db))) return V2W_E_ARG;
        L1Item& it = items[i];
        it.a = p.a; it.b = p.b; it.da = p.da; it.db = p.db;
        if (p.rows == 1 || (pa == p.valid && pb == p.valid)) {
            it.shape = (long long)p.rows * p.valid; it.pa = it.pb = 0;
            units[i] = (it.shape + phase16(p.a) + 3) >> 2;
        } else {
            if (p.rows > 0x7fffffffll) return V2W_E_SHAPE;
            it.shape = (p.rows << 32) | p.valid; it.pa = pa; it.pb = pb;
            units[i] = p.rows * ((p.valid + 3) >> 2);
        }
        if (units[i] > kMaxUnits) return V2W_E_SHAPE;
    }
    return 0;
}

int l1_args(const v2w_l1_pair* pairs, int n, float scale, const float* gout, L1Args* A) {
    long long units[V2W_LOSS_MAX_ITEMS];
    if (const int rc = l1_items(pairs, n, A->it, units)) return rc;
    deal_workgroups(units, n, V2W_L1_TARGET_WGS, A->starts);
    A->n = n; A->scale = scale; A->gout = gout;
    return 0;
}

int ls_args(const v2w_lsgan_item* items, int n, bool bwd, LsArgs* A, unsigned* maxnumel) {
    if (!items || n < 1 || n > V2W_LOSS_MAX_ITEMS) return V2W_E_ARG;
    *maxnumel = 0;
    for (int i = 0; i < n; ++i) {
        const v2w_lsgan_item& p = items[i];
        if (!ptr4(p.s) || p.rows <= 0 || p.valid <= 0 || p.pitch < 0 || (p.pitch && p.pitch < p.valid)) return V2W_E_ARG;
        if (p.target != 0.f && p.target != 1.f) return V2W_E_ARG;
        if (bwd && p.ds && !ptr4(p.ds)) return V2W_E_ARG;
        const long long numel = (long long)p.rows * p.valid;
        if (numel > 0x7fffffffll) return V2W_E_SHAPE;
        LsItem& it = A->it[i];
        it.s = p.s; it.ds = p.ds; it.numel = (unsigned)numel; it.valid = (unsigned)p.valid;
        it.pitch = (unsigned)(p.pitch ? p.pitch : p.valid); it.target = p.target;
        if (it.numel > *maxnumel) *maxnumel = it.numel;
    }
    A->n = n; A->gout = nullptr; A->gterm = nullptr;
    return 0;
}

// the dense call's arguments and plan, with the batch split: rows % B == 0, and a flat item's row length where the kernels find it
int l1_len_args(const v2w_l1_pair* pairs, int n, const int32_t* ext, int B, float scale, const float* gout, L1LenArgs* L) {
    if (!ptr4(ext) || B < 1) return V2W_E_ARG;
    if (const int rc = l1_args(pairs, n, scale, gout, &L->A)) return rc;
    for (int i = 0; i < n; ++i) {
        if (pairs[i].rows % B) return V2W_E_ARG;
        if (pairs[i].rows > 0x7fffffffll) return V2W_E_SHAPE;
        if (L->A.it[i].flat()) L->A.it[i].pb = pairs[i].valid;
    }
    L->ext = ext; L->B = B;
    return 0;
}

int ls_len_args(const v2w_lsgan_item* items, int n, const int32_t* ext, int B, bool bwd, LsLenArgs* L, unsigned* maxnumel) {
    if (!ptr4(ext) || B < 1) return V2W_E_ARG;
    if (const int rc = ls_args(items, n, bwd, &L->A, maxnumel)) return rc;
    for (int i = 0; i < n; ++i)
        if (items[i].rows % B) return V2W_E_ARG;
    L->ext = ext; L->B = B;
    return 0;
}

}  // namespace

extern "C" int v2w_l1_multi_plan(const v2w_l1_pair* pairs, int n, int32_t* starts) {
    if (!starts) return V2W_E_ARG;
    L1Item items[V2W_LOSS_MAX_ITEMS];
    long long units[V2W_LOSS_MAX_ITEMS];
    if (const int rc = l1_items(pairs, n, items, units)) return rc;
    return deal_workgroups(units, n, V2W_L1_TARGET_WGS, starts);
}

extern "C" long long v2w_l1_multi_scratch_bytes(const v2w_l1_pair* pairs, int n) {
    int32_t starts[V2W_LOSS_MAX_ITEMS + 1];
    const int w = v2w_l1_multi_plan(pairs, n, starts);
    return w < 0 ? (long long)w : (long long)w * (long long)sizeof(double);
}

extern "C" int v2w_l1_mean_multi(const v2w_l1_pair* pairs, int n, float scale, float* term, float* total, void* scratch, void* stream) {
    if (!scratch || (!term && !total) || (reinterpret_cast<uintptr_t>(scratch) & 7)) return V2W_E_ARG;
    L1Args A;
    if (const int rc = l1_args(pairs, n, scale, nullptr, &A)) return rc;
    hipStream_t st = (hipStream_t)stream;
    double* part = static_cast<double*>(scratch);
    V2W_LAUNCH(l1_multi_kernel<false>, dim3(A.starts[n]), dim3(kThreads), 0, st, A, part);
    V2W_LAUNCH(l1_finish_kernel, dim3(1), dim3(kThreads), 0, st, A, part, term, total);
    return v2w_launch_status();
}

extern "C" int v2w_l1_mean_multi_bwd(const v2w_l1_pair* pairs, int n, float scale, const float* gout, void* stream) {
    if (!gout) return V2W_E_ARG;
    L1Args A;
    if (const int rc = l1_args(pairs, n, scale, gout, &A)) return rc;
    bool any = false;
    for (int i = 0; i < n; ++i) any = any || A.it[i].da || A.it[i].db;
    if (!any) return V2W_E_ARG;
    V2W_LAUNCH(l1_multi_kernel<true>, dim3(A.starts[n]), dim3(kThreads), 0, (hipStream_t)stream, A, static_cast<double*>(nullptr));
    return v2w_launch_status();
}

extern "C" int v2w_l1_masked_plan(int C, int F) {
    if (C <= 0 || F <= 0) return V2W_E_ARG;
    const long long n = (long long)C * F;
    if (n > 0x7fffffffll - 3) return V2W_E_SHAPE;
    const long long g = ((n + 3) / 4 + kMaskedUnitsPerWg - 1) / kMaskedUnitsPerWg;
    return g < 1 ? 1 : (g > kMaskedMaxWgs ? kMaskedMaxWgs : (int)g);
}

// geo: any 1 <= hop <= n_fft (v2w_l1_masked_geo); the kernels' frame count, pad = (n_fft - hop) / 2 rounded down, is the same
static int l1_masked(const float* a, const float* b, int B, int C, int F, const int32_t* len, int len_mul, int hop, int n_fft,
                     float* per_item, float* total, void* ws, void* stream, bool geo) {
    if (!a || !b || !len || !ws || (!per_item && !total) || B <= 0 || len_mul < 1 || hop < 1 || n_fft < hop) return V2W_E_ARG;
    if (!geo && (n_fft % hop || (n_fft - hop) % 2)) return V2W_E_ARG;
    if (!ptr4(a) || !ptr4(b) || (reinterpret_cast<uintptr_t>(ws) & 7)) return V2W_E_ARG;
    const int G = v2w_l1_masked_plan(C, F);
    if (G < 0) return G;
    if (B > 65535) return V2W_E_SHAPE;                        // (grid.y)
    hipStream_t st = (hipStream_t)stream;
    double* part = static_cast<double*>(ws);
    if (F % 4 == 0 && aligned16(a) && aligned16(b))
        V2W_LAUNCH(l1_masked_kernel<true>, dim3(G, B), dim3(kThreads), 0, st, a, b, len, len_mul, hop, n_fft, C, F, part);
    else
        V2W_LAUNCH(l1_masked_kernel<false>, dim3(G, B), dim3(kThreads), 0, st, a, b, len, len_mul, hop, n_fft, C, F, part);
    V2W_LAUNCH(l1_masked_finish_kernel, dim3(1), dim3(kThreads), 0, st, part, len, len_mul, hop, n_fft, B, C, F, G, per_item, total);
    return v2w_launch_status();
}

extern "C" int v2w_l1_masked(const float* a, const float* b, int B, int C, int F, const int32_t* len, int len_mul, int hop, int n_fft,
                             float* per_item, float* total, void* ws, void* stream) {
    return l1_masked(a, b, B, C, F, len, len_mul, hop, n_fft, per_item, total, ws, stream, false);
}

extern "C" int v2w_l1_masked_geo(const float* a, const float* b, int B, int C, int F, const int32_t* len, int len_mul, int hop, int n_fft,
                                 float* per_item, float* total, void* ws, void* stream) {
    return l1_masked(a, b, B, C, F, len, len_mul, hop, n_fft, per_item, total, ws, stream, true);
}

extern "C" int v2w_lsgan_multi(const v2w_lsgan_item* items, int n, float* term, float* total, void* stream) {
    if (!term && !total) return V2W_E_ARG;
    LsArgs A;
    unsigned maxnumel;
    if (const int rc = ls_args(items, n, false, &A, &maxnumel)) return rc;
    V2W_LAUNCH(lsgan_multi_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, A, term, total);
    return v2w_launch_status();
}

extern "C" int v2w_lsgan_multi_bwd(const v2w_lsgan_item* items, int n, const float* gout, const float* gterm, void* stream) {
    if (!gout && !gterm) return V2W_E_ARG;
    LsArgs A;
    unsigned maxnumel;
    if (const int rc = ls_args(items, n, true, &A, &maxnumel)) return rc;
    A.gout = gout; A.gterm = gterm;
    unsigned nbx = (maxnumel + kThreads - 1) / kThreads;
    if (nbx > 256) nbx = 256;
    V2W_LAUNCH(lsgan_multi_bwd_kernel, dim3(nbx, n), dim3(kThreads), 0, (hipStream_t)stream, A);
    return v2w_launch_status();
}

extern "C" int v2w_l1_mean_multi_len(const v2w_l1_pair* pairs, int n, const int32_t* ext, int B, float scale, float* term, float* total,
                                     void* scratch, void* stream) {
    if (!scratch || (!term && !total) || (reinterpret_cast<uintptr_t>(scratch) & 7)) return V2W_E_ARG;
    L1LenArgs L;
    if (const int rc = l1_len_args(pairs, n, ext, B, scale, nullptr, &L)) return rc;
    hipStream_t st = (hipStream_t)stream;
    double* part = static_cast<double*>(scratch);
    V2W_LAUNCH(l1_multi_len_kernel<false>, dim3(L.A.starts[n]), dim3(kThreads), 0, st, L, part);
    V2W_LAUNCH(l1_finish_len_kernel, dim3(1), dim3(kThreads), 0, st, L, part, term, total);
    return v2w_launch_status();
}

extern "C" int v2w_l1_mean_multi_len_bwd(const v2w_l1_pair* pairs, int n, const int32_t* ext, int B, float scale, const float* gout,
                                         void* stream) {
    if (!gout) return V2W_E_ARG;
    L1LenArgs L;
    if (const int rc = l1_len_args(pairs, n, ext, B, scale, gout, &L)) return rc;
    bool any = false;
    for (int i = 0; i < n; ++i) any = any || L.A.it[i].da || L.A.it[i].db;
    if (!any) return V2W_E_ARG;
    V2W_LAUNCH(l1_multi_len_kernel<true>, dim3(L.A.starts[n]), dim3(kThreads), 0, (hipStream_t)stream, L, static_cast<double*>(nullptr));
    return v2w_launch_status();
}

extern "C" int v2w_lsgan_multi_len(const v2w_lsgan_item* items, int n, const int32_t* ext, int B, float* term, float* total, void* stream) {
    if (!term && !total) return V2W_E_ARG;
    LsLenArgs L;
    unsigned maxnumel;
    if (const int rc = ls_len_args(items, n, ext, B, false, &L, &maxnumel)) return rc;
    V2W_LAUNCH(lsgan_multi_len_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, L, term, total);
    return v2w_launch_status();
}

extern "C" int v2w_lsgan_multi_len_bwd(const v2w_lsgan_item* items, int n, const int32_t* ext, int B, const float* gout, const float* gterm,
                                       void* stream) {
    if (!gout && !gterm) return V2W_E_ARG;
    LsLenArgs L;
    unsigned maxnumel;
    if (const int rc = ls_len_args(items, n, ext, B, true, &L, &maxnumel)) return rc;
    L.A.gout = gout; L.A.gterm = gterm;
    unsigned nbx = (maxnumel + kThreads - 1) / kThreads;
    if (nbx > 256) nbx = 256;
    V2W_LAUNCH(lsgan_multi_len_bwd_kernel, dim3(nbx, n), dim3(kThreads), 0, (hipStream_t)stream, L);
    return v2w_launch_status();
}

extern "C" int v2w_map_extents(const int32_t* len, int len_mul, int L, int B, const int32_t* chains, int n, const int32_t* layers,
                               int n_layers, int32_t* ext, void* stream) {
    if (!len || !chains || !ext || (n_layers > 0 && !layers) || B < 1 || n < 1 || len_mul < 1 || L < 0 || n_layers < 0) return V2W_E_ARG;
    if ((long long)n * B > 0x7fffffffll - kThreads) return V2W_E_SHAPE;
    V2W_LAUNCH(map_extents_kernel, dim3((n * B + kThreads - 1) / kThreads), dim3(kThreads), 0, (hipStream_t)stream, len, len_mul, L, B,
               chains, n, layers, ext);
    return v2w_launch_status();
}

extern "C" int v2w_mask_tail(const float* x, float* out, long long rows, int B, int L, const int32_t* len, int len_mul, void* stream) {
    if (!ptr4(x) || !ptr4(out) || !len || rows < 1 || B < 1 || rows % B || L < 1 || len_mul < 1) return V2W_E_ARG;
    if (rows / B > 0x7fffffffll) return V2W_E_SHAPE;
    const int units = (L + 3) >> 2;
    int gx = (units + kThreads * 4 - 1) / (kThreads * 4);                 // four units per thread
    if (gx > 1024) gx = 1024;
    const dim3 grid(gx, rows < 65535 ? (unsigned)rows : 65535u);
    const int rpi = (int)(rows / B);
    if (L % 4 == 0 && aligned16(x) && aligned16(out))
        V2W_LAUNCH(mask_tail_kernel<true>, grid, dim3(kThreads), 0, (hipStream_t)stream, x, out, rows, rpi, L, len, len_mul);
    else
        V2W_LAUNCH(mask_tail_kernel<false>, grid, dim3(kThreads), 0, (hipStream_t)stream, x, out, rows, rpi, L, len, len_mul);
    return v2w_launch_status();
}
