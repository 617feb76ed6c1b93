// Shared device helpers for the Vec2Wav gfx950 kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <cxxabi.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <type_traits>
#include <utility>
#include "../../include/vec2wav_hip.h"

#define V2W_WAVE 64  // CDNA wavefront width (hard-coded: warpSize folds to 64 on gfx950)

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int raw16 __attribute__((ext_vector_type(4)));   // one 16-byte MFMA operand fragment, type-agnostic
typedef __bf16 b8 __attribute__((ext_vector_type(8)));
typedef __bf16 b4 __attribute__((ext_vector_type(4)));
typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef _Float16 h4 __attribute__((ext_vector_type(4)));

// The unit of the packed weights (v2w_pack_split / v2w_pack_bf16 / v2w_split_pack_batch): bytes of the MFMA A fragments of one
// (32-row block, 16-channel k-step, tap), [hi, lo][64 lanes][16 B]; the bf16 packs fill the first KiB only.
#define V2W_FRAG_UNIT 2048

static inline int v2w_launch_status() {
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : (int)e;
}

// Host-only "would this launch be taken?" queries run the launcher itself up to the launch with this sentinel for a stream: every shape
// check the real call makes is made, nothing is launched, no attribute is set, no pointer is dereferenced.
#define V2W_DRY_STREAM (reinterpret_cast<hipStream_t>(static_cast<intptr_t>(-1)))
static inline bool v2w_dry(hipStream_t s) { return s == V2W_DRY_STREAM; }

// Name sink (include/vec2wav_hip.h, ABI v33): a "stream" with bit 0 set that is not the dry-run sentinel points at the caller's v2w_name_sink.
// A call made with it goes as far as a real call - every launch site is V2W_LAUNCH, every attribute change v2w_max_lds() - and appends the
// demangled name of each kernel it reaches instead of launching it.  The runtime maps the host stub to the kernel's symbol
// (hipKernelNameRefByPtr: a table lookup, no device needed), so no launch site spells a name.
static inline v2w_name_sink* v2w_sink(hipStream_t s) {
    const uintptr_t u = reinterpret_cast<uintptr_t>(s);
    if (!(u & 1) || s == V2W_DRY_STREAM) return nullptr;
    v2w_name_sink* k = reinterpret_cast<v2w_name_sink*>(u & ~static_cast<uintptr_t>(1));
    return k->magic == V2W_NAME_SINK_MAGIC ? k : nullptr;
}
static inline void v2w_sink_add(v2w_name_sink* k, const void* host_fn) {
    const char* m = hipKernelNameRefByPtr(host_fn, nullptr);
    int st = 0;
    char* d = m ? abi::__cxa_demangle(m, nullptr, nullptr, &st) : nullptr;
    const char* nm = d ? d : (m ? m : "?");
    const int n = (int)strlen(nm);
    if (k->buf && k->cap > 0 && k->len + n + 2 <= k->cap) {
        memcpy(k->buf + k->len, nm, n);
        k->buf[k->len + n] = '\n';
        k->len += n + 1;
        k->buf[k->len] = 0;
    }
    free(d);
}
#define V2W_LAUNCH(kern, grid, block, lds, stream, ...)                                                          \
    do {                                                                                                         \
        if (v2w_name_sink* v2w_ns_ = v2w_sink(stream)) v2w_sink_add(v2w_ns_, reinterpret_cast<const void*>(kern)); \
        else hipLaunchKernelGGL(kern, grid, block, lds, stream, __VA_ARGS__);                                    \
    } while (0)
// hipFuncAttributeMaxDynamicSharedMemorySize for a launch that needs more than 64 KB of LDS (set at every such launch: the library keeps no
// per-device state to remember it in); nothing to set for a name sink
static inline hipError_t v2w_max_lds(const void* host_fn, int lds, hipStream_t s) {
    return v2w_sink(s) ? hipSuccess : hipFuncSetAttribute(host_fn, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
}

// The launch of a kernel that may need more than 64 KB of dynamic LDS (160 KB per workgroup is the CU's all): V2W_E_SHAPE past that, the
// attribute's error if it cannot be set, else the launch and its status.
template <typename K, typename... A>
static inline int v2w_launch_lds(K kern, dim3 grid, dim3 block, size_t lds, hipStream_t stream, const A&... args) {
    if (lds > 64 * 1024) {
        if (lds > 160 * 1024) return V2W_E_SHAPE;
        hipError_t e = v2w_max_lds(reinterpret_cast<const void*>(kern), (int)lds, stream);
        if (e != hipSuccess) return (int)e;
    }
    V2W_LAUNCH(kern, grid, block, lds, stream, args...);
    return v2w_launch_status();
}

static inline bool v2w_al16(const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; }   // 16-byte aligned (or NULL)

// start[0 .. nmax] of a launch that carries n <= nmax problems side by side: workgroups [start[q], start[q + 1]) belong to problem q, which
// owns blocks[q] of them; the entries past start[n] hold a sentinel no workgroup id reaches (the kernels count the entries <= blockIdx.x).
// Returns the grid.
static inline int v2w_fill_starts(int* start, int nmax, const int* blocks, int n) {
    int grid = 0;
    for (int i = 0; i <= nmax; ++i) {
        start[i] = i <= n ? grid : 0x7fffffff;
        if (i < n) grid += blocks[i];
    }
    return grid;
}

// Compute units of the CURRENT device (the device the caller's stream belongs to: every entry point runs with it made current).
// Asked of the runtime at every launch of a persistent kernel - no process-wide cache: a value remembered from the first caller's
// device would size the grids of every other device in the process.
static inline int v2w_num_cus() {
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
    return n;
}

__device__ __forceinline__ float v2w_lrelu(float v, float slope) { return v > 0.f ? v : v * slope; }

// v / d with r = 1.f / d precomputed (one true division per thread instead of one per element): q = v*r is within one ulp of the
// quotient and r is the correctly rounded reciprocal, so one Newton step on the exact fma residual yields the correctly rounded
// quotient (Markstein) - the same bits as the division - in three VALU instructions instead of ~10.  (Denormal quotients excepted;
// the path's values are O(1).)
__device__ __forceinline__ float v2w_div_by(float v, float d, float r) {
    const float q = v * r;
    return fmaf(fmaf(-q, d, v), r, q);
}

// Sum over the 64 lanes of a wave (all lanes receive the total).
__device__ __forceinline__ double v2w_wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}
__device__ __forceinline__ float v2w_wave_sum(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// Block-wide sum for blocks of up to 1024 threads; `red` is >= 16 elements of LDS scratch.
template <typename T>
__device__ __forceinline__ T v2w_block_sum(T v, T* red) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nw = (blockDim.x + 63) >> 6;
    v = v2w_wave_sum(v);
    __syncthreads();  // protect `red` against a previous use
    if (lane == 0) red[wave] = v;
    __syncthreads();
    T t = 0;
    for (int i = 0; i < nw; ++i) t += red[i];  // fixed order: deterministic
    return t;
}

// ---- batches of unequal lengths in mel_spectrogram's framing: the frames item b counts, min(frames of len[b] * len_mul samples, F).
// pad = (n_fft - hop) / 2 rounded down; reflect padding needs more than pad samples, one frame needs n_fft padded ones.  The sample count
// stays in 64 bits, so every len[b] and len_mul >= 1 is taken as it is (negative: no frame) - the mel kernels and the masked L1 agree.
__device__ __forceinline__ int v2w_item_frames(const int32_t* __restrict__ len, int b, int len_mul, int hop, int n_fft, int F) {
    const int pad = (n_fft - hop) / 2;
    const long long n = (long long)len[b] * len_mul;
    if (n <= pad || n + 2 * pad < n_fft) return 0;
    const long long fr = (n + 2 * pad - n_fft) / hop + 1;
    return fr < F ? (int)fr : F;
}

// ---- bf16 storage format on raw words: element 0 of a packed pair is the low half
__device__ __forceinline__ unsigned int v2w_bf16x2(float lo, float hi) {
    typedef __bf16 b2 __attribute__((ext_vector_type(2)));
    b2 v; v[0] = (__bf16)lo; v[1] = (__bf16)hi;          // plain casts: v_cvt_pk_bf16_f32 (round to nearest even, NaN stays NaN)
    return __builtin_bit_cast(unsigned int, v);
}
__device__ __forceinline__ float v2w_bf16_lo(unsigned int w) { return __builtin_bit_cast(float, w << 16); }
__device__ __forceinline__ float v2w_bf16_hi(unsigned int w) { return __builtin_bit_cast(float, w & 0xffff0000u); }

// ---- wave primitives
// a wave-uniform value as a scalar register (the pointer form, over pin_s, is in v2w_tile.h)
__device__ __forceinline__ int v2w_uni(int v) { return __builtin_amdgcn_readfirstlane(v); }
// DPP move inside rows of 16 lanes, e.g. quad_perm [1,0,3,2] (0xB1) / [2,3,0,1] (0x4E): the value of lane ^ 1 / lane ^ 2 in every group of four
template <int CTRL> __device__ __forceinline__ float v2w_dpp(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), CTRL, 0xF, 0xF, true));
}
__device__ __forceinline__ float v2w_readlane(float v, int l) {           // (the builtin is typed int: a float argument would be CONVERTED)
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), l));
}
// sum over the 16 lanes of a DPP row, in every lane of the row (fixed order): quad xor 1, quad xor 2, half mirror, mirror
__device__ __forceinline__ float v2w_row16_sum(float v) {
    v += v2w_dpp<0xB1>(v);
    v += v2w_dpp<0x4E>(v);
    v += v2w_dpp<0x141>(v);
    v += v2w_dpp<0x140>(v);
    return v;
}

// One-instruction VALU forms.  max(v, w): fmaxf(v, w) costs two v_max here - hipcc first canonicalises an operand that comes out of an
// MFMA with v_max_f32(v, v).  Scalar-form multiplies and adds beside MFMAs: left to -O3 these are SLP-packed into v_pk_mul_f32 /
// v_pk_add_f32, which issue at well under half the rate of two plain instructions next to matrix work (MI355X guide, 'price of one
// filler beside MFMAs').
__device__ __forceinline__ float v2w_max(float v, float w) { float t; asm("v_max_f32 %0, %1, %2" : "=v"(t) : "v"(v), "v"(w)); return t; }
__device__ __forceinline__ float v2w_mul(float v, float w) { float t; asm("v_mul_f32 %0, %1, %2" : "=v"(t) : "v"(v), "v"(w)); return t; }
__device__ __forceinline__ float v2w_fma(float a, float b, float c) { float t; asm("v_fma_f32 %0, %1, %2, %3" : "=v"(t) : "v"(a), "v"(b), "v"(c)); return t; }
__device__ __forceinline__ float v2w_add(float v, float w) { float t; asm("v_add_f32 %0, %1, %2" : "=v"(t) : "v"(v), "v"(w)); return t; }

// f(std::integral_constant<int, I>{}) for every I of the sequence, in order
template <int... I, class F> __device__ __forceinline__ void v2w_static_for(std::integer_sequence<int, I...>, F&& f) { (f(std::integral_constant<int, I>{}), ...); }

// Workgroup barrier for LDS hand-overs only: __syncthreads() also fences global memory - a wave that has just issued its tile's output
// stores would wait vmcnt(0) (the stores' acknowledgement, thousands of cycles under load) before it may even arrive at the barrier.
__device__ __forceinline__ void v2w_lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// LDS-DMA: 16 bytes per lane from `src` to LDS byte address lds + 16 * lane (lds wave-uniform: it goes through M0).  Inline asm ON
// PURPOSE: hipcc orders every later LDS read behind a builtin LDS-DMA with s_waitcnt vmcnt(0) (it cannot prove the buffers distinct),
// which would serialise copy and compute.  Hidden from its bookkeeping, the copy only makes the compiler's own vmcnt waits more
// conservative (vmcnt retires in order); the caller waits for the data itself, with a counted vmcnt.
__device__ __forceinline__ void v2w_lds_dma16(unsigned lds, const void* src) {
    unsigned m0_save;                                    // M0 is a reserved register: hand it back as found
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %2, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(m0_save) : "s"(lds), "v"(src) : "memory");
}

// ---- f32 MFMA fragments shared by the tile kernels.  A/B operands are ONE float per lane; for the 32x32x2 shape lane l
// holds A[row l&31][k l>>5] / B[k l>>5][col l&31], for 16x16x4 A[l&15][l>>4] / B[l>>4][l&15].
template <int MF> struct Frag;
template <> struct Frag<32> {
    typedef f32x16 acc_t;
    static constexpr int NREG = 16, KSTEP = 2;
    __device__ static __forceinline__ acc_t mfma(float a, float b, acc_t c) {
        return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
    }
    // C/D map: col = lane&31, row = (reg&3) + 8*(reg>>2) + 4*(lane>>5)
    __device__ static __forceinline__ int row(int reg, int hk) { return (reg & 3) + 8 * (reg >> 2) + 4 * hk; }
};
template <> struct Frag<16> {
    typedef f32x4 acc_t;
    static constexpr int NREG = 4, KSTEP = 4;
    __device__ static __forceinline__ acc_t mfma(float a, float b, acc_t c) {
        return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
    }
    // C/D map: col = lane&15, row = (lane>>4)*4 + reg
    __device__ static __forceinline__ int row(int reg, int hk) { return hk * 4 + reg; }
};


// ---- in-kernel timeline, DIAGNOSTIC builds only (-DV2W_TIMELINE, built and read by tools/stage_timeline.py / tools/tile_timeline.py):
// lane 0 of every wave stores s_memtime stamps into a side buffer that no kernel reads.  In the product build V2W_STAMP compiles to
// nothing and the setters do not exist.  Each instrumented source file owns its buffer pointer (no relocatable device code needed)
// and exports its setter with V2W_TL_SETTER(name).
#ifdef V2W_TIMELINE
#define V2W_TL_SLOTS 32
static __device__ unsigned long long* v2w_tl_buf;      // [blocks][4 waves][V2W_TL_SLOTS]
static __device__ int v2w_tl_blocks;
#define V2W_TL_SETTER(name)                                                                          \
    extern "C" int name(void* buf, int nblocks) {                                                    \
        hipError_t e = hipMemcpyToSymbol(HIP_SYMBOL(v2w_tl_buf), &buf, sizeof(buf));                  \
        if (e == hipSuccess) e = hipMemcpyToSymbol(HIP_SYMBOL(v2w_tl_blocks), &nblocks, sizeof(nblocks)); \
        return (int)e;                                                                               \
    }
__device__ __forceinline__ void v2w_tl_stamp(int k) {
    if ((threadIdx.x & 63) == 0 && (int)blockIdx.x < v2w_tl_blocks && (threadIdx.x >> 6) < 4 && k < V2W_TL_SLOTS - 3) {
        unsigned long long* dst = v2w_tl_buf + ((size_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * V2W_TL_SLOTS;
        dst[k] = __builtin_amdgcn_s_memtime();
        if (k == 0) {
            dst[V2W_TL_SLOTS - 1] = __builtin_amdgcn_s_getreg((31 << 11) | 4);        // HW_REG_HW_ID
            dst[V2W_TL_SLOTS - 2] = __builtin_amdgcn_s_getreg((31 << 11) | 20);       // HW_REG_XCC_ID
            dst[V2W_TL_SLOTS - 3] = __builtin_amdgcn_s_memrealtime();                 // 100 MHz: comparable across CUs
        }
    }
}
#define V2W_STAMP(k) v2w_tl_stamp(k)
#else
#define V2W_STAMP(k) ((void)0)
#endif
