// mel_spectrogram of the generated audio on the device (reference: vec2wav/dataset.py:53-77,
// called on the generator output in train.py:172-174, 266-269, 282-284):
//   reflect pad (n_fft - hop)/2  ->  STFT (hann window, center=False, onesided)  ->  sqrt(re^2 + im^2 + 1e-9)
//   ->  mel filterbank  ->  log(clamp(., 1e-5))
// The STFT is a dense contraction.  Frame f multiplies the window's support only, ypad[f*hop + left + t] for t < win, so with the padded
// signal de-interleaved by hop phase, Xg[b][p][f] = ypad[b][f*hop + left + p] (p < hop), frame f of the windowed DFT is
// S[c][f] = sum_{j < k} sum_{p < hop} Wd[c][left + j*hop + p] * Xg[b][p][f + j]  - a Conv1d with CP >= hop input channels (the channels
// [hop, CP) are zeros: the tile kernel's channel blocks), k = ceil(win / hop) taps (pad_left = 0) and 2*(n_fft/2+1) output channels (cos
// rows, then -sin rows, window folded in): it runs on the f32 MFMA tile kernel through v2w_conv1d_fwd.  This file holds the two
// memory-bound ends, each step written once as a device function; the kernels are its instantiations.  The first entry points
// (v2w_mel_phases, v2w_mel_finish and their _len / _bwd forms) are the geometry win = n_fft = 2 pad + hop, left = 0, CP = hop of the same kernels.
#include "v2w_common.h"

namespace {

// ---- batches of unequal lengths: item b holds Lb = min(len[b] * len_mul, L) samples
__device__ __forceinline__ int mel_item_samples(const int32_t* __restrict__ len, int b, int len_mul, int L) {
    const long long n = (long long)len[b] * len_mul;
    return n < 0 ? 0 : (n > L ? L : (int)n);
}
// frames of an item of Lb samples: reflect padding needs Lb > pad, one frame needs Lb + 2 pad >= n_fft
__device__ __forceinline__ int mel_item_frames(int Lb, int hop, int pad, int n_fft) {
    return (Lb > pad && Lb + 2 * pad >= n_fft) ? (Lb + 2 * pad - n_fft) / hop + 1 : 0;
}

// ---- the phase step (include/vec2wav_hip.h, "any frame geometry").  Nothing here is derived from anything else: hop, CP, pad, left, k,
// n_fft are the caller's (mel_geo_ok checks them on the host); k and n_fft are read with lengths only.

// Xg (B, CP, FP): Xg[b][p][f] = ypad[b][f*hop + left + p] for p < hop, ypad = reflect-padded y (pad samples per side; torch 'reflect': no
// edge repeat), 0 past the padded signal and in the channels [hop, CP).  LEN: the reflection about the item's own last sample, 0 from column
// roundup4(F_b + k - 1) on (the FP of the item's own B = 1 call; no frame of the item reads further); every load index s satisfies 0 <= s < Lb
template <bool LEN>
__device__ __forceinline__ void mel_phase(const float* __restrict__ y, float* __restrict__ xp, const int32_t* __restrict__ len, int len_mul,
                                          int L, int hop, int CP, int pad, int left, int k, int n_fft, int FP) {
    const int b = blockIdx.y;
    int Lb = L, FPb = FP;
    if (LEN) {
        Lb = mel_item_samples(len, b, len_mul, L);
        const int Fb = mel_item_frames(Lb, hop, pad, n_fft);
        FPb = Fb > 0 ? (Fb + k - 1 + 3) / 4 * 4 : 0;
    }
    const int Lp = Lb + 2 * pad;
    for (int idx = blockIdx.x * 256 + threadIdx.x; idx < CP * FP; idx += gridDim.x * 256) {
        const int p = idx / FP, f = idx - p * FP;
        float v = 0.f;
        if (p < hop && f < FPb) {
            const int i = f * hop + left + p;
            if (i < Lp) {
                int s = i - pad;
                s = s < 0 ? -s : (s >= Lb ? 2 * (Lb - 1) - s : s);   // -s <= pad < Lb;  2(Lb-1) - s >= Lb - 1 - pad >= 0
                v = y[(size_t)b * L + s];
            }
        }
        xp[((size_t)b * CP + p) * FP + f] = v;
    }
}
#define V2W_MEL_PHASE_ARGS const float* __restrict__ src, float* __restrict__ dst, const int32_t* __restrict__ len, int len_mul, \
                           int L, int hop, int CP, int pad, int left, int k, int n_fft, int FP
__global__ void __launch_bounds__(256) mel_phase_kernel(V2W_MEL_PHASE_ARGS) {
    mel_phase<false>(src, dst, len, len_mul, L, hop, CP, pad, left, k, n_fft, FP);
}
__global__ void __launch_bounds__(256) mel_phase_len_kernel(V2W_MEL_PHASE_ARGS) {
    mel_phase<true>(src, dst, len, len_mul, L, hop, CP, pad, left, k, n_fft, FP);
}

// Backward of mel_phase_kernel: dy[b][s] = sum of dxp over the padded positions i that read y[s]: i = s + pad always, the left reflection
// i = pad - s for 1 <= s <= pad, the right reflection i = 2(Lb-1) - s + pad for Lb-1-pad <= s <= Lb-2, added in that order.  The padded
// position i is Xg[(i - left) % hop][(i - left) / hop] where 0 <= i - left < hop * FP, and is read by nothing elsewhere (samples past the
// last frame: unused).  LEN: the right reflection about the ITEM's last sample, the columns from its own FPb = roundup4(Fb + k - 1) on read
// as 0 (whatever they hold), dy[b, Lb:] = +0.0, an item without a frame all +0.0: the bits of the B = 1 plain call on dxp[b, :, :FPb].
template <bool LEN>
__device__ __forceinline__ void mel_phase_bwd(const float* __restrict__ dxp, float* __restrict__ dy, const int32_t* __restrict__ len, int len_mul,
                                              int L, int hop, int CP, int pad, int left, int k, int n_fft, int FP) {
    const int b = blockIdx.y;
    int Lb = L, FPb = FP;
    if (LEN) {
        Lb = mel_item_samples(len, b, len_mul, L);
        const int Fb = mel_item_frames(Lb, hop, pad, n_fft);
        FPb = Fb > 0 ? (Fb + k - 1 + 3) / 4 * 4 : 0;
        FPb = FPb < FP ? FPb : FP;
    }
    const float* xb = dxp + (size_t)b * CP * FP;
    auto at = [&](int i) {
        const int q = i - left;
        return (q >= 0 && q / hop < FPb) ? xb[(size_t)(q % hop) * FP + q / hop] : 0.f;
    };
    for (int s = blockIdx.x * 256 + threadIdx.x; s < L; s += gridDim.x * 256) {
        float v = 0.f;
        if (s < Lb && FPb > 0) {
            v = at(s + pad);
            if (s >= 1 && s <= pad) v += at(pad - s);
            if (s >= Lb - 1 - pad && s <= Lb - 2) v += at(2 * (Lb - 1) - s + pad);
        }
        dy[(size_t)b * L + s] = v;
    }
}
__global__ void __launch_bounds__(256) mel_phase_bwd_kernel(V2W_MEL_PHASE_ARGS) {
    mel_phase_bwd<false>(src, dst, len, len_mul, L, hop, CP, pad, left, k, n_fft, FP);
}
__global__ void __launch_bounds__(256) mel_phase_len_bwd_kernel(V2W_MEL_PHASE_ARGS) {
    mel_phase_bwd<true>(src, dst, len, len_mul, L, hop, CP, pad, left, k, n_fft, FP);
}
#undef V2W_MEL_PHASE_ARGS

// ---- the finish step.  spec (B, Cs, FP): rows [0, nb) = Re, rows [nb, 2nb) = Im of the nb = n_fft/2+1 bins.  One workgroup = FT frames of
// one batch item, FT = 16, or 8 for the bin counts whose 16-frame block passes 64 KiB of LDS (nb = 1025: n_fft 2048).  Its three steps:

// the frames item b counts: F without lengths, else min(its own frames, F, Ft)
template <bool LEN>
__device__ __forceinline__ int mel_item_fb(const int32_t* __restrict__ len, int b, int len_mul, int hop, int n_fft, int F, int Ft) {
    if (!LEN) return F;
    const int Fb = v2w_item_frames(len, b, len_mul, hop, n_fft, F);
    return Fb < Ft ? Fb : Ft;
}

// mag[nb][FT]: the magnitudes of the frames [f0, f0 + FT) below Fb of one item's spec sb, `fill` at and past Fb (nothing there is loaded)
template <int FT>
__device__ __forceinline__ void mel_stage_mag(const float* __restrict__ sb, float* mag, int FP, int nb, int f0, int Fb, float fill) {
    for (int idx = threadIdx.x; idx < nb * FT; idx += 256) {
        const int c = idx / FT, f = f0 + idx % FT;
        float m = fill;
        if (f < Fb) {
            const float re = sb[(size_t)c * FP + f], im = sb[(size_t)(nb + c) * FP + f];
            m = sqrtf(re * re + im * im + 1e-9f);
        }
        mag[idx] = m;
    }
}

// one output of the filterbank: the dot of the dense basis row br with frame ff's magnitudes, fmaf over the bins c = 0 .. nb - 1
template <int FT>
__device__ __forceinline__ float mel_acc(const float* __restrict__ br, const float* mag, int nb, int ff) {
    float acc = 0.f;
    for (int c = 0; c < nb; ++c) acc = fmaf(br[c], mag[c * FT + ff], acc);
    return acc;
}

// The last step of the backward: d_mag = basisT @ d_acc (basisT the (nb, n_mels) transpose, so the dot reads rows), then
//   d_re = d_mag * re / mag, d_im = d_mag * im / mag      (mag = sqrt(re^2 + im^2 + 1e-9) > 0)
// into the rows < 2 * nb of the frames < Fb of one item's dspec db; the rest of dspec is the caller's zero fill.
template <int FT>
__device__ __forceinline__ void mel_scatter_dspec(const float* __restrict__ sb, float* __restrict__ db, const float* __restrict__ basisT,
                                                  const float* mag, const float* dacc, int FP, int nb, int n_mels, int f0, int Fb) {
    for (int idx = threadIdx.x; idx < nb * FT; idx += 256) {
        const int c = idx / FT, ff = idx - c * FT;
        const int f = f0 + ff;
        if (f >= Fb) continue;
        const float* bt = basisT + (size_t)c * n_mels;
        float dm = 0.f;
        for (int m = 0; m < n_mels; ++m) dm = fmaf(bt[m], dacc[m * FT + ff], dm);
        const float s = dm / mag[idx];
        db[(size_t)c * FP + f] = s * sb[(size_t)c * FP + f];
        db[(size_t)(nb + c) * FP + f] = s * sb[(size_t)(nb + c) * FP + f];
    }
}

// out (B, n_mels, F) = log(clamp(basis @ |spec|, 1e-5)): magnitudes into LDS, then the FT x n_mels outputs.  LEN: the first Fb frames of
// item b (the same operations in the same order), 0.0 in the frames [Fb, F); a workgroup at or past Fb leaves spec unread.
template <int FT, bool LEN>
__device__ __forceinline__ void mel_finish(const float* __restrict__ spec, const float* __restrict__ basis, float* __restrict__ out,
                                           const int32_t* __restrict__ len, int len_mul, int hop, int n_fft, int Cs, int FP, int F, int nb,
                                           int n_mels) {
    extern __shared__ float mag[];                     // [nb][FT]
    const int b = blockIdx.y, f0 = blockIdx.x * FT;
    const int Fb = mel_item_fb<LEN>(len, b, len_mul, hop, n_fft, F, F);
    if (LEN && f0 >= Fb) {                             // (uniform over the workgroup) nothing of the item here: zeros
        for (int idx = threadIdx.x; idx < n_mels * FT; idx += 256) {
            const int m = idx / FT, f = f0 + idx % FT;
            if (f < F) out[((size_t)b * n_mels + m) * F + f] = 0.f;
        }
        return;
    }
    mel_stage_mag<FT>(spec + (size_t)b * Cs * FP, mag, FP, nb, f0, Fb, 0.f);
    __syncthreads();
    for (int idx = threadIdx.x; idx < n_mels * FT; idx += 256) {
        const int m = idx / FT, ff = idx - m * FT;
        const int f = f0 + ff;
        if (f >= F) continue;
        float v = 0.f;
        if (f < Fb) {
            const float acc = mel_acc<FT>(basis + (size_t)m * nb, mag, nb, ff);
            v = logf(fmaxf(acc, 1e-5f));
        }
        out[((size_t)b * n_mels + m) * F + f] = v;
    }
}
#define V2W_MEL_FINISH_ARGS const float* __restrict__ spec, const float* __restrict__ basis, float* __restrict__ out, \
                            const int32_t* __restrict__ len, int len_mul, int hop, int n_fft, int Cs, int FP, int F, int nb, int n_mels
__global__ void __launch_bounds__(256) mel_finish_kernel(V2W_MEL_FINISH_ARGS) {
    mel_finish<16, false>(spec, basis, out, len, len_mul, hop, n_fft, Cs, FP, F, nb, n_mels);
}
__global__ void __launch_bounds__(256) mel_finish_len_kernel(V2W_MEL_FINISH_ARGS) {
    mel_finish<16, true>(spec, basis, out, len, len_mul, hop, n_fft, Cs, FP, F, nb, n_mels);
}
template <bool LEN>
__global__ void __launch_bounds__(256) mel_finish8_kernel(V2W_MEL_FINISH_ARGS) {
    mel_finish<8, LEN>(spec, basis, out, len, len_mul, hop, n_fft, Cs, FP, F, nb, n_mels);
}
#undef V2W_MEL_FINISH_ARGS

// Backward of the finish without lengths for the same block: with acc = basis @ mag,
//   d_acc = g / acc where acc >= 1e-5 (the clamp passes the gradient on its closed side), then mel_scatter_dspec.
// dspec must be zero-filled: only rows < 2*nb, frames < F are written.
template <int FT>
__device__ __forceinline__ void mel_finish_bwd(const float* __restrict__ spec, const float* __restrict__ basis, const float* __restrict__ basisT,
                                               const float* __restrict__ gout, float* __restrict__ dspec, int Cs, int FP, int F, int nb,
                                               int n_mels) {
    extern __shared__ float mag[];                     // [nb][FT] then d_acc [n_mels][FT]
    float* dacc = mag + (size_t)nb * FT;
    const int b = blockIdx.y, f0 = blockIdx.x * FT;
    const float* sb = spec + (size_t)b * Cs * FP;
    mel_stage_mag<FT>(sb, mag, FP, nb, f0, F, 1.f);
    __syncthreads();
    for (int idx = threadIdx.x; idx < n_mels * FT; idx += 256) {
        const int m = idx / FT, ff = idx - m * FT;
        const int f = f0 + ff;
        float d = 0.f;
        if (f < F) {
            const float acc = mel_acc<FT>(basis + (size_t)m * nb, mag, nb, ff);
            if (acc >= 1e-5f) d = gout[((size_t)b * n_mels + m) * F + f] / acc;
        }
        dacc[idx] = d;
    }
    __syncthreads();
    mel_scatter_dspec<FT>(sb, dspec + (size_t)b * Cs * FP, basisT, mag, dacc, FP, nb, n_mels, f0, F);
}
#define V2W_MEL_FINISH_BWD_ARGS const float* __restrict__ spec, const float* __restrict__ basis, const float* __restrict__ basisT, \
                                const float* __restrict__ gout, float* __restrict__ dspec, int Cs, int FP, int F, int nb, int n_mels
__global__ void __launch_bounds__(256) mel_finish_bwd_kernel(V2W_MEL_FINISH_BWD_ARGS) {
    mel_finish_bwd<16>(spec, basis, basisT, gout, dspec, Cs, FP, F, nb, n_mels);
}
__global__ void __launch_bounds__(256) mel_finish8_bwd_kernel(V2W_MEL_FINISH_BWD_ARGS) {
    mel_finish_bwd<8>(spec, basis, basisT, gout, dspec, Cs, FP, F, nb, n_mels);
}
#undef V2W_MEL_FINISH_BWD_ARGS

// ---- the mel L1 training loss, fused into the finish step (include/vec2wav_hip.h, "Fused mel L1 training loss").  The target is dense,
// (B, Ft, n_mels) or (B, n_mels, Ft), read through its frame and mel strides.  Item b counts Fb = min(its own frames, F, Ft) frames; without
// lengths Fb = F (the host checks Ft >= F).  Every select below is on f < Fb: nothing at or past Fb, of spec or of the target, is loaded.

// mel_finish_kernel up to v = logf(fmaxf(acc, 1e-5f)), the same operations in the same order; in place of the store, |v - t| (one fp32
// rounding) is added in fp64: a thread's entries in index order, then the workgroup's fixed-order reduction, to ONE partial
// part[b * gridDim.x + blockIdx.x].  A workgroup whose frames all lie at or past Fb writes 0.0 and reads nothing.  The reduction's 16
// doubles reuse the magnitudes' LDS (v2w_block_sum syncs before it writes them).
template <int FT, bool LEN>
__global__ void __launch_bounds__(256)
mel_loss_fwd_kernel(const float* __restrict__ spec, const float* __restrict__ basis, const float* __restrict__ tgt, int ts_f, int ts_m,
                    const int32_t* __restrict__ len, int len_mul, int hop, int n_fft, int Cs, int FP, int F, int Ft, int nb, int n_mels,
                    double* __restrict__ part) {
    extern __shared__ __align__(8) float mag[];        // [nb][FT], at least 16 doubles
    const int b = blockIdx.y, f0 = blockIdx.x * FT;
    const int Fb = mel_item_fb<LEN>(len, b, len_mul, hop, n_fft, F, Ft);
    double* po = part + (size_t)b * gridDim.x + blockIdx.x;
    if (f0 >= Fb) {                                    // (uniform over the workgroup)
        if (threadIdx.x == 0) *po = 0.0;
        return;
    }
    mel_stage_mag<FT>(spec + (size_t)b * Cs * FP, mag, FP, nb, f0, Fb, 0.f);
    __syncthreads();
    const float* tb = tgt + (size_t)b * n_mels * Ft;
    double sum = 0.0;
    for (int idx = threadIdx.x; idx < n_mels * FT; idx += 256) {
        const int m = idx / FT, ff = idx - m * FT;
        const int f = f0 + ff;
        if (f >= Fb) continue;
        const float acc = mel_acc<FT>(basis + (size_t)m * nb, mag, nb, ff);
        const float v = logf(fmaxf(acc, 1e-5f));
        sum += (double)fabsf(v - tb[(size_t)f * ts_f + (size_t)m * ts_m]);
    }
    const double s = v2w_block_sum(sum, reinterpret_cast<double*>(mag));
    if (threadIdx.x == 0) *po = s;
}

// per_item[b] = (item b's partials, added in index order) / (n_mels * Fb), 0 for Fb = 0; total = scale * (the items' sums) / (n_mels *
// sum Fb); coef = scale / (n_mels * sum Fb), the factor of the backward; both 0 when no item has a frame.  One workgroup: thread t takes
// the items t, t + 256, ...; the sums over the items go through the fixed-order block reduction.  len == NULL: every item counts F frames.
__global__ void __launch_bounds__(256)
mel_loss_finish_kernel(const double* __restrict__ part, const int32_t* __restrict__ len, int len_mul, int hop, int n_fft,
                       int B, int n_mels, int F, int Ft, int tiles, float scale,
                       float* __restrict__ per_item, float* __restrict__ total, float* __restrict__ coef) {
    __shared__ double red[16];
    double tot = 0.0, cnt = 0.0;
    for (int b = threadIdx.x; b < B; b += 256) {
        const int Fb = len ? mel_item_fb<true>(len, b, len_mul, hop, n_fft, F, Ft) : F;
        double s = 0.0;
        for (int g = 0; g < tiles; ++g) s += part[(size_t)b * tiles + g];
        const double ne = (double)n_mels * (double)Fb;
        if (per_item) per_item[b] = Fb > 0 ? (float)(s / ne) : 0.f;
        tot += s;                                      // (an item without frames wrote zeros)
        cnt += ne;
    }
    tot = v2w_block_sum(tot, red);
    cnt = v2w_block_sum(cnt, red);
    if (threadIdx.x == 0) {
        if (total) total[0] = cnt > 0.0 ? (float)((double)scale * (tot / cnt)) : 0.f;
        if (coef) coef[0] = cnt > 0.0 ? (float)((double)scale / cnt) : 0.f;
    }
}

// mel_finish_bwd_kernel with d_acc = (gout * coef) * sgn(v - t) / acc where f < Fb and acc >= 1e-5f, else 0 (sgn(0) = 0; on the closed
// side of the clamp v = logf(acc)).  gout and coef are one device float each.  dspec is zero-filled by the caller: only rows < 2 * nb of
// the frames < Fb are written, and a workgroup at or past Fb reads nothing.
template <int FT, bool LEN>
__global__ void __launch_bounds__(256)
mel_loss_bwd_kernel(const float* __restrict__ spec, const float* __restrict__ basis, const float* __restrict__ basisT,
                    const float* __restrict__ tgt, int ts_f, int ts_m, const float* __restrict__ gout, const float* __restrict__ coef,
                    const int32_t* __restrict__ len, int len_mul, int hop, int n_fft, float* __restrict__ dspec,
                    int Cs, int FP, int F, int Ft, int nb, int n_mels) {
    extern __shared__ float mag[];                     // [nb][FT] then d_acc [n_mels][FT]
    float* dacc = mag + (size_t)nb * FT;
    const int b = blockIdx.y, f0 = blockIdx.x * FT;
    const int Fb = mel_item_fb<LEN>(len, b, len_mul, hop, n_fft, F, Ft);
    if (f0 >= Fb) return;                              // (uniform over the workgroup)
    const float gc = gout[0] * coef[0];
    const float* sb = spec + (size_t)b * Cs * FP;
    const float* tb = tgt + (size_t)b * n_mels * Ft;
    mel_stage_mag<FT>(sb, mag, FP, nb, f0, Fb, 1.f);
    __syncthreads();
    for (int idx = threadIdx.x; idx < n_mels * FT; idx += 256) {
        const int m = idx / FT, ff = idx - m * FT;
        const int f = f0 + ff;
        float d = 0.f;
        if (f < Fb) {
            const float acc = mel_acc<FT>(basis + (size_t)m * nb, mag, nb, ff);
            if (acc >= 1e-5f) {
                const float v = logf(fmaxf(acc, 1e-5f)), t = tb[(size_t)f * ts_f + (size_t)m * ts_m];
                const float g = v > t ? gc : (v < t ? -gc : 0.f);
                d = g / acc;
            }
        }
        dacc[idx] = d;
    }
    __syncthreads();
    mel_scatter_dspec<FT>(sb, dspec + (size_t)b * Cs * FP, basisT, mag, dacc, FP, nb, n_mels, f0, Fb);
}

// ---- host side

// The geometry of a phase call.  The first entry points name hop, pad and FP only: the window is the frame (win = n_fft = 2 pad + hop, left
// = 0) over CP = hop channels, and k = ceil(n_fft / hop) taps cover it - n_fft / hop wherever lengths are taken ((2 pad) % hop == 0 there).
// An n_fft past int (no length reaches a frame of it; unread without lengths) stays at INT_MAX.
struct MelGeo { int B, L, n_fft, win, hop, CP, pad, left, k, FP; };
inline MelGeo mel_first_geo(int B, int L, int hop, int pad, int FP) {
    const long long n = 2ll * pad + hop;
    const int n_fft = n > 0x7fffffffll ? 0x7fffffff : (int)n;
    return MelGeo{B, L, n_fft, n_fft, hop, hop, pad, 0, hop > 0 ? (int)((n_fft + (long long)hop - 1) / hop) : 0, FP};
}

// 0, V2W_E_ARG or V2W_E_SHAPE (the kernels' int arithmetic: CP * FP, the padded position (FP - 1) * hop + left + hop - 1 and L + 2 * pad)
inline int mel_geo_ok(const MelGeo& g) {
    if (g.B <= 0 || g.L <= 1 || g.hop < 1 || g.n_fft < g.hop || g.win < 1 || g.win > g.n_fft || g.CP < g.hop || g.pad < 0 || g.pad >= g.L ||
        g.left < 0 || g.left > g.n_fft - g.win || g.k < 1 || (long long)g.k * g.hop < g.win || g.FP <= 0) return V2W_E_ARG;
    if (g.B > 65535) return V2W_E_SHAPE;                      // (grid.y)
    if ((long long)g.CP * g.FP > 0x7fffffffll || (long long)g.hop * g.FP + g.left > 0x7fffffffll || (long long)g.L + 2ll * g.pad > 0x7fffffffll)
        return V2W_E_SHAPE;
    return 0;
}

// One phase launch, forward (y -> xp) or backward (dxp -> dy): a thread per element of the result, at most 1024 workgroups per item
inline dim3 mel_phase_grid(long long n, int B) {
    const long long gx = (n + 255) / 256;
    return dim3(gx > 1024 ? 1024 : (int)gx, B);
}
int mel_phase_launch(const float* src, float* dst, const MelGeo& g, bool lengths, const int32_t* len, int len_mul, bool bwd, void* stream) {
    if (!src || !dst || (lengths && (!len || len_mul < 1))) return V2W_E_ARG;
    if (const int rc = mel_geo_ok(g)) return rc;
    const auto kern = bwd ? (lengths ? mel_phase_len_bwd_kernel : mel_phase_bwd_kernel) : (lengths ? mel_phase_len_kernel : mel_phase_kernel);
    V2W_LAUNCH(kern, mel_phase_grid(bwd ? g.L : (long long)g.CP * g.FP, g.B), dim3(256), 0, (hipStream_t)stream, src, dst,
               lengths ? len : nullptr, lengths ? len_mul : 1, g.L, g.hop, g.CP, g.pad, g.left, g.k, g.n_fft, g.FP);
    return v2w_launch_status();
}

// The arguments every finish launch shares: 0, V2W_E_ARG or V2W_E_SHAPE (the kernels' n_mels * 16 is an int)
inline int mel_finish_args_ok(const void* spec, const void* basis, const void* out, int B, int Cs, int FP, int F, int nb, int n_mels) {
    if (!spec || !basis || !out || B <= 0 || F <= 0 || FP < F || nb <= 0 || Cs < 2 * nb || n_mels <= 0) return V2W_E_ARG;
    if ((long long)n_mels * 16 > 0x7fffffffll || B > 65535) return V2W_E_SHAPE;
    return 0;
}
// and those of its per-item form (the kernel's sample count of F frames is an int)
inline int mel_len_args_ok(const int32_t* len, int len_mul, int hop, int n_fft, int F) {
    if (!len || len_mul < 1 || hop < 1 || n_fft < hop) return V2W_E_ARG;
    if ((long long)F * hop + n_fft > 0x7fffffffll) return V2W_E_SHAPE;
    return 0;
}

// frames per workgroup: 16 where a block of `rows` floats per frame (forward: nb, backward: nb + n_mels) fits 64 KiB of LDS, else 8; 0: not
// even 8.  Every output is the same chain of operations either way.
inline int mel_ft(long long rows) { return rows * 16 * 4 <= 64 * 1024 ? 16 : (rows * 8 * 4 <= 64 * 1024 ? 8 : 0); }

// f(FT, LEN) with the runtime pair as integral constants
template <class Fn>
inline void mel_dispatch(int ft, bool lengths, Fn&& f) {
    if (ft == 16) { if (lengths) f(std::integral_constant<int, 16>{}, std::true_type{}); else f(std::integral_constant<int, 16>{}, std::false_type{}); }
    else { if (lengths) f(std::integral_constant<int, 8>{}, std::true_type{}); else f(std::integral_constant<int, 8>{}, std::false_type{}); }
}

// One finish launch after its argument checks.  first: the first entry points take the 16-frame block only.  len == NULL: no lengths.
int mel_finish_launch(const float* spec, const float* basis, float* out, int B, int Cs, int FP, int F, int nb, int n_mels,
               const int32_t* len, int len_mul, int hop, int n_fft, bool first, void* stream) {
    const int ft = mel_ft(nb);
    if (!ft || (first && ft != 16)) return V2W_E_SHAPE;
    const auto kern = ft == 16 ? (len ? mel_finish_len_kernel : mel_finish_kernel) : (len ? mel_finish8_kernel<true> : mel_finish8_kernel<false>);
    V2W_LAUNCH(kern, dim3((F + ft - 1) / ft, B), dim3(256), (size_t)nb * ft * sizeof(float), (hipStream_t)stream,
               spec, basis, out, len, len_mul, hop, n_fft, Cs, FP, F, nb, n_mels);
    return v2w_launch_status();
}

int mel_finish_bwd_launch(const float* spec, const float* basis, const float* basisT, const float* gout, float* dspec,
                   int B, int Cs, int FP, int F, int nb, int n_mels, bool first, void* stream) {
    if (!basisT || !gout) return V2W_E_ARG;
    if (const int rc = mel_finish_args_ok(spec, basis, dspec, B, Cs, FP, F, nb, n_mels)) return rc;
    const int ft = mel_ft((long long)nb + n_mels);
    if (!ft || (first && ft != 16)) return V2W_E_SHAPE;
    const auto kern = ft == 16 ? mel_finish_bwd_kernel : mel_finish8_bwd_kernel;
    V2W_LAUNCH(kern, dim3((F + ft - 1) / ft, B), dim3(256),
               (size_t)(nb + n_mels) * ft * sizeof(float), (hipStream_t)stream, spec, basis, basisT, gout, dspec, Cs, FP, F, nb, n_mels);
    return v2w_launch_status();
}

// The arguments the two v2w_mel_loss launches share: 0, V2W_E_ARG or V2W_E_SHAPE
inline int mel_loss_args_ok(const void* spec, const void* basis, const void* tgt, int ts_f, int ts_m, int B, int Cs, int FP, int F, int Ft,
                            int nb, int n_mels, const int32_t* len, int len_mul, int hop, int n_fft) {
    if (const int rc = mel_finish_args_ok(spec, basis, tgt, B, Cs, FP, F, nb, n_mels)) return rc;
    if (Ft <= 0) return V2W_E_ARG;
    if ((long long)n_mels * Ft > 0x7fffffffll) return V2W_E_SHAPE;            // (the target's index within an item is an int product)
    if (!((ts_f == n_mels && ts_m == 1) || (ts_f == 1 && ts_m == Ft))) return V2W_E_ARG;      // dense, frames first or mels first
    if (!len) return Ft < F ? V2W_E_ARG : 0;
    return mel_len_args_ok(len, len_mul, hop, n_fft, F);
}

}  // namespace

// ---- the first entry points: y (B, L) -> xp (B, hop, FP); FP >= F + n_fft/hop - 1 frame columns (F = number of STFT frames),
// pad = (n_fft - hop)/2.  With per-item lengths (include/vec2wav_hip.h): len a device array of B int32, item b holds min(len[b] * len_mul, L)
// samples, and (2 pad) % hop == 0.  The backward takes the forward's arguments, dxp -> dy: the reflected samples fold back onto their sources.
extern "C" int v2w_mel_phases(const float* y, float* xp, int B, int L, int hop, int pad, int FP, void* stream) {
    return mel_phase_launch(y, xp, mel_first_geo(B, L, hop, pad, FP), false, nullptr, 1, false, stream);
}

extern "C" int v2w_mel_phases_bwd(const float* dxp, float* dy, int B, int L, int hop, int pad, int FP, void* stream) {
    return mel_phase_launch(dxp, dy, mel_first_geo(B, L, hop, pad, FP), false, nullptr, 1, true, stream);
}

extern "C" int v2w_mel_phases_len(const float* y, float* xp, int B, int L, int hop, int pad, int FP, const int32_t* len, int len_mul,
                                  void* stream) {
    if (hop > 0 && pad >= 0 && (2ll * pad) % hop) return V2W_E_ARG;
    return mel_phase_launch(y, xp, mel_first_geo(B, L, hop, pad, FP), true, len, len_mul, false, stream);
}

extern "C" int v2w_mel_phases_len_bwd(const float* dxp, float* dy, int B, int L, int hop, int pad, int FP, const int32_t* len, int len_mul,
                                      void* stream) {
    if (hop > 0 && pad >= 0 && (2ll * pad) % hop) return V2W_E_ARG;
    return mel_phase_launch(dxp, dy, mel_first_geo(B, L, hop, pad, FP), true, len, len_mul, true, stream);
}

// spec (B, Cs, FP) from the DFT conv (Cs >= 2*nb rows), basis (n_mels, nb) -> out (B, n_mels, F) = log(clamp(basis @ |spec|, 1e-5)), on the
// 16-frame block.  _len keeps its conditions on n_fft / hop.  _bwd: gout (B, n_mels, F) -> dspec (B, Cs, FP), which the caller zero-fills
// (pad rows / frames stay 0); basisT (nb, n_mels) is the transposed filterbank.
extern "C" int v2w_mel_finish(const float* spec, const float* basis, float* out, int B, int Cs, int FP, int F, int nb, int n_mels,
                              void* stream) {
    if (const int rc = mel_finish_args_ok(spec, basis, out, B, Cs, FP, F, nb, n_mels)) return rc;
    return mel_finish_launch(spec, basis, out, B, Cs, FP, F, nb, n_mels, nullptr, 1, 1, 1, true, stream);
}

extern "C" int v2w_mel_finish_len(const float* spec, const float* basis, float* out, int B, int Cs, int FP, int F, int nb, int n_mels,
                                  const int32_t* len, int len_mul, int hop, int n_fft, void* stream) {
    const int ra = mel_finish_args_ok(spec, basis, out, B, Cs, FP, F, nb, n_mels), rl = mel_len_args_ok(len, len_mul, hop, n_fft, F);
    if (ra == V2W_E_ARG || rl == V2W_E_ARG || n_fft % hop || (n_fft - hop) % 2) return V2W_E_ARG;     // (an argument before a shape)
    if (ra || rl) return V2W_E_SHAPE;
    return mel_finish_launch(spec, basis, out, B, Cs, FP, F, nb, n_mels, len, len_mul, hop, n_fft, true, stream);
}

extern "C" int v2w_mel_finish_bwd(const float* spec, const float* basis, const float* basisT, const float* gout, float* dspec,
                                  int B, int Cs, int FP, int F, int nb, int n_mels, void* stream) {
    return mel_finish_bwd_launch(spec, basis, basisT, gout, dspec, B, Cs, FP, F, nb, n_mels, true, stream);
}

// ---- any frame geometry (include/vec2wav_hip.h): y (B, L) -> xp (B, CP, FP), xp[b][p][f] = ypad[b][f*hop + left + p] for p < hop, else 0
extern "C" int v2w_mel_phases_geo(const float* y, float* xp, int B, int L, int n_fft, int win, int hop, int CP, int pad, int left, int k,
                                  int FP, void* stream) {
    return mel_phase_launch(y, xp, MelGeo{B, L, n_fft, win, hop, CP, pad, left, k, FP}, false, nullptr, 1, false, stream);
}

extern "C" int v2w_mel_phases_geo_len(const float* y, float* xp, int B, int L, int n_fft, int win, int hop, int CP, int pad, int left, int k,
                                      int FP, const int32_t* len, int len_mul, void* stream) {
    return mel_phase_launch(y, xp, MelGeo{B, L, n_fft, win, hop, CP, pad, left, k, FP}, true, len, len_mul, false, stream);
}

extern "C" int v2w_mel_phases_geo_bwd(const float* dxp, float* dy, int B, int L, int n_fft, int win, int hop, int CP, int pad, int left, int k,
                                      int FP, void* stream) {
    return mel_phase_launch(dxp, dy, MelGeo{B, L, n_fft, win, hop, CP, pad, left, k, FP}, false, nullptr, 1, true, stream);
}

extern "C" int v2w_mel_phases_geo_len_bwd(const float* dxp, float* dy, int B, int L, int n_fft, int win, int hop, int CP, int pad, int left,
                                          int k, int FP, const int32_t* len, int len_mul, void* stream) {
    return mel_phase_launch(dxp, dy, MelGeo{B, L, n_fft, win, hop, CP, pad, left, k, FP}, true, len, len_mul, true, stream);
}

// The finish calls for any nb whose 8-frame block fits 64 KiB of LDS: the 16-frame block (and its bits) wherever the first entry points
// take it.  _len drops their conditions on n_fft / hop: pad = (n_fft - hop) / 2 rounded down, as mel_spectrogram pads.
extern "C" int v2w_mel_finish_geo(const float* spec, const float* basis, float* out, int B, int Cs, int FP, int F, int nb, int n_mels,
                                  void* stream) {
    if (const int rc = mel_finish_args_ok(spec, basis, out, B, Cs, FP, F, nb, n_mels)) return rc;
    return mel_finish_launch(spec, basis, out, B, Cs, FP, F, nb, n_mels, nullptr, 1, 1, 1, false, stream);
}

extern "C" int v2w_mel_finish_geo_len(const float* spec, const float* basis, float* out, int B, int Cs, int FP, int F, int nb, int n_mels,
                                      const int32_t* len, int len_mul, int hop, int n_fft, void* stream) {
    if (const int rc = mel_finish_args_ok(spec, basis, out, B, Cs, FP, F, nb, n_mels)) return rc;
    if (const int rc = mel_len_args_ok(len, len_mul, hop, n_fft, F)) return rc;
    return mel_finish_launch(spec, basis, out, B, Cs, FP, F, nb, n_mels, len, len_mul, hop, n_fft, false, stream);
}

extern "C" int v2w_mel_finish_geo_bwd(const float* spec, const float* basis, const float* basisT, const float* gout, float* dspec,
                                      int B, int Cs, int FP, int F, int nb, int n_mels, void* stream) {
    return mel_finish_bwd_launch(spec, basis, basisT, gout, dspec, B, Cs, FP, F, nb, n_mels, false, stream);
}

// ---- the mel L1 training loss fused into the finish step (include/vec2wav_hip.h).  len == NULL: no lengths, the LEN = false kernels.
extern "C" int v2w_mel_loss_plan(int B, int F, int nb, int n_mels, long long* scratch_bytes) {
    if (B <= 0 || F <= 0 || nb <= 0 || n_mels <= 0) return V2W_E_ARG;
    const int ft = mel_ft(nb);
    if (!ft || B > 65535) return V2W_E_SHAPE;
    const int tiles = (F + ft - 1) / ft;
    if (scratch_bytes) *scratch_bytes = (long long)B * tiles * (long long)sizeof(double);
    return tiles;
}

extern "C" int v2w_mel_loss_fwd(const float* spec, const float* basis, const float* tgt, int ts_f, int ts_m,
                                int B, int Cs, int FP, int F, int Ft, int nb, int n_mels,
                                const int32_t* len, int len_mul, int hop, int n_fft, float scale,
                                float* per_item, float* total, float* coef, void* ws, void* stream) {
    if (const int rc = mel_loss_args_ok(spec, basis, tgt, ts_f, ts_m, B, Cs, FP, F, Ft, nb, n_mels, len, len_mul, hop, n_fft)) return rc;
    if (!ws || (reinterpret_cast<uintptr_t>(ws) & 7) || (!per_item && !total && !coef) || !(scale == scale)) return V2W_E_ARG;
    const int ft = mel_ft(nb);
    if (!ft) return V2W_E_SHAPE;
    const int tiles = (F + ft - 1) / ft;
    size_t lds = (size_t)nb * ft * sizeof(float);
    if (lds < 16 * sizeof(double)) lds = 16 * sizeof(double);                  // (the reduction's doubles live there too)
    hipStream_t st = (hipStream_t)stream;
    double* part = static_cast<double*>(ws);
    mel_dispatch(ft, len != nullptr, [&](auto FT, auto LEN) {
        V2W_LAUNCH((mel_loss_fwd_kernel<decltype(FT)::value, decltype(LEN)::value>), dim3(tiles, B), dim3(256), lds, st, spec, basis, tgt,
                   ts_f, ts_m, len, len_mul, hop, n_fft, Cs, FP, F, Ft, nb, n_mels, part);
    });
    V2W_LAUNCH(mel_loss_finish_kernel, dim3(1), dim3(256), 0, st, part, len, len_mul, hop, n_fft, B, n_mels, F, Ft, tiles, scale,
               per_item, total, coef);
    return v2w_launch_status();
}

extern "C" int v2w_mel_loss_bwd(const float* spec, const float* basis, const float* basisT, const float* tgt, int ts_f, int ts_m,
                                const float* gout, const float* coef, float* dspec,
                                int B, int Cs, int FP, int F, int Ft, int nb, int n_mels,
                                const int32_t* len, int len_mul, int hop, int n_fft, void* stream) {
    if (!basisT || !gout || !coef || !dspec) return V2W_E_ARG;
    if (const int rc = mel_loss_args_ok(spec, basis, tgt, ts_f, ts_m, B, Cs, FP, F, Ft, nb, n_mels, len, len_mul, hop, n_fft)) return rc;
    const int ft = mel_ft((long long)nb + n_mels);
    if (!ft) return V2W_E_SHAPE;
    mel_dispatch(ft, len != nullptr, [&](auto FT, auto LEN) {
        V2W_LAUNCH((mel_loss_bwd_kernel<decltype(FT)::value, decltype(LEN)::value>), dim3((F + ft - 1) / ft, B), dim3(256),
                   (size_t)(nb + n_mels) * ft * sizeof(float), (hipStream_t)stream, spec, basis, basisT, tgt, ts_f, ts_m, gout, coef,
                   len, len_mul, hop, n_fft, dspec, Cs, FP, F, Ft, nb, n_mels);
    });
    return v2w_launch_status();
}
