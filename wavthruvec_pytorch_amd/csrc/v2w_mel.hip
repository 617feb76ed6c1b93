// mel_spectrogram of the generated audio on the device (reference: vec2wav/dataset.py:53-77,
// called on the generator output in train.py:172-174, 266-269, 282-284):
//   reflect pad (n_fft - hop)/2  ->  STFT (hann window, center=False, onesided)  ->  sqrt(re^2 + im^2 + 1e-9)
//   ->  mel filterbank  ->  log(clamp(., 1e-5))
// The STFT is a dense contraction: with the padded signal de-interleaved by hop phase, Xp[b][p][f] = ypad[b][f*hop + p], frame f
// of the windowed DFT is  S[c][f] = sum_{j < n_fft/hop} sum_{p < hop} Wd[c][j*hop + p] * Xp[b][p][f + j]  - a Conv1d with hop
// input channels, n_fft/hop taps (pad_left = 0) and 2*(n_fft/2+1) output channels (cos rows, then -sin rows, window folded in):
// it runs on the f32 MFMA tile kernel through v2w_conv1d_fwd.  This file holds the two memory-bound ends.
#include "v2w_common.h"

namespace {

// Xp (B, hop, FP): Xp[b][p][f] = ypad[b][f*hop + p],  ypad = reflect-padded y (pad samples per side), 0 past the padded signal
__global__ void __launch_bounds__(256)
mel_phase_kernel(const float* __restrict__ y, float* __restrict__ xp, int L, int hop, int pad, int FP) {
    const int b = blockIdx.y;
    const int Lp = L + 2 * pad;
    for (int idx = blockIdx.x * 256 + threadIdx.x; idx < hop * FP; idx += gridDim.x * 256) {
        const int p = idx / FP, f = idx - p * FP;
        const int i = f * hop + p;
        float v = 0.f;
        if (i < Lp) {
            int s = i - pad;
            s = s < 0 ? -s : (s >= L ? 2 * (L - 1) - s : s);     // torch 'reflect': no edge repeat
            v = y[(size_t)b * L + s];
        }
        xp[((size_t)b * hop + p) * FP + f] = v;
    }
}

// spec (B, Cs, FP): rows [0, nb) = Re, rows [nb, 2nb) = Im of the nb = n_fft/2+1 bins.  One block = 16 frames of one batch item:
// magnitudes into LDS, then the 16 x n_mels outputs (each a dot over the bins with the dense filterbank row).
#define V2W_MEL_FT 16
__global__ void __launch_bounds__(256)
mel_finish_kernel(const float* __restrict__ spec, const float* __restrict__ basis, float* __restrict__ out,
                  int Cs, int FP, int F, int nb, int n_mels) {
    extern __shared__ float mag[];                     // [nb][V2W_MEL_FT]
    const int b = blockIdx.y, f0 = blockIdx.x * V2W_MEL_FT;
    const float* sb = spec + (size_t)b * Cs * FP;
    for (int idx = threadIdx.x; idx < nb * V2W_MEL_FT; idx += 256) {
        const int c = idx / V2W_MEL_FT, ff = idx - c * V2W_MEL_FT;
        const int f = f0 + ff;
        float m = 0.f;
        if (f < F) {
            const float re = sb[(size_t)c * FP + f], im = sb[(size_t)(nb + c) * FP + f];
            m = sqrtf(re * re + im * im + 1e-9f);
        }
        mag[idx] = m;
    }
    __syncthreads();
    for (int idx = threadIdx.x; idx < n_mels * V2W_MEL_FT; idx += 256) {
        const int m = idx / V2W_MEL_FT, ff = idx - m * V2W_MEL_FT;
        const int f = f0 + ff;
        if (f >= F) continue;
        const float* br = basis + (size_t)m * nb;
        float acc = 0.f;
        for (int c = 0; c < nb; ++c) acc = fmaf(br[c], mag[c * V2W_MEL_FT + ff], acc);
        out[((size_t)b * n_mels + m) * F + f] = logf(fmaxf(acc, 1e-5f));
    }
}

// Backward of mel_finish_kernel for the same 16-frame block: with acc = basis @ mag,
//   d_acc = g / acc where acc >= 1e-5 (the clamp passes the gradient on its closed side), d_mag = basis^T @ d_acc,
//   d_re = d_mag * re / mag, d_im = d_mag * im / mag      (mag = sqrt(re^2 + im^2 + 1e-9) > 0)
// basisT is the (nb, n_mels) transpose so phase 3 reads rows.  dspec must be zero-filled: only rows < 2*nb, frames < F are written.
__global__ void __launch_bounds__(256)
mel_finish_bwd_kernel(const float* __restrict__ spec, const float* __restrict__ basis, const float* __restrict__ basisT,
                      const float* __restrict__ gout, float* __restrict__ dspec, int Cs, int FP, int F, int nb, int n_mels) {
    extern __shared__ float mag[];                     // [nb][FT] then d_acc [n_mels][FT]
    float* dacc = mag + (size_t)nb * V2W_MEL_FT;
    const int b = blockIdx.y, f0 = blockIdx.x * V2W_MEL_FT;
    const float* sb = spec + (size_t)b * Cs * FP;
    float* db = dspec + (size_t)b * Cs * FP;
    for (int idx = threadIdx.x; idx < nb * V2W_MEL_FT; idx += 256) {
        const int c = idx / V2W_MEL_FT, f = f0 + idx % V2W_MEL_FT;
        float m = 1.f;
        if (f < F) {
            const float re = sb[(size_t)c * FP + f], im = sb[(size_t)(nb + c) * FP + f];
            m = sqrtf(re * re + im * im + 1e-9f);
        }
        mag[idx] = m;
    }
    __syncthreads();
    for (int idx = threadIdx.x; idx < n_mels * V2W_MEL_FT; idx += 256) {
        const int m = idx / V2W_MEL_FT, ff = idx - m * V2W_MEL_FT;
        const int f = f0 + ff;
        float d = 0.f;
        if (f < F) {
            const float* br = basis + (size_t)m * nb;
            float acc = 0.f;
            for (int c = 0; c < nb; ++c) acc = fmaf(br[c], mag[c * V2W_MEL_FT + ff], acc);
            if (acc >= 1e-5f) d = gout[((size_t)b * n_mels + m) * F + f] / acc;
        }
        dacc[idx] = d;
    }
    __syncthreads();
    for (int idx = threadIdx.x; idx < nb * V2W_MEL_FT; idx += 256) {
        const int c = idx / V2W_MEL_FT, ff = idx - c * V2W_MEL_FT;
        const int f = f0 + ff;
        if (f >= F) continue;
        const float* bt = basisT + (size_t)c * n_mels;
        float dm = 0.f;
        for (int m = 0; m < n_mels; ++m) dm = fmaf(bt[m], dacc[m * V2W_MEL_FT + ff], dm);
        const float s = dm / mag[idx];
        db[(size_t)c * FP + f] = s * sb[(size_t)c * FP + f];
        db[(size_t)(nb + c) * FP + f] = s * sb[(size_t)(nb + c) * FP + f];
    }
}

// Backward of mel_phase_kernel: dy[b][s] = sum of dxp over the padded positions i that read y[s]: i = s + pad always, the
// left reflection i = pad - s for 1 <= s <= pad, the right reflection i = 2(L-1) - s + pad for L-1-pad <= s <= L-2.
__global__ void __launch_bounds__(256)
mel_phase_bwd_kernel(const float* __restrict__ dxp, float* __restrict__ dy, int L, int hop, int pad, int FP) {
    const int b = blockIdx.y;
    const float* xb = dxp + (size_t)b * hop * FP;
    auto at = [&](int i) { return i / hop < FP ? xb[(size_t)(i % hop) * FP + i / hop] : 0.f; };    // samples past the last frame: unused
    for (int s = blockIdx.x * 256 + threadIdx.x; s < L; s += gridDim.x * 256) {
        float v = at(s + pad);
        if (s >= 1 && s <= pad) v += at(pad - s);
        if (s >= L - 1 - pad && s <= L - 2) v += at(2 * (L - 1) - s + pad);
        dy[(size_t)b * L + s] = v;
    }
}

// ---- batches of unequal lengths: item b holds Lb = min(len[b] * len_mul, L) samples
__device__ __forceinline__ int mel_item_samples(const int32_t* __restrict__ len, int b, int len_mul, int L) {
    const long long n = (long long)len[b] * len_mul;
    return n < 0 ? 0 : (n > L ? L : (int)n);
}
// frames of an item of Lb samples: reflect padding needs Lb > pad, one frame needs Lb + 2 pad >= n_fft
__device__ __forceinline__ int mel_item_frames(int Lb, int hop, int pad, int n_fft) {
    return (Lb > pad && Lb + 2 * pad >= n_fft) ? (Lb + 2 * pad - n_fft) / hop + 1 : 0;
}

// mel_phase_kernel with the reflection about the item's own last sample; 0 from column roundup4(F_b + k - 1) on (the FP of the item's own
// B = 1 call; no frame of the item reads further) and past the padded item.  Every load index s satisfies 0 <= s < Lb.
__global__ void __launch_bounds__(256)
mel_phase_len_kernel(const float* __restrict__ y, float* __restrict__ xp, const int32_t* __restrict__ len, int len_mul,
                     int L, int hop, int pad, int FP) {
    const int b = blockIdx.y;
    const int Lb = mel_item_samples(len, b, len_mul, L);
    const int n_fft = 2 * pad + hop;
    const int Fb = mel_item_frames(Lb, hop, pad, n_fft);
    const int Lp = Fb > 0 ? Lb + 2 * pad : 0;
    const int FPb = Fb > 0 ? (Fb + n_fft / hop - 1 + 3) / 4 * 4 : 0;
    for (int idx = blockIdx.x * 256 + threadIdx.x; idx < hop * FP; idx += gridDim.x * 256) {
        const int p = idx / FP, f = idx - p * FP;
        const int i = f * hop + p;
        float v = 0.f;
        if (f < FPb && i < Lp) {
            int s = i - pad;
            s = s < 0 ? -s : (s >= Lb ? 2 * (Lb - 1) - s : s);   // -s <= pad < Lb;  2(Lb-1) - s >= Lb - 1 - pad >= 0
            v = y[(size_t)b * L + s];
        }
        xp[((size_t)b * hop + p) * FP + f] = v;
    }
}

// mel_finish_kernel for the first Fb frames of item b (the same operations in the same order); 0.0 in the frames [Fb, F)
__global__ void __launch_bounds__(256)
mel_finish_len_kernel(const float* __restrict__ spec, const float* __restrict__ basis, float* __restrict__ out,
                      const int32_t* __restrict__ len, int len_mul, int hop, int n_fft,
                      int Cs, int FP, int F, int nb, int n_mels) {
    extern __shared__ float mag[];                     // [nb][V2W_MEL_FT]
    const int b = blockIdx.y, f0 = blockIdx.x * V2W_MEL_FT;
    const int pad = (n_fft - hop) / 2;
    const long long n = (long long)len[b] * len_mul;
    const long long nmax = (long long)F * hop + n_fft;                      // (more samples than F frames need)
    int Fb = mel_item_frames((int)(n < 0 ? 0 : (n > nmax ? nmax : n)), hop, pad, n_fft);
    Fb = Fb < F ? Fb : F;
    if (f0 >= Fb) {                                    // (uniform over the workgroup) nothing of the item here: zeros, spec unread
        for (int idx = threadIdx.x; idx < n_mels * V2W_MEL_FT; idx += 256) {
            const int m = idx / V2W_MEL_FT, f = f0 + idx % V2W_MEL_FT;
            if (f < F) out[((size_t)b * n_mels + m) * F + f] = 0.f;
        }
        return;
    }
    const float* sb = spec + (size_t)b * Cs * FP;
    for (int idx = threadIdx.x; idx < nb * V2W_MEL_FT; idx += 256) {
        const int c = idx / V2W_MEL_FT, ff = idx - c * V2W_MEL_FT;
        const int f = f0 + ff;
        float m = 0.f;
        if (f < Fb) {
            const float re = sb[(size_t)c * FP + f], im = sb[(size_t)(nb + c) * FP + f];
            m = sqrtf(re * re + im * im + 1e-9f);
        }
        mag[idx] = m;
    }
    __syncthreads();
    for (int idx = threadIdx.x; idx < n_mels * V2W_MEL_FT; idx += 256) {
        const int m = idx / V2W_MEL_FT, ff = idx - m * V2W_MEL_FT;
        const int f = f0 + ff;
        if (f >= F) continue;
        float v = 0.f;
        if (f < Fb) {
            const float* br = basis + (size_t)m * nb;
            float acc = 0.f;
            for (int c = 0; c < nb; ++c) acc = fmaf(br[c], mag[c * V2W_MEL_FT + ff], acc);
            v = logf(fmaxf(acc, 1e-5f));
        }
        out[((size_t)b * n_mels + m) * F + f] = v;
    }
}

// What the index arithmetic of the phase kernels holds in `int`: hop * FP (the flat index of xp) and L + 2 * pad (the padded length; the
// reflected indices 2 (L - 1) - s + pad stay below it).  Past 2^31 - 1 the launch would wrap them: V2W_E_SHAPE, nothing is launched.
inline bool mel_phase_ints_fit(int L, int hop, int pad, int FP) {
    return (long long)hop * FP <= 0x7fffffffll && (long long)L + 2ll * pad <= 0x7fffffffll;
}

// ---- any STFT frame geometry (win <= n_fft, 1 <= hop <= n_fft; include/vec2wav_hip.h, "any frame geometry").  Frame f multiplies the
// window's support only, ypad[f*hop + left + t] for t < win, so with Xg[b][p][f] = ypad[b][f*hop + left + p] (p < hop) the DFT conv has
// k = ceil(win / hop) taps over CP >= hop input channels; the channels [hop, CP) are zeros (the tile kernel's channel blocks).  Nothing
// here is derived from anything else: hop, CP, pad, left, k, n_fft are the caller's (v2w_mel_geo_ok checks them on the host).

// LEN: the reflection about the item's own last sample, 0 from column roundup4(F_b + k - 1) on; every load index s satisfies 0 <= s < Lb
template <bool LEN>
__global__ void __launch_bounds__(256)
mel_phase_geo_kernel(const float* __restrict__ y, float* __restrict__ xp, const int32_t* __restrict__ len, int len_mul,
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

// Backward of mel_phase_geo_kernel<false>: the padded position i is Xg[(i - left) % hop][(i - left) / hop] where 0 <= i - left < hop * FP,
// and is read by nothing elsewhere.  The sample itself, then the left reflection, then the right one, as mel_phase_bwd_kernel adds them.
__global__ void __launch_bounds__(256)
mel_phase_geo_bwd_kernel(const float* __restrict__ dxp, float* __restrict__ dy, int L, int hop, int CP, int pad, int left, int FP) {
    const int b = blockIdx.y;
    const float* xb = dxp + (size_t)b * CP * FP;
    auto at = [&](int i) {
        const int q = i - left;
        return (q >= 0 && q / hop < FP) ? xb[(size_t)(q % hop) * FP + q / hop] : 0.f;
    };
    for (int s = blockIdx.x * 256 + threadIdx.x; s < L; s += gridDim.x * 256) {
        float v = at(s + pad);
        if (s >= 1 && s <= pad) v += at(pad - s);
        if (s >= L - 1 - pad && s <= L - 2) v += at(2 * (L - 1) - s + pad);
        dy[(size_t)b * L + s] = v;
    }
}

// mel_finish_kernel / mel_finish_len_kernel on 8 frames per workgroup, for the bin counts whose 16-frame block passes 64 KiB of LDS
// (nb = 1025: n_fft 2048).  Every output is the same chain of operations in the same order: fmaf over the bins c = 0 .. nb - 1.
#define V2W_MEL_FT8 8
template <bool LEN>
__global__ void __launch_bounds__(256)
mel_finish8_kernel(const float* __restrict__ spec, const float* __restrict__ basis, float* __restrict__ out,
                   const int32_t* __restrict__ len, int len_mul, int hop, int n_fft, int Cs, int FP, int F, int nb, int n_mels) {
    extern __shared__ float mag[];                     // [nb][V2W_MEL_FT8]
    const int b = blockIdx.y, f0 = blockIdx.x * V2W_MEL_FT8;
    int Fb = F;
    if (LEN) {
        const int pad = (n_fft - hop) / 2;
        const long long n = (long long)len[b] * len_mul;
        const long long nmax = (long long)F * hop + n_fft;
        Fb = mel_item_frames((int)(n < 0 ? 0 : (n > nmax ? nmax : n)), hop, pad, n_fft);
        Fb = Fb < F ? Fb : F;
        if (f0 >= Fb) {                                // (uniform over the workgroup) zeros, spec unread
            for (int idx = threadIdx.x; idx < n_mels * V2W_MEL_FT8; idx += 256) {
                const int m = idx / V2W_MEL_FT8, f = f0 + idx % V2W_MEL_FT8;
                if (f < F) out[((size_t)b * n_mels + m) * F + f] = 0.f;
            }
            return;
        }
    }
    const float* sb = spec + (size_t)b * Cs * FP;
    for (int idx = threadIdx.x; idx < nb * V2W_MEL_FT8; idx += 256) {
        const int c = idx / V2W_MEL_FT8, f = f0 + idx % V2W_MEL_FT8;
        float m = 0.f;
        if (f < Fb) {
            const float re = sb[(size_t)c * FP + f], im = sb[(size_t)(nb + c) * FP + f];
            m = sqrtf(re * re + im * im + 1e-9f);
        }
        mag[idx] = m;
    }
    __syncthreads();
    for (int idx = threadIdx.x; idx < n_mels * V2W_MEL_FT8; idx += 256) {
        const int m = idx / V2W_MEL_FT8, ff = idx - m * V2W_MEL_FT8;
        const int f = f0 + ff;
        if (f >= F) continue;
        float v = 0.f;
        if (f < Fb) {
            const float* br = basis + (size_t)m * nb;
            float acc = 0.f;
            for (int c = 0; c < nb; ++c) acc = fmaf(br[c], mag[c * V2W_MEL_FT8 + ff], acc);
            v = logf(fmaxf(acc, 1e-5f));
        }
        out[((size_t)b * n_mels + m) * F + f] = v;
    }
}

// mel_finish_bwd_kernel on 8 frames per workgroup
__global__ void __launch_bounds__(256)
mel_finish8_bwd_kernel(const float* __restrict__ spec, const float* __restrict__ basis, const float* __restrict__ basisT,
                       const float* __restrict__ gout, float* __restrict__ dspec, int Cs, int FP, int F, int nb, int n_mels) {
    extern __shared__ float mag[];                     // [nb][FT8] then d_acc [n_mels][FT8]
    float* dacc = mag + (size_t)nb * V2W_MEL_FT8;
    const int b = blockIdx.y, f0 = blockIdx.x * V2W_MEL_FT8;
    const float* sb = spec + (size_t)b * Cs * FP;
    float* db = dspec + (size_t)b * Cs * FP;
    for (int idx = threadIdx.x; idx < nb * V2W_MEL_FT8; idx += 256) {
        const int c = idx / V2W_MEL_FT8, f = f0 + idx % V2W_MEL_FT8;
        float m = 1.f;
        if (f < F) {
            const float re = sb[(size_t)c * FP + f], im = sb[(size_t)(nb + c) * FP + f];
            m = sqrtf(re * re + im * im + 1e-9f);
        }
        mag[idx] = m;
    }
    __syncthreads();
    for (int idx = threadIdx.x; idx < n_mels * V2W_MEL_FT8; idx += 256) {
        const int m = idx / V2W_MEL_FT8, ff = idx - m * V2W_MEL_FT8;
        const int f = f0 + ff;
        float d = 0.f;
        if (f < F) {
            const float* br = basis + (size_t)m * nb;
            float acc = 0.f;
            for (int c = 0; c < nb; ++c) acc = fmaf(br[c], mag[c * V2W_MEL_FT8 + ff], acc);
            if (acc >= 1e-5f) d = gout[((size_t)b * n_mels + m) * F + f] / acc;
        }
        dacc[idx] = d;
    }
    __syncthreads();
    for (int idx = threadIdx.x; idx < nb * V2W_MEL_FT8; idx += 256) {
        const int c = idx / V2W_MEL_FT8, ff = idx - c * V2W_MEL_FT8;
        const int f = f0 + ff;
        if (f >= F) continue;
        const float* bt = basisT + (size_t)c * n_mels;
        float dm = 0.f;
        for (int m = 0; m < n_mels; ++m) dm = fmaf(bt[m], dacc[m * V2W_MEL_FT8 + ff], dm);
        const float s = dm / mag[idx];
        db[(size_t)c * FP + f] = s * sb[(size_t)c * FP + f];
        db[(size_t)(nb + c) * FP + f] = s * sb[(size_t)(nb + c) * FP + f];
    }
}

// The geometry of the three v2w_mel_phases_geo* calls: 0, V2W_E_ARG or V2W_E_SHAPE (the kernels' int arithmetic: CP * FP, the padded
// position (FP - 1) * hop + left + hop - 1 and L + 2 * pad)
inline int mel_geo_ok(int B, int L, int n_fft, int win, int hop, int CP, int pad, int left, int k, int FP) {
    if (B <= 0 || L <= 1 || hop < 1 || n_fft < hop || win < 1 || win > n_fft || CP < hop || pad < 0 || pad >= L || left < 0 ||
        left > n_fft - win || k < 1 || (long long)k * hop < win || FP <= 0) return V2W_E_ARG;
    if (B > 65535) return V2W_E_SHAPE;                        // (grid.y)
    if ((long long)CP * FP > 0x7fffffffll || (long long)hop * FP + left > 0x7fffffffll || (long long)L + 2ll * pad > 0x7fffffffll)
        return V2W_E_SHAPE;
    return 0;
}

inline int mel_finish_args_ok(const void* spec, const void* basis, const void* out, int B, int Cs, int FP, int F, int nb, int n_mels) {
    if (!spec || !basis || !out || B <= 0 || F <= 0 || FP < F || nb <= 0 || Cs < 2 * nb || n_mels <= 0) return V2W_E_ARG;
    if ((long long)n_mels * V2W_MEL_FT > 0x7fffffffll || B > 65535) return V2W_E_SHAPE;
    return 0;
}

// ---- the mel L1 training loss, fused into the finish kernels (include/vec2wav_hip.h, "Fused mel L1 training loss").  The target is dense,
// (B, Ft, n_mels) or (B, n_mels, Ft), read through its frame and mel strides.  Item b counts Fb = min(its own frames, F, Ft) frames; without
// lengths Fb = F (the host checks Ft >= F).  Every select below is on f < Fb: nothing at or past Fb, of spec or of the target, is loaded.
template <bool LEN>
__device__ __forceinline__ int mel_loss_frames(const int32_t* __restrict__ len, int b, int len_mul, int hop, int n_fft, int F, int Ft) {
    if (!LEN) return F;
    const long long n = (long long)len[b] * len_mul;
    const long long nmax = (long long)F * hop + n_fft;                      // (more samples than F frames need)
    int Fb = mel_item_frames((int)(n < 0 ? 0 : (n > nmax ? nmax : n)), hop, (n_fft - hop) / 2, n_fft);
    Fb = Fb < F ? Fb : F;
    return Fb < Ft ? Fb : Ft;
}

// mel_finish_kernel / mel_finish8_kernel (FT = 16 / 8 frames per workgroup) up to v = logf(fmaxf(acc, 1e-5f)), the same operations in the
// same order; in place of the store, |v - t| (one fp32 rounding) is added in fp64: a thread's entries in index order, then the workgroup's
// fixed-order reduction, to ONE partial part[b * gridDim.x + blockIdx.x].  A workgroup whose frames all lie at or past Fb writes 0.0 and
// reads nothing.  The reduction's 16 doubles reuse the magnitudes' LDS (v2w_block_sum syncs before it writes them).
template <int FT, bool LEN>
__global__ void __launch_bounds__(256)
mel_loss_fwd_kernel(const float* __restrict__ spec, const float* __restrict__ basis, const float* __restrict__ tgt, int ts_f, int ts_m,
                    const int32_t* __restrict__ len, int len_mul, int hop, int n_fft, int Cs, int FP, int F, int Ft, int nb, int n_mels,
                    double* __restrict__ part) {
    extern __shared__ __align__(8) float mag[];        // [nb][FT], at least 16 doubles
    const int b = blockIdx.y, f0 = blockIdx.x * FT;
    const int Fb = mel_loss_frames<LEN>(len, b, len_mul, hop, n_fft, F, Ft);
    double* po = part + (size_t)b * gridDim.x + blockIdx.x;
    if (f0 >= Fb) {                                    // (uniform over the workgroup)
        if (threadIdx.x == 0) *po = 0.0;
        return;
    }
    const float* sb = spec + (size_t)b * Cs * FP;
    for (int idx = threadIdx.x; idx < nb * FT; idx += 256) {
        const int c = idx / FT, f = f0 + idx % FT;
        float m = 0.f;
        if (f < Fb) {
            const float re = sb[(size_t)c * FP + f], im = sb[(size_t)(nb + c) * FP + f];
            m = sqrtf(re * re + im * im + 1e-9f);
        }
        mag[idx] = m;
    }
    __syncthreads();
    const float* tb = tgt + (size_t)b * n_mels * Ft;
    double sum = 0.0;
    for (int idx = threadIdx.x; idx < n_mels * FT; idx += 256) {
        const int m = idx / FT, ff = idx - m * FT;
        const int f = f0 + ff;
        if (f >= Fb) continue;
        const float* br = basis + (size_t)m * nb;
        float acc = 0.f;
        for (int c = 0; c < nb; ++c) acc = fmaf(br[c], mag[c * FT + ff], acc);
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
        const int Fb = len ? mel_loss_frames<true>(len, b, len_mul, hop, n_fft, F, Ft) : F;
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

// mel_finish_bwd_kernel / mel_finish8_bwd_kernel with d_acc = (gout * coef) * sgn(v - t) / acc where f < Fb and acc >= 1e-5f, else 0
// (sgn(0) = 0; on the closed side of the clamp v = logf(acc)).  gout and coef are one device float each.  dspec is zero-filled by the
// caller: only rows < 2 * nb of the frames < Fb are written, and a workgroup at or past Fb reads nothing.
template <int FT, bool LEN>
__global__ void __launch_bounds__(256)
mel_loss_bwd_kernel(const float* __restrict__ spec, const float* __restrict__ basis, const float* __restrict__ basisT,
                    const float* __restrict__ tgt, int ts_f, int ts_m, const float* __restrict__ gout, const float* __restrict__ coef,
                    const int32_t* __restrict__ len, int len_mul, int hop, int n_fft, float* __restrict__ dspec,
                    int Cs, int FP, int F, int Ft, int nb, int n_mels) {
    extern __shared__ float mag[];                     // [nb][FT] then d_acc [n_mels][FT]
    float* dacc = mag + (size_t)nb * FT;
    const int b = blockIdx.y, f0 = blockIdx.x * FT;
    const int Fb = mel_loss_frames<LEN>(len, b, len_mul, hop, n_fft, F, Ft);
    if (f0 >= Fb) return;                              // (uniform over the workgroup)
    const float gc = gout[0] * coef[0];
    const float* sb = spec + (size_t)b * Cs * FP;
    const float* tb = tgt + (size_t)b * n_mels * Ft;
    float* db = dspec + (size_t)b * Cs * FP;
    for (int idx = threadIdx.x; idx < nb * FT; idx += 256) {
        const int c = idx / FT, f = f0 + idx % FT;
        float m = 1.f;
        if (f < Fb) {
            const float re = sb[(size_t)c * FP + f], im = sb[(size_t)(nb + c) * FP + f];
            m = sqrtf(re * re + im * im + 1e-9f);
        }
        mag[idx] = m;
    }
    __syncthreads();
    for (int idx = threadIdx.x; idx < n_mels * FT; idx += 256) {
        const int m = idx / FT, ff = idx - m * FT;
        const int f = f0 + ff;
        float d = 0.f;
        if (f < Fb) {
            const float* br = basis + (size_t)m * nb;
            float acc = 0.f;
            for (int c = 0; c < nb; ++c) acc = fmaf(br[c], mag[c * FT + ff], acc);
            if (acc >= 1e-5f) {
                const float v = logf(fmaxf(acc, 1e-5f)), t = tb[(size_t)f * ts_f + (size_t)m * ts_m];
                const float g = v > t ? gc : (v < t ? -gc : 0.f);
                d = g / acc;
            }
        }
        dacc[idx] = d;
    }
    __syncthreads();
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

// mel_phase_bwd_kernel for an item of Lb samples: the right reflection about ITS last sample, the columns from its own
// FPb = roundup4(Fb + k - 1) on read as 0 (whatever they hold), dy[b, Lb:] = +0.0; an item without a frame is all +0.0.  The sample, its left
// reflection, its right reflection, in that order: the bits of the B = 1 mel_phase_bwd_kernel on dxp[b, :, :FPb].
__global__ void __launch_bounds__(256)
mel_phase_len_bwd_kernel(const float* __restrict__ dxp, float* __restrict__ dy, const int32_t* __restrict__ len, int len_mul,
                         int L, int hop, int pad, int FP) {
    const int b = blockIdx.y;
    const int Lb = mel_item_samples(len, b, len_mul, L);
    const int n_fft = 2 * pad + hop;
    const int Fb = mel_item_frames(Lb, hop, pad, n_fft);
    int FPb = Fb > 0 ? (Fb + n_fft / hop - 1 + 3) / 4 * 4 : 0;
    FPb = FPb < FP ? FPb : FP;
    const float* xb = dxp + (size_t)b * hop * FP;
    auto at = [&](int i) { return i / hop < FPb ? xb[(size_t)(i % hop) * FP + i / hop] : 0.f; };
    for (int s = blockIdx.x * 256 + threadIdx.x; s < L; s += gridDim.x * 256) {
        float v = 0.f;
        if (s < Lb && Fb > 0) {
            v = at(s + pad);
            if (s >= 1 && s <= pad) v += at(pad - s);
            if (s >= Lb - 1 - pad && s <= Lb - 2) v += at(2 * (Lb - 1) - s + pad);
        }
        dy[(size_t)b * L + s] = v;
    }
}

// mel_phase_geo_bwd_kernel in the same per-item form
__global__ void __launch_bounds__(256)
mel_phase_geo_len_bwd_kernel(const float* __restrict__ dxp, float* __restrict__ dy, const int32_t* __restrict__ len, int len_mul,
                             int L, int hop, int CP, int pad, int left, int k, int n_fft, int FP) {
    const int b = blockIdx.y;
    const int Lb = mel_item_samples(len, b, len_mul, L);
    const int Fb = mel_item_frames(Lb, hop, pad, n_fft);
    int FPb = Fb > 0 ? (Fb + k - 1 + 3) / 4 * 4 : 0;
    FPb = FPb < FP ? FPb : FP;
    const float* xb = dxp + (size_t)b * CP * FP;
    auto at = [&](int i) {
        const int q = i - left;
        return (q >= 0 && q / hop < FPb) ? xb[(size_t)(q % hop) * FP + q / hop] : 0.f;
    };
    for (int s = blockIdx.x * 256 + threadIdx.x; s < L; s += gridDim.x * 256) {
        float v = 0.f;
        if (s < Lb && Fb > 0) {
            v = at(s + pad);
            if (s >= 1 && s <= pad) v += at(pad - s);
            if (s >= Lb - 1 - pad && s <= Lb - 2) v += at(2 * (Lb - 1) - s + pad);
        }
        dy[(size_t)b * L + s] = v;
    }
}

// The arguments the two v2w_mel_loss launches share: 0, V2W_E_ARG or V2W_E_SHAPE
inline int mel_loss_args_ok(const void* spec, const void* basis, const void* tgt, int ts_f, int ts_m, int B, int Cs, int FP, int F, int Ft,
                            int nb, int n_mels, const int32_t* len, int len_mul, int hop, int n_fft) {
    if (const int rc = mel_finish_args_ok(spec, basis, tgt, B, Cs, FP, F, nb, n_mels)) return rc;
    if (Ft <= 0) return V2W_E_ARG;
    if ((long long)n_mels * Ft > 0x7fffffffll) return V2W_E_SHAPE;            // (the target's index within an item is an int product)
    if (!((ts_f == n_mels && ts_m == 1) || (ts_f == 1 && ts_m == Ft))) return V2W_E_ARG;      // dense, frames first or mels first
    if (!len) return Ft < F ? V2W_E_ARG : 0;
    if (len_mul < 1 || hop < 1 || n_fft < hop) return V2W_E_ARG;
    if ((long long)F * hop + n_fft > 0x7fffffffll) return V2W_E_SHAPE;         // (the kernel's sample count of F frames is an int)
    return 0;
}

// frames per workgroup of the fused forward: 16 where v2w_mel_finish fits them into 64 KiB of LDS, else 8; 0: not even 8
inline int mel_loss_fwd_ft(int nb) {
    return (size_t)nb * V2W_MEL_FT * sizeof(float) <= 64 * 1024 ? V2W_MEL_FT : ((size_t)nb * V2W_MEL_FT8 * sizeof(float) <= 64 * 1024 ? V2W_MEL_FT8 : 0);
}

}  // namespace

// y (B, L) -> xp (B, hop, FP); FP >= F + n_fft/hop - 1 frames columns (F = number of STFT frames), pad = (n_fft - hop)/2.
extern "C" int v2w_mel_phases(const float* y, float* xp, int B, int L, int hop, int pad, int FP, void* stream) {
    if (!y || !xp || B <= 0 || L <= 1 || hop <= 0 || pad < 0 || pad >= L || FP <= 0) return V2W_E_ARG;
    if (!mel_phase_ints_fit(L, hop, pad, FP)) return V2W_E_SHAPE;
    int gx = (int)(((long long)hop * FP + 255) / 256); if (gx > 1024) gx = 1024;
    V2W_LAUNCH(mel_phase_kernel, dim3(gx, B), dim3(256), 0, (hipStream_t)stream, y, xp, L, hop, pad, FP);
    return v2w_launch_status();
}

// spec (B, Cs, FP) from the DFT conv (Cs >= 2*nb rows), basis (n_mels, nb) -> out (B, n_mels, F) = log(clamp(basis @ |spec|, 1e-5))
extern "C" int v2w_mel_finish(const float* spec, const float* basis, float* out, int B, int Cs, int FP, int F, int nb, int n_mels,
                              void* stream) {
    if (!spec || !basis || !out || B <= 0 || F <= 0 || FP < F || nb <= 0 || Cs < 2 * nb || n_mels <= 0) return V2W_E_ARG;
    const size_t lds = (size_t)nb * V2W_MEL_FT * sizeof(float);
    if (lds > 64 * 1024 || (long long)n_mels * V2W_MEL_FT > 0x7fffffffll) return V2W_E_SHAPE;      // (the kernel's n_mels * 16 is an int)
    V2W_LAUNCH(mel_finish_kernel, dim3((F + V2W_MEL_FT - 1) / V2W_MEL_FT, B), dim3(256), lds, (hipStream_t)stream,
                       spec, basis, out, Cs, FP, F, nb, n_mels);
    return v2w_launch_status();
}

// The two ends with per-item lengths (include/vec2wav_hip.h): len a device array of B int32, item b holds min(len[b] * len_mul, L) samples.
extern "C" int v2w_mel_phases_len(const float* y, float* xp, int B, int L, int hop, int pad, int FP, const int32_t* len, int len_mul,
                                  void* stream) {
    if (!y || !xp || !len || len_mul < 1 || B <= 0 || L <= 1 || hop <= 0 || pad < 0 || pad >= L || FP <= 0 || (2 * pad) % hop) return V2W_E_ARG;
    if (!mel_phase_ints_fit(L, hop, pad, FP)) return V2W_E_SHAPE;
    int gx = (int)(((long long)hop * FP + 255) / 256); if (gx > 1024) gx = 1024;
    V2W_LAUNCH(mel_phase_len_kernel, dim3(gx, B), dim3(256), 0, (hipStream_t)stream, y, xp, len, len_mul, L, hop, pad, FP);
    return v2w_launch_status();
}

extern "C" int v2w_mel_finish_len(const float* spec, const float* basis, float* out, int B, int Cs, int FP, int F, int nb, int n_mels,
                                  const int32_t* len, int len_mul, int hop, int n_fft, void* stream) {
    if (!spec || !basis || !out || B <= 0 || F <= 0 || FP < F || nb <= 0 || Cs < 2 * nb || n_mels <= 0) return V2W_E_ARG;
    if (!len || len_mul < 1 || hop < 1 || n_fft < hop || n_fft % hop || (n_fft - hop) % 2) return V2W_E_ARG;
    const size_t lds = (size_t)nb * V2W_MEL_FT * sizeof(float);
    if (lds > 64 * 1024 || (long long)n_mels * V2W_MEL_FT > 0x7fffffffll) return V2W_E_SHAPE;
    if ((long long)F * hop + n_fft > 0x7fffffffll) return V2W_E_SHAPE;         // (the kernel's sample count of F frames is an int)
    V2W_LAUNCH(mel_finish_len_kernel, dim3((F + V2W_MEL_FT - 1) / V2W_MEL_FT, B), dim3(256), lds, (hipStream_t)stream,
                       spec, basis, out, len, len_mul, hop, n_fft, Cs, FP, F, nb, n_mels);
    return v2w_launch_status();
}

// Backward of v2w_mel_finish: gout (B, n_mels, F) -> dspec (B, Cs, FP), which the caller zero-fills (pad rows / frames stay 0).
// basisT (nb, n_mels) is the transposed filterbank.
extern "C" int v2w_mel_finish_bwd(const float* spec, const float* basis, const float* basisT, const float* gout, float* dspec,
                                  int B, int Cs, int FP, int F, int nb, int n_mels, void* stream) {
    if (!spec || !basis || !basisT || !gout || !dspec || B <= 0 || F <= 0 || FP < F || nb <= 0 || Cs < 2 * nb || n_mels <= 0)
        return V2W_E_ARG;
    const size_t lds = (size_t)(nb + n_mels) * V2W_MEL_FT * sizeof(float);
    if (lds > 64 * 1024) return V2W_E_SHAPE;
    V2W_LAUNCH(mel_finish_bwd_kernel, dim3((F + V2W_MEL_FT - 1) / V2W_MEL_FT, B), dim3(256), lds, (hipStream_t)stream,
                       spec, basis, basisT, gout, dspec, Cs, FP, F, nb, n_mels);
    return v2w_launch_status();
}

// Backward of v2w_mel_phases: dxp (B, hop, FP) -> dy (B, L); the reflected samples fold back onto their sources.
extern "C" int v2w_mel_phases_bwd(const float* dxp, float* dy, int B, int L, int hop, int pad, int FP, void* stream) {
    if (!dxp || !dy || B <= 0 || L <= 1 || hop <= 0 || pad < 0 || pad >= L || FP <= 0) return V2W_E_ARG;
    if (!mel_phase_ints_fit(L, hop, pad, FP)) return V2W_E_SHAPE;
    int gx = (int)(((long long)L + 255) / 256); if (gx > 1024) gx = 1024;
    V2W_LAUNCH(mel_phase_bwd_kernel, dim3(gx, B), dim3(256), 0, (hipStream_t)stream, dxp, dy, L, hop, pad, FP);
    return v2w_launch_status();
}

// ---- any frame geometry (include/vec2wav_hip.h): y (B, L) -> xp (B, CP, FP), xp[b][p][f] = ypad[b][f*hop + left + p] for p < hop, else 0
extern "C" int v2w_mel_phases_geo(const float* y, float* xp, int B, int L, int n_fft, int win, int hop, int CP, int pad, int left, int k,
                                  int FP, void* stream) {
    if (!y || !xp) return V2W_E_ARG;
    if (const int rc = mel_geo_ok(B, L, n_fft, win, hop, CP, pad, left, k, FP)) return rc;
    int gx = (int)(((long long)CP * FP + 255) / 256); if (gx > 1024) gx = 1024;
    V2W_LAUNCH(mel_phase_geo_kernel<false>, dim3(gx, B), dim3(256), 0, (hipStream_t)stream, y, xp, static_cast<const int32_t*>(nullptr), 1,
                       L, hop, CP, pad, left, k, n_fft, FP);
    return v2w_launch_status();
}

extern "C" int v2w_mel_phases_geo_len(const float* y, float* xp, int B, int L, int n_fft, int win, int hop, int CP, int pad, int left, int k,
                                      int FP, const int32_t* len, int len_mul, void* stream) {
    if (!y || !xp || !len || len_mul < 1) return V2W_E_ARG;
    if (const int rc = mel_geo_ok(B, L, n_fft, win, hop, CP, pad, left, k, FP)) return rc;
    int gx = (int)(((long long)CP * FP + 255) / 256); if (gx > 1024) gx = 1024;
    V2W_LAUNCH(mel_phase_geo_kernel<true>, dim3(gx, B), dim3(256), 0, (hipStream_t)stream, y, xp, len, len_mul,
                       L, hop, CP, pad, left, k, n_fft, FP);
    return v2w_launch_status();
}

extern "C" int v2w_mel_phases_geo_bwd(const float* dxp, float* dy, int B, int L, int n_fft, int win, int hop, int CP, int pad, int left, int k,
                                      int FP, void* stream) {
    if (!dxp || !dy) return V2W_E_ARG;
    if (const int rc = mel_geo_ok(B, L, n_fft, win, hop, CP, pad, left, k, FP)) return rc;
    int gx = (int)(((long long)L + 255) / 256); if (gx > 1024) gx = 1024;
    V2W_LAUNCH(mel_phase_geo_bwd_kernel, dim3(gx, B), dim3(256), 0, (hipStream_t)stream, dxp, dy, L, hop, CP, pad, left, FP);
    return v2w_launch_status();
}

// v2w_mel_finish for any nb whose 8-frame block fits 64 KiB of LDS: the 16-frame kernel (and its bits) wherever v2w_mel_finish takes it
extern "C" int v2w_mel_finish_geo(const float* spec, const float* basis, float* out, int B, int Cs, int FP, int F, int nb, int n_mels,
                                  void* stream) {
    if (const int rc = mel_finish_args_ok(spec, basis, out, B, Cs, FP, F, nb, n_mels)) return rc;
    if ((size_t)nb * V2W_MEL_FT * sizeof(float) <= 64 * 1024) return v2w_mel_finish(spec, basis, out, B, Cs, FP, F, nb, n_mels, stream);
    const size_t lds = (size_t)nb * V2W_MEL_FT8 * sizeof(float);
    if (lds > 64 * 1024) return V2W_E_SHAPE;
    V2W_LAUNCH(mel_finish8_kernel<false>, dim3((F + V2W_MEL_FT8 - 1) / V2W_MEL_FT8, B), dim3(256), lds, (hipStream_t)stream,
                       spec, basis, out, static_cast<const int32_t*>(nullptr), 1, 1, 1, Cs, FP, F, nb, n_mels);
    return v2w_launch_status();
}

// v2w_mel_finish_len without its conditions on n_fft / hop: pad = (n_fft - hop) / 2 rounded down, as mel_spectrogram pads
extern "C" int v2w_mel_finish_geo_len(const float* spec, const float* basis, float* out, int B, int Cs, int FP, int F, int nb, int n_mels,
                                      const int32_t* len, int len_mul, int hop, int n_fft, void* stream) {
    if (const int rc = mel_finish_args_ok(spec, basis, out, B, Cs, FP, F, nb, n_mels)) return rc;
    if (!len || len_mul < 1 || hop < 1 || n_fft < hop) return V2W_E_ARG;
    if ((long long)F * hop + n_fft > 0x7fffffffll) return V2W_E_SHAPE;         // (the kernel's sample count of F frames is an int)
    size_t lds = (size_t)nb * V2W_MEL_FT * sizeof(float);
    if (lds <= 64 * 1024) {
        V2W_LAUNCH(mel_finish_len_kernel, dim3((F + V2W_MEL_FT - 1) / V2W_MEL_FT, B), dim3(256), lds, (hipStream_t)stream,
                           spec, basis, out, len, len_mul, hop, n_fft, Cs, FP, F, nb, n_mels);
        return v2w_launch_status();
    }
    lds = (size_t)nb * V2W_MEL_FT8 * sizeof(float);
    if (lds > 64 * 1024) return V2W_E_SHAPE;
    V2W_LAUNCH(mel_finish8_kernel<true>, dim3((F + V2W_MEL_FT8 - 1) / V2W_MEL_FT8, B), dim3(256), lds, (hipStream_t)stream,
                       spec, basis, out, len, len_mul, hop, n_fft, Cs, FP, F, nb, n_mels);
    return v2w_launch_status();
}

extern "C" int v2w_mel_finish_geo_bwd(const float* spec, const float* basis, const float* basisT, const float* gout, float* dspec,
                                      int B, int Cs, int FP, int F, int nb, int n_mels, void* stream) {
    if (!basisT || !gout) return V2W_E_ARG;
    if (const int rc = mel_finish_args_ok(spec, basis, dspec, B, Cs, FP, F, nb, n_mels)) return rc;
    if ((size_t)(nb + n_mels) * V2W_MEL_FT * sizeof(float) <= 64 * 1024)
        return v2w_mel_finish_bwd(spec, basis, basisT, gout, dspec, B, Cs, FP, F, nb, n_mels, stream);
    const size_t lds = (size_t)(nb + n_mels) * V2W_MEL_FT8 * sizeof(float);
    if (lds > 64 * 1024) return V2W_E_SHAPE;
    V2W_LAUNCH(mel_finish8_bwd_kernel, dim3((F + V2W_MEL_FT8 - 1) / V2W_MEL_FT8, B), dim3(256), lds, (hipStream_t)stream,
                       spec, basis, basisT, gout, dspec, Cs, FP, F, nb, n_mels);
    return v2w_launch_status();
}

// ---- the mel L1 training loss fused into the finish kernels (include/vec2wav_hip.h).  len == NULL: no lengths, the LEN = false kernels.
extern "C" int v2w_mel_loss_plan(int B, int F, int nb, int n_mels, long long* scratch_bytes) {
    if (B <= 0 || F <= 0 || nb <= 0 || n_mels <= 0) return V2W_E_ARG;
    const int ft = mel_loss_fwd_ft(nb);
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
    const int ft = mel_loss_fwd_ft(nb);
    if (!ft) return V2W_E_SHAPE;
    const int tiles = (F + ft - 1) / ft;
    size_t lds = (size_t)nb * ft * sizeof(float);
    if (lds < 16 * sizeof(double)) lds = 16 * sizeof(double);                  // (the reduction's doubles live there too)
    hipStream_t st = (hipStream_t)stream;
    double* part = static_cast<double*>(ws);
#define V2W_MEL_LOSS_FWD(FT, LEN)                                                                                          \
    V2W_LAUNCH((mel_loss_fwd_kernel<FT, LEN>), dim3(tiles, B), dim3(256), lds, st, spec, basis, tgt, ts_f, ts_m, len, len_mul, \
               hop, n_fft, Cs, FP, F, Ft, nb, n_mels, part)
    if (ft == V2W_MEL_FT) { if (len) V2W_MEL_LOSS_FWD(V2W_MEL_FT, true); else V2W_MEL_LOSS_FWD(V2W_MEL_FT, false); }
    else { if (len) V2W_MEL_LOSS_FWD(V2W_MEL_FT8, true); else V2W_MEL_LOSS_FWD(V2W_MEL_FT8, false); }
#undef V2W_MEL_LOSS_FWD
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
    const int ft = (size_t)(nb + n_mels) * V2W_MEL_FT * sizeof(float) <= 64 * 1024 ? V2W_MEL_FT : V2W_MEL_FT8;
    const size_t lds = (size_t)(nb + n_mels) * ft * sizeof(float);
    if (lds > 64 * 1024) return V2W_E_SHAPE;
    hipStream_t st = (hipStream_t)stream;
#define V2W_MEL_LOSS_BWD(FT, LEN)                                                                                          \
    V2W_LAUNCH((mel_loss_bwd_kernel<FT, LEN>), dim3((F + FT - 1) / FT, B), dim3(256), lds, st, spec, basis, basisT, tgt, ts_f, ts_m, \
               gout, coef, len, len_mul, hop, n_fft, dspec, Cs, FP, F, Ft, nb, n_mels)
    if (ft == V2W_MEL_FT) { if (len) V2W_MEL_LOSS_BWD(V2W_MEL_FT, true); else V2W_MEL_LOSS_BWD(V2W_MEL_FT, false); }
    else { if (len) V2W_MEL_LOSS_BWD(V2W_MEL_FT8, true); else V2W_MEL_LOSS_BWD(V2W_MEL_FT8, false); }
#undef V2W_MEL_LOSS_BWD
    return v2w_launch_status();
}

// Backward of v2w_mel_phases_len / v2w_mel_phases_geo_len: their arguments, dxp -> dy
extern "C" int v2w_mel_phases_len_bwd(const float* dxp, float* dy, int B, int L, int hop, int pad, int FP, const int32_t* len, int len_mul,
                                      void* stream) {
    if (!dxp || !dy || !len || len_mul < 1 || B <= 0 || L <= 1 || hop <= 0 || pad < 0 || pad >= L || FP <= 0 || (2 * pad) % hop) return V2W_E_ARG;
    if (B > 65535 || !mel_phase_ints_fit(L, hop, pad, FP)) return V2W_E_SHAPE;
    int gx = (int)(((long long)L + 255) / 256); if (gx > 1024) gx = 1024;
    V2W_LAUNCH(mel_phase_len_bwd_kernel, dim3(gx, B), dim3(256), 0, (hipStream_t)stream, dxp, dy, len, len_mul, L, hop, pad, FP);
    return v2w_launch_status();
}

extern "C" int v2w_mel_phases_geo_len_bwd(const float* dxp, float* dy, int B, int L, int n_fft, int win, int hop, int CP, int pad, int left,
                                          int k, int FP, const int32_t* len, int len_mul, void* stream) {
    if (!dxp || !dy || !len || len_mul < 1) return V2W_E_ARG;
    if (const int rc = mel_geo_ok(B, L, n_fft, win, hop, CP, pad, left, k, FP)) return rc;
    int gx = (int)(((long long)L + 255) / 256); if (gx > 1024) gx = 1024;
    V2W_LAUNCH(mel_phase_geo_len_bwd_kernel, dim3(gx, B), dim3(256), 0, (hipStream_t)stream, dxp, dy, len, len_mul,
               L, hop, CP, pad, left, k, n_fft, FP);
    return v2w_launch_status();
}
