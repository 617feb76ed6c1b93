/*
 * vec2wav_hip.h - C ABI of libvec2wav_hip.so: the Vec2Wav generator forward path as
 * hand-written HIP kernels for gfx950 (MI355X / CDNA4).
 *
 * The reference (p1an-lin-jung/WavThruVec_pytorch) has no FFI/operator layer: its boundary is
 * the Python nn.Module surface (vec2wav/models.py:77-156, vec2wav/modules.py:5-30) and everything
 * underneath is stock torch ops.  Each entry point below therefore cites the reference statement
 * (file:line under /root/reference) whose arithmetic it replaces; the Python mirror of the
 * reference surface (wavthruvec_pytorch_amd/models.py) is the only caller.  INTEGRATION.md shows
 * the ctypes binding.
 *
 * Conventions (all entry points):
 *   - plain pointers and sizes, no torch types; every pointer is a DEVICE pointer unless said
 *     otherwise; activations are fp32, channels-first, contiguous (B, C, L);
 *   - `stream` is a hipStream_t passed as void* (0 = the null stream); launches are asynchronous,
 *     nothing allocates, nothing synchronises, no ownership is transferred;
 *   - return value: 0 = enqueued; < 0 = bad argument (V2W_E_*); > 0 = a hipError_t from the launch;
 *   - no global mutable state: safe to call concurrently on distinct streams.
 *
 * Folded weight layout ("wf"): fp32 [k][C_in][C_out] (C_out fastest) for both Conv1d and
 * ConvTranspose1d, produced by v2w_wn_fold_* from the reference's weight_g/weight_v parameters.
 */
#ifndef VEC2WAV_HIP_H
#define VEC2WAV_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define V2W_ABI_VERSION 35

#define V2W_E_ARG      (-1)  /* null pointer / non-positive size */
#define V2W_E_SHAPE    (-2)  /* shape not supported by the requested algorithm */
#define V2W_E_ALGO     (-3)  /* unknown algorithm id */

/* algorithm selector of the conv entry points */
#define V2W_ALGO_AUTO   0    /* MFMA tile kernel when the shape allows, else the direct kernel */
#define V2W_ALGO_DIRECT 1    /* one-thread-per-output scalar FMA kernel: any shape; cross-check */
#define V2W_ALGO_MFMA   2    /* f32 MFMA (v_mfma_f32_32x32x2_f32 / 16x16x4_f32) implicit GEMM; V2W_E_SHAPE if unsupported */
#define V2W_ALGO_BF16   4    /* bf16 operands (rne), ONE v_mfma_f32_32x32x16_bf16 per product, fp32 accumulate: BASELINE configs[2];
                              * same kernel, tiles and buffers as V2W_ALGO_SPLIT with fragments from v2w_pack_bf16 */
#define V2W_ALGO_SPLIT  3    /* split-f16 MFMA: x = hi + lo halves, x_hi*w_hi + x_hi*w_lo + x_lo*w_hi accumulated in fp32 (~22-bit
                              * products; v_mfma_f32_32x32x16_f16); needs wps / winv from v2w_pack_split; Conv1d with
                              * C_in % 16 == 0, C_out % 64 == 0 and an odd k >= 3, else V2W_E_SHAPE */
#define V2W_ALGO_WINO   5    /* (ABI v35) exact-fp32 Winograd F(2,3) over output pairs (t, t + dil) on v_mfma_f32_32x32x2_f32: 4 / 10 / 15 products
                              * per output pair and channel pair for k = 3 / 7 / 11 against 6 / 14 / 22; `wp` holds the v2w_pack_wino stream.
                              * Conv1d with C_in % 32 == 0, C_in >= 64, C_out % 64 == 0, an odd k >= 3 and symmetric padding; unit input stride,
                              * no channel slices, no mask / rowsum_part / out_slope, more than 128 workgroups (sum over the problems of
                              * B * ceil(pairs / 64) * C_out / 64, pairs = dil * ceil(L / (2 dil))); else V2W_E_SHAPE and nothing is launched
                              * (the caller runs V2W_ALGO_MFMA).  Not taken by V2W_ALGO_AUTO. */

int         v2w_abi_version(void);
const char* v2w_build_arch(void);       /* "gfx950" */

/* ---- Which kernels would this call launch?  (ABI v33; host-only.)  Every launching entry point - the ones whose last argument is the stream -
 * accepts a NAME SINK in place of the stream: the call runs every shape check and every kernel selection it would make, launches nothing, sets
 * no attribute, dereferences no tensor pointer, and appends the demangled name of each kernel it would have launched, one per line and in launch
 * order, to the caller's buffer (exactly the string `rocprofv3 --kernel-trace` prints for that kernel: "void (anonymous namespace)::
 * wide_stage_bf16_kernel<1, 4, 1, 2, 2, 32, false, true, 2, false>((anonymous namespace)::WideArgs)").  The return value is the one the real call
 * would give up to the launch (0, or V2W_E_*).  bench.py labels its per-kernel rooflines and looks up the counter profiles with these names
 * instead of a table of template arguments kept by hand.  The sink is the caller's: { V2W_NAME_SINK_MAGIC, buf, cap, 0 }; `len` counts
 * the bytes written (names that do not fit are dropped, `len` stays below cap, the buffer is always NUL-terminated). */
typedef struct { uint64_t magic; char* buf; int32_t cap; int32_t len; } v2w_name_sink;
#define V2W_NAME_SINK_MAGIC 0x5632574e414d4531ull
#define V2W_NAME_SINK_STREAM(sink) ((void*)((uintptr_t)(sink) | (uintptr_t)1))   /* pass as `stream`: real stream handles are aligned pointers */

/* ---- K0: weight-norm fold (torch.nn.utils.weight_norm pre-forward hook, dim=0; triggered by
 * models.py:18-33,58-61,83,90-92,100).  w = g * v / ||v||, norm over all dims but 0.
 * conv : v (C_out, C_in, k), g (C_out)  -> wf [k][C_in][C_out]      (norm per C_out)
 * convt: v (C_in, C_out, k), g (C_in)   -> wf [k][C_in][C_out]      (norm per C_in)
 * g == NULL means "weight norm already removed" (models.py:149-156): v is the plain weight, relayout only.
 * scratch: >= rows floats (rows = C_out for conv, C_in for convt). */
int v2w_wn_fold_conv (const float* v, const float* g, float* wf, float* scratch,
                      int c_out, int c_in, int k, void* stream);
int v2w_wn_fold_convt(const float* v, const float* g, float* wf, float* scratch,
                      int c_in, int c_out, int k, void* stream);

/* dgrad weights: out[t][C_out][C_in] = wf[k-1-t][C_in][C_out]; the conv that back-propagates through Conv1d(w, dilation d)
 * is a Conv1d of the output gradient with these weights and the same dilation (then v2w_pack_mfma(out, k, C_out, C_in)). */
int v2w_wf_transpose_flip(const float* wf, float* out, int k, int c_in, int c_out, void* stream);
/* general form: out[m][C_out][C_in] = wf[t_start + m*t_step][C_in][C_out], m < n.  Phase r of ConvTranspose1d(k, u, pad):
 * t_start = (r+pad)%u, t_step = u, n = taps of the phase; run as Conv1d over dy's phase r with pad_left = (r+pad)/u. */
int v2w_wf_gather_transpose(const float* wf, float* out, int k, int c_in, int c_out, int t_start, int t_step, int n, void* stream);

/* MFMA operand packing: wf [k][C_in][C_out] -> wp, the same k*C_in*C_out weights as a stream of 1 KiB MFMA A-fragments
 * (64 lanes x float4 = four consecutive MFMA k-steps) in exactly the order the tile kernel of that layer consumes them:
 * [row block mb][C_in chunk][tap, phase-major for a transposed conv][fragment]; the kernel reads it strictly
 * sequentially.  u = 1 for Conv1d, the stride for ConvTranspose1d.  Returns V2W_E_SHAPE when the layer has no MFMA
 * tile configuration (C_in % 16 != 0, C_out neither 16 nor a multiple of 32, unsupported stride): such layers run on
 * the direct kernel with wp = NULL. */
int v2w_pack_mfma(const float* wf, float* wp, int k, int c_in, int c_out, int u, void* stream);
/* the stream of the layer's input-gradient conv (== v2w_pack_mfma of v2w_wf_transpose_flip(wf)) straight from wf [k][c_out][c_in]:
 * c_in / c_out are the GRADIENT conv's channel counts (backward of models.py:65-70: dx = conv(dy; W^T, taps reversed)) */
int v2w_pack_mfma_dgrad(const float* wf, float* wp, int k, int c_in, int c_out, void* stream);
/* n matrices back to back -> n packed streams back to back in one launch (the groups of a grouped conv) */
int v2w_pack_mfma_batch(const float* wf, float* wp, int k, int c_in, int c_out, int u, int n, void* stream);
/* V2W_ALGO_WINO (ABI v35): wf [k][c_in][c_out] -> wpw, v2w_wino_terms(k) * c_in * c_out floats: the transformed weights of every segment
 * term (G0 = g0, G1 = (g0+g1+g2)/2, G2 = (g0-g1+g2)/2, G3 = g2 for 3 taps; g0, g0+g1, g1 for 2; g0, -g0 for 1) in MFMA A-fragment order
 * [32-row block][32-channel chunk][segment][4-k-step unit][term].  V2W_E_SHAPE unless k is odd and >= 3, c_in % 32 == 0, c_out % 32 == 0. */
int v2w_pack_wino(const float* wf, float* wpw, int k, int c_in, int c_out, void* stream);
int v2w_wino_terms(int k);   /* weight matrices of the Winograd form of a k-tap conv: 4 (k/3) + {0, 2, 3}[k % 3]; 0 for even k or k < 3 */

/* Batched form of fold + pack for every MFMA layer of a generator: two launches instead of three per layer.
 *   v2w_fold_plan       (host only) fills mf/ck of each descriptor and starts[2*(n+1)] (block prefix sums of the scale
 *                       and of the pack kernel); returns the dynamic-LDS byte count (> 0) the pack kernel needs, or
 *                       V2W_E_SHAPE when a layer has no MFMA tile configuration (fold such layers one by one).
 *   v2w_fold_pack_batch descs_dev / starts_dev are DEVICE copies of the planned arrays; nblk_scale = starts[n],
 *                       nblk_pack = starts[2n+1].
 * v: weight_v (conv (C_out,C_in,k); transposed (C_in,C_out,k)); g: weight_g or NULL; scale: >= rows floats scratch. */
typedef struct {
    const float* v; const float* g; float* wp; float* scale;
    int32_t c_in, c_out, k, u, transposed;
    int32_t mf, ck;     /* filled by v2w_fold_plan */
    int32_t _pad;
    float* wf;          /* optional (ABI v28): the folded weight in the plain layout [k][C_in][C_out] as well (what v2w_wn_fold_conv / _convt
                         * write) - a forward that will be back-propagated needs it for the gradient kernels; NULL: not written */
    float* wpd;         /* optional (ABI v28; Conv1d layers with C_in == C_out whose tile configuration has MF == CK only, else must be NULL):
                         * the fragment stream of the layer's INPUT-GRADIENT conv (tap-reversed transpose, what v2w_pack_mfma_dgrad builds
                         * from wf) in the same pass */
    float* wpw;         /* optional (ABI v35; Conv1d layers whose tile configuration is MF == CK == 32 with an odd k >= 3, else must be NULL):
                         * the V2W_ALGO_WINO stream of the layer (what v2w_pack_wino builds from wf) in the same pass.
                         * A transposed layer with k == 2 u, u in {2, 4}, C_in % 32 == 0 and >= 64, u * C_out % 64 == 0: the stream of
                         * v2w_convt1d_wino_fwd, 3 * u * C_out * C_in floats - the weight as a two-tap Conv1d over u * C_out rows (row =
                         * co * u + phase, taps (w[phase + u], w[phase]) on (x[t - 1], x[t])), per row the terms g0, g0 + g1, g1 of the two-tap
                         * segment, in MFMA A-fragment order [32-row block][32-channel chunk][4-k-step unit][term] */
} v2w_fold_desc;
int v2w_fold_plan(v2w_fold_desc* descs, int n, int32_t* starts);
int v2w_fold_pack_batch(const v2w_fold_desc* descs_dev, const int32_t* starts_dev, int n,
                        int nblk_scale, int nblk_pack, int lds_bytes, void* stream);

/* ---- K1/K5/K6/K7: fused [per-(b,c) affine] -> leaky_relu -> dilated Conv1d -> +bias [-> +residual]
 * [-> += out] [-> / out_div].  Replaces F.leaky_relu + Conv1d (+ `xt + x`, `xs += ...`, `xs / num_kernels`)
 * of models.py:37-44 (ResBlock1), 65-70 (ResBlock2), 123 (conv_pre), 135-141 (mean over kernels).
 *   in   (B, C_in, L)     in_a/in_s   (B, C_in)  or NULL : x = in_a*in + in_s before the activation
 *                                                          (the CondBN affine of modules.py:25-28 folded into the load)
 *   res  (B, C_out, L) or NULL; res_a/res_s (B, C_out) or NULL : residual = res_a*res + res_s
 *   out  (B, C_out, L);   padding = dil*(k-1)/2 (utils.py:35-36), k odd
 *   slope: leaky_relu negative slope applied to the conv operand (1.0f = none)
 *   accumulate != 0: out = out_old + value ; out_div != 0: out = value / out_div (applied last) */
typedef struct {
    const float* in;   const float* in_a;  const float* in_s;
    const float* wf;   /* [k][C_in][C_out]: read by the direct kernel; may be NULL when algo == V2W_ALGO_MFMA */
    const float* wp;   /* v2w_pack_mfma() form: read by the MFMA kernel; NULL -> direct kernel under V2W_ALGO_AUTO */
    const float* bias;
    const float* res;  const float* res_a; const float* res_s;
    const float* add0; const float* add1;   /* optional extra addends (B, C_out, L): out = (add0 [+ add1]) + value, then / out_div;
                                             * the explicit form of `xs += ...` (models.py:137-141) when the branches ran
                                             * concurrently into separate buffers; exclusive with `accumulate` */
    const float* mask_src; const float* mask_a; const float* mask_s;   /* optional (backward use): the conv result is
                                             * multiplied by lrelu'(mask_a*mask_src + mask_s) = 1 or mask_slope BEFORE bias /
                                             * residual / addends; mask_src (B, C_out, L), mask_a/_s (B, C_out) or NULL */
    float*       out;
    int32_t B, C_in, C_out, L, k, dil;
    float   slope;
    int32_t accumulate;
    float   out_div;
    int32_t algo;
    float   mask_slope;
    int32_t in_stride, in_phase;  /* 0/1, 0: plain.  > 1: the conv reads the de-interleaved phase in[.., in_stride*l + in_phase] of a
                                   * (B, C_in, in_stride*L) tensor (dgrad of a transposed conv, one launch per phase) */
    int32_t pad_left;             /* -1: symmetric padding dil*(k-1)/2.  >= 0: taps sit at offsets -pad_left + t*dil (k may be even) */
    const void*  wps;             /* V2W_ALGO_SPLIT: v2w_pack_split() fragments of this layer; else ignored */
    const float* winv;            /* V2W_ALGO_SPLIT: device pointer to 1/scale of the layer (sc[0] of v2w_pack_split) */
    int32_t in_ct, out_ct;        /* 0: plain.  > 0: `in` / `out` (and res, add, mask_src) point at the first channel of a C_in / C_out
                                   * channel slice of tensors with in_ct / out_ct channels per batch item: one group of a grouped
                                   * Conv1d (models.py:222-227), one launch per group (or 4 per launch through _fwd_multi).
                                   * Not combined with the per-(b, channel) affines; f32 MFMA and direct kernels only */
    float   out_slope;            /* 0 or 1: none.  Else leaky_relu(value, out_slope) on what is stored (applied last): the
                                   * discriminators keep the ACTIVATED feature maps (models.py:184-186, 236-238) */
    int32_t io_bf16;              /* V2W_ALGO_BF16 only (else must be 0): activation STORAGE in bf16 - BASELINE configs[2] priced at 2 bytes
                                   * per activation.  bit 0: `in` is bf16; bit 1: `out`, `res`, `add0`, `add1` are bf16.
                                   * Accumulation, bias, affines and the residual arithmetic stay fp32; one rounding at the store. */
    float*  rowsum_part;          /* optional, masked (mask_src != NULL) f32 MFMA launches with float4-aligned operands only: the launch also
                                   * writes, per position tile and output channel, (sum of the values it stored, 0) to
                                   * rowsum_part[tile][C_out][2] - tiles = v2w_conv1d_tile_config()[9] - for v2w_bn_reduce_partials to add up:
                                   * the bias gradient of the layer whose output gradient this launch produces (backward of models.py:65-70)
                                   * without another pass over the tensor.  V2W_E_ARG when the launch cannot provide it. */
    float*  splitk_ws;
    int64_t splitk_ws_bytes;      /* optional CALLER-OWNED scratch for the f32 MFMA path (ABI v28; the library allocates nothing and keeps no
                                   * state between calls): a launch that cannot fill the chip (<= 128 workgroups: inference at B = 1) is split
                                   * over slices of C_in, every slice stores plain partial sums to its own slab of this buffer and a second
                                   * kernel adds the slabs in slice order and applies bias / residual / addends / division (deterministic).
                                   * v2w_conv1d_splitk_ws_bytes() says how many bytes this launch would use (0: it runs unsplit); NULL, or fewer
                                   * bytes than that: the launch runs unsplit - same values up to the summation order over C_in.  Launches that
                                   * share a buffer must be ordered on ONE stream (a module keeps one buffer per stream it launches on).
                                   * _fwd_multi reads the fields of a[0]. */
} v2w_conv1d_args;
int v2w_conv1d_fwd(const v2w_conv1d_args* a, void* stream);   /* `a` is a HOST pointer, read before return */
/* Bytes of `splitk_ws` the f32 MFMA launch of a[0..n) would use (sizes only are read; 0: no split / another kernel serves it). */
long long v2w_conv1d_splitk_ws_bytes(const v2w_conv1d_args* a, int n);
/* a[0..n) (n <= 4) convs that share B, C_in, C_out, L in ONE launch (MFMA path; V2W_E_SHAPE -> issue them one by one):
 * the residual branches of one generator stage, heaviest first. */
int v2w_conv1d_fwd_multi(const v2w_conv1d_args* a, int n, void* stream);

/* ---- split-f16 weights (V2W_ALGO_SPLIT).  wf [k][C_in][C_out] (folded fp32) -> wps: k*C_in*C_out*4 + 2048 bytes (the tail is padding) holding, per 32-row
 * block, chunk of 32 input channels and tap, the (hi, lo) half-precision MFMA A fragments of scale*w in consumption order;
 * scale = the power of two that puts max|w| of the layer into [8192, 16384).  The halves do NOT all stay in the normal f16 range: a scaled
 * weight below about 2^-3 - a weight some 2^-16 of the layer's maximum or less - has an f16 SUBNORMAL lo half, which carries an absolute error
 * of 2^-25 / scale (<= 2^-38 max|w|) instead of the relative 2^-22.
 * sc: 4 floats of device memory: [0] = 1/scale (the `winv` of v2w_conv1d_args), [1] = scale, [2] = scratch.
 * Activations are split on the fly by the conv kernel and must satisfy |x| <= 65504 (they are clamped there); they are not scaled: below
 * |x| of about 2^-3 their lo half is subnormal as well (absolute error 2^-25 per operand instead of 2^-22 |x|). */
int v2w_split_supported(int c_in, int c_out, int u);   /* 1 when V2W_ALGO_SPLIT serves this layer shape */
int v2w_split_packable(int c_in, int c_out);           /* 1 when v2w_pack_split / _bf16 / _batch accept the shape (C_in % 16; C_out % 32, or C_out == 16 zero-padded to 32 rows) */
int v2w_pack_split(const float* wf, void* wps, float* sc, int k, int c_in, int c_out, void* stream);
int v2w_pack_bf16(const float* wf, void* wps, float* sc, int k, int c_in, int c_out, void* stream);   /* same buffers, V2W_ALGO_BF16 */
/* Batched weight-norm fold + split pack of n Conv1d layers straight from the parameters (weight_v (C_out, C_in, k), weight_g or
 * NULL): three launches for all of them.  descs / starts are DEVICE arrays; starts[0..n] = prefix sums of c_out,
 * starts[n+1..2n+1] = prefix sums of ceil(c_out/32)*(c_in/16); nblk_* = their totals; k_max = largest kernel size. */
typedef struct {
    const float* v; const float* g;   /* weight_v, weight_g (NULL: plain weight) */
    void* wps; float* sc;             /* outputs: as v2w_pack_split */
    float* rowscale;                  /* c_out floats of workspace */
    int32_t c_in, c_out, k;
    int32_t mode;                     /* 0: split f16 (hi, lo) fragments; 1: bf16 fragments for V2W_ALGO_BF16 */
} v2w_split_desc;
/* all_bf16 != 0: every descriptor has mode 1 (no scale record is kept: two launches instead of three) */
int v2w_split_pack_batch(const v2w_split_desc* descs_dev, const int32_t* starts_dev, int n, int nblk_rows, int nblk_pack,
                         int k_max, int all_bf16, void* stream);

/* ---- K6 fused pair for the narrow stages (C == 32 or 16; MFMA path): two chained convs of one residual block in ONE kernel,
 * the intermediate stays in LDS (these layers are HBM-bound as separate launches).
 *   res_mode 0 (ResBlock2, models.py:65-70): t1 = x + conv_{k,dil1}(lrelu(x)) + b1 ; out = t1 + conv_{k,dil2}(lrelu(t1)) + b2
 *   res_mode 1 (ResBlock1 pair, models.py:37-44): t1 = conv_{k,dil1}(lrelu(x)) + b1 ; out = x + conv_{k,dil2}(lrelu(t1)) + b2
 *   x = in_a*in + in_s when the affine is given; then out = ((add0 [+ add1]) + out) [/ out_div] as in v2w_conv1d_args.
 *   wp1 / wp2: v2w_pack_mfma(k, C, C, 1) streams.  a[0..n) (n <= 4) share B, C, L and go out as one launch.
 * Returns V2W_E_SHAPE when C or the receptive field does not fit: run the two convs with v2w_conv1d_fwd instead. */
typedef struct {
    const float* in; const float* in_a; const float* in_s;
    const float* wp1; const float* bias1; const float* wp2; const float* bias2;
    const float* add0; const float* add1;
    float* out;
    int32_t B, C, L, k, dil1, dil2;
    int32_t res_mode;
    float slope, out_div;
} v2w_pair_args;
int v2w_resblock_pair_fwd(const v2w_pair_args* a, int n, void* stream);

/* ---- K6+K7 fused for a narrow ResBlock2 stage (C == 32 or 16): the whole residual section of models.py:135-141,
 *   out = ( sum_j [ t1_j + conv_{k_j,dil2_j}(lrelu(t1_j)) + b2_j ] ) / out_div,  t1_j = x + conv_{k_j,dil1_j}(lrelu(x)) + b1_j,
 * x = in_a*in + in_s, in ONE kernel: x is read once, every t1_j stays in LDS, the branch sum stays in registers and is
 * added in the reference's order.  nk <= 4 branches.  V2W_E_SHAPE -> use the per-branch entry points. */
typedef struct {
    const float* in; const float* in_a; const float* in_s;
    const float* wp1[4]; const float* bias1[4]; const float* wp2[4]; const float* bias2[4];
    int32_t k[4], dil1[4], dil2[4];
    float* out;
    int32_t nk, B, C, L;
    float slope, out_div;
    /* optional fused tail of the generator (ABI v29; v2w_resblock2_stage_fwd with C == 16 only; models.py:143-145): when post_out != NULL the
     * kernel does not write `out` (it may be NULL) but  post_out (B, 1, L) fp32 = tanh(conv_post(leaky_relu(stage output, post_slope)))  with
     * post_w = the folded conv_post weight [post_k][C][1] (v2w_wn_fold_conv), post_b its bias (1 value or NULL), post_k odd <= 9.  The
     * stage's output - 168 MB at BASELINE configs[1] - is neither written nor read back, one launch less. */
    const float* post_w; const float* post_b; float* post_out;
    int32_t post_k;
    float post_slope;
    /* optional INPUT-GRADIENT form (ABI v31; v2w_resblock2_stage_fwd only; the backward of models.py:135-141 for a narrow stage, train.py:214):
     * when bwd_mask2 != NULL the kernel computes, with dr = in_a * in + in_s (the caller passes in = dL/d(out), in_a = 1 / nk, in_s = 0),
     *     bwd_mid[j] (B, C, L) = dt1_j = dr + lrelu'(bwd_mask1[j]) * conv(dr; wp1[j])                  bwd_mask1[j] = the forward's t1_j
     *     out (B, C, L)        = sum_j dt1_j + lrelu'(bwd_mask2_a * bwd_mask2 + bwd_mask2_s) * sum_j conv(dt1_j; wp2[j])      bwd_mask2 = the forward's xr
     * where wp1[j] / wp2[j] are the fragment streams of the TRANSPOSED, tap-reversed weights of conv2_j / conv1_j (v2w_pack_mfma_dgrad),
     * dil1[j] / dil2[j] their dilations (conv2_j's first), lrelu'(v) = v > 0 ? 1 : bwd_slope.  slope must be 1, the biases NULL, out_div 0. */
    const float* bwd_mask1[4]; float* bwd_mid[4];
    const float* bwd_mask2; const float* bwd_mask2_a; const float* bwd_mask2_s;
    float bwd_slope;
    /* bwd_rowsum[j] (optional): v2w_resblock2_stage_bwd_rows(a) rows of [C][2] floats - per (tile, wave) the channel sums of dt1_j over the
     * positions the tile owns (second value 0): the bias gradient of conv1_j after v2w_bn_reduce_partials adds the rows up. */
    float* bwd_rowsum[4];
} v2w_stage_args;
int v2w_resblock2_stage_fwd(const v2w_stage_args* a, void* stream);
int v2w_resblock2_stage_bwd_rows(const v2w_stage_args* a);
/* Winograd F(2,3) form of the plain forward for C == 32 (no tail, no gradient form): the same section with 4 / 10 / 15 MFMA terms
 * per output pair for k = 3 / 7 / 11 instead of 6 / 14 / 22.  HERE wp1[j] / wp2[j] are the v2w_pack_wino streams of the layers (v2w_fold_desc::wpw
 * writes them in the batched fold).  Every k odd and >= 3, every dil1 == 1, dil2 such that the pairs of a 256-position window cover its kept
 * outputs (1, 2, 3, ...; the standard set (3,1,3), (7,1,3), (11,1,3) is the measured case).  Results equal v2w_resblock2_stage_fwd up to Winograd
 * rounding; fixed summation order, run-to-run bit-identical.  V2W_E_SHAPE otherwise (the caller then uses v2w_resblock2_stage_fwd with the
 * v2w_pack_mfma streams).  v2w_resblock2_stage_wino_tile: outputs a tile keeps, i.e. the positions between tile starts (0: shape not taken). */
int v2w_resblock2_stage_wino_fwd(const v2w_stage_args* a, void* stream);
int v2w_resblock2_stage_wino_tile(const v2w_stage_args* a);
/* ... with per-item valid lengths, as v2w_resblock2_stage_fwd_len: bit-identical to v2w_resblock2_stage_wino_fwd when every length is L */
int v2w_resblock2_stage_wino_fwd_len(const v2w_stage_args* a, const int32_t* len, int len_mul, void* stream);
/* The same section for an 8-channel stage (the sixth stage of a x640 generator, upsample_rates (5,4,4,2,2,2); ABI v27), fp32 on the
 * vector ALU: C == 8, odd kernel sizes, halos <= 32, nk <= 4.  HERE wp1[j] / wp2[j] are the FOLDED weights [k][C][C] of
 * v2w_wn_fold_conv (there is no fragment stream for 8 channels).  V2W_E_SHAPE otherwise. */
int v2w_resblock2_stage_small_fwd(const v2w_stage_args* a, void* stream);

/* Split-operand counterpart (V2W_ALGO_SPLIT / V2W_ALGO_BF16 arithmetic) for C == 32 or 16 - and, with bf16 != 0 on bf16 tensors
 * (io_bf16 == 3), for the wide stages C == 64 / 128 / 256 as well (csrc/v2w_stage_bf16_wide.hip: x and t1_j resident in LDS, one kernel): wps / sc from v2w_pack_split or
 * v2w_pack_bf16 (or the batch) of the (k, C, C) layers; bf16 != 0 selects the bf16 single-MFMA form.  V2W_E_SHAPE otherwise.
 * Fragment streams: the fp32-tensor kernels (io_bf16 == 0: csrc/v2w_stage_split.hip) walk ONE weight stream - there the 2*nk streams must
 * lie BACK TO BACK in execution order (wps1[0], wps2[0], wps1[1], ...; (C/16)*k units of 2 KiB each, slices of one buffer), V2W_E_ARG if
 * they do not.  The bf16-tensor kernels (io_bf16 == 3: v2w_stage_bf16_wide.hip, v2w_stage_bf16_n16.hip, v2w_stage_bf16.hip) take every
 * stream through its own pointer: any placement. */
typedef struct {
    const float* in; const float* in_a; const float* in_s;
    const void*  wps1[4]; const float* sc1[4]; const float* bias1[4];
    const void*  wps2[4]; const float* sc2[4]; const float* bias2[4];
    int32_t k[4], dil1[4], dil2[4];
    float* out;
    int32_t nk, B, C, L;
    float slope, out_div;
    int32_t bf16;
    int32_t io_bf16;   /* bf16 != 0 only: bit 0 `in` is bf16, bit 1 `out` is bf16 (see v2w_conv1d_args) */
    /* optional fused tail of the generator (bf16 != 0, io_bf16 == 3, C == 16 only; models.py:143-145): when post_out != NULL the kernel does
     * not write `out` (it may be NULL) but  post_out (B, 1, L) fp32 = tanh(conv_post(leaky_relu(stage output, post_slope)))  with
     * post_w = the folded conv_post weight [post_k][C][1] (v2w_wn_fold_conv), post_b its bias (1 value or NULL), post_k odd <= 9 */
    const float* post_w; const float* post_b; float* post_out;
    int32_t post_k;
    float post_slope;
    /* optional fused UPSAMPLER of the next stage (ABI v28; bf16 != 0, io_bf16 == 3, the reference's block set k = (3, 7, 11), dilations (1, 3);
     * models.py:128-129): when up_out != NULL the kernel does not write `out` (it may be NULL) but
     *   up_out (B, C / 2, up_u L) bf16 = ConvTranspose1d(leaky_relu(stage output, up_slope); up_k = 2 up_u taps, stride up_u, padding up_u / 2) + up_bias
     * and, when up_stats_part != NULL, the BatchNorm partial sums of those fp32 values as v2w_convt1d_bf16_fwd writes them
     * ([v2w_resblock2_stage_up_tiles()][C / 2][2], for v2w_bn_reduce_partials).  up_wps: the fragments of v2w_pack_bf16_convt(k = up_k, C, C / 2,
     * up_u).  Served: (C, up_u) = (256, 4), (128, 4), (64, 2), (32, 2); V2W_E_SHAPE otherwise (run the stage and v2w_convt1d_bf16_fwd). */
    const void* up_wps; const float* up_bias; void* up_out; float* up_stats_part;
    int32_t up_k, up_u;
    float up_slope;
    /* ResBlock1 pair mode (ABI v28; rb1 != 0, bf16 != 0, io_bf16 == 3; models.py:37-44 on bf16 tensors): the nk entries are independent PROBLEMS -
     * branch p of a stage at one of its three (dilated conv, conv) pairs - run in one launch:
     *   out_b[p] = ( x_p + conv_{k[p], dil2[p]}(lrelu(conv_{k[p], dil1[p]}(lrelu x_p) + bias1[p])) + bias2[p] ) [ + add0 + add1 ] / out_div ,
     *   x_p = in_a * in_b[p] + in_s (in_b[p] == NULL: `in`; in_a / in_s as above, NULL for the second and third pair).
     * add0 / add1 (bf16 (B, C, L) or NULL): added, add0 + add1 first, by the LAST problem of the launch before the division - the final pair of
     * the last branch takes the other branches' results: ((r0 + r1) + r2) / nk.  `out`, post_*, up_* are not used.  C = 16 .. 256. */
    int32_t rb1;
    const void* in_b[4]; void* out_b[4];
    const void* add0; const void* add1;
} v2w_stage_split_args;
int v2w_resblock2_stage_split_fwd(const v2w_stage_split_args* a, void* stream);
/* Shape query (ABI v28; host-only, nothing is launched or dereferenced): 0 when the call above would run this stage as one kernel, else the
 * code it would return.  Read: B, C, L, nk, k, dil1, dil2, bf16, io_bf16, slope, post_* and the ALIGNMENT of `in` / `out` when they are set
 * (NULL tensor and weight pointers count as aligned). */
int v2w_resblock2_stage_split_config(const v2w_stage_split_args* a);
/* Rows of up_stats_part a call with the fused upsampler (up_u != 0) fills; <= 0: that call would not run fused.  Host-only, as above. */
int v2w_resblock2_stage_up_tiles(const v2w_stage_split_args* a);

/* ---- the residual convolutions of a WIDE ResBlock2 stage (C = 64 or 128) on bf16 tensors (BASELINE configs[2]: bf16 compute / fp32
 * accumulate, bf16 activation storage), one launch per conv position of the block instead of one per branch group
 * (csrc/v2w_conv_bf16_res.hip; models.py:135-141 with ResBlock2.forward, models.py:65-70, inlined):
 *   mode 0  t1_j = x + conv_{k_j,dil_j}(lrelu(x)) + bias_j  for j < nbr, x = in_a * in[0] + in_s (per (b, c); NULL: x = in[0]):
 *           in[0] is read ONCE for all branches, out[j] receives t1_j;
 *   mode 1  out[0] = ( sum_j [ in[j] + conv_{k_j,dil_j}(lrelu(in[j])) + bias_j ] ) / out_div   (out_div == 0: no division):
 *           one accumulator across the branches, nothing but out[0] is written.
 * in / out are bf16 (B, C, L) tensors, 16-byte aligned, L % 4 == 0; wps[j] = the fragments of v2w_pack_bf16 / v2w_split_pack_batch of
 * the (k_j, C, C) layer; k odd.  Served: C % 64 == 0 whose resident tile - every channel of 256 positions and the largest halo
 * h = max_j dil_j (k_j - 1) / 2 of the launch - fits the LDS twice per CU: C = 64 with h <= 32 and C = 128 with h <= 24; C >= 192 is not.
 * in_a and in_s come together (both or neither, in either mode).  The residual is rebuilt from the staged (activated, bf16) operand: exact
 * for values >= 0, to 2^-9 relative below.  V2W_E_ARG: a NULL tensor or weight pointer of a branch in use, half an affine, nbr outside
 * 1 .. 3, a mode other than 0 / 1, slope <= 0.  V2W_E_SHAPE: shape not served (the caller issues the per-layer launches instead). */
typedef struct {
    const void* in[3];
    const float* in_a; const float* in_s;
    const void* wps[3]; const float* bias[3];
    void* out[3];
    int32_t k[3], dil[3];
    int32_t nbr, mode, B, C, L;
    float slope, out_div;
    int32_t _pad;
} v2w_branch_convs_args;
int v2w_branch_convs_bf16_fwd(const v2w_branch_convs_args* a, void* stream);

/* ---- K2: fused leaky_relu -> ConvTranspose1d(k, stride u, padding (k-u)/2) -> +bias
 * (models.py:128-129).  in (B, C_in, L) -> out (B, C_out, L*u); requires (k-u) even and >= 0. */
typedef struct {
    const float* in; const float* wf; const float* wp; const float* bias; float* out;
    float* stats_part;  /* optional (MFMA path only): [ntiles][C_out][2] per-tile (sum, sumsq) of the output, the fused form of
                         * v2w_bn_stats; ntiles = cfg[9] of v2w_convt1d_tile_config; reduce with v2w_bn_reduce_partials */
    int32_t B, C_in, C_out, L, k, u;
    float   slope;
    int32_t algo;
    int32_t io_bf16;    /* v2w_convt1d_bf16_fwd only (else 0): bit 0 `in` is bf16, bit 1 `out` is bf16 (see v2w_conv1d_args) */
    int32_t _pad;
    float*  splitk_ws;  /* v2w_convt1d_fwd only: caller-owned split-over-C_in scratch, as in v2w_conv1d_args (NULL: unsplit) */
    int64_t splitk_ws_bytes;
} v2w_convt1d_args;
int v2w_convt1d_fwd(const v2w_convt1d_args* a, void* stream);
long long v2w_convt1d_splitk_ws_bytes(const v2w_convt1d_args* a);   /* as v2w_conv1d_splitk_ws_bytes */

/* bf16 counterpart (V2W_ALGO_BF16 arithmetic: bf16 operands, fp32 accumulate - BASELINE configs[2]) of v2w_convt1d_fwd for the
 * transposed convs of models.py:128-129.  The transposed conv runs as a Conv1d over UP * C_out virtual output channels on the bf16
 * matrix pipe (csrc/v2w_conv_bf16.hip); `a->wp` must point at the fragments of v2w_pack_bf16_convt (a->wf is ignored), `a->stats_part`
 * (optional) receives [v2w_convt1d_bf16_tiles(a)][C_out][2] partial (sum, sumsq) for v2w_bn_reduce_partials.
 * C_in % 32 == 0, u in 2..8, (k - u) even; V2W_E_SHAPE otherwise. */
int       v2w_pack_bf16_convt(const float* wf, void* wps, int k, int c_in, int c_out, int u, void* stream);
long long v2w_pack_bf16_convt_bytes(int k, int c_in, int c_out, int u);   /* size of `wps`; 0 = unsupported shape */
int       v2w_convt1d_bf16_fwd(const v2w_convt1d_args* a, void* stream);
int       v2w_convt1d_bf16_tiles(const v2w_convt1d_args* a);               /* rows of stats_part (host-only query) */

/* Introspection for profiling: which conv_tile_kernel<MF,U,MI,NI,WM,WN,CK,NPF,RING> instantiation the MFMA path uses for
 * this problem (only the sizes of `a` are read).  0 and cfg[10] filled (cfg[9] = number of position tiles), or V2W_E_SHAPE
 * when the direct kernel would run. */
int v2w_conv1d_tile_config(const v2w_conv1d_args* a, int32_t* cfg);
int v2w_convt1d_tile_config(const v2w_convt1d_args* a, int32_t* cfg);
/* The same for the V2W_ALGO_BF16 kernels: cfg[10] = MI, NI, WM, WN, NPF, EPI, IN_BF, OUT_BF, CK, VEC of the conv_bf16_kernel
 * instantiation a launch of these n (<= 4) problems / this transposed conv would run (sizes, io_bf16 and the alignment of `in` are
 * read; nothing is dereferenced).  V2W_E_SHAPE when the bf16 kernels do not take the shape. */
int v2w_conv1d_bf16_config(const v2w_conv1d_args* a, int n, int32_t* cfg);
int v2w_convt1d_bf16_config(const v2w_convt1d_args* a, int32_t* cfg);

/* ---- K3: per-stage conditioning  z = fcs[i](cat(spk, noise))  (models.py:120,131), legacy
 * spectral_norm power iteration on cbns[i].layer (modules.py:16,24) and [gamma|beta] = (W/sigma) z + b.
 * One call serves every stage (they depend on spk/noise only).  Arrays of n_stages DEVICE pointers are
 * passed by value inside the struct (HOST struct).
 *   spk (B, spk_dim), noise (B, noise_dim); fc_w[i] (128, spk_dim+noise_dim), fc_b[i] (128)
 *   sn_w[i] (2C_i, 128) = weight_orig, sn_b[i] (2C_i), sn_u[i] (2C_i), sn_v[i] (128)
 *   training != 0: one power iteration, u and v are UPDATED IN PLACE (as the reference's hook does)
 *   gb[i] (B, 2C_i): gamma = gb[:, :C], beta = gb[:, C:]   (chunk(2,1), modules.py:24)
 *   z_ws: workspace of n_stages*B*128 floats; sigma_ws: n_stages floats
 *   fc_w[i] == fc_b[i] == NULL: no fcs layer, z = cat(spk, noise) itself (needs spk_dim+noise_dim == 128;
 *   noise may be NULL with noise_dim == 0) - ConditionalBatchNorm1d.forward(inputs, noise) used on its own. */
#define V2W_MAX_STAGES 8
typedef struct {
    const float* spk; const float* noise;
    const float* fc_w[V2W_MAX_STAGES]; const float* fc_b[V2W_MAX_STAGES];
    const float* sn_w[V2W_MAX_STAGES]; const float* sn_b[V2W_MAX_STAGES];
    float* sn_u[V2W_MAX_STAGES]; float* sn_v[V2W_MAX_STAGES];
    float* gb[V2W_MAX_STAGES];
    int32_t C[V2W_MAX_STAGES];
    float* z_ws; float* sigma_ws;
    int32_t n_stages, B, spk_dim, noise_dim, training;
} v2w_cond_args;
int v2w_cond_gamma_beta(const v2w_cond_args* a, void* stream);
/* The spectral-norm half alone (ABI v28): sigma_ws[i] = u_i . (W_i v_i) of every stage (training != 0: after the power iteration, u / v
 * updated in place).  Read: sn_w, sn_u, sn_v, C, n_stages, training, sigma_ws.  In eval mode sigma is a function of the parameters only. */
int v2w_cond_sigma(const v2w_cond_args* a, void* stream);
/* Eval mode (ABI v28), one launch for every stage: from (spk, noise) straight to the folded per-sample affine of the Conditional BatchNorm
 * with its RUNNING statistics (modules.py:20-30 in eval; models.py:131-133):  z = fcs[i](cat(spk, noise)),
 * [gamma | beta] = (W_i z) / sigma_ws[i] + b_i,  a_out[i][b][c] = gamma / sqrt(running_var[i][c] + eps[i]),
 * s_out[i][b][c] = beta - a_out * running_mean[i][c].  c.sigma_ws must hold v2w_cond_sigma's result for the current parameters;
 * c.gb / c.z_ws / c.sn_u / c.sn_v are not used.  Replaces v2w_cond_gamma_beta + n_stages x v2w_bn_finalize(training = 0). */
typedef struct {
    v2w_cond_args c;
    const float* running_mean[V2W_MAX_STAGES]; const float* running_var[V2W_MAX_STAGES];
    float* a_out[V2W_MAX_STAGES]; float* s_out[V2W_MAX_STAGES];
    float eps[V2W_MAX_STAGES];
} v2w_cond_eval_args;
int v2w_cond_affine_eval(const v2w_cond_eval_args* e, void* stream);

/* ---- K4: BatchNorm1d(affine=False) statistics and finalisation (modules.py:14,23).
 * v2w_bn_stats   : x (B,C,L) -> stats[2C] doubles = [sum_c | sumsq_c] over (B,L); deterministic two-level
 *                  reduction; partial_ws >= 2*C*V2W_BN_SPLITS doubles.
 *                  In data-parallel runs the host all-reduces `stats` (RCCL, sum) between the two calls.
 * v2w_bn_finalize: training: mean/biased var from stats (count = stats[2C]), running_mean/var
 *                  momentum update with the unbiased var, num_batches_tracked += 1 (int64);
 *                  eval: running stats are used, nothing is written.
 *                  Then the folded per-sample affine  a[b,c] = gamma*rstd, s[b,c] = beta - gamma*mean*rstd
 *                  (so that CondBN(x) = a*x + s, modules.py:23-28) from gb (B, 2C). */
#define V2W_BN_SPLITS 64
/* stats: 2C+1 doubles = [sum_c | sumsq_c | count]; count = B*L is written by the kernel so that one
 * all-reduce(sum) of the whole array yields the global sums AND the global element count. */
int v2w_bn_stats(const float* x, double* stats, double* partial_ws, int B, int C, int L, void* stream);
/* Fixed-order fp64 reduction of the per-tile partials written by v2w_convt1d_fwd(stats_part) -> stats[2C+1].
 * part: [ntiles][C][2] floats, each (sum, sumsq) row entry read as one 8-byte pair: `part` must be 8-byte aligned (here and in
 * v2w_bn_reduce_finalize; every producer's row buffer is). */
int v2w_bn_reduce_partials(const float* part, int ntiles, int C, double count, double* stats, void* stream);
int v2w_bn_finalize(const double* stats, const float* gb,
                    float* running_mean, float* running_var, int64_t* num_batches_tracked,
                    float* a_out, float* s_out, int B, int C, int training,
                    float momentum, float eps, void* stream);
/* v2w_bn_reduce_partials + v2w_bn_finalize(training = 1) as ONE launch (ABI v34; one block per channel: its rows added in the same fixed
 * order, `stats` [2C+1] written as v2w_bn_reduce_partials writes it, then the running statistics and (a, s) of that channel): bit-identical
 * to the two calls.  A data-parallel run, which all-reduces `stats` between them, keeps the two calls. */
int v2w_bn_reduce_finalize(const float* part, int ntiles, double count, const float* gb,
                           float* running_mean, float* running_var, int64_t* num_batches_tracked,
                           double* stats, float* a_out, float* s_out, int B, int C, float momentum, float eps, void* stream);
/* Two-level form for layers with thousands of partial rows (ABI v28; the fused stage kernels write one row per 224 positions):
 * v2w_bn_reduce_slices adds slice s of the rows of `part` ([ntiles][C][2] floats) into slices[s][2 C] fp64 ([sum | sumsq], nslices <= 1024
 * blocks reading whole rows), v2w_bn_finalize_slices is v2w_bn_finalize(training = 1) on those slices, added in slice order, with the element
 * count given.  Deterministic; same values as the one-level form up to the order of the fp64 additions.  Both refuse nslices outside
 * 1 .. 1024 with V2W_E_ARG. */
int v2w_bn_reduce_slices(const float* part, int ntiles, int C, double* slices, int nslices, void* stream);
int v2w_bn_finalize_slices(const double* slices, int nslices, double count, const float* gb,
                           float* running_mean, float* running_var, int64_t* num_batches_tracked,
                           float* a_out, float* s_out, int B, int C, float momentum, float eps, void* stream);

/* ---- K5 (standalone form): out = a[b,c]*x + s[b,c] over (B,C,L).  Only ConditionalBatchNorm1d.forward used on
 * its own (modules.py:20-30) materialises the normalised tensor; Generator.forward folds the affine into its
 * consumers' loads instead.  One grid row per (b, c): B * C <= 65 535, V2W_E_SHAPE otherwise. */
int v2w_affine_apply(const float* x, const float* a, const float* s, float* out, int B, int C, int L, void* stream);

/* ---- backward building blocks (the forward entry points above run dgrad: see v2w_wf_transpose_flip).
 * v2w_wgrad: dwf [k][C_in][C_out] = sum_{b,q} lrelu(x_a*x + x_s)[b,ci,q + off_t] * dy[b,co,u*q + r_t]
 *   Conv1d(k, dil): u = 1 ; ConvTranspose1d(k, stride u, pad (k-u)/2): `dil` ignored, dy is (B, C_out, u*Lq).
 *   x (B, C_in, Lq); slab_ws: v2w_wgrad_slabs(...) * k*C_in*C_out floats (per-split partials, summed in fixed order).
 *   V2W_E_SHAPE unless C_in and C_out are multiples of 16. */
int v2w_wgrad_slabs(int B, int c_in, int c_out, int Lq);
int v2w_wgrad(const float* x, const float* x_a, const float* x_s, const float* dy, float* dwf, float* slab_ws,
              int B, int c_in, int c_out, int Lq, int k, int dil, int u, float slope, void* stream);

/* v2w_wgrad_bf16 (ABI v30): the same Conv1d weight gradient from bf16 OPERANDS, fp32 accumulation - what the reference's autocast backward
 * computes (vec2wav/train.py:167,214: `loss_gen_all.backward()` of a forward run under torch.autocast).  act(x) = lrelu(x_a*x + x_s) is
 * evaluated in fp32 and rounded once.  io_bf16 = 0: x and dy are fp32 tensors (rounded while staged); 3: both are bf16 tensors.
 *   slab_ws: v2w_wgrad_bf16_slabs(...) * k*C_in*C_out floats.  V2W_E_SHAPE (and 0 slabs) unless C_in == C_out in {16, 32} or a multiple of 64,
 *   k odd <= 11, Lq % 8 == 0 and the halo (k-1)/2*dil fits the staged tile: the caller runs v2w_wgrad then. */
int v2w_wgrad_bf16_slabs(int B, int c_in, int c_out, int Lq, int k);
int v2w_wgrad_bf16(const void* x, const float* x_a, const float* x_s, const void* dy, float* dwf, float* slab_ws,
                   int B, int c_in, int c_out, int Lq, int k, int dil, float slope, int io_bf16, void* stream);

/* Conditional BatchNorm backward (modules.py:20-30).  Given dx = dL/d(gamma*xhat+beta) and xr (the BN input):
 *   v2w_cbn_bwd_sums : dgb (B, 2C) = [dgamma | dbeta] and csum[2C] fp64 = [sum_b gamma*dbeta | sum_b gamma*dgamma]
 *                      (a data-parallel run all-reduces csum between the two calls); s12_ws: 2*B*C floats.
 *   v2w_cbn_bwd_apply: dxr = A*dx + Bc*xr + Cc  (train: full BatchNorm backward with batch statistics `stats` = the
 *                      forward's [sum|sumsq|count]; eval: dxr = gamma*rstd*dx); tab_ws: B*C + 2C floats. */
int v2w_cbn_bwd_sums(const float* dx, const float* xr, const float* gb, const double* stats,
                     const float* running_mean, const float* running_var, float* s12_ws, float* dgb, double* csum,
                     int B, int C, int L, int training, float eps, void* stream);
int v2w_cbn_bwd_apply(const float* dx, const float* xr, const float* gb, const double* stats, const double* csum,
                      const float* running_mean, const float* running_var, float* tab_ws, float* dxr,
                      int B, int C, int L, int training, float eps, void* stream);
/* tanh + conv_post backward (models.py:143-145): dp = dy*(1-y^2) (dp_ws: B*L floats; its sum is d conv_post.bias),
 * dx = lrelu'(x) * conv_post^T(dp), dwf [k][C_in][1]; part_ws: C_in*k*512 doubles (ABI v32: the one-pass kernel for C_in = 16, k = 7 writes one
 * row of partial weight gradients per persistent workgroup; 64 rows before). */
int v2w_tail_bwd(const float* dy, const float* y, const float* x, const float* wf, float* dp_ws, double* part_ws,
                 float* dx, float* dwf, int B, int C_in, int L, int k, float slope, void* stream);
/* weight-norm backward: (dwf [k][C_in][C_out], v, g) -> dv (v's layout), dg; g == NULL: dv = dw relayouted, dg untouched. */
int v2w_wn_bwd(const float* dwf, const float* v, const float* g, float* dv, float* dg,
               int c_in, int c_out, int k, int transposed, void* stream);
/* conditioning backward of one stage: dgb (B,2C) -> d weight_orig (2C,128), d layer.bias (2C), d fcs.weight (128,D), d fcs.bias;
 * z (B,128) and sigma are the forward's; dz_ws: B*128 + 1 floats. */
int v2w_cond_bwd(const float* dgb, const float* z, const float* sn_w, const float* sn_u, const float* sn_v, const float* sigma,
                 const float* spk, const float* noise, float* d_sn_w, float* d_sn_b, float* d_fc_w, float* d_fc_b,
                 float* dz_ws, int B, int C, int spk_dim, int noise_dim, void* stream);

/* ---- K8: leaky_relu(slope) -> Conv1d(C_in -> 1, k, pad (k-1)/2) -> +bias -> tanh  (models.py:143-145).
 * in (B, C_in, L) -> out (B, 1, L); wf [k][C_in][1]. */
/* the same with a bf16 input tensor (bf16 activation storage of BASELINE configs[2]); output stays fp32 */
int v2w_conv_post_tanh_bf16in(const void* x_bf16, const float* wf, const float* bias, float* out,
                              int B, int c_in, int L, int k, float slope, void* stream);
int v2w_conv_post_tanh(const float* in, const float* wf, const float* bias, float* out,
                       int B, int C_in, int L, int k, float slope, void* stream);

/* ---- Batches of unequal lengths (additive entry points; the argument structs above are unchanged).  `len` is a DEVICE array of B int32 and
 * len_mul >= 1: item b's sequence ends at Lb = len[b] * len_mul positions of the call's INPUT rate (clamped to L).  Inputs at or past Lb count
 * as zero padding after the activation, whatever the tensor holds there (stale workspace, NaN); each item computes what its own unpadded
 * call would.  Outputs at or past Lb (Lb * u for a transposed conv) are unspecified and workgroups whose outputs all lie there return at once -
 * except in the generator's last layer (the stage kernel's fused tail, v2w_conv_post_tanh_len), which stores exactly 0 there.  The grids do not
 * depend on the values.  V2W_E_ARG: len == NULL, len_mul < 1, or a call these kernels do not serve - any algorithm but V2W_ALGO_AUTO / _MFMA /
 * _WINO (no direct-kernel fallback), mask_src / rowsum_part / out_slope / channel slices / in_stride > 1, stats_part, the input-gradient form. */
int v2w_conv1d_fwd_len(const v2w_conv1d_args* a, int n, const int32_t* len, int len_mul, void* stream);   /* n <= 4 problems as _fwd_multi */
int v2w_convt1d_fwd_len(const v2w_convt1d_args* a, const int32_t* len, int len_mul, void* stream);
/* The second convs of a ResBlock2 stage's branches as ONE Winograd launch on one accumulator (additive in ABI v35; fp32; the f32 counterpart
 * of v2w_branch_convs_bf16_fwd mode 1).  a[0 .. n), n <= 3, are the SOURCES: of each, `in` (B, C, L), `wp` (its v2w_pack_wino / fold `wpw`
 * stream), `bias`, `k`, `dil`, `slope`; C_in == C_out, and B, C, L, dil and slope are shared.  `out` and `out_div` are a[0]'s.  Every source's
 * input is also its residual:
 *     out = ((y + ((b_0 + b_1) + b_2)) + ((in_0 + in_1) + in_2)) / out_div,   y = sum_j conv_j(lrelu(in_j)) from the shared accumulators
 * (the division as in v2w_conv1d_fwd; a different rounding order from three convs that add r_0, r_1, r_2).  res / add0 / add1 / accumulate
 * must be unset (V2W_E_ARG).  len == NULL: full lengths; else as v2w_conv1d_fwd_len.  V2W_E_SHAPE (nothing launched): an input affine
 * (in_a), dilations that differ, an even k, C % 64 != 0, and whatever V2W_ALGO_WINO declines but a small launch - the caller then issues
 * the convs one by one. */
int v2w_conv1d_wino_sum_fwd(const v2w_conv1d_args* a, int n, const int32_t* len, int len_mul, void* stream);
/* The same with the order given in which a workgroup walks the sources: `order` (host memory) is a permutation of 0 .. n - 1 (V2W_E_ARG
 * otherwise), NULL leaves the choice to the library (v2w_conv1d_wino_sum_fwd).  The order changes only the order in which the sources'
 * products are accumulated; bias and residual sums keep the association above, by source index.  v2w_wino_sum_order: the library's
 * choice for sources of kernel sizes k[0 .. n), n <= 3 (host only, launches nothing).  New symbols over unchanged structs. */
int v2w_conv1d_wino_sum_fwd_order(const v2w_conv1d_args* a, int n, const int32_t* len, int len_mul, const int32_t* order, void* stream);
int v2w_wino_sum_order(const int32_t* k, int n, int32_t* order);
/* The FIRST convs of a ResBlock2 stage's branches as ONE Winograd launch that stages their common input once per tile (additive in ABI v35;
 * fp32).  a[0 .. n), n <= 3, are convs over the same input: they share `in`, `in_a` / `in_s`, `res`, `res_a` / `res_s`, B, C_in, C_out, L,
 * `dil` and `slope` (V2W_E_ARG otherwise, and for two problems with one `out`); each has its own `wp` (v2w_pack_wino / fold `wpw` stream),
 * `bias`, `k` and `out`:
 *     out_j = conv_j(lrelu(in_a * in + in_s)) + bias_j [+ (res_a * res + res_s)]
 * with the operations of the V2W_ALGO_WINO launch of a[j] alone, in its order: the same bits.  V2W_E_SHAPE (nothing launched; the caller
 * issues v2w_conv1d_fwd_multi): C_in > 64 (the kernel's two chunk buffers must hold the whole input window), add0 / add1 / accumulate /
 * out_div set, and whatever V2W_ALGO_WINO declines but a small launch.  No per-item lengths.  A new symbol over unchanged structs. */
int v2w_conv1d_wino_fan_fwd(const v2w_conv1d_args* a, int n, void* stream);
/* The upsampler form of the Winograd kernel: out = ConvTranspose1d(lrelu(in_a * in + in_s)) + bias for k == 2 u run as ONE two-tap Conv1d
 * over u * C_out rows and a pixel shuffle, 3 products per output pair and row where v2w_convt1d_fwd issues 4.  a->wp = the layer's fold
 * `wpw` stream (v2w_fold_desc); in_a / in_s (B, C_in): optional per-(item, channel) affine in front of the leaky_relu (both or neither);
 * a->stats_part (optional): [v2w_convt1d_wino_tiles(a)][C_out][2] per-tile (sum, sumsq) of the stored values for v2w_bn_reduce_partials.
 * a->wf, algo, splitk_ws are not read.  Served: u in {2, 4}, C_in % 32 == 0 and >= 64, u * C_out % 64 == 0, any B and L; V2W_E_SHAPE
 * otherwise (nothing launched).  The values differ from v2w_convt1d_fwd's in the last bits (other products, other rounding order).
 * v2w_convt1d_wino_tiles (host-only; only the sizes of `a` are read): the launch's position tiles, and in *wgs (optional) its workgroups. */
int v2w_convt1d_wino_fwd(const v2w_convt1d_args* a, const float* in_a, const float* in_s, void* stream);
int v2w_convt1d_wino_tiles(const v2w_convt1d_args* a, int32_t* wgs);
int v2w_resblock2_stage_fwd_len(const v2w_stage_args* a, const int32_t* len, int len_mul, void* stream);
int v2w_conv_post_tanh_len(const float* in, const float* wf, const float* bias, float* out,
                           int B, int C_in, int L, int k, float slope, const int32_t* len, int len_mul, void* stream);

/* ---- mel_spectrogram of the generated audio (vec2wav/dataset.py:53-77, train.py:172-174,266-269).
 * The STFT itself is a Conv1d over the hop-phase de-interleaved signal and runs through v2w_conv1d_fwd (hop input channels,
 * n_fft/hop taps, pad_left = 0, windowed DFT rows as weights: see wavthruvec_pytorch_amd/mel.py); these are its two ends:
 *   v2w_mel_phases: y (B, L) -> xp (B, hop, FP), xp[b][p][f] = reflect_pad(y, pad)[f*hop + p] (0 past the padded signal)
 *   v2w_mel_finish: spec (B, Cs, FP) (rows [0,nb) = Re, [nb,2nb) = Im), basis (n_mels, nb) -> out (B, n_mels, F) =
 *                   log(clamp(basis @ sqrt(Re^2 + Im^2 + 1e-9), 1e-5))                                    (dataset.py:31-41,72-75) */
int v2w_mel_phases(const float* y, float* xp, int B, int L, int hop, int pad, int FP, void* stream);
int v2w_mel_finish(const float* spec, const float* basis, float* out, int B, int Cs, int FP, int F, int nb, int n_mels, void* stream);
/* Their backward (the training loss F.l1_loss(y_mel, mel_spectrogram(y_g_hat)) back-propagates through it, train.py:172-174,204):
 *   v2w_mel_finish_bwd: gout (B, n_mels, F), the forward's spec, basis and basisT (nb, n_mels) -> dspec (B, Cs, FP); the caller
 *                       zero-fills dspec (pad rows and frames >= F are not written).  d log(clamp(x, 1e-5)) = 1/x for x >= 1e-5.
 *   v2w_mel_phases_bwd: dxp (B, hop, FP) -> dy (B, L): every sample sums the padded positions that read it (reflections fold back).
 * Between them the DFT conv's input gradient is v2w_conv1d_fwd with the tap-flipped transposed weights and pad_left = k - 1.
 * V2W_E_ARG: a NULL operand, B <= 0, L <= 1, hop <= 0, pad < 0, pad >= L (the reflection needs more than pad samples), FP <= 0 (phases);
 * F <= 0, FP < F, nb <= 0, Cs < 2 * nb, n_mels <= 0 (finish).  V2W_E_SHAPE, nothing launched: B > 65535 (the grid's second dimension); hop * FP
 * or L + 2 * pad past 2^31 - 1 (the phase calls index with int: the largest each takes is 2^31 - 1); nb > 1024 (v2w_mel_finish, _len) or nb + n_mels > 1024 (v2w_mel_finish_bwd):
 * 64 bytes of LDS per bin, and per mel in the backward, of 64 KiB; n_mels * 16 past 2^31 - 1; F * hop + n_fft past 2^31 - 1 (v2w_mel_finish_len). */
int v2w_mel_finish_bwd(const float* spec, const float* basis, const float* basisT, const float* gout, float* dspec,
                       int B, int Cs, int FP, int F, int nb, int n_mels, void* stream);
int v2w_mel_phases_bwd(const float* dxp, float* dy, int B, int L, int hop, int pad, int FP, void* stream);
/* The two ends for a batch of unequal lengths (additive; forward only; `len` / len_mul as under "Batches of unequal lengths" above: item b
 * holds Lb = min(len[b] * len_mul, L) samples, whatever y[b, Lb:] holds - NaN, Inf, stale workspace - reaches no stored value, the grids do
 * not depend on the values).  With n_fft = 2 * pad + hop (a multiple of hop) and k = n_fft / hop, item b has
 *   F_b = (Lb + 2 * pad - n_fft) / hop + 1 frames if Lb > pad (reflect padding needs more than pad samples) and Lb + 2 * pad >= n_fft, else 0.
 *   v2w_mel_phases_len: xp[b][p][f] = ypad_b[f * hop + p], ypad_b = y[b, :Lb] reflected about ITS ends (index 0 and index Lb - 1): the bits
 *                       of a B = 1 v2w_mel_phases call on y[b, :Lb] over that call's roundup4(F_b + k - 1) columns; exactly 0 in the columns
 *                       past them (no frame of the item reads those) and past Lb + 2 * pad; all 0 for an item with F_b = 0.  No load
 *                       address is at or past Lb within row b.
 *   v2w_mel_finish_len: (takes no L: F_b is clamped to F = the frames of L) frames f < F_b as v2w_mel_finish computes them (same operations in the same order); frames F_b <= f < F store
 *                       exactly 0.0 - the zero padding of a padded target mel (dataset.py:194-218), not log(1e-5).  A workgroup (16 frames)
 *                       whose frames all lie at or past F_b stores its zeros without reading spec.
 * The DFT conv between them is v2w_conv1d_fwd on the whole xp as before: an item's F_b + k - 1 columns are no integer multiple of len[b],
 * so v2w_conv1d_fwd_len does not apply and no tile is skipped.  V2W_E_ARG as the plain calls, and for len == NULL, len_mul < 1,
 * (2 * pad) % hop != 0 (phases) or n_fft % hop != 0 / n_fft < hop / n_fft - hop odd (finish). */
int v2w_mel_phases_len(const float* y, float* xp, int B, int L, int hop, int pad, int FP, const int32_t* len, int len_mul, void* stream);
int v2w_mel_finish_len(const float* spec, const float* basis, float* out, int B, int Cs, int FP, int F, int nb, int n_mels,
                       const int32_t* len, int len_mul, int hop, int n_fft, void* stream);
/* Any frame geometry: 1 <= hop <= n_fft, 1 <= win <= n_fft.  The calls above keep their conditions and their bits: they are the calls below at
 * win = n_fft = 2 * pad + hop, left = 0, CP = hop, k = ceil(n_fft / hop), on the same kernels.  The caller
 * states every quantity; nothing is derived from another: pad samples of reflection per side (mel_spectrogram: (n_fft - hop) / 2 rounded
 * down), left = (n_fft - win) / 2 zero weights before the window, k = ceil(win / hop) taps, CP >= hop channels (rounded up to the tile
 * kernel's channel block), FP >= F + k - 1 columns.  Frame f multiplies the window's support only, ypad[f * hop + left + t] for t < win,
 * so the DFT conv (v2w_conv1d_fwd, pad_left = 0) has k taps over CP channels and weights [j][p][c] = Wd[c][left + j * hop + p] for
 * p < hop and j * hop + p < win, else 0.
 *   v2w_mel_phases_geo:     y (B, L) -> xp (B, CP, FP): xp[b][p][f] = reflect_pad(y, pad)[f * hop + left + p] for p < hop where that index
 *                           is below L + 2 * pad, else exactly +0.0 (the channels [hop, CP), the columns past the padded signal).
 *   v2w_mel_phases_geo_len: item b holds Lb = min(len[b] * len_mul, L) samples and F_b = (Lb + 2 * pad - n_fft) / hop + 1 frames if Lb > pad
 *                           and Lb + 2 * pad >= n_fft, else 0: the bits of the B = 1 v2w_mel_phases_geo call on y[b, :Lb] over that call's
 *                           roundup4(F_b + k - 1) columns, +0.0 in the columns past them.  No load address is at or past Lb within row b.
 *   v2w_mel_phases_geo_bwd: dxp (B, CP, FP) -> dy (B, L): the sample's own position s + pad, then its left reflection pad - s
 *                           (1 <= s <= pad), then its right one 2 (L - 1) - s + pad (L - 1 - pad <= s <= L - 2), added in that order; the
 *                           padded position i is dxp[b][(i - left) % hop][(i - left) / hop] for 0 <= i - left < hop * FP and 0 elsewhere.
 *   v2w_mel_finish_geo, _geo_bwd: v2w_mel_finish and v2w_mel_finish_bwd for every nb: where those fit their 16 frames per workgroup into
 *                           64 KiB of LDS, their launch (the same kernel, the same bits); otherwise 8 frames per workgroup (nb = 1025:
 *                           n_fft 2048), every output the same operations in the same order.
 *   v2w_mel_finish_geo_len: v2w_mel_finish_len with pad = (n_fft - hop) / 2 rounded down and no condition on n_fft % hop or its parity.
 * V2W_E_ARG: a NULL operand, B <= 0, L <= 1, hop < 1, n_fft < hop, win < 1, win > n_fft, CP < hop, pad < 0, pad >= L, left < 0,
 * left + win > n_fft, k < 1, k * hop < win, FP <= 0; len == NULL or len_mul < 1; the finish calls' own.  V2W_E_SHAPE: B > 65535; CP * FP,
 * hop * FP + left or L + 2 * pad past 2^31 - 1; nb > 2048 (finish, _len) or nb + n_mels > 2048 (backward); F * hop + n_fft past 2^31 - 1 (_len). */
int v2w_mel_phases_geo(const float* y, float* xp, int B, int L, int n_fft, int win, int hop, int CP, int pad, int left, int k, int FP,
                       void* stream);
int v2w_mel_phases_geo_len(const float* y, float* xp, int B, int L, int n_fft, int win, int hop, int CP, int pad, int left, int k, int FP,
                           const int32_t* len, int len_mul, void* stream);
int v2w_mel_phases_geo_bwd(const float* dxp, float* dy, int B, int L, int n_fft, int win, int hop, int CP, int pad, int left, int k, int FP,
                           void* stream);
int v2w_mel_finish_geo(const float* spec, const float* basis, float* out, int B, int Cs, int FP, int F, int nb, int n_mels, void* stream);
int v2w_mel_finish_geo_len(const float* spec, const float* basis, float* out, int B, int Cs, int FP, int F, int nb, int n_mels,
                           const int32_t* len, int len_mul, int hop, int n_fft, void* stream);
int v2w_mel_finish_geo_bwd(const float* spec, const float* basis, const float* basisT, const float* gout, float* dspec,
                           int B, int Cs, int FP, int F, int nb, int n_mels, void* stream);
/* Fused mel L1 training loss (additive; train.py:172-176,204: F.l1_loss(y_mel, mel_spectrogram(y_g_hat)) and its backward), with or
 * without per-item lengths.  The forward's first two steps are the existing ones (v2w_mel_phases / _len / _geo / _geo_len, then the DFT conv);
 * the calls below replace v2w_mel_finish + an L1 and their backwards: the (B, n_mels, F) mel is never stored.
 * tgt is the padded target, DENSE: (B, Ft, n_mels) read with (ts_f, ts_m) = (n_mels, 1), or (B, n_mels, Ft) with (ts_f, ts_m) = (1, Ft);
 * it is never written.  len == NULL: every item counts F_b = F frames (Ft >= F).  len a DEVICE array of B int32 (len_mul >= 1, "Batches of
 * unequal lengths"): F_b = min(frames(len[b] * len_mul), F, Ft), frames(n) as v2w_mel_finish_geo_len states it (pad = (n_fft - hop) / 2 rounded
 * down).  With v[b][m][f] = logf(fmaxf(acc, 1e-5f)) as v2w_mel_finish[_geo] computes it (the same operations in the same order):
 *   v2w_mel_loss_plan  host only: tiles = ceil(F / 16), or ceil(F / 8) where 16 frames of nb bins pass 64 KiB of LDS (as v2w_mel_finish_geo
 *                      chooses); *scratch_bytes (may be NULL) = B * tiles * 8, the size of ws.  Returns tiles > 0 or a V2W_E_* code.
 *   v2w_mel_loss_fwd   launch 1, grid (tiles, B): workgroup (g, b) adds |v - t| (one fp32 rounding each) over its frames f < F_b in fp64 -
 *                      a thread's entries in index order, then the fixed-order workgroup reduction - and writes ONE partial ws[b * tiles + g];
 *                      a workgroup at or past F_b writes 0.0 and reads nothing.  Launch 2, one workgroup: item b's partials are added in
 *                      index order, S_b, and the items' sums in a fixed order:
 *                        per_item[b] = S_b / (n_mels * F_b), 0 for F_b = 0                      (B floats; may be NULL)
 *                        total[0]    = scale * sum_b S_b / (n_mels * sum_b F_b)                 (may be NULL)
 *                        coef[0]     = scale / (n_mels * sum_b F_b)                             (may be NULL: the backward's factor)
 *                      total and coef are 0 when no item has a frame.  No atomics: the same call gives the same bits, an item's per_item
 *                      depends on no other item, and the frame counts never come to the host.
 *   v2w_mel_loss_bwd   v2w_mel_finish_geo_bwd with d_acc = (gout[0] * coef[0]) * sgn(v - t) / acc where f < F_b and acc >= 1e-5f, else 0
 *                      (sgn(0) = 0); gout and coef are DEVICE floats.  dspec is zero-filled by the caller: only rows < 2 * nb of the frames
 *                      f < F_b are written.
 * spec frames and target entries at or past F_b are never loaded (selects, not multiplies): NaN or Inf there reaches nothing.
 *   v2w_mel_phases_len_bwd, v2w_mel_phases_geo_len_bwd: v2w_mel_phases_bwd / v2w_mel_phases_geo_bwd for item b of Lb = min(len[b] * len_mul, L)
 *                      samples and F_b = frames(Lb): the right reflection is about the item's own last sample (2 (Lb - 1) - s + pad for
 *                      Lb - 1 - pad <= s <= Lb - 2), the columns from the item's own roundup4(F_b + k - 1) on read as 0 whatever they
 *                      hold, dy[b, Lb:] = +0.0, and an item with F_b = 0 is all +0.0.  The three additions keep their order:
 *                      dy[b, :Lb] has the bits of the B = 1 plain call on a dense copy of dxp[b, :, :roundup4(F_b + k - 1)].
 * V2W_E_ARG: a NULL operand (per_item, total, coef: all three NULL), ws not 8-byte aligned, scale NaN, Ft <= 0, (ts_f, ts_m) neither of the
 * two dense layouts, len == NULL and Ft < F, len != NULL and len_mul < 1 / hop < 1 / n_fft < hop, and the cases of v2w_mel_finish_geo[_bwd]
 * and of v2w_mel_phases_len / _geo_len.  V2W_E_SHAPE: theirs (B > 65535, nb > 2048 or nb + n_mels > 2048 in the backward, F * hop + n_fft
 * past 2^31 - 1) and n_mels * Ft past 2^31 - 1. */
int v2w_mel_loss_plan(int B, int F, int nb, int n_mels, long long* scratch_bytes);
int v2w_mel_loss_fwd(const float* spec, const float* basis, const float* tgt, int ts_f, int ts_m,
                     int B, int Cs, int FP, int F, int Ft, int nb, int n_mels,
                     const int32_t* len, int len_mul, int hop, int n_fft, float scale,
                     float* per_item, float* total, float* coef, void* ws, void* stream);
int v2w_mel_loss_bwd(const float* spec, const float* basis, const float* basisT, const float* tgt, int ts_f, int ts_m,
                     const float* gout, const float* coef, float* dspec,
                     int B, int Cs, int FP, int F, int Ft, int nb, int n_mels,
                     const int32_t* len, int len_mul, int hop, int n_fft, void* stream);
int v2w_mel_phases_len_bwd(const float* dxp, float* dy, int B, int L, int hop, int pad, int FP, const int32_t* len, int len_mul, void* stream);
int v2w_mel_phases_geo_len_bwd(const float* dxp, float* dy, int B, int L, int n_fft, int win, int hop, int CP, int pad, int left, int k,
                               int FP, const int32_t* len, int len_mul, void* stream);

/* ---- MPD / MSD discriminator forwards (models.py:158-275): the memory-bound ends; the convolutions run
 * through v2w_conv1d_fwd (in_ct / out_ct for groups, out_slope for the activated feature maps, dil = period for the (k, 1) Conv2d).
 *   v2w_phase_split: x (B, C, L, inner) -> out (B, s*C, ceil(L/s), inner), out[b][((c/Cg)*s + r)*Cg + c%Cg][u][w] = x[b][c][s*u + r][w]
 *                    (0 past L): a stride-s conv becomes a stride-1 conv over the stacked phases (Cg = channels per group).
 *   v2w_unfold1:     x (B, T) read as (H, inner) rows, reflect-padded on the right to H*inner (models.py:176-181) ->
 *                    out (B, rows, U*inner), out[b][j][u*inner + w] = xpad[(s*u + j - pad)*inner + w], U = (H + 2 pad - k)/s + 1,
 *                    rows >= k (the extra rows are 0): the C_in = 1 layers as 1-tap convs over `rows` channels.
 *   v2w_avgpool4:    AvgPool1d(4, 2, padding=2) (models.py:255-258): x (B, L) -> out (B, L/2 + 1). */
int v2w_phase_split(const float* x, float* out, int B, int C, int Cg, int L, int inner, int s, int ipitch, int opitch, void* stream);
int v2w_unfold1(const float* x, float* out, int B, int T, int H, int inner, int s, int k, int pad, int rows, int opitch, void* stream);
/* Row pitches (floats between consecutive channel rows; 0 = dense): the f32 MFMA kernel's float4 staging needs rows that are
 * multiples of 4 floats, so the discriminators keep (B, C, pitch) buffers with pitch = roundup4(length), run the convs at
 * L = pitch and return the feature maps as [:, :, :length] views.  The tail positions come out of a conv as ordinary
 * positions; v2w_zero_tail restores the zero padding before a stride-1 conv reads that buffer directly. */
int v2w_zero_tail(float* x, long long rows, int pitch, int valid, void* stream);
/* x (B, C, L, inner) -> out (B, k*C, U, inner), out[b][j*C + c][u][w] = x[b][c][s*u + j - pad][w] (0 outside), U = (L + 2 pad - k)/s + 1:
 * a short strided conv (DiscriminatorP: k = 5, stride 3) as one 1-tap conv over k*C channels with the reference's exact MAC count. */
int v2w_unfold_taps(const float* x, float* out, int B, int C, int L, int inner, int s, int k, int pad, int ipitch, int opitch, void* stream);
int v2w_avgpool4(const float* x, float* out, int B, int L, void* stream);

/* ---- discriminator backward (train.py:188-215 differentiates through MPD / MSD in both optimisation steps).  Input gradients of
 * the convs run through v2w_conv1d_fwd with v2w_wf_transpose_flip weights; weight gradients through v2w_wgrad_slice:
 *   v2w_wgrad_slice: v2w_wgrad for a Conv1d whose taps sit at offsets (t - tap0)*dil (tap0 = -1: symmetric) on channel slices:
 *                    x / dy point at the first channel of a c_in / c_out slice of tensors with x_ct / dy_ct channels per batch
 *                    item (0: dense).  slab_ws as for v2w_wgrad.
 *   v2w_disc_dz:     dz = (g + d) * lrelu'(f) over `rows` rows of `pitch` floats ([valid, pitch) = 0): f the ACTIVATED feature map,
 *                    g the gradient that arrived on the returned map (dense rows x valid, or NULL), d the next conv's input
 *                    gradient (pitched, or NULL); slope = 1: no activation (conv_post).
 *   v2w_phase_merge: inverse of v2w_phase_split (gradient of the stacked phases back to (B, C, L, inner)).
 *   v2w_fold1:       backward of v2w_unfold1: dxu (B, rows, ipitch) -> dx (B, T), the reflected tail folded back.
 *   v2w_avgpool4_bwd: backward of v2w_avgpool4: dout (B, L/2 + 1) -> dx (B, L).
 *   v2w_cout1_wgrad: weight gradient of a C_out = 1 conv: dwf [k][C] = sum_{b,l} x[b][c][l + (t - tap0)*dil] * dz[b][l]. */
int v2w_wgrad_slice(const float* x, const float* dy, float* dwf, float* slab_ws, int B, int c_in, int c_out, int Lq,
                    int k, int dil, int tap0, int x_ct, int dy_ct, void* stream);
/* every group of a grouped Conv1d in one launch per tap group (grid.z = group): x (B, G*c_in, Lq), dy (B, G*c_out, Lq),
 * dwf [G][k][c_in][c_out]; slab_ws: G * v2w_wgrad_group_slabs(B, c_in, c_out, Lq, G) * k*c_in*c_out floats (the position splits
 * that fill the GPU are shared out over the G groups of the launch) */
int v2w_wgrad_group_slabs(int B, int c_in, int c_out, int Lq, int ngroups);
int v2w_wgrad_groups(const float* x, const float* dy, float* dwf, float* slab_ws, int B, int c_in, int c_out, int Lq,
                     int k, int dil, int tap0, int ngroups, void* stream);
/* rowsum (optional, one float per row): the sum of each dz row, produced by the same pass; v2w_rowsum_reduce adds them over the
 * batch items (fp64, fixed order) into the bias gradient db (C). */
int v2w_disc_dz(const float* f, const float* g, const float* d, float* dz, float* rowsum, long long rows, int pitch, int valid, float slope,
                void* stream);
int v2w_rowsum_reduce(const float* rowsum, float* db, int B, int C, void* stream);
/* v2w_disc_dz with d in the phase-stacked form dxs (B, s*C, dpitch) of the strided layer above (v2w_phase_merge folded in) */
int v2w_disc_dz_merge(const float* f, const float* g, const float* dxs, float* dz, float* rowsum, int B, int C, int Cg, int L, int inner,
                      int s, int dpitch, int pitch, float slope, void* stream);
int v2w_phase_merge(const float* dxs, float* out, int B, int C, int Cg, int L, int inner, int s, int ipitch, int opitch, void* stream);
int v2w_fold1(const float* dxu, float* dx, int B, int T, int H, int inner, int s, int k, int pad, int rows, int ipitch, void* stream);
int v2w_avgpool4_bwd(const float* dout, float* dx, int B, int L, void* stream);
int v2w_cout1_wgrad(const float* x, const float* dz, float* dwf, int B, int C, int L, int k, int dil, int tap0, void* stream);

/* ---- GAN training losses (additive in ABI v35; models.py:278-310 feature_loss / discriminator_loss / generator_loss and the mel term
 * F.l1_loss of train.py:204): the loss values and the gradients that start the backward, forward and backward of a whole call in one
 * launch each (the L1 forward: one streaming launch and one finishing launch).  Up to V2W_LOSS_MAX_ITEMS tensors (pairs) per call; the
 * descriptors are HOST arrays, read before the call returns (as v2w_conv1d_fwd_multi reads its problems).
 *
 * A tensor is `rows` rows of `valid` floats, consecutive rows `pitch` floats apart; floats [valid, pitch) of a row are never read.
 * pitch == valid or pitch == 0: dense, any length and any (4-byte) alignment.  Otherwise pitch % 4 == 0 and the base is 16-byte
 * aligned - the form of the discriminators' feature maps ((B, C, roundup4(U)) buffers returned as [:, :, :U] views, their 4-D
 * (b, C, U, inner) views and the leading-dim halves of a real-plus-generated batch), which are read in place.
 *
 * L1 (feature loss / mel term):
 *   forward   term[i] = mean |a_i - b_i| (n floats, may be NULL), total[0] = scale * sum_i term[i] in list order (may be NULL).
 *             Deterministic: workgroups are dealt to the pairs in proportion to their sizes by a plan that depends on the descriptors
 *             only, each writes one fp64 partial to `scratch`, the finishing launch adds them in index order in fp64; no atomics.
 *   backward  da_i = sgn(a_i - b_i) * ((scale * gout[0]) / numel_i), db_i = -da_i, written DENSE (rows x valid); either may be NULL
 *             (a pair with both NULL is skipped).  sgn = (a > b) - (a < b); the coefficient is the correctly rounded fp32 quotient of
 *             the fp32 product; gout is a DEVICE scalar, read by the kernel.  The forward ignores da / db.
 *   v2w_l1_multi_plan (host only): starts[i] = first workgroup of pair i, starts[n] = workgroups of the streaming launch, which is
 *             also the return value (> 0), at most V2W_L1_TARGET_WGS + n; every pair has at least one.  A pair counts
 *             rows * ceil(valid / 4) units of four floats (both sides dense: ceil((rows * valid + s) / 4), s = floats of `a` past a
 *             16-byte line); chunk = max(2048, ceil(sum of units / V2W_L1_TARGET_WGS)); pair i gets ceil(units_i / chunk) workgroups.
 *   v2w_l1_multi_scratch_bytes (host only): bytes of `scratch` (8-byte aligned) the forward needs: 8 per workgroup.
 * LSGAN terms (numel_i < 2^31, target 0 or 1):
 *   forward   term[i] = mean (target_i - s_i)^2, total[0] = sum_i term[i] in list order, fp64 inside; one launch, no scratch.
 *   backward  ds_i = 2 (s_i - target_i) * g_i / numel_i, dense; g_i = gout[0] + gterm[i], DEVICE pointers of which one may be NULL
 *             (gterm: n floats, the gradients that arrived on the single terms); items with ds == NULL are skipped. */
#define V2W_LOSS_MAX_ITEMS 64
#define V2W_L1_TARGET_WGS  2048
typedef struct {
    const float* a; const float* b;
    float* da; float* db;                  /* backward only */
    int64_t rows;
    int32_t valid, pitch_a, pitch_b, _pad;
} v2w_l1_pair;
typedef struct {
    const float* s;
    float* ds;                             /* backward only */
    int64_t rows;
    int32_t valid, pitch;
    float target;
    int32_t _pad;
} v2w_lsgan_item;
int       v2w_l1_multi_plan(const v2w_l1_pair* pairs, int n, int32_t* starts);
long long v2w_l1_multi_scratch_bytes(const v2w_l1_pair* pairs, int n);
int v2w_l1_mean_multi(const v2w_l1_pair* pairs, int n, float scale, float* term, float* total, void* scratch, void* stream);
int v2w_l1_mean_multi_bwd(const v2w_l1_pair* pairs, int n, float scale, const float* gout, void* stream);
int v2w_lsgan_multi(const v2w_lsgan_item* items, int n, float* term, float* total, void* stream);
int v2w_lsgan_multi_bwd(const v2w_lsgan_item* items, int n, const float* gout, const float* gterm, void* stream);
/* The same terms over the maps and scores of a PADDED batch of B utterances of unequal lengths (additive in ABI v35; the dense entry points
 * above and their kernels are unchanged).  The descriptors are the same structs.  New arguments: B, the items of the batch, and `ext`, a
 * DEVICE array of n x B int32: ext[i * B + b] = the floats at the head of each of item b's rows of descriptor i that exist for that
 * utterance.  The period of a period discriminator's (b, C, H, period) maps is FOLDED INTO the table (its entries are H_b * period, as
 * v2w_map_extents writes them): the kernels take no `inner` argument.  rows % B == 0; row r belongs to item r / (rows / B) and counts its
 * first v = min(max(ext, 0), valid) floats.  For the leading-dim halves of a real-plus-generated batch B is the half's batch and both
 * halves use the same extents.  With rpi = rows / B and den_i = rpi * sum_b v_ib (formed on the device, exact in fp64; nothing is read back):
 *   L1     term[i] = (sum of |a - b| over the counted floats) / den_i, 0 when den_i == 0; total[0] = scale * sum_i term[i] in list order.
 *          backward: da = sgn(a - b) * ((scale * gout[0]) / den_i) on the counted floats and +0.0 on every other float of the dense
 *          (rows x valid) gradient; db = -da on the counted floats, +0.0 on the others.  den_i == 0: both all +0.0.
 *   LSGAN  term[i] = (sum of (target_i - s)^2 over the counted floats) / den_i, 0 when den_i == 0; total[0] = sum_i term[i].
 *          backward: ds = 2 (s - target_i) * g_i / den_i on the counted floats, +0.0 on the others.
 * A float that is not counted is SELECTED away, never multiplied by a mask: NaN or Inf there reaches no term and no gradient (the
 * discriminators do compute values past an utterance's end).  A 16-byte unit that holds no counted float is not loaded at all; the others
 * are loaded as the dense kernels load them (one 16-byte access where the unit is whole and on a 16-byte line) and masked per float.
 * Work split: v2w_l1_multi_plan and v2w_l1_multi_scratch_bytes of the same descriptors - the units, the workgroups and the order of every
 * sum are the dense call's and depend on the descriptors only, never on the extents (a workgroup with nothing to count writes a zero
 * partial at once; in the backward it stores its zeros).  So: fp64 partials, no atomics, the same call gives the same bits, and with
 * ext >= valid everywhere every output has the bits of the dense entry point.
 * Besides the dense calls' errors - V2W_E_ARG: ext NULL or not 4-byte aligned, B < 1, rows % B != 0; V2W_E_SHAPE: rows >= 2^31. */
int v2w_l1_mean_multi_len(const v2w_l1_pair* pairs, int n, const int32_t* ext, int B, float scale, float* term, float* total,
                          void* scratch, void* stream);
int v2w_l1_mean_multi_len_bwd(const v2w_l1_pair* pairs, int n, const int32_t* ext, int B, float scale, const float* gout, void* stream);
int v2w_lsgan_multi_len(const v2w_lsgan_item* items, int n, const int32_t* ext, int B, float* term, float* total, void* stream);
int v2w_lsgan_multi_len_bwd(const v2w_lsgan_item* items, int n, const int32_t* ext, int B, const float* gout, const float* gterm,
                            void* stream);
/* The extent table of a discriminator's maps from the utterances' lengths, one launch (additive).  len: DEVICE array of B int32, item b
 * holds m = min(max(len[b] * len_mul, 0), L) samples (64-bit product).  chains: DEVICE array of n rows {period, pools, depth, size};
 * layers: DEVICE array of n_layers rows {k, stride, pad}.  Row i: m <- ceil(m / period); `pools` times m <- m / 2 + 1
 * (AvgPool1d(4, 2, padding=2)); for l < depth: m <- (m + 2 pad_l - k_l) / stride_l + 1 (0 when the numerator is negative); every step
 * keeps 0 at 0; size > 0: m <- min(m, size).  ext[i * B + b] = m * period, the floats of a row that exist.  V2W_E_ARG: a NULL pointer,
 * B < 1, n < 1, len_mul < 1, L < 0, n_layers < 0.  The kernel trusts the tables (period, stride >= 1, depth <= n_layers). */
int v2w_map_extents(const int32_t* len, int len_mul, int L, int B, const int32_t* chains, int n, const int32_t* layers, int n_layers,
                    int32_t* ext, void* stream);
/* out[r][j] = j < m_b ? x[r][j] : +0.0 for `rows` dense rows of L floats, row r of item b = r / (rows / B), m_b as above (additive): what a
 * trainer applies to the generated batch before the discriminators, and - on the gradient - the backward of itself.  A select: NaN past
 * m_b does not pass, floats of x at or past m_b in a unit with no float before m_b are not loaded.  out may be x.  V2W_E_ARG: NULL
 * pointers, rows < 1, B < 1, rows % B != 0, L < 1, len_mul < 1. */
int v2w_mask_tail(const float* x, float* out, long long rows, int B, int L, const int32_t* len, int len_mul, void* stream);
/* Masked mel L1 of a batch of unequal lengths (additive; forward only - the validation loop of train.py:246-289, batched): a, b (B, C, F)
 * dense fp32; `len` a DEVICE array of B int32, len_mul >= 1 as under "Batches of unequal lengths": item b counts its first
 * F_b = min(frames(len[b] * len_mul), F) frames, frames(n) as v2w_mel_finish_len states it with pad = (n_fft - hop) / 2.
 *   per_item[b] = (sum of |a - b| over the C x F_b valid elements) / (C * F_b), 0 for F_b = 0      (B floats, may be NULL)
 *   total[0]    = (sum over b of those sums) / (C * sum_b F_b), 0 when no item has a frame         (may be NULL)
 * Elements at or past F_b are selected away (never multiplied by a mask): NaN or Inf there reaches nothing.
 * Work split: an item is ceil(C * F / 4) units of four floats - 16-byte loads when F % 4 == 0 and both pointers are 16-byte aligned, else
 * element loads - shared out over G = v2w_l1_masked_plan(C, F) = clamp(ceil(units / 1024), 1, 256) workgroups, grid (G, B): it depends on
 * the shape only.  Workgroup (g, b) writes ONE fp64 partial to ws[b * G + g] (ws: B * G doubles, 8-byte aligned); a finishing launch adds
 * an item's G partials in index order and the items' sums in a fixed order: no atomics, the same call gives the same bits, and an item's
 * value depends on no other item.
 * Roundings on the way to one value: [1] fp32 for each a - b (the absolute value is exact); every sum is fp64 - per thread at most
 * 4 * ceil(units / (256 G)) additions in a chain, [6 + 4] in the workgroup's reduction, [G] over the partials (total: + [ceil(B / 256) +
 * 6 + 4] over the items), [1] the fp64 quotient, then [1] fp32 for the stored value.
 * V2W_E_ARG: a NULL a / b / len / ws, per_item and total both NULL, len_mul < 1, hop < 1, n_fft < hop, n_fft % hop != 0, n_fft - hop odd, a pointer not
 * 4-byte (ws: 8-byte) aligned; V2W_E_SHAPE: C * F >= 2^31 - 3 or B > 65535. */
int v2w_l1_masked_plan(int C, int F);        /* host only: G > 0, or a V2W_E_* code */
int v2w_l1_masked(const float* a, const float* b, int B, int C, int F, const int32_t* len, int len_mul, int hop, int n_fft,
                  float* per_item, float* total, void* ws, void* stream);
/* v2w_l1_masked for any 1 <= hop <= n_fft (additive): the same kernels, launches and bits, pad = (n_fft - hop) / 2 rounded down as
 * mel_spectrogram pads; no condition on n_fft % hop or on the parity of n_fft - hop. */
int v2w_l1_masked_geo(const float* a, const float* b, int B, int C, int F, const int32_t* len, int len_mul, int hop, int n_fft,
                      float* per_item, float* total, void* ws, void* stream);

/* ---- Multi-resolution STFT loss (additive in ABI v35; Yamamoto et al., Parallel WaveGAN: spectral convergence + log-magnitude L1 over
 * several STFT resolutions), forward and backward, on the DFT conv's output as the mel_spectrogram pipeline leaves it - the project's own
 * framing (v2w_mel_phases[_geo]: reflect padding of (n_fft - hop) / 2 per side, no centring), not torch.stft(center=True).  Up to
 * V2W_STFT_LOSS_MAX_ITEMS resolutions per call, every one of them in the same launches; the descriptors are a HOST array, read before the
 * call returns.
 *
 * Operands of one resolution: spec_x (generated) and spec_y (target), each (B, Cs, FP) fp32 with rows [0, nb) = Re and rows [nb, 2 nb) = Im
 * over the frames [0, F).  The rows [2 nb, Cs) and the columns [F, FP) are not part of the spectrum: the rows are never read, the columns
 * may be loaded but are selected away (never multiplied by a mask), so Inf or NaN made from whatever they hold reaches nothing.  FP % 4 == 0
 * and 16-byte aligned bases (every row starts on a 16-byte line); F % 4 is arbitrary.  With N = B * nb * F and per entry
 *     X = sqrt(Re_x^2 + Im_x^2 + 1e-9f),  Y = sqrt(Re_y^2 + Im_y^2 + 1e-9f)        (v2w_mel_finish's magnitude: X, Y >= 3.1e-5)
 *   forward   Sd = sum (Y - X)^2,  Sy = sum Y^2,  Sl = sum |log Y - log X|  over the N entries;
 *             sc[r] = sqrt(Sd) / sqrt(Sy) = ||Y - X||_F / ||Y||_F,  mag[r] = Sl / N,  total[0] = (sum_r sc_r) / n,  total[1] = (sum_r mag_r) / n
 *             in list order; sums[3 r + {0, 1, 2}] = (Sd, Sy, Sl) of resolution r, DEVICE fp64, what the backward reads.  sc, mag (n floats),
 *             total (2 floats) and sums (3 n doubles, 8-byte aligned) may each be NULL, not all four.
 *   backward  g_sc_r = g_sc[0] / n + gterm_sc[r],  g_mag_r = g_mag[0] / n + gterm_mag[r]: DEVICE pointers read by the kernel (no host sync), each
 *             may be NULL (= 0), not all four; gterm_*: n floats, the gradients that arrived on the single terms.  With those,
 *                 dX = g_sc_r (X - Y) / (sqrt(Sd) sqrt(Sy)) + g_mag_r sgn(X - Y) / (N X),   dRe = dX Re_x / X,   dIm = dX Im_x / X
 *             into dspec_x (B, Cs, FP).  The first term is exactly 0 when Sd == 0 (torch's subgradient of a norm at 0); sgn(0) = 0; the sign
 *             is that of the fp32 difference X - Y of the fp32 magnitudes.  Magnitudes are recomputed from the specs, not stored.
 *             The KERNEL writes every float of dspec_x exactly once: the rows [2 nb, Cs) and the columns [F, FP) are +0.0 on return
 *             (the input-gradient conv reads them), so the caller need not zero-fill the buffer.  spec_y gets no gradient.
 * Work split.  A unit is four consecutive frames of one (item, bin): four 16-byte loads.  The forward counts B * nb * ceil(F / 4) units per
 * resolution, the backward B * (nb + ceil((Cs - 2 nb) / 2)) * (FP / 4) (the pad rows two at a time).  Resolution r gets
 * ceil(units_r / chunk_r) workgroups of 256 threads, chunk_r = max(2048, ceil(units_r / V2W_STFT_LOSS_TARGET_WGS)): at least one, at most
 * V2W_STFT_LOSS_TARGET_WGS, from its own descriptor only.
 *   v2w_stft_loss_plan (host only): the forward's split: starts[i] = first workgroup of resolution i, starts[n] = workgroups of the streaming
 *             launch, also the return value (> 0).
 *   v2w_stft_loss_scratch_bytes (host only): bytes of caller-owned `scratch` (8-byte aligned) the forward needs: 24 per workgroup.
 * Deterministic: each workgroup of the streaming launch writes ONE fp64 triple to scratch; the finishing launch (one workgroup) adds a
 * resolution's triples - thread t the triples t, t + 256, ... in index order, the 256 sums through the fixed-order block reduction - no
 * atomics, the same call gives the same bits, and a resolution's values (given the same g_sc_r and g_mag_r, its gradient too) are the bits of the call that holds it alone.
 * Roundings on the way to one value (u = 2^-24).  X = sqrt(fma(Im, Im, Re * Re) + 1e-9f), each operation ONE fp32 rounding and the same
 * three for both signals (equal spectra give X == Y bit for bit, hence sc == 0, mag == 0 and dspec_x == 0): [3] on a sum of positive terms
 * under the root and [1] the root (correctly rounded), at most 2.5 u relative.  Y - X and log Y - log X: [1] fp32 each on the fp32 magnitudes and their logf (logf: a few u relative to
 * |log|, measured in tests/mel_ref.py); the squares, every sum, both roots, the quotients and the means over r are fp64 - per thread at most
 * 4 * ceil(chunk / 256) additions in a chain, [6 + 4] in the workgroup's reduction, [ceil(workgroups / 256) + 6 + 4] over the triples - then
 * [1] fp32 for each stored value.  Backward, per entry, every line ONE correctly rounded fp32 operation on the fp32 X, Y:
 *     c_sc = g_sc_r / (sqrt(Sd) sqrt(Sy)), c_mag = g_mag_r / N      each computed in fp64 and rounded once to fp32 (c_sc = 0 for Sd == 0);
 *                                                                   g_*_r itself: [1] the division by n, [1] the addition
 *     d  = X - Y
 *     r  = 1 / X
 *     m  = c_mag * r,  signed by d (0 for d == 0)
 *     dX = fma(c_sc, d, m)
 *     w  = dX * r
 *     dRe = w * Re_x,  dIm = w * Im_x
 * V2W_E_ARG: a NULL items / spec_x / spec_y (backward: dspec_x, sums) or scratch, every output NULL (backward: every gradient NULL), n < 1
 * or n > V2W_STFT_LOSS_MAX_ITEMS, B / F / nb <= 0, FP < F, Cs < 2 nb, FP % 4 != 0, a spec not 16-byte, a double not 8-byte or a float not
 * 4-byte aligned.  V2W_E_SHAPE: Cs * FP or B * Cs * FP past 2^31 - 1. */
#define V2W_STFT_LOSS_MAX_ITEMS  8
#define V2W_STFT_LOSS_TARGET_WGS 1024
typedef struct {
    const float* spec_x; const float* spec_y;
    float* dspec_x;                        /* backward only */
    int32_t B, Cs, FP, F, nb, _pad;
} v2w_stft_loss_item;
int       v2w_stft_loss_plan(const v2w_stft_loss_item* items, int n, int32_t* starts);
long long v2w_stft_loss_scratch_bytes(const v2w_stft_loss_item* items, int n);
int v2w_stft_loss_multi(const v2w_stft_loss_item* items, int n, float* sc, float* mag, float* total, double* sums, void* scratch,
                        void* stream);
int v2w_stft_loss_multi_bwd(const v2w_stft_loss_item* items, int n, const double* sums, const float* g_sc, const float* g_mag,
                            const float* gterm_sc, const float* gterm_mag, void* stream);
/* The same loss for a padded batch of unequal lengths (additive; "Batches of unequal lengths": `len` a DEVICE array of B int32, len_mul >= 1,
 * the grids depend on the shapes only).  hop and n_fft are HOST arrays of n int32, the frame geometry of each resolution; the descriptors are
 * the dense call's.  Item b of resolution r counts F_b = min(frames(len[b] * len_mul), F) frames, frames(n) as v2w_mel_finish_geo_len states it
 * with pad = (n_fft[r] - hop[r]) / 2 rounded down (0 unless n > pad and n + 2 pad >= n_fft; with F the frames of the batch's L samples this
 * is the frames of min(len[b] * len_mul, L)), and everything above holds with "the frames [0, F)" of item b read as [0, F_b):
 *   forward   Sd, Sy, Sl over the entries (b, bin, f < F_b);  N_r = nb * sum_b F_b, counted ONCE on the device by the finishing launch (the
 *             counts added as fp64 integers, exact) - no length and no frame count comes to the host;  sc[r] = sqrt(Sd) / sqrt(Sy),
 *             mag[r] = Sl / N_r, both exactly 0 when N_r == 0 (no 0 / 0);  total as above.  sums holds FOUR doubles per resolution:
 *             sums[4 r + {0, 1, 2, 3}] = (Sd, Sy, Sl, N_r), what v2w_stft_loss_multi_len_bwd reads (4 n doubles, 8-byte aligned).
 *   backward  the dense call's lines, one fp32 operation each, with c_mag = g_mag_r / N_r from sums[4 r + 3] (computed in fp64, rounded once;
 *             0 when N_r == 0) on the entries f < F_b.  Every float of dspec_x is written exactly once: the columns [F_b, FP) of item b and
 *             the rows [2 nb, Cs) are +0.0.
 * Work split, scratch and plan: the dense call's (v2w_stft_loss_plan, v2w_stft_loss_scratch_bytes) - a unit is four frames of one (item,
 * bin) of the padded batch.  A unit whose four frames lie at or past F_b issues no load: the forward adds nothing for it, the backward
 * stores its zeros.  Frames at or past F_b inside a partly valid unit are loaded and SELECTED away (never multiplied by a mask): NaN, Inf
 * or stale workspace there reaches no stored value.  No atomics; the same call gives the same bits; the chunks and the order of every sum
 * are the dense call's, so with every F_b == F the sums, sc, mag, total and dspec_x have the bits of v2w_stft_loss_multi / _multi_bwd.
 * Roundings: the dense block's, with these differences only: a thread's chain and a workgroup's triple hold the valid entries alone (a
 * skipped entry adds an exact 0.0 or nothing); N_r is an exact integer in fp64 (nb * sum_b F_b < 2^53); mag and c_mag divide by it.
 * V2W_E_ARG / V2W_E_SHAPE: everything the dense calls refuse, with their codes; then V2W_E_ARG for a NULL hop / n_fft / len, len_mul < 1,
 * hop[r] < 1 or n_fft[r] < hop[r]; V2W_E_SHAPE for B > 65535 or F * hop[r] + n_fft[r] past 2^31 - 1 (as the mel _len calls). */
int v2w_stft_loss_multi_len(const v2w_stft_loss_item* items, int n, const int32_t* hop, const int32_t* n_fft, const int32_t* len,
                            int len_mul, float* sc, float* mag, float* total, double* sums, void* scratch, void* stream);
int v2w_stft_loss_multi_len_bwd(const v2w_stft_loss_item* items, int n, const int32_t* hop, const int32_t* n_fft, const int32_t* len,
                                int len_mul, const double* sums, const float* g_sc, const float* g_mag, const float* gterm_sc,
                                const float* gterm_mag, void* stream);

/* ---- AdamW (additive in ABI v35; torch.optim.AdamW as train.py:96-99 constructs it and train.py:198,215 steps it: decoupled weight
 * decay, no amsgrad, no maximize): the step of up to V2W_ADAMW_MAX_ITEMS parameter tensors in ONE launch that reads p, g, m, v and
 * writes p, m, v once (28 bytes per parameter).  The descriptors and the hyperparameters are HOST memory, read before the call returns.
 * p, g, m (exp_avg), v (exp_avg_sq): `numel` dense fp32 each, 4-byte aligned; items whose four pointers share their 16-byte phase take
 * 16-byte accesses, the others float-by-float ones.  Every element of p, m and v is written exactly once and nothing else is written;
 * no atomics, no scratch, no library state.  The kernel never sees the step count t: the caller passes bias_corr1 = 1 - beta1^t and
 * bias_corr2_sqrt = sqrt(1 - beta2^t), each computed in double and rounded once to fp32 (no device step tensor, no host sync).
 *
 * Arithmetic.  Launch constants, each computed on the host in double from the fp32 fields and rounded ONCE to fp32:
 *     decay = 1 - lr * weight_decay,  omb1 = 1 - beta1,  omb2 = 1 - beta2,  rbc2 = 1 / bias_corr2_sqrt,  step = lr / bias_corr1
 * Per element, every line ONE correctly rounded fp32 operation (fma = fused multiply-add, one rounding), in this order:
 *     pd  = p * decay
 *     d   = g - m
 *     m'  = fma(omb1, d, m)                       3 roundings on m': omb1, d, m'
 *     gg  = g * g
 *     tg  = omb2 * gg
 *     v'  = fma(beta2, v, tg)                     4 roundings on v': omb2, gg, tg, v'
 *     den = fma(sqrt(v'), rbc2, eps)              sqrt correctly rounded
 *     q   = m' / den                              correctly rounded
 *     p'  = fma(-step, q, pd)                    15 roundings on p': decay, pd, the 3 of m', the 4 of v', sqrt, rbc2, den, step, q, p'
 * which is p <- p (1 - lr wd);  m <- m + (1 - b1)(g - m);  v <- b2 v + (1 - b2) g g;  p <- p - (lr / bias_corr1) m / (sqrt(v) / bias_corr2_sqrt
 * + eps), torch's order.  Against that formula evaluated exactly from the same fp32 inputs, with u = 2^-24:
 *     |m' - exact| <= 3u (|m| + |g|),   |v' - exact| <= 4u (|v| + g g),   |p' - exact| <= 15u (|p| + step (|m| + |g|) / den)
 * to first order (|m'| <= |m| + |g|; v' and den are sums of non-negative terms, so their relative errors add up).
 *
 * V2W_E_ARG: items or h NULL; n < 1 or n > V2W_ADAMW_MAX_ITEMS; a NULL or not 4-byte aligned pointer; numel <= 0; a beta outside [0, 1);
 * eps < 0, lr < 0, bias_corr1 <= 0 or bias_corr2_sqrt <= 0 (or a NaN among them); p, m or v of one item overlapping each other.
 * V2W_E_SHAPE: numel > 2^42 (more than 2^40 units).
 * V2W_ADAMW_MAX_ITEMS: the table travels by value in the kernel arguments, which hold 4 KB with the hidden ones (3584 bytes are the
 * library's own limit, as for the loss kernels): 80 * 40 (items) + 81 * 4 (starts) + 28 (constants) + 4 (n) = 3556 bytes.
 * The plan, v2w_adamw_multi_plan (host only; it reads the items like the launch does): starts[i] = first workgroup of tensor i, starts[n] =
 *     workgroups of the launch, also the return value (> 0), at most V2W_ADAMW_TARGET_WGS + n; every tensor has at least one.  A tensor counts
 *     ceil((numel + s) / 4) units of four floats, s = floats of p past a 16-byte line when g, m and v have the same phase, else 0;
 *     chunk = max(2048, ceil(sum of units / V2W_ADAMW_TARGET_WGS)); tensor i gets ceil(units_i / chunk) workgroups of 256 threads. */
#define V2W_ADAMW_MAX_ITEMS  80
#define V2W_ADAMW_TARGET_WGS 2048
typedef struct {
    float* p;
    const float* g;
    float* m;
    float* v;
    int64_t numel;
} v2w_adamw_item;
typedef struct {
    float lr, beta1, beta2, eps, weight_decay, bias_corr1, bias_corr2_sqrt;
    int32_t _pad;
} v2w_adamw_hyper;
int v2w_adamw_multi_plan(const v2w_adamw_item* items, int n, int32_t* starts);
int v2w_adamw_multi(const v2w_adamw_item* items, int n, const v2w_adamw_hyper* h, void* stream);

/* ---- Global-norm gradient clipping and the non-finite guard (additive in ABI v35; torch.nn.utils.clip_grad_norm_ with norm_type 2, and
 * an AdamW step that takes the clip coefficient from DEVICE memory): one streaming launch over up to V2W_ADAMW_MAX_ITEMS gradient
 * tensors, one finishing launch, and the coefficient consumed by the step's kernel - no gradient is rewritten, the host reads nothing.
 * The descriptors are the AdamW ones, HOST memory read before the call returns, and so is the work split: v2w_adamw_multi_plan's units,
 * chunk and starts[], 16-byte accesses for an item whose pointers share their 16-byte phase and float-by-float ones otherwise.  For the
 * two entries that touch g only (sumsq, scale) the plan is taken of the item with p = m = v = g: the phase is g's own, every item takes
 * 16-byte accesses, and p, m, v are neither read nor checked.  No atomics, no library state; every value below that leaves a kernel
 * leaves it through an ordinary vector store.
 *
 *   v2w_grad_sumsq_partials (host only)  the workgroups W of the sumsq launch for these items (> 0) = the floats it writes: the return
 *       value of v2w_adamw_multi_plan for the items with p = m = v = g.
 *   v2w_grad_sumsq_multi  partials[w] = sum of g^2 over the chunk of workgroup w, for w in [0, W); nothing else is written.  A list of
 *       more than V2W_ADAMW_MAX_ITEMS tensors is several calls into consecutive ranges of one caller-owned buffer.
 *       Order (fixed: the same call gives the same bits): thread t of 256 takes the units t, t + 256, ... of the chunk in that order
 *       and the four floats of a unit in index order, acc = fma(x, x, acc) from acc = 0 (masked floats enter as 0): a chain of
 *       T = 4 * ceil(chunk_i / 256) roundings at most, chunk_i = ceil(units_i / workgroups_i) <= the plan's chunk; then the block sum
 *       of 4 waves (v2w_sn's: a butterfly of 6 additions over the 64 lanes, then the waves' sums in wave order), 6 + 4 roundings.
 *   v2w_grad_norm_finish  one workgroup; thread t adds the partials [t * c, (t + 1) * c), c = ceil(n_partials / 256), in index order in
 *       fp64, the 256 sums go through the same block sum in fp64: S.  Thread 0 writes
 *         out[0] = (float)sqrt(S)                                     the total L2 norm
 *         out[1] = (float)min(1, max_norm / (sqrt(S) + 1e-6))         the clip coefficient, in fp64 and rounded once (torch's formula: 1 for
 *                                                                     max_norm = +inf and a finite norm; NaN passes through the min)
 *         out[2] = 1.0 when (float)sqrt(S) is finite, else 0.0
 *         out[3] = out[3] + (1 - out[2])                              a running count of non-finite norms: read, incremented, written back.
 *       `out` is the caller's (4 floats, 4-byte aligned; the count starts from whatever the caller put there).
 *   v2w_scale_multi       g[e] = g[e] * coef[0] for every element, ONE fp32 multiplication each, the coefficient read from DEVICE memory
 *       by the kernel: a coefficient of exactly 1.0 leaves every bit as it was (no branch on it anywhere).
 *   v2w_adamw_multi_clipped  v2w_adamw_multi with g replaced by g' = g * clip[1] (ONE fp32 multiplication, ahead of the list of operations
 *       above; g itself is only read).  clip: the 4 floats v2w_grad_norm_finish wrote, DEVICE memory read by the kernel.  With
 *       skip_nonfinite != 0 and clip[2] == 0 every workgroup returns before its first load: p, m and v keep their bits.  With
 *       clip[1] == 1.0 the step's bits are v2w_adamw_multi's.  The same kernel body as v2w_adamw_multi, compiled a second time.
 *
 * Bounds, u = 2^-24, to first order, against the exact value from the same fp32 inputs.
 *   Sum of squares: every term is >= 0, so the relative errors of a chain add up: |partial - exact| <= (T + 10) u * exact, and the fp64
 *       sum S inherits it (its own roundings are 2^-29 of u each).  The norm is a square root - half the relative error - and one
 *       rounding to fp32:   |out[0] - exact norm| <= ((T + 10) / 2 + 1) u * norm.   At the generator's parameter list (chunk 2048, T = 32)
 *       that is 22 u.  The coefficient, where it is below 1, has the norm's relative error and its own rounding: (T + 10) / 2 + 2.
 *       A square overflows fp32 for |g| > 1.8e19: such a gradient reads as a non-finite norm.
 *   Clipped step, against the AdamW formula evaluated exactly at g clip[1]: one more rounding on g' wherever g enters -
 *       4 roundings on m' (was 3), 6 on v' (was 4: g' enters twice), 18 on p' (was 15), on the same magnitudes taken at g':
 *       |m' - exact| <= 4u (|m| + |g'|),   |v' - exact| <= 6u (|v| + g' g'),   |p' - exact| <= 18u (|p| + step (|m| + |g'|) / den)
 *   tests/clip_ref.py restates both in fp64.
 *
 * V2W_E_ARG: items NULL; n < 1 or n > V2W_ADAMW_MAX_ITEMS; numel <= 0; g (sumsq, scale) or any of p, g, m, v (clipped step: every check of
 * v2w_adamw_multi) NULL or not 4-byte aligned; partials, coef, clip or out NULL or not 4-byte aligned; n_partials < 1; max_norm negative
 * or NaN.  V2W_E_SHAPE: numel > 2^42. */
int v2w_grad_sumsq_partials(const v2w_adamw_item* items, int n);
int v2w_grad_sumsq_multi(const v2w_adamw_item* items, int n, float* partials, void* stream);
int v2w_grad_norm_finish(const float* partials, int n_partials, float max_norm, float* out, void* stream);
int v2w_scale_multi(const v2w_adamw_item* items, int n, const float* coef, void* stream);
int v2w_adamw_multi_clipped(const v2w_adamw_item* items, int n, const v2w_adamw_hyper* h, const float* clip, int skip_nonfinite, void* stream);

/* ---- Exponential moving average of the weights (additive in ABI v35; the reference has none - GAN vocoders are evaluated and shipped from
 * e <- decay e + (1 - decay) p): the average updated by the AdamW step's own kernel, in the pass that already holds p' in registers - read
 * p, g, m, v, e and write p, m, v, e once, 36 bytes per parameter, one launch per V2W_ADAMW_EMA_MAX_ITEMS tensors - plus the two lines alone
 * (v2w_ema_multi: parameters stepped by something else, buffers) and an in-place exchange of p and e (v2w_swap_multi: validate or
 * synthesise from the average without moving a storage pointer).  The descriptors are HOST memory, read before the call returns.
 * The caller passes ema_omd = 1 - decay, computed in double and rounded ONCE to fp32.
 *
 * Arithmetic of the average, after p' of the operation list of v2w_adamw_multi (v2w_ema_multi: with the stored p for p'), every line ONE
 * correctly rounded fp32 operation:
 *     de  = p' - e
 *     e'  = fma(ema_omd, de, e)                   3 roundings on e': ema_omd, de, e'
 * Against e + (1 - decay)(p' - e) evaluated exactly from the STORED p' and the fp32 ema_omd (whose own rounding is then the caller's, not the
 * kernel's: 2 of the 3 remain), with u = 2^-24:  |e' - exact| <= 3u (|e| + |p'|)  to first order (|de| <= |p'| + |e|, ema_omd <= 1 and
 * |e'| <= |e| + |p'|).  ema_omd == 0 leaves every bit of a finite e as it was (fma(0, de, e) = e for a finite de); ema_omd == 1 gives
 * fma(1, p' - e, e), which is p' to one rounding, not bit for bit.  tests/ema_ref.py restates the lines, the bound and the closed form
 * e_T = d^T e_0 + (1 - d) sum_t d^(T-1-t) p_t in fp64.
 *
 *   v2w_adamw_ema_multi  the AdamW step with the average updated in the same pass.  clip == NULL: the arithmetic of v2w_adamw_multi
 *       (skip_nonfinite is then not looked at: there is no flag to read); otherwise that of v2w_adamw_multi_clipped, g' = g * clip[1] read
 *       from DEVICE memory.  The same kernel body as those two, compiled twice more behind a template flag: p', m' and v' are bit for bit
 *       those of the existing entry points on the same inputs.  Every element of p, m, v and e is written exactly once and nothing else
 *       is written; no atomics, no scratch, no library state; every value leaves through an ordinary vector store.  With
 *       skip_nonfinite != 0 and clip[2] == 0 every workgroup returns before its first load: p, m, v AND e keep their bits - a skipped step
 *       does not move the average either.
 *   v2w_ema_multi   the two lines alone, p only read: up to V2W_ADAMW_MAX_ITEMS items of v2w_ema_item; every element of e is written once.
 *   v2w_swap_multi  exchanges the contents of p and e in place: each thread loads both values of its units, then stores both - one launch,
 *       every element read once and written once, bit for bit.  Its descriptor is v2w_swap_item: the layout of v2w_ema_item with both
 *       pointers writable (a struct of its own, so that no const is cast away); up to V2W_ADAMW_MAX_ITEMS items.
 *
 * The work split is v2w_adamw_multi_plan's: units of four floats, chunk = max(2048, ceil(sum of units / V2W_ADAMW_TARGET_WGS)), starts[],
 * at least one workgroup per tensor.  An item takes 16-byte accesses only when ALL its pointers share their 16-byte phase - the five of a
 * v2w_adamw_ema_item, p and e of the other two - and its units are then cut at the 16-byte lines (ceil((numel + s) / 4) units, s = floats
 * of p past a line); otherwise it takes float-by-float accesses and counts ceil(numel / 4).  v2w_adamw_ema_multi_plan and
 * v2w_ema_multi_plan (host only; v2w_swap_multi's plan is v2w_ema_multi_plan of the same pointers) read the items like the launch does.
 *
 * V2W_ADAMW_EMA_MAX_ITEMS: the table travels by value in the kernel arguments under the library's 3584 bytes: 64 * 48 (items) + 65 * 4
 * (starts) + 28 (constants) + 4 (ema_omd) + 4 (n) = 3368 bytes; the pair table is 80 * 24 + 81 * 4 + 4 = 2248.
 *
 * V2W_E_ARG: every case of v2w_adamw_multi (v2w_adamw_multi_clipped when clip != NULL: clip not 4-byte aligned) with
 * V2W_ADAMW_EMA_MAX_ITEMS for the item limit; e NULL or not 4-byte aligned; e overlapping p, m or v of its item; ema_omd outside [0, 1] or
 * NaN.  v2w_ema_multi / v2w_swap_multi: items NULL; n < 1 or n > V2W_ADAMW_MAX_ITEMS; p or e NULL or not 4-byte aligned; numel <= 0; p and e
 * of one item overlapping; ema_omd outside [0, 1] or NaN.  The plans: the items' cases, and starts NULL.  V2W_E_SHAPE: numel > 2^42. */
#define V2W_ADAMW_EMA_MAX_ITEMS 64
typedef struct {
    float* p;
    const float* g;
    float* m;
    float* v;
    float* e;
    int64_t numel;
} v2w_adamw_ema_item;
typedef struct {
    const float* p;
    float* e;
    int64_t numel;
} v2w_ema_item;
typedef struct {
    float* p;
    float* e;
    int64_t numel;
} v2w_swap_item;
int v2w_adamw_ema_multi_plan(const v2w_adamw_ema_item* items, int n, int32_t* starts);
int v2w_adamw_ema_multi(const v2w_adamw_ema_item* items, int n, const v2w_adamw_hyper* h, const float* clip, int skip_nonfinite, float ema_omd,
                        void* stream);
int v2w_ema_multi_plan(const v2w_ema_item* items, int n, int32_t* starts);
int v2w_ema_multi(const v2w_ema_item* items, int n, float ema_omd, void* stream);
int v2w_swap_multi(const v2w_swap_item* items, int n, void* stream);

/* ---- Spectral norm of conv weights (additive in ABI v35; legacy torch.nn.utils.spectral_norm as models.py:219-258 applies it to the first
 * DiscriminatorS: one power iteration per training forward, W / sigma): up to V2W_SN_MAX_LAYERS weight matrices per call, the step in 4
 * launches (2 without the iteration), its backward in 2, whatever the number of layers.  Nothing is allocated, no state is kept.
 *
 * A layer is W = weight_orig (C_out, C_in / groups, k) contiguous - R = c_out rows of N = c_in * k floats; a Conv2d (.., k, 1) weight has the
 * same memory - with u (R) and v (N).  The descriptors live in DEVICE memory for the launches; the plan fills their offsets on the HOST copy
 * first.  Per call the caller hands over a workspace `ws` (16-byte aligned, v2w_sn_grids::ws_bytes; contents meaningless between calls, the
 * step and the backward may share it) and a KEEP slab `keep` (16-byte aligned, v2w_sn_grids::keep_bytes) that receives, at float offset
 * keep_off of each layer: sigma (one float, three unused), the u of this call (R floats, padded to a multiple of 4), the v of this call (N
 * floats, padded likewise).  The slab is what the backward of THIS call reads: a later step overwrites u and v in place, not the slab.
 *
 *   v2w_sn_plan (host only)  checks every descriptor, fills blk_t / blk_r / blk_s / ws_off / keep_off and *g; returns ws_bytes (> 0).
 *       V2W_E_ARG: descs or g NULL; n < 1 or n > V2W_SN_MAX_LAYERS; c_out, c_in or k <= 0; w, u, v or wf NULL or not 4-byte aligned.
 *       V2W_E_SHAPE: R * N >= 2^31.
 *       Work split, with nb = ceil(R / 64): the W^T u launch gives the layer nb * ceil(N / 256) workgroups (64 rows x 256 columns each), the
 *       W v launch ceil(R / 4) (one wave per row), the relayout launches ceil(R / 64) * ceil(N / 64) tiles; ws holds per layer
 *       max(nb * N + R, tiles) floats rounded up to 4: nb partial rows of W^T u then t = W v (step), one partial per tile (backward).
 *   v2w_sn_step   training != 0:  a = W^T u;  v <- a / max(||a||, 1e-12);  t = W v;  u <- t / max(||t||, 1e-12);  sigma = sum_o u[o] t[o]
 *                 (sigma REUSES the t = W v that the u update formed - no third matrix-vector product - with the new, rounded u);
 *                 wf[j][c][o] = w[o][c][j] / sigma, the layout of v2w_wn_fold_conv.  u and v are overwritten in place.
 *                 training == 0: no iteration, u and v are not written; t = W v and sigma = sum_o u[o] t[o] from the stored vectors; wf as above.
 *                 Either way sigma and the u, v the call used go to the keep slab.
 *   v2w_sn_bwd    dw[o][c][j] = dwf[j][c][o] / sigma - (sum(dwf . w) / sigma^2) u[o] v[c k + j]  with sigma, u, v from the keep slab (u, v
 *                 are constants of the forward, as under torch.no_grad in the reference's hook).  dwf[i] / dw[i]: HOST arrays of n device
 *                 pointers, read before the call returns; dwf[i] is [k][c_in][c_out] like wf, dw[i] is shaped like w; a layer with both
 *                 NULL is skipped.  V2W_E_ARG: one of a pair NULL, all pairs NULL, a pointer not 4-byte aligned.
 *   Both launching calls: V2W_E_ARG for a NULL descs_dev / g / keep / ws, n out of range or != g->n, ws or keep not 16-byte aligned,
 *   ws_bytes < g->ws_bytes.
 *
 * Memory access: rows are read with 16-byte loads when N % 4 == 0 and the base pointer is 16-byte aligned (the "vector path"), else with
 * coalesced 4-byte loads; wf and dwf are always accessed along C_out, 4 bytes per lane, 256 consecutive bytes per wave.
 * Determinism: no atomics; sums across workgroups go through ws and are added in index order; a layer's results are the same bits
 * whatever else shares the launch.
 *
 * Arithmetic: every operation below is ONE correctly rounded fp32 operation (fma = fused multiply-add); "chain of m" = m of them applied one
 * after the other to one accumulator that starts at 0; a "wave sum" is 6 additions (butterfly over 64 lanes), a "block sum" of W waves a
 * wave sum and then W additions in wave order.  The number in brackets is the roundings on the path to one output entry.
 *   a[j]    one partial per band of 64 rows: an fma chain of 16 (every 4th row of the band) in each of 4 waves, 3 additions to combine the
 *           waves; then nb - 1 additions over the bands in index order                                              [16 + 3 + nb - 1]
 *   q       = sum_j a[j]^2: per thread an fma chain of ceil(N / 1024), block sum of 16 waves                         [ceil(N / 1024) + 22]
 *   dn      = max(sqrt(q), 1e-12)                                                                                    [1]
 *   v[j]    = a[j] / dn                                                                                              [1]
 *   t[o]    vector path: 4 fma chains of ceil(N / 256) per lane, 2 additions (x + y) + (z + w), wave sum             [ceil(N / 256) + 8]
 *           scalar path: one fma chain of ceil(N / 64) per lane, wave sum                                            [ceil(N / 64) + 6]
 *   p       = sum_o t[o]^2: per thread an fma chain of ceil(R / 256), block sum of 4 waves                           [ceil(R / 256) + 10]
 *   du      = max(sqrt(p), 1e-12)                                                                                    [1]
 *   u[o]    = t[o] / du                                                                                              [1]
 *   sigma   = sum_o u[o] t[o]: as p                                                                                  [ceil(R / 256) + 10]
 *   wf      = w / sigma                                                                                              [1]
 *   dot     = sum dwf w: per 64 x 64 tile an fma chain of 16 per thread and a block sum of 4 waves; then over the layer's tiles per thread
 *             a chain of ceil(tiles / 256) additions and a block sum of 4 waves                                      [26 + ceil(tiles / 256) + 10]
 *   s2      = sigma sigma;  coef = dot / s2;  g = dwf / sigma;  uv = u[o] v[c];  dw = fma(-coef, uv, g)              [1 each]
 * tests/sn_ref.py restates this in fp64 and turns the counts into per-entry bounds. */
#define V2W_SN_MAX_LAYERS 64
typedef struct {
    const float* w;
    float* u;
    float* v;
    float* wf;
    int32_t c_out, c_in, k;          /* c_in: input channels per group */
    int32_t blk_t, blk_r, blk_s;     /* filled by v2w_sn_plan: the layer's first workgroup in the three grid shapes */
    int64_t ws_off, keep_off;        /* filled by v2w_sn_plan: float offsets of the layer in ws and in keep */
} v2w_sn_desc;                       /* 72 bytes */
typedef struct {
    int32_t n, grid_t, grid_r, grid_s;
    int64_t ws_bytes, keep_bytes;
} v2w_sn_grids;                      /* 32 bytes; HOST memory, filled by v2w_sn_plan, read by the launching calls before they return */
long long v2w_sn_plan(v2w_sn_desc* descs, int n, v2w_sn_grids* g);
int v2w_sn_step(const v2w_sn_desc* descs_dev, int n, int training, const v2w_sn_grids* g, float* keep, void* ws, long long ws_bytes,
                void* stream);
int v2w_sn_bwd(const v2w_sn_desc* descs_dev, int n, const v2w_sn_grids* g, const float* keep, const float* const* dwf, float* const* dw,
               void* ws, long long ws_bytes, void* stream);

/* ---- Sample-rate conversion and peak normalisation (ABI v35, additive): the two ends of the audio path.  The reference reads every training
 * target through librosa.load(path, sr=16000) and normalize(audio) * 0.95 on a host core (vec2wav/dataset.py:16-20,133); a 16 kHz generator's
 * output wants 44.1 or 48 kHz for playback.  Both are one band-limited rational-ratio resampler, here the polyphase form of
 * torchaudio.functional.resample's Hann-windowed sinc (lowpass_filter_width lpw, rolloff):
 *
 *   g = gcd(orig, new), M = orig / g (input step), L = new / g (phases), base = min(M, L) * rolloff
 *   t(p, k) = (k / M - p / L) * base;   h[p][k] = sinc(pi t) cos^2(pi t / (2 lpw)) base / M  where |t| < lpw, else 0
 *   y[q L + p] = sum_k h[p][k] x[q M + k],  x = 0 outside [0, n);   N = ceil(L n / M) outputs for n inputs
 *
 * Per phase the non-zero taps are one run of at most NT = ceil(2 lpw M / base): the caller hands the run's first index k0[p] (int32, L of
 * them) and the table h (fp32, (L, NT) row-major, a shorter run padded with 0 at its end).  k0 must not decrease with p and
 * k0[L - 1] - k0[0] <= M (true of the formula: k0[p] = floor(M p / L - lpw M / base) + 1); taps that such a table would place outside the
 * staged window read as 0.  34 multiply-adds per output at 441 : 160 against the 475 of the strided-conv form.
 *
 *   out[b][q L + p] = fma(h[p][NT - 1], x[..], ... fma(h[p][1], x[..], fma(h[p][0], x[b][q M + k0[p]], +0)))       fp32, tap order
 *
 * so |out - exact| <= (NT + 1) 2^-24 sum_j |h[p][j] x[..]|, and an output none of whose taps meets a non-zero sample is exactly 0.
 * x is float32, or with in_i16 != 0 int16 PCM read as x / 32768 (exact).  Item b holds n_b = min(max(len[b], 0), Lin) samples (len: B int32
 * on the device, NULL: every item Lin): out[b][0 .. N_b) is what the item alone gives, out[b][N_b .. Lout) is written as +0.0, and
 * x[b][n_b ..] is never loaded.  M = L = NT = 1, h = {1}, k0 = {0} is the float32 copy of x (a -0.0 comes out +0.0) with the same per-item
 * tail.  Offsets are 64-bit.  No atomics; the same bits from run to run.
 *
 * v2w_resample_plan (host only) fills g: `tile` outputs per workgroup of 256 threads - the largest of 4096, 2048, .. 256 whose LDS fits -,
 * `tiles` = ceil(Lout / tile) per item, `grid` = B * tiles and `lds_bytes` =
 *   4 * (L * (NT | 1) + L + ((tile - 1) / L + 2) * M + NT + 4)           (table rows at an odd pitch, k0, the input window, 4 floats)
 * which must not exceed 64 KiB: V2W_E_SHAPE when it does at tile = 256, that is unless
 *   L * ((NT | 1) + 1) + ((255 / L) + 2) * M + NT + 4 <= 16384
 * (in short L * (NT + 2) + 2 M + 256 M / L below 16 Ki floats: 441 : 160 and 160 : 441 use 48 and 31 KiB; a ratio of two large coprime rates
 * such as 16000 : 44101 does not fit), and when B * tiles passes 2^31 - 1.
 *
 * v2w_resample: one launch (resample_kernel).  peak_part != NULL: (B, tiles) floats, [b][tile] = the maximum of |out| over that tile (a
 * plain store per workgroup).  V2W_E_ARG: x, y, h or k0 NULL, a pointer not aligned to its element, a size <= 0,
 * Lout < ceil(L * Lin / M); the plan's V2W_E_SHAPE.  Nothing is launched on refusal.
 *
 * v2w_peak_scale: librosa.util.normalize(y) * peak per item, in place, one launch (peak_scale_kernel): m = max over the item's `parts`
 * partials (exact in any order), s = peak / m, y[b][i] = y[b][i] * s - one division and one multiplication, |error| <= 2.5 * 2^-24 |y peak / m|
 * with the float `peak` counted.  A row whose m is below FLT_MIN (or NaN) keeps its bits.  The partials are v2w_resample's, or any (B, parts)
 * floats whose row maximum is the item's.  V2W_E_ARG: y or peak_part NULL or not 4-byte aligned, B, Lout or parts <= 0, peak not a
 * finite positive float.  V2W_E_SHAPE: B * ceil(Lout / 4096) past 2^31 - 1. */
typedef struct {
    int32_t tile, tiles, grid, lds_bytes;
} v2w_resample_grids;                /* 16 bytes; HOST memory, filled by v2w_resample_plan */
int v2w_resample_plan(int M, int L, int NT, int B, int Lout, v2w_resample_grids* g);
int v2w_resample(const void* x, int in_i16, float* y, int B, int Lin, int Lout, const float* h, const int32_t* k0, int M, int L, int NT,
                 const int32_t* len, float* peak_part, void* stream);
int v2w_peak_scale(float* y, int B, int Lout, const float* peak_part, int parts, float peak, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VEC2WAV_HIP_H */
