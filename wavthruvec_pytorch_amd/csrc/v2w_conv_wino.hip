// Winograd F(2,3) Conv1d on the gfx950 f32 MFMA pipe (V2W_ALGO_WINO): the wide residual convs of the generator
// (models.py:65-70 of the reference: leaky_relu -> dilated Conv1d, odd k, stride 1) with fewer multiplies.
//
// The arithmetic is in v2w_wino.h: the outputs go in pairs (t, t + dil), every segment of <= 3 taps feeds four accumulator classes,
// and a k = 3 / 7 / 11 conv issues 4 / 10 / 15 products per output pair and channel pair instead of 6 / 14 / 22 (x0.69 over a ResBlock2
// layer triple).  Every coefficient is 0, +-1 or 1/2, folded into the weights by the packers; the input side is x_j -+ x_j'.
//
// GEMM view per workgroup: M = MT output channels, N = NTP output PAIRS (2 NTP positions), K = C_in x terms, four accumulator sets.
// The staging is a copy of conv_tile_kernel's (v2w_conv_mfma.hip; the LDS tile geometry, TileGeom, is shared through v2w_tile.h - hipcc
// allocates other register counts for either kernel when item / prefetch / commit / stage_scalar, the weight ring or the prologue tables
// come from one shared definition, so each kernel keeps its own): the activated signal (CondBN affine + leaky_relu applied once) in the LDS tile
// Xs[positions][36 floats], position-major, channels permuted so that a lane's four k-steps are one ds_read_b128; double-buffered over
// chunks of 32 input channels.  Unlike there the next chunk is loaded and written after the MFMA phase (its registers would cost the third
// wave per SIMD; the other workgroups on the CU cover the latency).
// Lane column j of a wave owns pair P; pair P's first output sits at t(P) = 2 dil (P / dil) + P % dil, so every operand x_j of
// every segment is a row offset from the lane's base row.  Per unit (4 k-steps) of a 3-tap segment a lane reads x0..x3 (4 x
// ds_read_b128), forms u0..u3 (16 VALU adds against 16 MI MFMAs) and runs MI MFMAs per term and k-step.
// A (weights): v2w_pack_wino / the batched fold store the transformed weights in MFMA A-fragment order, [row block][chunk][segment]
// [unit][term], 1 KiB per fragment, a 4-deep ring in registers as in conv_tile_kernel.
// Tile: 64 output channels x 64 pairs (MI = 1), 4 accumulator sets = 64 registers per lane; launch bound three waves per SIMD (measured
// at B = 32 x T = 256: two waves per SIMD with the register-prefetched staging ran 10-20 % slower, MI = 2 at one wave slower still: 9.95 against 8.97 ms per forward).
// Tail tile: d ceil(L / 2d) pairs seldom fill the last tile of a row (dil 3, L = 1280: 642 pairs, the 11th tile holds 2, one live).  A column-wave with no
// output position below the end runs no segment and no epilogue, and the partial tail tiles of a problem are its last workgroups
// (wino_tile_order): stage 0's k = 11 launch 448 -> 430 us, stage 1's 464 -> 447 us.
// Epilogue: the output transform in registers, then bias [+ res_a*res + res_s] [+ add0 (+ add1) | + out] [/ out_div] per element
// in conv_tile_kernel's order; second outputs of a pair at or past L are not stored.  Fixed summation order, no atomics.
// Summed form (conv_wino_sum_kernel, v2w_conv1d_wino_sum_fwd): up to three convs of one dilation - the second convs of a stage's branches - on
// the same accumulators, one output transform, then t = y + ((b0 + b1) + b2); t += (in_0[go] + in_1[go]) + in_2[go]; t = t / out_div (the
// division above): NOT the rounding order of three launches that add r0, r1, r2 (B = 32 x T = 256: max |dy| = 3.7e-7 at max |y| = 0.40).
// Its epilogue loads the residuals of four rows (24 loads with three sources, the count a compile-time constant then) before the rows'
// output transform and stores - they were three dependent loads per stored element behind the last MFMA: the summed launches of stages
// 0 / 1 / 2 805 -> 789, 760 -> 740, 807 -> 767 us.  The sources are walked in branch order (wino_sum_order; any other order can be asked
// for, v2w_conv1d_wino_sum_fwd_order - none measured faster); bias and residual sums are by branch index whatever the walk.
// Fan-out form (conv_wino_fan_kernel, v2w_conv1d_wino_fan_fwd): up to three convs of one dilation over ONE input of at most 64 channels - the
// first convs of the 64-channel stage's branches - in one workgroup per tile: tables and the activated window staged once (the two chunk
// buffers hold its whole K extent), then branch after branch accumulate, transform, store to out_j, zero.  Each conv keeps the one-conv
// kernel's operations and their order, so its bits.  B = 32 x L = 20 480, k = (3, 7, 11): 893 us in 15 360 workgroups -> 750 us in 5 120.
// Upsampler form (conv_wino_up_kernel, v2w_convt1d_wino_fwd): ConvTranspose1d(k = 2 u, stride u) as one two-tap conv over u * C_out rows (row =
// channel * u + phase) on the two-tap segment - 3 products per output pair where the direct tile issues 4 - with a pixel-shuffle store straight
// from the accumulators (a lane's four consecutive rows are the u phases of 4 / u channels: 2 u contiguous output floats per channel) and
// conv_tile_kernel's per-tile BatchNorm sums.  B = 32 x T = 256: ups.1 / ups.2 / ups.3 219 / 225 / 158 -> 181 / 190 / 128 us.
// Host side: the forms share the tile constants (WinoTile), the launch geometry (wino_geometry: tiles, LDS rows and their bound, table offset,
// LDS bytes - a launcher passes only its form's halo, resident chunks, table rows and affine), the served-conv test (wino_served) and the
// TileArgs builder (wino_tile_args).  In the body the output transform is one lambda; the zeroing of the accumulators and the restarts of
// a weight stream stay written out at each site: as lambdas they changed hipcc's register assignment.
#include "v2w_tile.h"
#include "v2w_internal.h"
#include "v2w_wino.h"

namespace {

constexpr int WCK = 32;                 // channels per chunk
typedef TileGeom<32, WCK> WG;           // the LDS signal tile of conv_tile_kernel's 32-channel chunks (v2w_tile.h)
constexpr int WGPC = 4;                 // A fragments (units of 4 k-steps) per chunk and term
constexpr int WHMAX = 32;               // staging slots cover 2 NTP + 2 WHMAX rows
// The tile of <MI, WN>: the one set of constants the device body, the kernels' launchers and the host queries derive theirs from.
template <int MI, int WN> struct WinoTile {
    static constexpr int WM = 2, NTHREADS = 64 * WM * WN;
    static constexpr int MT = 32 * MI * WM, NTP = 32 * WN;             // output channels x output pairs of a workgroup
    static constexpr int XMAX = 2 * NTP + 2 * WHMAX;                   // the most LDS rows a tile may read (wino_geometry checks it)
    static constexpr int NPF = ((WCK / 2) * ((XMAX / 4 + 7) / 8 * 8) + NTHREADS - 1) / NTHREADS;      // staging items per thread
    static_assert(NTHREADS * NPF < 8 * 8192, "item index range of the magic division");
};
// (MI = 2, a 128 x 64-pair tile with 128 accumulators per lane, spills at two waves per SIMD and ran slower at one)
typedef WinoTile<1, 2> WT;              // the tile every entry point launches
__host__ __device__ inline int wino_tpos(int P, int d) { const int q = P / d; return 2 * d * q + (P - q * d); }
__host__ __device__ inline int wino_npairs(int L, int d) { return d * ((L + 2 * d - 1) / (2 * d)); }   // output pairs of a row of L positions

// Position tile `v` of a problem in launch order -> batch item b and tile tl of the item (v2w_tile.h places v on a workgroup).  Item-major
// (v = b * ntl + tl) unless the item's last tile is partial (tail_last: npairs % NTP != 0): that tile's dead column-waves do no matrix work,
// so the B tail tiles take the highest v - no full workgroup then queues behind a cheap one at the end of the problem.
__host__ __device__ inline void wino_tile_order(int v, int B, int ntl, bool tail_last, int& b, int& tl) {
    b = v / ntl; tl = v - b * ntl;
    if (tail_last) {
        const int nf = ntl - 1, nfull = B * nf;
        if (v >= nfull) { b = v - nfull; tl = nf; }
        else { b = v / nf; tl = v - b * nf; }
    }
}

// The summed form (v2w_conv1d_wino_sum_fwd): up to WSRC convs of one dilation whose results add - the second convs of a ResBlock2 stage's
// branches.  The output transform is linear, so every source's terms add into the same four accumulator classes: one workgroup walks the
// sources one after another (own input, weight stream, K, halo), pays prologue, output transform and epilogue once and writes only the sum.
// `p` holds what the sources share (and the first source walked); the input of each source is also its residual.
// in / wp / K / hl are in WALK order (launch_wino_sum picks it: it fixes which source's chunk 0 is staged under which source's last chunk and
// which source runs last, next to the epilogue); res / bias are in BRANCH order, so that the bias and residual sums keep their association
// (b0 + b1) + b2 and (t1_0 + t1_1) + t1_2 whatever the walk - only the accumulation order of the products follows it.
constexpr int WSRC = 3;
struct WinoSumArgs {
    TileArgs p;
    const float* in[WSRC]; const float* wp[WSRC];
    int K[WSRC], hl[WSRC];
    const float* res[WSRC]; const float* bias[WSRC];
    int nsrc;
};
// The fan-out form (v2w_conv1d_wino_fan_fwd): up to WSRC convs of one dilation over ONE input - the first convs of a ResBlock2 stage's
// branches - each with its own weight stream, bias and output.  At C_in <= 64 the kernel's two chunk buffers hold the whole K extent of the
// activated signal, so one workgroup stages it once (with the widest branch's halo: the LDS rows and pos0 serve every branch) and walks the
// branches one after another: accumulate, output transform, epilogue, store to out_j, zero the accumulators, next weight stream.  Every
// branch runs the one-conv kernel's operations in its order (same staged values, fragment order, epilogue expression): the same bits.
// `p` holds what the branches share (input, affines, residual, sizes; hl / hr: the widest branch's halo).
struct WinoFanArgs {
    TileArgs p;
    const float* wp[WSRC]; const float* bias[WSRC]; float* out[WSRC];
    int K[WSRC], hl[WSRC];
    int nsrc;
};
// The upsampler form (v2w_convt1d_wino_fwd): ConvTranspose1d(k = 2 U, stride U, padding U / 2) as ONE two-tap Conv1d over U * C_out rows
// (row = channel * U + phase; taps (w[phase + U], w[phase]) on (x[t - 1], x[t]), t = 0 .. L) followed by a pixel shuffle: the two-tap
// segment's 3 products per output pair (v2w_wino.h) where the direct tile issues 4.  `p` is the conv's problem: Cout = U * C_out ROWS, CoutT =
// C_out channels of `out` (B, C_out, U L), K = 2, dil = 1, hl = 1, hr = 0, L = the INPUT length (the conv has L + 1 output positions), `bias`
// per channel, `evec` = out is 8-byte aligned, `stats_part` as in conv_tile_kernel's transposed form.
template <int U> struct WinoUpArgs { TileArgs p; };
template <class A> struct wino_up_of { static constexpr int value = 0; };
template <int U> struct wino_up_of<WinoUpArgs<U>> { static constexpr int value = U; };
__device__ __forceinline__ const TileArgs& wino_problem(const MultiArgs& m, int pq) { return m.p[pq]; }
template <int U> __device__ __forceinline__ const TileArgs& wino_problem(const WinoUpArgs<U>& a, int) { return a.p; }
__device__ __forceinline__ const TileArgs& wino_problem(const WinoSumArgs& a, int) { return a.p; }
__device__ __forceinline__ const TileArgs& wino_problem(const WinoFanArgs& a, int) { return a.p; }

// LEN: per-item valid lengths, as in conv_tile_body (v2w_conv_mfma.hip): inputs at and past Lb = min(L, len[b] * len_mul) select 0, a tile
// whose first output position lies there returns at once; its own kernel name (conv_wino_len_kernel).
// ARGS = WinoSumArgs: the summed form (one problem per launch); WinoFanArgs: the fan-out form (one problem per launch, C_in <= 64, no LEN);
// MultiArgs: one conv per problem; WinoUpArgs<U>: the upsampler form (one problem per launch, no LEN).
template <int MI, int WN, int NPF, bool VEC, bool LEN, class ARGS>
__device__ __forceinline__ void conv_wino_body(const ARGS& m) {
    constexpr bool SUM = std::is_same<ARGS, WinoSumArgs>::value;
    constexpr bool FAN = std::is_same<ARGS, WinoFanArgs>::value;
    constexpr int UP = wino_up_of<ARGS>::value;              // the upsampler form's stride (0: a Conv1d)
    static_assert(!FAN || (MI == 1 && !LEN), "the fan-out form is written for MI = 1 without per-item lengths");
    static_assert(!UP || (MI == 1 && !LEN && (UP == 2 || UP == 4)), "the upsampler form is written for MI = 1, stride 2 / 4, without per-item lengths");
    typedef Frag<32> F;
    typedef F::acc_t acc_t;
    typedef WinoTile<MI, WN> T;
    constexpr int WM = T::WM, NTHREADS = T::NTHREADS, MT = T::MT, NTP = T::NTP;
    static_assert(NPF == T::NPF, "the launchers instantiate the kernels with the tile's own NPF");
    constexpr int RING = 4;

    extern __shared__ __attribute__((aligned(16))) float smem[];

    int pq = 0, id = blockIdx.x;
    if constexpr (!SUM && !FAN && !UP) { pq = tile_problem(m); id = blockIdx.x - m.start[pq]; }
    const TileArgs& p = wino_problem(m, pq);
    const int mtiles = p.Cout / MT;
    const TileId ti = tile_coords(mtiles, id);
    const int mt = ti.mt;
    if (ti.tile >= p.ntiles) return;
    const int d = p.dil;
    int b, tl;
    wino_tile_order(ti.tile, p.B, p.ntl, wino_npairs(UP ? p.L + 1 : p.L, d) % NTP != 0, b, tl);      // (UP: output positions t = 0 .. L)
    const int P0 = tl * NTP;                 // first output pair of the tile
    const int m0 = mt * MT;
    int Lb = p.L;                            // end of this item's sequence (LEN; else the tensor's)
    if constexpr (LEN) {
        const int lv = p.len[b] * p.len_mul;
        Lb = lv < p.L ? lv : p.L;
        if (wino_tpos(P0, d) >= Lb) return;  // the tile's first (smallest) output position lies past the item's end
    }

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lr = lane & 31;
    const int hk = lane >> 5;
    const int wm0 = (wave / WN) * (32 * MI);
    const int wn0 = (wave % WN) * 32;
    // a column-wave whose first (smallest) output position lies at or past the end stores nothing: it stages and keeps every barrier, but
    // runs no segment (no A-fragment load, no MFMA) and no epilogue - the tail tile of a row whose pairs do not fill it, a LEN item's last tile
    const bool live = wino_tpos(P0 + wn0, d) < (UP ? Lb + 1 : Lb);
    const int L = p.L;
    int K = p.K, hl = p.hl;                  // (SUM: of the source whose chunks are being multiplied)
    const float* sin = p.in;                 // the tensor the staging reads, pos0 the position of its LDS row 0 (floor to a float4) -
    int pos0 = (wino_tpos(P0, d) - hl) & ~3; // SUM: already the NEXT source's while the last chunk of a source is multiplied
    if constexpr (FAN) { K = m.K[0]; hl = m.hl[0]; }          // (p.hl: the widest branch's - pos0 and the LDS rows serve every branch)
    const float slope = p.slope;
    const int nch = p.Cin / WCK;
    const int bufsz = p.xrows * WG::RS;
    float* const etab = smem + p.atab_off;   // bias, res_a, res_s [MT] each (FAN: bias [WSRC][MT], then res_a, res_s)
    float* const atab = etab + (FAN ? WSRC + 2 : 3) * MT;     // folded CondBN affine of this batch item: a[Cin] then s[Cin]

    acc_t acc[4][MI];
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int i = 0; i < MI; ++i)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[c][i][e] = 0.f;

    // the output transform of accumulator element e of row block i: the pair's two outputs
    auto out_transform = [&](int e, int i, float (&y)[2]) {
        const float M0 = acc[0][i][e], M1 = acc[1][i][e], M2 = acc[2][i][e], M3 = acc[3][i][e];
        y[0] = (M0 + M1) + M2; y[1] = (M1 - M2) - M3;
    };

    // ---- signal staging: conv_tile_kernel's (an item = one slot-adjacent channel pair x 4 positions)
    const int nq = p.xrows >> 2;
    const int nq8 = (nq + 7) >> 3;
    const unsigned magic = (unsigned)(((1ull << 32) + nq8 - 1) / nq8);
    f32x4 pf[NPF][2];
    const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
    auto item = [&](int s, int& c0, int& row, bool& in_img, bool& in_seq) {
        int t = tid;
        asm volatile("" : "+v"(t));
        const int idx = t + s * NTHREADS;
        const int g = idx >> 4;
        const int pg = (int)__umulhi((unsigned)g, magic);
        const int quad = (g - pg * nq8) * 8 + (idx & 7);
        const int P = 2 * pg + ((idx >> 3) & 1);
        row = quad * 4;
        in_img = quad < nq && P < WCK / 2;
        c0 = WG::pair_c0(in_img ? P : 0);
        const int pos = pos0 + row;
        in_seq = in_img && pos >= 0 && pos < L;
    };
    auto prefetch = [&](int ci0) {
        const float* xsrc = sin + (size_t)(b * p.CinT + ci0) * L + pos0;
#pragma unroll
        for (int s = 0; s < NPF; ++s) {
            int c0, row; bool in_img, in_seq;
            item(s, c0, row, in_img, in_seq);
            pf[s][0] = zero4; pf[s][1] = zero4;
            if (in_seq) {
                pf[s][0] = *reinterpret_cast<const f32x4*>(xsrc + (size_t)c0 * L + row);
                pf[s][1] = *reinterpret_cast<const f32x4*>(xsrc + (size_t)(c0 + 2) * L + row);
            }
        }
    };
    auto commit = [&](int ci0, float* Xs) {
#pragma unroll
        for (int s = 0; s < NPF; ++s) {
            int c0, row; bool in_img, in_seq;
            item(s, c0, row, in_img, in_seq);
            if (!in_img) continue;
            float a0 = 1.f, s0 = 0.f, a1 = 1.f, s1 = 0.f;
            if (!SUM && p.in_a) {
                a0 = atab[ci0 + c0]; s0 = atab[p.Cin + ci0 + c0];
                a1 = atab[ci0 + c0 + 2]; s1 = atab[p.Cin + ci0 + c0 + 2];
            }
            float* dst = Xs + row * WG::RS + WG::slot(c0);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                f32x2 v = {0.f, 0.f};        // padding stays exactly 0 (it pads the ACTIVATED signal)
                if (in_seq && (!LEN || pos0 + row + e < Lb)) {      // (LEN: per element - Lb need not be a multiple of 4)
                    v[0] = v2w_lrelu(fmaf(a0, pf[s][0][e], s0), slope); v[1] = v2w_lrelu(fmaf(a1, pf[s][1][e], s1), slope);
                }
                *reinterpret_cast<f32x2*>(dst + e * WG::RS) = v;
            }
        }
    };
    auto stage_scalar = [&](int ci0, float* Xs) {   // any L / alignment: dword loads straight into LDS
        for (int c = wave; c < WCK; c += WM * WN) {
            const int ch = b * p.CinT + ci0 + c;
            const float* xsrc = sin + (size_t)ch * L;
            const float av = !SUM && p.in_a ? p.in_a[ch] : 1.f;
            const float sv = !SUM && p.in_s ? p.in_s[ch] : 0.f;
            float* dst = Xs + WG::slot(c);
            for (int j = lane; j < p.xrows; j += 64) {
                const int l = pos0 + j;
                float v = 0.f;
                if (l >= 0 && l < Lb) v = v2w_lrelu(fmaf(av, xsrc[l], sv), slope);
                dst[j * WG::RS] = v;
            }
        }
    };

    // ---- weight ring: fragments in consumption order, "next" is always +1 KiB per row block
    int nfrag = nch * (UP ? wino_seg_terms(2) : wino_terms(K)) * WGPC;
    const f32x4* ap[MI];
#pragma unroll
    for (int i = 0; i < MI; ++i)
        ap[i] = reinterpret_cast<const f32x4*>(p.wp) + ((size_t)((m0 + wm0) / 32 + i) * nfrag) * 64;
    int fidx = 0;
    f32x4 ar[RING][MI];
    const unsigned lane16 = (unsigned)lane * 16u;
    auto load_next = [&](f32x4 (&a)[MI]) {
        const int f = fidx < nfrag ? fidx : nfrag - 1;
        unsigned l16 = lane16;
        asm volatile("" : "+v"(l16));
#pragma unroll
        for (int i = 0; i < MI; ++i)
            a[i] = *reinterpret_cast<const f32x4*>(reinterpret_cast<const char*>(ap[i] + (size_t)f * 64) + l16);
        ++fidx;
    };

    // ---- one segment of NTAP taps whose x0 sits at `x` (this lane's float4 of unit 0), rows `dstep` floats apart.  Each segment
    // consumes NTERM * 4 fragments - a multiple of the ring - so every segment starts at ring slot 0.
    auto segment = [&](auto ntap_c, const float* x, int dstep) {
        constexpr int NTAP = decltype(ntap_c)::value;
        constexpr int NX = NTAP + 1;
        constexpr int NTERM = wino_seg_terms(NTAP);
#pragma unroll
        for (int gg = 0; gg < WGPC; ++gg) {
            f32x4 xr[NX];
#pragma unroll
            for (int j = 0; j < NX; ++j) xr[j] = *reinterpret_cast<const f32x4*>(x + j * dstep + 8 * gg);
            f32x4 u[NTERM];
            if constexpr (NTAP == 3) {
                u[0] = xr[0] - xr[2]; u[1] = xr[1] + xr[2];
                u[2] = xr[2] - xr[1]; u[3] = xr[1] - xr[3];
            } else if constexpr (NTAP == 2) {
                u[0] = xr[0] - xr[1]; u[1] = xr[1]; u[2] = xr[1] - xr[2];
            } else {
                u[0] = xr[0]; u[1] = xr[1];
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int t = 0; t < NTERM; ++t) {
                const int cls = NTAP == 3 ? t : (NTAP == 2 ? (t == 2 ? 3 : t) : (t == 1 ? 3 : 0));    // accumulator class of the term
                const int slot = (gg * NTERM + t) % RING;
                load_next(ar[(slot + RING - 1) % RING]);
#pragma unroll
                for (int kk = 0; kk < 4; ++kk)
#pragma unroll
                    for (int i = 0; i < MI; ++i) acc[cls][i] = F::mfma(ar[slot][i][kk], u[t][kk], acc[cls][i]);
            }
        }
    };

    // ---- prologue: epilogue constants, affine table, chunk 0, first fragments
    int nsrc = 1;
    if constexpr (SUM || FAN) nsrc = m.nsrc;
    for (int c = tid; c < MT; c += NTHREADS) {
        if constexpr (FAN) {
            for (int j = 0; j < nsrc; ++j) etab[j * MT + c] = m.bias[j] ? m.bias[j][m0 + c] : 0.f;
            etab[WSRC * MT + c] = p.res_a ? p.res_a[b * p.Cout + m0 + c] : 1.f;
            etab[(WSRC + 1) * MT + c] = p.res_a ? p.res_s[b * p.Cout + m0 + c] : 0.f;
            continue;
        }
        if constexpr (UP) {                  // row c of the tile is channel (m0 + c) / UP
            etab[c] = p.bias ? p.bias[(m0 + c) / UP] : 0.f;
            continue;
        }
        if constexpr (SUM) {                 // (b0 + b1) + b2
            float bv = m.bias[0] ? m.bias[0][m0 + c] : 0.f;
            for (int j = 1; j < nsrc; ++j) bv += m.bias[j] ? m.bias[j][m0 + c] : 0.f;
            etab[c] = bv;
            continue;
        }
        etab[c] = p.bias ? p.bias[m0 + c] : 0.f;
        etab[MT + c] = p.res_a ? p.res_a[b * p.Cout + m0 + c] : 1.f;
        etab[2 * MT + c] = p.res_a ? p.res_s[b * p.Cout + m0 + c] : 0.f;
    }
    if (!SUM && p.in_a) {
        for (int c = tid; c < p.Cin; c += NTHREADS) {
            atab[c] = p.in_a[b * p.Cin + c];
            atab[p.Cin + c] = p.in_s[b * p.Cin + c];
        }
        __syncthreads();
    }
    if constexpr (VEC) { prefetch(0); commit(0, smem); }
    else stage_scalar(0, smem);
#pragma unroll
    for (int g = 0; g + 1 < RING; ++g) load_next(ar[g]);
    __builtin_amdgcn_sched_barrier(0);
    __syncthreads();

    const int P = P0 + wn0 + lr;                   // this lane's output pair
    const int t0 = wino_tpos(P, d);                // ... and its first output position
    int lbase = (t0 - hl - pos0) * WG::RS + 4 * hk;           // x of tap 0 for output t0, unit 0
    const int dstep = d * WG::RS;
    typedef std::integral_constant<int, 3> S3;
    typedef std::integral_constant<int, 2> S2;
    typedef std::integral_constant<int, 1> S1;
    // FAN: one branch's output transform and epilogue, t = y + bias_j [+ fmaf(res_a, res[go], res_s)] as the one-conv epilogue below computes
    // it; the residual loads of EB rows are issued before the rows' output transform and stores (as in the summed epilogue), and are
    // reloaded per branch - kept across the branches they would cost 32 registers next to the 64 accumulators.
    auto fan_epilogue = [&](int j) {
        if constexpr (FAN) {
            float* const outp = m.out[j];
            const float* const res = p.res;
            const float* const bt = etab + j * MT;
            constexpr int EB = 4;
            // (the addresses are the same for every branch: behind this opaque copy they are computed per branch, in the epilogue -
            // hoisted in front of the branch loop the 32 row addresses lived in scratch)
            int lq = tid;
            asm volatile("" : "+v"(lq));
            const int tq = wino_tpos(P0 + wn0 + (lq & 31), d), hq = (lq & 63) >> 5;      // t0 and hk again, from the thread index
#pragma unroll
            for (int e0 = 0; e0 < 16; e0 += EB) {
                float rv[EB][2];
#pragma unroll
                for (int q = 0; q < EB; ++q) {
                    const size_t rowoff = ((size_t)b * p.CoutT + m0 + wm0 + F::row(e0 + q, hq)) * L;
#pragma unroll
                    for (int h = 0; h < 2; ++h) {
                        const int pos = tq + h * d;
                        rv[q][h] = (res && pos < L) ? res[rowoff + pos] : 0.f;
                    }
                }
#pragma unroll
                for (int q = 0; q < EB; ++q) {
                    const int e = e0 + q, col = wm0 + F::row(e, hq);
                    float y[2];
                    out_transform(e, 0, y);
                    const size_t rowoff = ((size_t)b * p.CoutT + m0 + col) * L;
                    const float bias = bt[col], ra = etab[WSRC * MT + col], rs = etab[(WSRC + 1) * MT + col];
#pragma unroll
                    for (int h = 0; h < 2; ++h) {
                        const int pos = tq + h * d;
                        if (pos >= L) continue;
                        float t = y[h] + bias;
                        if (res) t += fmaf(ra, rv[q][h], rs);
                        outp[rowoff + pos] = t;
                    }
                }
            }
        }
    };
    // SUM: the sources one after another on the same accumulators; the double buffer runs on across a source boundary (the last chunk of a
    // source stages chunk 0 of the next: one prologue staging per workgroup), the fragment pointer and the weight ring restart there.
    for (int js = 0, cc = 0; js < nsrc; ++js) {
        for (int ch = 0; ch < nch; ++ch, ++cc) {
            const int par = SUM ? cc : ch;
            const float* Xs = smem + (par & 1) * bufsz;
            float* Xn = smem + ((par + 1) & 1) * bufsz;
            bool more = ch + 1 < nch;
            if constexpr (FAN) more = more && js == 0;     // branch 0 stages chunk 1 into the other buffer; the later branches find both there
            int cn = (ch + 1) * WCK;
            if (live) {
                const float* xt = Xs + lbase;
                if constexpr (UP) segment(S2{}, xt, dstep);
                else {
                    int s = 0;
                    for (; s + 3 <= K; s += 3) segment(S3{}, xt + s * dstep, dstep);
                    if (K - s == 2) segment(S2{}, xt + s * dstep, dstep);
                    else if (K - s == 1) segment(S1{}, xt + s * dstep, dstep);
                }
            }
            if constexpr (SUM) {
                if (!more && js + 1 < nsrc) {
                    more = true; cn = 0;
                    K = m.K[js + 1]; hl = m.hl[js + 1]; sin = m.in[js + 1];
                    pos0 = (wino_tpos(P0, d) - hl) & ~3;
                    lbase = (t0 - hl - pos0) * WG::RS + 4 * hk;
                    nfrag = nch * wino_terms(K) * WGPC;
#pragma unroll
                    for (int i = 0; i < MI; ++i)
                        ap[i] = reinterpret_cast<const f32x4*>(m.wp[js + 1]) + ((size_t)((m0 + wm0) / 32 + i) * nfrag) * 64;
                    fidx = 0;
#pragma unroll
                    for (int g = 0; g + 1 < RING; ++g) load_next(ar[g]);
                }
            }
            if (more) {
                if constexpr (VEC) { prefetch(cn); commit(cn, Xn); }
                else stage_scalar(cn, Xn);
                __syncthreads();
            }
        }
        if constexpr (FAN) {
            // branch boundary (no barrier from here on: neither buffer is overwritten, the tables are constant): the next branch's stream,
            // K, fragment count and base row, the ring restarted - its first fragments fly under this branch's epilogue - then the
            // accumulators start from zero.  pos0 and sin stay.
            if (!live) return;
            if (js + 1 < nsrc) {
                K = m.K[js + 1];
                lbase += (hl - m.hl[js + 1]) * WG::RS;        // = (t0 - hl_j - pos0) * RS + 4 hk of the next branch
                hl = m.hl[js + 1];
                nfrag = nch * wino_terms(K) * WGPC;
#pragma unroll
                for (int i = 0; i < MI; ++i)
                    ap[i] = reinterpret_cast<const f32x4*>(m.wp[js + 1]) + ((size_t)((m0 + wm0) / 32 + i) * nfrag) * 64;
                fidx = 0;
#pragma unroll
                for (int g = 0; g + 1 < RING; ++g) load_next(ar[g]);
            }
            fan_epilogue(js);
#pragma unroll
            for (int c = 0; c < 4; ++c)
#pragma unroll
                for (int i = 0; i < MI; ++i)
#pragma unroll
                    for (int e = 0; e < 16; ++e) acc[c][i][e] = 0.f;
        }
    }
    if constexpr (FAN) return;

    if constexpr (UP) {
        // ---- upsampler epilogue: output transform (the two-tap segment feeds M0, M1, M3: y(t) = M0 + M1, y(t + 1) = M1 - M3), + bias[channel],
        // pixel-shuffle store out[b][c][UP t + phase - PAD].  A lane's four consecutive rows are 4 / UP channels x UP phases, so with its pair
        // (t0, t0 + 1) it owns 2 UP contiguous output floats per channel from o0 = UP t0 - PAD on; t0 is even, so o0 has PAD's parity and the
        // run goes out as 8-byte stores (UP = 4: four; UP = 2: a float, a pair, a float).  Outputs outside [0, UP L) are not stored.
        // stats_part: per (tile, channel) (sum, sumsq) of the stored values - lanes, then the 32 lanes of a row through shuffles, then the WN
        // column-waves through LDS in wave order, one slot per (tile, channel); no atomics.  A dead column-wave contributes zeros.
        constexpr int PAD = UP / 2, NV = 2 * UP, CT = MT / UP;
        float* const stats = p.stats_part;
        if (!live && !stats) return;
        float* const outp = p.out;
        const int Lo = UP * L, o0 = UP * t0 - PAD;
        const bool evec = p.evec != 0;
        float* const red = etab + MT;         // [WN][CT][2] (the residual-affine slots of the table: this form has no residual)
#pragma unroll
        for (int r0 = 0; r0 < 16; r0 += UP) {
            const int row = wm0 + F::row(r0, hk);             // first row of the channel inside the tile (a multiple of UP)
            const float bias = etab[row];
            float v[NV];
#pragma unroll
            for (int ph = 0; ph < UP; ++ph) {
                const float M0 = acc[0][0][r0 + ph], M1 = acc[1][0][r0 + ph], M3 = acc[3][0][r0 + ph];
                v[ph] = (M0 + M1) + bias; v[UP + ph] = (M1 - M3) + bias;
            }
            float* const orow = outp + ((size_t)b * p.CoutT + (m0 + row) / UP) * Lo;
            float s1 = 0.f, s2 = 0.f;
#pragma unroll
            for (int i = 0; i < NV; ++i) {
                const int o = o0 + i;
                const bool ok = live && o >= 0 && o < Lo;
                if (ok) { s1 += v[i]; s2 = fmaf(v[i], v[i], s2); }
                if (!ok) continue;
                // (element i opens an aligned pair when o is even, i.e. i has PAD's parity: Lo is even, so its partner is inside too)
                if (((i ^ PAD) & 1) == 0 && i + 1 < NV && evec) { f32x2 w = {v[i], v[i + 1]}; *reinterpret_cast<f32x2*>(orow + o) = w; }
                else if (((i ^ PAD) & 1) == 0 || i == 0 || !evec) orow[o] = v[i];
            }
            if (stats) {
#pragma unroll
                for (int off = 16; off > 0; off >>= 1) { s1 += __shfl_xor(s1, off, 64); s2 += __shfl_xor(s2, off, 64); }
                if (lr == 0) {
                    red[((wave % WN) * CT + row / UP) * 2 + 0] = s1;
                    red[((wave % WN) * CT + row / UP) * 2 + 1] = s2;
                }
            }
        }
        if (stats) {
            __syncthreads();
            for (int c = tid; c < CT; c += NTHREADS) {
                float t1 = 0.f, t2 = 0.f;
#pragma unroll
                for (int w = 0; w < WN; ++w) { t1 += red[(w * CT + c) * 2]; t2 += red[(w * CT + c) * 2 + 1]; }
                stats[((size_t)ti.tile * p.CoutT + m0 / UP + c) * 2 + 0] = t1;
                stats[((size_t)ti.tile * p.CoutT + m0 / UP + c) * 2 + 1] = t2;
            }
        }
        return;
    }

    if (!live) return;
    // ---- epilogue: output transform, then + bias [+ residual] [+ addends | + out] [/ out_div], conv_tile_kernel's order
    float* const outp = p.out;
    const float dinv = p.out_div != 0.f ? 1.f / p.out_div : 1.f;
    if constexpr (SUM) {
        // The sources' own inputs are their residuals: t = (y + bias) + ((t1_0 + t1_1) + t1_2).  The residual loads of EB rows (2 EB NS
        // of them) are issued before the rows' output transform and stores, so that they fly together: one by one behind each store
        // (the output may alias an input for all the compiler knows) they were 3 dependent round trips per stored element after the last MFMA.
        // NS: the number of sources at compile time (3: a ResBlock2 stage), 0: m.nsrc at run time.
        auto epilogue = [&](auto ns_c) {
            constexpr int NS = decltype(ns_c)::value;
            constexpr int NR = NS ? NS : WSRC;
            constexpr int EB = 4;
            const int ns = NS ? NS : nsrc;
#pragma unroll
            for (int e0 = 0; e0 < 16; e0 += EB) {
                float rv[EB][2][NR];
#pragma unroll
                for (int q = 0; q < EB; ++q) {
                    const size_t rowoff = ((size_t)b * p.CoutT + m0 + wm0 + F::row(e0 + q, hk)) * L;
#pragma unroll
                    for (int h = 0; h < 2; ++h) {
                        const int pos = t0 + h * d;
#pragma unroll
                        for (int j = 0; j < NR; ++j) rv[q][h][j] = (pos < L && j < ns) ? m.res[j][rowoff + pos] : 0.f;
                    }
                }
#pragma unroll
                for (int q = 0; q < EB; ++q) {
                    const int e = e0 + q, col = wm0 + F::row(e, hk);
                    float y[2];
                    out_transform(e, 0, y);
                    const size_t rowoff = ((size_t)b * p.CoutT + m0 + col) * L;
                    const float bias = etab[col];
#pragma unroll
                    for (int h = 0; h < 2; ++h) {
                        const int pos = t0 + h * d;
                        if (pos >= L) continue;
                        float t = y[h] + bias;
                        float r = rv[q][h][0];
                        if (NS == 3) r = (r + rv[q][h][1]) + rv[q][h][2];
                        else {
#pragma unroll
                            for (int j = 1; j < NR; ++j) if (j < ns) r += rv[q][h][j];
                        }
                        t += r;
                        if (p.out_div != 0.f) t = v2w_div_by(t, p.out_div, dinv);
                        outp[rowoff + pos] = t;
                    }
                }
            }
        };
        static_assert(!SUM || MI == 1, "the summed form's epilogue is written for MI = 1");
        if (nsrc == 3) epilogue(std::integral_constant<int, 3>{});
        else epilogue(std::integral_constant<int, 0>{});
        return;
    }
#pragma unroll
    for (int i = 0; i < MI; ++i) {
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int col = wm0 + i * 32 + F::row(e, hk);
            float y[2];
            out_transform(e, i, y);
            const size_t rowoff = ((size_t)b * p.CoutT + m0 + col) * L;
            const float bias = etab[col], ra = etab[MT + col], rs = etab[2 * MT + col];
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int pos = t0 + h * d;
                if (pos >= L) continue;
                const size_t go = rowoff + pos;
                float t = y[h] + bias;
                if (p.res) t += fmaf(ra, p.res[go], rs);
                if (p.add1) t += p.add0[go] + p.add1[go];      // (add0 + add1) + value: the reference's `xs += ...` order
                else if (p.accumulate) t += outp[go];
                else if (p.add0) t += p.add0[go];
                if (p.out_div != 0.f) t = v2w_div_by(t, p.out_div, dinv);
                outp[go] = t;
            }
        }
    }
}

template <int MI, int WN, int NPF, bool VEC>
__global__ void __launch_bounds__(128 * WN, 3)
conv_wino_kernel(const MultiArgs m) {
    conv_wino_body<MI, WN, NPF, VEC, false>(m);
}

template <int MI, int WN, int NPF, bool VEC>
__global__ void __launch_bounds__(128 * WN, 3)
conv_wino_len_kernel(const MultiArgs m) {
    conv_wino_body<MI, WN, NPF, VEC, true>(m);
}

template <int MI, int WN, int NPF, bool VEC>
__global__ void __launch_bounds__(128 * WN, 3)
conv_wino_sum_kernel(const WinoSumArgs a) {
    conv_wino_body<MI, WN, NPF, VEC, false>(a);
}

template <int MI, int WN, int NPF, bool VEC>
__global__ void __launch_bounds__(128 * WN, 3)
conv_wino_sum_len_kernel(const WinoSumArgs a) {
    conv_wino_body<MI, WN, NPF, VEC, true>(a);
}

template <int MI, int WN, int NPF, bool VEC>
__global__ void __launch_bounds__(128 * WN, 3)
conv_wino_fan_kernel(const WinoFanArgs a) {
    conv_wino_body<MI, WN, NPF, VEC, false>(a);
}

template <int U, int MI, int WN, int NPF, bool VEC>
__global__ void __launch_bounds__(128 * WN, 3)
conv_wino_up_kernel(const WinoUpArgs<U> a) {
    conv_wino_body<MI, WN, NPF, VEC, false>(a);
}

// The launch geometry of a problem, the one place that computes it (the four launchers and v2w_convt1d_wino_tiles call it): position tiles
// (ntl per item, ntiles) of `npos` output positions, the LDS rows of the widest tile for the halo hl / hr (xrows), the offset of the
// prologue tables behind `resident_chunks` chunk buffers (atab_off) and in *lds the dynamic LDS bytes with `etab_rows` epilogue rows of MT
// floats [+ the affine table].  p.xrows only grows (a fresh problem holds 0): the summed form calls this once per source and so sizes the
// launch for the widest.  V2W_E_SHAPE: more rows than the staging slots cover, or more tiles than an int holds.
template <class T>
int wino_geometry(TileArgs& p, int npos, int hl, int hr, int resident_chunks, int etab_rows, bool affine, size_t* lds) {
    const int d = p.dil;
    p.ntl = (wino_npairs(npos, d) + T::NTP - 1) / T::NTP;
    const long long ntiles = (long long)p.B * p.ntl;
    if (ntiles >= (1ll << 31)) return V2W_E_SHAPE;
    p.ntiles = (int)ntiles;
    int rows = p.xrows;                     // LDS rows the widest tile reads: x_K of the last pair's second output
    for (int tl = 0; tl < p.ntl; ++tl) {
        const int P0 = tl * T::NTP;
        const int pos0 = (wino_tpos(P0, d) - hl) & ~3;
        const int r = wino_tpos(P0 + T::NTP - 1, d) + d + hr - pos0 + 1;
        if (r > rows) rows = r;
    }
    p.xrows = (rows + 3) & ~3;
    if (p.xrows > T::XMAX) return V2W_E_SHAPE;
    p.atab_off = resident_chunks * p.xrows * WG::RS;
    *lds = ((size_t)p.atab_off + etab_rows * T::MT + (affine ? 2 * p.Cin : 0)) * sizeof(float);
    return 0;
}
// ... with the inputs of the forms that run one conv per problem (one-conv, upsampler): own halo, two chunk buffers when there is a second
// chunk, bias / res_a / res_s rows, the affine table when the problem has one
template <class T>
int wino_geometry_conv(TileArgs& p, int npos, size_t* lds) {
    return wino_geometry<T>(p, npos, p.hl, p.hr, p.Cin / WCK > 1 ? 2 : 1, 3, p.in_a != nullptr, lds);
}
inline bool wino_vec4(const TileArgs& p) { return p.L % 4 == 0 && v2w_al16(p.in); }      // float4 staging: rows of whole, aligned quads

// One conv per problem.  V2W_E_SHAPE also for a launch of at most `min_wgs` live workgroups (the caller's size rule).
template <int MI, int WN>
int launch_wino(const TileArgs* ps, int nprob, long min_wgs, hipStream_t stream) {
    typedef WinoTile<MI, WN> T;
    constexpr int NPF = T::NPF;
    MultiArgs m{};
    size_t lds = 0;
    int blocks[V2W_MAX_MULTI];
    bool vec = true;
    long wgs = 0;
    for (int i = 0; i < nprob; ++i) {
        TileArgs& p = m.p[i] = ps[i];
        if (p.Cout % T::MT != 0) return V2W_E_SHAPE;
        size_t l;
        if (const int rc = wino_geometry_conv<T>(p, p.L, &l)) return rc;
        if (l > lds) lds = l;
        p.vec4 = wino_vec4(p);
        vec = vec && p.vec4;
        blocks[i] = tile_blocks(p.ntiles, p.Cout / T::MT);
        wgs += (long)p.ntiles * (p.Cout / T::MT);
    }
    if (wgs <= min_wgs) return V2W_E_SHAPE;
    const int grid = v2w_fill_starts(m.start, V2W_MAX_MULTI, blocks, nprob);
    const bool lens = m.p[0].len != nullptr;      // (all problems of the launch or none: v2w_conv1d_wino)
    auto kern = lens ? (vec ? conv_wino_len_kernel<MI, WN, NPF, true> : conv_wino_len_kernel<MI, WN, NPF, false>)
                    : (vec ? conv_wino_kernel<MI, WN, NPF, true> : conv_wino_kernel<MI, WN, NPF, false>);
    return v2w_launch_lds(kern, dim3(grid), dim3(T::NTHREADS), lds, stream, m);
}

// The summed form: ps[0 .. nsrc) are the sources (shared B, C, L, dil, slope, out, out_div, len); one problem, one grid.
// The order in which a workgroup of the summed form walks its sources (branch indices; Ks: their kernel sizes).  Branch order: on MI355X
// k = 3 last, longest first and the other four orders of k = (3, 7, 11) all ran within the launches' own spread of it at C = 256 / 128 / 64
// (profiles/r14_cfg2_wino_sum_walk_orders.txt), and this one keeps the 64-channel stage's accumulation order.
inline void wino_sum_order(const int* Ks, int nsrc, int* walk) {
    (void)Ks;
    for (int j = 0; j < nsrc; ++j) walk[j] = j;
}

// `order`: the walk order, a permutation of 0 .. nsrc - 1 (null: wino_sum_order's).
template <int MI, int WN>
int launch_wino_sum(const TileArgs* ps, int nsrc, const int32_t* order, hipStream_t stream) {
    typedef WinoTile<MI, WN> T;
    constexpr int NPF = T::NPF;
    WinoSumArgs a{};
    int walk[WSRC];
    int Ks[WSRC];
    for (int j = 0; j < nsrc; ++j) Ks[j] = ps[j].K;
    wino_sum_order(Ks, nsrc, walk);
    if (order) {
        unsigned seen = 0;
        for (int j = 0; j < nsrc; ++j) {
            if (order[j] < 0 || order[j] >= nsrc || (seen >> order[j] & 1u)) return V2W_E_ARG;
            seen |= 1u << order[j];
            walk[j] = order[j];
        }
    }
    TileArgs p = ps[walk[0]];
    if (p.Cout % T::MT != 0) return V2W_E_SHAPE;
    const int nbuf = nsrc * (p.Cin / WCK) > 1 ? 2 : 1;
    size_t lds = 0;
    bool vec = true;
    for (int j = 0; j < nsrc; ++j) {        // (the rows of the widest source: wino_geometry keeps the maximum)
        if (const int rc = wino_geometry<T>(p, p.L, ps[j].hl, ps[j].hr, nbuf, 3, false, &lds)) return rc;
        vec = vec && wino_vec4(ps[j]);
        const TileArgs& w = ps[walk[j]];
        a.in[j] = w.in; a.wp[j] = w.wp; a.K[j] = w.K; a.hl[j] = w.hl;
        a.res[j] = ps[j].in; a.bias[j] = ps[j].bias;
    }
    a.nsrc = nsrc;
    p.vec4 = vec;
    a.p = p;
    const int grid = tile_blocks(p.ntiles, p.Cout / T::MT);
    auto kern = p.len ? (vec ? conv_wino_sum_len_kernel<MI, WN, NPF, true> : conv_wino_sum_len_kernel<MI, WN, NPF, false>)
                      : (vec ? conv_wino_sum_kernel<MI, WN, NPF, true> : conv_wino_sum_kernel<MI, WN, NPF, false>);
    return v2w_launch_lds(kern, dim3(grid), dim3(T::NTHREADS), lds, stream, a);
}

// The fan-out form: ps[0 .. nsrc) are the branches (shared in, in_a / in_s, res, res_a / res_s, B, C, L, dil, slope); one problem, one grid
// of one workgroup per tile.  C_in of at most two chunks: the double buffer then holds the whole activated window (V2W_E_SHAPE otherwise).
template <int MI, int WN>
int launch_wino_fan(const TileArgs* ps, int nsrc, hipStream_t stream) {
    typedef WinoTile<MI, WN> T;
    constexpr int NPF = T::NPF;
    WinoFanArgs a{};
    TileArgs p = ps[0];
    const int nch = p.Cin / WCK;
    if (p.Cout % T::MT != 0 || nch > 2) return V2W_E_SHAPE;
    int hmax = 0;
    for (int j = 0; j < nsrc; ++j) {
        a.wp[j] = ps[j].wp; a.bias[j] = ps[j].bias; a.out[j] = ps[j].out; a.K[j] = ps[j].K; a.hl[j] = ps[j].hl;
        if (ps[j].hl > hmax) hmax = ps[j].hl;
    }
    a.nsrc = nsrc;
    p.hl = p.hr = hmax;                     // (the widest branch's rows serve every branch; all nch chunks stay resident)
    size_t lds;
    if (const int rc = wino_geometry<T>(p, p.L, hmax, hmax, nch, WSRC + 2, p.in_a != nullptr, &lds)) return rc;
    const bool vec = p.vec4 = wino_vec4(p);
    a.p = p;
    const int grid = tile_blocks(p.ntiles, p.Cout / T::MT);
    auto kern = vec ? conv_wino_fan_kernel<MI, WN, NPF, true> : conv_wino_fan_kernel<MI, WN, NPF, false>;
    return v2w_launch_lds(kern, dim3(grid), dim3(T::NTHREADS), lds, stream, a);
}

// Which transposed convs the upsampler form serves: k == 2 u, u in {2, 4}, C_in % 32 == 0 and >= 64, u * C_out % 64 == 0, fp32 tensors.
int wino_up_shape(const v2w_convt1d_args* a) {
    if (!a) return V2W_E_ARG;
    if (a->B <= 0 || a->C_in <= 0 || a->C_out <= 0 || a->L <= 0 || a->k <= 0 || a->u <= 0 || a->io_bf16 != 0) return V2W_E_ARG;
    if ((a->u != 2 && a->u != 4) || a->k != 2 * a->u) return V2W_E_SHAPE;
    if (a->C_in % WCK != 0 || a->C_in < 64 || (a->u * a->C_out) % WT::MT != 0) return V2W_E_SHAPE;
    if ((long long)a->u * a->L >= (1ll << 31) - 4 * WT::NTP * a->u) return V2W_E_SHAPE;      // (output positions are ints)
    return 0;
}
// The upsampler form's problem (as WinoUpArgs describes it) and its launch geometry: the launcher and the tile query share both, so the
// planner's bn.part{i} rows are the launch's tiles.  The conv has L + 1 output positions.
TileArgs wino_up_problem(const v2w_convt1d_args* a, const float* in_a, const float* in_s) {
    TileArgs p{};
    p.in = a->in; p.in_a = in_a; p.in_s = in_s; p.wp = a->wp; p.bias = a->bias; p.out = a->out; p.stats_part = a->stats_part;
    p.B = a->B; p.Cin = p.CinT = a->C_in; p.Cout = a->u * a->C_out; p.CoutT = a->C_out; p.L = a->L; p.K = 2; p.dil = 1;
    p.hl = 1; p.hr = 0; p.pad = a->u / 2; p.up_u = a->u;
    p.slope = a->slope;
    return p;
}
inline int wino_up_geometry(TileArgs& p, size_t* lds) { return wino_geometry_conv<WT>(p, p.L + 1, lds); }

template <int U>
int launch_wino_up(TileArgs p, hipStream_t stream) {
    size_t lds;
    if (const int rc = wino_up_geometry(p, &lds)) return rc;
    const bool vec = p.vec4 = wino_vec4(p);
    p.evec = (reinterpret_cast<uintptr_t>(p.out) & 7) == 0;
    WinoUpArgs<U> a{};
    a.p = p;
    const int grid = tile_blocks(p.ntiles, p.Cout / WT::MT);
    auto kern = vec ? conv_wino_up_kernel<U, 1, 2, WT::NPF, true> : conv_wino_up_kernel<U, 1, 2, WT::NPF, false>;
    return v2w_launch_lds(kern, dim3(grid), dim3(WT::NTHREADS), lds, stream, a);
}

// wpw float index o = (((mb * nch + ch) * nfr + fi) * 64 + lane) * 4 + j, nfr = wino_terms(k) * 4, fragment fi = (segment, unit gg, term)
// (wino_frag) holds the term's transformed weight at channel ch*32 + gg*8 + 2j + lane/32, output channel mb*32 + lane%32.
__global__ void __launch_bounds__(256)
pack_wino_kernel(const float* __restrict__ wf, float* __restrict__ wp, int K, int Cin, int Cout) {
    const int nch = Cin / WCK, nfr = wino_terms(K) * WGPC;
    const size_t total = (size_t)(Cout / 32) * nch * nfr * 256;
    for (size_t o = (size_t)blockIdx.x * 256 + threadIdx.x; o < total; o += (size_t)gridDim.x * 256) {
        const int j = o & 3, lane = (o >> 2) & 63;
        size_t rest = o >> 8;
        const int fi = rest % nfr; rest /= nfr;
        const int ch = rest % nch;
        const int mb = rest / nch;
        int s0, ntap, gg, term;
        wino_frag(K, WGPC, fi, s0, ntap, gg, term);
        const int c = ch * WCK + gg * 8 + 2 * j + lane / 32, co = mb * 32 + lane % 32;
        auto g = [&](int t) { return t < ntap ? wf[((size_t)(s0 + t) * Cin + c) * Cout + co] : 0.f; };
        wp[o] = wino_weight(ntap, term, g(0), g(1), g(2));
    }
}

// Which Conv1d problems the kernel serves, whatever the form: C_in % 32 == 0 and >= 64, C_out % 64 == 0, odd k >= 3 with symmetric padding,
// plain unit-stride input, no channel slices, none of the backward / discriminator epilogues.
bool wino_served(const v2w_conv1d_args* q) {
    return q->C_in % WCK == 0 && q->C_in >= 64 && q->C_out % WT::MT == 0 && wino_terms(q->k) != 0 && q->pad_left < 0
        && q->in_stride <= 1 && !q->mask_src && !q->rowsum_part && (q->out_slope == 0.f || q->out_slope == 1.f)
        && (q->in_ct <= 0 || q->in_ct == q->C_in) && (q->out_ct <= 0 || q->out_ct == q->C_out);
}
// ... and the problem of a served conv
TileArgs wino_tile_args(const v2w_conv1d_args* q, const int32_t* len, int len_mul) {
    TileArgs p{};
    p.len = len; p.len_mul = len_mul;
    p.in = q->in; p.in_a = q->in_a; p.in_s = q->in_s; p.wp = q->wp; p.bias = q->bias;
    p.res = q->res; p.res_a = q->res_a; p.res_s = q->res_s; p.out = q->out;
    p.add0 = q->add0; p.add1 = q->add1;
    p.B = q->B; p.Cin = q->C_in; p.Cout = q->C_out; p.L = q->L; p.K = q->k; p.dil = q->dil;
    p.CinT = q->C_in; p.CoutT = q->C_out;
    p.hl = p.hr = q->dil * (q->k - 1) / 2;
    p.slope = q->slope; p.accumulate = q->accumulate; p.out_div = q->out_div;
    return p;
}

}  // namespace

// V2W_ALGO_WINO (V2W_E_SHAPE: not served; the caller then uses the direct-form f32 MFMA kernel): what wino_served serves, in launches of
// more than 128 workgroups of 64 channels x 64 pairs.
int v2w_conv1d_wino(const v2w_conv1d_args* a, int n, hipStream_t stream, const int32_t* len, int len_mul) {
    if (n < 1 || n > V2W_MAX_MULTI) return V2W_E_ARG;
    TileArgs ps[V2W_MAX_MULTI];
    for (int i = 0; i < n; ++i) {
        const v2w_conv1d_args* q = a + i;
        if (q->B != a->B || q->C_in != a->C_in || q->C_out != a->C_out || q->L != a->L || !wino_served(q)) return V2W_E_SHAPE;
        if (!q->wp) return V2W_E_ARG;
        if (len && len_mul < 1) return V2W_E_ARG;
        ps[i] = wino_tile_args(q, len, len_mul);
    }
    return launch_wino<1, 2>(ps, n, 128, stream);     // (the f32 MFMA path splits launches of <= 128 workgroups over C_in: inference at B = 1)
}

// The summed form (include/vec2wav_hip.h): out = (sum_j in_j + sum_j conv_j(lrelu(in_j)) + sum_j bias_j) [/ out_div] in one launch.
// Serves what v2w_conv1d_wino serves, of any size, with C_in == C_out, one dilation and no input affine; V2W_E_SHAPE otherwise.
extern "C" int v2w_conv1d_wino_sum_fwd(const v2w_conv1d_args* a, int n, const int32_t* len, int len_mul, void* stream) {
    return v2w_conv1d_wino_sum_fwd_order(a, n, len, len_mul, nullptr, stream);
}

// ... with the walk order given: `order` (host memory) is a permutation of 0 .. n - 1, null leaves the choice to the library.  The order
// changes only the order in which the sources' products are accumulated, never the bias or the residual sum.
extern "C" int v2w_conv1d_wino_sum_fwd_order(const v2w_conv1d_args* a, int n, const int32_t* len, int len_mul, const int32_t* order, void* stream) {
    if (!a || n < 1 || n > WSRC || (len && len_mul < 1)) return V2W_E_ARG;
    TileArgs ps[WSRC];
    for (int i = 0; i < n; ++i) {
        const v2w_conv1d_args* q = a + i;
        if (!q->in || !q->wp || !a->out) return V2W_E_ARG;
        if (q->B <= 0 || q->C_in <= 0 || q->L <= 0 || q->k <= 0 || q->dil <= 0) return V2W_E_ARG;
        if (q->res || q->res_a || q->add0 || q->add1 || q->accumulate || (q->in_a == nullptr) != (q->in_s == nullptr)) return V2W_E_ARG;
        if (q->B != a->B || q->C_in != a->C_in || q->C_out != a->C_in || q->L != a->L || q->dil != a->dil || q->slope != a->slope) return V2W_E_SHAPE;
        if (q->in_a) return V2W_E_SHAPE;        // (the second convs read lrelu(t1_j); one conv with an input affine: V2W_ALGO_WINO)
        if (!wino_served(q)) return V2W_E_SHAPE;
        ps[i] = wino_tile_args(q, len, len_mul);
        ps[i].out = a->out; ps[i].out_div = a->out_div;
    }
    return launch_wino_sum<1, 2>(ps, n, order, (hipStream_t)stream);
}

// The fan-out form (include/vec2wav_hip.h): out_j = conv_j(lrelu(in_a * in + in_s)) + bias_j [+ res_a * res + res_s], j < n, in one launch
// that stages the input once per tile.  Every out_j holds the bits of the V2W_ALGO_WINO launch of a[j] alone.
extern "C" int v2w_conv1d_wino_fan_fwd(const v2w_conv1d_args* a, int n, void* stream) {
    if (!a || n < 1 || n > WSRC) return V2W_E_ARG;
    TileArgs ps[WSRC];
    for (int i = 0; i < n; ++i) {
        const v2w_conv1d_args* q = a + i;
        if (!q->in || !q->wp || !q->out) return V2W_E_ARG;
        if (q->B <= 0 || q->C_in <= 0 || q->C_out <= 0 || q->L <= 0 || q->k <= 0 || q->dil <= 0) return V2W_E_ARG;
        if ((q->in_a == nullptr) != (q->in_s == nullptr) || (q->res_a == nullptr) != (q->res_s == nullptr)) return V2W_E_ARG;
        if (q->in != a->in || q->in_a != a->in_a || q->in_s != a->in_s || q->res != a->res || q->res_a != a->res_a || q->res_s != a->res_s)
            return V2W_E_ARG;
        if (q->B != a->B || q->C_in != a->C_in || q->C_out != a->C_out || q->L != a->L || q->dil != a->dil || q->slope != a->slope) return V2W_E_ARG;
        for (int j = 0; j < i; ++j)
            if (a[j].out == q->out) return V2W_E_ARG;
        if (!wino_served(q)) return V2W_E_SHAPE;
        if (q->add0 || q->add1 || q->accumulate || q->out_div != 0.f) return V2W_E_SHAPE;     // (the first convs have none of these)
        ps[i] = wino_tile_args(q, nullptr, 0);
    }
    return launch_wino_fan<1, 2>(ps, n, (hipStream_t)stream);
}

// The upsampler form (include/vec2wav_hip.h): out = ConvTranspose1d(lrelu(in_a * in + in_s); k = 2 u, stride u, padding u / 2) + bias on the
// two-tap Winograd segment, a->wp = the layer's fold `wpw` stream; any launch size.  V2W_E_SHAPE: not served, nothing launched.
extern "C" int v2w_convt1d_wino_fwd(const v2w_convt1d_args* a, const float* in_a, const float* in_s, void* stream) {
    if (const int rc = wino_up_shape(a)) return rc;
    if (!a->in || !a->wp || !a->out || (in_a == nullptr) != (in_s == nullptr)) return V2W_E_ARG;
    const TileArgs p = wino_up_problem(a, in_a, in_s);
    return a->u == 4 ? launch_wino_up<4>(p, (hipStream_t)stream) : launch_wino_up<2>(p, (hipStream_t)stream);
}

// Host-only shape query of the upsampler form: the number of position tiles (= rows of stats_part) of the launch v2w_convt1d_wino_fwd
// would make, and in *wgs (optional) its live workgroups - the planner's size rule reads them; V2W_E_SHAPE when the form does not serve it.
extern "C" int v2w_convt1d_wino_tiles(const v2w_convt1d_args* a, int32_t* wgs) {
    if (const int rc = wino_up_shape(a)) return rc;
    TileArgs p = wino_up_problem(a, nullptr, nullptr);
    size_t lds;
    if (const int rc = wino_up_geometry(p, &lds)) return rc;
    const long long w = (long long)p.ntiles * (p.Cout / WT::MT);
    if (w >= (1ll << 31)) return V2W_E_SHAPE;
    if (wgs) *wgs = (int32_t)w;
    return p.ntiles;
}

extern "C" int v2w_wino_sum_order(const int32_t* k, int n, int32_t* order) {
    if (!k || !order || n < 1 || n > WSRC) return V2W_E_ARG;
    int Ks[WSRC], walk[WSRC];
    for (int j = 0; j < n; ++j) Ks[j] = k[j];
    wino_sum_order(Ks, n, walk);
    for (int j = 0; j < n; ++j) order[j] = walk[j];
    return 0;
}

extern "C" int v2w_wino_terms(int k) { return wino_terms(k); }

extern "C" int v2w_pack_wino(const float* wf, float* wpw, int k, int c_in, int c_out, void* stream) {
    if (!wf || !wpw || k <= 0 || c_in <= 0 || c_out <= 0) return V2W_E_ARG;
    if (wino_terms(k) == 0 || c_in % WCK != 0 || c_out % 32 != 0) return V2W_E_SHAPE;
    const size_t total = (size_t)wino_terms(k) * c_in * c_out;
    int grid = (int)((total + 255) / 256); if (grid > 4096) grid = 4096;
    V2W_LAUNCH(pack_wino_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, wf, wpw, k, c_in, c_out);
    return v2w_launch_status();
}
