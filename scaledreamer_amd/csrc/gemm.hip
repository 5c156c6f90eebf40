// gemm.hip — fp16 MFMA GEMM / implicit-GEMM convolution for the frozen SD-2.1 UNet (gfx950).
//
//   C[M,N] = act( A[M,K] . W[N,K]^T + bias[N] + row_bias[m / rows_per_group][N] ) + residual[M,N]
//
// A is either a row-major activation matrix (Linear / 1x1 conv on NHWC tensors) or an implicit im2col view
// of an NHWC tensor for 3x3 convolutions (stride 1/2, optional fused nearest-2x upsample, zero padding):
// k = (ky, kx, cin), weights pre-packed [Cout][ky][kx][Cin].  Replaces the cuDNN/cuBLAS calls behind
// diffusers' UNet2DConditionModel in the reference (stable_diffusion_asd_guidance.py:319-331; layer
// inventory SURVEY.md Appendix A.1).
//
// CDNA4 mapping: WM x WN waves per block, each owning a (BM/WM) x (BN/WN) register tile of v_mfma_f32_16x16x32_f16
// fragments (fp32 accumulation); k-step 64.  Both operands stream HBM/L2 -> LDS with global_load_lds (16 B per lane, no
// VGPR round trip), double buffered, one barrier per k-step.  LDS rows are 128 B; the 16-B chunk index is XOR-swizzled
// with (row & 7) on the SOURCE address and on the ds_read_b128 side (bank-conflict free).  The MFMA is issued with the
// weight fragment as the A operand, so each lane ends up with 4 consecutive output channels of one row -> 8-byte stores.
// Out-of-range rows / taps read a zero page instead of branching.  The second kernel of this file, conv3x3_win_kernel,
// keeps the input window of a 16x16-pixel patch LDS-resident across the 9 taps of a stride-1 3x3 convolution.
#include <stdlib.h>

#include "asd_common.h"
#include <map>
#include <atomic>
#include <mutex>
#include <cstring>
#include <iterator>

#include "gemm_tile.h"


// KG > 1: intra-block split-K.  KG groups of WM x WN waves share the block's barriers; group g owns its own pair of LDS stages and
// the k-steps ks0 + g, ks0 + g + KG, ...; at the end the groups' accumulators are summed through LDS and group 0 runs the epilogue.
// For launches with few blocks (M <= 1280): a 64x64 block alone on its CU runs ONE wave per SIMD, so every k-step exposes its LDS
// read latency and its barrier (1280^3: ~1100 cycles per k-step for 512 cycles of MFMA); two or four waves per SIMD overlap them
// and the barrier count per K halves / quarters — without the fp32 slabs and the second launch of split-K across blocks.
// LN (asd_gemm_args.ln_mode == 1): the rows of A are the INPUT of a LayerNorm folded into this GEMM (gemm_tile.h: ln_fold): their sum and
// sum of squares are reduced from the A fragments as they pass through the main loop, so the normalised tensor never exists and the
// LayerNorm launch and its pass over the activations are gone.  The reduction runs on the MATRIX pipe, which these load-bound launches
// leave 80 % idle: mfma(ones, x) puts sum_k x[row] into every register of the lane that owns the row's outputs, mfma(x, x) the Gram
// block whose diagonal is sum_k x^2 — two MFMAs per fragment and 32-wide k slice with operands already in registers, exact fp16
// products accumulated in fp32.  (The first version used 8 v_dot2_f32_f16 per fragment and slice: the VALU issue slots it took made the
// 20480-row launches 40 % slower, more than the LayerNorm kernel had cost.)
template <int BM, int BN, int WM, int WN, bool CONV, int NST = 2, int KG = 1, bool LN = false>
__global__ __launch_bounds__(WM * WN * KG * 64) void gemm_f16_kernel(const asd_gemm_args p) {
    constexpr int NW = WM * WN;               // waves per k-group
    constexpr int TM = BM / WM / 16, TN = BN / WN / 16;
    constexpr int RB = 128;                   // LDS row bytes (64 halfs)
    constexpr int A_BYTES = BM * RB, B_BYTES = BN * RB;
    constexpr int STAGE_BYTES = A_BYTES + B_BYTES;
    constexpr int ASLABS = BM / 8, TSLABS = (BM + BN) / 8;   // 8-row slabs (1 KiB per wave instruction); A first, then W
    constexpr int SPW = (TSLABS + NW - 1) / NW;            // slabs per wave (slab id = wave + j * NW)
    static_assert(BM % (WM * 16) == 0 && BN % (WN * 16) == 0, "wave tile must be a multiple of 16 x 16");
    static_assert(NST == 2 || TSLABS % NW == 0, "ring variants count their loads per wave: every wave must own the same number of slabs");
    static_assert(KG == 1 || NST == 2, "k-groups use the two-stage loop");
    extern __shared__ __attribute__((aligned(16))) char smem[];  // [KG][NST][A | W]

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave_all = __builtin_amdgcn_readfirstlane(tid >> 6);   // scalar: slab ids, LDS destinations (M0) and operand bases stay in SGPRs
    const int kg = KG > 1 ? wave_all / NW : 0;                        // k-group of this wave
    const int wave = wave_all - kg * NW;                              // wave within its group
    char* const gsm = smem + kg * (NST * STAGE_BYTES);
    const int wm = wave / WN, wn = wave % WN;
    // (parity form of the upsampling convolution, upsample == 3: every parity's rows are tiled on their own, so a block lies in one
    // parity whatever the row count; its rows are valid below m_lim = the end of that parity's rows)
    const bool up3 = CONV && p.upsample == 3;
    const int up_mq = up3 ? p.M >> 2 : 1;
    const int tiles_pp = (up_mq + BM - 1) / BM;                  // M tiles per parity
    const int tiles_m = up3 ? 4 * tiles_pp : (p.M + BM - 1) / BM, tiles_n = (p.N + BN - 1) / BN;
    int item, tm_, tn_;
    if (!asd_xcd_item(blockIdx.x, tiles_m * tiles_n * p.split_k, item)) return;
    const int kz = item / (tiles_m * tiles_n);  // split-K slice
    asd_grouped_tile(item - kz * tiles_m * tiles_n, tiles_m, tiles_n, p.group_m, p.group_n, tm_, tn_);
    const int parity = up3 ? tm_ / tiles_pp : 0;
    const int m0 = up3 ? parity * up_mq + (tm_ - parity * tiles_pp) * BM : tm_ * BM, n0 = tn_ * BN;
    const int m_lim = up3 ? (parity + 1) * up_mq : p.M;
    const int k_steps_total = (p.K + 63) / 64;
    const int k_per = (k_steps_total + p.split_k - 1) / p.split_k;
    const int ks0 = kz * k_per, ks1 = min(k_steps_total, ks0 + k_per);

    // ---- per-lane source descriptors: lane -> (row = lane>>3 of an 8-row slab, physical chunk = lane&7) -------
    const int lrow = lane >> 3, pchunk = lane & 7;
    const char* zero = (const char*)p.zero_page;
    // fast conv addressing: when every 64-wide k-step lies inside one filter tap (Cin % 64 == 0) and the input is sampled
    // on a regular lattice (no fused upsample / transposed mode), the tap decode is wave-uniform (scalar) and a lane only
    // adds a uniform byte offset to the address of its output pixel's centre tap
    const bool fast_conv = CONV && (p.upsample == 0 || p.upsample == 3) && (p.Cin & 63) == 0;
    // upsample == 3: the 3x3 convolution over the nearest-2x upsampled image as FOUR 2x2 convolutions over the low-resolution image,
    // one per output-pixel parity (a, b) = (Y & 1, X & 1): output row Y = 2y + a reads image rows y - 1 + a .. y + a, so the nine taps
    // collapse onto 2 x 2 input pixels with pre-summed weights (packed per parity: W[4][N][4 * Cin]) — 4/9 of the multiply-adds.
    // The M axis is ordered [parity][batch][y][x] over LOW-resolution positions.
    const int par_a = parity >> 1, par_b = parity & 1;
    const char* const Wp = (const char*)p.W + ((CONV && p.upsample == 3) ? (size_t)parity * p.N * p.ldw * 2 : 0);
    // Descriptors are kept small (the accumulators need the registers): the swizzled chunk of a lane is the same in every
    // slab (row & 7 == lane >> 3), plain row-major operands are addressed as base + slab * stride, and only the conv
    // A slabs carry per-slab state (centre-tap address + packed (y, x)).
    const int lch = pchunk ^ lrow;               // logical 16-B chunk (8 halfs) that lands in this lane's LDS slot
    constexpr int ASPW = (ASLABS + NW - 1) / NW; // A slabs a wave can own (slab ids wave, wave + NW, ...)
    const char* a0 = nullptr;                    // plain A: address of (row m0 + lrow, chunk lch)
    const char* c_base[CONV ? ASPW : 1];         // conv: image base (generic path) or centre-tap address (fast path)
    int c_yx[CONV ? ASPW : 1];
    if (!CONV) {
        a0 = (const char*)p.A + (size_t)(m0 + lrow) * p.lda * 2 + lch * 16;
    } else {
#pragma unroll
        for (int j = 0; j < ASPW; ++j) {
            const int slab = wave + j * NW;
            int m = min(m0 + slab * 8 + lrow, m_lim - 1);   // clamped: validity is re-derived from the row index
            int hw = p.Hout * p.Wout, wrow = p.Wout;
            if (p.upsample == 3) { m -= parity * up_mq; hw = p.Hin * p.Win; wrow = p.Win; }   // low-resolution position
            const int b = m / hw, r = m - b * hw;
            int y = r / wrow, x = r - y * wrow;
            c_base[j] = (const char*)p.A + (size_t)b * p.Hin * p.Win * p.Cin * 2;
            if (fast_conv) {
                y *= p.stride; x *= p.stride;                    // input-lattice coordinates of the centre tap (before -pad)
                c_base[j] += ((size_t)(y * p.Win + x) * p.Cin) * 2 + lch * 16;
            }
            c_yx[j] = (y << 16) | x;
        }
    }
    constexpr bool WIDE_OK = (BN / WN) % 32 == 0;                       // wave extents that hold whole 32-channel groups
    const bool wide = WIDE_OK && p.wide_rows;                          // W tile in permuted row order (tile_epilogue)
    const int wl = wide ? wide_lane_row(lrow) : lrow;
    auto w_slab_rows = [&](int ws) { return wide ? wide_slab_rows(ws) : ws * 8; };
    const char* w0 = Wp + (size_t)(n0 + wl) * p.ldw * 2 + lch * 16;
    const size_t a_slab_stride = (size_t)8 * p.lda * 2, w_row_stride = (size_t)p.ldw * 2;
    // Row-major operands (W always, A of a plain GEMM): one 32-bit byte offset per slab against the scalar operand base
    // (global_load_lds saddr + voffset), advanced by 128 B per k-step — 3 instructions per 1-KiB wave-level load.  Rows past
    // M / N are clamped to the last row (their outputs are never stored), so every offset is always valid; only a ragged last
    // k-step (K % 64 != 0) takes the general path below, which substitutes the zero page per lane.
    unsigned roff[SPW];
#pragma unroll
    for (int j = 0; j < SPW; ++j) {
        const int slab = wave + j * NW;
        if (slab >= ASLABS) {
            const int row = min(n0 + w_slab_rows(slab - ASLABS) + wl, p.N - 1);
            roff[j] = (unsigned)row * (unsigned)(p.ldw * 2) + lch * 16 + (ks0 + kg) * 128;
            if (!CONV && p.w_seg_rows > 0) {      // segmented rows (asd_gemm_args.w_seg_*): the same rows at another offset along K
                const int seg = row / p.w_seg_rows;
                roff[j] = (unsigned)(row - seg * p.w_seg_rows) * (unsigned)(p.ldw * 2) + (unsigned)p.w_seg_off[seg] + lch * 16 + (ks0 + kg) * 128;
            }
        } else {
            const int row = min(m0 + slab * 8 + lrow, p.M - 1);
            roff[j] = CONV ? 0u : (unsigned)row * (unsigned)(p.lda * 2) + lch * 16 + (ks0 + kg) * 128;
            if (!CONV && p.a_seg_rows > 0) {
                const int seg = row / p.a_seg_rows;
                roff[j] = (unsigned)(row - seg * p.a_seg_rows) * (unsigned)(p.lda * 2) + (unsigned)p.a_seg_off[seg] + lch * 16 + (ks0 + kg) * 128;
            }
        }
    }

    auto issue_rows = [&](int stage) __attribute__((always_inline)) {
        char* st = gsm + stage * STAGE_BYTES;
#pragma unroll
        for (int j = 0; j < SPW; ++j) {
            const int slab = wave + j * NW;
            if (j * NW + NW - 1 >= TSLABS && slab >= TSLABS) continue;    // only the last j can run past the tile (wave-uniform)
            if (CONV && slab < ASLABS) continue;
            const char* base = slab >= ASLABS ? Wp : (const char*)p.A;
            load_slab(base + roff[j], st + slab * 8 * RB);
            roff[j] += 128 * KG;
        }
    };
    // general path: conv A slabs (only_conv_a) or every slab with per-lane zero-page substitution
    auto issue_general = [&](int ks, int stage, bool only_conv_a) __attribute__((always_inline)) {
        char* st = gsm + stage * STAGE_BYTES;     // slab s of the stage lives at st + s * 1 KiB (A slabs, then W slabs)
        const int k0 = ks * 64;
        const int kc = k0 + lch * 8;              // first k of this lane's chunk
        const bool k_ok = kc < p.K;
        int opaque = 0;                           // defeats loop-invariant hoisting of the per-slab addresses (register budget)
        asm volatile("" : "+v"(opaque));
        int tdy = 0, tdx = 0;
        long long toff = 0;
        if (fast_conv) {
            const int tap = k0 / p.Cin, c0 = k0 - tap * p.Cin;           // wave-uniform
            if (p.upsample == 3) { tdy = (tap >> 1) - 1 + par_a; tdx = (tap & 1) - 1 + par_b; }
            else { const int ky = tap / 3, kx = tap - ky * 3; tdy = ky - p.pad; tdx = kx - p.pad; }
            toff = ((long long)(tdy * p.Win + tdx) * p.Cin + c0) * 2;
        }
#pragma unroll
        for (int j = 0; j < SPW; ++j) {
            const int slab = wave + j * NW;
            if (slab >= TSLABS) continue;      // wave-uniform
            if (only_conv_a && slab >= ASLABS) continue;
            const char* src;
            if (slab >= ASLABS) {
                const int ws = slab - ASLABS;
                const int wr = w_slab_rows(ws);
                src = (k_ok && n0 + wr + wl < p.N) ? w0 + (wr + opaque) * w_row_stride + (size_t)k0 * 2 : zero;
            } else if (!CONV) {
                src = (k_ok && m0 + slab * 8 + lrow < p.M) ? a0 + (slab + opaque) * a_slab_stride + (size_t)k0 * 2 : zero;
            } else {
                constexpr int JA = CONV ? ASPW : 1;
                const int ja = j < JA ? j : JA - 1;      // A slabs of a wave are its first ones
                const bool row_ok = m0 + slab * 8 + lrow < m_lim;
                const int sy = c_yx[ja] >> 16, sx = c_yx[ja] & 0xffff;
                if (fast_conv) {
                    const int yi = sy + tdy, xi = sx + tdx;
                    const bool ok = row_ok && (unsigned)yi < (unsigned)p.Hin && (unsigned)xi < (unsigned)p.Win;
                    src = ok ? c_base[ja] + toff : zero;
                } else {
                    const int tap = kc / p.Cin, c0 = kc - tap * p.Cin;   // chunks never straddle a tap (Cin % 8 == 0)
                    const int ky = tap / 3, kx = tap - ky * 3;
                    int yi = sy * p.stride + ky - p.pad, xi = sx * p.stride + kx - p.pad;
                    bool ok = row_ok && k_ok;
                    if (p.upsample == 3) {  // parity form: 2 x 2 taps over the low-resolution image
                        yi = sy + (tap >> 1) - 1 + par_a; xi = sx + (tap & 1) - 1 + par_b;
                        ok = ok && yi >= 0 && xi >= 0 && yi < p.Hin && xi < p.Win;
                    } else if (p.upsample == 1) {  // conv over the nearest-2x upsampled image: bounds in the upsampled frame
                        ok = ok && yi >= 0 && xi >= 0 && yi < 2 * p.Hin && xi < 2 * p.Win;
                        yi >>= 1; xi >>= 1;
                    } else if (p.upsample == 2) {
                        // input gradient of a stride-2 convolution: dX[y,x] += dY[(y+pad-ky)/2, (x+pad-kx)/2] W[ky,kx]
                        // for the taps where both numerators are even (the other taps read the zero page)
                        yi = sy + p.pad - ky; xi = sx + p.pad - kx;
                        ok = ok && yi >= 0 && xi >= 0 && !(yi & 1) && !(xi & 1) && (yi >> 1) < p.Hin && (xi >> 1) < p.Win;
                        yi >>= 1; xi >>= 1;
                    } else {
                        ok = ok && yi >= 0 && xi >= 0 && yi < p.Hin && xi < p.Win;
                    }
                    src = ok ? c_base[ja] + ((size_t)(yi * p.Win + xi) * p.Cin + c0) * 2 : zero;
                }
            }
            load_slab(src, st + slab * 8 * RB);
        }
    };
    auto issue = [&](int ks, int stage) __attribute__((always_inline)) {
        if (ks * 64 + 64 > p.K || (CONV && !fast_conv)) {   // ragged last k-step / generic conv addressing
            issue_general(ks, stage, false);
        } else {
            issue_rows(stage);
            if (CONV) issue_general(ks, stage, true);
        }
    };

    floatx4 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = floatx4{0.f, 0.f, 0.f, 0.f};
    floatx4 sacc[LN ? TM : 1], qacc[LN ? TM : 1];      // LN: sum x (every register) and the Gram block of fragment row i
#pragma unroll
    for (int i = 0; i < (LN ? TM : 1); ++i) sacc[i] = qacc[i] = floatx4{0.f, 0.f, 0.f, 0.f};
    const half8 ln_ones = {(half_t)1.f, (half_t)1.f, (half_t)1.f, (half_t)1.f, (half_t)1.f, (half_t)1.f, (half_t)1.f, (half_t)1.f};
    float ls1[LN ? TM : 1], ls2[LN ? TM : 1];          // sum x, sum x^2 of row (lane & 15) of fragment row i, once the loop is done
    // sum x sits in every register of the lane; the Gram block's diagonal element of row b = lane & 15 sits in lane b + 16 (b >> 2),
    // register b & 3 (the MFMA result layout: lane (col, 4-row group g) holds rows 4 g .. 4 g + 3 of column col)
    auto ln_extract = [&]() __attribute__((always_inline)) {
        if constexpr (LN) {
            const int b = lane & 15;
#pragma unroll
            for (int i = 0; i < TM; ++i) {
                ls1[i] = sacc[i][0];
                const float d = (b & 2) ? ((b & 1) ? qacc[i][3] : qacc[i][2]) : ((b & 1) ? qacc[i][1] : qacc[i][0]);
                ls2[i] = __shfl(d, b + 16 * (b >> 2), 64);
            }
        }
    };

    // fragment reads: lane -> row (lane&15) of a 16-row sub-tile, k-quarter (lane>>4); chunk = kh*4 + quarter.  Sub-tiles
    // start at multiples of 16 rows, so the swizzle term (row & 7) is the same for all of them: two lane offsets (kh = 0, 1)
    // plus compile-time immediates cover every fragment of the wave
    const int frow = lane & 15, fq = lane >> 4;
    const int fa0 = (wm * (BM / WM) + frow) * RB, fb0 = A_BYTES + (wn * (BN / WN) + frow) * RB;
    const int fsw[2] = {((fq) ^ (frow & 7)) * 16, ((4 + fq) ^ (frow & 7)) * 16};

    // Input gradient of a stride-2 convolution (upsample == 2): tap (ky, kx) reaches output row Y only when Y + pad - ky is even.
    // When the whole tile lies in ONE image row (always at W >= BM), the k-steps of the other ky parity multiply zero pages for
    // every row of the tile: skip them (wave-uniform) — 6 or 3 of the 9 taps remain, 2x fewer k-steps on average.
    int live_ky_parity = -1;    // -1: every k-step is live
    if (NST == 2 && KG == 1 && CONV && p.upsample == 2 && (p.Cin & 63) == 0) {
        const int m_last = min(m0 + BM, p.M) - 1;
        if (m0 / p.Wout == m_last / p.Wout) live_ky_parity = ((m0 / p.Wout) % p.Hout + p.pad) & 1;
    }
    auto live = [&](int ks) -> bool {
        if (!CONV || live_ky_parity < 0) return true;
        const int ky = ((ks * 64) / p.Cin) / 3;
        return (ky & 1) == live_ky_parity;
    };
    auto compute = [&](const char* As) __attribute__((always_inline)) {
        // big register tiles: keep ONE set of fragments live (no cross-kh prefetch), the loop is load-bound anyway
#pragma unroll TM * TN >= 32 ? 1 : 2
        for (int kh = 0; kh < 2; ++kh) {
            half8 xa[TM], wb[TN];
            const int fs = TM * TN >= 32 ? (((kh * 4 + fq) ^ (frow & 7)) * 16) : fsw[kh];
#pragma unroll
            for (int i = 0; i < TM; ++i) xa[i] = *(const half8*)(As + fa0 + fs + i * 16 * RB);
#pragma unroll
            for (int j = 0; j < TN; ++j) wb[j] = *(const half8*)(As + fb0 + fs + j * 16 * RB);
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wb[j], xa[i], acc[i][j], 0, 0, 0);
            if constexpr (LN) {
#pragma unroll
                for (int i = 0; i < TM; ++i) {
                    sacc[i] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ln_ones, xa[i], sacc[i], 0, 0, 0);
                    qacc[i] = __builtin_amdgcn_mfma_f32_16x16x32_f16(xa[i], xa[i], qacc[i], 0, 0, 0);
                }
            }
        }
    };
    if constexpr (KG > 1) {
        int k = ks0 + kg;
        const int iters = (ks1 - ks0 + KG - 1) / KG;     // block-uniform: every group passes every barrier
        if (k < ks1) issue(k, 0);
        for (int it = 0, stage = 0; it < iters; ++it, stage ^= 1) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            const int kn = k + KG;
            if (kn < ks1) issue(kn, stage ^ 1);
            if (k < ks1) compute(gsm + stage * STAGE_BYTES);
            k = kn;
        }
        ln_extract();
        // sum the groups' accumulators into group 0: [wave][fragment][lane] floatx4, 16 B per lane (conflict-free)
        floatx4* red = (floatx4*)smem;
#pragma unroll 1
        for (int g = KG - 1; g >= 1; --g) {
            __syncthreads();     // main loop / previous round done with this LDS
            if (kg == g) {
#pragma unroll
                for (int i = 0; i < TM; ++i)
#pragma unroll
                    for (int j = 0; j < TN; ++j) red[((wave * TM + i) * TN + j) * 64 + lane] = acc[i][j];
            }
            __syncthreads();
            if (kg == 0) {
#pragma unroll
                for (int i = 0; i < TM; ++i)
#pragma unroll
                    for (int j = 0; j < TN; ++j) {
                        const floatx4 t = red[((wave * TM + i) * TN + j) * 64 + lane];
                        acc[i][j][0] += t[0]; acc[i][j][1] += t[1]; acc[i][j][2] += t[2]; acc[i][j][3] += t[3];
                    }
            }
            if constexpr (LN) {      // the groups saw disjoint k-steps of the rows: their partial sums add up the same way
                float* redf = (float*)(red + NW * TM * TN * 64);
                __syncthreads();
                if (kg == g) {
#pragma unroll
                    for (int i = 0; i < TM; ++i) { redf[((wave * TM + i) * 2) * 64 + lane] = ls1[i]; redf[((wave * TM + i) * 2 + 1) * 64 + lane] = ls2[i]; }
                }
                __syncthreads();
                if (kg == 0) {
#pragma unroll
                    for (int i = 0; i < TM; ++i) { ls1[i] += redf[((wave * TM + i) * 2) * 64 + lane]; ls2[i] += redf[((wave * TM + i) * 2 + 1) * 64 + lane]; }
                }
            }
        }
    } else if constexpr (NST > 2) {
        // Ring of NST stages for launches with FEW blocks (M <= 1280 layers, weight-streaming low-resolution convolutions): a block
        // that is alone on its CU cannot rely on co-resident blocks to cover its load latency, and with two stages each k-step
        // costs one full L2 / HBM round trip (~0.6 us: 1280^3 takes 14 us for 1.7 us of MFMA work).  NST - 1 tiles are in flight;
        // every wave owns SPW loads per tile and loads retire in order, so "tile i has landed" is vmcnt(<= tiles still allowed
        // in flight * SPW); the barrier then makes tile i visible and guarantees that everyone is done with tile i - 1, whose
        // stage the next issue overwrites.
        const int nk = ks1 - ks0;
        if (nk > 0) {
#pragma unroll
            for (int s = 0; s < NST - 1; ++s)
                if (s < nk) issue(ks0 + s, s);
            int stage = 0, fill = NST - 1;
            for (int i = 0; i < nk; ++i) {
                ring_wait<SPW, NST - 2>(nk - 1 - i);
                __builtin_amdgcn_s_barrier();
                if (i + NST - 1 < nk) issue(ks0 + i + NST - 1, fill);
                compute(gsm + stage * STAGE_BYTES);
                stage = stage + 1 == NST ? 0 : stage + 1;
                fill = fill + 1 == NST ? 0 : fill + 1;
            }
        }
    } else {
    int k = ks0;
    while (k < ks1 && !live(k)) ++k;
    if (k < ks1) {
        // Two stages.  Measured (tools/map_ab.py): 3- and 4-stage rings with vmcnt(n) waits are 5-40 % SLOWER on every shape of the
        // step with MANY blocks — the extra LDS costs the second / third co-resident block per CU, and it is the co-resident
        // blocks (independent barriers, out of phase) that fill each other's load and barrier bubbles.
        issue(k, 0);
        for (int stage = 0;; stage ^= 1) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();  // this tile visible block-wide; everyone is done reading the previous one
            int kn = k + 1;
            while (kn < ks1 && !live(kn)) ++kn;
            if (kn < ks1) issue(kn, stage ^ 1);
            compute(gsm + stage * STAGE_BYTES);
            if (kn >= ks1) break;
            k = kn;
        }
    }
    }
    if constexpr (KG == 1) ln_extract();

    // ---- epilogue ---------------------------------------------------------------------------------
    // acc[i][j][r] = C[m = m0 + wm*(BM/WM) + i*16 + (lane&15)][n = n0 + wn*(BN/WN) + j*16 + (lane>>4)*4 + r]
    const int em = lane & 15, en = (lane >> 4) * 4;
    auto out_row = [&](int i) {
        const int m = m0 + wm * (BM / WM) + i * 16 + em;
        if (m >= m_lim) return -1;
        if (CONV && p.upsample == 3) {      // [parity][b][y][x] -> output pixel (b, 2y + a, 2x + b)
            const int q = m - parity * up_mq, hwq = p.Hin * p.Win;
            const int bb = q / hwq, r = q - bb * hwq, y = r / p.Win, x = r - y * p.Win;
            return (bb * p.Hout + 2 * y + par_a) * p.Wout + 2 * x + par_b;
        }
        return m;
    };
    if (KG > 1 && kg != 0) {    // group 0 stores; the others only keep the GroupNorm reduction's block barriers company
        if (p.split_k == 1 && p.act != 2 && p.gn_partials != nullptr) {
            __syncthreads(); __syncthreads();    // gn_tile_begin
            __syncthreads();                     // gn_tile_end
        }
        return;
    }
    if (p.split_k > 1) {  // split-K: fp32 partial slabs, finished by splitk_epilogue_kernel
        tile_epilogue<TM, TN>(p, acc, n0 + wn * (BN / WN), kz, m0, out_row, false, nullptr);
        return;
    }
    float ln_mean[LN ? TM : 1], ln_rstd[LN ? TM : 1];
    if constexpr (LN) {
        const float inv_k = 1.f / (float)p.K;
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            ln_mean[i] = ls1[i] * inv_k;
            ln_rstd[i] = rsqrtf(fmaxf(ls2[i] * inv_k - ln_mean[i] * ln_mean[i], 0.f) + p.ln_eps);
            const int m = m0 + wm * (BM / WM) + i * 16 + em;
            if (p.ln_stats && n0 == 0 && wn == 0 && lane < 16 && m < p.M) { p.ln_stats[2 * m] = ln_mean[i]; p.ln_stats[2 * m + 1] = ln_rstd[i]; }
        }
    }
    if (p.act == 2) {
        // fused GEGLU (attention.py:49-56): the weight rows were interleaved in 32-row groups [16 value | 16 gate] at pack
        // time, so fragments 2j' / 2j'+1 of a lane hold value and gate of the same 4 channels; output has N/2 columns
        if constexpr (TN % 2 == 0) {
#pragma unroll
            for (int i = 0; i < TM; ++i) {
                const int m = m0 + wm * (BM / WM) + i * 16 + em;
                if (m >= p.M) continue;
#pragma unroll
                for (int j = 0; j < TN; j += 2) {
                    const int n = n0 + wn * (BN / WN) + j * 16 + en;      // value columns n..n+3, gate columns n+16..n+19
                    if (n + 16 >= p.N) continue;
                    const half4 bx = *(const half4*)((const half_t*)p.bias + n), bg = *(const half4*)((const half_t*)p.bias + n + 16);
                    float va[4] = {acc[i][j][0], acc[i][j][1], acc[i][j][2], acc[i][j][3]};
                    float vg[4] = {acc[i][j + 1][0], acc[i][j + 1][1], acc[i][j + 1][2], acc[i][j + 1][3]};
                    if (p.ln_mode) {
                        ln_fold<4>(p, va, m, n, LN ? ln_mean[i] : 0.f, LN ? ln_rstd[i] : 0.f);
                        ln_fold<4>(p, vg, m, n + 16, LN ? ln_mean[i] : 0.f, LN ? ln_rstd[i] : 0.f);
                    }
                    half4 o;
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        o[r] = (half_t)((va[r] + (float)bx[r]) * gelu_erf(vg[r] + (float)bg[r]));
                    *(half4*)((half_t*)p.C + (size_t)m * p.ldc + (n >> 5) * 16 + (n & 15)) = o;
                }
            }
        }
        return;
    }
    const bool gn = p.gn_partials != nullptr;     // block-uniform
    float* gn_lds = (float*)smem;
    if (gn) gn_tile_begin(gn_lds);
    tile_epilogue<TM, TN>(p, acc, n0 + wn * (BN / WN), kz, m0, out_row, gn, gn_lds, LN ? ln_mean : nullptr, LN ? ln_rstd : nullptr);
    if (gn) gn_tile_end(p, gn_lds, (m0 / BM) * ((p.N + BN - 1) / BN) + n0 / BN);
}

// ---------------------------------------------------------------------------------------------------------------------
// 3x3 stride-1 pad-1 convolution with an LDS-resident input WINDOW (the implicit GEMM above re-fetches every input pixel
// once per filter tap; its time is the tile-load time).  A block owns a 16 x 16 patch of output pixels x BN channels.  Per
// 64-channel chunk it brings the 18 x 18 input window (324 rows x 128 B, zero page outside the image) into LDS ONCE and
// runs the 9 taps against it by shifting the fragment row (ty + ky) * 18 + tx + kx; only the BN x 64 weight tile of each
// (tap, chunk) streams per step.  Bytes loaded per flop drop from (1/256 + 1/BN)/128 to (41.5 KB/9 + BN * 128 B) per
// 256 * BN * 128 flop — 2.3x less at BN = 128.  8 waves = 4 (M: 4 patch rows of 16 pixels each) x 2 (N).  Split-K slices
// the channel chunks.
//
// Main loop (SQ counters of the first version — one barrier per tap, compiler-scheduled just-in-time fragment reads: a third
// of the wave cycles parked at waitcnt/barrier, a third stalled behind the partner wave's MFMAs, 45 % MFMA busy):
//  * one barrier per TWO taps: weight tiles s+2, s+3 are issued at even s into a 4-slot ring, the next chunk's window 16
//    slabs at a time over three even steps;
//  * the window swizzle is keyed on the window COLUMN (wx & 7), not the row, so the fragment address of patch row i is the
//    address of row 0 plus an immediate: ~10 address VALU per step instead of ~60 between the MFMAs;
//  * fragment reads are software-pipelined by hand at half-step (32-channel) granularity through two register sets:
//    the reads of half-step h+1 fly while the 16 MFMAs of half-step h run.  hipcc only ever emits lgkmcnt(0), so the
//    ds_read_b128 / s_waitcnt pairs are inline asm (the waits carry the fragment registers as operands, which orders the
//    MFMAs behind them).
// ---------------------------------------------------------------------------------------------------------------------
#define LDS_READ16(dst, addr, OFF) asm volatile("ds_read_b128 %0, %1 offset:%2" : "=&v"(dst) : "v"(addr), "n"(OFF) : "memory")
#define LGKM_WAIT(N, F)                                                                                                  \
    asm volatile("s_waitcnt lgkmcnt(" #N ")"                                                                             \
                 : "+v"(F.a[0]), "+v"(F.a[1]), "+v"(F.a[2]), "+v"(F.a[3]), "+v"(F.w[0]), "+v"(F.w[1]), "+v"(F.w[2]), "+v"(F.w[3]))

template <int BN>
__global__ __launch_bounds__(512) void conv3x3_win_kernel(const asd_gemm_args p) {
    constexpr int WN = 2, TM = 4, TN = BN / WN / 16;
    constexpr int RB = 128;
    constexpr int WIN = 18, WIN_ROWS = WIN * WIN, WIN_SLABS = (WIN_ROWS + 7) / 8;      // 324 rows, 41 slabs
    constexpr int A_BYTES = WIN_SLABS * 8 * RB, W_BYTES = BN * RB;
    constexpr int WSLABS = BN / 8, WSPW = (WSLABS + 7) / 8;
    extern __shared__ __attribute__((aligned(16))) char smem[];                        // [A0 | A1 | W0 | W1 | W2 | W3]
    char* const a_buf = smem;
    char* const w_buf = smem + 2 * A_BYTES;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int tiles_x = p.Wout / 16, tiles_y = p.Hout / 16;
    const int tiles_m = (p.M / (p.Hout * p.Wout)) * tiles_y * tiles_x;
    const int tiles_n = (p.N + BN - 1) / BN;
    int item, tm, tn_;
    if (!asd_xcd_item(blockIdx.x, tiles_m * tiles_n * p.split_k, item)) return;
    const int kz = item / (tiles_m * tiles_n);
    asd_grouped_tile(item - kz * tiles_m * tiles_n, tiles_m, tiles_n, p.group_m, p.group_n, tm, tn_);
    const int n0 = tn_ * BN;
    const int b = tm / (tiles_y * tiles_x), tr = tm - b * tiles_y * tiles_x;
    const int y0 = (tr / tiles_x) * 16, x0 = (tr - (tr / tiles_x) * tiles_x) * 16;
    const int n_chunks = p.Cin / 64;
    const int c_per = (n_chunks + p.split_k - 1) / p.split_k;
    const int c0 = kz * c_per, c1 = min(n_chunks, c0 + c_per);
    const int steps = (c1 - c0) * 9;

    const int lrow = lane >> 3, pchunk = lane & 7;
    const char* zero = (const char*)p.zero_page;
    const char* img = (const char*)p.A + (size_t)b * p.Hin * p.Win * p.Cin * 2;
    const bool wide = p.wide_rows != 0;                                // W tile in permuted row order (tile_epilogue)
    const int wl = wide ? wide_lane_row(lrow) : lrow;
    const char* w0 = (const char*)p.W + (size_t)(n0 + wl) * p.ldw * 2 + (pchunk ^ lrow) * 16;
    const size_t w_row_stride = (size_t)p.ldw * 2;

    auto load_window_slab = [&](int slab, int chunk, char* dst_buf) {   // slab: wave-uniform, < WIN_SLABS
        const int wrow = slab * 8 + lrow;
        const int wy = (wrow * 3641) >> 16, wx = wrow - wy * WIN;        // wrow / 18 for wrow < 328
        const int yi = y0 - 1 + wy, xi = x0 - 1 + wx;
        const bool ok = wrow < WIN_ROWS && (unsigned)yi < (unsigned)p.Hin && (unsigned)xi < (unsigned)p.Win;
        const char* src = ok ? img + ((size_t)(yi * p.Win + xi) * p.Cin + chunk * 64) * 2 + (pchunk ^ (wx & 7)) * 16 : zero;
        load_slab(src, dst_buf + slab * 8 * RB);
    };
    auto load_w_tile = [&](int step, char* dst_buf) {
        const int chunk = c0 + step / 9, tap = step - (step / 9) * 9;
        const size_t koff = ((size_t)tap * p.Cin + chunk * 64) * 2;
#pragma unroll
        for (int j = 0; j < WSPW; ++j) {
            const int slab = wave + j * 8;
            if (slab >= WSLABS) continue;
            const int wr = wide ? wide_slab_rows(slab) : slab * 8;
            const char* src = (n0 + wr + wl < p.N) ? w0 + wr * w_row_stride + koff : zero;
            load_slab(src, dst_buf + slab * 8 * RB);
        }
    };

    floatx4 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = floatx4{0.f, 0.f, 0.f, 0.f};

    // fragment addressing (LDS byte offsets).  Window row of patch pixel (wm*4 + i, frow) under tap (ky, kx):
    // (wm*4 + ky + i) * 18 + frow + kx; its 16-B chunk c sits at c ^ ((frow + kx) & 7) — independent of i and ky.
    const int frow = lane & 15, fq = lane >> 4;
    const unsigned lds_a = (unsigned)(size_t)a_buf + (unsigned)((wm * 4 * WIN + frow) * RB);
    const unsigned lds_w = (unsigned)(size_t)w_buf + (unsigned)((wn * (BN / WN) + frow) * RB);
    const unsigned fsww[2] = {(unsigned)(((fq) ^ (frow & 7)) * 16), (unsigned)(((4 + fq) ^ (frow & 7)) * 16)};
    struct Frag { half8 a[4], w[4]; };          // w[2], w[3] mirror w[0], w[1] at TN == 2 (operands of the wait only)
    static_assert(TM == 4 && (TN == 4 || TN == 2), "fragment sets are written for 4 x {2, 4} sub-tiles");

    // issue the 8 (6) fragment reads of half-step (step s, channel half kh)
    auto read_frags = [&](Frag& f, int s, int kh) {
        const int cl = s / 9, tap = s - cl * 9;
        const int ky = tap / 3, kx = tap - ky * 3;
        const unsigned aa = lds_a + (unsigned)((cl & 1) * A_BYTES + (ky * WIN + kx) * RB) + (unsigned)(((kh * 4 + fq) ^ ((frow + kx) & 7)) * 16);
        const unsigned wa = lds_w + (unsigned)((s & 3) * W_BYTES) + fsww[kh];
        LDS_READ16(f.a[0], aa, 0 * WIN * RB);
        LDS_READ16(f.a[1], aa, 1 * WIN * RB);
        LDS_READ16(f.a[2], aa, 2 * WIN * RB);
        LDS_READ16(f.a[3], aa, 3 * WIN * RB);
        LDS_READ16(f.w[0], wa, 0 * 16 * RB);
        LDS_READ16(f.w[1], wa, 1 * 16 * RB);
        if constexpr (TN == 4) {
            LDS_READ16(f.w[2], wa, 2 * 16 * RB);
            LDS_READ16(f.w[3], wa, 3 * 16 * RB);
        } else {
            f.w[2] = f.w[0]; f.w[3] = f.w[1];
        }
    };
    auto mma = [&](const Frag& f) {
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j)
                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(f.w[j], f.a[i], acc[i][j], 0, 0, 0);
    };
    constexpr int NRD = TM + TN;                                        // reads per half-step

    if (steps > 0) {
        for (int slab = wave; slab < WIN_SLABS; slab += 8) load_window_slab(slab, c0, a_buf);
        load_w_tile(0, w_buf);
        if (steps > 1) load_w_tile(1, w_buf + W_BYTES);
        Frag f0, f1;
#pragma unroll 1
        for (int s = 0; s < steps; s += 2) {
            const int cl = s / 9;
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();           // tiles s, s+1 (and a completed window) visible; everyone is past step s-1
            if (s + 2 < steps) load_w_tile(s + 2, w_buf + ((s + 2) & 3) * W_BYTES);
            if (s + 3 < steps) load_w_tile(s + 3, w_buf + ((s + 3) & 3) * W_BYTES);
            // window of chunk cl+1 -> buffer (cl+1)&1, free once every wave is past chunk cl-1 (s >= 9 cl + 1); three even
            // steps issue it, the barrier two steps later publishes it before step 9 (cl+1)
            if (c0 + cl + 1 < c1 && s > 9 * cl) {
                const int base = ((s - 9 * cl - 1) >> 1) * 16;
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const int slab = base + h * 8 + wave;
                    if (slab < WIN_SLABS) load_window_slab(slab, c0 + cl + 1, a_buf + ((cl + 1) & 1) * A_BYTES);
                }
            }
            const bool two = s + 1 < steps;         // wave-uniform
            read_frags(f0, s, 0);
            read_frags(f1, s, 1);
            if constexpr (NRD == 8) LGKM_WAIT(8, f0); else LGKM_WAIT(6, f0);
            mma(f0);
            __builtin_amdgcn_sched_barrier(0);
            if (two) {
                read_frags(f0, s + 1, 0);
                if constexpr (NRD == 8) LGKM_WAIT(8, f1); else LGKM_WAIT(6, f1);
                mma(f1);
                __builtin_amdgcn_sched_barrier(0);
                read_frags(f1, s + 1, 1);
                if constexpr (NRD == 8) LGKM_WAIT(8, f0); else LGKM_WAIT(6, f0);
                mma(f0);
                __builtin_amdgcn_sched_barrier(0);
                LGKM_WAIT(0, f1);
                mma(f1);
            } else {
                LGKM_WAIT(0, f1);
                mma(f1);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
    }

    // acc[i][j][r] = C[pixel (y0 + wm*4 + i, x0 + (lane&15))][n0 + wn*BN/2 + j*16 + (lane>>4)*4 + r]
    const bool gn = p.gn_partials != nullptr && p.split_k == 1;     // block-uniform
    float* gn_lds = (float*)smem;
    if (gn) gn_tile_begin(gn_lds);
    tile_epilogue<TM, TN>(p, acc, n0 + wn * (BN / WN), kz, b * p.Hout * p.Wout,
                          [&](int i) { return (b * p.Hout + y0 + wm * 4 + i) * p.Wout + x0 + frow; }, gn, gn_lds);
    if (gn) gn_tile_end(p, gn_lds, tm * tiles_n + tn_);
}

// ---------------------------------------------------------------------------------------------------------------------
// Two-blocks-per-CU variant of the window convolution.  Co-resident blocks have independent barriers and drift out of phase, so
// one block's MFMAs run under the other's loads, waits and epilogue — worth 10-22 % wherever a launch has >= 512 blocks (VAE
// 512^2 / 256^2 layers, UNet 64^2 layers; tools/win_ab.py).  To fit twice into 160 KB of LDS and 128 registers the block keeps
// ONE window buffer (the reload at a chunk switch is exposed; the neighbour covers it), a two-slot weight ring with a barrier
// per tap, and the compiler's just-in-time fragment schedule (<= 128 VGPRs).  Column-keyed window swizzle as in conv3x3_win_kernel.
// ---------------------------------------------------------------------------------------------------------------------
// NW = 4 (tile configurations 13 / 14): four waves per block, each owning 4 patch rows x ALL BN channels.  A wave tile of 64 px x 64 ch
// needs 8 KB of fragment reads per 32-deep k slice for 256 cycles of MFMA on its SIMD; the CU's LDS delivers 128 B/clk = 8 KB per
// SIMD in those 256 cycles, i.e. the 8-wave form (64 x 64 at BN = 128, 64 x 32 at BN = 64) saturates the LDS read port before the
// matrix pipe.  Doubling the channel extent of the wave tile cuts the reads per MFMA by a quarter / a third.
template <int BN, int NW = 8>
__global__ __launch_bounds__(NW * 64, NW / 2) void conv3x3_win2_kernel(const asd_gemm_args p) {
    constexpr int WN = NW / 4, TM = 4, TN = BN / WN / 16;
    constexpr int RB = 128;
    constexpr int WIN = 18, WIN_ROWS = WIN * WIN, WIN_SLABS = (WIN_ROWS + 7) / 8;      // 324 rows, 41 slabs
    constexpr int A_BYTES = WIN_SLABS * 8 * RB, W_BYTES = BN * RB;
    constexpr int WSLABS = BN / 8, WSPW = (WSLABS + NW - 1) / NW;
    extern __shared__ __attribute__((aligned(16))) char smem[];                        // [A0 | A1 | W0 | W1]
    char* const a_buf = smem;
    char* const w_buf = smem + A_BYTES;

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WN, wn = wave - wm * WN;
    const int tiles_x = p.Wout / 16, tiles_y = p.Hout / 16;
    const int tiles_m = (p.M / (p.Hout * p.Wout)) * tiles_y * tiles_x;
    const int tiles_n = (p.N + BN - 1) / BN;
    int item, tm, tn_;
    if (!asd_xcd_item(blockIdx.x, tiles_m * tiles_n * p.split_k, item)) return;
    const int kz = item / (tiles_m * tiles_n);
    asd_grouped_tile(item - kz * tiles_m * tiles_n, tiles_m, tiles_n, p.group_m, p.group_n, tm, tn_);
    const int n0 = tn_ * BN;
    const int b = tm / (tiles_y * tiles_x), tr = tm - b * tiles_y * tiles_x;
    const int y0 = (tr / tiles_x) * 16, x0 = (tr - (tr / tiles_x) * tiles_x) * 16;
    const int n_chunks = p.Cin / 64;
    const int c_per = (n_chunks + p.split_k - 1) / p.split_k;
    const int c0 = kz * c_per, c1 = min(n_chunks, c0 + c_per);
    const int steps = (c1 - c0) * 9;

    const int lrow = lane >> 3, pchunk = lane & 7, lch = pchunk ^ lrow;
    const char* zero = (const char*)p.zero_page;
    const char* img = (const char*)p.A + (size_t)b * p.Hin * p.Win * p.Cin * 2;
    const bool wide = p.wide_rows != 0;                                // W tile in permuted row order (tile_epilogue)
    const int wl = wide ? wide_lane_row(lrow) : lrow;
    const char* w0 = (const char*)p.W + (size_t)(n0 + wl) * p.ldw * 2 + lch * 16;
    const size_t w_row_stride = (size_t)p.ldw * 2;

    auto load_window_slab = [&](int slab, int chunk, char* dst_buf) {   // slab: wave-uniform, < WIN_SLABS
        const int wrow = slab * 8 + lrow;
        const int wy = (wrow * 3641) >> 16, wx = wrow - wy * WIN;        // wrow / 18 for wrow < 328
        const int yi = y0 - 1 + wy, xi = x0 - 1 + wx;
        const bool ok = wrow < WIN_ROWS && (unsigned)yi < (unsigned)p.Hin && (unsigned)xi < (unsigned)p.Win;
        const char* src = ok ? img + ((size_t)(yi * p.Win + xi) * p.Cin + chunk * 64) * 2 + (pchunk ^ (wx & 7)) * 16 : zero;   // column-keyed swizzle
        load_slab(src, dst_buf + slab * 8 * RB);
    };
    auto load_w_tile = [&](int step, char* dst_buf) {
        const int chunk = c0 + step / 9, tap = step - (step / 9) * 9;
        const size_t koff = ((size_t)tap * p.Cin + chunk * 64) * 2;
#pragma unroll
        for (int j = 0; j < WSPW; ++j) {
            const int slab = wave + j * NW;
            if (slab >= WSLABS) continue;
            const int wr = wide ? wide_slab_rows(slab) : slab * 8;
            const char* src = (n0 + wr + wl < p.N) ? w0 + wr * w_row_stride + koff : zero;
            load_slab(src, dst_buf + slab * 8 * RB);
        }
    };

    floatx4 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = floatx4{0.f, 0.f, 0.f, 0.f};

    const int frow = lane & 15, fq = lane >> 4;
    const int fb0 = (wn * (BN / WN) + frow) * RB;
    const int fswb[2] = {((fq) ^ (frow & 7)) * 16, ((4 + fq) ^ (frow & 7)) * 16};

    if (steps > 0) {
        for (int slab = wave; slab < WIN_SLABS; slab += NW) load_window_slab(slab, c0, a_buf);
        load_w_tile(0, w_buf);
#pragma unroll 1
        for (int s = 0; s < steps; ++s) {
            const int cl = s / 9, tap = s - cl * 9;
            if (tap == 0 && s > 0) {   // chunk switch: everyone is done with the old window, reload it (exposed; the co-resident block covers)
                __builtin_amdgcn_s_barrier();
                for (int slab = wave; slab < WIN_SLABS; slab += NW) load_window_slab(slab, c0 + cl, a_buf);
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            if (s + 1 < steps) load_w_tile(s + 1, w_buf + ((s + 1) & 1) * W_BYTES);
            const char* Wt = w_buf + (s & 1) * W_BYTES;
            const int ky = tap / 3, kx = tap - ky * 3;
            // window row of patch pixel (wm*4 + i, frow) under tap (ky, kx): (wm*4 + ky + i) * 18 + frow + kx; its chunk c sits at
            // c ^ ((frow + kx) & 7) — independent of i and ky, so patch row i is an immediate offset from row 0
            const char* Ar = a_buf + ((wm * 4 + ky) * WIN + frow + kx) * RB;
            const int csw = (frow + kx) & 7;
            if constexpr (NW == 4) {
                // 256 registers per wave: both k halves' fragments are requested up front, so the LDS latency is paid once per tap
                // (under the other resident waves' MFMAs) instead of before every group of MFMAs
                half8 xa[2][TM], wb[2][TN];
#pragma unroll
                for (int kh = 0; kh < 2; ++kh) {
                    const char* Ak = Ar + (((kh * 4 + fq) ^ csw) * 16);
#pragma unroll
                    for (int i = 0; i < TM; ++i) xa[kh][i] = *(const half8*)(Ak + i * WIN * RB);
#pragma unroll
                    for (int j = 0; j < TN; ++j) wb[kh][j] = *(const half8*)(Wt + fb0 + fswb[kh] + j * 16 * RB);
                }
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int kh = 0; kh < 2; ++kh)
#pragma unroll
                    for (int i = 0; i < TM; ++i)
#pragma unroll
                        for (int j = 0; j < TN; ++j)
                            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wb[kh][j], xa[kh][i], acc[i][j], 0, 0, 0);
            } else {
#pragma unroll
            for (int kh = 0; kh < 2; ++kh) {
                half8 xa[TM], wb[TN];
                const char* Ak = Ar + (((kh * 4 + fq) ^ csw) * 16);
#pragma unroll
                for (int i = 0; i < TM; ++i) xa[i] = *(const half8*)(Ak + i * WIN * RB);
#pragma unroll
                for (int j = 0; j < TN; ++j) wb[j] = *(const half8*)(Wt + fb0 + fswb[kh] + j * 16 * RB);
#pragma unroll
                for (int i = 0; i < TM; ++i)
#pragma unroll
                    for (int j = 0; j < TN; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wb[j], xa[i], acc[i][j], 0, 0, 0);
            }
            }
        }
    }

    // acc[i][j][r] = C[pixel (y0 + wm*4 + i, x0 + (lane&15))][n0 + wn*BN/2 + j*16 + (lane>>4)*4 + r]
    const bool gn = p.gn_partials != nullptr && p.split_k == 1;     // block-uniform
    float* gn_lds = (float*)smem;
    if (gn) gn_tile_begin(gn_lds);
    tile_epilogue<TM, TN>(p, acc, n0 + wn * (BN / WN), kz, b * p.Hout * p.Wout,
                          [&](int i) { return (b * p.Hout + y0 + wm * 4 + i) * p.Wout + x0 + frow; }, gn, gn_lds);
    if (gn) gn_tile_end(p, gn_lds, tm * tiles_n + tn_);
}

// sums the split-K slabs and applies the same epilogue (4 outputs per thread)
__global__ __launch_bounds__(256) void splitk_epilogue_kernel(const asd_gemm_args p, int splits) {
    const size_t q = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t total4 = (size_t)p.M * p.N / 4;
    if (q >= total4) return;
    const int m = (int)((q * 4) / p.N), n = (int)((q * 4) % p.N);
    floatx4 v = {0.f, 0.f, 0.f, 0.f};
    for (int s = 0; s < splits; ++s) {
        const floatx4 t = *(const floatx4*)(p.workspace + ((size_t)s * p.M + m) * p.N + n);
        v[0] += t[0]; v[1] += t[1]; v[2] += t[2]; v[3] += t[3];
    }
    if (p.bias) {
        const half4 b = *(const half4*)((const half_t*)p.bias + n);
        v[0] += (float)b[0]; v[1] += (float)b[1]; v[2] += (float)b[2]; v[3] += (float)b[3];
    }
    if (p.row_bias) {
        const half4 b = *(const half4*)((const half_t*)p.row_bias + (size_t)(m / p.rows_per_group) * p.ld_row_bias + n);
        v[0] += (float)b[0]; v[1] += (float)b[1]; v[2] += (float)b[2]; v[3] += (float)b[3];
    }
    if (p.act == 1) {
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = asd_silu_fast(v[r]);
    }
    if (p.residual) {
        const half4 b = *(const half4*)((const half_t*)p.residual + (size_t)m * p.ldr + n);
        v[0] += (float)b[0]; v[1] += (float)b[1]; v[2] += (float)b[2]; v[3] += (float)b[3];
    }
    if (p.out_f32) {
        *(floatx4*)((float*)p.C + (size_t)m * p.ldc + n) = v;
    } else {
        half4 o = {(half_t)v[0], (half_t)v[1], (half_t)v[2], (half_t)v[3]};
        *(half4*)((half_t*)p.C + (size_t)m * p.ldc + n) = o;
    }
}

// Split-K epilogue that also leaves the GroupNorm statistics records of its output (asd_gemm_args.gn_partials): the low-resolution
// convolutions of the UNet (8x8, 16x16: M = 64 / 256 rows per batch element) are the split-K layers, and their consumer is a
// GroupNorm whose separate statistics launch costs as much as the reduction itself.  A block owns 64 rows x 64 channels
// (16 float4 columns x 16 row lanes x 4 passes), sums the slabs, applies the epilogue, stores fp16 and reduces sum / sum of squares of
// the stored values per group into ONE record at index (m / 64) * (N / 64) + n / 64 — (gn_rows / 64) * (N / 64) records per batch element.
__global__ __launch_bounds__(256) void splitk_epilogue_gn_kernel(const asd_gemm_args p, int splits) {
    __shared__ float lds64[64];
    const int tiles_n = p.N / 64;
    const int mb = blockIdx.x / tiles_n, nb = blockIdx.x - mb * tiles_n;
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const int n = nb * 64 + tx * 4;
    if (threadIdx.x < 64) lds64[threadIdx.x] = 0.f;
    __syncthreads();
    floatx4 cs = {0.f, 0.f, 0.f, 0.f}, cq = {0.f, 0.f, 0.f, 0.f};
    half4 bias = {0, 0, 0, 0};
    if (p.bias) bias = *(const half4*)((const half_t*)p.bias + n);
    // slabs outermost, the block's four row passes inside: four independent 16-byte loads per trip (the trip count is `splits`,
    // as in splitk_epilogue_kernel; with the rows outermost it was 4 x splits dependent round trips)
    floatx4 v[4];
    int mrow[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        v[i] = floatx4{0.f, 0.f, 0.f, 0.f};
        mrow[i] = min(mb * 64 + i * 16 + ty, p.M - 1);
    }
    for (int s = 0; s < splits; ++s) {
        floatx4 t[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) t[i] = *(const floatx4*)(p.workspace + ((size_t)s * p.M + mrow[i]) * p.N + n);
#pragma unroll
        for (int i = 0; i < 4; ++i) { v[i][0] += t[i][0]; v[i][1] += t[i][1]; v[i][2] += t[i][2]; v[i][3] += t[i][3]; }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int m = mb * 64 + i * 16 + ty;
        if (m >= p.M) continue;
        floatx4 w = v[i];
        w[0] += (float)bias[0]; w[1] += (float)bias[1]; w[2] += (float)bias[2]; w[3] += (float)bias[3];
        if (p.row_bias) {
            const half4 b = *(const half4*)((const half_t*)p.row_bias + (size_t)(m / p.rows_per_group) * p.ld_row_bias + n);
            w[0] += (float)b[0]; w[1] += (float)b[1]; w[2] += (float)b[2]; w[3] += (float)b[3];
        }
        if (p.act == 1) {
#pragma unroll
            for (int r = 0; r < 4; ++r) w[r] = asd_silu_fast(w[r]);
        }
        if (p.residual) {
            const half4 b = *(const half4*)((const half_t*)p.residual + (size_t)m * p.ldr + n);
            w[0] += (float)b[0]; w[1] += (float)b[1]; w[2] += (float)b[2]; w[3] += (float)b[3];
        }
        const half4 o = {(half_t)w[0], (half_t)w[1], (half_t)w[2], (half_t)w[3]};
        *(half4*)((half_t*)p.C + (size_t)m * p.ldc + n) = o;
#pragma unroll
        for (int r = 0; r < 4; ++r) { const float f = (float)o[r]; cs[r] += f; cq[r] = fmaf(f, f, cq[r]); }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int g = (n + r) / p.gn_cg;
        atomicAdd(&lds64[2 * g], cs[r]);
        atomicAdd(&lds64[2 * g + 1], cq[r]);
    }
    __syncthreads();
    if (threadIdx.x < 64) p.gn_partials[(size_t)blockIdx.x * 64 + threadIdx.x] = lds64[threadIdx.x];
}

// Split-K epilogue of a layer whose ONLY consumer is GroupNorm(32)(+SiLU) (asd_gemm_args.gn_apply): a block owns ALL rows of one batch
// element x ONE group, so after summing the slabs and storing C it holds every value of its group — mean / rstd come from one block
// reduction and the normalised tensor gn_apply_y = silu?(C * a + b) leaves in the same launch.  Replaces splitk_epilogue_gn_kernel +
// gn_apply_kernel (two launches, the records, and a second trip of C through HBM) on the UNet's 8x8 / 16x16 / 32x32 split-K
// convolutions (ResBlock: GroupNorm32 -> SiLU -> conv, openaimodel.py:206-222).  Statistics are taken from the STORED fp16 values
// with fp32 sums, var = max(E[x^2] - mean^2, 0): the arithmetic of gn_stats_kernel / gn_apply_kernel (nn_ops.hip).
// 1024 threads per block (the block is alone with its group: 160 blocks per launch at batch 5, so the memory parallelism has to come
// from waves per CU — with 256 threads the launch took longer than the two it replaces); NV: float4 items per thread
// (>= rows * (cg / 4) / 1024), four slabs in flight per trip.
#define GNA_THREADS 1024
template <int NV>
__global__ __launch_bounds__(GNA_THREADS) void splitk_epilogue_gnapply_kernel(const asd_gemm_args p, int splits, float inv_cnt /* 1 / (rows x cg), divided on the host */) {
    __shared__ float red[2 * (GNA_THREADS / 64)];
    const int cg = p.gn_cg, g4 = cg >> 2, rows = p.gn_rows;
    const int b = blockIdx.x >> 5, g = blockIdx.x & 31;
    const int n0 = g * cg, total = rows * g4, tid = threadIdx.x;
    floatx4 v[NV];
    int mrow[NV], ncol[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int e = min(tid + GNA_THREADS * i, total - 1);
        const int r = e / g4;
        mrow[i] = b * rows + r;
        ncol[i] = n0 + (e - r * g4) * 4;
        v[i] = floatx4{0.f, 0.f, 0.f, 0.f};
    }
    // operands of the epilogue that do not depend on the slabs: requested first
    half4 bias[NV], rbias[NV], resid[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int m = mrow[i], n = ncol[i];
        bias[i] = p.bias ? *(const half4*)((const half_t*)p.bias + n) : half4{0, 0, 0, 0};
        rbias[i] = p.row_bias ? *(const half4*)((const half_t*)p.row_bias + (size_t)(m / p.rows_per_group) * p.ld_row_bias + n) : half4{0, 0, 0, 0};
        resid[i] = p.residual ? *(const half4*)((const half_t*)p.residual + (size_t)m * p.ldr + n) : half4{0, 0, 0, 0};
    }
    // four slabs per trip: 4 NV independent 16-byte loads in flight (a 10-way split is three dependent round trips, not ten)
    for (int s = 0; s < splits; s += 4) {
        floatx4 t[4][NV];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int su = min(s + u, splits - 1);
#pragma unroll
            for (int i = 0; i < NV; ++i) t[u][i] = *(const floatx4*)(p.workspace + ((size_t)su * p.M + mrow[i]) * p.N + ncol[i]);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const float on = s + u < splits ? 1.f : 0.f;
#pragma unroll
            for (int i = 0; i < NV; ++i) {
                v[i][0] = fmaf(t[u][i][0], on, v[i][0]); v[i][1] = fmaf(t[u][i][1], on, v[i][1]);
                v[i][2] = fmaf(t[u][i][2], on, v[i][2]); v[i][3] = fmaf(t[u][i][3], on, v[i][3]);
            }
        }
    }
    float cs = 0.f, cq = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int m = mrow[i], n = ncol[i];
        floatx4 w = v[i];
#pragma unroll
        for (int r = 0; r < 4; ++r) w[r] += (float)bias[i][r];
#pragma unroll
        for (int r = 0; r < 4; ++r) w[r] += (float)rbias[i][r];
        if (p.act == 1) {
#pragma unroll
            for (int r = 0; r < 4; ++r) w[r] = asd_silu_fast(w[r]);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) w[r] += (float)resid[i][r];
        const half4 o = {(half_t)w[0], (half_t)w[1], (half_t)w[2], (half_t)w[3]};
        const bool live = tid + GNA_THREADS * i < total;
        if (live) *(half4*)((half_t*)p.C + (size_t)m * p.ldc + n) = o;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float f = (float)o[r];
            v[i][r] = f;                              // the stored value: what GroupNorm sees
            if (live) { cs += f; cq = fmaf(f, f, cq); }
        }
    }
    // block sum of (cs, cq): wave reduction by shuffles, sixteen waves through LDS
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { cs += __shfl_xor(cs, off, 64); cq += __shfl_xor(cq, off, 64); }
    if ((tid & 63) == 0) { red[(tid >> 6) * 2] = cs; red[(tid >> 6) * 2 + 1] = cq; }
    __syncthreads();
    float sum = 0.f, sq = 0.f;
#pragma unroll
    for (int w = 0; w < GNA_THREADS / 64; ++w) { sum += red[2 * w]; sq += red[2 * w + 1]; }
    if (p.gn_apply_stats && tid == 0) { p.gn_apply_stats[b * 64 + g * 2] = sum; p.gn_apply_stats[b * 64 + g * 2 + 1] = sq; }
    const float mean = sum * inv_cnt;
    const float var = fmaxf(sq * inv_cnt - mean * mean, 0.f);
    const float rstd = rsqrtf(var + p.gn_apply_eps);
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        if (tid + GNA_THREADS * i >= total) continue;
        const int m = mrow[i], n = ncol[i];
        const half4 gm = *(const half4*)((const half_t*)p.gn_apply_gamma + n), bt = *(const half4*)((const half_t*)p.gn_apply_beta + n);
        half4 o;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float sa = rstd * (float)gm[r];
            float f = fmaf(v[i][r], sa, (float)bt[r] - mean * sa);
            if (p.gn_apply_silu) f = asd_silu_fast(f);
            o[r] = (half_t)f;
        }
        *(half4*)((half_t*)p.gn_apply_y + (size_t)m * p.N + n) = o;
    }
}

// float4 items per thread of splitk_epilogue_gnapply_kernel for this (plan-resolved) launch; 0 = the fused form does not apply
static int asd_gemm_gn_apply_nv(const asd_gemm_args* a) {
    if (!a->gn_apply || a->split_k <= 1 || a->partials_only || a->out_f32 || a->act == 2 || a->gn_bwd_x) return 0;
    if (a->gn_cg < 4 || a->gn_cg % 4 || a->N != 32 * a->gn_cg || a->gn_rows < 1 || a->M % a->gn_rows || a->ldc % 4) return 0;
    if (a->conv && a->upsample == 3) return 0;      // parity-major row order
    const int need = (a->gn_rows * (a->gn_cg / 4) + GNA_THREADS - 1) / GNA_THREADS;
    // rows x group of 1024 x 20 and more (the 32x32 level) stay on the records path: 160 blocks of that size took 32 us where the records
    // epilogue + apply launch take ~20 (gpurun_out/r6m_on/step_breakdown.txt: 9 launches, 0.29 ms)
    return need <= 1 ? 1 : need <= 3 ? 3 : 0;
}

// the reduction launch behind a split-K main kernel
static void asd_launch_splitk_epilogue(const asd_gemm_args* a, hipStream_t s) {
    const int nv = a->gn_apply_y ? asd_gemm_gn_apply_nv(a) : 0;
    if (nv > 0) {
        const dim3 grid((a->M / a->gn_rows) * 32);
        const float inv_cnt = 1.f / ((float)a->gn_rows * (float)a->gn_cg);
        if (nv == 1) hipLaunchKernelGGL(splitk_epilogue_gnapply_kernel<1>, grid, dim3(GNA_THREADS), 0, s, *a, a->split_k, inv_cnt);
        else hipLaunchKernelGGL(splitk_epilogue_gnapply_kernel<3>, grid, dim3(GNA_THREADS), 0, s, *a, a->split_k, inv_cnt);
        return;
    }
    const size_t total4 = (size_t)a->M * a->N / 4;
    if (a->gn_partials) hipLaunchKernelGGL(splitk_epilogue_gn_kernel, dim3((a->M / 64) * (a->N / 64)), dim3(256), 0, s, *a, a->split_k);
    else hipLaunchKernelGGL(splitk_epilogue_kernel, dim3(asd_div_up(total4, 256)), dim3(256), 0, s, *a, a->split_k);
}


// ---- tile configurations -------------------------------------------------------------------------------------------
// ONE table: a row is the kind, the numbers and the launcher instantiated FROM those numbers (ASD_TILE), so the geometry a launch
// computes and the kernel it starts cannot differ.  Dispatch, tuner, cost model and asd_gemm_tile_info (Python, tools) read the rows;
// the 1-based tile_cfg of the plans (gemm_plans.json) is the row index + 1, so rows are appended, never moved.
struct asd_gemm_tile {
    int kind;                  // ASD_TILE_*
    int bm, bn, wm, wn;        // block tile (rows x channels) and its wm x wn waves: a block has wm * wn * kg * 64 threads in every kind
    int nst, kg;               // stages of the operand ring and k-groups of the plain kernel (2, 1 in the other kinds)
    int (*launch)(asd_gemm_args* a, hipStream_t s);     // group_m / group_n, grid, LDS size and launch of a validated problem
};

// super-tile of the block order (asd_grouped_tile): about one XCD's worth of concurrent blocks, near-square in bytes
static void asd_pick_group(int tiles_m, int tiles_n, int bm, int bn, size_t lds, int* gm, int* gn) {
    const int conc = 32 * (2 * lds <= 160 * 1024 ? 2 : 1);      // blocks an XCD (32 CUs) runs at a time
    int m = (int)lroundf(sqrtf((float)conc * (float)bn / (float)bm));
    m = m < 1 ? 1 : (m > tiles_m ? tiles_m : m);
    int n = conc / m;
    n = n < 1 ? 1 : (n > tiles_n ? tiles_n : n);
    if (n == tiles_n) { m = conc / n; m = m < 1 ? 1 : (m > tiles_m ? tiles_m : m); }
    *gm = m; *gn = n;
}

template <int BM, int BN, int WM, int WN, int NST, int KG>
static int asd_launch_plain(asd_gemm_args* a, hipStream_t s) {
    const int tiles = (a->conv && a->upsample == 3 ? 4 * asd_div_up(a->M / 4, BM) : asd_div_up(a->M, BM)) * asd_div_up(a->N, BN);
    const size_t lds = (size_t)NST * KG * (BM + BN) * 128;
    if (a->group_m < 1 || a->group_n < 1) asd_pick_group(asd_div_up(a->M, BM), asd_div_up(a->N, BN), BM, BN, lds, &a->group_m, &a->group_n);
    const dim3 grid(8 * asd_div_up(tiles * a->split_k, 8)), block(WM * WN * KG * 64);   // asd_xcd_item
    if (a->conv) asd_launch_lds<gemm_f16_kernel<BM, BN, WM, WN, true, NST, KG, false>>(grid, block, lds, s, *a);
    else if (a->ln_mode == 1) asd_launch_lds<gemm_f16_kernel<BM, BN, WM, WN, false, NST, KG, true>>(grid, block, lds, s, *a);
    else asd_launch_lds<gemm_f16_kernel<BM, BN, WM, WN, false, NST, KG, false>>(grid, block, lds, s, *a);
    return ASD_OK;
}

// LDS-window 3x3 convolution, 16x16-pixel patch x BN, NW waves.  One block per CU (conv3x3_win_kernel: double-buffered window, pipelined
// loop), or TWO (conv3x3_win2_kernel: single window buffer, two weight slots)
template <bool TWO, int BN, int NW>
static int asd_launch_window(asd_gemm_args* a, hipStream_t s) {
    const size_t lds = (size_t)(TWO ? 1 : 2) * (41 * 1024 + 2 * BN * 128);
    const int tiles_n = asd_div_up(a->N, BN);
    if (a->group_m < 1 || a->group_n < 1) asd_pick_group(a->M / 256, tiles_n, 256, BN, TWO ? (size_t)80 * 1024 : lds, &a->group_m, &a->group_n);
    const dim3 grid(8 * asd_div_up((a->M / 256) * tiles_n * a->split_k, 8)), block(NW * 64);   // asd_xcd_item
    if constexpr (TWO) asd_launch_lds<conv3x3_win2_kernel<BN, NW>>(grid, block, lds, s, *a);
    else asd_launch_lds<conv3x3_win_kernel<BN>>(grid, block, lds, s, *a);
    return ASD_OK;
}

// ping-pong window convolution of gemm_pp.hip (eight waves, two per SIMD staggered by a barrier; one block per CU):
// (4 TM x 16) pixels x (32 TN) channels.  The instantiations live there: a row without one does not load.
size_t asd_conv_pp_lds_bytes(int tm, int tn);
template <int TM, int TN> void asd_conv_pp_launch(const asd_gemm_args* a, int blocks, hipStream_t s);
template <int TM, int TN>
static int asd_launch_pp(asd_gemm_args* a, hipStream_t s) {
    const int tiles_m = a->M / (64 * TM), tiles_n = a->N / (32 * TN);
    if (a->group_m < 1 || a->group_n < 1) asd_pick_group(tiles_m, tiles_n, 64 * TM, 32 * TN, asd_conv_pp_lds_bytes(TM, TN), &a->group_m, &a->group_n);
    asd_conv_pp_launch<TM, TN>(a, 8 * asd_div_up(tiles_m * tiles_n * a->split_k, 8), s);
    return ASD_OK;
}

// weight-streaming 3x3 convolution of the 8x8 level (gemm_ws.hip): all <= 320 rows x 64 channels x one channel slice per block
int asd_conv_ws_launch(const asd_gemm_args* a, hipStream_t s);
static int asd_launch_ws(asd_gemm_args* a, hipStream_t s) {
    if (asd_conv_ws_launch(a, s) != ASD_OK) { asd_set_error("weight-streaming convolution: bad image count"); return ASD_ERR_ARG; }
    return ASD_OK;
}

// the launcher of a row, instantiated from the row's own numbers; what a kind's kernel fixes is asserted here
template <int KIND, int BM, int BN, int WM, int WN, int NST, int KG>
static int asd_tile_launch(asd_gemm_args* a, hipStream_t s) {
    if constexpr (KIND == ASD_TILE_PLAIN) return asd_launch_plain<BM, BN, WM, WN, NST, KG>(a, s);
    else {
        static_assert(NST == 2 && KG == 1, "only the plain kernel has a ring depth and k-groups to choose");
        if constexpr (KIND == ASD_TILE_WIN) { static_assert(BM == 256 && WM * WN == 8, "window: 256 pixels, eight waves"); return asd_launch_window<false, BN, 8>(a, s); }
        else if constexpr (KIND == ASD_TILE_WIN2) { static_assert(BM == 256, "window: 256 pixels"); return asd_launch_window<true, BN, WM * WN>(a, s); }
        else if constexpr (KIND == ASD_TILE_PP) { static_assert(BM % 64 == 0 && BN % 32 == 0 && WM * WN == 8, "ping-pong: eight waves"); return asd_launch_pp<BM / 64, BN / 32>(a, s); }
        else { static_assert(KIND == ASD_TILE_WS && BM == 320 && BN == 64 && WM * WN == 4, "weight streaming: 5 x 64 rows, four waves"); return asd_launch_ws(a, s); }
    }
}
#define ASD_TILE(KIND, BM, BN, WM, WN, NST, KG) {ASD_TILE_##KIND, BM, BN, WM, WN, NST, KG, &asd_tile_launch<ASD_TILE_##KIND, BM, BN, WM, WN, NST, KG>}
static constexpr asd_gemm_tile asd_gemm_tiles[] = {
    // 0-7: the tiles of the cost model (asd_gemm_pick_tile)
    ASD_TILE(PLAIN, 128, 64, 2, 2, 2, 1), ASD_TILE(PLAIN, 128, 128, 2, 2, 2, 1), ASD_TILE(PLAIN, 256, 64, 4, 2, 2, 1), ASD_TILE(PLAIN, 256, 128, 4, 2, 2, 1),
    ASD_TILE(PLAIN, 128, 320, 2, 4, 2, 1), ASD_TILE(PLAIN, 256, 256, 2, 4, 2, 1), ASD_TILE(PLAIN, 256, 320, 2, 4, 2, 1), ASD_TILE(PLAIN, 320, 128, 5, 2, 2, 1),
    // 8-11: window convolution, one block per CU (8, 9) and two (10, 11)
    ASD_TILE(WIN, 256, 64, 4, 2, 2, 1), ASD_TILE(WIN, 256, 128, 4, 2, 2, 1), ASD_TILE(WIN2, 256, 64, 4, 2, 2, 1), ASD_TILE(WIN2, 256, 128, 4, 2, 2, 1),
    ASD_TILE(PLAIN, 64, 64, 2, 2, 2, 1),    // 12: small tile, 32 KB LDS: five blocks per CU for the latency-bound K <= 1280 linears
    ASD_TILE(WIN2, 256, 64, 4, 1, 2, 1), ASD_TILE(WIN2, 256, 128, 4, 1, 2, 1),    // 13, 14: window convolution, two blocks per CU, FOUR waves with 64 px x BN wave tiles
    // 15-19: for launches with few blocks (a block alone on its CU runs one wave per SIMD and has nobody to hide its LDS / barrier /
    // load latencies): 15 = 64x64 with a 4-stage operand ring; 16-19 = intra-block split-K (k-groups sharing the block's barriers):
    // 64x64 x 2 groups, 64x64 x 4 groups, 128x64 x 2, 128x128 x 2
    ASD_TILE(PLAIN, 64, 64, 2, 2, 4, 1), ASD_TILE(PLAIN, 64, 64, 2, 2, 2, 2), ASD_TILE(PLAIN, 64, 64, 2, 2, 2, 4), ASD_TILE(PLAIN, 128, 64, 2, 2, 2, 2),
    ASD_TILE(PLAIN, 128, 128, 2, 2, 2, 2),
    // 20-24: ping-pong window convolution: 32x16 px x 128 ch, 16x16 px x 256 / 320 / 128 / 160 ch
    ASD_TILE(PP, 512, 128, 4, 2, 2, 1), ASD_TILE(PP, 256, 256, 4, 2, 2, 1), ASD_TILE(PP, 256, 320, 4, 2, 2, 1), ASD_TILE(PP, 256, 128, 4, 2, 2, 1),
    ASD_TILE(PP, 256, 160, 4, 2, 2, 1),
    ASD_TILE(WS, 320, 64, 2, 2, 2, 1),      // 25
    // 26-28: deeper operand rings for the one-block-per-CU launches of the 16x16 / 8x8 levels (K >= 1280 linears that take 13 us for 1.7 us
    // of MFMA work: with NST - 1 tiles in flight a k-step costs 1 / (NST - 1) of an L2 / HBM round trip): 128x64 x 6 stages (144 KB),
    // 64x64 x 8 (128 KB), 128x128 x 4 (128 KB)
    ASD_TILE(PLAIN, 128, 64, 2, 2, 6, 1), ASD_TILE(PLAIN, 64, 64, 2, 2, 8, 1), ASD_TILE(PLAIN, 128, 128, 2, 2, 4, 1)};
#define ASD_GEMM_NCFG ((int)(sizeof(asd_gemm_tiles) / sizeof(asd_gemm_tiles[0])))

// the rows the selection rules name (gemm_tile.h) are the rows they mean
static constexpr bool asd_cfg_is(int cfg, int kind, int bm, int bn) {
    return asd_gemm_tiles[cfg].kind == kind && asd_gemm_tiles[cfg].bm == bm && asd_gemm_tiles[cfg].bn == bn;
}
static_assert(asd_cfg_is(ASD_CFG_128x64, ASD_TILE_PLAIN, 128, 64) && asd_cfg_is(ASD_CFG_128x128, ASD_TILE_PLAIN, 128, 128) &&
              asd_cfg_is(ASD_CFG_256x64, ASD_TILE_PLAIN, 256, 64) && asd_cfg_is(ASD_CFG_256x128, ASD_TILE_PLAIN, 256, 128) &&
              asd_cfg_is(ASD_CFG_256x256, ASD_TILE_PLAIN, 256, 256) && asd_cfg_is(ASD_CFG_320x128, ASD_TILE_PLAIN, 320, 128) &&
              asd_cfg_is(ASD_CFG_WIN_64, ASD_TILE_WIN, 256, 64) && asd_cfg_is(ASD_CFG_WIN_128, ASD_TILE_WIN, 256, 128) &&
              asd_cfg_is(ASD_CFG_WIN2_64, ASD_TILE_WIN2, 256, 64) && asd_cfg_is(ASD_CFG_WIN2_128, ASD_TILE_WIN2, 256, 128),
              "a named tile configuration moved");

static bool asd_cfg_is_plain(int cfg) { return asd_gemm_tiles[cfg].kind == ASD_TILE_PLAIN; }
static bool asd_cfg_is_pp(int cfg) { return asd_gemm_tiles[cfg].kind == ASD_TILE_PP; }
static bool asd_cfg_is_ws(int cfg) { return asd_gemm_tiles[cfg].kind == ASD_TILE_WS; }
static bool asd_cfg_is_window(int cfg) { return !asd_cfg_is_plain(cfg) && !asd_cfg_is_ws(cfg); }      // WIN, WIN2, PP
static int asd_cfg_wave_n(int cfg) { return asd_gemm_tiles[cfg].bn / asd_gemm_tiles[cfg].wn; }         // columns per wave
// (split_k resolved) 3x3 stride-1 pad-1 convolution on <= 5 images of 8 x 8 pixels, whole 32-channel chunks per slice, fp32 slabs
static bool asd_conv_ws_ok(const asd_gemm_args* a) {
    return a->conv && a->stride == 1 && a->pad == 1 && a->upsample == 0 && a->Hin == 8 && a->Win == 8 && a->Hout == 8 && a->Wout == 8 &&
           a->M % 64 == 0 && a->M / 64 <= 5 && a->N % 64 == 0 && a->split_k >= 2 && a->Cin % (32 * a->split_k) == 0 && !a->gn_bwd_x && !a->ln_mode;
}

static bool asd_conv_window_ok(const asd_gemm_args* a) {
    return a->conv && a->stride == 1 && a->pad == 1 && a->upsample == 0 && a->Cin % 64 == 0 && a->Hin == a->Hout &&
           a->Win == a->Wout && a->Hout % 16 == 0 && a->Wout % 16 == 0;
}

// ping-pong window kernel: whole patches (rows of the image divisible by the patch rows), whole N tiles
static bool asd_conv_pp_ok(const asd_gemm_args* a, int cfg) {   // 32-channel chunks: Cin = 32 (the padded RGB input of the VAE) qualifies too
    return a->conv && a->stride == 1 && a->pad == 1 && a->upsample == 0 && a->Cin % 32 == 0 && a->Hin == a->Hout && a->Win == a->Wout &&
           a->Hout % 16 == 0 && a->Wout % 16 == 0 && a->Hout % (asd_gemm_tiles[cfg].bm / 16) == 0 && a->N % asd_gemm_tiles[cfg].bn == 0;
}
static int g_force_tile = -1;   // tuning hook (asd_gemm_force_tile, tools/gemm_sweep.py); -1 = cost model

// Load-bound cost model (see the kernel comment): a block spends ~ k_steps * (BM + BN) on its tile loads, the chip runs
// 256 blocks at a time at full aggregate rate (fewer blocks run up to ~1.5x faster each), padding is wasted work, and
// every block pays a fixed prologue/epilogue.  Returns the cheapest configuration for the given split.
static int asd_gemm_pick_tile(int M, int N, int K, int split) {
    const int ksteps = asd_div_up(asd_div_up(K, 64), split);
    double best = 1e300;
    int best_cfg = 1;
    for (int c = 0; c < ASD_GEMM_NCFG && asd_cfg_is_plain(c); ++c) {      // the plain rows in front of the first window row
        const int bm = asd_gemm_tiles[c].bm, bn = asd_gemm_tiles[c].bn;
        if (bn > 64 && N % bn != 0 && !(bn == 128 && N % 128 == 0)) continue;   // wide tiles only without N padding
        if (bn == 64 && N % 128 == 0) continue;
        const long long blocks = (long long)asd_div_up(M, bm) * asd_div_up(N, bn) * split;
        const double per_block = (double)ksteps * (bm + bn) + 6.0 * 64 + 0.02 * bm * bn;   // loads + prologue + epilogue stores
        const double rounds = blocks >= 256 ? (double)blocks / 256.0 : 0.62 + 0.38 * (double)blocks / 256.0;
        const double cost = per_block * rounds;
        if (cost < best) { best = cost; best_cfg = c; }
    }
    return best_cfg;
}

// ---- tuned plans: (tile configuration, split-K) per problem shape ---------------------------------------------------------
// The kernel is bound by tile loads, so the best tile / split depends on the shape in ways the closed-form model above only
// roughly captures.  Like a BLAS library's tuned-kernel table: asd_gemm_tune() times every valid candidate once and records
// the winner; asd_gemm_f16 with split_k == 0 ("auto") looks the shape up (falling back to the cost model).  The table for the
// shapes of the shipped configs is committed (scaledreamer_amd/diffusion/gemm_plans.json) and pushed with asd_gemm_plan_set.
struct asd_plan_key {
    int32_t M, N, K, conv, a, b, c, d, e;
    bool operator<(const asd_plan_key& o) const { return memcmp(this, &o, sizeof(*this)) < 0; }
};
struct asd_plan_val { int32_t tile, split; };
static std::map<asd_plan_key, asd_plan_val> g_plans;
static std::mutex g_plans_mu;
static std::atomic<uint64_t> g_plan_gen{1};     // bumped by everything that can change what a launch resolves to (asd_gemm_plan_generation)

static asd_plan_key asd_plan_key_of(const asd_gemm_args* a) {
    asd_plan_key k;
    memset(&k, 0, sizeof(k));
    k.M = a->M; k.N = a->N; k.K = a->K; k.conv = a->conv ? 1 : 0;
    if (a->conv) { k.a = a->Hin; k.b = a->Cin; k.c = a->stride; k.d = a->upsample; k.e = a->pad; }
    else k.a = a->act == 2 ? -a->lda : a->lda;
    return k;
}
static bool asd_plan_lookup(const asd_gemm_args* a, asd_plan_val* out) {
    std::lock_guard<std::mutex> lk(g_plans_mu);
    auto it = g_plans.find(asd_plan_key_of(a));
    if (it == g_plans.end()) return false;
    *out = it->second;
    return true;
}
// default split when no plan exists: fill the 256 CUs when the output has few 128x128 tiles and the reduction is long
static int asd_default_split(const asd_gemm_args* a) {
    if (a->act == 2) return 1;
    const int bn = a->N % 128 == 0 ? 128 : 64;
    const int tiles = asd_div_up(a->M, 128) * asd_div_up(a->N, bn);
    if (tiles >= 256 || a->K < 1024) return 1;
    const int target = tiles <= 128 ? 512 : 640;
    int s = target / tiles;
    if (s > 16) s = 16;
    if (s > a->K / 512) s = a->K / 512;
    return s < 1 ? 1 : s;
}

// reads n16 16-byte words (brings an operand back into the caches after a flush); the xor keeps the loads alive
__global__ void asd_touch_kernel(const uint4* __restrict__ p, size_t n16, unsigned* __restrict__ sink) {
    unsigned acc = 0;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n16; i += (size_t)gridDim.x * blockDim.x) {
        const uint4 v = p[i];
        acc ^= v.x ^ v.y ^ v.z ^ v.w;
    }
    if (acc == 0x9e3779b9u) sink[0] = acc;
}

__global__ void asd_spin_kernel(long long cycles) {
    const long long t0 = wall_clock64();
    while (wall_clock64() - t0 < cycles) {}
}

// tile configuration of a (validated, plan-resolved: split_k >= 1) problem: the tuned one, else the cost model
static int asd_gemm_resolve_cfg(const asd_gemm_args* a) {
    int cfg = asd_gemm_pick_tile(a->M, a->N, a->K, a->split_k);
    // without a tuned plan: the LDS-window kernel wins on every stride-1 3x3 layer with at least 16 patches (tools/gemm_sweep.py)
    if (asd_conv_window_ok(a) && a->M >= 4096 && a->split_k <= a->Cin / 64) {
        const bool wide = a->N % 128 == 0;
        cfg = wide ? ASD_CFG_WIN_128 : ASD_CFG_WIN_64;
        if ((a->M / 256) * asd_div_up(a->N, asd_gemm_tiles[cfg].bn) * a->split_k >= 512) cfg = wide ? ASD_CFG_WIN2_128 : ASD_CFG_WIN2_64;   // enough blocks for two per CU
    }
    if (a->act == 2 && asd_cfg_wave_n(cfg) % 32 != 0)      // GEGLU: per-wave width % 32 (the 320-wide tiles have 80)
        cfg = a->N % 256 == 0 ? ASD_CFG_256x256 : (a->N % 128 == 0 ? ASD_CFG_256x128 : ASD_CFG_256x64);
    if (a->tile_cfg >= 1 && a->tile_cfg <= ASD_GEMM_NCFG) cfg = a->tile_cfg - 1;
    if (g_force_tile >= 0 && g_force_tile < ASD_GEMM_NCFG) cfg = g_force_tile;
    if (a->conv && a->upsample == 3 && asd_cfg_is_window(cfg)) cfg = a->N % 128 == 0 ? ASD_CFG_128x128 : ASD_CFG_128x64;
    return cfg;
}

#define ASD_SPLITK_GN_MAX_RECORDS 96     // = GN_FOLD_RECORDS of nn_ops.hip: the apply kernel sums them in its prologue, no reduce launch
// GroupNorm statistics in the epilogue: records per batch element, 0 when this launch cannot produce them
static int asd_gemm_gn_records_cfg(const asd_gemm_args* a, int cfg, bool need_ptr) {
    if (a->gn_bwd_x && !(a->gn_bwd_fstats && a->gn_bwd_gamma && a->gn_bwd_beta && a->ldc == a->N)) return 0;
    if ((need_ptr && !a->gn_partials) || a->split_k < 1 || a->out_f32 || a->act == 2 || a->gn_cg < 1 || a->gn_rows < 1 || a->N != 32 * a->gn_cg || a->M % a->gn_rows) return 0;
    if (a->conv && a->upsample == 3) return 0;      // parity-major row order: the tiles of a batch element are not contiguous
    if (a->split_k > 1) {     // statistics in the split-K epilogue (splitk_epilogue_gn_kernel): 64 x 64 blocks, few enough records to fold
        if (a->gn_bwd_x || a->N % 64 || a->gn_rows % 64 || a->ldc % 4) return 0;
        const int nrec = (a->gn_rows / 64) * (a->N / 64);
        return nrec <= ASD_SPLITK_GN_MAX_RECORDS ? nrec : 0;
    }
    const int bm = asd_gemm_tiles[cfg].bm, tiles_n = asd_div_up(a->N, asd_gemm_tiles[cfg].bn);
    return a->gn_rows % bm == 0 ? (a->gn_rows / bm) * tiles_n : 0;      // whole row tiles per image (window patches never leave theirs)
}

// split_k == 0 ("auto"): the tuned plan of this shape, else cost model + default split; a tile the caller named stays
static void asd_gemm_resolve_plan(asd_gemm_args* a) {
    if (a->split_k != 0) return;
    int32_t t = 0, sk = 1;
    asd_gemm_plan_get(a, &t, &sk);
    a->split_k = sk;
    if (!a->tile_cfg) a->tile_cfg = t;
}

extern "C" {

int asd_gemm_force_tile(int32_t cfg) {
    g_force_tile = cfg;
    ++g_plan_gen;
    return ASD_OK;
}

int asd_gemm_plan_set(int32_t M, int32_t N, int32_t K, int32_t conv, int32_t s0, int32_t s1, int32_t s2, int32_t s3, int32_t s4,
                      int32_t tile_cfg, int32_t split_k) {
    ASD_CHECK_ARG(tile_cfg >= 0 && tile_cfg <= ASD_GEMM_NCFG && split_k >= 1, "bad plan");
    asd_plan_key k;
    memset(&k, 0, sizeof(k));
    k.M = M; k.N = N; k.K = K; k.conv = conv ? 1 : 0; k.a = s0; k.b = s1; k.c = s2; k.d = s3; k.e = s4;
    std::lock_guard<std::mutex> lk(g_plans_mu);
    g_plans[k] = asd_plan_val{tile_cfg, split_k};
    ++g_plan_gen;
    return ASD_OK;
}

int asd_gemm_plan_get(const asd_gemm_args* a, int32_t* tile_cfg, int32_t* split_k) {
    ASD_CHECK_ARG(a && tile_cfg && split_k, "null argument");
    asd_plan_val v;
    if (asd_plan_lookup(a, &v)) { *tile_cfg = v.tile; *split_k = v.split; return ASD_OK; }
    *tile_cfg = 0;
    *split_k = asd_default_split(a);
    return 1;   // not tuned: cost model + default split
}

int32_t asd_gemm_gn_records(const asd_gemm_args* a_in) {
    if (!a_in || a_in->M <= 0 || a_in->N <= 0 || a_in->K <= 0) return 0;
    asd_gemm_args a = *a_in;
    asd_gemm_resolve_plan(&a);
    return asd_gemm_gn_records_cfg(&a, asd_gemm_resolve_cfg(&a), false);
}

int32_t asd_gemm_gn_applies(const asd_gemm_args* a_in) {
    if (!a_in || a_in->M <= 0 || a_in->N <= 0 || a_in->K <= 0) return 0;
    asd_gemm_args a = *a_in;
    asd_gemm_resolve_plan(&a);
    return asd_gemm_gn_apply_nv(&a) > 0 ? 1 : 0;
}

int asd_gemm_plan_count(void) {
    std::lock_guard<std::mutex> lk(g_plans_mu);
    return (int)g_plans.size();
}

int64_t asd_gemm_workspace_bytes(const asd_gemm_args* a_in) {
    if (!a_in) return 0;
    asd_gemm_args a = *a_in;
    if (a.split_k < 0) a.split_k = 0;       // this entry has always read a negative split as "auto"
    asd_gemm_resolve_plan(&a);
    // an upper bound under ln_mode, whose launch drops to split 1 whatever the plan says
    return a.split_k > 1 ? (int64_t)a.split_k * a.M * a.N * 4 : 0;
}

int asd_gemm_f16(const asd_gemm_args* a_in, void* stream) {
    ASD_CHECK_ARG(a_in, "null argument");
    asd_gemm_args a_copy = *a_in;           // group_m / group_n / ld_row_bias are filled in here when the caller left them 0
    asd_gemm_args* a = &a_copy;
    if (a->ld_row_bias <= 0) a->ld_row_bias = a->N;
    asd_gemm_resolve_plan(a);
    ASD_CHECK_ARG(a && a->A && a->W && a->C && a->zero_page, "null argument");
    ASD_CHECK_ARG(a->M > 0 && a->N > 0 && a->K > 0, "empty problem");
    ASD_CHECK_ARG(a->K % 8 == 0, "K must be a multiple of 8");
    ASD_CHECK_ARG(a->N % 4 == 0 && a->ldc % 4 == 0, "N and ldc must be multiples of 4");
    ASD_CHECK_ARG(a->ldw % 8 == 0 && (a->conv || a->lda % 8 == 0), "leading dimensions must be multiples of 8 halfs (16 B)");
    if (a->conv) {
        ASD_CHECK_ARG(a->Cin % 8 == 0 && a->K == (a->upsample == 3 ? 4 : 9) * a->Cin, "conv: Cin must be a multiple of 8 and K = 9*Cin (4*Cin in the parity form)");
        ASD_CHECK_ARG(a->upsample != 3 || (a->stride == 1 && a->Hout == 2 * a->Hin && a->Wout == 2 * a->Win && !a->gn_bwd_x),
                      "parity-form upsample conv: stride 1, Hout = 2*Hin, Wout = 2*Win");
        ASD_CHECK_ARG(a->Hout > 0 && a->Wout > 0 && a->M % (a->Hout * a->Wout) == 0, "conv: M must be B*Hout*Wout");
    }
    ASD_CHECK_ARG(a->split_k >= 1 && (a->split_k == 1 || a->workspace), "split-K needs a workspace");
    if (a->a_seg_rows > 0 || a->w_seg_rows > 0 || a->partials_only)
        ASD_CHECK_ARG(!a->conv && a->K % 64 == 0 && a->a_seg_rows >= 0 && a->w_seg_rows >= 0 && (!a->partials_only || a->split_k > 1) &&
                      (a->a_seg_rows == 0 || (a->M + a->a_seg_rows - 1) / a->a_seg_rows <= 9) && (a->w_seg_rows == 0 || (a->N + a->w_seg_rows - 1) / a->w_seg_rows <= 6),
                      "segmented rows / partials_only: plain GEMM, K % 64 == 0, at most 9 (A) and 6 (W) segments, split_k > 1 for partials_only");
    ASD_CHECK_ARG((size_t)a->N * a->ldw * 2 < ((size_t)1 << 32) && (a->conv || (size_t)a->M * a->lda * 2 < ((size_t)1 << 32)),
                  "row-major operands are addressed with 32-bit byte offsets (< 4 GiB each)");
    if (a->act == 2)
        ASD_CHECK_ARG(a->N % 32 == 0 && a->bias && !a->conv && !a->residual && !a->row_bias && !a->out_f32 && a->split_k == 1,
                      "GEGLU epilogue: N % 32 == 0, bias required, no conv / residual / row_bias / fp32 output / split-K");
    if (a->ln_mode) {
        ASD_CHECK_ARG((a->ln_mode == 1 || a->ln_mode == 2) && a->ln_sc && !a->out_f32, "LayerNorm fold: ln_mode 1 | 2, ln_sc required, fp16 output");
        ASD_CHECK_ARG(a->ln_mode == 1 || (a->ln_stats && a->N % 4 == 0), "LayerNorm fold, mode 2: the column statistics ln_stats[N][2] are required");
        ASD_CHECK_ARG(a->ln_mode == 2 || !a->conv, "LayerNorm fold, mode 1: plain GEMM only (the rows of A are the LayerNorm's rows)");
        if (a->split_k > 1) { a->split_k = 1; a->tile_cfg = 0; }      // the row statistics (mode 1) and the fold itself need the whole K in one block
    }
    int cfg = asd_gemm_resolve_cfg(a);
    ASD_CHECK_ARG(a->act != 2 || (!asd_cfg_is_window(cfg) && asd_cfg_wave_n(cfg) % 32 == 0),
                  "GEGLU epilogue needs a tile whose per-wave width is a multiple of 32 columns");
    ASD_CHECK_ARG(asd_gemm_tiles[cfg].bn == 64 || a->N % asd_gemm_tiles[cfg].bn == 0 || (asd_gemm_tiles[cfg].bn == 128 && a->N % 4 == 0),
                  "tile configuration does not divide N");
    if (asd_gemm_gn_records_cfg(a, cfg, true) == 0) a->gn_partials = nullptr;
    {   // wide-row epilogue (tile_epilogue): whole 32-channel groups per wave, 16-byte aligned rows everywhere
        auto al16 = [](const void* q) { return ((uintptr_t)q & 15) == 0; };
        const int wave_n = asd_cfg_wave_n(cfg);
        a->wide_rows = wave_n % 32 == 0 && a->act != 2 && a->N % 8 == 0 && a->ldc % 8 == 0 && al16(a->C) && (!a->bias || al16(a->bias)) &&
                       (!a->row_bias || (al16(a->row_bias) && a->ld_row_bias % 8 == 0)) && (!a->residual || (al16(a->residual) && a->ldr % 8 == 0)) &&
                       !(a->gn_partials && a->gn_bwd_x);
    }
    static const bool trace = getenv("ASD_GEMM_TRACE") != nullptr;      // tools/gemm_shapes.py: one line per launch
    if (trace)
        fprintf(stderr, "ASD_GEMM %d %d %d conv=%d %d %d %d %d %d s=%d p=%d u=%d cfg=%d split=%d act=%d res=%d f32=%d gn=%d\n", a->M, a->N, a->K, a->conv, a->Hin,
                a->Win, a->Cin, a->Hout, a->Wout, a->stride, a->pad, a->upsample, cfg, a->split_k, a->act, a->residual != nullptr, a->out_f32,
                a->gn_partials ? (a->gn_bwd_x ? 2 : 1) : 0);
    if (asd_cfg_is_ws(cfg))
        ASD_CHECK_ARG(asd_conv_ws_ok(a), "weight-streaming convolution: 3x3 stride-1 pad-1 on <= 5 images of 8x8, N % 64 == 0, split_k >= 2, Cin % (32 split_k) == 0");
    if (asd_cfg_is_window(cfg)) {
        ASD_CHECK_ARG(asd_cfg_is_pp(cfg) ? asd_conv_pp_ok(a, cfg) : asd_conv_window_ok(a),
                      "window convolution needs a 3x3 stride-1 pad-1 conv with Cin % 64 == 0 (ping-pong: % 32) and H, W % 16 == 0");
        ASD_CHECK_ARG(a->split_k == 1 || a->split_k <= a->Cin / 64, "window convolution: split_k exceeds the channel chunks");
    }
    hipStream_t s = (hipStream_t)stream;
    const int rc = asd_gemm_tiles[cfg].launch(a, s);
    if (rc != ASD_OK) return rc;
    if (a->split_k > 1 && !a->partials_only) asd_launch_splitk_epilogue(a, s);      // (the convolution kinds never see partials_only: plain GEMM only)
    ASD_LAUNCH_CHECK();
    return ASD_OK;
}


// candidates of one shape: the rules of the first autotuner (hip_ops._candidates, round 1) restated
static int asd_tune_candidates(const asd_gemm_args* a, int (*out)[2], int max_out) {
    static const int sk_plain[] = {1, 2, 3, 4, 6, 8, 12, 16}, sk_win[] = {1, 2, 3, 4, 5, 6, 8, 10};
    const bool geglu = a->act == 2, window_ok = asd_conv_window_ok(a);
    int n = 0;
    for (int t = 0; t < ASD_GEMM_NCFG && n < max_out; ++t) {
        const int bm = asd_gemm_tiles[t].bm, bn = asd_gemm_tiles[t].bn;
        if (asd_cfg_is_ws(t)) {
            static const int sk_ws[] = {2, 4, 5, 8, 10, 16, 20};
            for (int sk : sk_ws) {
                asd_gemm_args q = *a;
                q.split_k = sk;
                if (!asd_conv_ws_ok(&q) || (a->N / 64) * sk > 512 || (a->N / 64) * sk < 64) continue;
                if (n < max_out) { out[n][0] = t + 1; out[n][1] = sk; ++n; }
            }
            continue;
        }
        if (asd_cfg_is_window(t)) {
            if (asd_cfg_is_pp(t) ? !asd_conv_pp_ok(a, t) : (!window_ok || (bn != 64 && a->N % bn != 0))) continue;
            const int tiles = (a->M / bm) * asd_div_up(a->N, bn);
            for (int sk : sk_win) {
                if (sk > 1 && (a->Cin / 64 < 2 * sk || tiles * sk > 1536)) continue;
                if (n < max_out) { out[n][0] = t + 1; out[n][1] = sk; ++n; }
            }
            continue;
        }
        if (bn != 64 && a->N % bn != 0) continue;
        const bool few = asd_gemm_tiles[t].nst > 2 || asd_gemm_tiles[t].kg > 1;      // the few-block variants: only where they can win
        if (few && ((a->conv && a->upsample == 2) || (long long)asd_div_up(a->M, bm) * asd_div_up(a->N, bn) > 512 || a->K < 512)) continue;
        if (geglu && asd_cfg_wave_n(t) % 32 != 0) continue;
        if (bn == 64 && a->N % 128 == 0 && a->N >= 256 && bm == 128) continue;
        const int tiles = asd_div_up(a->M, bm) * asd_div_up(a->N, bn);
        for (int sk : sk_plain) {
            if (sk > 1 && (geglu || a->K / sk < 256 || tiles * sk > 1536)) continue;
            if (few && sk != 1 && sk != 2 && sk != 4) continue;     // (tuning time: every candidate is launched six times)
            if (n < max_out) { out[n][0] = t + 1; out[n][1] = sk; ++n; }
        }
    }
    return n;
}

/* Time every valid (tile, split-K) candidate of this problem on `stream` (which must not be capturing) and record the winner
 * in the plan table: among the candidates within 4 % of the fastest the smallest split wins (split-K multiplies the HBM
 * traffic of the output by 2 * split in fp32 partial slabs), then the fastest.  The launches are queued behind a spin kernel
 * so that the events bracket GPU time only (an eager launch costs the host ~8 us, more than some candidates run).
 * `scratch` holds the split-K slabs; candidates that need more than scratch_bytes are skipped. */
int asd_gemm_tune(const asd_gemm_args* a_in, void* scratch, int64_t scratch_bytes, void* stream) {
    ASD_CHECK_ARG(a_in, "null argument");
    hipStream_t s = (hipStream_t)stream;
    int cand[160][2];
    const int n = asd_tune_candidates(a_in, cand, 160);
    ASD_CHECK_ARG(n > 0, "no tile configuration fits this problem");
    hipEvent_t e0, e1;
    if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) { asd_set_error("hipEventCreate failed"); return ASD_ERR_LAUNCH; }
    float best_ms = 1e30f;
    float ms_of[160];
    // ASD_GEMM_TUNE_COLD=1 (tools/gemm_tune.py): time every candidate with HBM-cold weights and cache-warm activations
    static char* cold_flush = nullptr;
    static const size_t cold_bytes = (size_t)320 << 20;
    static const bool want_cold = getenv("ASD_GEMM_TUNE_COLD") && getenv("ASD_GEMM_TUNE_COLD")[0] == '1';
    if (want_cold && !cold_flush && hipMalloc((void**)&cold_flush, cold_bytes) != hipSuccess) cold_flush = nullptr;
    const size_t a_bytes = a_in->conv ? (size_t)(a_in->M / (a_in->Hout * a_in->Wout)) * a_in->Hin * a_in->Win * a_in->Cin * 2
                                      : (size_t)a_in->M * a_in->lda * 2;
    for (int i = 0; i < n; ++i) {
        ms_of[i] = 1e30f;
        asd_gemm_args a = *a_in;
        a.gn_partials = nullptr;          // the record count depends on the tile: the caller's buffer is sized for the final plan only
        a.tile_cfg = cand[i][0];
        a.split_k = cand[i][1];
        if (a.split_k > 1) {
            if ((int64_t)a.split_k * a.M * a.N * 4 > scratch_bytes) continue;
            a.workspace = (float*)scratch;
        }
        if (asd_gemm_f16(&a, stream) != ASD_OK) continue;       // warm-up (also validates the candidate)
        float ms = 0.f;
        if (cold_flush) {
            // the step's conditions: the weights come from HBM (1.7 GB of them stream through a 256 MB Infinity Cache every
            // step), the activations were written by the previous launch.  Evict everything, read A back in, then time ONE launch.
            for (int r = 0; r < 4; ++r) {
                (void)hipMemsetAsync(cold_flush, r, cold_bytes, s);
                hipLaunchKernelGGL(asd_touch_kernel, dim3(1024), dim3(256), 0, s, (const uint4*)a.A, a_bytes / 16, (unsigned*)cold_flush);
                hipLaunchKernelGGL(asd_spin_kernel, dim3(1), dim3(1), 0, s, 2000LL);
                hipEventRecord(e0, s);
                asd_gemm_f16(&a, stream);
                hipEventRecord(e1, s);
                hipEventSynchronize(e1);
                float t = 0.f;
                hipEventElapsedTime(&t, e0, e1);
                ms += t;
            }
        } else {
            hipLaunchKernelGGL(asd_spin_kernel, dim3(1), dim3(1), 0, s, 20000LL);   // ~200 us at the 100 MHz wall clock
            hipEventRecord(e0, s);
            for (int r = 0; r < 5; ++r) asd_gemm_f16(&a, stream);
            hipEventRecord(e1, s);
            hipEventSynchronize(e1);
            hipEventElapsedTime(&ms, e0, e1);
        }
        ms_of[i] = ms;
        if (ms < best_ms) best_ms = ms;
    }
    hipEventDestroy(e0);
    hipEventDestroy(e1);
    int pick = -1;
    for (int i = 0; i < n; ++i) {
        if (ms_of[i] > 1.04f * best_ms) continue;
        if (pick < 0 || cand[i][1] < cand[pick][1] || (cand[i][1] == cand[pick][1] && ms_of[i] < ms_of[pick])) pick = i;
    }
    if (pick < 0) { asd_set_error("asd_gemm_tune: no candidate ran"); return ASD_ERR_LAUNCH; }
    const asd_plan_key k = asd_plan_key_of(a_in);
    std::lock_guard<std::mutex> lk(g_plans_mu);
    g_plans[k] = asd_plan_val{cand[pick][0], cand[pick][1]};
    ++g_plan_gen;
    return ASD_OK;
}

uint64_t asd_gemm_plan_generation(void) { return g_plan_gen.load(); }

/* enumerate the plan table (persisting what asd_gemm_tune found): entry i -> 11 ints {M,N,K,conv,s0..s4,tile,split} */
int asd_gemm_plan_entry(int32_t i, int32_t* out11) {
    std::lock_guard<std::mutex> lk(g_plans_mu);
    if (i < 0 || i >= (int)g_plans.size() || !out11) return ASD_ERR_ARG;
    auto it = g_plans.begin();
    std::advance(it, i);
    const asd_plan_key& k = it->first;
    const int32_t v[11] = {k.M, k.N, k.K, k.conv, k.a, k.b, k.c, k.d, k.e, it->second.tile, it->second.split};
    memcpy(out11, v, sizeof(v));
    return ASD_OK;
}

/* row i of the tile table -> 7 ints {kind (ASD_TILE_*), bm, bn, wm, wn, stages, k-groups}; an error status past the end */
int asd_gemm_tile_info(int32_t i, int32_t* out7) {
    if (i < 0 || i >= ASD_GEMM_NCFG || !out7) return ASD_ERR_ARG;
    const asd_gemm_tile& t = asd_gemm_tiles[i];
    const int32_t v[7] = {t.kind, t.bm, t.bn, t.wm, t.wn, t.nst, t.kg};
    memcpy(out7, v, sizeof(v));
    return ASD_OK;
}

}  // extern "C"
