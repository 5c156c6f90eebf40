// text.hip — the entries of the CLIP text tower (scaledreamer_amd/diffusion/text_hip.py) that the GEMM / LayerNorm / attention entries do
// not cover, replacing transformers' CLIPTextModel.forward as the reference calls it once per string
// (custom/amortized/models/prompt_processors/stable_diffusion_multi_prompt_processor.py:58-70):
//   asd_text_embed_f16        token_embedding[id] + position_embedding[t]            (CLIPTextEmbeddings.forward)
//   asd_attention_causal_f16  causal multi-head self-attention over <= 128 tokens    (CLIPAttention.forward with the causal mask)
//   asd_gelu_f16              0.5 x (1 + erf(x / sqrt 2))                            (CLIPMLP's activation when hidden_act = "gelu")
//
// Causal attention, one workgroup per (sequence, head), four waves.  A head's K (L x 64) and V are at most 16 KB each, so both live in
// LDS whole and there is no key loop to pipeline and no online softmax: a wave takes 16 query rows at a time and holds the whole score
// row of each (<= 128 keys: 8 accumulator tiles) in registers.  As in attention.hip everything is computed transposed, so the
// probabilities never leave registers:
//   S^T = K Q^T    MFMA 16x16x32: A = K fragment from LDS (lane: key l&15, d = 8 (l>>4) .. +8), B = Q fragment read from memory
//                  -> lane (l&15) owns ONE query, its 4 accumulator rows are keys 16 kt + 4 (l>>4) + r
//   O^T = V^T P^T  A = V^T fragment from LDS, B = P^T = exp2(..) rounded to fp16 in place; the k index of this MFMA runs over two
//                  16-key tiles in the order the score accumulators already have (keys 4 lg .. +4 of tile 2j, then of tile 2j + 1),
//                  and the V^T fragment is read in the same order, so P needs no transpose
//                  -> the same lane owns the same query and 4 consecutive head-dim values: 8-byte stores.
// Key tiles wholly above the diagonal (kt > qt) are never computed; the diagonal tile is masked per element (key > query -> -inf)
// before the maximum, so a masked probability is exactly 0 and rows <= t do not depend on rows > t bit for bit.
//
// LDS images (bank of byte a for ds_read_b64 / b128: (a / 4) % 64, i.e. a 256-byte bank row):
//   K    [key][64] fp16, 128-byte rows, read with ds_read_b128 by (key l&15, chunk ks 4 + lg): linear rows would put 16 keys on two
//        16-byte slots; the 16-byte chunk index is XORed with (key & 7), the swizzle of attention.hip's K tile.
//   V^T  [d][136] fp16: 128 keys + 8 of padding = 272-byte rows.  ds_read_b64 works per 32-lane half (16 rows d x 2 lane groups):
//        row d starts 16 bytes further along the bank row than row d - 1 and the two lane groups are 8 bytes apart: the 32 reads of
//        a half cover the 256-byte bank row exactly once.  V arrives row-major ([key][d], the layout of the fused qkv GEMM) and is
//        transposed on its way into LDS with 2-byte writes, lanes along the keys (consecutive 2-byte addresses of one row).
// Keys and query rows from L up to the tile edge are never read from memory: their LDS rows are written as zeros (finite, so a zero
// probability times them is zero) and their Q fragments are zeros; their outputs are not stored.
#include "gemm_tile.h"

#define TXT_BLOCK 256
#define TXT_HD 64
#define TXT_MAX_L 128
#define TXT_VT_LD 136                                  // fp16 per V^T row: 128 keys + 8
#define TXT_K_BYTES (TXT_MAX_L * TXT_HD * 2)           // 16384
#define TXT_VT_BYTES (TXT_HD * TXT_VT_LD * 2)          // 17408

// ---- token + position embedding ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TXT_BLOCK) void text_embed_kernel(const int32_t* __restrict__ ids, int64_t rows, int L, int vocab, int C,
                                                                const half_t* __restrict__ tok, const half_t* __restrict__ pos,
                                                                half_t* __restrict__ out) {
    const int c8 = C >> 3;
    const int64_t n = rows * c8;
    for (int64_t i = (int64_t)blockIdx.x * TXT_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * TXT_BLOCK) {
        const int64_t row = i / c8;
        const int c = (int)(i - row * c8) * 8;
        int id = ids[row];
        id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);       // the wrapper has validated the ids; never read outside the table
        const int t = (int)(row % L);
        const half8 a = *(const half8*)(tok + (size_t)id * C + c), b = *(const half8*)(pos + (size_t)t * C + c);
        half8 o;
#pragma unroll
        for (int k = 0; k < 8; ++k) o[k] = (half_t)((float)a[k] + (float)b[k]);
        *(half8*)(out + (size_t)row * C + c) = o;
    }
}

// ---- exact-form GELU: gelu_erf of gemm_tile.h, the formula of the GEGLU epilogue ---------------------------------------------------------
__global__ __launch_bounds__(TXT_BLOCK) void gelu_kernel(const half_t* __restrict__ x, int64_t n, half_t* __restrict__ y) {
    const int64_t n8 = n >> 3;
    for (int64_t i = (int64_t)blockIdx.x * TXT_BLOCK + threadIdx.x; i < n8; i += (int64_t)gridDim.x * TXT_BLOCK) {
        const half8 v = *(const half8*)(x + i * 8);
        half8 o;
#pragma unroll
        for (int k = 0; k < 8; ++k) o[k] = (half_t)gelu_erf((float)v[k]);
        *(half8*)(y + i * 8) = o;
    }
    const int64_t t = 8 * n8 + threadIdx.x;
    if (blockIdx.x == 0 && t < n) y[t] = (half_t)gelu_erf((float)x[t]);
}

// ---- causal self-attention ----------------------------------------------------------------------------------------------------------------
struct CausalArgs {
    const half_t* q; int ldq;
    const half_t* k; int ldk;
    const half_t* v; int ldv;
    half_t* o; int ldo;
    int heads, L;
    float scale;
};

__global__ __launch_bounds__(TXT_BLOCK) void attention_causal_kernel(const CausalArgs p) {
    __shared__ __attribute__((aligned(16))) char smem[TXT_K_BYTES + TXT_VT_BYTES];
    char* Ks = smem;
    half_t* Vt = (half_t*)(smem + TXT_K_BYTES);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = (int)blockIdx.x / p.heads, h = (int)blockIdx.x % p.heads;
    const int L = p.L;
    const int nq = (L + 15) >> 4;                  // 16-row query tiles = 16-key tiles
    const int lpad16 = nq * 16, lpad32 = ((nq + 1) >> 1) * 32;
    const size_t row0 = (size_t)b * L;

    // ---- K: 16-byte chunks, chunk index XOR (key & 7); rows L .. lpad16 are zeros
    for (int i = tid; i < lpad16 * 8; i += TXT_BLOCK) {
        const int key = i >> 3, c = i & 7;
        half8 val = {0, 0, 0, 0, 0, 0, 0, 0};
        if (key < L) val = *(const half8*)(p.k + (row0 + key) * p.ldk + h * TXT_HD + c * 8);
        *(half8*)(Ks + key * 128 + ((c ^ (key & 7)) * 16)) = val;
    }
    // ---- V -> V^T: lanes along the keys; columns L .. lpad32 are zeros
    for (int i = tid; i < lpad32 * 8; i += TXT_BLOCK) {
        const int key = i % lpad32, c = i / lpad32;
        half8 val = {0, 0, 0, 0, 0, 0, 0, 0};
        if (key < L) val = *(const half8*)(p.v + (row0 + key) * p.ldv + h * TXT_HD + c * 8);
#pragma unroll
        for (int e = 0; e < 8; ++e) Vt[(c * 8 + e) * TXT_VT_LD + key] = val[e];
    }
    __syncthreads();

    const int lq16 = lane & 15, lg = lane >> 4;
    const float sl2 = p.scale * 1.44269504088896340736f;        // softmax in the log2 domain
    for (int qt = nq - 1 - wave; qt >= 0; qt -= 4) {              // the long rows first: wave 0 takes tiles nq - 1 and nq - 5
        const int qi = qt * 16 + lq16;
        half8 qf[2];
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            qf[ks] = half8{0, 0, 0, 0, 0, 0, 0, 0};
            if (qi < L) qf[ks] = *(const half8*)(p.q + (row0 + qi) * p.ldq + h * TXT_HD + ks * 32 + lg * 8);
        }
        // ---- S^T = K Q^T over the key tiles 0 .. qt
        floatx4 s[8];
#pragma unroll
        for (int kt = 0; kt < 8; ++kt) {
            s[kt] = floatx4{-INFINITY, -INFINITY, -INFINITY, -INFINITY};
            if (kt <= qt) {                                       // wave-uniform
                const int row = kt * 16 + lq16;
                floatx4 a = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int ks = 0; ks < 2; ++ks) {
                    const half8 kf = *(const half8*)(Ks + row * 128 + (((ks * 4 + lg) ^ (row & 7)) * 16));
                    a = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf, qf[ks], a, 0, 0, 0);
                }
                if (kt == qt) {                                   // the diagonal tile: key 16 kt + 4 lg + r against query 16 qt + lq16
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if (lg * 4 + r > lq16) a[r] = -INFINITY;
                }
                s[kt] = a;
            }
        }
        // ---- softmax of the row: key 0 is never masked, so the maximum is finite
        float mx = -INFINITY;
#pragma unroll
        for (int kt = 0; kt < 8; ++kt)
#pragma unroll
            for (int r = 0; r < 4; ++r) mx = fmaxf(mx, s[kt][r]);
        mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        const float nm = -mx * sl2;
        half8 pb[4];          // [j]: B operand of PV k-step j: keys 4 lg .. +4 of tile 2j (elements 0-3) and of tile 2j + 1 (4-7)
        float sum = 0.f;
#pragma unroll
        for (int kt = 0; kt < 8; ++kt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const half_t e = (half_t)__builtin_amdgcn_exp2f(fmaf(s[kt][r], sl2, nm));      // exp2(-inf) = 0 for masked / absent keys
                pb[kt >> 1][(kt & 1) * 4 + r] = e;
                sum += (float)e;                                  // the normaliser of exactly what multiplies V
            }
        sum += __shfl_xor(sum, 16, 64);
        sum += __shfl_xor(sum, 32, 64);
        // ---- O^T = V^T P^T
        floatx4 oacc[4];
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) oacc[dt] = floatx4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (2 * j <= qt) {                                    // wave-uniform; keys 32 j .. 32 j + 31 < lpad32
#pragma unroll
                for (int dt = 0; dt < 4; ++dt) {
                    const half_t* vrow = Vt + (dt * 16 + lq16) * TXT_VT_LD + 32 * j + 4 * lg;
                    const half4 v_lo = *(const half4*)vrow, v_hi = *(const half4*)(vrow + 16);
                    const half8 vf = half8{v_lo[0], v_lo[1], v_lo[2], v_lo[3], v_hi[0], v_hi[1], v_hi[2], v_hi[3]};
                    oacc[dt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(vf, pb[j], oacc[dt], 0, 0, 0);
                }
            }
        }
        if (qi < L) {
            const float inv = 1.f / sum;
            half_t* dst = p.o + (row0 + qi) * p.ldo + h * TXT_HD;
#pragma unroll
            for (int dt = 0; dt < 4; ++dt) {
                const floatx4 v = oacc[dt];
                const half4 o = {(half_t)(v[0] * inv), (half_t)(v[1] * inv), (half_t)(v[2] * inv), (half_t)(v[3] * inv)};
                *(half4*)(dst + dt * 16 + lg * 4) = o;
            }
        }
    }
}

extern "C" {

int asd_text_embed_f16(const int32_t* input_ids, int32_t P, int32_t L, int32_t vocab, int32_t C, const void* token_embedding,
                       const void* position_embedding, void* x, void* stream) {
    ASD_CHECK_ARG(input_ids && token_embedding && position_embedding && x, "null argument");
    ASD_CHECK_ARG(P >= 1 && L >= 1 && vocab >= 1, "P, L and vocab must be >= 1");
    ASD_CHECK_ARG(C >= 8 && C % 8 == 0, "channels must be a multiple of 8");
    ASD_CHECK_ARG((((uintptr_t)token_embedding | (uintptr_t)position_embedding | (uintptr_t)x) & 15) == 0, "tables and x must be 16-byte aligned");
    const int64_t rows = (int64_t)P * L;
    hipLaunchKernelGGL(text_embed_kernel, dim3(asd_grid_for(rows * (C / 8), TXT_BLOCK)), dim3(TXT_BLOCK), 0, (hipStream_t)stream, input_ids, rows, (int)L,
                       (int)vocab, (int)C, (const half_t*)token_embedding, (const half_t*)position_embedding, (half_t*)x);
    ASD_LAUNCH_CHECK();
    return ASD_OK;
}

int asd_attention_causal_f16(const void* q, int32_t ldq, const void* k, int32_t ldk, const void* v, int32_t ldv, void* o, int32_t ldo,
                             int32_t batch, int32_t heads, int32_t L, float scale, void* stream) {
    ASD_CHECK_ARG(q && k && v && o, "null argument");
    ASD_CHECK_ARG(batch > 0 && heads > 0 && (int64_t)batch * heads <= INT32_MAX, "bad batch / heads");
    ASD_CHECK_ARG(L >= 1 && L <= TXT_MAX_L, "sequence length must be in [1, 128]");
    ASD_CHECK_ARG(scale > 0.f && scale < INFINITY, "scale must be positive and finite");
    ASD_CHECK_ARG(ldq >= heads * TXT_HD && ldk >= heads * TXT_HD && ldv >= heads * TXT_HD && ldo >= heads * TXT_HD, "leading dimension below heads * 64");
    ASD_CHECK_ARG(ldq % 8 == 0 && ldk % 8 == 0 && ldv % 8 == 0 && ldo % 4 == 0, "leading dimensions must keep 16-byte (o: 8-byte) alignment");
    ASD_CHECK_ARG((((uintptr_t)q | (uintptr_t)k | (uintptr_t)v) & 15) == 0 && ((uintptr_t)o & 7) == 0, "q, k, v must be 16-byte and o 8-byte aligned");
    CausalArgs a{(const half_t*)q, ldq, (const half_t*)k, ldk, (const half_t*)v, ldv, (half_t*)o, ldo, heads, L, scale};
    hipLaunchKernelGGL(attention_causal_kernel, dim3((unsigned)(batch * heads)), dim3(TXT_BLOCK), 0, (hipStream_t)stream, a);
    ASD_LAUNCH_CHECK();
    return ASD_OK;
}

int asd_gelu_f16(const void* x, int64_t n, void* y, void* stream) {
    ASD_CHECK_ARG(x && y && n > 0, "bad argument");
    ASD_CHECK_ARG((((uintptr_t)x | (uintptr_t)y) & 15) == 0, "x and y must be 16-byte aligned");
    hipLaunchKernelGGL(gelu_kernel, dim3(asd_grid_for(n / 8, TXT_BLOCK)), dim3(TXT_BLOCK), 0, (hipStream_t)stream, (const half_t*)x, n, (half_t*)y);
    ASD_LAUNCH_CHECK();
    return ASD_OK;
}

}  // extern "C"
