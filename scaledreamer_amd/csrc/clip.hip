// clip.hip — the parts of a CLIP ViT evaluation that are not a GEMM, a LayerNorm or an attention (those are asd_gemm_f16, asd_layernorm_f16
// and asd_attention_f16): the image front end, the token assembly, quick-GELU and the image-text scoring.  The schedule that strings them
// together is scaledreamer_amd/clip_eval.py.
//
// asd_clip_preprocess_u8: crop the left H x H square of every frame, resize it to S x S as PIL's Image.resize(BILINEAR) does on 8-bit data
//   (two passes of integer multiply-accumulates over host-built tap tables, rounded to a byte after each pass), normalise in fp32 and
//   scatter into the patch rows the patch-embedding GEMM reads: row b g^2 + py g + px (stride ldp), column c P^2 + dy P + dx, zero up to Kpad.
//   Both sides of the crop are H, so either both passes run or (H == S) none does; the second kernel then reads the frames directly.
// asd_clip_embed_f16: LayerNorm_pre(cat(class, patches) + position) into [B, Lpad, C]; a wave owns a row, as in asd_layernorm_f16; the
//   rows L .. Lpad of every image are written as zeros (they are keys the attention masks; they must be finite, nothing more).
// asd_quick_gelu_f16: y = x sigmoid(1.702 x), 16-byte loads and stores, any n (the last n % 8 values one by one).
// asd_clip_score_f32: fp32 throughout, no atomics.  Pass 1: a block takes CS_IMGS images (L2-normalised into LDS) and CS_PCHUNK prompts and
//   leaves each image's best (value, index) of that chunk in the workspace; a dot product is summed in the same order wherever it is
//   computed, so equal text rows give equal values and the lowest index wins.  Pass 2: a wave per image folds the chunks and computes
//   the similarity with the image's own prompt.  clip_score_layout is the one definition of the chunk count and the workspace size.
#include <math.h>

#include "asd_common.h"


#define CLIP_BLOCK 256
#define CLIP_PREC_BITS 22          // PIL's PRECISION_BITS = 32 - 8 - 2

// ---- preprocess -------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int clip8(int v) {
    v >>= CLIP_PREC_BITS;
    return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// horizontal pass over the cropped square: tmp [B, H, S, 3]
__global__ __launch_bounds__(CLIP_BLOCK) void clip_resize_h_kernel(const uint8_t* __restrict__ frames, int64_t n, int H, int Wfull, int S,
                                                                   const int32_t* __restrict__ bounds, const int32_t* __restrict__ kk, int ksize,
                                                                   uint8_t* __restrict__ tmp) {
    for (int64_t i = (int64_t)blockIdx.x * CLIP_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * CLIP_BLOCK) {
        const int xx = (int)(i % S);
        const int64_t row = i / S;                                  // b H + y
        const int xmin = bounds[2 * xx], cnt = bounds[2 * xx + 1];
        const uint8_t* __restrict__ src = frames + (row * Wfull + xmin) * 3;
        const int32_t* __restrict__ k = kk + (int64_t)xx * ksize;
        int s0 = 1 << (CLIP_PREC_BITS - 1), s1 = s0, s2 = s0;
        for (int x = 0; x < cnt; ++x) {
            const int w = k[x];
            s0 += (int)src[3 * x] * w; s1 += (int)src[3 * x + 1] * w; s2 += (int)src[3 * x + 2] * w;
        }
        uint8_t* __restrict__ o = tmp + i * 3;
        o[0] = (uint8_t)clip8(s0); o[1] = (uint8_t)clip8(s1); o[2] = (uint8_t)clip8(s2);
    }
}

struct ClipNorm {
    float mean[3], std[3];
};

// vertical pass (or, with do_v == 0, a plain read of the S x S frame), normalisation, patch rows.  src: rows of row_stride bytes, images of
// img_stride bytes, Hin rows each.
__global__ __launch_bounds__(CLIP_BLOCK) void clip_resize_v_patch_kernel(const uint8_t* __restrict__ src, int64_t row_stride, int64_t img_stride,
                                                                         int64_t n, int S, int P, int Kpad, int ldp, int do_v,
                                                                         const int32_t* __restrict__ bounds, const int32_t* __restrict__ kk,
                                                                         int ksize, ClipNorm nm, uint8_t* __restrict__ resized,
                                                                         half_t* __restrict__ patches) {
    const int g = S / P, pp = P * P;
    for (int64_t i = (int64_t)blockIdx.x * CLIP_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * CLIP_BLOCK) {
        const int xx = (int)(i % S);
        const int64_t by = i / S;
        const int yy = (int)(by % S);
        const int64_t b = by / S;
        int px[3];
        if (do_v) {
            const int ymin = bounds[2 * yy], cnt = bounds[2 * yy + 1];
            const uint8_t* __restrict__ s = src + b * img_stride + ymin * row_stride + (int64_t)xx * 3;
            const int32_t* __restrict__ k = kk + (int64_t)yy * ksize;
            int s0 = 1 << (CLIP_PREC_BITS - 1), s1 = s0, s2 = s0;
            for (int y = 0; y < cnt; ++y) {
                const int w = k[y];
                s0 += (int)s[0] * w; s1 += (int)s[1] * w; s2 += (int)s[2] * w;
                s += row_stride;
            }
            px[0] = clip8(s0); px[1] = clip8(s1); px[2] = clip8(s2);
        } else {
            const uint8_t* __restrict__ s = src + b * img_stride + yy * row_stride + (int64_t)xx * 3;
            px[0] = s[0]; px[1] = s[1]; px[2] = s[2];
        }
        if (resized) {
            uint8_t* __restrict__ o = resized + i * 3;
            o[0] = (uint8_t)px[0]; o[1] = (uint8_t)px[1]; o[2] = (uint8_t)px[2];
        }
        const int py = yy / P, dy = yy - py * P, pxi = xx / P, dx = xx - pxi * P;
        half_t* __restrict__ row = patches + ((b * g + py) * g + pxi) * ldp;
#pragma unroll
        for (int c = 0; c < 3; ++c) row[c * pp + dy * P + dx] = (half_t)(((float)px[c] / 255.0f - nm.mean[c]) / nm.std[c]);
        if (dy == 0 && dx == 0)
            for (int c = 3 * pp; c < Kpad; ++c) row[c] = (half_t)0.f;
    }
}

// ---- token assembly + pre-LayerNorm: a wave owns a row of [B, Lpad, C], NV = ceil(C / 512) 16-byte loads per lane ------------------------
template <int NV>
__global__ __launch_bounds__(CLIP_BLOCK) void clip_embed_kernel(const half_t* __restrict__ patch, const half_t* __restrict__ cls,
                                                                const half_t* __restrict__ pos, const half_t* __restrict__ gamma,
                                                                const half_t* __restrict__ beta, float eps, int64_t rows, int g2, int C, int Lpad,
                                                                half_t* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), n_waves = (int64_t)gridDim.x * 4;
    const int L = g2 + 1;
    const float inv_c = 1.f / (float)C;
    for (int64_t row = wave; row < rows; row += n_waves) {
        const int64_t b = row / Lpad;
        const int t = (int)(row - b * Lpad);
        half_t* __restrict__ o = out + row * C;
        if (t >= L) {
            half8 z;
#pragma unroll
            for (int k = 0; k < 8; ++k) z[k] = (half_t)0.f;
#pragma unroll
            for (int j = 0; j < NV; ++j)
                if (lane * 8 + j * 512 < C) *(half8*)(o + lane * 8 + j * 512) = z;
            continue;
        }
        const half_t* __restrict__ xr = t == 0 ? cls : patch + (b * g2 + (t - 1)) * C;
        const half_t* __restrict__ pr = pos + (int64_t)t * C;
        float v[NV][8];
        float s = 0.f;
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const int c = lane * 8 + j * 512;
            if (c < C) {
                const half8 a = *(const half8*)(xr + c), p = *(const half8*)(pr + c);
#pragma unroll
                for (int k = 0; k < 8; ++k) { v[j][k] = (float)a[k] + (float)p[k]; s += v[j][k]; }
            }
        }
        const float mean = asd_wave_sum(s) * inv_c;
        float q = 0.f;
#pragma unroll
        for (int j = 0; j < NV; ++j)
            if (lane * 8 + j * 512 < C) {
#pragma unroll
                for (int k = 0; k < 8; ++k) { const float d = v[j][k] - mean; q = fmaf(d, d, q); }
            }
        const float rstd = rsqrtf(asd_wave_sum(q) * inv_c + eps);
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const int c = lane * 8 + j * 512;
            if (c < C) {
                const half8 gm = *(const half8*)(gamma + c), bt = *(const half8*)(beta + c);
                half8 y;
#pragma unroll
                for (int k = 0; k < 8; ++k) y[k] = (half_t)((v[j][k] - mean) * rstd * (float)gm[k] + (float)bt[k]);
                *(half8*)(o + c) = y;
            }
        }
    }
}

// ---- quick-GELU ---------------------------------------------------------------------------------------------------------------------------
#define CLIP_QG_T (-1.702f * 1.4426950408889634f)      // x sigmoid(1.702 x) = x / (1 + exp2(-1.702 log2(e) x))
__device__ __forceinline__ float quick_gelu_f(float x) { return x * asd_sigmoid_exp2(CLIP_QG_T * x); }

__global__ __launch_bounds__(CLIP_BLOCK) void quick_gelu_kernel(const half_t* __restrict__ x, int64_t n, half_t* __restrict__ y) {
    const int64_t n8 = n >> 3;
    for (int64_t i = (int64_t)blockIdx.x * CLIP_BLOCK + threadIdx.x; i < n8; i += (int64_t)gridDim.x * CLIP_BLOCK) {
        const half8 v = *(const half8*)(x + i * 8);
        half8 o;
#pragma unroll
        for (int k = 0; k < 8; ++k) o[k] = (half_t)quick_gelu_f((float)v[k]);
        *(half8*)(y + i * 8) = o;
    }
    const int64_t t = 8 * n8 + threadIdx.x;
    if (blockIdx.x == 0 && t < n) y[t] = (half_t)quick_gelu_f((float)x[t]);
}

// ---- scoring ------------------------------------------------------------------------------------------------------------------------------
#define CS_IMGS 8              // images of a block
#define CS_PCHUNK 64           // prompts of a block: 16 per wave
#define CS_MAX_D 1024          // CS_IMGS rows of D floats in LDS: 32 KB

struct ClipScoreLayout {
    int64_t chunks;            // prompt chunks
    int64_t ws_bytes;          // {float value [B, chunks], int32 index [B, chunks]}
};

static bool clip_score_layout(const char* fn, int64_t B, int64_t P, ClipScoreLayout* out) {
    if (B < 0 || P < 1 || B > INT32_MAX || P > INT32_MAX) {
        asd_set_error("%s: B must be >= 0 and P >= 1 (got %lld, %lld)", fn, (long long)B, (long long)P);
        return false;
    }
    out->chunks = (P + CS_PCHUNK - 1) / CS_PCHUNK;
    if (out->chunks > 65535) {
        asd_set_error("%s: %lld prompts exceed one grid", fn, (long long)P);
        return false;
    }
    out->ws_bytes = B * out->chunks * 8;
    return true;
}

// 1 / |row| of a row of D floats, in every lane of the wave
__device__ __forceinline__ float clip_inv_norm(const float* __restrict__ r, int D) {
    float s = 0.f;
    for (int d = asd_lane(); d < D; d += 64) s = fmaf(r[d], r[d], s);
    return 1.f / sqrtf(asd_wave_sum(s));
}

// <normalised image row, text row>, in every lane of the wave: the one order of summation of this file
__device__ __forceinline__ float clip_dot(const float* __restrict__ a, const float* __restrict__ t, int D) {
    float s = 0.f;
    for (int d = asd_lane(); d < D; d += 64) s = fmaf(a[d], t[d], s);
    return asd_wave_sum(s);
}

__global__ __launch_bounds__(CLIP_BLOCK) void clip_score_chunk_kernel(const float* __restrict__ img, const float* __restrict__ txt, int B, int P, int D,
                                                                      int chunks, float* __restrict__ part_val, int32_t* __restrict__ part_idx) {
    extern __shared__ __attribute__((aligned(16))) float s_img[];      // [CS_IMGS][D], normalised
    __shared__ float s_val[4][CS_IMGS];
    __shared__ int s_idx[4][CS_IMGS];
    const int lane = asd_lane(), wave = (int)threadIdx.x >> 6;
    const int b0 = (int)blockIdx.x * CS_IMGS, p0 = (int)blockIdx.y * CS_PCHUNK;
    const int nb = B - b0 < CS_IMGS ? B - b0 : CS_IMGS;
    for (int i = wave; i < nb; i += 4) {
        const float* __restrict__ r = img + (int64_t)(b0 + i) * D;
        const float inv = clip_inv_norm(r, D);
        for (int d = lane; d < D; d += 64) s_img[i * D + d] = r[d] * inv;
    }
    __syncthreads();
    float best[CS_IMGS];
    int besti[CS_IMGS];
#pragma unroll
    for (int i = 0; i < CS_IMGS; ++i) { best[i] = -INFINITY; besti[i] = P; }
    const int p_end = p0 + CS_PCHUNK < P ? p0 + CS_PCHUNK : P;
    for (int p = p0 + wave; p < p_end; p += 4) {
        const float* __restrict__ t = txt + (int64_t)p * D;
#pragma unroll
        for (int i = 0; i < CS_IMGS; ++i) {
            if (i < nb) {                                  // block-uniform
                const float v = clip_dot(s_img + i * D, t, D);
                if (v > best[i]) { best[i] = v; besti[i] = p; }      // p ascends within a wave: the first maximum stays
            }
        }
    }
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < CS_IMGS; ++i) { s_val[wave][i] = best[i]; s_idx[wave][i] = besti[i]; }
    }
    __syncthreads();
    const int i = (int)threadIdx.x;
    if (i < nb) {
        float v = s_val[0][i];
        int at = s_idx[0][i];
        for (int w = 1; w < 4; ++w) {
            const float u = s_val[w][i];
            const int ui = s_idx[w][i];
            if (u > v || (u == v && ui < at)) { v = u; at = ui; }
        }
        part_val[(int64_t)(b0 + i) * chunks + blockIdx.y] = v;
        part_idx[(int64_t)(b0 + i) * chunks + blockIdx.y] = at;
    }
}

// one wave per image: fold the chunks (lowest index among equal values), similarity with the own prompt
__global__ __launch_bounds__(64) void clip_score_fold_kernel(const float* __restrict__ img, const float* __restrict__ txt, const int32_t* __restrict__ own,
                                                             int P, int D, int chunks, const float* __restrict__ part_val,
                                                             const int32_t* __restrict__ part_idx, float* __restrict__ sim, int32_t* __restrict__ top1) {
    const int b = (int)blockIdx.x, lane = asd_lane();
    float v = -INFINITY;
    int at = P;
    for (int c = lane; c < chunks; c += 64) {
        const float u = part_val[(int64_t)b * chunks + c];
        const int ui = part_idx[(int64_t)b * chunks + c];
        if (u > v || (u == v && ui < at)) { v = u; at = ui; }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const float u = __shfl_xor(v, o, 64);
        const int ui = __shfl_xor(at, o, 64);
        if (u > v || (u == v && ui < at)) { v = u; at = ui; }
    }
    const float* __restrict__ r = img + (int64_t)b * D;
    const int o = own[b];
    float s = NAN;
    if (o >= 0 && o < P) {                                 // wave-uniform
        const float inv = clip_inv_norm(r, D);
        const float* __restrict__ t = txt + (int64_t)o * D;
        float acc = 0.f;
        for (int d = lane; d < D; d += 64) acc = fmaf(r[d] * inv, t[d], acc);
        s = asd_wave_sum(acc);
    }
    if (lane == 0) { sim[b] = s; top1[b] = at; }
}

extern "C" {

int asd_clip_preprocess_u8(const uint8_t* frames, int32_t B, int32_t H, int32_t Wfull, int32_t S, int32_t P, int32_t Kpad, const int32_t* bounds,
                           const int32_t* kk, int32_t ksize, uint8_t* tmp, uint8_t* resized, void* patches, int32_t ldp, void* stream) {
    ASD_CHECK_ARG(B >= 0 && H >= 1 && S >= 1 && P >= 1, "B must be >= 0, H, S and P >= 1");
    ASD_CHECK_ARG(Wfull >= H, "the frame is narrower than it is high: no left H x H square to crop");
    ASD_CHECK_ARG(S % P == 0, "the patch size must divide the image size");
    ASD_CHECK_ARG(Kpad >= 3 * P * P && Kpad % 8 == 0, "Kpad must be a multiple of 8 and >= 3 P^2");
    ASD_CHECK_ARG(ldp >= Kpad, "the row stride of the patch rows must be >= Kpad");
    if (B == 0) return ASD_OK;
    ASD_CHECK_ARG(frames && patches, "null argument");
    const bool pass = H != S;
    ASD_CHECK_ARG(!pass || (bounds && kk && tmp && ksize >= 1), "H != S needs the tap tables (bounds [S, 2], kk [S, ksize]) and tmp [B, H, S, 3]");
    ClipNorm nm = {{0.48145466f, 0.4578275f, 0.40821073f}, {0.26862954f, 0.26130258f, 0.27577711f}};
    hipStream_t s = (hipStream_t)stream;
    const int64_t n_out = (int64_t)B * S * S;
    if (pass) {
        const int64_t n_h = (int64_t)B * H * S;
        hipLaunchKernelGGL(clip_resize_h_kernel, dim3(asd_grid_for(n_h, CLIP_BLOCK)), dim3(CLIP_BLOCK), 0, s, frames, n_h, (int)H, (int)Wfull, (int)S,
                           bounds, kk, (int)ksize, tmp);
        ASD_LAUNCH_CHECK();
        hipLaunchKernelGGL(clip_resize_v_patch_kernel, dim3(asd_grid_for(n_out, CLIP_BLOCK)), dim3(CLIP_BLOCK), 0, s, (const uint8_t*)tmp, (int64_t)S * 3,
                           (int64_t)H * S * 3, n_out, (int)S, (int)P, (int)Kpad, (int)ldp, 1, bounds, kk, (int)ksize, nm, resized, (half_t*)patches);
    } else {
        hipLaunchKernelGGL(clip_resize_v_patch_kernel, dim3(asd_grid_for(n_out, CLIP_BLOCK)), dim3(CLIP_BLOCK), 0, s, frames, (int64_t)Wfull * 3,
                           (int64_t)H * Wfull * 3, n_out, (int)S, (int)P, (int)Kpad, (int)ldp, 0, bounds, kk, (int)ksize, nm, resized, (half_t*)patches);
    }
    ASD_LAUNCH_CHECK();
    return ASD_OK;
}

int asd_clip_embed_f16(const void* patch, const void* class_embedding, const void* position_embedding, const void* gamma, const void* beta, float eps,
                       int32_t B, int32_t g2, int32_t C, int32_t Lpad, void* out, void* stream) {
    ASD_CHECK_ARG(patch && class_embedding && position_embedding && gamma && beta && out, "null argument");
    ASD_CHECK_ARG(B >= 1 && g2 >= 1, "B and g2 must be >= 1");
    ASD_CHECK_ARG(C % 8 == 0 && C >= 8 && C <= 2048, "channels must be a multiple of 8 and <= 2048");
    ASD_CHECK_ARG(Lpad >= g2 + 1 && Lpad % 8 == 0, "Lpad must be a multiple of 8 and >= g2 + 1");
    ASD_CHECK_ARG((((uintptr_t)patch | (uintptr_t)class_embedding | (uintptr_t)position_embedding | (uintptr_t)gamma | (uintptr_t)beta | (uintptr_t)out) & 15) == 0,
                  "operands must be 16-byte aligned");
    const int64_t rows = (int64_t)B * Lpad;
    int blocks = asd_div_up(rows, 4);
    if (blocks > 2048) blocks = 2048;
    hipStream_t s = (hipStream_t)stream;
#define EMBED_LAUNCH(NV) hipLaunchKernelGGL((clip_embed_kernel<NV>), dim3(blocks), dim3(CLIP_BLOCK), 0, s, (const half_t*)patch, (const half_t*)class_embedding, \
                                            (const half_t*)position_embedding, (const half_t*)gamma, (const half_t*)beta, eps, rows, (int)g2, (int)C, (int)Lpad, (half_t*)out)
    if (C <= 512) EMBED_LAUNCH(1);
    else if (C <= 1024) EMBED_LAUNCH(2);
    else if (C <= 1536) EMBED_LAUNCH(3);
    else EMBED_LAUNCH(4);
#undef EMBED_LAUNCH
    ASD_LAUNCH_CHECK();
    return ASD_OK;
}

int asd_quick_gelu_f16(const void* x, int64_t n, void* y, void* stream) {
    ASD_CHECK_ARG(x && y && n > 0, "bad argument");
    ASD_CHECK_ARG((((uintptr_t)x | (uintptr_t)y) & 15) == 0, "x and y must be 16-byte aligned");
    hipLaunchKernelGGL(quick_gelu_kernel, dim3(asd_grid_for(n / 8, CLIP_BLOCK)), dim3(CLIP_BLOCK), 0, (hipStream_t)stream, (const half_t*)x, n, (half_t*)y);
    ASD_LAUNCH_CHECK();
    return ASD_OK;
}

int64_t asd_clip_score_workspace(int64_t B, int64_t P) {
    ClipScoreLayout lay;
    if (!clip_score_layout(__func__, B, P, &lay)) return -1;
    return lay.ws_bytes;
}

int asd_clip_score_f32(const float* img, const float* txt, const int32_t* own, int64_t B, int64_t P, int32_t D, float* sim, int32_t* top1,
                       void* workspace, int64_t workspace_bytes, void* stream) {
    ClipScoreLayout lay;
    if (!clip_score_layout(__func__, B, P, &lay)) return ASD_ERR_ARG;
    ASD_CHECK_ARG(D >= 1 && D <= CS_MAX_D, "D must be in [1, 1024]");
    if (B == 0) return ASD_OK;
    ASD_CHECK_ARG(img && txt && own && sim && top1, "null argument");
    ASD_CHECK_ARG(workspace && workspace_bytes >= lay.ws_bytes && ((uintptr_t)workspace & 3) == 0,
                  "workspace smaller than asd_clip_score_workspace, or not 4-byte aligned");
    float* part_val = (float*)workspace;
    int32_t* part_idx = (int32_t*)workspace + B * lay.chunks;
    hipStream_t s = (hipStream_t)stream;
    const size_t lds = (size_t)CS_IMGS * D * sizeof(float);
    hipLaunchKernelGGL(clip_score_chunk_kernel, dim3((unsigned)((B + CS_IMGS - 1) / CS_IMGS), (unsigned)lay.chunks), dim3(CLIP_BLOCK), lds, s, img, txt,
                       (int)B, (int)P, (int)D, (int)lay.chunks, part_val, part_idx);
    ASD_LAUNCH_CHECK();
    hipLaunchKernelGGL(clip_score_fold_kernel, dim3((unsigned)B), dim3(64), 0, s, img, txt, own, (int)P, (int)D, (int)lay.chunks, (const float*)part_val,
                       (const int32_t*)part_idx, sim, top1);
    ASD_LAUNCH_CHECK();
    return ASD_OK;
}

}  // extern "C"
