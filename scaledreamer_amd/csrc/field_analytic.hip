// field_analytic.hip — analytic normals of the fused field for gfx950 (wave64, one thread per point): the gradient of the activated
// density with respect to the sample position, and its derivative with respect to the hash tables and the MLP weights.
//
// Replaces, behind the C ABI of include/asd_hip.h:
//   normal_type "analytic" of ImplicitVolume.forward (threestudio/models/geometry/implicit_volume.py:114-116, 181-190):
//   normal = -F.normalize(autograd.grad(density, points, create_graph=True)), and the double backward tcnn / autograd give it.
//
// Notation for one point p:
//   u_k = (p_k - bbox_min_k) / (bbox_max_k - bbox_min_k), c_k = 1 / (bbox_max_k - bbox_min_k), enc[32] = hash-grid encoding of u,
//   D[j][k] = d enc_j / d u_k = s_l * sum over the 8 corners of (+-1 on axis k) * (the other two axes' weights) * T[idx]  (the encode's own gathers),
//   a = W1 enc, m_h = [a_h > 0], raw = w2 . relu(a) + bias(p), sigma = act(raw), g = W1^T (m * w2) = d(MLP out) / d enc.
// Forward:   grad raw_k = c_k sum_j g_j D[j][k] + d bias / d p_k;  grad = act'(raw) grad raw;  normal = -+ grad / max(|grad|, 1e-12).
// Backward:  G = dL/dgrad (the normalise backward and the sign folded in), Gh = act'(raw) G,
//            dL/draw = dL/dsigma act'(raw) + act''(raw) (G . grad raw)    -> the ordinary value path (w2, W1, tables with the value weights),
//            t_j = sum_k c_k Gh_k D[j][k]:  dw2_h += m_h (W1 t)_h,  dW1[h][j] += m_h w2_h t_j,
//            tables: corner c of level l, feature f: += wt_c denc_f + dwt_c g_{2l+f},  dwt_c = s_l sum_k c_k Gh_k d wt_c / d frac_k.
// ReLU and trilinear second derivatives act on the points only and the points carry no gradient: not formed.
//
// Registers: D would be 96 floats on top of enc[32] and g[32] — the budget at which asd_encode's comment reports spills.  Instead the
// corners are gathered again with g (forward) or Gh (backward) already known, so a pass accumulates 3 (or 2 per level) values; the
// second pass finds the 128 corners in the L2 the first one filled.
//
// Where this implementation and the reference differ on purpose: at |p| = 0 the sphere / blob_magic3d bias gradient is 0 here (the reference
// divides 0 by 0: NaN); outside the bounding box the position is clamped to the unit cube (asd_unit), so the encoding's gradient is 0 there.
#include <math.h>

#include "asd_common.h"
#include "field_math.h"

#define AN_W2N 256          // second-layer weight-gradient sums of one block: 64 density + 3 x 64 feature
#define AN_W2_COPIES 16     // one LDS copy per row of 16 lanes, as field_bwd_sample_kernel (ASD_FIELD_W2_COPIES)

__device__ __forceinline__ float an_act_grad2(const asd_field_cfg& c, float raw) {
    switch (c.activation) {
        case ASD_ACT_SOFTPLUS: {
            if (raw > 20.f) return 0.f;
            const float s = asd_sigmoid(raw);
            return s * (1.f - s);
        }
        case ASD_ACT_EXP: return expf(raw);
        case ASD_ACT_TRUNC_EXP: return raw <= 15.f ? expf(raw) : 0.f;
        default: return 0.f;
    }
}

// d bias / d p (field_bias); 0 at |p| = 0
__device__ __forceinline__ void an_bias_grad(const asd_field_cfg& c, float px, float py, float pz, float (&db)[3]) {
    const float r2 = px * px + py * py + pz * pz;
    const float r = sqrtf(r2);
    float k = 0.f;
    if (c.bias_mode == ASD_BIAS_BLOB_MAGIC3D) k = r > 0.f ? -c.blob_scale / (c.blob_std * r) : 0.f;
    else if (c.bias_mode == ASD_BIAS_BLOB_DREAMFUSION) k = -(c.blob_scale * expf(-0.5f * r2 / (c.blob_std * c.blob_std))) / (c.blob_std * c.blob_std);
    else if (c.bias_mode == ASD_BIAS_SPHERE) k = r > 0.f ? 1.f / r : 0.f;
    db[0] = k * px; db[1] = k * py; db[2] = k * pz;
}

// out = w2 . relu(W1 enc) in mlp1's order of operations, and g = W1^T (m * w2)
template <int NIN, int H>
__device__ __forceinline__ float an_mlp1_g(const float* __restrict__ w1, const float* __restrict__ w2, const float (&enc)[NIN],
                                           float (&g)[NIN]) {
    float out = 0.f;
#pragma unroll
    for (int k = 0; k < NIN; ++k) g[k] = 0.f;
#pragma unroll 4
    for (int h = 0; h < H; ++h) {
        float a = 0.f;
#pragma unroll
        for (int k = 0; k < NIN; ++k) a = fmaf(w1[h * NIN + k], enc[k], a);
        out = fmaf(w2[h], fmaxf(a, 0.f), out);
        const float coef = a > 0.f ? w2[h] : 0.f;
#pragma unroll
        for (int k = 0; k < NIN; ++k) g[k] = fmaf(coef, w1[h * NIN + k], g[k]);
    }
    return out;
}

// The passes below gather the corners asd_encode (or an earlier pass) already read.  Left alone, hipcc merges the loads and keeps all 256
// corner values alive from the first pass to the last: 800+ spilled VGPRs.  Passing the position through an empty asm makes the
// addresses new values to the compiler, so each pass loads for itself (from the L2) and holds one group of levels at a time.
__device__ __forceinline__ float an_again(float v) {
    asm volatile("" : "+v"(v));
    return v;
}

// gu_k = sum_j g_j D[j][k]; x, y, z already in the unit cube.  gs: this thread's column of the block's LDS copy of g (stride 256 floats), so
// the level loop stays a loop (fully unrolled, with g in registers, hipcc forms the cells of all 16 levels ahead of the gathers and spills them).
template <int L>
__device__ __forceinline__ void an_pos_grad(const asd_grid_meta& m, const float* __restrict__ params, float x, float y, float z,
                                            const float* gs, float (&gu)[3]) {
    gu[0] = gu[1] = gu[2] = 0.f;
#pragma unroll 2
    for (int l = 0; l < L; ++l) {
        const asd_cell q = asd_cell_of(m, l, x, y, z);
        const float2* __restrict__ tab = reinterpret_cast<const float2*>(params) + m.offset[l];
        float2 v[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) v[c] = tab[asd_corner_index(m, l, q, c)];
        const float ga = gs[(2 * l) * 256], gb = gs[(2 * l + 1) * 256];
        float dx = 0.f, dy = 0.f, dz = 0.f;
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            float wt, ex, ey, ez;
            asd_corner_weight_grad(q, c, wt, ex, ey, ez);
            const float gv = fmaf(ga, v[c].x, gb * v[c].y);
            dx = fmaf(ex, gv, dx); dy = fmaf(ey, gv, dy); dz = fmaf(ez, gv, dz);
        }
        gu[0] = fmaf(q.s, dx, gu[0]); gu[1] = fmaf(q.s, dy, gu[1]); gu[2] = fmaf(q.s, dz, gu[2]);
    }
}

// t_j = sum_k gh_k D[j][k]  (gh_k = c_k Gh_k), written to this thread's LDS column ts
template <int L>
__device__ __forceinline__ void an_pos_grad_t(const asd_grid_meta& m, const float* __restrict__ params, float x, float y, float z,
                                              float gh0, float gh1, float gh2, float* ts) {
#pragma unroll 2
    for (int l = 0; l < L; ++l) {
        const asd_cell q = asd_cell_of(m, l, x, y, z);
        const float2* __restrict__ tab = reinterpret_cast<const float2*>(params) + m.offset[l];
        float2 v[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) v[c] = tab[asd_corner_index(m, l, q, c)];
        float t0 = 0.f, t1 = 0.f;
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            float wt, ex, ey, ez;
            asd_corner_weight_grad(q, c, wt, ex, ey, ez);
            const float dwt = q.s * fmaf(gh0, ex, fmaf(gh1, ey, gh2 * ez));
            t0 = fmaf(dwt, v[c].x, t0);
            t1 = fmaf(dwt, v[c].y, t1);
        }
        ts[(2 * l) * 256] = t0; ts[(2 * l + 1) * 256] = t1;
    }
}

// ---------------------------------------------------------------------------------------------------
// forward: sigma, features, grad, normal; saves the centre encoding
// ---------------------------------------------------------------------------------------------------
template <int L, int H, int C>
__global__ __launch_bounds__(256, 4) void field_analytic_fwd_kernel(const asd_grid_meta m, const asd_field_cfg c, const float* __restrict__ grid,
                                                                    const float* __restrict__ w1d, const float* __restrict__ w2d,
                                                                    const float* __restrict__ w1f, const float* __restrict__ w2f,
                                                                    const float* __restrict__ points, int n, float* __restrict__ sigma,
                                                                    float* __restrict__ features, float* __restrict__ grad,
                                                                    float* __restrict__ normal, float* __restrict__ enc_save) {
    constexpr int NIN = 2 * L;
    __shared__ float g_s[NIN * 256];     // [k][thread]: each thread reads and writes its own column only (no barrier)
    float* const gs = g_s + threadIdx.x;
    const float sign = c.field_mode == ASD_FIELD_SDF ? 1.f : -1.f;
    const float bx = c.bbox_max[0] - c.bbox_min[0], by = c.bbox_max[1] - c.bbox_min[1], bz = c.bbox_max[2] - c.bbox_min[2];
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
        const float px = points[3 * (size_t)i], py = points[3 * (size_t)i + 1], pz = points[3 * (size_t)i + 2];
        const float ux = (px - c.bbox_min[0]) / bx, uy = (py - c.bbox_min[1]) / by, uz = (pz - c.bbox_min[2]) / bz;
        float enc[NIN], g[NIN];
        asd_encode<L, false>(m, grid, ux, uy, uz, enc);
        const float raw = an_mlp1_g<NIN, H>(w1d, w2d, enc, g) + field_bias(c, px, py, pz);
        sigma[i] = field_act(c, raw);
        if (enc_save) asd_row_store(enc_save + (size_t)i * NIN, enc);
        if (C > 0 && features) {
            float f[C > 0 ? C : 1];
            mlpC<NIN, H, (C > 0 ? C : 1)>(w1f, w2f, enc, f);
#pragma unroll
            for (int o = 0; o < C; ++o) features[(size_t)i * C + o] = f[o];
        }
        float gu[3], db[3];
#pragma unroll
        for (int k = 0; k < NIN; ++k) gs[k * 256] = g[k];
        an_pos_grad<L>(m, grid, an_again(asd_unit(ux)), an_again(asd_unit(uy)), an_again(asd_unit(uz)), gs, gu);
        an_bias_grad(c, px, py, pz, db);
        const float ap = field_act_grad(c, raw);
        const float g0 = ap * ((ux >= 0.f && ux <= 1.f ? gu[0] / bx : 0.f) + db[0]);
        const float g1 = ap * ((uy >= 0.f && uy <= 1.f ? gu[1] / by : 0.f) + db[1]);
        const float g2 = ap * ((uz >= 0.f && uz <= 1.f ? gu[2] / bz : 0.f) + db[2]);
        if (grad) {
            grad[3 * (size_t)i] = g0; grad[3 * (size_t)i + 1] = g1; grad[3 * (size_t)i + 2] = g2;
        }
        const float inv = sign / fmaxf(sqrtf(g0 * g0 + g1 * g1 + g2 * g2), 1e-12f);
        normal[3 * (size_t)i] = g0 * inv; normal[3 * (size_t)i + 1] = g1 * inv; normal[3 * (size_t)i + 2] = g2 * inv;
    }
}

// ---------------------------------------------------------------------------------------------------
// backward, sample pass: one thread per sample.  Leaves the rows of the fixed-order first-layer reduction
//   row i     : (DA = [draw m w2 | feature hidden gradient], ENC = enc_i)       the value path
//   row n + i : (DA = [m w2 | 0],                            ENC = t_i)         the second-order term of dW1
// the per-block second-layer sums w2part[block][AN_W2N] (summed by slab_reduce_kernel), and for the scatter pass the rows
// denc_i (ordinary encoding gradient), g_i and gh_i = c Gh.
// ---------------------------------------------------------------------------------------------------
template <int L, int H, int C>
__global__ __launch_bounds__(256, 2) void field_analytic_bwd_sample_kernel(
    const asd_grid_meta m, const asd_field_cfg c, const float* __restrict__ grid, const float* __restrict__ w1d, const float* __restrict__ w2d,
    const float* __restrict__ w1f, const float* __restrict__ w2f, const float* __restrict__ points, const float* __restrict__ enc_save, int n,
    const float* __restrict__ d_sigma, const float* __restrict__ d_features, const float* __restrict__ d_normal, const float* __restrict__ d_grad,
    float* __restrict__ da /*[2n, 2H]*/, float* __restrict__ t_out /*[n, 2L]*/, float* __restrict__ denc_out /*[n, 2L]*/,
    float* __restrict__ g_out /*[n, 2L]*/, float* __restrict__ gh_out /*[n, 4]*/, float* __restrict__ w2part /*[blocks, AN_W2N]*/) {
    constexpr int NIN = 2 * L, W2S = AN_W2N + 1;
    static_assert(H + 3 * H == AN_W2N && (C == 0 || C == 3), "second-layer sums: 64 + 3 x 64");
    __shared__ float w2_acc[AN_W2_COPIES * W2S];
    __shared__ float g_s[NIN * 256];     // [k][thread]: g for the first gather pass, then t; a thread touches its own column only
    const int tid = threadIdx.x;
    float* const gs = g_s + tid;
    const int w2c = (tid >> 4) * W2S;
    const bool row_last = (tid & 15) == 15;
    for (int q = tid; q < AN_W2_COPIES * W2S; q += 256) w2_acc[q] = 0.f;
    __syncthreads();
    const int i = blockIdx.x * 256 + tid;
    const bool active = i < n;
    const bool second = d_normal || d_grad;      // uniform: without it only the value path runs
    const float sign = c.field_mode == ASD_FIELD_SDF ? 1.f : -1.f;
    const float bx = c.bbox_max[0] - c.bbox_min[0], by = c.bbox_max[1] - c.bbox_min[1], bz = c.bbox_max[2] - c.bbox_min[2];
    float px = 0.f, py = 0.f, pz = 0.f, ds = 0.f;
    float enc[NIN];
#pragma unroll
    for (int k = 0; k < NIN; ++k) enc[k] = 0.f;
    const float* const enc_row = enc_save + (size_t)(active ? i : 0) * NIN;
    if (active) {
        px = points[3 * (size_t)i]; py = points[3 * (size_t)i + 1]; pz = points[3 * (size_t)i + 2];
        ds = d_sigma ? d_sigma[i] : 0.f;
        asd_row_load(enc_row, enc);
    }
    const float ux = (px - c.bbox_min[0]) / bx, uy = (py - c.bbox_min[1]) / by, uz = (pz - c.bbox_min[2]) / bz;
    float* const da_row = da + (size_t)(active ? i : 0) * (2 * H);
    float* const da_row2 = da + ((size_t)n + (active ? i : 0)) * (2 * H);

    // ---- feature MLP: its ordinary backward -------------------------------------------------------------------------
    float dencf[NIN];
#pragma unroll
    for (int k = 0; k < NIN; ++k) dencf[k] = 0.f;
    {
        float df[3];
#pragma unroll
        for (int o = 0; o < 3; ++o) df[o] = (C > 0 && active && d_features) ? d_features[(size_t)i * 3 + o] : 0.f;
#pragma unroll 1
        for (int h0 = 0; h0 < H; h0 += 4) {
            float dav[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int h = h0 + j;
                float dav_j = 0.f;
                if (C > 0 && d_features) {
                    float a = 0.f;
#pragma unroll
                    for (int k = 0; k < NIN; ++k) a = fmaf(w1f[h * NIN + k], enc[k], a);
                    const float hv = fmaxf(a, 0.f);
                    float dh = 0.f;
#pragma unroll
                    for (int o = 0; o < 3; ++o) {
                        dh = fmaf(df[o], w2f[o * H + h], dh);
                        const float v = asd_row_sum15(df[o] * hv);
                        if (row_last) w2_acc[w2c + H + o * H + h] += v;
                    }
                    dav_j = a > 0.f ? dh : 0.f;
#pragma unroll
                    for (int k = 0; k < NIN; ++k) dencf[k] = fmaf(dav_j, w1f[h * NIN + k], dencf[k]);
                }
                dav[j] = dav_j;
            }
            if (active) {
                *reinterpret_cast<float4*>(da_row + H + h0) = make_float4(dav[0], dav[1], dav[2], dav[3]);
                if (second) *reinterpret_cast<float4*>(da_row2 + H + h0) = make_float4(0.f, 0.f, 0.f, 0.f);
            }
        }
    }

    // ---- density MLP: raw, g ----------------------------------------------------------------------------------------
    float g[NIN];
    const float raw = an_mlp1_g<NIN, H>(w1d, w2d, enc, g) + field_bias(c, px, py, pz);

    // ---- position gradient again, G = dL/dgrad, dL/draw ---------------------------------------------------------------
    const float ap = field_act_grad(c, raw);
    float draw = ds * ap;
    float gh0 = 0.f, gh1 = 0.f, gh2 = 0.f;
    const float x = asd_unit(ux), y = asd_unit(uy), z = asd_unit(uz);
    if (second) {
        float gu[3], db[3];
#pragma unroll
        for (int k = 0; k < NIN; ++k) gs[k * 256] = g[k];
        an_pos_grad<L>(m, grid, x, y, z, gs, gu);
        an_bias_grad(c, px, py, pz, db);
        const float c0 = ux >= 0.f && ux <= 1.f ? 1.f / bx : 0.f, c1 = uy >= 0.f && uy <= 1.f ? 1.f / by : 0.f,
                    c2 = uz >= 0.f && uz <= 1.f ? 1.f / bz : 0.f;
        const float graw0 = c0 * gu[0] + db[0], graw1 = c1 * gu[1] + db[1], graw2 = c2 * gu[2] + db[2];
        float G0 = 0.f, G1 = 0.f, G2 = 0.f;
        if (d_normal && active) {
            const float d0 = d_normal[3 * (size_t)i], d1 = d_normal[3 * (size_t)i + 1], d2 = d_normal[3 * (size_t)i + 2];
            const float r0 = ap * graw0, r1 = ap * graw1, r2 = ap * graw2;
            const float len = sqrtf(r0 * r0 + r1 * r1 + r2 * r2);
            if (len > 1e-12f) {
                const float inv = 1.f / len;
                const float n0 = r0 * inv, n1 = r1 * inv, n2 = r2 * inv;
                const float dot = n0 * d0 + n1 * d1 + n2 * d2;
                G0 = sign * (d0 - n0 * dot) * inv; G1 = sign * (d1 - n1 * dot) * inv; G2 = sign * (d2 - n2 * dot) * inv;
            } else {
                G0 = sign * d0 * 1e12f; G1 = sign * d1 * 1e12f; G2 = sign * d2 * 1e12f;
            }
        }
        if (d_grad && active) {
            G0 += d_grad[3 * (size_t)i]; G1 += d_grad[3 * (size_t)i + 1]; G2 += d_grad[3 * (size_t)i + 2];
        }
        draw = fmaf(an_act_grad2(c, raw), G0 * graw0 + G1 * graw1 + G2 * graw2, draw);
        gh0 = c0 * (ap * G0); gh1 = c1 * (ap * G1); gh2 = c2 * (ap * G2);
    }

    // ---- rows of the scatter pass -----------------------------------------------------------------------------------------
    if (active) {
        float4* dd = reinterpret_cast<float4*>(denc_out + (size_t)i * NIN);
        float4* dg = reinterpret_cast<float4*>(g_out + (size_t)i * NIN);
#pragma unroll
        for (int q = 0; q < NIN / 4; ++q) {
            dd[q] = make_float4(fmaf(draw, g[4 * q], dencf[4 * q]), fmaf(draw, g[4 * q + 1], dencf[4 * q + 1]),
                                fmaf(draw, g[4 * q + 2], dencf[4 * q + 2]), fmaf(draw, g[4 * q + 3], dencf[4 * q + 3]));
            dg[q] = make_float4(g[4 * q], g[4 * q + 1], g[4 * q + 2], g[4 * q + 3]);
        }
        *reinterpret_cast<float4*>(gh_out + 4 * (size_t)i) = make_float4(gh0, gh1, gh2, 0.f);
    }

    // ---- t = D (c Gh): the input of the second-order rows --------------------------------------------------------------------
    float t[NIN];
#pragma unroll
    for (int k = 0; k < NIN; ++k) t[k] = 0.f;
    if (second) {
        an_pos_grad_t<L>(m, grid, an_again(x), an_again(y), an_again(z), gh0, gh1, gh2, gs);
#pragma unroll
        for (int k = 0; k < NIN; ++k) t[k] = gs[k * 256];
        if (active) asd_row_store(t_out + (size_t)i * NIN, t);
    }

    // ---- density MLP hidden gradients: both rows, and dw2_h = sum_i draw relu(a_h) + m_h (W1 t)_h -------------------------------
    if (active) asd_row_load(enc_row, enc);
#pragma unroll 1
    for (int h0 = 0; h0 < H; h0 += 4) {
        float dav[4], dav2[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int h = h0 + j;
            float a = 0.f, wt = 0.f;
#pragma unroll
            for (int k = 0; k < NIN; ++k) {
                a = fmaf(w1d[h * NIN + k], enc[k], a);
                wt = fmaf(w1d[h * NIN + k], t[k], wt);
            }
            const bool on = a > 0.f;       // the same a as in an_mlp1_g: the same enc, the same order
            const float v = asd_row_sum15(active ? fmaf(draw, fmaxf(a, 0.f), on ? wt : 0.f) : 0.f);
            if (row_last) w2_acc[w2c + h] += v;
            dav2[j] = on ? w2d[h] : 0.f;
            dav[j] = draw * dav2[j];
        }
        if (active) {
            *reinterpret_cast<float4*>(da_row + h0) = make_float4(dav[0], dav[1], dav[2], dav[3]);
            if (second) *reinterpret_cast<float4*>(da_row2 + h0) = make_float4(dav2[0], dav2[1], dav2[2], dav2[3]);
        }
    }
    __syncthreads();
    for (int q = tid; q < AN_W2N; q += 256) {
        float a = 0.f;
#pragma unroll
        for (int cpy = 0; cpy < AN_W2_COPIES; ++cpy) a += w2_acc[cpy * W2S + q];
        w2part[(size_t)blockIdx.x * AN_W2N + q] = a;
    }
}

// ---------------------------------------------------------------------------------------------------
// backward, scatter pass: one thread per (sample, level), level-major inside a 256-sample tile (hashgrid_bwd_kernel's order: one
// level's table stays hot per wave), plain fp32 atomics.  Entry of corner c += wt_c denc + dwt_c g.
// ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void field_analytic_scatter_kernel(const asd_grid_meta m, const asd_field_cfg c,
                                                                     const float* __restrict__ points, const float* __restrict__ denc,
                                                                     const float* __restrict__ g, const float* __restrict__ gh, int n,
                                                                     float* __restrict__ d_grid) {
    const int L = (int)m.n_levels;
    const int64_t total = (int64_t)((n + 255) / 256) * 256 * L;
    for (int64_t tt = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; tt < total; tt += (int64_t)gridDim.x * blockDim.x) {
        int64_t i;
        int l;
        asd_point_level(tt, L, i, l);
        if (i >= n) continue;
        const float2 de = reinterpret_cast<const float2*>(denc)[i * L + l];
        const float2 gg = reinterpret_cast<const float2*>(g)[i * L + l];
        const float4 h = reinterpret_cast<const float4*>(gh)[i];
        const bool second = (h.x != 0.f || h.y != 0.f || h.z != 0.f) && (gg.x != 0.f || gg.y != 0.f);
        if (de.x == 0.f && de.y == 0.f && !second) continue;
        const float x = asd_unit((points[3 * i] - c.bbox_min[0]) / (c.bbox_max[0] - c.bbox_min[0]));
        const float y = asd_unit((points[3 * i + 1] - c.bbox_min[1]) / (c.bbox_max[1] - c.bbox_min[1]));
        const float z = asd_unit((points[3 * i + 2] - c.bbox_min[2]) / (c.bbox_max[2] - c.bbox_min[2]));
        const asd_cell q = asd_cell_of(m, l, x, y, z);
        float* __restrict__ tab = d_grid + 2u * (size_t)m.offset[l];
#pragma unroll
        for (int cn = 0; cn < 8; ++cn) {
            float wt, ex, ey, ez;
            asd_corner_weight_grad(q, cn, wt, ex, ey, ez);
            const float dwt = q.s * fmaf(h.x, ex, fmaf(h.y, ey, h.z * ez));
            const uint32_t idx = asd_corner_index(m, l, q, cn);
            atomicAdd(tab + 2u * (size_t)idx, fmaf(dwt, gg.x, wt * de.x));
            atomicAdd(tab + 2u * (size_t)idx + 1, fmaf(dwt, gg.y, wt * de.y));
        }
    }
}

// ---------------------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------------------
// The workspace of asd_field_analytic_bwd, in floats from its start: the size query returns `total`, the pass takes every pointer from here.
struct analytic_bwd_layout {
    int n_slabs;        // slabs reserved = blocks of field_wgrad_kernel over the 2 n rows
    int n_blocks;       // blocks of the sample pass = rows of w2part
    int64_t da;         // [2 n][128] hidden-layer gradients: value rows, then the second-order rows
    int64_t t;          // [n][32] inputs of the second-order rows
    int64_t slabs;      // [n_slabs][128][32]
    int64_t denc, g;    // [n][32] each: rows of the scatter pass
    int64_t gh;         // [n][4]
    int64_t w2part;     // [n_blocks][AN_W2N]
    int64_t total;
};
static analytic_bwd_layout analytic_bwd_layout_init(int64_t n) {
    analytic_bwd_layout L;
    asd_ws_cursor w;
    L.n_slabs = asd_field_wgrad_chunks(2 * n);
    L.n_blocks = asd_div_up(n, 256);
    L.da = w.take(2 * n * 128);
    L.t = w.take(n * 32);
    L.slabs = w.take((int64_t)L.n_slabs * 128 * 32);
    L.denc = w.take(n * 32);
    L.g = w.take(n * 32);
    L.gh = w.take(n * 4);
    L.w2part = w.take((int64_t)L.n_blocks * AN_W2N);
    L.total = w.o;
    return L;
}

extern "C" {

int asd_field_analytic_fwd(const asd_grid_meta* meta, const asd_field_cfg* cfg, const float* grid_params, const float* w1_density,
                           const float* w2_density, const float* w1_feature, const float* w2_feature, const float* points, int32_t n,
                           float* sigma, float* features, float* grad, float* normal, float* enc_save, void* stream) {
    if (n == 0) return ASD_OK;
    ASD_CHECK_ARG(meta && cfg && grid_params && w1_density && w2_density && points && sigma && normal && n > 0, "null argument");
    if (!asd_field_supported(meta, cfg, "analytic field")) return ASD_ERR_UNSUPPORTED;
    if (meta->n_masked_levels != 0) {
        asd_set_error("analytic field kernels take no level limit (n_masked_levels = %u): the position gradient of a progressive grid is not "
                      "implemented, use finite-difference normals", meta->n_masked_levels);
        return ASD_ERR_UNSUPPORTED;
    }
    ASD_CHECK_ARG(cfg->n_feature_dims == 0 || !features || (w1_feature && w2_feature), "feature weights missing");
    hipLaunchKernelGGL((field_analytic_fwd_kernel<16, 64, 3>), dim3(asd_grid_for(n, 256)), dim3(256), 0, (hipStream_t)stream, *meta, *cfg,
                       grid_params, w1_density, w2_density, w1_feature, w2_feature, points, n, sigma,
                       cfg->n_feature_dims == 3 ? features : nullptr, grad, normal, enc_save);
    ASD_LAUNCH_CHECK();
    return ASD_OK;
}

int asd_field_analytic_bwd_workspace(const asd_field_cfg* cfg, int32_t n, int64_t* n_floats) {
    ASD_CHECK_ARG(cfg && n_floats && n >= 0, "bad argument");
    *n_floats = analytic_bwd_layout_init(n).total;
    return ASD_OK;
}

int asd_field_analytic_bwd(const asd_grid_meta* meta, const asd_field_cfg* cfg, const float* grid_params, const float* w1_density,
                           const float* w2_density, const float* w1_feature, const float* w2_feature, const float* points,
                           const float* enc_save, const float* sigma, int32_t n, const float* d_sigma, const float* d_features,
                           const float* d_normal, const float* d_grad, float* d_grid_params, float* dw1_density, float* dw2_density,
                           float* dw1_feature, float* dw2_feature, float* workspace, void* stream) {
    if (n == 0) return ASD_OK;
    ASD_CHECK_ARG(meta && cfg && grid_params && w1_density && w2_density && points && enc_save && sigma && d_grid_params && dw1_density &&
                      dw2_density && workspace && n > 0,
                  "null argument");
    if (!asd_field_supported(meta, cfg, "analytic field")) return ASD_ERR_UNSUPPORTED;
    if (meta->n_masked_levels != 0) {
        asd_set_error("analytic field kernels take no level limit (n_masked_levels = %u): the position gradient of a progressive grid is not "
                      "implemented, use finite-difference normals", meta->n_masked_levels);
        return ASD_ERR_UNSUPPORTED;
    }
    ASD_CHECK_ARG(cfg->n_feature_dims == 3 || !d_features, "d_features given but no feature network");
    ASD_CHECK_ARG(cfg->n_feature_dims == 0 || (dw1_feature && dw2_feature && w1_feature && w2_feature), "feature gradients missing");
    hipStream_t s = (hipStream_t)stream;
    const analytic_bwd_layout L = analytic_bwd_layout_init(n);
    float *const da = workspace + L.da, *const t = workspace + L.t, *const slabs = workspace + L.slabs, *const denc = workspace + L.denc,
          *const g = workspace + L.g, *const gh = workspace + L.gh, *const w2part = workspace + L.w2part;
    const bool second = d_normal || d_grad;
    const int rows = second ? 2 * n : n;        // without a normal gradient the second-order rows are neither written nor read
    const int n_slabs = asd_field_wgrad_chunks(rows);
    ASD_CHECK_ARG(n_slabs <= L.n_slabs, "more weight-gradient slabs than the workspace reserves");
    const dim3 grid(L.n_blocks), block(256);
#define ASD_ANALYTIC_BWD_LAUNCH(C_)                                                                                                          \
    hipLaunchKernelGGL((field_analytic_bwd_sample_kernel<16, 64, C_>), grid, block, 0, s, *meta, *cfg, grid_params, w1_density, w2_density, \
                       w1_feature, w2_feature, points, enc_save, n, d_sigma, d_features, d_normal, d_grad, da, t, denc, g, gh, w2part)
    if (cfg->n_feature_dims == 3) ASD_ANALYTIC_BWD_LAUNCH(3); else ASD_ANALYTIC_BWD_LAUNCH(0);
#undef ASD_ANALYTIC_BWD_LAUNCH
    hipLaunchKernelGGL(field_analytic_scatter_kernel, dim3(asd_point_level_grid(n, (int)meta->n_levels)), block, 0, s, *meta, *cfg, points, denc, g, gh, n,
                       d_grid_params);
    asd_field_wgrad_tail(da, enc_save, t, n, rows, nullptr, false, slabs, n_slabs, dw1_density, cfg->n_feature_dims == 3 ? dw1_feature : nullptr, s);
    // w2part rows [64 density | 3 x 64 feature]
    asd_field_slab_reduce_launch(w2part, L.n_blocks, AN_W2N, 64, dw2_density, s);
    if (cfg->n_feature_dims == 3) asd_field_slab_reduce_launch(w2part + 64, L.n_blocks, AN_W2N, 3 * 64, dw2_feature, s);
    ASD_LAUNCH_CHECK();
    return ASD_OK;
}

}  // extern "C"
