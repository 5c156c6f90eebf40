// field.hip — hash-grid encode + tiny-MLP field kernels for gfx950 (wave64, one thread per point).
//
// Replaces, behind the C ABI of include/asd_hip.h:
//   tcnn.Encoding forward/backward          (reference threestudio/models/networks.py:55-64)
//   ImplicitVolume.forward/forward_density  (threestudio/models/geometry/implicit_volume.py:109-207)
//   NeuralEnvironmentMapBackground.forward  (threestudio/models/background/neural_environment_map_background.py:46-67)
//
// Roofline: HBM/L2 gather bound — 16 levels x 8 corners x 8 B = 1024 B gathered per encode
// (SURVEY.md §8d); the MLPs (2112 / 2240 MAC per point) run on the VALU with the weights read through
// the scalar cache (uniform addresses -> s_load), so no LDS or VGPR is spent on weights.
// Level limit (asd_grid_meta.n_masked_levels, ProgressiveBandHashGrid networks.py:129-167): 64 B x active levels per encode — the masked
// levels' gathers, finite-difference re-encodes, atomics and paged items are skipped, their outputs are exact zeros.
#include <stdarg.h>
#include <stdio.h>
#include <string.h>
#include <math.h>

#include "asd_common.h"
#include "field_paged.h"
#include "field_math.h"


// ---------------------------------------------------------------------------------------------------
// generic tcnn.Encoding forward / backward: one thread per (point, level)
// ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void hashgrid_fwd_kernel(const asd_grid_meta m, const float* __restrict__ params,
                                                           const float* __restrict__ x, int n,
                                                           float* __restrict__ out) {
    const int L = (int)m.n_levels;
    const int64_t total = (int64_t)((n + 255) / 256) * 256 * L;  // whole 256-point tiles, level-major inside
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
        int64_t i;
        int l;
        asd_point_level(t, L, i, l);
        if (i >= n) continue;
        if (l >= asd_active_levels(m)) {       // level limit: a wave is on one level, so the compare is uniform
            reinterpret_cast<float2*>(out)[i * L + l] = make_float2(0.f, 0.f);
            continue;
        }
        const float s = m.scale[l];
        const asd_cell q = asd_cell_at(s, asd_unit(x[3 * i]), asd_unit(x[3 * i + 1]), asd_unit(x[3 * i + 2]));
        const float2* __restrict__ tab = reinterpret_cast<const float2*>(params) + m.offset[l];
        float2 v[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) v[c] = tab[asd_corner_index(m, l, q, c)];
        float f0 = 0.f, f1 = 0.f;
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const float wt = asd_corner_weight(q, c);
            f0 = fmaf(wt, v[c].x, f0);
            f1 = fmaf(wt, v[c].y, f1);
        }
        reinterpret_cast<float2*>(out)[i * L + l] = make_float2(f0, f1);
    }
}

__global__ __launch_bounds__(256) void hashgrid_bwd_kernel(const asd_grid_meta m, const float* __restrict__ x,
                                                           const float* __restrict__ dout, int n,
                                                           float* __restrict__ dparams) {
    const int L = (int)m.n_levels;
    const int64_t total = (int64_t)((n + 255) / 256) * 256 * L;  // whole 256-point tiles, level-major inside
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
        int64_t i;
        int l;
        asd_point_level(t, L, i, l);
        if (i >= n || l >= asd_active_levels(m)) continue;       // level limit: dout of a masked level is ignored
        const float2 g = reinterpret_cast<const float2*>(dout)[i * L + l];
        if (g.x == 0.f && g.y == 0.f) continue;
        const float s = m.scale[l];
        const asd_cell q = asd_cell_at(s, asd_unit(x[3 * i]), asd_unit(x[3 * i + 1]), asd_unit(x[3 * i + 2]));
        float* __restrict__ tab = dparams + 2u * (size_t)m.offset[l];
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const float wt = asd_corner_weight(q, c);
            const uint32_t idx = asd_corner_index(m, l, q, c);
            atomicAdd(tab + 2u * (size_t)idx, wt * g.x);
            atomicAdd(tab + 2u * (size_t)idx + 1, wt * g.y);
        }
    }
}

// ---------------------------------------------------------------------------------------------------
// field helpers
// ---------------------------------------------------------------------------------------------------
// field_bias, field_act, field_act_grad, mlp1, mlpC: field_math.h (shared with field_analytic.hip)

// ENC = 1: the "encoding" of a point is the trilinear sample of a channel-last feature volume [D][H][W][2 L] — the generator-backed
// geometries (3DConv-net: get_trilinear_feature = F.grid_sample(bilinear, zeros, align_corners = False),
// custom/amortized/models/geometry/utils.py:95-110) — instead of the hash grid; m.resolution[0..2] = W, H, D; (x, y, z) in [0, 1] are
// mapped to grid_sample's [-1, 1] (x -> W, y -> H, z -> D).  Everything behind the encoding (MLP heads, bias, finite differences) is shared.
__device__ __forceinline__ void vox_axis(float x01, int size, int& i0, float& w1) {
    const float ix = (((2.f * x01 - 1.f) + 1.f) * (float)size - 1.f) * 0.5f;   // align_corners = False
    const float f = floorf(ix);
    i0 = (int)f;
    w1 = ix - f;
}
template <int NC>
__device__ __forceinline__ void vox_encode(const asd_grid_meta& m, const float* __restrict__ vox, float x, float y, float z, float (&enc)[NC]) {
    const int W = (int)m.resolution[0], Hh = (int)m.resolution[1], D = (int)m.resolution[2];
    int x0, y0, z0;
    float fx, fy, fz;
    vox_axis(x, W, x0, fx); vox_axis(y, Hh, y0, fy); vox_axis(z, D, z0, fz);
#pragma unroll
    for (int k = 0; k < NC; ++k) enc[k] = 0.f;
#pragma unroll
    for (int corner = 0; corner < 8; ++corner) {
        const int dx = corner & 1, dy = (corner >> 1) & 1, dz = corner >> 2;
        const int xi = x0 + dx, yi = y0 + dy, zi = z0 + dz;
        if (xi < 0 || xi >= W || yi < 0 || yi >= Hh || zi < 0 || zi >= D) continue;
        const float w = (dx ? fx : 1.f - fx) * (dy ? fy : 1.f - fy) * (dz ? fz : 1.f - fz);
        const float4* row = reinterpret_cast<const float4*>(vox + (((size_t)zi * Hh + yi) * W + xi) * NC);
#pragma unroll
        for (int q = 0; q < NC / 4; ++q) {
            const float4 v = row[q];
            enc[4 * q] = fmaf(w, v.x, enc[4 * q]); enc[4 * q + 1] = fmaf(w, v.y, enc[4 * q + 1]);
            enc[4 * q + 2] = fmaf(w, v.z, enc[4 * q + 2]); enc[4 * q + 3] = fmaf(w, v.w, enc[4 * q + 3]);
        }
    }
}

template <int L, int H, int ENC = 0, bool LIMITED = true>
__device__ __forceinline__ float field_raw(const asd_grid_meta& m, const asd_field_cfg& c,
                                           const float* __restrict__ grid, const float* __restrict__ w1d,
                                           const float* __restrict__ w2d, float px, float py, float pz,
                                           float (&enc)[2 * L]) {
    const float x = (px - c.bbox_min[0]) / (c.bbox_max[0] - c.bbox_min[0]);
    const float y = (py - c.bbox_min[1]) / (c.bbox_max[1] - c.bbox_min[1]);
    const float z = (pz - c.bbox_min[2]) / (c.bbox_max[2] - c.bbox_min[2]);
    if constexpr (ENC == 1) vox_encode<2 * L>(m, grid, x, y, z, enc);
    else asd_encode<L, LIMITED>(m, grid, x, y, z, enc);
    return mlp1<2 * L, H>(w1d, w2d, enc) + field_bias(c, px, py, pz);
}

// ---------------------------------------------------------------------------------------------------
// sigma only (marcher sigma_fn, occupancy update)
// ---------------------------------------------------------------------------------------------------
// LIMITED: the meta carries a level limit.  Two instantiations, chosen by the host: on a plain grid the kernel is the one without the
// per-level compares, which cost it registers (71 -> 78 VGPRs, 7 -> 6 waves per SIMD) and 2 % of its time on an MI355X
template <int L, int H, bool LIMITED>
__global__ __launch_bounds__(256, 4) void field_density_kernel(const asd_grid_meta m, const asd_field_cfg c,
                                                            const float* __restrict__ grid,
                                                            const float* __restrict__ w1d,
                                                            const float* __restrict__ w2d,
                                                            const float* __restrict__ points, int n,
                                                            const int* __restrict__ n_dev,
                                                            float* __restrict__ sigma) {
    const int nn = n_dev ? min(*n_dev, n) : n;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < nn; i += gridDim.x * 256) {
        float enc[2 * L];
        const float raw = field_raw<L, H, 0, LIMITED>(m, c, grid, w1d, w2d, points[3 * i], points[3 * i + 1], points[3 * i + 2], enc);
        sigma[i] = field_act(c, raw);
    }
}

// ---------------------------------------------------------------------------------------------------
// training forward: sigma, features, finite-difference normal; saves the centre encoding
// ---------------------------------------------------------------------------------------------------
template <int L, int H, int C, int ENC = 0>
__global__ __launch_bounds__(256, 4) void field_fwd_kernel(const asd_grid_meta m, const asd_field_cfg c,
                                                        const float* __restrict__ grid,
                                                        const float* __restrict__ w1d, const float* __restrict__ w2d,
                                                        const float* __restrict__ w1f, const float* __restrict__ w2f,
                                                        const float* __restrict__ points, int n,
                                                        const int* __restrict__ n_dev, float* __restrict__ sigma,
                                                        float* __restrict__ features, float* __restrict__ normal,
                                                        float* __restrict__ fd_grad, float* __restrict__ enc_save) {
    const float fd_sign = c.field_mode == ASD_FIELD_SDF ? 1.f : -1.f;
    const int nn = n_dev ? min(*n_dev, n) : n;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < nn; i += gridDim.x * 256) {
        const float px = points[3 * i], py = points[3 * i + 1], pz = points[3 * i + 2];
        float enc[2 * L];
        const float raw = field_raw<L, H, ENC>(m, c, grid, w1d, w2d, px, py, pz, enc);
        const float s = field_act(c, raw);
        sigma[i] = s;
        if (enc_save) asd_row_store(enc_save + (size_t)i * 2 * L, enc);
        if (features) {
            float f[C];
            mlpC<2 * L, H, C>(w1f, w2f, enc, f);
#pragma unroll
            for (int o = 0; o < C; ++o) features[(size_t)i * C + o] = f[o];
        }
        if (normal || fd_grad) {
            float nr[3];
#pragma unroll 1
            for (int k = 0; k < 3; ++k) {
                const float qx = asd_clampf(px + (k == 0 ? c.fd_eps : 0.f), -c.radius, c.radius);
                const float qy = asd_clampf(py + (k == 1 ? c.fd_eps : 0.f), -c.radius, c.radius);
                const float qz = asd_clampf(pz + (k == 2 ? c.fd_eps : 0.f), -c.radius, c.radius);
                float e2[2 * L];
                const float sk = field_act(c, field_raw<L, H, ENC>(m, c, grid, w1d, w2d, qx, qy, qz, e2));
                nr[k] = fd_sign * (sk - s) / c.fd_eps;
            }
            if (fd_grad) {
                fd_grad[3 * (size_t)i] = nr[0];
                fd_grad[3 * (size_t)i + 1] = nr[1];
                fd_grad[3 * (size_t)i + 2] = nr[2];
            }
            if (normal) {
                const float len = sqrtf(nr[0] * nr[0] + nr[1] * nr[1] + nr[2] * nr[2]);
                const float inv = 1.f / fmaxf(len, 1e-12f);
                normal[3 * (size_t)i] = nr[0] * inv;
                normal[3 * (size_t)i + 1] = nr[1] * inv;
                normal[3 * (size_t)i + 2] = nr[2] * inv;
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------
// training backward, two kernels:
//  (1) field_bwd_sample_kernel — one thread per sample (no block-level synchronisation, full occupancy):
//      re-evaluates the hidden layers from the saved encoding, forms the hidden-layer gradients
//      DA[row][0:64] (density MLP) / DA[row][64:128] (feature MLP), back-propagates to the encoding and
//      scatters into the hash-table gradient (fp32 hardware atomics); second-layer weight gradients are
//      wave-reduced and accumulated through LDS (one global atomic per block and weight).
//      With a normal gradient the 3 finite-difference points become 3 extra rows per sample.
//  (2) field_wgrad_kernel — dW1 = DA^T . ENC as a tall-skinny GEMM over the sample axis (K = rows), 4x4
//      register tiles fed by 16-byte LDS reads, one partial slab per 2048-row chunk, summed by
//      slab_reduce_kernel in a fixed order.
// DA costs 512 B/row of HBM write+read (288 GB of HBM3E: materialise instead of re-synchronising).
// ---------------------------------------------------------------------------------------------------
#define ASD_FIELD_BWD_BLOCKS 2   // blocks per CU the sample pass is compiled for (213 VGPRs; 3 was measured: see DESIGN.md)
#define ASD_FIELD_W2_COPIES 16  // second-layer weight-gradient terms are summed over each row of 16 lanes with four DPP adds and the row's
                                // last lane adds the sum to the row's OWN copy with a plain LDS read-modify-write (16 rows per block = the 16
                                // copies).  The first form had every lane issue an LDS float atomic — 256 per sample; LDS float atomics retire
                                // ~0.3 lanes per clock and CU on gfx950, which made them, not the arithmetic, the bound of this kernel (round 5).
#define ASD_FIELD_NAGG 5   // levels scattered with wave-level run aggregation (asd_scatter_runs): the dense ones.  Level 5 (102^3 cells in a 2^19-entry
                           // hashed table) was the bulk of this kernel's atomic requests (runs of ~2.5 samples); it is paged with the finer ones
#define ASD_FIELD_NPRIV 3   // levels whose gradient is accumulated in per-XCD copies first (asd_scatter_runs)
#define ASD_FIELD_PRIV_CAP (1 << 17)   // floats per copy reserved in the workspace (levels 0-2 of the 16-level grid: 106 034)
#define WG_ROWS 512    // rows per wgrad block.  2048 (rounds 1-2) gave the headline step 212 blocks of four waves for 256 CUs — one wave per
                       // SIMD with nobody to hide the LDS latency; 512: 846 blocks, three to four per CU, wgrad + slab reduction 0.24 -> 0.09 ms
                       // (same box: 1024 -> 0.13, 256 -> 0.10)
#define WG_TILE 64     // rows per LDS tile

// PRE: the MLP half already ran on the matrix pipe (csrc/field_mfma.hip: asd_field_bwd_mlp_mfma left the weight gradients and the encoding
// gradients denc_pre[n][2 L]); this kernel then only scatters — no finite-difference rows in that form, and da_out is not touched.
template <int L, int H, int C, int ENC = 0, bool PRE = false>
__global__ __launch_bounds__(256, ASD_FIELD_BWD_BLOCKS) void field_bwd_sample_kernel(
    const asd_grid_meta m, const asd_field_cfg c, const float* __restrict__ grid, const float* __restrict__ w1d,
    const float* __restrict__ w2d, const float* __restrict__ w1f, const float* __restrict__ w2f,
    const float* __restrict__ points, const float* __restrict__ enc_save, const float* __restrict__ sigma, int n,
    const int* __restrict__ n_dev, const float* __restrict__ d_sigma, const float* __restrict__ d_features,
    const float* __restrict__ d_normal, const float* __restrict__ d_fd_grad, float* __restrict__ d_grid,
    float* __restrict__ da_out /*[rows,2H]*/,
    float* __restrict__ enc_fd /*[3n, 2L] or NULL*/, float* __restrict__ dw2d, float* __restrict__ dw2f,
    float* __restrict__ priv /*[ASD_PRIV_COPIES][priv_stride] per-XCD copies of the gradient of levels < ASD_FIELD_NPRIV*/, uint32_t priv_stride,
    float* __restrict__ denc_out = nullptr /* ENC == 1: [rows', 2L] gradient w.r.t. the sampled features, row' = 4 i + pt (i with no normal) */,
    float* __restrict__ pts_out = nullptr /* ENC == 1: [rows', 3] the sampled positions in grid_sample's [-1, 1] */,
    float* __restrict__ pg_g = nullptr /* paged scatter (field_paged.h): [n_pts * n, 2 (L - NAGG)] gradient w.r.t. the fine levels' features, row = pt * n + i */,
    float* __restrict__ pg_pos = nullptr /* ... and the rows' unit-cube positions [n_pts * n, 3] */,
    const float* __restrict__ denc_pre = nullptr /* PRE: [n, 2L] */) {
    constexpr int NIN = 2 * L;
    // second-layer weight-gradient sums of the block: no wave-level reduction — each row of 16 lanes adds its sum into its own copy of the
    // accumulator (row stride W2N + 1: the 16 copies of one h sit in 16 banks), the copies are summed at the end.
    constexpr int W2N = (C > 0 ? C : 1) * H + H, W2S = W2N + 1;
    __shared__ float w2_acc[ASD_FIELD_W2_COPIES * W2S];
    static_assert(ASD_FIELD_W2_COPIES == 16, "row sums: one copy per row of 16 lanes of the 256-thread block");
    const int w2c = (threadIdx.x >> 4) * W2S;
    const bool row_last = (threadIdx.x & 15) == 15;
    const int nn = n_dev ? min(*n_dev, n) : n;
    if (n_dev && (int)blockIdx.x * 256 >= nn) return;       // capacity-sized launch (device-side count): nothing lives in this block
    const int tid = threadIdx.x;
    for (int q = tid; q < ASD_FIELD_W2_COPIES * W2S; q += 256) w2_acc[q] = 0.f;
    __syncthreads();
    const int i = blockIdx.x * 256 + tid;
    const bool active = i < nn;
    float px = 0.f, py = 0.f, pz = 0.f, s = 0.f, ds = 0.f;
    float enc[NIN];
#pragma unroll
    for (int k = 0; k < NIN; ++k) enc[k] = 0.f;
    if (active) {
        px = points[3 * i]; py = points[3 * i + 1]; pz = points[3 * i + 2];
        s = sigma[i];
        ds = d_sigma ? d_sigma[i] : 0.f;
        asd_row_load(enc_save + (size_t)i * NIN, enc);
    }
    const float bx = c.bbox_max[0] - c.bbox_min[0], by = c.bbox_max[1] - c.bbox_min[1], bz = c.bbox_max[2] - c.bbox_min[2];

    // gradient through the finite-difference normal: d sigma_k and an extra term on d sigma
    float dsk[3] = {0.f, 0.f, 0.f}, rawk[3] = {0.f, 0.f, 0.f};
    const bool with_fd = d_normal || d_fd_grad;
    const float fd_sign = c.field_mode == ASD_FIELD_SDF ? 1.f : -1.f;
    if (with_fd && active) {
        float nr[3];
#pragma unroll 1
        for (int k = 0; k < 3; ++k) {
            const float qx = asd_clampf(px + (k == 0 ? c.fd_eps : 0.f), -c.radius, c.radius);
            const float qy = asd_clampf(py + (k == 1 ? c.fd_eps : 0.f), -c.radius, c.radius);
            const float qz = asd_clampf(pz + (k == 2 ? c.fd_eps : 0.f), -c.radius, c.radius);
            float e2[NIN];
            rawk[k] = field_raw<L, H, ENC>(m, c, grid, w1d, w2d, qx, qy, qz, e2);
            nr[k] = fd_sign * (field_act(c, rawk[k]) - s) / c.fd_eps;
            // the encoding of the offset point is needed again below (its row of the weight-gradient GEMM and the back-propagation
            // through the density MLP): park it in enc_fd now instead of gathering its 128 corners a second time
            float4* dst = reinterpret_cast<float4*>(enc_fd + ((size_t)k * n + i) * NIN);
#pragma unroll
            for (int q = 0; q < NIN / 4; ++q) dst[q] = make_float4(e2[4 * q], e2[4 * q + 1], e2[4 * q + 2], e2[4 * q + 3]);
        }
        float dnr[3] = {0.f, 0.f, 0.f};
        if (d_normal) {
            const float len = sqrtf(nr[0] * nr[0] + nr[1] * nr[1] + nr[2] * nr[2]);
            const float g0 = d_normal[3 * (size_t)i], g1 = d_normal[3 * (size_t)i + 1], g2 = d_normal[3 * (size_t)i + 2];
            if (len > 1e-12f) {
                const float inv = 1.f / len;
                const float n0 = nr[0] * inv, n1 = nr[1] * inv, n2 = nr[2] * inv;
                const float dot = n0 * g0 + n1 * g1 + n2 * g2;
                dnr[0] = (g0 - n0 * dot) * inv; dnr[1] = (g1 - n1 * dot) * inv; dnr[2] = (g2 - n2 * dot) * inv;
            } else {
                dnr[0] = g0 * 1e12f; dnr[1] = g1 * 1e12f; dnr[2] = g2 * 1e12f;
            }
        }
        if (d_fd_grad) {
            dnr[0] += d_fd_grad[3 * (size_t)i]; dnr[1] += d_fd_grad[3 * (size_t)i + 1]; dnr[2] += d_fd_grad[3 * (size_t)i + 2];
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            dsk[k] = fd_sign * dnr[k] / c.fd_eps;
            ds -= fd_sign * dnr[k] / c.fd_eps;
        }
    }

    const int n_pts = with_fd ? 4 : 1;
#pragma unroll 1
    for (int pt = 0; pt < n_pts; ++pt) {
        float qx = px, qy = py, qz = pz, draw;
        float e[NIN];
        size_t row;
        if (pt == 0) {
#pragma unroll
            for (int k = 0; k < NIN; ++k) e[k] = enc[k];
            float ag;  // d sigma / d raw recovered from sigma itself (softplus: 1 - exp(-sigma))
            if (c.activation == ASD_ACT_SOFTPLUS) ag = 1.f - expf(-s);
            else if (c.activation == ASD_ACT_EXP) ag = s;
            else if (c.activation == ASD_ACT_TRUNC_EXP) ag = fminf(s, 3269017.37f /* e^15 */);
            else ag = 1.f;
            draw = ds * ag;
            row = (size_t)i;
        } else {
            const int k = pt - 1;
            qx = asd_clampf(px + (k == 0 ? c.fd_eps : 0.f), -c.radius, c.radius);
            qy = asd_clampf(py + (k == 1 ? c.fd_eps : 0.f), -c.radius, c.radius);
            qz = asd_clampf(pz + (k == 2 ? c.fd_eps : 0.f), -c.radius, c.radius);
            if (active) {       // written by this thread above
                const float4* src = reinterpret_cast<const float4*>(enc_fd + ((size_t)k * n + i) * NIN);
#pragma unroll
                for (int q = 0; q < NIN / 4; ++q) {
                    const float4 v = src[q];
                    e[4 * q] = v.x; e[4 * q + 1] = v.y; e[4 * q + 2] = v.z; e[4 * q + 3] = v.w;
                }
            } else {
#pragma unroll
                for (int q = 0; q < NIN; ++q) e[q] = 0.f;
            }
            draw = dsk[k] * field_act_grad(c, rawk[k]);
            row = (size_t)n + (size_t)k * n + i;  // FD rows live behind the n centre rows
        }
        float denc[NIN];
#pragma unroll
        for (int k = 0; k < NIN; ++k) denc[k] = 0.f;
        if constexpr (PRE) {
            if (active) asd_row_load(denc_pre + (size_t)i * NIN, denc);
        } else {
        float* da_row = da_out + row * (2 * H);
        // ---- density MLP: da_h = draw * w2[h] * [a_h > 0] ------------------------------------------------------
#pragma unroll 1
        for (int h0 = 0; h0 < H; h0 += 4) {
            float dav[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int h = h0 + j;
                float a = 0.f;
#pragma unroll
                for (int k = 0; k < NIN; ++k) a = fmaf(w1d[h * NIN + k], e[k], a);
                const float v = asd_row_sum15(active ? draw * fmaxf(a, 0.f) : 0.f);
                if (row_last) w2_acc[w2c + h] += v;
                const float da = (active && a > 0.f) ? draw * w2d[h] : 0.f;
                dav[j] = da;
#pragma unroll
                for (int k = 0; k < NIN; ++k) denc[k] = fmaf(da, w1d[h * NIN + k], denc[k]);
            }
            if (active)
                *reinterpret_cast<float4*>(da_row + h0) = make_float4(dav[0], dav[1], dav[2], dav[3]);
        }
        // ---- feature MLP (centre point only) -------------------------------------------------------------------
        if (C > 0) {
            float df[C > 0 ? C : 1];
#pragma unroll
            for (int o = 0; o < C; ++o) df[o] = (pt == 0 && active && d_features) ? d_features[(size_t)i * C + o] : 0.f;
#pragma unroll 1
            for (int h0 = 0; h0 < H; h0 += 4) {
                float dav[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int h = h0 + j;
                    float da = 0.f;
                    if (pt == 0 && d_features) {
                        float a = 0.f;
#pragma unroll
                        for (int k = 0; k < NIN; ++k) a = fmaf(w1f[h * NIN + k], e[k], a);
                        const float hv = fmaxf(a, 0.f);
                        float dh = 0.f;
#pragma unroll
                        for (int o = 0; o < C; ++o) {
                            dh = fmaf(df[o], w2f[o * H + h], dh);
                            const float v = asd_row_sum15(df[o] * hv);
                            if (row_last) w2_acc[w2c + H + o * H + h] += v;
                        }
                        da = a > 0.f ? dh : 0.f;
#pragma unroll
                        for (int k = 0; k < NIN; ++k) denc[k] = fmaf(da, w1f[h * NIN + k], denc[k]);
                    }
                    dav[j] = da;
                }
                if (active)
                    *reinterpret_cast<float4*>(da_row + H + h0) = make_float4(dav[0], dav[1], dav[2], dav[3]);
            }
        }
        }   // !PRE
        if constexpr (ENC == 0) {
            // level limit: denc of a masked level is W1^T . da, not zero — dropped here, so neither scatter nor the paged rows see it
            const int act = asd_active_levels(m);
#pragma unroll
            for (int l = 0; l < L; ++l)
                if (l >= act) { denc[2 * l] = 0.f; denc[2 * l + 1] = 0.f; }
        }
        if constexpr (ENC == 1) {
            // the scatter into the feature volume is asd_voxel_sample_bwd's (run-aggregated, request-coalesced): leave it the rows
            if (active) {
                const size_t ro = with_fd ? (size_t)4 * i + pt : (size_t)i;
                float4* dst = reinterpret_cast<float4*>(denc_out + ro * NIN);
#pragma unroll
                for (int q = 0; q < NIN / 4; ++q) dst[q] = make_float4(denc[4 * q], denc[4 * q + 1], denc[4 * q + 2], denc[4 * q + 3]);
                pts_out[3 * ro] = 2.f * ((qx - c.bbox_min[0]) / bx) - 1.f;
                pts_out[3 * ro + 1] = 2.f * ((qy - c.bbox_min[1]) / by) - 1.f;
                pts_out[3 * ro + 2] = 2.f * ((qz - c.bbox_min[2]) / bz) - 1.f;
            }
        } else {
            const float ux = (qx - c.bbox_min[0]) / bx, uy = (qy - c.bbox_min[1]) / by, uz = (qz - c.bbox_min[2]) / bz;
            if (pg_g) {
                // coarse levels as before (run-aggregated atomics, per-XCD copies); the fine levels' rows go to the paged scatter
                asd_scatter_runs<L, ASD_FIELD_NAGG, ASD_FIELD_NPRIV, false>(m, d_grid, ux, uy, uz, denc, active, priv, priv_stride);
                if (active) {
                    constexpr int NFINE = L - ASD_FIELD_NAGG;
                    const size_t rr = (size_t)pt * n + i;
                    float4* dst = reinterpret_cast<float4*>(pg_g + rr * (2 * ASD_PG_NF_PAD));
                    static_assert(NFINE == ASD_PG_NF && ASD_PG_NF_PAD >= ASD_PG_NF && ASD_PG_NF_PAD % 2 == 0, "paged levels");
                    float row[2 * ASD_PG_NF_PAD];                        // (rows of ASD_PG_NF_PAD levels: the pair behind the last level is zero)
#pragma unroll
                    for (int k = 0; k < 2 * ASD_PG_NF_PAD; ++k) row[k] = 0.f;
#pragma unroll
                    for (int k = 0; k < 2 * NFINE; ++k) row[k] = denc[2 * ASD_FIELD_NAGG + k];
#pragma unroll
                    for (int q = 0; q < ASD_PG_NF_PAD / 2; ++q) dst[q] = make_float4(row[4 * q], row[4 * q + 1], row[4 * q + 2], row[4 * q + 3]);
                    pg_pos[3 * rr] = asd_unit(ux); pg_pos[3 * rr + 1] = asd_unit(uy); pg_pos[3 * rr + 2] = asd_unit(uz);
                }
            } else {
                asd_scatter_runs<L, ASD_FIELD_NAGG, ASD_FIELD_NPRIV>(m, d_grid, ux, uy, uz, denc, active, priv, priv_stride);
            }
        }
    }
    __syncthreads();
    for (int q = tid; q < W2N; q += 256) {
        float a = 0.f;
#pragma unroll
        for (int cpy = 0; cpy < ASD_FIELD_W2_COPIES; ++cpy) a += w2_acc[cpy * W2S + q];
        w2_acc[q] = a;       // copy 0's slot q is only read by this thread
    }
    __syncthreads();
    if constexpr (PRE) return;
    for (int q = tid; q < H; q += 256) atomicAdd(&dw2d[q], w2_acc[q]);
    if (C > 0 && dw2f)
        for (int q = tid; q < C * H; q += 256) atomicAdd(&dw2f[q], w2_acc[H + q]);
}

// folds the per-XCD copies of the coarsest levels' gradient into the table: d_grid[j] += sum_x priv[x][j]  (fixed order)
__global__ __launch_bounds__(256) void asd_priv_reduce_kernel(const float* __restrict__ priv, uint32_t stride, uint32_t len,
                                                              float* __restrict__ d_grid) {
    const uint32_t j = (blockIdx.x * 256u + threadIdx.x) * 4u;
    if (j >= len) return;      // len and stride are multiples of 4 (two floats per entry, offsets of levels are multiples of 8 entries)
    float4 a = *reinterpret_cast<const float4*>(d_grid + j);
#pragma unroll
    for (int x = 0; x < ASD_PRIV_COPIES; ++x) {
        const float4 v = *reinterpret_cast<const float4*>(priv + (size_t)x * stride + j);
        a.x += v.x; a.y += v.y; a.z += v.z; a.w += v.w;
    }
    *reinterpret_cast<float4*>(d_grid + j) = a;
}

// slab[b][h][k] = sum over the block's rows of DA[row][h] * ENC[row][k]   (h < HH = 128, k < 32)
template <int HH, int NIN>
__global__ __launch_bounds__(256) void field_wgrad_kernel(const float* __restrict__ da, const float* __restrict__ enc_a,
                                                          const float* __restrict__ enc_b, int rows_a, int rows_total,
                                                          const int* __restrict__ n_dev, int n_max,
                                                          float* __restrict__ slabs) {
    static_assert(HH == 128 && NIN == 32, "tile mapping assumes a 128 x 32 output");
    __shared__ __attribute__((aligned(16))) float da_s[WG_TILE * HH];   // 32 KB
    __shared__ __attribute__((aligned(16))) float en_s[WG_TILE * NIN];  //  8 KB
    const int tid = threadIdx.x;
    const int h0 = (tid >> 3) * 4, k0 = (tid & 7) * 4;
    // live rows: with a device-side sample count the centre rows end at *n_dev (rows beyond it hold garbage)
    const int live_a = n_dev ? min(*n_dev, n_max) : rows_a;
    float acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;
    const int r_begin = blockIdx.x * WG_ROWS, r_end = min(rows_total, r_begin + WG_ROWS);
    if (r_begin >= live_a && r_end <= rows_a) {      // a chunk of dead centre rows (capacity-sized launch)
        if (rows_total == rows_a) return;            // ... whose slab slab_reduce_kernel does not read either
        float* slab0 = slabs + (size_t)blockIdx.x * HH * NIN;
#pragma unroll
        for (int i = 0; i < 4; ++i) *reinterpret_cast<float4*>(slab0 + (h0 + i) * NIN + k0) = make_float4(0.f, 0.f, 0.f, 0.f);
        return;
    }
    for (int r0 = r_begin; r0 < r_end; r0 += WG_TILE) {
        __syncthreads();
        // stage 64 rows of DA (512 B each) and ENC (128 B each), zero-filling dead rows
        for (int q = tid; q < WG_TILE * HH / 4; q += 256) {
            const int r = r0 + q / (HH / 4), cq = q % (HH / 4);
            const bool ok = r < r_end && (r < rows_a ? r < live_a : true);
            const float4 v = ok ? reinterpret_cast<const float4*>(da + (size_t)r * HH)[cq] : make_float4(0.f, 0.f, 0.f, 0.f);
            reinterpret_cast<float4*>(da_s)[q] = v;
        }
        for (int q = tid; q < WG_TILE * NIN / 4; q += 256) {
            const int r = r0 + q / (NIN / 4), cq = q % (NIN / 4);
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (r < r_end) {
                if (r < rows_a) { if (r < live_a) v = reinterpret_cast<const float4*>(enc_a + (size_t)r * NIN)[cq]; }
                else v = reinterpret_cast<const float4*>(enc_b + (size_t)(r - rows_a) * NIN)[cq];
            }
            reinterpret_cast<float4*>(en_s)[q] = v;
        }
        __syncthreads();
#pragma unroll 8
        for (int t = 0; t < WG_TILE; ++t) {
            const float4 a = *reinterpret_cast<const float4*>(da_s + t * HH + h0);
            const float4 e = *reinterpret_cast<const float4*>(en_s + t * NIN + k0);
            const float av[4] = {a.x, a.y, a.z, a.w}, ev[4] = {e.x, e.y, e.z, e.w};
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = fmaf(av[i], ev[j], acc[i][j]);
        }
    }
    float* slab = slabs + (size_t)blockIdx.x * HH * NIN;
#pragma unroll
    for (int i = 0; i < 4; ++i)
        *reinterpret_cast<float4*>(slab + (h0 + i) * NIN + k0) = make_float4(acc[i][0], acc[i][1], acc[i][2], acc[i][3]);
}

// sum the per-block slabs: out[j] += sum_b slabs[b][j]   (fixed order: reproducible).  A block owns 32 consecutive outputs x 32 slab
// lanes, four loads in flight per thread: the one-thread-per-output loop was a chain of n_blocks dependent round trips (503 us for
// the 1543 slabs of a Hyper-iNGP step, 42 us for the 211 of the headline step).
// live (optional): device-side count of the rows behind the slabs when they are all centre rows — only the slabs of live chunks are summed
__global__ __launch_bounds__(1024) void slab_reduce_kernel(const float* __restrict__ slabs, int n_blocks, int stride,
                                                           int len, float* __restrict__ out, const int* __restrict__ live = nullptr,
                                                           int rows_per_slab = 1) {
    __shared__ float part[32][33];
    if (live) n_blocks = min(n_blocks, (max(*live, 0) + rows_per_slab - 1) / rows_per_slab);
    const int jl = threadIdx.x & 31, lane = threadIdx.x >> 5;
    const int j = blockIdx.x * 32 + jl;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    if (j < len) {
        const float* src = slabs + j;
        int b = lane;
        for (; b + 96 < n_blocks; b += 128) {
            const float t0 = src[(size_t)b * stride], t1 = src[(size_t)(b + 32) * stride], t2 = src[(size_t)(b + 64) * stride],
                        t3 = src[(size_t)(b + 96) * stride];
            a0 += t0; a1 += t1; a2 += t2; a3 += t3;
        }
        for (; b < n_blocks; b += 32) a0 += src[(size_t)b * stride];
    }
    part[lane][jl] = (a0 + a1) + (a2 + a3);
    __syncthreads();
    if (lane == 0 && j < len) {
        float acc = 0.f;
#pragma unroll
        for (int l = 0; l < 32; ++l) acc += part[l][jl];
        out[j] += acc;
    }
}

// ---------------------------------------------------------------------------------------------------
// background environment map (L levels, H hidden, 2 hidden layers, 3 outputs)
// ---------------------------------------------------------------------------------------------------
template <int L, int H>
__global__ __launch_bounds__(256) void envmap_fwd_kernel(const asd_grid_meta m, const float* __restrict__ grid,
                                                         const float* __restrict__ w0, const float* __restrict__ w1,
                                                         const float* __restrict__ w2, const float* __restrict__ dirs,
                                                         int n, float* __restrict__ color) {
    constexpr int NIN = 2 * L;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
        float enc[NIN], h0[H], h1[H];
        asd_encode<L, false>(m, grid, (dirs[3 * i] + 1.f) / 2.f, (dirs[3 * i + 1] + 1.f) / 2.f, (dirs[3 * i + 2] + 1.f) / 2.f, enc);
#pragma unroll
        for (int h = 0; h < H; ++h) {
            float a = 0.f;
#pragma unroll
            for (int k = 0; k < NIN; ++k) a = fmaf(w0[h * NIN + k], enc[k], a);
            h0[h] = fmaxf(a, 0.f);
        }
#pragma unroll
        for (int h = 0; h < H; ++h) {
            float a = 0.f;
#pragma unroll
            for (int k = 0; k < H; ++k) a = fmaf(w1[h * H + k], h0[k], a);
            h1[h] = fmaxf(a, 0.f);
        }
#pragma unroll
        for (int o = 0; o < 3; ++o) {
            float a = 0.f;
#pragma unroll
            for (int k = 0; k < H; ++k) a = fmaf(w2[o * H + k], h1[k], a);
            color[3 * (size_t)i + o] = asd_sigmoid(a);
        }
    }
}

// backward: per-thread gradients, weight grads reduced per wave with shuffles then global atomics
// (n = number of rays = a few thousand: this kernel is latency-, not throughput-bound)
template <int L, int H>
__global__ __launch_bounds__(256) void envmap_bwd_kernel(const asd_grid_meta m, const float* __restrict__ grid,
                                                         const float* __restrict__ w0, const float* __restrict__ w1,
                                                         const float* __restrict__ w2, const float* __restrict__ dirs,
                                                         const float* __restrict__ d_color, int n,
                                                         float* __restrict__ d_grid, float* __restrict__ dw0,
                                                         float* __restrict__ dw1, float* __restrict__ dw2) {
    constexpr int NIN = 2 * L;
    // weight gradients: wave sums -> per-block LDS cells -> one global atomic per weight and block (64 wave leaders hammering the
    // same 432 addresses ran at the hot-address atomic rate)
    static_assert(H <= 16 && NIN <= 16, "factor rows of 17 words");
    __shared__ float w_acc[3 * H + H * H + H * NIN];
    __shared__ float xch[4 * 2 * 64 * 17];
    for (int q = threadIdx.x; q < 3 * H + H * H + H * NIN; q += 256) w_acc[q] = 0.f;
    __syncthreads();
    const int i = blockIdx.x * 256 + threadIdx.x;
    const bool active = i < n;
    float enc[NIN], a0[H], a1[H], dout[3], dh1[H], dh0[H], denc[NIN];
    float x = 0.f, y = 0.f, z = 0.f;
    if (active) {
        x = (dirs[3 * i] + 1.f) / 2.f; y = (dirs[3 * i + 1] + 1.f) / 2.f; z = (dirs[3 * i + 2] + 1.f) / 2.f;
        asd_encode<L, false>(m, grid, x, y, z, enc);
    } else {
#pragma unroll
        for (int k = 0; k < NIN; ++k) enc[k] = 0.f;
    }
#pragma unroll
    for (int h = 0; h < H; ++h) {
        float a = 0.f;
#pragma unroll
        for (int k = 0; k < NIN; ++k) a = fmaf(w0[h * NIN + k], enc[k], a);
        a0[h] = a;
    }
#pragma unroll
    for (int h = 0; h < H; ++h) {
        float a = 0.f;
#pragma unroll
        for (int k = 0; k < H; ++k) a = fmaf(w1[h * H + k], fmaxf(a0[k], 0.f), a);
        a1[h] = a;
    }
#pragma unroll
    for (int o = 0; o < 3; ++o) {
        float a = 0.f;
#pragma unroll
        for (int k = 0; k < H; ++k) a = fmaf(w2[o * H + k], fmaxf(a1[k], 0.f), a);
        const float s = asd_sigmoid(a);
        dout[o] = active ? d_color[3 * (size_t)i + o] * s * (1.f - s) : 0.f;
    }
    // Weight gradients = sums over rays of outer products.  One wave_sum per entry (432 six-step shuffle reductions, each followed by a
    // lead-lane LDS atomic) was the critical path of this 16-block launch; instead the lanes park the two factor vectors of a layer in
    // the wave's LDS rows (pitch 17 words: conflict-free) and every lane sums a few ENTRIES over the wave's 64 rays.
    float* const fa = xch + (threadIdx.x >> 6) * (2 * 64 * 17);      // [ray][17]: the gradient factor
    float* const fb = fa + 64 * 17;                                   // [ray][17]: the activation factor
    const int lane = threadIdx.x & 63;
    auto outer_sums = [&](int n_out, int n_in, float* dst) __attribute__((always_inline)) {
        __syncthreads();                                              // the factors of this layer are in place
        for (int e = lane; e < n_out * n_in; e += 64) {
            const int o = e / n_in, k = e - o * n_in;
            float acc = 0.f;
#pragma unroll 8
            for (int r = 0; r < 64; ++r) acc = fmaf(fa[r * 17 + o], fb[r * 17 + k], acc);
            atomicAdd(&dst[e], acc);                                  // the block's four waves meet here (distinct cells within a wave)
        }
        __syncthreads();                                              // before the rows are overwritten
    };
#pragma unroll
    for (int o = 0; o < 3; ++o) fa[lane * 17 + o] = dout[o];
#pragma unroll
    for (int k = 0; k < H; ++k) fb[lane * 17 + k] = fmaxf(a1[k], 0.f);
    outer_sums(3, H, w_acc);                                          // dw2[o][k]
#pragma unroll
    for (int k = 0; k < H; ++k) {
        float acc = 0.f;
#pragma unroll
        for (int o = 0; o < 3; ++o) acc = fmaf(dout[o], w2[o * H + k], acc);
        dh1[k] = a1[k] > 0.f ? acc : 0.f;
    }
#pragma unroll
    for (int k = 0; k < H; ++k) { fa[lane * 17 + k] = dh1[k]; fb[lane * 17 + k] = fmaxf(a0[k], 0.f); }
    outer_sums(H, H, w_acc + 3 * H);                                  // dw1[h][k]
#pragma unroll
    for (int k = 0; k < H; ++k) {
        float acc = 0.f;
#pragma unroll
        for (int h = 0; h < H; ++h) acc = fmaf(dh1[h], w1[h * H + k], acc);
        dh0[k] = a0[k] > 0.f ? acc : 0.f;
    }
#pragma unroll
    for (int k = 0; k < H; ++k) fa[lane * 17 + k] = dh0[k];
#pragma unroll
    for (int k = 0; k < NIN; ++k) fb[lane * 17 + k] = enc[k];
    outer_sums(H, NIN, w_acc + 3 * H + H * H);                        // dw0[h][k]
#pragma unroll
    for (int k = 0; k < NIN; ++k) {
        float acc = 0.f;
#pragma unroll
        for (int h = 0; h < H; ++h) acc = fmaf(dh0[h], w0[h * NIN + k], acc);
        denc[k] = acc;
    }
    // a wave is 64 consecutive pixels of an image row: on the three coarse levels (cells of 1/4 .. 1/64 of the direction cube) its
    // lanes fall into a handful of cells, so runs are summed across lanes and only run heads issue atomics
    asd_scatter_runs<L, 3>(m, d_grid, x, y, z, denc, active);
    __syncthreads();
    for (int q = threadIdx.x; q < 3 * H; q += 256) atomicAdd(&dw2[q], w_acc[q]);
    for (int q = threadIdx.x; q < H * H; q += 256) atomicAdd(&dw1[q], w_acc[3 * H + q]);
    for (int q = threadIdx.x; q < H * NIN; q += 256) atomicAdd(&dw0[q], w_acc[3 * H + H * H + q]);
}

int asd_field_bwd_mlp_mfma(const asd_field_cfg* cfg, const float* w1d, const float* w2d, const float* w1f, const float* w2f, const float* enc, const float* sigma,
                           int32_t n, const int32_t* n_dev, const float* d_sigma, const float* d_features, float* denc_out, float* dw2d, float* dw2f,
                           float* dw1_slabs, int blocks, hipStream_t s);      // field_mfma.hip
int asd_field_bwd_mlp_mfma_blocks(int32_t n);

// ---------------------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------------------
static thread_local char g_err[512] = "";
void asd_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

hipEvent_t g_asd_probe_start = nullptr, g_asd_probe_stop = nullptr;

__global__ void asd_trace_mark_kernel() {}

extern "C" {

int asd_probe_events(void* start_event, void* stop_event) {
    g_asd_probe_start = (hipEvent_t)start_event;
    g_asd_probe_stop = (hipEvent_t)stop_event;
    return ASD_OK;
}

// an empty launch with a name of its own: brackets a region of a rocprofv3 kernel trace (tools/db_steps.py looks for it)
int asd_probe_mark(void* stream) {
    asd_trace_mark_kernel<<<1, 1, 0, (hipStream_t)stream>>>();
    return ASD_OK;
}

const char* asd_last_error(void) { return g_err; }
const char* asd_version(void) { return "asd_hip 0.1 (gfx950)"; }

uint32_t asd_grid_meta_init(asd_grid_meta* m, uint32_t n_levels, uint32_t n_features, uint32_t log2_hashmap_size,
                            uint32_t base_resolution, double per_level_scale) {
    memset(m, 0, sizeof(*m));
    if (n_levels == 0 || n_levels > ASD_MAX_LEVELS || n_features != 2) {
        asd_set_error("asd_grid_meta_init: need 1..%d levels and 2 features per level", ASD_MAX_LEVELS);
        return 0;
    }
    m->n_levels = n_levels;
    m->n_features = n_features;
    uint32_t offset = 0;
    const float log2_scale = log2f((float)per_level_scale);
    for (uint32_t l = 0; l < n_levels; ++l) {
        const float scale = exp2f((float)l * log2_scale) * (float)base_resolution - 1.0f;
        const uint32_t res = (uint32_t)ceilf(scale) + 1u;
        const uint64_t dense = (uint64_t)res * res * res;
        uint64_t size = (dense + 7u) / 8u * 8u;
        const uint64_t cap = 1ull << log2_hashmap_size;
        if (size > cap) size = cap;
        m->scale[l] = scale;
        m->resolution[l] = res;
        m->offset[l] = offset;
        m->size[l] = (uint32_t)size;
        m->dense[l] = dense <= size ? 1u : 0u;
        offset += (uint32_t)size;
    }
    m->n_params = offset * n_features;
    return m->n_params;
}

int asd_hashgrid_fwd(const asd_grid_meta* meta, const float* params, const float* x, int32_t n, float* out,
                     void* stream) {
    if (n == 0) return ASD_OK;
    ASD_CHECK_ARG(meta && params && x && out && n > 0, "null argument");
    ASD_CHECK_LEVEL_LIMIT(meta);
    hipLaunchKernelGGL(hashgrid_fwd_kernel, dim3(asd_point_level_grid(n, (int)meta->n_levels)), dim3(256), 0, (hipStream_t)stream, *meta,
                       params, x, n, out);
    ASD_LAUNCH_CHECK();
    return ASD_OK;
}

int asd_hashgrid_bwd(const asd_grid_meta* meta, const float* x, const float* dout, int32_t n, float* dparams,
                     void* stream) {
    if (n == 0) return ASD_OK;
    ASD_CHECK_ARG(meta && x && dout && dparams && n > 0, "null argument");
    ASD_CHECK_LEVEL_LIMIT(meta);
    hipLaunchKernelGGL(hashgrid_bwd_kernel, dim3(asd_point_level_grid(n, (int)meta->n_levels)), dim3(256), 0, (hipStream_t)stream, *meta,
                       x, dout, n, dparams);
    ASD_LAUNCH_CHECK();
    return ASD_OK;
}

int asd_field_supported(const asd_grid_meta* m, const asd_field_cfg* c, const char* what) {
    if (m->n_levels != 16 || c->n_hidden != 64 || !(c->n_feature_dims == 3 || c->n_feature_dims == 0)) {
        asd_set_error("%s kernels are built for 16 levels x 2 features, 64 hidden units, 0/3 feature dims "
                      "(got %u levels, %d hidden, %d feature dims)", what, m->n_levels, c->n_hidden, c->n_feature_dims);
        return 0;
    }
    return 1;
}

int asd_field_density(const asd_grid_meta* meta, const asd_field_cfg* cfg, const float* grid_params,
                      const float* w1_density, const float* w2_density, const float* points, int32_t n,
                      const int32_t* n_dev, float* sigma, void* stream) {
    if (n == 0) return ASD_OK;
    ASD_CHECK_ARG(meta && cfg && grid_params && w1_density && w2_density && points && sigma && n > 0, "null argument");
    ASD_CHECK_LEVEL_LIMIT(meta);
    if (!asd_field_supported(meta, cfg, "field")) return ASD_ERR_UNSUPPORTED;
    if (meta->n_masked_levels == 0)
        hipLaunchKernelGGL((field_density_kernel<16, 64, false>), dim3(asd_grid_for(n, 256)), dim3(256), 0, (hipStream_t)stream,
                           *meta, *cfg, grid_params, w1_density, w2_density, points, n, n_dev, sigma);
    else
        hipLaunchKernelGGL((field_density_kernel<16, 64, true>), dim3(asd_grid_for(n, 256)), dim3(256), 0, (hipStream_t)stream,
                           *meta, *cfg, grid_params, w1_density, w2_density, points, n, n_dev, sigma);
    ASD_LAUNCH_CHECK();
    return ASD_OK;
}

int asd_field_fwd(const asd_grid_meta* meta, const asd_field_cfg* cfg, const float* grid_params,
                  const float* w1_density, const float* w2_density, const float* w1_feature,
                  const float* w2_feature, const float* points, int32_t n, const int32_t* n_dev, float* sigma,
                  float* features, float* normal, float* fd_grad, float* enc_save, void* stream) {
    if (n == 0) return ASD_OK;
    ASD_CHECK_ARG(meta && cfg && grid_params && w1_density && w2_density && points && sigma && n > 0, "null argument");
    ASD_CHECK_LEVEL_LIMIT(meta);
    if (!asd_field_supported(meta, cfg, "field")) return ASD_ERR_UNSUPPORTED;
    ASD_CHECK_ARG(cfg->n_feature_dims == 0 || !features || (w1_feature && w2_feature), "feature weights missing");
    hipLaunchKernelGGL((field_fwd_kernel<16, 64, 3>), dim3(asd_grid_for(n, 256)), dim3(256), 0, (hipStream_t)stream,
                       *meta, *cfg, grid_params, w1_density, w2_density, w1_feature, w2_feature, points, n, n_dev,
                       sigma, cfg->n_feature_dims == 3 ? features : nullptr, normal, fd_grad, enc_save);
    ASD_LAUNCH_CHECK();
    return ASD_OK;
}

// The workspace of asd_field_bwd and asd_voxfield_bwd, in floats from its start: the size queries return `total`, the passes take every pointer
// from here.  Every region starts on a 256-byte boundary; -1: not part of this configuration.
struct field_bwd_layout {
    bool mfma;          // hash grid, 3 feature dims, no normal gradient: MLP half + first-layer weight gradients on the matrix pipe (field_mfma.hip)
    int n_slabs;        // slabs reserved = blocks of the launch that writes them
    int64_t da;         // [rows][128] hidden-layer gradients, field_bwd_sample_kernel<PRE = false> -> field_wgrad_kernel; not with mfma: its MLP kernel has
                        // no such argument and field_bwd_sample_kernel<PRE = true> skips the block that forms them
    int64_t enc_fd;     // [3 n][32] encodings of the finite-difference points (normal gradient only)
    int64_t slabs;      // [n_slabs][128][32] first-layer weight-gradient partial sums (field_wgrad_kernel | field_bwd_mlp_mfma_kernel)
    int64_t priv;       // hash grid: per-XCD copies of the gradient of the ASD_FIELD_NPRIV coarsest levels
    int64_t pg_g, pg_pos, pg_ws;    // hash grid, paged scatter of the fine levels (field_paged.h): gradients [rows][2 ASD_PG_NF_PAD], positions [rows][3], items
    int64_t denc;       // mfma: [n][32] encoding gradients between the MLP pass and the scatter | voxel: [rows][32] feature-gradient rows
    int64_t pts;        // voxel: [rows][3] the rows' positions for asd_voxel_sample_bwd_rows
    int64_t total;
};
static int field_wgrad_chunks(int64_t rows) { return (int)((rows + WG_ROWS - 1) / WG_ROWS); }      // blocks of field_wgrad_kernel
// the same reduction for csrc/field_analytic.hip (field_math.h)
int asd_field_wgrad_chunks(int64_t rows) { return field_wgrad_chunks(rows); }
void asd_field_slab_reduce_launch(const float* slabs, int n_slabs, int stride, int len, float* out, hipStream_t s) {
    hipLaunchKernelGGL(slab_reduce_kernel, dim3(asd_div_up(len, 32)), dim3(1024), 0, s, slabs, n_slabs, stride, len, out, (const int*)nullptr, 1);
}
// The first-layer weight-gradient tail of every field backward (field_math.h).  ONE n_slabs — the blocks of the launch that wrote or writes
// the slabs — sizes the launch and both reductions.
void asd_field_wgrad_tail(const float* da, const float* enc_a, const float* enc_b, int rows_a, int rows_total, const int* n_dev, bool slabs_written,
                          float* slabs, int n_slabs, float* dw1_density, float* dw1_feature, hipStream_t s) {
    // the matrix-pipe pass has written every block's slab; of field_wgrad_kernel's, with a device-side count and centre rows only, the slabs of
    // dead chunks are neither written nor summed
    const int* live = (!slabs_written && n_dev && rows_total == rows_a) ? n_dev : nullptr;
    if (!slabs_written)
        hipLaunchKernelGGL((field_wgrad_kernel<128, 32>), dim3(n_slabs), dim3(256), 0, s, da, enc_a, enc_b, rows_a, rows_total, n_dev, rows_a, slabs);
    // slab layout [h < 64: density | h >= 64: feature][k]; both halves are contiguous H*32 blocks
    hipLaunchKernelGGL(slab_reduce_kernel, dim3(asd_div_up(64 * 32, 32)), dim3(1024), 0, s, slabs, n_slabs, 128 * 32, 64 * 32, dw1_density, live, WG_ROWS);
    if (dw1_feature)
        hipLaunchKernelGGL(slab_reduce_kernel, dim3(asd_div_up(64 * 32, 32)), dim3(1024), 0, s, slabs + 64 * 32, n_slabs, 128 * 32, 64 * 32, dw1_feature,
                           live, WG_ROWS);
}
static bool field_paged_on() {      // ASD_FIELD_PAGED=0: the transposed-lane atomics of asd_scatter_runs for every level, the A/B partner
    static const bool on = !(getenv("ASD_FIELD_PAGED") && atoi(getenv("ASD_FIELD_PAGED")) == 0);
    return on;
}
static field_bwd_layout field_bwd_layout_init(const asd_field_cfg* cfg, int64_t n, int with_normal, bool voxel) {
    field_bwd_layout L;
    asd_ws_cursor w;
    const int64_t rows = n * (with_normal ? 4 : 1);
    const bool paged = !voxel && field_paged_on();
    L.mfma = !voxel && !with_normal && cfg->n_feature_dims == 3;
    L.n_slabs = L.mfma ? asd_field_bwd_mlp_mfma_blocks((int32_t)n) : field_wgrad_chunks(rows);
    L.da = L.mfma ? -1 : w.take(rows * 128);
    L.enc_fd = with_normal ? w.take(3 * n * 32) : -1;
    L.slabs = w.take((int64_t)L.n_slabs * 128 * 32);
    L.priv = !voxel ? w.take((int64_t)ASD_PRIV_COPIES * ASD_FIELD_PRIV_CAP) : -1;
    L.pg_g = paged ? w.take(rows * (2 * ASD_PG_NF_PAD)) : -1;
    L.pg_pos = paged ? w.take(rows * 3) : -1;
    L.pg_ws = paged ? w.take(asd_paged_workspace_floats(rows)) : -1;
    L.denc = L.mfma ? w.take(n * 32) : voxel ? w.take(rows * 32) : -1;
    L.pts = voxel ? w.take(rows * 3) : -1;
    L.total = w.o;
    return L;
}

int asd_field_bwd_workspace(const asd_field_cfg* cfg, int32_t n, int32_t with_normal, int64_t* n_floats) {
    ASD_CHECK_ARG(cfg && n_floats && n >= 0, "bad argument");
    *n_floats = field_bwd_layout_init(cfg, n, with_normal, false).total;
    return ASD_OK;
}

int asd_field_bwd(const asd_grid_meta* meta, const asd_field_cfg* cfg, const float* grid_params,
                  const float* w1_density, const float* w2_density, const float* w1_feature,
                  const float* w2_feature, const float* points, const float* enc_save, const float* sigma, int32_t n,
                  const int32_t* n_dev, const float* d_sigma, const float* d_features, const float* d_normal,
                  const float* d_fd_grad, float* d_grid_params, float* dw1_density, float* dw2_density, float* dw1_feature, float* dw2_feature,
                  float* workspace, void* stream) {
    if (n == 0) return ASD_OK;
    ASD_CHECK_ARG(meta && cfg && grid_params && w1_density && w2_density && points && enc_save && sigma &&
                      d_grid_params && dw1_density && dw2_density && workspace && n > 0,
                  "null argument");
    ASD_CHECK_LEVEL_LIMIT(meta);
    if (!asd_field_supported(meta, cfg, "field")) return ASD_ERR_UNSUPPORTED;
    ASD_CHECK_ARG(cfg->n_feature_dims == 3 || !d_features, "d_features given but no feature network");
    ASD_CHECK_ARG(cfg->n_feature_dims == 0 || (dw1_feature && dw2_feature && w1_feature && w2_feature), "feature gradients missing");
    hipStream_t s = (hipStream_t)stream;
    const int with_normal = d_normal != nullptr || d_fd_grad != nullptr;
    const int64_t rows = (int64_t)n * (with_normal ? 4 : 1);
    const field_bwd_layout L = field_bwd_layout_init(cfg, n, with_normal, false);
    auto at = [&](int64_t off) { return off < 0 ? (float*)nullptr : workspace + off; };
    float *const da = at(L.da), *const enc_fd = at(L.enc_fd), *const slabs = at(L.slabs), *priv = at(L.priv);
    uint32_t priv_stride = 2u * meta->offset[ASD_FIELD_NPRIV];   // floats per copy
    if (priv_stride > (uint32_t)ASD_FIELD_PRIV_CAP) priv_stride = 0;    // a grid with larger coarse levels: straight into the table
    if (priv_stride > 0) {
        if (hipMemsetAsync(priv, 0, (size_t)ASD_PRIV_COPIES * priv_stride * sizeof(float), s) != hipSuccess) {
            asd_set_error("hipMemsetAsync of the per-XCD gradient copies failed");
            return ASD_ERR_LAUNCH;
        }
    } else {
        priv = d_grid_params;
    }
    // the levels >= ASD_FIELD_NAGG (hashed: neighbouring samples share no entry) through the paged scatter — no global atomics
    static_assert(16 - ASD_FIELD_NAGG == ASD_PG_NF, "field_paged.h is sized for the levels >= ASD_FIELD_NAGG of the 16-level grid");
    asd_paged_plan plan;
    // (level limit: with no active level >= ASD_FIELD_NAGG there is nothing to page — no row writes, no fill, no accumulate)
    const bool paged = field_paged_on() && asd_active_levels(*meta) > ASD_FIELD_NAGG && asd_paged_plan_init(meta, ASD_FIELD_NAGG, &plan);
    float *const pg_g = paged ? at(L.pg_g) : nullptr, *const pg_pos = paged ? at(L.pg_pos) : nullptr;
    const dim3 grid(asd_div_up(n, 256)), block(256);
    // slabs of the first-layer weight gradient: one per block of the launch that writes them, and slab_reduce_kernel sums that many
    const int n_slabs = L.mfma ? asd_field_bwd_mlp_mfma_blocks(n) : field_wgrad_chunks(rows);
    ASD_CHECK_ARG(n_slabs <= L.n_slabs, "more weight-gradient slabs than the workspace reserves");
    ASD_PROBE_START(s);
    if (L.mfma) {
        // the MLP half and the first-layer weight gradient on the matrix pipe (field_mfma.hip) where there are no finite-difference rows: the
        // headline renderer (lambda_orient = 0); the sample kernel then only scatters
        float* const denc = at(L.denc);
        const int rc = asd_field_bwd_mlp_mfma(cfg, w1_density, w2_density, w1_feature, w2_feature, enc_save, sigma, n, n_dev, d_sigma, d_features, denc,
                                              dw2_density, dw2_feature, slabs, n_slabs, s);
        if (rc != ASD_OK) return rc;
        hipLaunchKernelGGL((field_bwd_sample_kernel<16, 64, 3, 0, true>), grid, block, 0, s, *meta, *cfg, grid_params, w1_density, w2_density,
                           w1_feature, w2_feature, points, enc_save, sigma, n, n_dev, d_sigma, d_features, d_normal, d_fd_grad,
                           d_grid_params, da, enc_fd, dw2_density, dw2_feature, priv, priv_stride, (float*)nullptr, (float*)nullptr,
                           pg_g, pg_pos, (const float*)denc);
    } else {
#define ASD_FIELD_BWD_LAUNCH(C_)                                                                                                     \
    hipLaunchKernelGGL((field_bwd_sample_kernel<16, 64, C_>), grid, block, 0, s, *meta, *cfg, grid_params, w1_density, w2_density,  \
                       w1_feature, w2_feature, points, enc_save, sigma, n, n_dev, d_sigma, d_features, d_normal, d_fd_grad,        \
                       d_grid_params, da, enc_fd, dw2_density, dw2_feature, priv, priv_stride, (float*)nullptr, (float*)nullptr,   \
                       pg_g, pg_pos)
    if (cfg->n_feature_dims == 3) ASD_FIELD_BWD_LAUNCH(3); else ASD_FIELD_BWD_LAUNCH(0);
#undef ASD_FIELD_BWD_LAUNCH
    }
    if (priv_stride > 0)
        hipLaunchKernelGGL(asd_priv_reduce_kernel, dim3(asd_div_up(priv_stride / 4, 256)), block, 0, s, priv, priv_stride, priv_stride,
                           d_grid_params);
    if (paged) {
        const int rc = asd_paged_scatter(meta, &plan, pg_pos, pg_g, n, with_normal ? 4 : 1, n_dev, d_grid_params, at(L.pg_ws), s);
        if (rc != ASD_OK) return rc;
    }
    ASD_PROBE_STOP(s);
    asd_field_wgrad_tail(da, enc_save, enc_fd, n, (int)rows, n_dev, L.mfma, slabs, n_slabs, dw1_density, cfg->n_feature_dims == 3 ? dw1_feature : nullptr, s);
    ASD_LAUNCH_CHECK();
    return ASD_OK;
}

// ---- the same fused field over a sampled feature volume (3DConv-net: stylegan_3dconv_net.py:244-346) ---------------------------------
static asd_grid_meta vox_meta(int D, int H, int W) {
    asd_grid_meta m;
    memset(&m, 0, sizeof(m));
    m.n_levels = 16; m.n_features = 2;
    m.resolution[0] = (uint32_t)W; m.resolution[1] = (uint32_t)H; m.resolution[2] = (uint32_t)D;
    return m;
}
static int voxfield_supported(const asd_field_cfg* c, int C) {
    if (C != 32 || c->n_hidden != 64 || !(c->n_feature_dims == 3 || c->n_feature_dims == 0)) {
        asd_set_error("voxel field kernels are built for 32 feature channels, 64 hidden units, 0/3 feature dims (got %d channels, %d hidden, %d feature dims)",
                      C, c->n_hidden, c->n_feature_dims);
        return 0;
    }
    return 1;
}

int asd_voxfield_fwd(const float* voxel_cl, int32_t D, int32_t H, int32_t W, int32_t C, const asd_field_cfg* cfg, const float* w1_sdf, const float* w2_sdf,
                     const float* w1_feature, const float* w2_feature, const float* points, int32_t n, float* sdf, float* features, float* normal,
                     float* fd_grad, float* enc_save, void* stream) {
    if (n == 0) return ASD_OK;
    ASD_CHECK_ARG(voxel_cl && cfg && w1_sdf && w2_sdf && points && sdf && n > 0 && D > 0 && H > 0 && W > 0, "null argument");
    if (!voxfield_supported(cfg, C)) return ASD_ERR_UNSUPPORTED;
    ASD_CHECK_ARG(cfg->n_feature_dims == 0 || !features || (w1_feature && w2_feature), "feature weights missing");
    const asd_grid_meta m = vox_meta(D, H, W);
    hipLaunchKernelGGL((field_fwd_kernel<16, 64, 3, 1>), dim3(asd_grid_for(n, 256)), dim3(256), 0, (hipStream_t)stream, m, *cfg, voxel_cl, w1_sdf, w2_sdf,
                       w1_feature, w2_feature, points, n, (const int*)nullptr, sdf, cfg->n_feature_dims == 3 ? features : nullptr, normal, fd_grad, enc_save);
    ASD_LAUNCH_CHECK();
    return ASD_OK;
}

int asd_voxfield_bwd_workspace(const asd_field_cfg* cfg, int32_t n, int32_t with_normal, int64_t* n_floats) {
    ASD_CHECK_ARG(cfg && n_floats && n >= 0, "bad argument");
    *n_floats = field_bwd_layout_init(cfg, n, with_normal, true).total;
    return ASD_OK;
}

int asd_voxfield_bwd(const float* voxel_cl, int32_t D, int32_t H, int32_t W, int32_t C, const asd_field_cfg* cfg, const float* w1_sdf, const float* w2_sdf,
                     const float* w1_feature, const float* w2_feature, const float* points, const float* enc_save, const float* sdf, int32_t n,
                     const float* d_sdf, const float* d_features, const float* d_normal, const float* d_fd_grad, float* d_voxel_cl, float* dw1_sdf,
                     float* dw2_sdf, float* dw1_feature, float* dw2_feature, float* workspace, void* stream) {
    if (n == 0) return ASD_OK;
    ASD_CHECK_ARG(voxel_cl && cfg && w1_sdf && w2_sdf && points && enc_save && sdf && d_voxel_cl && dw1_sdf && dw2_sdf && workspace && n > 0, "null argument");
    if (!voxfield_supported(cfg, C)) return ASD_ERR_UNSUPPORTED;
    ASD_CHECK_ARG(cfg->n_feature_dims == 3 || !d_features, "d_features given but no feature network");
    ASD_CHECK_ARG(cfg->n_feature_dims == 0 || (dw1_feature && dw2_feature && w1_feature && w2_feature), "feature gradients missing");
    hipStream_t s = (hipStream_t)stream;
    const int with_normal = d_normal != nullptr || d_fd_grad != nullptr;
    const int64_t rows = (int64_t)n * (with_normal ? 4 : 1);
    const field_bwd_layout L = field_bwd_layout_init(cfg, n, with_normal, true);
    float *const da = workspace + L.da, *const enc_fd = with_normal ? workspace + L.enc_fd : nullptr, *const slabs = workspace + L.slabs;
    float *const denc = workspace + L.denc, *const pts = workspace + L.pts;
    const int n_slabs = field_wgrad_chunks(rows);       // blocks of field_wgrad_kernel = slabs slab_reduce_kernel sums
    ASD_CHECK_ARG(n_slabs <= L.n_slabs, "more weight-gradient slabs than the workspace reserves");
    const asd_grid_meta m = vox_meta(D, H, W);
    const dim3 grid(asd_div_up(n, 256)), block(256);
#define ASD_VOXFIELD_BWD_LAUNCH(C_)                                                                                                        \
    hipLaunchKernelGGL((field_bwd_sample_kernel<16, 64, C_, 1>), grid, block, 0, s, m, *cfg, voxel_cl, w1_sdf, w2_sdf, w1_feature, w2_feature, \
                       points, enc_save, sdf, n, (const int*)nullptr, d_sdf, d_features, d_normal, d_fd_grad, (float*)nullptr, da, enc_fd,  \
                       dw2_sdf, dw2_feature, (float*)nullptr, 0u, denc, pts)
    if (cfg->n_feature_dims == 3) ASD_VOXFIELD_BWD_LAUNCH(3); else ASD_VOXFIELD_BWD_LAUNCH(0);
#undef ASD_VOXFIELD_BWD_LAUNCH
    const int rc = asd_voxel_sample_bwd_rows(denc, D, H, W, C, pts, (int32_t)rows, d_voxel_cl, 128, stream);     // += (atomics), amortized.hip
    if (rc != ASD_OK) return rc;
    asd_field_wgrad_tail(da, enc_save, enc_fd, n, (int)rows, nullptr, false, slabs, n_slabs, dw1_sdf, cfg->n_feature_dims == 3 ? dw1_feature : nullptr, s);
    ASD_LAUNCH_CHECK();
    return ASD_OK;
}

int asd_envmap_fwd(const asd_grid_meta* meta, const float* grid_params, const float* w0, const float* w1,
                   const float* w2, int32_t n_hidden, const float* dirs, int32_t n, float* color, void* stream) {
    if (n == 0) return ASD_OK;
    ASD_CHECK_ARG(meta && grid_params && w0 && w1 && w2 && dirs && color && n > 0, "null argument");
    if (meta->n_levels != 4 || n_hidden != 16) {
        asd_set_error("envmap kernels are built for 4 levels and 16 hidden units (got %u, %d)", meta->n_levels, n_hidden);
        return ASD_ERR_UNSUPPORTED;
    }
    if (meta->n_masked_levels != 0) {
        asd_set_error("envmap kernels take no level limit (n_masked_levels = %u): the background grid is not progressive", meta->n_masked_levels);
        return ASD_ERR_UNSUPPORTED;
    }
    if (n == 0) return ASD_OK;
    hipLaunchKernelGGL((envmap_fwd_kernel<4, 16>), dim3(asd_grid_for(n, 256)), dim3(256), 0, (hipStream_t)stream, *meta,
                       grid_params, w0, w1, w2, dirs, n, color);
    ASD_LAUNCH_CHECK();
    return ASD_OK;
}

int asd_envmap_bwd(const asd_grid_meta* meta, const float* grid_params, const float* w0, const float* w1,
                   const float* w2, int32_t n_hidden, const float* dirs, const float* d_color, int32_t n,
                   float* d_grid_params, float* dw0, float* dw1, float* dw2, void* stream) {
    if (n == 0) return ASD_OK;
    ASD_CHECK_ARG(meta && grid_params && w0 && w1 && w2 && dirs && d_color && d_grid_params && dw0 && dw1 && dw2 && n > 0,
                  "null argument");
    if (meta->n_levels != 4 || n_hidden != 16) {
        asd_set_error("envmap kernels are built for 4 levels and 16 hidden units (got %u, %d)", meta->n_levels, n_hidden);
        return ASD_ERR_UNSUPPORTED;
    }
    if (meta->n_masked_levels != 0) {
        asd_set_error("envmap kernels take no level limit (n_masked_levels = %u): the background grid is not progressive", meta->n_masked_levels);
        return ASD_ERR_UNSUPPORTED;
    }
    if (n == 0) return ASD_OK;
    hipLaunchKernelGGL((envmap_bwd_kernel<4, 16>), dim3(asd_div_up(n, 256)), dim3(256), 0, (hipStream_t)stream, *meta,
                       grid_params, w0, w1, w2, dirs, d_color, n, d_grid_params, dw0, dw1, dw2);
    ASD_LAUNCH_CHECK();
    return ASD_OK;
}

}  // extern "C"
