// volsdf.hip — the importance-sampled VolSDF renderer of the amortized workloads as pass-level entries for gfx950
// (custom/amortized/models/renderers/generative_space_volsdf_volume_renderer.py on top of threestudio/models/estimators.py and
// threestudio/models/renderers/neus_volume_renderer.py): everything between the rays and the image that is not a field, background or
// hypernetwork call.  All tensors are dense [n_rays, S] fp32 (every ray holds exactly S samples: offset = ray * S, count = S).
//   asd_volsdf_edges          importance resampling + the "uniform" s -> t map                    (one thread per output edge)
//   asd_volsdf_samples        mid-points, directions, t_mid, t_len, ray index of every interval   (one thread per sample)
//   asd_volsdf_proposal_cdf   VolSDF density of the proposal SDF -> transmittance cdf             (one wave per ray)
//   asd_volsdf_composite_fwd  density -> alpha -> weights and every per-ray image in ONE pass     (one wave per ray)
//   asd_volsdf_composite_bwd  its gradient w.r.t. sdf, features, background and the variance      (one wave per ray + one tiny reduce)
// Roofline: bandwidth-trivial (4 096 rays x 193 samples x ~36 B = 28 MB per compositing pass); what these kernels buy is launches —
// seven forward and one or two backward where the composed path enqueues about ninety (782 -> 702 per Hyper-iNGP step).
// Shared with render.hip and neus.hip, in ray_composite.h: the learned variance read on the device (here always with the VolSDF clamp)
// and the density, the colour read, the transmittance step, the per-ray images and the common part of their gradients; the
// variance-gradient reduce is sdf_dp_reduce of neus.hip.
#include "asd_common.h"
#include "ray_composite.h"

#define VOLSDF_RAYS_PER_BLOCK 4     // 256 threads = 4 waves = 4 rays
#define VOLSDF_MAX_CDF_SAMPLES 2048 // asd_volsdf_proposal_cdf keeps one float per sample of its 4 rays in LDS (32 KB)

// ---- sampling ---------------------------------------------------------------------------------------------------------------------
// asd_importance_resample's search and interpolation (amortized.hip: same arithmetic, bit-identical edges) with the s -> t map behind it
__global__ __launch_bounds__(256) void volsdf_edges_kernel(const float* __restrict__ vals, const float* __restrict__ cdfs, int n_rays, int e_in,
                                                           int n_out, const float* __restrict__ jitter, float near, float far,
                                                           float* __restrict__ s_out, float* __restrict__ t_out) {
    const int per = n_out + 1;
    const long long total = (long long)n_rays * per;
    for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < total; q += (long long)gridDim.x * 256) {
        const int r = (int)(q / per), j = (int)(q - (long long)r * per);
        const float* v = vals + (size_t)r * e_in;
        const float* c = cdfs + (size_t)r * e_in;
        const float u = jitter ? ((float)j + jitter[r]) / (float)(n_out + 1) : (float)j / (float)n_out;
        int lo = 0, hi = e_in - 2;
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (c[mid] <= u) lo = mid; else hi = mid - 1;
        }
        const float c0 = c[lo], c1 = c[lo + 1];
        const float w = c1 > c0 ? fminf(fmaxf((u - c0) / (c1 - c0), 0.f), 1.f) : 0.f;
        const float s = fmaf(w, v[lo + 1] - v[lo], v[lo]);
        if (s_out) s_out[q] = s;
        t_out[q] = s * far + (1.f - s) * near;      // _transform_stot("uniform"): s * t_max + (1 - s) * t_min, two roundings per product
    }
}

__global__ __launch_bounds__(256) void volsdf_samples_kernel(const float* __restrict__ rays_o, const float* __restrict__ rays_d,
                                                             const float* __restrict__ t_edges, int n_rays, int S, float* __restrict__ points,
                                                             float* __restrict__ t_dirs, float* __restrict__ t_mid, float* __restrict__ t_len,
                                                             int64_t* __restrict__ ray_idx) {
    const long long total = (long long)n_rays * S;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int r = (int)(i / S), j = (int)(i - (long long)r * S);
        const float t0 = t_edges[(size_t)r * (S + 1) + j], t1 = t_edges[(size_t)r * (S + 1) + j + 1];
        const float tm = (t0 + t1) * 0.5f;
        const float dx = rays_d[3 * r], dy = rays_d[3 * r + 1], dz = rays_d[3 * r + 2];
        if (points) {       // o + d * t_mid: separate multiply and add, as the reference forms it
            points[3 * (size_t)i] = rays_o[3 * r] + dx * tm;
            points[3 * (size_t)i + 1] = rays_o[3 * r + 1] + dy * tm;
            points[3 * (size_t)i + 2] = rays_o[3 * r + 2] + dz * tm;
        }
        if (t_dirs) { t_dirs[3 * (size_t)i] = dx; t_dirs[3 * (size_t)i + 1] = dy; t_dirs[3 * (size_t)i + 2] = dz; }
        if (t_mid) t_mid[i] = tm;
        if (t_len) t_len[i] = t1 - t0;
        if (ray_idx) ray_idx[i] = r;
    }
}

// cdf[r, j] = 1 - exp(-sum_{k<j} sigma_k dt_k), cdf[r, S] = 1.  The 64 lanes of a ray's wave evaluate the densities (expm1 and a division per
// sample) and the final exponentials side by side; the running sum in between stays ONE sequential fmaf chain in lane 0 — the rounding of
// asd_transmittance_cdf and of the oracle — over values that wait in LDS.
__global__ __launch_bounds__(256) void volsdf_proposal_cdf_kernel(const float* __restrict__ sdf, const float* __restrict__ t_edges,
                                                                  const float* __restrict__ p, int n_rays, int S, float* __restrict__ cdf) {
    extern __shared__ float lds[];
    const int wid = threadIdx.x >> 6, lane = asd_lane();
    const int r = blockIdx.x * VOLSDF_RAYS_PER_BLOCK + wid;
    const bool live = r < n_rays;             // (no early return: the block meets at two barriers)
    float* acc_s = lds + (size_t)wid * S;
    const float* t = t_edges + (size_t)(live ? r : 0) * (S + 1);
    if (live) {
        const sdf_var v = sdf_variance(p, 1);
        for (int j = lane; j < S; j += 64) {
            float sg, em1;
            acc_s[j] = volsdf_sigma(sdf[(size_t)r * S + j], v.a, sg, em1);
        }
    }
    __syncthreads();
    if (live && lane == 0) {
        float acc = 0.f, t0 = t[0];
        for (int j = 0; j < S; ++j) {
            const float t1 = t[j + 1], sg = acc_s[j];
            acc_s[j] = acc;
            acc = fmaf(sg, t1 - t0, acc);
            t0 = t1;
        }
    }
    __syncthreads();
    if (live) {
        float* o = cdf + (size_t)r * (S + 1);
        for (int j = lane; j < S; j += 64) o[j] = 1.f - expf(-acc_s[j]);
        if (lane == 0) o[S] = 1.f;
    }
}

// ---- compositing ------------------------------------------------------------------------------------------------------------------
// composite_fwd_kernel<2> of render.hip with the alpha formed in place (get_alpha: |dt| sigma(sdf), not clamped: the transmittance is the
// running product of (1 - alpha), whatever its sign) and the normal image accumulated in the same trip.
__global__ __launch_bounds__(256) void volsdf_composite_fwd_kernel(
    const float* __restrict__ sdf, const float* __restrict__ feat, int color_act, const float* __restrict__ normal,
    const float* __restrict__ t_edges, const float* __restrict__ p, const float* __restrict__ bg, int n_rays, int S,
    float* __restrict__ weights, float* __restrict__ opacity, float* __restrict__ depth, float* __restrict__ rgb_fg, float* __restrict__ z_var,
    float* __restrict__ comp_rgb, float* __restrict__ comp_normal) {
    const int r = blockIdx.x * VOLSDF_RAYS_PER_BLOCK + (threadIdx.x >> 6);
    if (r >= n_rays) return;
    const int lane = asd_lane();
    const size_t b = (size_t)r * S;
    const float* t = t_edges + (size_t)r * (S + 1);
    const sdf_var v = sdf_variance(p, 1);
    float carry = 1.f;
    ray_images img;
    ray_normal nrm;
    for (int j0 = 0; j0 < S; j0 += 64) {
        const int j = j0 + lane;
        const bool valid = j < S;
        const size_t i = b + j;
        float alpha = 0.f, tm = 0.f;
        if (valid) {
            const float t0 = t[j], t1 = t[j + 1];
            float sg, em1;
            alpha = fabsf(t1 - t0) * volsdf_sigma(sdf[i], v.a, sg, em1);
            tm = (t0 + t1) * 0.5f;
        }
        const float T = ray_trans_step(alpha, carry);
        if (valid) {
            const float w = T * alpha;
            weights[i] = w;
            img.add(w, tm, feat, i, color_act);
            if (normal) nrm.add(w, normal, i);
        }
    }
    img.reduce();
    // z_variance = sum_i w_i (t_i - depth)^2, unnormalised and unmasked (generative_space_volsdf_volume_renderer.py:380-385); every lane
    // reads back the weights it wrote itself
    float zv = 0.f;
    for (int j = lane; j < S; j += 64) {
        const float tm = (t[j] + t[j + 1]) * 0.5f;
        zv = fmaf(weights[b + j], (tm - img.dp) * (tm - img.dp), zv);
    }
    zv = asd_wave_sum(zv);
    if (normal) nrm.reduce();
    if (lane == 0) {
        z_var[r] = zv;
        img.store(r, bg, opacity, depth, rgb_fg, comp_rgb);
        if (normal) nrm.store(r, img.op, comp_normal);
    }
}

// inclusive SUFFIX sum across the 64 lanes of a wave: lane l receives sum_{k >= l} v_k
__device__ __forceinline__ float volsdf_wave_suffix_sum(float v) {
    const int lane = asd_lane();
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const float u = __shfl_down(v, o, 64);
        if (lane + o < 64) v += u;
    }
    return v;
}

// Backward.  With gw_i = dL/dw_i (all seven images and the weights themselves) and S_i = sum_{j>i} w_j gw_j:
//   dL/dalpha_i = T_i gw_i - S_i / (1 - alpha_i),  dL/dsdf_i = dL/dalpha_i |dt_i| dsigma/ds,  dL/da = sum_i dL/dalpha_i |dt_i| dsigma/da,
//   dsigma/ds = -a^2 e / 2 (0 at s = 0, as torch's sign / abs give),  dsigma/da = 0.5 + 0.5 sign(s) expm1(-|s| a) - a s e / 2,  e = exp(-|s| a).
// Nothing but weights, opacity and depth is kept from the forward pass: alpha and the transmittance are formed again (the exponential is
// needed for the derivatives anyway).  The normal image is differentiable in the opacity only; its unit vector is re-accumulated first.
// S_i is summed from the FAR end of the ray (a suffix scan, walking the trips backwards) instead of `total - prefix`: behind the surface, where
// T_i and S_i both vanish, the difference of two sums of the whole ray would leave a rounding residue of ~1e-7 in every sample — harmless in
// d_sdf, but dL/da adds it up over every sample inside the object.  The suffix sums wait in d_sdf (each lane reads back what it wrote itself).
// dp_partial[r] receives the ray's part of dL/da (a wave sum: no atomics), sdf_dp_reduce adds the rays in a fixed order.
__global__ __launch_bounds__(256) void volsdf_composite_bwd_kernel(
    const float* __restrict__ sdf, const float* __restrict__ feat, int color_act, const float* __restrict__ normal,
    const float* __restrict__ t_edges, const float* __restrict__ p, const float* __restrict__ bg, int n_rays, int S,
    const float* __restrict__ weights, const float* __restrict__ opacity, const float* __restrict__ depth,
    const float* __restrict__ d_comp_rgb, const float* __restrict__ d_rgb_fg, const float* __restrict__ d_opacity, const float* __restrict__ d_depth,
    const float* __restrict__ d_z_var, const float* __restrict__ d_weights, const float* __restrict__ d_comp_normal,
    float* __restrict__ d_sdf, float* __restrict__ d_feat, float* __restrict__ d_bg, float* __restrict__ dp_partial) {
    const int r = blockIdx.x * VOLSDF_RAYS_PER_BLOCK + (threadIdx.x >> 6);
    if (r >= n_rays) return;
    const int lane = asd_lane();
    const size_t b = (size_t)r * S;
    const float* t = t_edges + (size_t)r * (S + 1);
    const sdf_var v = sdf_variance(p, 1);
    const float op = opacity[r], zm = depth[r];
    ray_grads g;
    g.load(r, d_comp_rgb, d_rgb_fg, d_opacity, d_depth, bg, op, d_bg);
    const float gzv = d_z_var ? d_z_var[r] : 0.f;
    if (normal && d_comp_normal) {      // d opacity += d comp_normal . (normalize(sum_i w_i n_i) + 1) / 2
        ray_normal nrm;
        for (int j = lane; j < S; j += 64) nrm.add(weights[b + j], normal, b + j);
        nrm.reduce();
        float u[3];
        nrm.shade(u);
#pragma unroll
        for (int k = 0; k < 3; ++k) g.gop = fmaf(d_comp_normal[3 * (size_t)r + k], u[k], g.gop);
    }
    auto gw_of = [&](size_t i, float tm, const float (&col)[3]) {
        float gw = g.gw(i, tm, col, d_weights);
        // d z_var / d w_i = (t_i - depth)^2 - 2 t_i depth (1 - opacity): the second term is the depth moving under every other sample
        if (gzv != 0.f) gw += gzv * ((tm - zm) * (tm - zm) - 2.f * tm * zm * (1.f - op));
        return gw;
    };
    // pass 1, far to near: S_i = sum_{j>i} w_j gw_j
    float carry_s = 0.f;
    for (int j0 = ((S - 1) / 64) * 64; j0 >= 0; j0 -= 64) {
        const int j = j0 + lane;
        const bool valid = j < S;
        const size_t i = b + j;
        float wg = 0.f;
        if (valid) {
            const float col[3] = {ray_colour(feat, i, 0, color_act), ray_colour(feat, i, 1, color_act), ray_colour(feat, i, 2, color_act)};
            wg = weights[i] * gw_of(i, (t[j] + t[j + 1]) * 0.5f, col);
        }
        const float incl = volsdf_wave_suffix_sum(wg);
        float excl = __shfl_down(incl, 1, 64);      // the lanes behind this one
        if (lane == 63) excl = 0.f;
        if (valid) d_sdf[i] = carry_s + excl;
        carry_s += __shfl(incl, 0, 64);
    }
    // pass 2, near to far: the transmittances again, the gradients
    float carry_t = 1.f, dpa = 0.f;
    for (int j0 = 0; j0 < S; j0 += 64) {
        const int j = j0 + lane;
        const bool valid = j < S;
        const size_t i = b + j;
        float dt = 0.f, w = 0.f, gw = 0.f, alpha = 0.f, s = 0.f, sg = 0.f, em1 = 0.f, Ssuf = 0.f;
        float col[3] = {0.f, 0.f, 0.f};
        if (valid) {
            const float t0 = t[j], t1 = t[j + 1];
            dt = fabsf(t1 - t0);
            s = sdf[i];
            alpha = dt * volsdf_sigma(s, v.a, sg, em1);
            w = weights[i];
            Ssuf = d_sdf[i];
#pragma unroll
            for (int k = 0; k < 3; ++k) col[k] = ray_colour(feat, i, k, color_act);
            gw = gw_of(i, (t0 + t1) * 0.5f, col);
        }
        const float om = 1.f - alpha;
        const float T = ray_trans_step(alpha, carry_t);
        if (valid) {
            // d w_j / d alpha_i = -w_j / (1 - alpha_i) for j > i holds for either sign of 1 - alpha_i (alpha is not clamped); only a
            // factor of exactly zero has no quotient form, and is kept away from it
            const float om_safe = fabsf(om) < 1e-10f ? copysignf(1e-10f, om) : om;
            const float da = T * gw - Ssuf / om_safe;
            const float beta = 1.f / v.a;
            const float e = expf(-fabsf(s) / beta);       // (not em1 + 1: far from the surface that sum has no digits left)
            d_sdf[i] = da * dt * (-0.5f * v.a * v.a * e * sg * sg);
            dpa = fmaf(da * dt, (0.5f + 0.5f * sg * em1) - 0.5f * v.a * s * e, dpa);
            g.store_d_feat(d_feat, i, w, col, color_act);
        }
    }
    if (dp_partial) {
        dpa = asd_wave_sum(dpa);
        if (lane == 0) dp_partial[r] = dpa;
    }
}

extern "C" {

int asd_volsdf_edges(const float* vals, const float* cdfs, int32_t n_rays, int32_t e_in, int32_t n_out, const float* jitter, float near_plane,
                     float far_plane, float* s_edges, float* t_edges, void* stream) {
    ASD_CHECK_ARG(vals && cdfs && t_edges, "null argument");
    ASD_CHECK_ARG(n_rays >= 0, "n_rays must not be negative");
    ASD_CHECK_ARG(e_in >= 2 && n_out >= 1, "need at least one input interval and one output interval");
    if (n_rays == 0) return ASD_OK;
    hipLaunchKernelGGL(volsdf_edges_kernel, dim3(asd_grid_for((int64_t)n_rays * (n_out + 1), 256)), dim3(256), 0, (hipStream_t)stream, vals, cdfs,
                       n_rays, e_in, n_out, jitter, near_plane, far_plane, s_edges, t_edges);
    ASD_LAUNCH_CHECK();
    return ASD_OK;
}

int asd_volsdf_samples(const float* rays_o, const float* rays_d, const float* t_edges, int32_t n_rays, int32_t S, float* points, float* t_dirs,
                       float* t_mid, float* t_len, int64_t* ray_idx, void* stream) {
    ASD_CHECK_ARG(rays_o && rays_d && t_edges, "null argument");
    ASD_CHECK_ARG(n_rays >= 0, "n_rays must not be negative");
    ASD_CHECK_ARG(S > 0, "need at least one sample per ray");
    if (n_rays == 0) return ASD_OK;
    hipLaunchKernelGGL(volsdf_samples_kernel, dim3(asd_grid_for((int64_t)n_rays * S, 256)), dim3(256), 0, (hipStream_t)stream, rays_o, rays_d, t_edges,
                       n_rays, S, points, t_dirs, t_mid, t_len, ray_idx);
    ASD_LAUNCH_CHECK();
    return ASD_OK;
}

int asd_volsdf_proposal_cdf(const float* sdf, const float* t_edges, const float* inv_std_param, int32_t n_rays, int32_t S, float* cdf, void* stream) {
    ASD_CHECK_ARG(sdf && t_edges && inv_std_param && cdf, "null argument");
    ASD_CHECK_ARG(n_rays >= 0, "n_rays must not be negative");
    ASD_CHECK_ARG(S > 0, "need at least one sample per ray");
    if (S > VOLSDF_MAX_CDF_SAMPLES) {
        asd_set_error("%s: at most %d proposal samples per ray (got %d)", __func__, VOLSDF_MAX_CDF_SAMPLES, S);
        return ASD_ERR_UNSUPPORTED;
    }
    if (n_rays == 0) return ASD_OK;
    hipLaunchKernelGGL(volsdf_proposal_cdf_kernel, dim3(asd_div_up(n_rays, VOLSDF_RAYS_PER_BLOCK)), dim3(256),
                       (size_t)VOLSDF_RAYS_PER_BLOCK * S * sizeof(float), (hipStream_t)stream, sdf, t_edges, inv_std_param, n_rays, S, cdf);
    ASD_LAUNCH_CHECK();
    return ASD_OK;
}

int asd_volsdf_composite_fwd(const float* sdf, const float* features, int32_t color_act, const float* normal, const float* t_edges,
                             const float* inv_std_param, const float* bg, int32_t n_rays, int32_t S, float* weights, float* opacity, float* depth,
                             float* rgb_fg, float* z_var, float* comp_rgb, float* comp_normal, void* stream) {
    ASD_CHECK_ARG(sdf && features && t_edges && inv_std_param && bg && weights && opacity && depth && rgb_fg && z_var && comp_rgb, "null argument");
    ASD_CHECK_ARG(!normal || comp_normal, "normals without a comp_normal output");
    ASD_CHECK_ARG(n_rays >= 0, "n_rays must not be negative");
    ASD_CHECK_ARG(S > 0, "need at least one sample per ray");
    ASD_CHECK_ARG(color_act == 0 || color_act == 1, "color_act: 0 (features are colours) or 1 (sigmoid)");
    if (n_rays == 0) return ASD_OK;
    hipLaunchKernelGGL(volsdf_composite_fwd_kernel, dim3(asd_div_up(n_rays, VOLSDF_RAYS_PER_BLOCK)), dim3(256), 0, (hipStream_t)stream, sdf, features,
                       color_act, normal, t_edges, inv_std_param, bg, n_rays, S, weights, opacity, depth, rgb_fg, z_var, comp_rgb, comp_normal);
    ASD_LAUNCH_CHECK();
    return ASD_OK;
}

int asd_volsdf_composite_bwd(const float* sdf, const float* features, int32_t color_act, const float* normal, const float* t_edges,
                             const float* inv_std_param, const float* bg, int32_t n_rays, int32_t S, const float* weights, const float* opacity,
                             const float* depth, const float* d_comp_rgb, const float* d_rgb_fg, const float* d_opacity, const float* d_depth,
                             const float* d_z_var, const float* d_weights, const float* d_comp_normal, float* d_sdf, float* d_features, float* d_bg,
                             float* d_inv_std_param, float* dp_partial, void* stream) {
    ASD_CHECK_ARG(sdf && features && t_edges && inv_std_param && bg && weights && opacity && depth && d_sdf && d_features, "null argument");
    ASD_CHECK_ARG(!d_comp_normal || normal, "a comp_normal gradient needs the normals of the forward pass");
    ASD_CHECK_ARG(!d_inv_std_param || dp_partial, "the variance gradient needs its [n_rays] partial-sum buffer");
    ASD_CHECK_ARG(n_rays >= 0, "n_rays must not be negative");
    ASD_CHECK_ARG(S > 0, "need at least one sample per ray");
    ASD_CHECK_ARG(color_act == 0 || color_act == 1, "color_act: 0 (features are colours) or 1 (sigmoid)");
    if (n_rays == 0) return ASD_OK;
    hipLaunchKernelGGL(volsdf_composite_bwd_kernel, dim3(asd_div_up(n_rays, VOLSDF_RAYS_PER_BLOCK)), dim3(256), 0, (hipStream_t)stream, sdf, features,
                       color_act, normal, t_edges, inv_std_param, bg, n_rays, S, weights, opacity, depth, d_comp_rgb, d_rgb_fg, d_opacity, d_depth,
                       d_z_var, d_weights, d_comp_normal, d_sdf, d_features, d_bg, d_inv_std_param ? dp_partial : (float*)nullptr);
    if (d_inv_std_param) sdf_dp_reduce(dp_partial, n_rays, inv_std_param, 1, d_inv_std_param, (hipStream_t)stream);
    ASD_LAUNCH_CHECK();
    return ASD_OK;
}

}  // extern "C"
