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
// The learned variance is read on the device from the raw parameter p: a = clamp(clamp(exp(10 p), 1e-6, 1e6), 0, 80)
// (LearnedVariance.forward + volsdf_density, neus_volume_renderer.py:19-23,31-44).
#include "asd_common.h"

#define VOLSDF_RAYS_PER_BLOCK 4     // 256 threads = 4 waves = 4 rays
#define VOLSDF_MAX_CDF_SAMPLES 2048 // asd_volsdf_proposal_cdf keeps one float per sample of its 4 rays in LDS (32 KB)

struct volsdf_var {
    float a;        // the clamped inverse standard deviation the density uses
    float beta;     // 1 / a: the density divides by it, as the reference does
    float dadp;     // d a / d p: 10 exp(10 p) where neither clamp is active (torch.clamp passes the gradient on the closed interval), else 0
};

__device__ __forceinline__ volsdf_var volsdf_variance(const float* __restrict__ p) {
    const float raw = expf(p[0] * 10.0f);
    const float a1 = fminf(fmaxf(raw, 1.0e-6f), 1.0e6f);
    volsdf_var v;
    v.a = fminf(fmaxf(a1, 0.f), 80.f);
    v.beta = 1.f / v.a;
    v.dadp = (raw >= 1.0e-6f && raw <= 80.f) ? 10.0f * raw : 0.f;
    return v;
}

// sigma = a (0.5 + 0.5 sign(s) expm1(-|s| / beta)) in the reference's operation order; em1 = expm1(-|s| / beta), sg = sign(s)
__device__ __forceinline__ float volsdf_sigma(float s, const volsdf_var& v, float& sg, float& em1) {
    sg = s > 0.f ? 1.f : (s < 0.f ? -1.f : 0.f);
    em1 = expm1f(-fabsf(s) / v.beta);
    return v.a * (0.5f + 0.5f * sg * em1);
}

__device__ __forceinline__ float volsdf_colour(const float* __restrict__ f, size_t i, int k, int act) {
    const float v = f[3 * i + k];
    return act == 1 ? 1.f / (1.f + expf(-v)) : v;
}

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
        const volsdf_var v = volsdf_variance(p);
        for (int j = lane; j < S; j += 64) {
            float sg, em1;
            acc_s[j] = volsdf_sigma(sdf[(size_t)r * S + j], v, sg, em1);
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
    const volsdf_var v = volsdf_variance(p);
    float carry = 1.f;
    float op = 0.f, dp = 0.f, c0 = 0.f, c1 = 0.f, c2 = 0.f, n0 = 0.f, n1 = 0.f, n2 = 0.f;
    for (int j0 = 0; j0 < S; j0 += 64) {
        const int j = j0 + lane;
        const bool valid = j < S;
        const size_t i = b + j;
        float alpha = 0.f, tm = 0.f;
        if (valid) {
            const float t0 = t[j], t1 = t[j + 1];
            float sg, em1;
            alpha = fabsf(t1 - t0) * volsdf_sigma(sdf[i], v, sg, em1);
            tm = (t0 + t1) * 0.5f;
        }
        const float incl = asd_wave_incl_prod(1.f - alpha);
        float excl = __shfl_up(incl, 1, 64);      // exclusive product: the inclusive scan shifted by one lane
        if (lane == 0) excl = 1.f;
        const float T = carry * excl;
        carry *= __shfl(incl, 63, 64);
        if (valid) {
            const float w = T * alpha;
            weights[i] = w;
            op += w;
            dp = fmaf(w, tm, dp);
            c0 = fmaf(w, volsdf_colour(feat, i, 0, color_act), c0);
            c1 = fmaf(w, volsdf_colour(feat, i, 1, color_act), c1);
            c2 = fmaf(w, volsdf_colour(feat, i, 2, color_act), c2);
            if (normal) {
                n0 = fmaf(w, normal[3 * i], n0);
                n1 = fmaf(w, normal[3 * i + 1], n1);
                n2 = fmaf(w, normal[3 * i + 2], n2);
            }
        }
    }
    op = asd_wave_sum(op); dp = asd_wave_sum(dp);
    c0 = asd_wave_sum(c0); c1 = asd_wave_sum(c1); c2 = asd_wave_sum(c2);
    // z_variance = sum_i w_i (t_i - depth)^2, unnormalised and unmasked (generative_space_volsdf_volume_renderer.py:380-385); every lane
    // reads back the weights it wrote itself
    float zv = 0.f;
    for (int j = lane; j < S; j += 64) {
        const float tm = (t[j] + t[j + 1]) * 0.5f;
        zv = fmaf(weights[b + j], (tm - dp) * (tm - dp), zv);
    }
    zv = asd_wave_sum(zv);
    if (normal) { n0 = asd_wave_sum(n0); n1 = asd_wave_sum(n1); n2 = asd_wave_sum(n2); }
    if (lane == 0) {
        opacity[r] = op;
        depth[r] = dp;
        z_var[r] = zv;
        rgb_fg[3 * (size_t)r] = c0; rgb_fg[3 * (size_t)r + 1] = c1; rgb_fg[3 * (size_t)r + 2] = c2;
        const float k = 1.f - op;
        comp_rgb[3 * (size_t)r] = c0 + bg[3 * (size_t)r] * k;
        comp_rgb[3 * (size_t)r + 1] = c1 + bg[3 * (size_t)r + 1] * k;
        comp_rgb[3 * (size_t)r + 2] = c2 + bg[3 * (size_t)r + 2] * k;
        if (normal) {       // lerp(0, (F.normalize(sum_i w_i n_i) + 1) / 2, opacity)
            const float len = fmaxf(sqrtf(n0 * n0 + n1 * n1 + n2 * n2), 1e-12f);
            comp_normal[3 * (size_t)r] = (n0 / len + 1.0f) * 0.5f * op;
            comp_normal[3 * (size_t)r + 1] = (n1 / len + 1.0f) * 0.5f * op;
            comp_normal[3 * (size_t)r + 2] = (n2 / len + 1.0f) * 0.5f * op;
        }
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
// dp_partial[r] receives the ray's part of dL/da (a wave sum: no atomics), volsdf_dp_reduce_kernel adds the rays in a fixed order.
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
    const volsdf_var v = volsdf_variance(p);
    const float op = opacity[r], zm = depth[r];
    float G[3], gop = d_opacity ? d_opacity[r] : 0.f;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float gc = d_comp_rgb ? d_comp_rgb[3 * (size_t)r + k] : 0.f;
        G[k] = gc + (d_rgb_fg ? d_rgb_fg[3 * (size_t)r + k] : 0.f);
        gop -= gc * bg[3 * (size_t)r + k];
        if (d_bg && lane == 0) d_bg[3 * (size_t)r + k] = gc * (1.f - op);
    }
    const float gdp = d_depth ? d_depth[r] : 0.f;
    const float gzv = d_z_var ? d_z_var[r] : 0.f;
    if (normal && d_comp_normal) {      // d opacity += d comp_normal . (normalize(sum_i w_i n_i) + 1) / 2
        float n0 = 0.f, n1 = 0.f, n2 = 0.f;
        for (int j = lane; j < S; j += 64) {
            const size_t i = b + j;
            const float w = weights[i];
            n0 = fmaf(w, normal[3 * i], n0);
            n1 = fmaf(w, normal[3 * i + 1], n1);
            n2 = fmaf(w, normal[3 * i + 2], n2);
        }
        n0 = asd_wave_sum(n0); n1 = asd_wave_sum(n1); n2 = asd_wave_sum(n2);
        const float len = fmaxf(sqrtf(n0 * n0 + n1 * n1 + n2 * n2), 1e-12f);
        gop = fmaf(d_comp_normal[3 * (size_t)r], (n0 / len + 1.0f) * 0.5f, gop);
        gop = fmaf(d_comp_normal[3 * (size_t)r + 1], (n1 / len + 1.0f) * 0.5f, gop);
        gop = fmaf(d_comp_normal[3 * (size_t)r + 2], (n2 / len + 1.0f) * 0.5f, gop);
    }
    auto gw_of = [&](size_t i, float tm, const float (&col)[3]) {
        float gw = gop + gdp * tm + (d_weights ? d_weights[i] : 0.f);
        gw = fmaf(G[0], col[0], gw);
        gw = fmaf(G[1], col[1], gw);
        gw = fmaf(G[2], col[2], gw);
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
            const float col[3] = {volsdf_colour(feat, i, 0, color_act), volsdf_colour(feat, i, 1, color_act), volsdf_colour(feat, i, 2, color_act)};
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
            alpha = dt * volsdf_sigma(s, v, sg, em1);
            w = weights[i];
            Ssuf = d_sdf[i];
#pragma unroll
            for (int k = 0; k < 3; ++k) col[k] = volsdf_colour(feat, i, k, color_act);
            gw = gw_of(i, (t0 + t1) * 0.5f, col);
        }
        const float om = 1.f - alpha;
        const float incl_t = asd_wave_incl_prod(om);
        float excl = __shfl_up(incl_t, 1, 64);
        if (lane == 0) excl = 1.f;
        const float T = carry_t * excl;
        carry_t *= __shfl(incl_t, 63, 64);
        if (valid) {
            // d w_j / d alpha_i = -w_j / (1 - alpha_i) for j > i holds for either sign of 1 - alpha_i (alpha is not clamped); only a
            // factor of exactly zero has no quotient form, and is kept away from it
            const float om_safe = fabsf(om) < 1e-10f ? copysignf(1e-10f, om) : om;
            const float da = T * gw - Ssuf / om_safe;
            const float e = expf(-fabsf(s) / v.beta);       // (not em1 + 1: far from the surface that sum has no digits left)
            d_sdf[i] = da * dt * (-0.5f * v.a * v.a * e * sg * sg);
            dpa = fmaf(da * dt, (0.5f + 0.5f * sg * em1) - 0.5f * v.a * s * e, dpa);
#pragma unroll
            for (int k = 0; k < 3; ++k) d_feat[3 * i + k] = w * G[k] * (color_act == 1 ? col[k] * (1.f - col[k]) : 1.f);
        }
    }
    if (dp_partial) {
        dpa = asd_wave_sum(dpa);
        if (lane == 0) dp_partial[r] = dpa;
    }
}

// d_p[0] = (sum_r dp_partial[r]) da/dp: one block, every thread a fixed strided subset, a fixed tree above — the same bits every run
__global__ __launch_bounds__(1024) void volsdf_dp_reduce_kernel(const float* __restrict__ dp_partial, int n_rays, const float* __restrict__ p,
                                                                float* __restrict__ d_p) {
    __shared__ double ws[1024];
    double acc = 0.0;
    for (int i = threadIdx.x; i < n_rays; i += 1024) acc += (double)dp_partial[i];
    ws[threadIdx.x] = acc;
    __syncthreads();
    for (int o = 512; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) ws[threadIdx.x] += ws[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) d_p[0] = (float)(ws[0] * (double)volsdf_variance(p).dadp);
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
    if (d_inv_std_param)
        hipLaunchKernelGGL(volsdf_dp_reduce_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, dp_partial, n_rays, inv_std_param, d_inv_std_param);
    ASD_LAUNCH_CHECK();
    return ASD_OK;
}

}  // extern "C"
