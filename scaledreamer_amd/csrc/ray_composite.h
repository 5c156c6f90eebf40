// ray_composite.h — what the "one wave per ray" compositing kernels of render.hip, neus.hip and volsdf.hip share: the colour read, the
// transmittance step, the per-ray images and their gradients' common part, and the learned variance of the two SDF renderers.  Device
// code only, every function inlined; every floating-point operation stands in the order the oracle comparison depends on.
// What differs stays in the kernels: the alpha model, the z-variance, and the three backward recurrences (each explained where it is).
#pragma once
#include "asd_common.h"

// colour of sample i, channel k: `f` holds activated colours, or — act == 1 — the raw features of a material that is
// colour = sigmoid(features) (NoMaterial, no_material.py:41-54): the activation and its gradient then ride in the compositing kernels
__device__ __forceinline__ float ray_colour(const float* __restrict__ f, size_t i, int k, int act) {
    const float v = f[3 * i + k];
    return act == 1 ? 1.f / (1.f + expf(-v)) : v;
}

// T_i = prod_{k<i} (1 - alpha_k) (nerfacc render_transmittance_from_alpha) for this lane's sample of a 64-sample trip: the inclusive wave
// product shifted by one lane, times `carry`, the product over the trips before; carry then takes this trip in.  A lane without a sample
// passes alpha = 0.
__device__ __forceinline__ float ray_trans_step(float alpha, float& carry) {
    const float incl = asd_wave_incl_prod(1.f - alpha);
    float excl = __shfl_up(incl, 1, 64);
    if (asd_lane() == 0) excl = 1.f;
    const float T = carry * excl;
    carry *= __shfl(incl, 63, 64);
    return T;
}

// opacity = sum w, depth = sum w t, rgb_fg = sum w colour (accumulate_along_rays), comp_rgb = rgb_fg + bg (1 - opacity)
struct ray_images {
    float op = 0.f, dp = 0.f, c[3] = {0.f, 0.f, 0.f};
    __device__ __forceinline__ void add(float w, float tm, const float* feat, size_t i, int act) {
        op += w;
        dp = fmaf(w, tm, dp);
#pragma unroll
        for (int k = 0; k < 3; ++k) c[k] = fmaf(w, ray_colour(feat, i, k, act), c[k]);
    }
    __device__ __forceinline__ void reduce() {
        op = asd_wave_sum(op); dp = asd_wave_sum(dp);
#pragma unroll
        for (int k = 0; k < 3; ++k) c[k] = asd_wave_sum(c[k]);
    }
    // one lane per ray calls this, after reduce()
    __device__ __forceinline__ void store(size_t r, const float* bg, float* opacity, float* depth, float* rgb_fg, float* comp_rgb) const {
        opacity[r] = op;
        depth[r] = dp;
        const float k1 = 1.f - op;
#pragma unroll
        for (int k = 0; k < 3; ++k) rgb_fg[3 * r + k] = c[k];
#pragma unroll
        for (int k = 0; k < 3; ++k) comp_rgb[3 * r + k] = c[k] + bg[3 * r + k] * k1;
    }
};

// the normal image: (F.normalize(sum_i w_i n_i) + 1) / 2 * opacity (neus_volume_renderer.py:337-344; the lerp(0, ., opacity) of
// generative_space_volsdf_volume_renderer.py is the same value)
struct ray_normal {
    float n[3] = {0.f, 0.f, 0.f};
    __device__ __forceinline__ void add(float w, const float* normal, size_t i) {
#pragma unroll
        for (int k = 0; k < 3; ++k) n[k] = fmaf(w, normal[3 * i + k], n[k]);
    }
    __device__ __forceinline__ void reduce() {
#pragma unroll
        for (int k = 0; k < 3; ++k) n[k] = asd_wave_sum(n[k]);
    }
    // u = (normalize(n) + 1) / 2 with F.normalize's floor on the length, after reduce()
    __device__ __forceinline__ void shade(float (&u)[3]) const {
        const float len = fmaxf(sqrtf(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]), 1e-12f);
#pragma unroll
        for (int k = 0; k < 3; ++k) u[k] = (n[k] / len + 1.0f) * 0.5f;
    }
    __device__ __forceinline__ void store(size_t r, float op, float* comp_normal) const {
        float u[3];
        shade(u);
#pragma unroll
        for (int k = 0; k < 3; ++k) comp_normal[3 * r + k] = u[k] * op;
    }
};

// The part of dL/dw_i every compositing backward has: G = dL/drgb_fg (comp_rgb passes its own on), gop = dL/dopacity with the background
// blend's share, gdp = dL/ddepth.  load() also stores d_bg = d_comp_rgb (1 - opacity) (lane 0).  A kernel with further images (z-variance,
// the normal image) adds their terms to gop or to gw() itself.
struct ray_grads {
    float G[3], gop, gdp;
    __device__ __forceinline__ void load(size_t r, const float* d_comp_rgb, const float* d_rgb_fg, const float* d_opacity, const float* d_depth,
                                         const float* bg, float op, float* d_bg) {
        gop = d_opacity ? d_opacity[r] : 0.f;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float gc = d_comp_rgb ? d_comp_rgb[3 * r + k] : 0.f;
            G[k] = gc + (d_rgb_fg ? d_rgb_fg[3 * r + k] : 0.f);
            gop -= gc * bg[3 * r + k];
            if (d_bg && asd_lane() == 0) d_bg[3 * r + k] = gc * (1.f - op);
        }
        gdp = d_depth ? d_depth[r] : 0.f;
    }
    __device__ __forceinline__ float gw(size_t i, float tm, const float (&col)[3], const float* d_weights) const {
        float g = gop + gdp * tm + (d_weights ? d_weights[i] : 0.f);
        g = fmaf(G[0], col[0], g);
        g = fmaf(G[1], col[1], g);
        g = fmaf(G[2], col[2], g);
        return g;
    }
    // dL/dfeatures of sample i with weight w: through the sigmoid where the kernel applied it
    __device__ __forceinline__ void store_d_feat(float* d_feat, size_t i, float w, const float (&col)[3], int act) const {
#pragma unroll
        for (int k = 0; k < 3; ++k) d_feat[3 * i + k] = w * G[k] * (act == 1 ? col[k] * (1.f - col[k]) : 1.f);
    }
};

// The learned variance, read on the device from the raw parameter p: a = clamp(exp(10 p), 1e-6, 1e6) (LearnedVariance.forward,
// neus_volume_renderer.py:26-37), for VolSDF clamped to [0, 80] on top (volsdf_density, :19-23).
struct sdf_var {
    float a;        // the clamped inverse standard deviation
    float dadp;     // d a / d p: 10 exp(10 p) where no clamp is active (torch.clamp passes the gradient on the closed interval), else 0
};

__device__ __forceinline__ sdf_var sdf_variance(const float* __restrict__ p, int use_volsdf) {
    const float raw = expf(p[0] * 10.0f);
    const float a1 = fminf(fmaxf(raw, 1.0e-6f), 1.0e6f);
    sdf_var v;
    v.a = use_volsdf ? fminf(fmaxf(a1, 0.f), 80.f) : a1;
    v.dadp = (raw >= 1.0e-6f && raw <= (use_volsdf ? 80.f : 1.0e6f)) ? 10.0f * raw : 0.f;
    return v;
}

// sigma = a (0.5 + 0.5 sign(s) expm1(-|s| / beta)), beta = 1 / a, in the reference's operation order (the density divides by beta, as the
// reference does); em1 = expm1(-|s| / beta), sg = sign(s)
__device__ __forceinline__ float volsdf_sigma(float s, float a, float& sg, float& em1) {
    const float beta = 1.f / a;
    sg = s > 0.f ? 1.f : (s < 0.f ? -1.f : 0.f);
    em1 = expm1f(-fabsf(s) / beta);
    return a * (0.5f + 0.5f * sg * em1);
}

// d_p[0] = (sum_r dp_partial[r]) da/dp, the rays added in a fixed order (neus.hip holds the kernel).  Enqueues one launch; the caller checks it.
void sdf_dp_reduce(const float* dp_partial, int n_rays, const float* p, int use_volsdf, float* d_p, hipStream_t stream);
