// neus.hip — the opacity model of `neus-volume-renderer` (threestudio/models/renderers/neus_volume_renderer.py) on packed, ragged rays for
// gfx950: ray r owns the samples [offset[r], offset[r] + count[r]) of every per-sample array.
//   asd_neus_step_alpha     alpha of a fixed step around an sdf value: alpha_fn / occ_eval_fn (:139-166, :364-377)   (one thread per sample)
//   asd_neus_prune_count    asd_prune_count with that alpha formed in place: keep flags + kept count per ray          (one wave per ray)
//   asd_neus_composite_fwd  get_alpha (:93-117) -> weights and every per-ray image in ONE pass                         (one wave per ray)
//   asd_neus_composite_bwd  its gradient w.r.t. sdf, normal, features, background and the variance                     (one wave per ray + one tiny reduce)
// Roofline: bandwidth-trivial (4 096 rays x ~100 kept samples x ~60 B); what these kernels buy is launches — the composed route forms alpha
// with about fifteen elementwise launches per pass, each way.  Per sample two exponentials, one expm1 and four IEEE divisions (neus_cdfs).
// Shared with render.hip and volsdf.hip, in ray_composite.h: the learned variance read on the device and the VolSDF density, the colour
// read, the transmittance step, the per-ray images and the common part of their gradients.  This file keeps the logistic-cdf model, its
// backward recurrence, and the variance-gradient reduce both SDF renderers launch.
#include "asd_common.h"
#include "ray_composite.h"

#define NEUS_RAYS_PER_BLOCK 4     // 256 threads = 4 waves = 4 rays

// The two logistic cdf values prev = sigmoid(xp), next = sigmoid(xn) with what the opacity and its derivatives need of them.  `delta` is
// xp - xn formed WITHOUT the subtraction (step a, or -iter_cos dt a).  The opacity lives on D = prev - next, the difference of two numbers
// that agree to a few per cent: formed from the rounded cdfs it carries their 6e-8 as ~1e-6 of D, and the derivative w.r.t. the variance
// (s - h) prev' - (s + h) next' loses another factor |s / h|.  With E = exp(-x): D = E_p expm1(delta) / ((1 + E_p)(1 + E_n)) and
// 1 - sigmoid(x) = E / (1 + E) have no cancellation; they are used where the difference is small (|delta| < 1) and the exponentials finite.
struct neus_cdf {
    float prev, next;   // the cdfs
    float omp, omn;     // 1 - prev, 1 - next
    float D;            // prev - next
};

__device__ __forceinline__ neus_cdf neus_cdfs(float xp, float xn, float delta) {
    const float Ep = expf(-xp), En = expf(-xn);
    neus_cdf c;
    c.prev = 1.f / (1.f + Ep);
    c.next = 1.f / (1.f + En);
    const bool fin = Ep < 1.0e18f && En < 1.0e18f;      // (1 + Ep)(1 + En) stays finite; beyond it both cdfs are below 1e-18 next to the 1e-5 of the ratio
    c.omp = fin ? Ep / (1.f + Ep) : 1.f - c.prev;
    c.omn = fin ? En / (1.f + En) : 1.f - c.next;
    c.D = (fin && fabsf(delta) < 1.f) ? Ep * expm1f(delta) / ((1.f + Ep) * (1.f + En)) : c.prev - c.next;
    return c;
}

// q = (prev - next + 1e-5) / (prev + 1e-5), before the clip
__device__ __forceinline__ float neus_ratio(const neus_cdf& c) { return (c.D + 1e-5f) / (c.prev + 1e-5f); }

// alpha of a sample of length `step` met head-on (alpha_fn, :154-164)
__device__ __forceinline__ float neus_step_alpha_of(float s, float a, float step, int use_volsdf) {
    if (use_volsdf) {
        float sg, em1;
        return step * volsdf_sigma(s, a, sg, em1);
    }
    const float q = neus_ratio(neus_cdfs((s + step * 0.5f) * a, (s - step * 0.5f) * a, step * a));
    return fminf(fmaxf(q, 0.f), 1.f);
}

// iter_cos of get_alpha (:98-104) from true_cos = dirs . normal; k = cos_anneal_ratio
__device__ __forceinline__ float neus_iter_cos(float c, float k) {
    return -(fmaxf(-c * 0.5f + 0.5f, 0.f) * (1.0f - k) + fmaxf(-c, 0.f) * k);
}

// alpha of sample i as the compositing pass forms it (get_alpha)
__device__ __forceinline__ float neus_sample_alpha(const float* __restrict__ sdf, const float* __restrict__ normal, const float* __restrict__ dirs,
                                                   size_t i, float dt, float a, float k, int use_volsdf) {
    const float s = sdf[i];
    if (use_volsdf) {
        float sg, em1;
        return fabsf(dt) * volsdf_sigma(s, a, sg, em1);
    }
    const float c = dirs[3 * i] * normal[3 * i] + dirs[3 * i + 1] * normal[3 * i + 1] + dirs[3 * i + 2] * normal[3 * i + 2];
    const float ic = neus_iter_cos(c, k);
    const float half = ic * dt * 0.5f;
    const float q = neus_ratio(neus_cdfs((s - half) * a, (s + half) * a, -(ic * dt) * a));
    return fminf(fmaxf(q, 0.f), 1.f);
}

// ---- sampling -----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void neus_step_alpha_kernel(const float* __restrict__ sdf, int n, const int* __restrict__ n_dev,
                                                              const float* __restrict__ p, float step, int use_volsdf, float* __restrict__ alpha) {
    const int live = n_dev ? min(n_dev[0], n) : n;
    const sdf_var v = sdf_variance(p, use_volsdf);
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < live; i += (long long)gridDim.x * 256)
        alpha[i] = neus_step_alpha_of(sdf[i], v.a, step, use_volsdf);
}

// prune_kernel of render.hip on alphas: T_i = prod_{k<i} (1 - alpha_k) (nerfacc render_visibility_from_alpha)
__global__ __launch_bounds__(256) void neus_prune_kernel(const float* __restrict__ sdf, const int* __restrict__ offset, const int* __restrict__ count,
                                                         int n_rays, const float* __restrict__ p, float step, int use_volsdf, float early_stop_eps,
                                                         float alpha_thre, uint8_t* __restrict__ keep, int* __restrict__ kept_count) {
    const int r = blockIdx.x * NEUS_RAYS_PER_BLOCK + (threadIdx.x >> 6);
    if (r >= n_rays) return;
    const int lane = asd_lane();
    const int b = offset[r], cnt = count[r];
    const sdf_var v = sdf_variance(p, use_volsdf);
    float carry = 1.f;
    int kept = 0;
    for (int j0 = 0; j0 < cnt; j0 += 64) {
        const int j = j0 + lane;
        const bool valid = j < cnt;
        const float alpha = valid ? neus_step_alpha_of(sdf[(size_t)b + j], v.a, step, use_volsdf) : 0.f;
        const float T = ray_trans_step(alpha, carry);
        const bool k = valid && (T >= early_stop_eps) && (alpha >= alpha_thre);
        if (valid) keep[(size_t)b + j] = (uint8_t)k;
        kept += __popcll(__ballot(k));
    }
    if (lane == 0) kept_count[r] = kept;
}

// ---- compositing --------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void neus_composite_fwd_kernel(
    const float* __restrict__ sdf, const float* __restrict__ normal, const float* __restrict__ dirs, const float* __restrict__ t_start,
    const float* __restrict__ t_end, const float* __restrict__ feat, int color_act, const float* __restrict__ p, float k_anneal, int use_volsdf,
    const float* __restrict__ bg, const int* __restrict__ offset, const int* __restrict__ count, int n_rays, float* __restrict__ weights,
    float* __restrict__ opacity, float* __restrict__ depth, float* __restrict__ rgb_fg, float* __restrict__ comp_rgb,
    float* __restrict__ comp_normal) {
    const int r = blockIdx.x * NEUS_RAYS_PER_BLOCK + (threadIdx.x >> 6);
    if (r >= n_rays) return;
    const int lane = asd_lane();
    const int cnt = count[r];
    const size_t b = (size_t)offset[r];
    const sdf_var v = sdf_variance(p, use_volsdf);
    float carry = 1.f;
    ray_images img;
    ray_normal nrm;
    for (int j0 = 0; j0 < cnt; j0 += 64) {
        const int j = j0 + lane;
        const bool valid = j < cnt;
        const size_t i = b + j;
        float alpha = 0.f, tm = 0.f;
        if (valid) {
            const float t0 = t_start[i], t1 = t_end[i];
            alpha = neus_sample_alpha(sdf, normal, dirs, i, t1 - t0, v.a, k_anneal, use_volsdf);
            tm = (t0 + t1) / 2.0f;
        }
        const float T = ray_trans_step(alpha, carry);
        if (valid) {
            const float w = T * alpha;
            weights[i] = w;
            img.add(w, tm, feat, i, color_act);
            if (comp_normal) nrm.add(w, normal, i);
        }
    }
    img.reduce();
    if (comp_normal) nrm.reduce();
    if (lane == 0) {
        img.store(r, bg, opacity, depth, rgb_fg, comp_rgb);
        if (comp_normal) nrm.store(r, img.op, comp_normal);
    }
}

// Backward.  With gw_i = dL/dw_i (the four images and the weights themselves), w_j = alpha_j prod_{k<j} (1 - alpha_k):
//   dL/dalpha_i = T_i (gw_i - R_i),   R_i = sum_{j>i} gw_j alpha_j prod_{i<k<j} (1 - alpha_k)
// R is the usual "what lies behind this sample" term WITHOUT its division by (1 - alpha_i): the NeuS alpha is clipped to [0, 1] and reaches 1
// exactly (a cdf that underflows), where w_j / (1 - alpha_i) is 0 / 0.  R obeys R_i = gw_{i+1} alpha_{i+1} + (1 - alpha_{i+1}) R_{i+1},
// R_last = 0: a scan of affine maps x -> b + m x from the FAR end of the ray (pass 1, walking the trips backwards; R_i waits in d_sdf, every
// lane reads back what it wrote itself).  Pass 2 walks near to far, forms T again and the chain rule through get_alpha:
//   NeuS    q = (D + 1e-5) / (prev + 1e-5) = 1 - next / den, D = prev - next, den = prev + 1e-5; dL/dq = dL/dalpha on 0 <= q <= 1, else 0
//           with r = prev / den, A = (1 - next) - r (1 - prev) = D + (1 - prev) 1e-5 / den, B = (1 - next) + r (1 - prev), h = iter_cos dt / 2:
//           dq/dsdf = -a (next / den) A,  dq/da = -(next / den) (A sdf + B h),  dq/dh = -a (next / den) B
//           (the chain through prev (1 - prev) and next (1 - next), regrouped so that no two nearly equal products are subtracted)
//           d iter_cos / d true_cos = 0.5 (1 - k) [0.5 - 0.5 c > 0] + k [-c > 0],  dL/dnormal = dL/dtrue_cos dirs
//   VolSDF  as asd_volsdf_composite_bwd: dsigma/ds = -a^2 e / 2 (0 at s = 0), dsigma/da = 0.5 + 0.5 sign(s) expm1(-|s| a) - a s e / 2
// dp_partial[r] receives the ray's part of dL/da (a wave sum: no atomics), neus_dp_reduce_kernel adds the rays in a fixed order.
__device__ __forceinline__ void neus_wave_suffix_affine(float& m, float& b) {
    const int lane = asd_lane();
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const float m2 = __shfl_down(m, o, 64), b2 = __shfl_down(b, o, 64);
        if (lane + o < 64) {        // F_l <- F_l o F_{l+o}
            b = fmaf(m, b2, b);
            m *= m2;
        }
    }
}

__global__ __launch_bounds__(256) void neus_composite_bwd_kernel(
    const float* __restrict__ sdf, const float* __restrict__ normal, const float* __restrict__ dirs, const float* __restrict__ t_start,
    const float* __restrict__ t_end, const float* __restrict__ feat, int color_act, const float* __restrict__ p, float k_anneal, int use_volsdf,
    const float* __restrict__ bg, const int* __restrict__ offset, const int* __restrict__ count, int n_rays, const float* __restrict__ weights,
    const float* __restrict__ opacity, const float* __restrict__ d_comp_rgb, const float* __restrict__ d_rgb_fg, const float* __restrict__ d_opacity,
    const float* __restrict__ d_depth, const float* __restrict__ d_weights, float* __restrict__ d_sdf, float* __restrict__ d_normal,
    float* __restrict__ d_feat, float* __restrict__ d_bg, float* __restrict__ dp_partial) {
    const int r = blockIdx.x * NEUS_RAYS_PER_BLOCK + (threadIdx.x >> 6);
    if (r >= n_rays) return;
    const int lane = asd_lane();
    const int cnt = count[r];
    const size_t b = (size_t)offset[r];
    const sdf_var v = sdf_variance(p, use_volsdf);
    ray_grads g;
    g.load(r, d_comp_rgb, d_rgb_fg, d_opacity, d_depth, bg, opacity[r], d_bg);
    // pass 1, far to near: R_i
    float carry_r = 0.f;
    for (int j0 = cnt > 0 ? ((cnt - 1) / 64) * 64 : -1; j0 >= 0; j0 -= 64) {
        const int j = j0 + lane;
        const bool valid = j < cnt;
        const size_t i = b + j;
        float m = 1.f, c = 0.f;     // the identity map behind the end of the ray
        if (valid) {
            const float t0 = t_start[i], t1 = t_end[i];
            const float col[3] = {ray_colour(feat, i, 0, color_act), ray_colour(feat, i, 1, color_act), ray_colour(feat, i, 2, color_act)};
            const float alpha = neus_sample_alpha(sdf, normal, dirs, i, t1 - t0, v.a, k_anneal, use_volsdf);
            m = 1.f - alpha;
            c = g.gw(i, (t0 + t1) / 2.0f, col, d_weights) * alpha;
        }
        neus_wave_suffix_affine(m, c);
        float m_behind = __shfl_down(m, 1, 64), c_behind = __shfl_down(c, 1, 64);     // the lanes behind this one
        if (lane == 63) { m_behind = 1.f; c_behind = 0.f; }
        if (valid) d_sdf[i] = fmaf(m_behind, carry_r, c_behind);
        carry_r = fmaf(__shfl(m, 0, 64), carry_r, __shfl(c, 0, 64));
    }
    // pass 2, near to far: the transmittances again, the gradients
    float carry_t = 1.f, dpa = 0.f;
    for (int j0 = 0; j0 < cnt; j0 += 64) {
        const int j = j0 + lane;
        const bool valid = j < cnt;
        const size_t i = b + j;
        float alpha = 0.f, s = 0.f, dt = 0.f, gw = 0.f, R = 0.f, w = 0.f;
        float q = 0.f, half = 0.f, cosv = 0.f, sg = 0.f, em1 = 0.f;
        neus_cdf cd = {0.f, 0.f, 0.f, 0.f, 0.f};
        float col[3] = {0.f, 0.f, 0.f};
        if (valid) {
            const float t0 = t_start[i], t1 = t_end[i];
            dt = t1 - t0;
            s = sdf[i];
            if (use_volsdf) {
                alpha = fabsf(dt) * volsdf_sigma(s, v.a, sg, em1);
            } else {
                cosv = dirs[3 * i] * normal[3 * i] + dirs[3 * i + 1] * normal[3 * i + 1] + dirs[3 * i + 2] * normal[3 * i + 2];
                const float ic = neus_iter_cos(cosv, k_anneal);
                half = ic * dt * 0.5f;
                cd = neus_cdfs((s - half) * v.a, (s + half) * v.a, -(ic * dt) * v.a);
                q = neus_ratio(cd);
                alpha = fminf(fmaxf(q, 0.f), 1.f);
            }
            w = weights[i];
            R = d_sdf[i];
#pragma unroll
            for (int k = 0; k < 3; ++k) col[k] = ray_colour(feat, i, k, color_act);
            gw = g.gw(i, (t0 + t1) / 2.0f, col, d_weights);
        }
        const float T = ray_trans_step(alpha, carry_t);
        if (valid) {
            const float da = T * (gw - R);
            float dn = 0.f;
            if (use_volsdf) {
                const float beta = 1.f / v.a;
                const float e = expf(-fabsf(s) / beta);       // (not em1 + 1: far from the surface that sum has no digits left)
                const float adt = fabsf(dt);
                d_sdf[i] = da * adt * (-0.5f * v.a * v.a * e * sg * sg);
                dpa = fmaf(da * adt, (0.5f + 0.5f * sg * em1) - 0.5f * v.a * s * e, dpa);
            } else {
                const float dq = (q >= 0.f && q <= 1.f) ? da : 0.f;
                const float den = cd.prev + 1e-5f;
                const float nd = -dq * (cd.next / den), r = cd.prev / den;
                const float A = cd.D + cd.omp * (1e-5f / den);      // (1 - next) - r (1 - prev)
                const float B = cd.omn + r * cd.omp;
                d_sdf[i] = nd * A * v.a;
                dpa += nd * fmaf(A, s, half * B);
                const float d_ic = nd * B * v.a * dt * 0.5f;
                dn = d_ic * ((-cosv * 0.5f + 0.5f > 0.f ? 0.5f * (1.0f - k_anneal) : 0.f) + (-cosv > 0.f ? k_anneal : 0.f));
            }
            if (d_normal) {
                d_normal[3 * i] = dn * dirs[3 * i];
                d_normal[3 * i + 1] = dn * dirs[3 * i + 1];
                d_normal[3 * i + 2] = dn * dirs[3 * i + 2];
            }
            g.store_d_feat(d_feat, i, w, col, color_act);
        }
    }
    if (dp_partial) {
        dpa = asd_wave_sum(dpa);
        if (lane == 0) dp_partial[r] = dpa;
    }
}

// d_p[0] = (sum_r dp_partial[r]) da/dp: one block, every thread a fixed strided subset, a fixed tree above — the same bits every run.
// Behind sdf_dp_reduce (ray_composite.h) for this file's backward pass and for asd_volsdf_composite_bwd.
__global__ __launch_bounds__(1024) void neus_dp_reduce_kernel(const float* __restrict__ dp_partial, int n_rays, const float* __restrict__ p,
                                                              int use_volsdf, float* __restrict__ d_p) {
    __shared__ double ws[1024];
    double acc = 0.0;
    for (int i = threadIdx.x; i < n_rays; i += 1024) acc += (double)dp_partial[i];
    ws[threadIdx.x] = acc;
    __syncthreads();
    for (int o = 512; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) ws[threadIdx.x] += ws[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) d_p[0] = (float)(ws[0] * (double)sdf_variance(p, use_volsdf).dadp);
}

void sdf_dp_reduce(const float* dp_partial, int n_rays, const float* p, int use_volsdf, float* d_p, hipStream_t stream) {
    hipLaunchKernelGGL(neus_dp_reduce_kernel, dim3(1), dim3(1024), 0, stream, dp_partial, n_rays, p, use_volsdf, d_p);
}

extern "C" {

int asd_neus_step_alpha(const float* sdf, int32_t n, const int32_t* n_dev, const float* inv_std_param, float step, int32_t use_volsdf, float* alpha,
                        void* stream) {
    ASD_CHECK_ARG(sdf && inv_std_param && alpha, "null argument");
    ASD_CHECK_ARG(n >= 0, "n must not be negative");
    if (n == 0) return ASD_OK;
    hipLaunchKernelGGL(neus_step_alpha_kernel, dim3(asd_grid_for(n, 256)), dim3(256), 0, (hipStream_t)stream, sdf, n, n_dev, inv_std_param, step,
                       use_volsdf != 0, alpha);
    ASD_LAUNCH_CHECK();
    return ASD_OK;
}

int asd_neus_prune_count(const float* sdf, const int32_t* offset, const int32_t* count, int32_t n_rays, const float* inv_std_param, float step,
                         int32_t use_volsdf, float early_stop_eps, float alpha_thre, uint8_t* keep, int32_t* kept_count, void* stream) {
    ASD_CHECK_ARG(sdf && offset && count && inv_std_param && keep && kept_count, "null argument");
    ASD_CHECK_ARG(n_rays >= 0, "n_rays must not be negative");
    if (n_rays == 0) return ASD_OK;
    hipLaunchKernelGGL(neus_prune_kernel, dim3(asd_div_up(n_rays, NEUS_RAYS_PER_BLOCK)), dim3(256), 0, (hipStream_t)stream, sdf, offset, count, n_rays,
                       inv_std_param, step, use_volsdf != 0, early_stop_eps, alpha_thre, keep, kept_count);
    ASD_LAUNCH_CHECK();
    return ASD_OK;
}

int asd_neus_composite_fwd(const float* sdf, const float* normal, const float* dirs, const float* t_start, const float* t_end, const float* features,
                           int32_t color_act, const float* inv_std_param, float cos_anneal_ratio, int32_t use_volsdf, const float* bg,
                           const int32_t* offset, const int32_t* count, int32_t n_rays, float* weights, float* opacity, float* depth, float* rgb_fg,
                           float* comp_rgb, float* comp_normal, void* stream) {
    ASD_CHECK_ARG(sdf && normal && dirs && t_start && t_end && features && inv_std_param && bg && offset && count, "null argument");
    ASD_CHECK_ARG(weights && opacity && depth && rgb_fg && comp_rgb, "null output");
    ASD_CHECK_ARG(n_rays >= 0, "n_rays must not be negative");
    ASD_CHECK_ARG(color_act == 0 || color_act == 1, "color_act: 0 (features are colours) or 1 (sigmoid)");
    if (n_rays == 0) return ASD_OK;
    hipLaunchKernelGGL(neus_composite_fwd_kernel, dim3(asd_div_up(n_rays, NEUS_RAYS_PER_BLOCK)), dim3(256), 0, (hipStream_t)stream, sdf, normal, dirs,
                       t_start, t_end, features, color_act, inv_std_param, cos_anneal_ratio, use_volsdf != 0, bg, offset, count, n_rays, weights, opacity,
                       depth, rgb_fg, comp_rgb, comp_normal);
    ASD_LAUNCH_CHECK();
    return ASD_OK;
}

int asd_neus_composite_bwd(const float* sdf, const float* normal, const float* dirs, const float* t_start, const float* t_end, const float* features,
                           int32_t color_act, const float* inv_std_param, float cos_anneal_ratio, int32_t use_volsdf, const float* bg,
                           const int32_t* offset, const int32_t* count, int32_t n_rays, const float* weights, const float* opacity,
                           const float* d_comp_rgb, const float* d_rgb_fg, const float* d_opacity, const float* d_depth, const float* d_weights,
                           float* d_sdf, float* d_normal, float* d_features, float* d_bg, float* d_inv_std_param, float* dp_partial, void* stream) {
    ASD_CHECK_ARG(sdf && normal && dirs && t_start && t_end && features && inv_std_param && bg && offset && count, "null argument");
    ASD_CHECK_ARG(weights && opacity, "null forward output");
    ASD_CHECK_ARG(d_sdf && d_features, "null gradient output");
    ASD_CHECK_ARG(!d_inv_std_param || dp_partial, "the variance gradient needs its [n_rays] partial-sum buffer");
    ASD_CHECK_ARG(n_rays >= 0, "n_rays must not be negative");
    ASD_CHECK_ARG(color_act == 0 || color_act == 1, "color_act: 0 (features are colours) or 1 (sigmoid)");
    if (n_rays == 0) return ASD_OK;
    hipLaunchKernelGGL(neus_composite_bwd_kernel, dim3(asd_div_up(n_rays, NEUS_RAYS_PER_BLOCK)), dim3(256), 0, (hipStream_t)stream, sdf, normal, dirs,
                       t_start, t_end, features, color_act, inv_std_param, cos_anneal_ratio, use_volsdf != 0, bg, offset, count, n_rays, weights, opacity,
                       d_comp_rgb, d_rgb_fg, d_opacity, d_depth, d_weights, d_sdf, d_normal, d_features, d_bg,
                       d_inv_std_param ? dp_partial : (float*)nullptr);
    if (d_inv_std_param) sdf_dp_reduce(dp_partial, n_rays, inv_std_param, use_volsdf != 0, d_inv_std_param, (hipStream_t)stream);
    ASD_LAUNCH_CHECK();
    return ASD_OK;
}

}  // extern "C"
