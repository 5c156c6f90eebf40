// background.hip — the two parameter-light backgrounds of the reference on the HIP path:
//   `textured-background`    (threestudio/models/background/textured_background.py:29-54): equirect texture [C,H,W], bilinear lookup
//   `solid-color-background` (threestudio/models/background/solid_color_background.py:36-51): one colour per view
//
// Texture lookup (spherical_xyz_to_uv + F.grid_sample(bilinear, reflection, align_corners = False)):
//   u = atan2(sqrt(x^2 + y^2), z) / pi        -> WIDTH   (grid_sample reads uv[..., 0] as x)
//   v = atan2(y, x) / (2 pi) + 0.5            -> HEIGHT
//   ix = u W - 0.5, iy = v H - 0.5.  u, v lie in [0, 1], so ix lies in [-0.5, W - 0.5]: the reflection about -0.5 / W - 0.5 never
//   moves it and grid_sample's clip to [0, W - 1] is a clamp of ix; the +1 neighbour of the last texel has weight 0 and is clamped too.
//   The texture does not wrap at the azimuth seam (v = 0 and v = 1 are different rows), as in the reference.
//
// Texture gradient: a camera's rays cover a small solid angle, so a whole view lands on a handful of texels (thousands of rays on
// one texel): per-ray global float atomics would all meet on one row.  Every workgroup therefore keeps a private fp32 copy of the
// gradient image in LDS, adds its contiguous slice of rays into it (ds_add_f32) and stores the copy as a slab of the workspace; a second
// pass sums the slabs per texel in slab order.  No memset, no global atomics.  One workgroup (small n): the copy is the result.
// Gradient images beyond BG_LDS_BUDGET (textures larger than 128 KiB of fp32) take global atomics into a zeroed d_texture: the
// contention falls as the texture grows.
#include "asd_common.h"

#define BG_MAX_C 8
#define BG_LDS_BUDGET (128 * 1024)      // bytes of the LDS gradient image; the CU has 160 KiB
#define BG_BLOCK 256
// The LDS pass's time is its LDS float adds, serial per CU: ~24 ns per ray of 3 channels measured, whatever the workgroup's size (1024 threads on
// 1024 rays: 25 us; 256 on 512: 15.5 us).  So the rays are spread over workgroups — one ray per thread up to BG_FEW_SLABS slabs, which the sum
// pass reads in the time of its launch; then 64 slabs until a workgroup holds BG_RAYS_PER_WG_MANY rays, then more slabs up to BG_MAX_SLABS.
#define BG_RAYS_PER_WG 256
#define BG_FEW_SLABS 64
#define BG_RAYS_PER_WG_MANY 1024
#define BG_MAX_SLABS 256
#define BG_PI_F 3.14159265358979323846f

enum { BG_ACT_NONE = 0, BG_ACT_SIGMOID = 1 };

// the four texels of a direction and the bilinear fractions
struct bg_tap {
    int x0, x1, y0, y1;
    float wx, wy;
};
__device__ __forceinline__ bg_tap bg_tap_of(float x, float y, float z, int H, int W) {
    const float xy = sqrtf(fmaf(x, x, y * y));
    const float u = atan2f(xy, z) / BG_PI_F;
    const float v = atan2f(y, x) / (2.f * BG_PI_F) + 0.5f;
    // fmaxf / fminf drop a NaN operand: a NaN direction reads texel 0 and every index stays inside the image
    const float ix = fminf(fmaxf(fmaf(u, (float)W, -0.5f), 0.f), (float)(W - 1));
    const float iy = fminf(fmaxf(fmaf(v, (float)H, -0.5f), 0.f), (float)(H - 1));
    const float fx = floorf(ix), fy = floorf(iy);
    bg_tap t;
    t.x0 = (int)fx; t.y0 = (int)fy;
    t.x1 = t.x0 + 1 < W ? t.x0 + 1 : W - 1;
    t.y1 = t.y0 + 1 < H ? t.y0 + 1 : H - 1;
    t.wx = ix - fx; t.wy = iy - fy;
    return t;
}
// grid_sample's sum: nw, ne, sw, se with the weights (1-wx)(1-wy), wx(1-wy), (1-wx)wy, wx wy
__device__ __forceinline__ void bg_weights(const bg_tap& t, float (&w)[4]) {
    const float ax = 1.f - t.wx, ay = 1.f - t.wy;
    w[0] = ax * ay; w[1] = t.wx * ay; w[2] = ax * t.wy; w[3] = t.wx * t.wy;
}
__device__ __forceinline__ float bg_sample(const float* __restrict__ plane, const bg_tap& t, const float (&w)[4], int W) {
    const float nw = plane[t.y0 * W + t.x0], ne = plane[t.y0 * W + t.x1], sw = plane[t.y1 * W + t.x0], se = plane[t.y1 * W + t.x1];
    return fmaf(se, w[3], fmaf(sw, w[2], fmaf(ne, w[1], nw * w[0])));
}

template <int C>
__global__ __launch_bounds__(BG_BLOCK) void bg_texture_fwd_kernel(const float* __restrict__ texture, int H, int W, int act,
                                                                  const float* __restrict__ dirs, int n, float* __restrict__ color) {
    for (int i = blockIdx.x * BG_BLOCK + threadIdx.x; i < n; i += gridDim.x * BG_BLOCK) {
        const bg_tap t = bg_tap_of(dirs[3 * (size_t)i], dirs[3 * (size_t)i + 1], dirs[3 * (size_t)i + 2], H, W);
        float w[4], out[C];
        bg_weights(t, w);
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const float s = bg_sample(texture + (size_t)c * H * W, t, w, W);
            out[c] = act == BG_ACT_SIGMOID ? asd_sigmoid(s) : s;
        }
        if constexpr (C % 4 == 0) {
            asd_row_store<C>(color + (size_t)i * C, out);      // 16-byte aligned rows: checked by the entry
        } else {
#pragma unroll
            for (int c = 0; c < C; ++c) color[(size_t)i * C + c] = out[c];
        }
    }
}

// d sample of ray i, channel c (the activation's derivative applied), and the ray's texels: shared by the LDS and the atomic pass
template <int C>
__device__ __forceinline__ void bg_ray_grad(const float* __restrict__ texture, int H, int W, int act, const float* __restrict__ dirs,
                                            const float* __restrict__ d_color, int i, bg_tap& t, float (&w)[4], float (&g)[C]) {
    t = bg_tap_of(dirs[3 * (size_t)i], dirs[3 * (size_t)i + 1], dirs[3 * (size_t)i + 2], H, W);
    bg_weights(t, w);
#pragma unroll
    for (int c = 0; c < C; ++c) {
        float d = d_color[(size_t)i * C + c];
        if (act == BG_ACT_SIGMOID) {
            const float s = asd_sigmoid(bg_sample(texture + (size_t)c * H * W, t, w, W));
            d *= s * (1.f - s);
        }
        g[c] = d;
    }
}

// LDS pass: workgroup b owns rays [b * per_wg, (b + 1) * per_wg) and slab b (or d_texture itself when it is the only one)
template <int C>
__global__ __launch_bounds__(BG_BLOCK) void bg_texture_bwd_lds_kernel(const float* __restrict__ texture, int H, int W, int act,
                                                                      const float* __restrict__ dirs, const float* __restrict__ d_color,
                                                                      int n, int per_wg, float* __restrict__ slabs, int64_t slab_stride) {
    extern __shared__ __attribute__((aligned(16))) float img[];
    const int hw = H * W, size = C * hw;
    for (int e = threadIdx.x; e < size; e += BG_BLOCK) img[e] = 0.f;
    __syncthreads();
    const int begin = blockIdx.x * per_wg;
    const int end = begin + per_wg < n ? begin + per_wg : n;
    for (int i = begin + threadIdx.x; i < end; i += BG_BLOCK) {
        bg_tap t;
        float w[4], g[C];
        bg_ray_grad<C>(texture, H, W, act, dirs, d_color, i, t, w, g);
        const int o[4] = {t.y0 * W + t.x0, t.y0 * W + t.x1, t.y1 * W + t.x0, t.y1 * W + t.x1};
#pragma unroll
        for (int c = 0; c < C; ++c)
#pragma unroll
            for (int k = 0; k < 4; ++k) atomicAdd(&img[c * hw + o[k]], w[k] * g[c]);
    }
    __syncthreads();
    float* __restrict__ dst = slabs + (size_t)blockIdx.x * slab_stride;      // 16-byte aligned: checked by the entry
    const int quads = size / 4;
    for (int q = threadIdx.x; q < quads; q += BG_BLOCK) reinterpret_cast<float4*>(dst)[q] = reinterpret_cast<const float4*>(img)[q];
    for (int e = 4 * quads + threadIdx.x; e < size; e += BG_BLOCK) dst[e] = img[e];
}

// d_texture[e] = slab 0 + slab 1 + ... in slab order
__global__ __launch_bounds__(BG_BLOCK) void bg_slab_sum_kernel(const float* __restrict__ slabs, int64_t slab_stride, int n_slabs, int size,
                                                               float* __restrict__ d_texture) {
    const int e = blockIdx.x * BG_BLOCK + threadIdx.x;
    if (e >= size) return;
    float acc = slabs[e];
    int s = 1;
    for (; s + 8 <= n_slabs; s += 8) {      // eight independent loads in flight, added in slab order
        float v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = slabs[(size_t)(s + k) * slab_stride + e];
#pragma unroll
        for (int k = 0; k < 8; ++k) acc += v[k];
    }
    for (; s < n_slabs; ++s) acc += slabs[(size_t)s * slab_stride + e];
    d_texture[e] = acc;
}

// large textures: per-ray global atomics into the zeroed d_texture
template <int C>
__global__ __launch_bounds__(BG_BLOCK) void bg_texture_bwd_atomic_kernel(const float* __restrict__ texture, int H, int W, int act,
                                                                         const float* __restrict__ dirs, const float* __restrict__ d_color,
                                                                         int n, float* __restrict__ d_texture) {
    const size_t hw = (size_t)H * W;
    for (int i = blockIdx.x * BG_BLOCK + threadIdx.x; i < n; i += gridDim.x * BG_BLOCK) {
        bg_tap t;
        float w[4], g[C];
        bg_ray_grad<C>(texture, H, W, act, dirs, d_color, i, t, w, g);
        const int o[4] = {t.y0 * W + t.x0, t.y0 * W + t.x1, t.y1 * W + t.x0, t.y1 * W + t.x1};
#pragma unroll
        for (int c = 0; c < C; ++c)
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float a = w[k] * g[c];
                if (a != 0.f) atomicAdd(d_texture + c * hw + o[k], a);
            }
    }
}

template <int C>
__global__ __launch_bounds__(BG_BLOCK) void bg_solid_fwd_kernel(const float* __restrict__ colors, int64_t rays_per_view, int64_t total,
                                                                float* __restrict__ out) {
    const int64_t per_view = rays_per_view * C;
    for (int64_t e = (int64_t)blockIdx.x * BG_BLOCK + threadIdx.x; e < total; e += (int64_t)gridDim.x * BG_BLOCK)
        out[e] = colors[(e / per_view) * C + e % C];
}

// one workgroup per view: lane partial sums over rays t, t + block, ..., then the wave sums and the waves in wave order
#define BG_SOLID_BLOCK 1024
template <int C>
__global__ __launch_bounds__(BG_SOLID_BLOCK) void bg_solid_bwd_kernel(const float* __restrict__ d_out, int64_t rays_per_view,
                                                                      float* __restrict__ d_colors) {
    __shared__ float part[BG_SOLID_BLOCK / ASD_WAVE][C];
    const float* __restrict__ src = d_out + (size_t)blockIdx.x * rays_per_view * C;
    float acc[C];
#pragma unroll
    for (int c = 0; c < C; ++c) acc[c] = 0.f;
    for (int64_t r = threadIdx.x; r < rays_per_view; r += BG_SOLID_BLOCK)
#pragma unroll
        for (int c = 0; c < C; ++c) acc[c] += src[r * C + c];
    const int wave = threadIdx.x / ASD_WAVE;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const float s = asd_wave_sum(acc[c]);
        if (asd_lane() == 0) part[wave][c] = s;
    }
    __syncthreads();
    if (threadIdx.x < C) {
        float s = 0.f;
        for (int w = 0; w < BG_SOLID_BLOCK / ASD_WAVE; ++w) s += part[w][threadIdx.x];
        d_colors[(size_t)blockIdx.x * C + threadIdx.x] = s;
    }
}

#define BG_DISPATCH_C(C, ...)                     \
    switch (C) {                                  \
        case 1: { constexpr int kC = 1; __VA_ARGS__; } break; \
        case 2: { constexpr int kC = 2; __VA_ARGS__; } break; \
        case 3: { constexpr int kC = 3; __VA_ARGS__; } break; \
        case 4: { constexpr int kC = 4; __VA_ARGS__; } break; \
        case 5: { constexpr int kC = 5; __VA_ARGS__; } break; \
        case 6: { constexpr int kC = 6; __VA_ARGS__; } break; \
        case 7: { constexpr int kC = 7; __VA_ARGS__; } break; \
        default: { constexpr int kC = 8; __VA_ARGS__; } break; \
    }

#define BG_CHECK_TEXTURE(C, H, W, act, n)                                                                           \
    ASD_CHECK_ARG((C) >= 1 && (C) <= BG_MAX_C, "channels outside 1..8");                                            \
    ASD_CHECK_ARG((H) >= 1 && (W) >= 1 && (int64_t)(C) * (H) * (W) < (int64_t)1 << 31, "texture size not positive or beyond 2^31 floats"); \
    ASD_CHECK_ARG((act) == BG_ACT_NONE || (act) == BG_ACT_SIGMOID, "activation is 0 (none) or 1 (sigmoid)");        \
    ASD_CHECK_ARG((n) >= 0, "negative ray count")

// THE layout of the backward pass: the size query and the pass both read it
struct bg_bwd_layout {
    int lds_path;            // gradient image within BG_LDS_BUDGET
    int n_wg, per_wg;        // LDS pass: workgroups and rays per workgroup
    int64_t slab_stride;     // floats, a multiple of 64
    int64_t slabs, total;    // workspace: offset of the slabs (0 when one workgroup writes d_texture itself) and floats in all
};
static bg_bwd_layout bg_bwd_layout_of(int C, int H, int W, int n) {
    bg_bwd_layout L{};
    const int64_t size = (int64_t)C * H * W;
    L.lds_path = size * 4 <= BG_LDS_BUDGET;
    asd_ws_cursor cur;
    if (L.lds_path) {
        L.n_wg = asd_div_up(n, BG_RAYS_PER_WG);
        if (L.n_wg < 1) L.n_wg = 1;
        if (L.n_wg > BG_FEW_SLABS) {
            L.n_wg = asd_div_up(n, BG_RAYS_PER_WG_MANY);
            if (L.n_wg < BG_FEW_SLABS) L.n_wg = BG_FEW_SLABS;
            if (L.n_wg > BG_MAX_SLABS) L.n_wg = BG_MAX_SLABS;
        }
        L.per_wg = n > 0 ? asd_div_up(n, L.n_wg) : 0;
        L.slab_stride = (size + 63) & ~(int64_t)63;
        if (L.n_wg > 1) L.slabs = cur.take(L.slab_stride * L.n_wg);
    }
    L.total = cur.o;
    return L;
}

extern "C" {

int asd_bg_texture_fwd(const float* texture, int32_t C, int32_t H, int32_t W, int32_t activation, const float* dirs, int32_t n, float* color,
                       void* stream) {
    BG_CHECK_TEXTURE(C, H, W, activation, n);
    if (n == 0) return ASD_OK;
    ASD_CHECK_ARG(C % 4 != 0 || ((uintptr_t)color & 15) == 0, "color is not 16-byte aligned (C = 4, 8: rows are stored as float4)");
    BG_DISPATCH_C(C, hipLaunchKernelGGL((bg_texture_fwd_kernel<kC>), dim3(asd_grid_for(n, BG_BLOCK)), dim3(BG_BLOCK), 0, (hipStream_t)stream,
                                        texture, H, W, activation, dirs, n, color));
    ASD_LAUNCH_CHECK();
    return ASD_OK;
}

int asd_bg_texture_bwd_workspace(int32_t C, int32_t H, int32_t W, int32_t n, int64_t* n_floats) {
    BG_CHECK_TEXTURE(C, H, W, BG_ACT_NONE, n);
    ASD_CHECK_ARG(n_floats != nullptr, "n_floats is NULL");
    *n_floats = bg_bwd_layout_of(C, H, W, n).total;
    return ASD_OK;
}

int asd_bg_texture_bwd(const float* texture, int32_t C, int32_t H, int32_t W, int32_t activation, const float* dirs, const float* d_color,
                       int32_t n, float* d_texture, float* workspace, void* stream) {
    BG_CHECK_TEXTURE(C, H, W, activation, n);
    const bg_bwd_layout L = bg_bwd_layout_of(C, H, W, n);
    const int size = C * H * W;
    hipStream_t s = (hipStream_t)stream;
    if (!L.lds_path) {
        if (hipMemsetAsync(d_texture, 0, (size_t)size * sizeof(float), s) != hipSuccess) {
            asd_set_error("%s: clearing d_texture failed", __func__);
            return ASD_ERR_LAUNCH;
        }
        if (n > 0)
            BG_DISPATCH_C(C, hipLaunchKernelGGL((bg_texture_bwd_atomic_kernel<kC>), dim3(asd_grid_for(n, BG_BLOCK)), dim3(BG_BLOCK), 0, s, texture,
                                                H, W, activation, dirs, d_color, n, d_texture));
        ASD_LAUNCH_CHECK();
        return ASD_OK;
    }
    const bool one = L.n_wg == 1;
    ASD_CHECK_ARG(one || workspace != nullptr, "workspace is NULL");
    float* slabs = one ? d_texture : workspace + L.slabs;
    ASD_CHECK_ARG(((uintptr_t)slabs & 15) == 0, "d_texture (one workgroup) / workspace is not 16-byte aligned");
    const size_t lds = ((size_t)size * sizeof(float) + 15) & ~(size_t)15;
    BG_DISPATCH_C(C, (asd_launch_lds<bg_texture_bwd_lds_kernel<kC>, BG_LDS_BUDGET>(dim3(L.n_wg), dim3(BG_BLOCK), lds, s, texture, (int)H, (int)W,
                                                                                  (int)activation, dirs, d_color, (int)n, L.per_wg, slabs,
                                                                                  L.slab_stride)));
    ASD_LAUNCH_CHECK();
    if (!one) {
        hipLaunchKernelGGL(bg_slab_sum_kernel, dim3(asd_div_up(size, BG_BLOCK)), dim3(BG_BLOCK), 0, s, (const float*)slabs, L.slab_stride, L.n_wg,
                           size, d_texture);
        ASD_LAUNCH_CHECK();
    }
    return ASD_OK;
}

#define BG_CHECK_SOLID(C, V, R)                                          \
    ASD_CHECK_ARG((C) >= 1 && (C) <= BG_MAX_C, "channels outside 1..8"); \
    ASD_CHECK_ARG((V) >= 0 && (R) >= 0, "negative view or ray count")

int asd_bg_solid_fwd(const float* colors, int32_t C, int32_t n_views, int32_t rays_per_view, float* out, void* stream) {
    BG_CHECK_SOLID(C, n_views, rays_per_view);
    const int64_t total = (int64_t)n_views * rays_per_view * C;
    if (total == 0) return ASD_OK;
    BG_DISPATCH_C(C, hipLaunchKernelGGL((bg_solid_fwd_kernel<kC>), dim3(asd_grid_for(total, BG_BLOCK)), dim3(BG_BLOCK), 0, (hipStream_t)stream,
                                        colors, (int64_t)rays_per_view, total, out));
    ASD_LAUNCH_CHECK();
    return ASD_OK;
}

int asd_bg_solid_bwd(const float* d_out, int32_t C, int32_t n_views, int32_t rays_per_view, float* d_colors, void* stream) {
    BG_CHECK_SOLID(C, n_views, rays_per_view);
    if (n_views == 0) return ASD_OK;
    BG_DISPATCH_C(C, hipLaunchKernelGGL((bg_solid_bwd_kernel<kC>), dim3(n_views), dim3(BG_SOLID_BLOCK), 0, (hipStream_t)stream, d_out,
                                        (int64_t)rays_per_view, d_colors));
    ASD_LAUNCH_CHECK();
    return ASD_OK;
}

}  // extern "C"
