// image.hip — float images to bytes for gfx950: what the validation / test passes of the reference do on the host with numpy and cv2
// (threestudio/utils/saving.py:77-109 get_rgb_image_, :179-221 get_grayscale_image_, :255-299 get_image_grid_; the per-image depth
// normalisation of threestudio/systems/scaledreamer.py:176-178,256-258).
//
// asd_image_minmax_f32: exact per-image extrema, deterministic, no atomics.  An image is cut into chunks of IMG_CHUNK floats, one
//   block per chunk; with one chunk per image the block writes minmax itself, otherwise it writes a (min, max) partial into the
//   workspace and a second launch (one block per image) folds the partials.  image_minmax_layout is the one definition of the chunk
//   count and the workspace size: the size query and the pass both call it.  A NaN is carried as a flag next to fminf / fmaxf (which
//   skip NaN operands) and turns both results of its image into NaN, like torch.min / torch.max; a NaN partial raises the flag again.
// asd_image_grid_u8: one launch for the whole grid.  out is [B, H, P W, 3] bytes, a pixel is 3 bytes, so FOUR consecutive pixels are
//   12 bytes starting on a dword boundary whatever P W is (a row of P W 3 bytes may start at any byte; a group of four pixels may span
//   two rows or two panels — each pixel is decoded on its own).  A thread converts four pixels, reading every source value once, and
//   stores three whole dwords; the n_pixels % 4 pixels at the very end go out as single bytes.  The panel table (<= 8 entries) is copied
//   from the kernel arguments to LDS with constant indices, so the per-lane lookup is an LDS read and nothing lands in scratch.
#include <float.h>
#include <math.h>

#include "asd_common.h"

#define IMG_BLOCK 256
#define IMG_CHUNK 16384         // floats of one image per block: 16 float4 loads per thread
#define IMG_MAX_PANELS 8

struct ImgMinmaxLayout {
    int64_t chunks;             // blocks per image
    int64_t ws_floats;          // partials [n_images, chunks, 2]; 0 when chunks == 1
};

static bool image_minmax_layout(const char* fn, int64_t n_images, int64_t n_per_image, ImgMinmaxLayout* out) {
    if (n_images < 0 || n_per_image < 1) {
        asd_set_error("%s: n_images must be >= 0 and n_per_image >= 1 (got %lld, %lld)", fn, (long long)n_images, (long long)n_per_image);
        return false;
    }
    const int64_t chunks = (n_per_image + IMG_CHUNK - 1) / IMG_CHUNK;
    if (n_images > INT32_MAX || chunks > INT32_MAX || n_images * chunks > INT32_MAX) {
        asd_set_error("%s: %lld images of %lld chunks exceed one grid", fn, (long long)n_images, (long long)chunks);
        return false;
    }
    out->chunks = chunks;
    out->ws_floats = chunks > 1 ? n_images * chunks * 2 : 0;
    return true;
}

struct ImgExtrema {
    float mn = INFINITY, mx = -INFINITY;
    bool nan = false;
    __device__ __forceinline__ void take(float v) {
        nan |= v != v;
        mn = fminf(mn, v);
        mx = fmaxf(mx, v);
    }
};

// the block's extrema to dst[0], dst[1] (thread 0): wave butterfly, then the four waves through LDS
__device__ __forceinline__ void img_block_extrema(ImgExtrema e, float* __restrict__ dst) {
    __shared__ float s_mn[IMG_BLOCK / ASD_WAVE], s_mx[IMG_BLOCK / ASD_WAVE];
    __shared__ int s_nan[IMG_BLOCK / ASD_WAVE];
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        e.mn = fminf(e.mn, __shfl_xor(e.mn, o, 64));
        e.mx = fmaxf(e.mx, __shfl_xor(e.mx, o, 64));
    }
    const bool wave_nan = __ballot(e.nan) != 0ull;
    const int wave = (int)threadIdx.x >> 6;
    if (asd_lane() == 0) {
        s_mn[wave] = e.mn; s_mx[wave] = e.mx; s_nan[wave] = wave_nan ? 1 : 0;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float mn = s_mn[0], mx = s_mx[0];
        int nan = s_nan[0];
#pragma unroll
        for (int w = 1; w < IMG_BLOCK / ASD_WAVE; ++w) {
            mn = fminf(mn, s_mn[w]); mx = fmaxf(mx, s_mx[w]); nan |= s_nan[w];
        }
        dst[0] = nan ? NAN : mn;
        dst[1] = nan ? NAN : mx;
    }
}

// block = (image, chunk); dst is minmax (chunks == 1) or the partials: [n_images, chunks, 2] either way
__global__ __launch_bounds__(IMG_BLOCK) void image_minmax_kernel(const float* __restrict__ x, int64_t n_per_image, int64_t chunks,
                                                                 float* __restrict__ dst) {
    const int64_t img = (int64_t)blockIdx.x / chunks, ch = (int64_t)blockIdx.x - img * chunks;
    const int64_t start = ch * IMG_CHUNK;
    const int len = (int)(n_per_image - start < IMG_CHUNK ? n_per_image - start : IMG_CHUNK);      // >= 1
    const float* __restrict__ p = x + img * n_per_image + start;
    const int t = (int)threadIdx.x;
    // an image starts wherever n_per_image puts it: scalars up to the next 16-byte boundary, float4 from there, scalars at the end
    int head = (int)(((16u - (unsigned)((uintptr_t)p & 15u)) & 15u) >> 2);
    if (head > len) head = len;
    const int body = (len - head) >> 2, tail = head + 4 * body;
    ImgExtrema e;
    if (t < head) e.take(p[t]);
    const float4* __restrict__ q = reinterpret_cast<const float4*>(p + head);
    for (int i = t; i < body; i += IMG_BLOCK) {
        const float4 v = q[i];
        e.take(v.x); e.take(v.y); e.take(v.z); e.take(v.w);
    }
    if (t < len - tail) e.take(p[tail + t]);
    img_block_extrema(e, dst + 2 * (int64_t)blockIdx.x);
}

// block = image: fold its partials
__global__ __launch_bounds__(IMG_BLOCK) void image_minmax_fold_kernel(const float* __restrict__ partial, int64_t chunks, float* __restrict__ minmax) {
    const float* __restrict__ p = partial + 2 * (int64_t)blockIdx.x * chunks;
    ImgExtrema e;
    for (int64_t i = threadIdx.x; i < 2 * chunks; i += IMG_BLOCK) e.take(p[i]);      // a min is a candidate maximum too: harmless, min <= max
    img_block_extrema(e, minmax + 2 * (int64_t)blockIdx.x);
}

// ---- grid ------------------------------------------------------------------------------------------------------------------------------
struct ImgGridPanels {
    AsdImagePanel p[IMG_MAX_PANELS];
};

// clip, rescale, truncate: fp32, no contraction, IEEE division (the library's flags).  fmaxf returns its other operand for a NaN, so a NaN
// becomes lo and is written as 0.
__device__ __forceinline__ uint32_t img_byte(float v, float lo, float hi) {
    v = fminf(fmaxf(v, lo), hi);
    const float u = (v - lo) / (hi - lo) * 255.0f;
    return (uint32_t)(int)u & 0xffu;
}

// the three bytes of output pixel (row, col) in bits 0-23; row = b H + h, col = panel W + w
__device__ __forceinline__ uint32_t img_pixel(const AsdImagePanel* __restrict__ panels, uint32_t row, uint32_t col, uint32_t H, uint32_t W) {
    const uint32_t pi = col / W, w = col - pi * W;
    const AsdImagePanel pn = panels[pi];
    const int64_t at = (int64_t)row * W + w;
    if (pn.kind == ASD_PANEL_RGB) {
        const float* __restrict__ s = pn.src + 3 * at;
        return img_byte(s[0], pn.lo, pn.hi) | (img_byte(s[1], pn.lo, pn.hi) << 8) | (img_byte(s[2], pn.lo, pn.hi) << 16);
    }
    float v = pn.src[at];
    if (pn.normalize) {
        const uint32_t b = row / H;
        const float mn = pn.minmax[2 * b], mx = pn.minmax[2 * b + 1];
        v = (v - mn) / (mx - mn);
    }
    v = v != v ? 0.f : (v > FLT_MAX ? FLT_MAX : (v < -FLT_MAX ? -FLT_MAX : v));      // nan_to_num
    return img_byte(v, pn.lo, pn.hi) * 0x010101u;
}

__global__ __launch_bounds__(IMG_BLOCK) void image_grid_u8_kernel(ImgGridPanels table, int P, uint32_t H, uint32_t W, uint32_t n_rows,
                                                                  uint8_t* __restrict__ out) {
    __shared__ AsdImagePanel s_panels[IMG_MAX_PANELS];
    const int t = (int)threadIdx.x;
#pragma unroll
    for (int j = 0; j < IMG_MAX_PANELS; ++j)
        if (t == j && j < P) s_panels[j] = table.p[j];
    __syncthreads();
    const uint32_t PW = (uint32_t)P * W;
    const uint32_t n_pixels = n_rows * PW;                  // < 2^31 (host check)
    const uint32_t n_groups = n_pixels >> 2;
    for (uint32_t g = blockIdx.x * IMG_BLOCK + t; g < n_groups; g += gridDim.x * IMG_BLOCK) {
        uint32_t row = (4u * g) / PW, col = 4u * g - row * PW;
        uint32_t px[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            px[k] = img_pixel(s_panels, row, col, H, W);
            if (++col == PW) { col = 0; ++row; }
        }
        uint32_t* __restrict__ o = reinterpret_cast<uint32_t*>(out + 12 * (int64_t)g);     // out is 4-byte aligned: so is every group
        o[0] = px[0] | (px[1] << 24);
        o[1] = (px[1] >> 8) | (px[2] << 16);
        o[2] = (px[2] >> 16) | (px[3] << 8);
    }
    const uint32_t q = 4u * n_groups + (uint32_t)t;          // the last n_pixels % 4 pixels: single bytes
    if (blockIdx.x == 0 && q < n_pixels) {
        const uint32_t row = q / PW, col = q - row * PW;
        const uint32_t px = img_pixel(s_panels, row, col, H, W);
        out[3 * (int64_t)q] = (uint8_t)px;
        out[3 * (int64_t)q + 1] = (uint8_t)(px >> 8);
        out[3 * (int64_t)q + 2] = (uint8_t)(px >> 16);
    }
}

extern "C" {

int64_t asd_image_minmax_workspace(int64_t n_images, int64_t n_per_image) {
    ImgMinmaxLayout lay;
    if (!image_minmax_layout(__func__, n_images, n_per_image, &lay)) return -1;
    return lay.ws_floats * (int64_t)sizeof(float);
}

int asd_image_minmax_f32(const float* x, int64_t n_images, int64_t n_per_image, float* minmax, void* workspace, int64_t workspace_bytes,
                         void* stream) {
    ImgMinmaxLayout lay;
    if (!image_minmax_layout(__func__, n_images, n_per_image, &lay)) return ASD_ERR_ARG;
    if (n_images == 0) return ASD_OK;
    ASD_CHECK_ARG(x && minmax, "null argument");
    ASD_CHECK_ARG(((uintptr_t)x & 3) == 0 && ((uintptr_t)minmax & 3) == 0, "x and minmax must be 4-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    if (lay.chunks == 1) {
        hipLaunchKernelGGL(image_minmax_kernel, dim3((unsigned)n_images), dim3(IMG_BLOCK), 0, s, x, n_per_image, (int64_t)1, minmax);
        ASD_LAUNCH_CHECK();
        return ASD_OK;
    }
    ASD_CHECK_ARG(workspace && workspace_bytes >= lay.ws_floats * (int64_t)sizeof(float) && ((uintptr_t)workspace & 3) == 0,
                  "workspace smaller than asd_image_minmax_workspace, or not 4-byte aligned");
    float* partial = (float*)workspace;
    hipLaunchKernelGGL(image_minmax_kernel, dim3((unsigned)(n_images * lay.chunks)), dim3(IMG_BLOCK), 0, s, x, n_per_image, lay.chunks, partial);
    ASD_LAUNCH_CHECK();
    hipLaunchKernelGGL(image_minmax_fold_kernel, dim3((unsigned)n_images), dim3(IMG_BLOCK), 0, s, (const float*)partial, lay.chunks, minmax);
    ASD_LAUNCH_CHECK();
    return ASD_OK;
}

int asd_image_grid_u8(const AsdImagePanel* panels, int32_t n_panels, int64_t B, int32_t H, int32_t W, uint8_t* out, void* stream) {
    ASD_CHECK_ARG(panels, "null argument");
    ASD_CHECK_ARG(n_panels >= 1 && n_panels <= IMG_MAX_PANELS, "n_panels must be in [1, 8]");
    ASD_CHECK_ARG(B >= 0 && H >= 1 && W >= 1, "B must be >= 0, H and W >= 1");
    ASD_CHECK_ARG((double)B * H * W * n_panels < 2147483648.0, "B * H * P * W must be below 2^31");
    ImgGridPanels table;
    for (int j = 0; j < IMG_MAX_PANELS; ++j) table.p[j] = panels[j < n_panels ? j : 0];
    for (int j = 0; j < n_panels; ++j) {
        const AsdImagePanel& p = panels[j];
        if (p.kind != ASD_PANEL_RGB && p.kind != ASD_PANEL_GRAYSCALE) {
            asd_set_error("%s: panel %d: kind %d is neither ASD_PANEL_RGB nor ASD_PANEL_GRAYSCALE", __func__, j, p.kind);
            return ASD_ERR_ARG;
        }
        if (!(p.hi > p.lo) || !isfinite(p.lo) || !isfinite(p.hi)) {
            asd_set_error("%s: panel %d: the range needs finite lo < hi (got %g, %g)", __func__, j, (double)p.lo, (double)p.hi);
            return ASD_ERR_ARG;
        }
        if (p.normalize && (p.kind != ASD_PANEL_GRAYSCALE || !p.minmax)) {
            asd_set_error("%s: panel %d: normalize is for grayscale panels and needs their minmax", __func__, j);
            return ASD_ERR_ARG;
        }
        if (B > 0 && (!p.src || ((uintptr_t)p.src & 3))) {
            asd_set_error("%s: panel %d: null or misaligned source", __func__, j);
            return ASD_ERR_ARG;
        }
    }
    if (B == 0) return ASD_OK;
    ASD_CHECK_ARG(out && ((uintptr_t)out & 3) == 0, "out must be 4-byte aligned");
    const int64_t n_pixels = B * H * (int64_t)W * n_panels;
    hipStream_t s = (hipStream_t)stream;
    ASD_PROBE_START(s);
    hipLaunchKernelGGL(image_grid_u8_kernel, dim3(asd_grid_for((n_pixels + 3) / 4, IMG_BLOCK)), dim3(IMG_BLOCK), 0, s, table, (int)n_panels, (uint32_t)H,
                       (uint32_t)W, (uint32_t)(B * H), out);
    ASD_PROBE_STOP(s);
    ASD_LAUNCH_CHECK();
    return ASD_OK;
}

}  // extern "C"
