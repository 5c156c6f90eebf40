// atlas.hip — a per-face UV atlas and its bake for gfx950: the texture route of the mesh exporter (threestudio/models/exporters/
// mesh_exporter.py:53-137) without xatlas, nvdiffrast or cv2.inpaint.  This is NOT xatlas's atlas: every face gets a cell of its own, so
// the texture resolution per face is uniform rather than proportional to its area, and there are 3 F texture vertices.
//
// Layout (asd_atlas_layout is its one definition; both kernels and Python take the struct from there):
//   F faces -> P = ceil(F / 2) cells, n = ceil(sqrt(P)) cells per row, cell side c = floor(T / n) texels, gutter g, leg L = c - 3 g - 1.
//   Cell k has its origin at texel ((k % n) c, (k / n) c).  In cell-local continuous texel coordinates (texel (i, j) has its centre at
//   (i + 1/2, j + 1/2)) face 2k is the lower triangle (g, g) (g + L, g) (g, g + L) for corners 0 1 2 of t_pos_idx and face 2k + 1 the
//   upper triangle (c - g, c - g) (c - g - L, c - g) (c - g, c - g - L): the lower one reflected through the cell's centre.
//   Texel (i, j) of a cell belongs to the lower face when i + j + 1 < c, to the upper face when i + j + 1 > c, to nobody on the
//   anti-diagonal, in a cell or half-cell without a face, and in the strip beyond n c.
// Why g = 1 is enough for bilinear sampling without mip-maps: a lookup at (x, y) inside the lower triangle reads texel centres strictly
//   within (x +- 1, y +- 1), so their coordinate sum is < x + y + 2 <= 2 g + L + 2 = c - g + 1 and every coordinate is > g - 1 >= 0.
//   Centre sums are integers (i + j + 1), so with g >= 1 they are < c: all four texels are the lower face's own, inside the cell.  The
//   upper triangle is the mirror image: sums > c + g - 1, coordinates < c - g + 1.  No lookup inside a face reads another face's texel:
//   no seams and no inpainting pass.
// A texel owned by a face holds the point of that face's UV triangle nearest to the texel centre — inside the triangle the centre itself
//   (`covered`), in the gutter its projection onto the triangle — mapped to 3-D by the barycentric weights of the face's corners.
//
// asd_atlas_bake is write-bound: 12 + 4 + 1 = 17 bytes per texel (285 MB at 4096^2) against a few cached loads.  gb_pos is [T, T, 3]
// fp32, a 12-byte stride per texel: a thread storing its own three floats would issue three 4-byte stores 12 bytes apart.  CHOSEN: the
// block stages the 256 positions of its tile in LDS (stride 3 dwords: odd, conflict-free) and writes the 3072 contiguous bytes back as
// 192 full-width 16-byte stores; `covered` goes out the same way as 64 dword stores instead of 256 single bytes.  The layout stays the
// reference's [T, T, 3], which geometry.export reads as [N, 3] without a transpose — that is why it is not three planes.
#include "asd_common.h"

#define ATLAS_MAX_T 8192
#define ATLAS_BLOCK 256

// ---- uv: three texture vertices of its own per face ----------------------------------------------------------------------------------
// v_tex = texel coordinate / T with an IEEE division: F threads, not T^2, and the quotient is then the correctly rounded one that a
// numpy restatement gives (exact when T is a power of two)
__global__ __launch_bounds__(ATLAS_BLOCK) void atlas_uv_kernel(AsdAtlasLayout lay, int64_t n_faces, float* __restrict__ v_tex,
                                                               int64_t* __restrict__ t_tex_idx) {
    const float T = (float)lay.texture_size;
    for (int64_t f = (int64_t)blockIdx.x * ATLAS_BLOCK + threadIdx.x; f < n_faces; f += (int64_t)gridDim.x * ATLAS_BLOCK) {
        const int k = (int)(f >> 1);
        const int ox = (k % lay.n) * lay.c, oy = (k / lay.n) * lay.c;
        const bool up = f & 1;
        const int a = up ? lay.c - lay.gutter : lay.gutter, s = up ? -lay.L : lay.L;
        const int x[3] = {ox + a, ox + a + s, ox + a}, y[3] = {oy + a, oy + a, oy + a + s};
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            v_tex[6 * f + 2 * q] = (float)x[q] / T;
            v_tex[6 * f + 2 * q + 1] = (float)y[q] / T;
            t_tex_idx[3 * f + q] = 3 * f + q;
        }
    }
}

// ---- bake: one thread per texel ------------------------------------------------------------------------------------------------------
// Every quantity up to the weights is a multiple of 1/2 below 2^14: exact in fp32.  The position is then, in this order and without
// contraction (the library is built with -ffp-contract=off):
//   b_k = w_k * rL (rL = fl(1 / L), computed once on the host),  pos = (p0 * b0 + p1 * b1) + p2 * b2
// with w1 = u, w2 = v, w0 = L - u - v >= 0 the exact weights times L: five roundings on the terms of corners 0 and 1, four on corner 2.
__global__ __launch_bounds__(ATLAS_BLOCK) void atlas_bake_kernel(AsdAtlasLayout lay, float rL, const float* __restrict__ v_pos,
                                                                 const int64_t* __restrict__ faces, int64_t n_verts, int64_t n_faces,
                                                                 float* __restrict__ gb_pos, int32_t* __restrict__ face_id,
                                                                 uint8_t* __restrict__ covered) {
    __shared__ __attribute__((aligned(16))) float s_pos[3 * ATLAS_BLOCK];
    __shared__ __attribute__((aligned(4))) uint8_t s_cov[ATLAS_BLOCK];
    const int T = lay.texture_size, c = lay.c, g = lay.gutter, L = lay.L, n = lay.n;
    const int64_t n_texels = (int64_t)T * T;
    const int64_t n_tiles = (n_texels + ATLAS_BLOCK - 1) / ATLAS_BLOCK;
    const int t = (int)threadIdx.x;
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int64_t base = tile * ATLAS_BLOCK, idx = base + t;
        int64_t face = -1;
        float pos[3] = {0.f, 0.f, 0.f};
        bool cov = false;
        if (idx < n_texels) {
            const int j = (int)((uint32_t)idx / (uint32_t)T), i = (int)(idx - (int64_t)j * T);      // idx < 8192^2: a 32-bit division
            const int ci = i / c, cj = j / c;
            if (ci < n && cj < n) {         // else: the strip beyond n c
                const int li = i - ci * c, lj = j - cj * c, d = li + lj + 1;
                const int64_t f = 2 * ((int64_t)cj * n + ci) + (d > c ? 1 : 0);
                if (d != c && f < n_faces) {
                    const int64_t ia = faces[3 * f], ib = faces[3 * f + 1], ic = faces[3 * f + 2];
                    if (ia >= 0 && ia < n_verts && ib >= 0 && ib < n_verts && ic >= 0 && ic < n_verts) {       // else nothing is read through it
                        face = f;
                        // (u, v): the texel centre relative to corner 0 along the two legs; the upper triangle is the lower one mirrored
                        const float x = (float)li + 0.5f, y = (float)lj + 0.5f, fl = (float)L;
                        float u = d > c ? (float)(c - g) - x : x - (float)g;
                        float v = d > c ? (float)(c - g) - y : y - (float)g;
                        cov = u >= 0.f && v >= 0.f && u + v <= fl;
                        // nearest point of the triangle {u >= 0, v >= 0, u + v <= L}: the clamp to the quadrant where that lies inside,
                        // else the nearest point of the hypotenuse (the nearest point of quadrant and half-plane together lies on the
                        // half-plane's edge once the quadrant's own nearest point violates it)
                        const float qu = fmaxf(u, 0.f), qv = fmaxf(v, 0.f);
                        if (qu + qv <= fl) {
                            u = qu; v = qv;
                        } else {
                            u = fminf(fmaxf((u - v + fl) * 0.5f, 0.f), fl);
                            v = fl - u;
                        }
                        const float b0 = (fl - u - v) * rL, b1 = u * rL, b2 = v * rL;
#pragma unroll
                        for (int q = 0; q < 3; ++q) pos[q] = (v_pos[3 * ia + q] * b0 + v_pos[3 * ib + q] * b1) + v_pos[3 * ic + q] * b2;
                    }
                }
            }
            face_id[idx] = (int32_t)face;
        }
        s_pos[3 * t] = pos[0]; s_pos[3 * t + 1] = pos[1]; s_pos[3 * t + 2] = pos[2];
        s_cov[t] = cov ? 1 : 0;
        __syncthreads();
        const int64_t here = n_texels - base < ATLAS_BLOCK ? n_texels - base : ATLAS_BLOCK;       // texels of this tile
        // base is a multiple of 256: the tile's 12 * 256 bytes of gb_pos and 256 bytes of covered start 16-byte and 4-byte aligned
        if (4 * t + 3 < 3 * here) {
            *reinterpret_cast<float4*>(gb_pos + 3 * base + 4 * t) = *reinterpret_cast<const float4*>(s_pos + 4 * t);
        } else {
            for (int q = 4 * t; q < 3 * here && q < 4 * t + 4; ++q) gb_pos[3 * base + q] = s_pos[q];
        }
        if (4 * t + 3 < here) {
            *reinterpret_cast<uint32_t*>(covered + base + 4 * t) = *reinterpret_cast<const uint32_t*>(s_cov + 4 * t);
        } else {
            for (int q = 4 * t; q < here && q < 4 * t + 4; ++q) covered[base + q] = s_cov[q];
        }
        __syncthreads();
    }
}

// ---- pack: clip to [0, 1], * 255, truncate (get_rgb_image_, threestudio/utils/saving.py:82-86), scatter -----------------------------
__global__ __launch_bounds__(ATLAS_BLOCK) void atlas_pack_u8_kernel(const float* __restrict__ values, const int64_t* __restrict__ texel_index,
                                                                    int64_t n_owned, int C, int64_t n_texels, uint8_t* __restrict__ image) {
    const int64_t total = n_owned * C;
    for (int64_t e = (int64_t)blockIdx.x * ATLAS_BLOCK + threadIdx.x; e < total; e += (int64_t)gridDim.x * ATLAS_BLOCK) {
        const int64_t k = (uint32_t)e / (uint32_t)C;      // e < 4 * 8192^2: a 32-bit division
        const int ch = (int)(e - k * C);
        const int64_t at = texel_index[k];
        if (at < 0 || at >= n_texels) continue;
        const float x = fminf(fmaxf(values[e], 0.f), 1.f) * 255.f;
        image[at * C + ch] = (uint8_t)(int)x;
    }
}

static bool atlas_layout_fill(const char* fn, int64_t n_faces, int32_t T, int32_t g, AsdAtlasLayout* out) {
    if (n_faces < 0 || n_faces > INT32_MAX) {
        asd_set_error("%s: n_faces must be in [0, 2^31) (got %lld)", fn, (long long)n_faces);
        return false;
    }
    if (T < 1 || T > ATLAS_MAX_T) {
        asd_set_error("%s: texture_size must be in [1, %d] (got %d)", fn, ATLAS_MAX_T, T);
        return false;
    }
    if (g < 0 || g > ATLAS_MAX_T) {
        asd_set_error("%s: gutter must be in [0, %d] (got %d)", fn, ATLAS_MAX_T, g);
        return false;
    }
    AsdAtlasLayout lay;
    lay.n_faces = (int32_t)n_faces; lay.texture_size = T; lay.gutter = g;
    lay.n = lay.c = lay.L = 0;      // no faces: no cells, and nothing to refuse
    if (n_faces > 0) {
        const int64_t P = (n_faces + 1) / 2;
        int64_t n = (int64_t)sqrt((double)P);
        while (n * n < P) ++n;
        while (n > 1 && (n - 1) * (n - 1) >= P) --n;
        const int64_t c = T / n, L = c - 3 * (int64_t)g - 1;
        if (L < 1) {
            const int64_t fit = n * (3 * (int64_t)g + 2);
            if (fit <= ATLAS_MAX_T)
                asd_set_error("%s: %lld faces do not fit a texture_size of %d with gutter %d (%lld cells per row of side %lld, leg %lld < 1): "
                              "the smallest texture_size that fits is %lld", fn, (long long)n_faces, T, g, (long long)n, (long long)c, (long long)L,
                              (long long)fit);
            else
                asd_set_error("%s: %lld faces do not fit a texture_size of %d with gutter %d (%lld cells per row of side %lld, leg %lld < 1): "
                              "the smallest texture_size that fits is %lld, beyond the limit of %d", fn, (long long)n_faces, T, g, (long long)n,
                              (long long)c, (long long)L, (long long)fit, ATLAS_MAX_T);
            return false;
        }
        lay.n = (int32_t)n; lay.c = (int32_t)c; lay.L = (int32_t)L;
    }
    *out = lay;
    return true;
}

// a layout handed back by the caller is what asd_atlas_layout would fill for its own first three fields
static bool atlas_layout_ok(const char* fn, const AsdAtlasLayout* lay, int64_t n_faces) {
    AsdAtlasLayout want;
    if (!lay) {
        asd_set_error("%s: null argument", fn);
        return false;
    }
    if (!atlas_layout_fill(fn, n_faces, lay->texture_size, lay->gutter, &want)) return false;
    if (lay->n_faces != want.n_faces || lay->n != want.n || lay->c != want.c || lay->L != want.L) {
        asd_set_error("%s: the layout is not asd_atlas_layout's for %lld faces", fn, (long long)n_faces);
        return false;
    }
    return true;
}

extern "C" {

int asd_atlas_layout(int64_t n_faces, int32_t texture_size, int32_t gutter, AsdAtlasLayout* out) {
    ASD_CHECK_ARG(out, "null argument");
    return atlas_layout_fill(__func__, n_faces, texture_size, gutter, out) ? ASD_OK : ASD_ERR_ARG;
}

int asd_atlas_uv(const AsdAtlasLayout* layout, int64_t n_faces, float* v_tex, int64_t* t_tex_idx, void* stream) {
    if (!atlas_layout_ok(__func__, layout, n_faces)) return ASD_ERR_ARG;
    if (n_faces == 0) return ASD_OK;
    ASD_CHECK_ARG(v_tex && t_tex_idx, "null argument");
    hipLaunchKernelGGL(atlas_uv_kernel, dim3(asd_grid_for(n_faces, ATLAS_BLOCK)), dim3(ATLAS_BLOCK), 0, (hipStream_t)stream, *layout, n_faces, v_tex,
                       t_tex_idx);
    ASD_LAUNCH_CHECK();
    return ASD_OK;
}

int asd_atlas_bake(const AsdAtlasLayout* layout, const float* v_pos, const int64_t* faces, int64_t n_verts, int64_t n_faces, float* gb_pos,
                   int32_t* face_id, uint8_t* covered, void* stream) {
    if (!atlas_layout_ok(__func__, layout, n_faces)) return ASD_ERR_ARG;
    ASD_CHECK_ARG(gb_pos && face_id && covered, "null output");
    ASD_CHECK_ARG(n_verts >= 0 && n_verts <= INT32_MAX, "n_verts must be in [0, 2^31)");
    ASD_CHECK_ARG(n_faces == 0 || (v_pos && faces), "null argument");
    ASD_CHECK_ARG(((uintptr_t)gb_pos & 15) == 0 && ((uintptr_t)covered & 3) == 0, "gb_pos must be 16-byte and covered 4-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const int64_t n_texels = (int64_t)layout->texture_size * layout->texture_size;
    if (n_faces == 0) {     // every texel unowned
        if (hipMemsetAsync(gb_pos, 0, (size_t)n_texels * 3 * sizeof(float), s) != hipSuccess ||
            hipMemsetAsync(face_id, 0xff, (size_t)n_texels * sizeof(int32_t), s) != hipSuccess ||
            hipMemsetAsync(covered, 0, (size_t)n_texels, s) != hipSuccess) {
            asd_set_error("%s: hipMemsetAsync failed", __func__);
            return ASD_ERR_LAUNCH;
        }
        return ASD_OK;
    }
    const float rL = 1.0f / (float)layout->L;
    ASD_PROBE_START(s);
    hipLaunchKernelGGL(atlas_bake_kernel, dim3(asd_grid_for(n_texels, ATLAS_BLOCK)), dim3(ATLAS_BLOCK), 0, s, *layout, rL, v_pos, faces, n_verts, n_faces,
                       gb_pos, face_id, covered);
    ASD_PROBE_STOP(s);
    ASD_LAUNCH_CHECK();
    return ASD_OK;
}

int asd_atlas_pack_u8(const float* values, const int64_t* texel_index, int64_t n_owned, int32_t C, uint8_t* image, int64_t n_texels, void* stream) {
    ASD_CHECK_ARG(n_owned >= 0 && n_owned <= (int64_t)ATLAS_MAX_T * ATLAS_MAX_T, "n_owned must be in [0, 8192^2]");
    ASD_CHECK_ARG(C >= 1 && C <= 4, "C must be in [1, 4]");
    ASD_CHECK_ARG(n_texels >= 0 && n_texels <= (int64_t)ATLAS_MAX_T * ATLAS_MAX_T, "n_texels must be in [0, 8192^2]");
    if (n_owned == 0) return ASD_OK;
    ASD_CHECK_ARG(values && texel_index && image, "null argument");
    hipLaunchKernelGGL(atlas_pack_u8_kernel, dim3(asd_grid_for(n_owned * C, ATLAS_BLOCK)), dim3(ATLAS_BLOCK), 0, (hipStream_t)stream, values, texel_index,
                       n_owned, (int)C, n_texels, image);
    ASD_LAUNCH_CHECK();
    return ASD_OK;
}

}  // extern "C"
