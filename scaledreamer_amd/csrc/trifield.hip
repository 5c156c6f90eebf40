// trifield.hip — host side of the fused field of `Triplane-transformer-sdf` (custom/amortized/models/geometry/triplane_transformer.py:139-240):
// contract -> three bilinear plane lookups (sample_from_planes, geometry/utils.py:81-93) concatenated to 96 features -> two VanillaMLP heads
// 96 -> 64 -> 64 -> 1 | 3 (no biases, ReLU) -> sdf + bias -> finite-difference sdf_grad — instead of a sampler launch plus library GEMMs that
// keep ~1.2 KB of autograd state per evaluation (245 GB at 256 x 256 x 4 views: the reference-shaped path needs activation checkpointing there).
//
// The kernels are trifield_mfma.hip (tiles of rows on the matrix pipe, forward and backward) and trifield_scatter.hip (the feature gradient
// into the planes: counting sort by plane cell + segmented reduction).  The backward pass re-gathers the features (nothing but the points is
// saved) and walks the samples in chunks; per chunk it leaves the 400-byte feature-gradient row and the position of every row for the scatter.
// The one-thread-per-sample first form of the field and the LDS-image scatter that used to live here are history: DESIGN.md 4.5 / 4.5b.
#include <stdlib.h>

#include "trifield_common.h"
#include "trifield_mfma.h"

// samples per backward chunk: the pass keeps the feature-gradient row and the position of each row (x 4 rows per sample with a normal
// gradient) and takes 1 M samples at a time (1.7 GB), so that its weight-gradient kernels amortise their prologue (56-80 KB of weight
// images per block) and epilogue (11 k atomics per wave) over 16-64 tiles per wave
#define TF_CHUNK (1024 * 1024)
static int64_t tf_chunk() {                    // ASD_TRI_CHUNK (samples, read per call): the tests walk several chunks at small sizes
    const char* e = getenv("ASD_TRI_CHUNK");
    if (e && atoll(e) >= 64) return atoll(e);
    return TF_CHUNK;
}

static int tf_check(const asd_field_cfg* c, int H, int W, int C) {
    ASD_CHECK_ARG(c && H > 0 && W > 0, "bad argument");
    if (C != 32 || c->n_hidden != 64 || c->n_feature_dims != 3 || c->field_mode != ASD_FIELD_SDF || !(c->bias_mode == ASD_BIAS_SPHERE || c->bias_mode == ASD_BIAS_CONST)) {
        asd_set_error("tri-plane field kernels: 3 x 32 channels, two hidden layers of 64, 3 feature dims, sdf mode, sphere / constant bias");
        return ASD_ERR_UNSUPPORTED;
    }
    return ASD_OK;
}

// the backward workspace, in floats from its start; every region starts on a 256-byte boundary.  asd_trifield_bwd_workspace returns `total`,
// asd_trifield_bwd takes every pointer from here.
struct tf_bwd_layout {
    int64_t chunk;              // samples per chunk, rows = chunk * (4 with a normal gradient, else 1)
    int64_t denc;               // [rows][96] feature-gradient rows (tfm_bwd_data_kernel)
    int64_t pts;                // [rows][3] the rows' positions in grid_sample coordinates (tfm_bwd_data_kernel)
    int64_t prep;               // tfm_prep_floats(H, W): scales, weight images, padded planes (tfm_prepare)
    int64_t sort_work;          // tfs_work_ints(rows, H, W) ints: the sort's bins and row lists; absent where the sorted scatter does not apply
    int64_t total;
};
static tf_bwd_layout tf_bwd_layout_init(int H, int W, int64_t n, int with_normal) {
    tf_bwd_layout L;
    asd_ws_cursor w;
    L.chunk = n < tf_chunk() ? n : tf_chunk();
    const int64_t rows = L.chunk * (with_normal ? 4 : 1);
    L.denc = w.take(rows * TF_NIN);
    L.pts = w.take(rows * 3);
    L.prep = w.take(tfm_prep_floats(H, W));
    L.sort_work = w.take(tfs_supported(H, W) ? tfs_work_ints((int)rows, H, W) : 0);
    L.total = w.o;
    return L;
}

extern "C" {

int asd_trifield_fwd_workspace(int32_t H, int32_t W, int64_t* n_floats) {
    ASD_CHECK_ARG(n_floats && H > 0 && W > 0, "bad argument");
    *n_floats = tfm_prep_floats(H, W);
    return ASD_OK;
}

int asd_trifield_fwd(const float* planes_cl, int32_t H, int32_t W, int32_t C, const asd_field_cfg* cfg, const float* const* weights /* [host] 6 device pointers:
                     sdf W1^T [96][64], W2 [64][64], W3 [1][64], feature W1^T, W2, W3 [3][64] */, const float* points, int32_t n, float* sdf, float* features,
                     float* normal, float* fd_grad, float* workspace, void* stream) {
    if (n == 0) return ASD_OK;
    ASD_CHECK_ARG(planes_cl && weights && points && sdf && workspace && n > 0, "null argument");
    const int rc = tf_check(cfg, H, W, C);
    if (rc != ASD_OK) return rc;
    const int rp = tfm_prepare(planes_cl, H, W, weights, workspace, (hipStream_t)stream);
    if (rp != ASD_OK) return rp;
    tfm_forward(tf_geom{H, W}, cfg, planes_cl, weights, workspace, points, n, sdf, features, normal, fd_grad, (hipStream_t)stream);
    ASD_LAUNCH_CHECK();
    return ASD_OK;
}

int asd_trifield_bwd_workspace(int32_t H, int32_t W, int32_t n, int32_t with_normal, int64_t* n_floats) {
    ASD_CHECK_ARG(n_floats && n >= 0 && H > 0 && W > 0, "bad argument");
    *n_floats = tf_bwd_layout_init(H, W, n, with_normal).total;
    return ASD_OK;
}

int asd_trifield_bwd(const float* planes_cl, int32_t H, int32_t W, int32_t C, const asd_field_cfg* cfg, const float* const* weights, const float* points,
                     const float* sdf, int32_t n, const float* d_sdf, const float* d_features, const float* d_normal, const float* d_fd_grad, float* d_planes_cl,
                     float* const* d_weights /* [host] 6 device pointers, same shapes (W1 gradients as W1^T), accumulated (+=) */, float* workspace, void* stream) {
    if (n == 0) return ASD_OK;
    ASD_CHECK_ARG(planes_cl && weights && d_weights && points && sdf && d_planes_cl && workspace && n > 0, "null argument");
    const int rc = tf_check(cfg, H, W, C);
    if (rc != ASD_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    const int with_fd = d_normal != nullptr || d_fd_grad != nullptr, npt = with_fd ? 4 : 1;
    const tf_bwd_layout L = tf_bwd_layout_init(H, W, n, with_fd);
    float* const denc = workspace + L.denc;
    float* const pts = workspace + L.pts;
    float* const prep = workspace + L.prep;
    int* const sort_work = (int*)(workspace + L.sort_work);
    const int rp = tfm_prepare(planes_cl, H, W, weights, prep, s);
    if (rp != ASD_OK) return rp;
    for (int64_t i0 = 0; i0 < n; i0 += L.chunk) {
        const int nc = (int)((n - i0) < L.chunk ? (n - i0) : L.chunk);
        const int rows = nc * npt;
        // feature-gradient rows of the chunk; the heads' weight gradients are accumulated by the pass itself
        tfm_backward_chunk(tf_geom{H, W}, cfg, planes_cl, weights, prep, points, sdf, (int)i0, nc, npt, d_sdf, d_features, d_normal, d_fd_grad, denc, pts, d_weights, s);
        // feature gradient -> planes
        if (tfs_supported(H, W)) {
            tfs_scatter(denc, pts, rows, H, W, d_planes_cl, sort_work, s);
        } else {        // planes too large for the sort's LDS bins: run-aggregated atomics (rows in ray order: C5 step 100.9 ms at a run of 8, 93.6 at 128)
            const int rc2 = asd_triplane_sample_bwd_rows(denc, H, W, 32, pts, rows, d_planes_cl, 128, stream);
            if (rc2 != ASD_OK) return rc2;
        }
    }
    ASD_LAUNCH_CHECK();
    return ASD_OK;
}

}  // extern "C"
