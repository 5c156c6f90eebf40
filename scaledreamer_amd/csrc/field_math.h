// field_math.h — the per-point arithmetic the field kernels share (field.hip, field_analytic.hip): density bias, density
// activation and the two VanillaMLP forms.  Moved here from field.hip unchanged, so every kernel that includes it rounds alike.
#pragma once
#include "asd_common.h"

#ifdef __HIPCC__
__device__ __forceinline__ float field_bias(const asd_field_cfg& c, float px, float py, float pz) {
    const float r2 = px * px + py * py + pz * pz;
    if (c.bias_mode == ASD_BIAS_BLOB_MAGIC3D) return c.blob_scale * (1.f - sqrtf(r2) / c.blob_std);
    if (c.bias_mode == ASD_BIAS_BLOB_DREAMFUSION) return c.blob_scale * expf(-0.5f * r2 / (c.blob_std * c.blob_std));
    if (c.bias_mode == ASD_BIAS_SPHERE) return sqrtf(r2) - c.bias_value;
    return c.bias_value;
}
__device__ __forceinline__ float field_act(const asd_field_cfg& c, float raw) {
    switch (c.activation) {
        case ASD_ACT_SOFTPLUS: return asd_softplus(raw);
        case ASD_ACT_EXP:
        case ASD_ACT_TRUNC_EXP: return expf(raw);
        default: return raw;
    }
}
__device__ __forceinline__ float field_act_grad(const asd_field_cfg& c, float raw) {
    switch (c.activation) {
        case ASD_ACT_SOFTPLUS: return raw > 20.f ? 1.f : asd_sigmoid(raw);
        case ASD_ACT_EXP: return expf(raw);
        case ASD_ACT_TRUNC_EXP: return expf(fminf(raw, 15.f));
        default: return 1.f;
    }
}

// out = W2 . relu(W1 . enc), single output.  Weight addresses are wave-uniform (scalar loads).
template <int NIN, int H>
__device__ __forceinline__ float mlp1(const float* __restrict__ w1, const float* __restrict__ w2,
                                      const float (&enc)[NIN]) {
    float out = 0.f;
#pragma unroll 4
    for (int h = 0; h < H; ++h) {
        float a = 0.f;
#pragma unroll
        for (int k = 0; k < NIN; ++k) a = fmaf(w1[h * NIN + k], enc[k], a);
        out = fmaf(w2[h], fmaxf(a, 0.f), out);
    }
    return out;
}
template <int NIN, int H, int C>
__device__ __forceinline__ void mlpC(const float* __restrict__ w1, const float* __restrict__ w2,
                                     const float (&enc)[NIN], float (&out)[C]) {
#pragma unroll
    for (int o = 0; o < C; ++o) out[o] = 0.f;
#pragma unroll 4
    for (int h = 0; h < H; ++h) {
        float a = 0.f;
#pragma unroll
        for (int k = 0; k < NIN; ++k) a = fmaf(w1[h * NIN + k], enc[k], a);
        a = fmaxf(a, 0.f);
#pragma unroll
        for (int o = 0; o < C; ++o) out[o] = fmaf(w2[o * H + h], a, out[o]);
    }
}
#endif  // __HIPCC__

// ---- the fixed-order first-layer weight-gradient reduction of field.hip, for the other field files ------------------------------
// slabs[b][128][32] = sum over chunk b's rows of DA[row][0:128]^T . ENC[row][0:32] (field_wgrad_kernel; rows < rows_a read enc_a, the rest
// enc_b), then out[j] += sum_b slabs[b * stride + j] in a fixed order (slab_reduce_kernel).  asd_field_wgrad_chunks(rows) slabs are written.
// (library-internal: not part of include/asd_hip.h)
extern "C" {
int asd_field_wgrad_chunks(int64_t rows);
// The whole tail: field_wgrad_kernel over n_slabs chunks (unless slabs_written: another pass left n_slabs slabs), then dw1_density += the slabs'
// density half and, with a feature network (dw1_feature != NULL), dw1_feature += their feature half.  n_dev (optional): device-side count of the
// live centre rows; rows_a is its bound.
void asd_field_wgrad_tail(const float* da, const float* enc_a, const float* enc_b, int rows_a, int rows_total, const int* n_dev, bool slabs_written,
                          float* slabs, int n_slabs, float* dw1_density, float* dw1_feature, hipStream_t s);
void asd_field_slab_reduce_launch(const float* slabs, int n_slabs, int stride, int len, float* out, hipStream_t s);
// 1 if the fused field kernels are built for this grid and configuration; otherwise 0 and the error text, which names `what` kernels
int asd_field_supported(const asd_grid_meta* m, const asd_field_cfg* c, const char* what);
}
