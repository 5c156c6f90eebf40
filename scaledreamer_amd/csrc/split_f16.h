// split_f16.h — fp32 mathematics on the fp16 matrix pipe: THE split-fp16 scheme of conv3d.hip, trifield_mfma.hip, field_mfma.hip and tritx.hip.
//
// gfx950 has no reduced-precision fp32 matrix path (no xf32; v_mfma_f32_*_f32 runs at the vector rate, 1/16 of fp16), so every fp32 operand is
// SPLIT into two fp16 planes
//     x * s = hi + lo,   hi = fp16(x * s),  lo = fp16(x * s - hi)        (s: a power of two that puts max|x| into [2^TOP, 2^(TOP + 1)))
// and a product of two operands is formed from three fp16 MFMA products with fp32 accumulation,
//     a . b  =  a_hi b_hi + a_hi b_lo + a_lo b_hi      (+ a_lo b_lo ~ 2^-22 |a||b|, dropped),
// i.e. 22 significant bits per operand (fp32 has 24) at 1/3 of the fp16 MFMA rate instead of 1/16.  Products of fp16 values are exact in
// fp32, so the only roundings are the two splits and the fp32 accumulation the library path has as well.  What the scale spans (a tensor, a
// head, a row of the operand as the contraction sees it) is the caller's choice; it factors out of the product either way.
#pragma once
#include "asd_common.h"

// scale = 2^(TOP - floor(log2 amax)) from max|x| (or its bit pattern: non-negative floats order like their bit patterns, which is how the absmax
// kernels commit it).  ONE guard rule: zero (nothing to scale) or not finite (nothing to save) gives 1; the exponent is clamped to [-100, EMAX],
// so the scale and its reciprocal are always normal numbers.  EMAX = 100 where one scale spans a tensor, a head or a tile.  tritx.hip, whose
// scales are per ROW, takes 126: a row far below fp32's normal range (maximum 2^-130: exponent field 0, scale 2^126) then lands at 2^-4, where
// hi and lo (fp16 down to 2^-24) still hold every bit such a row has, instead of at 2^-30, below fp16 altogether.
// TOP = 14 leaves fp16 (max 65504 < 2^16) one bit above the largest element; field_mfma.hip takes 13 (see there).
template <int TOP, int EMAX = 100>
__device__ __forceinline__ float asd_split_scale_bits(unsigned amax_bits) {
    static_assert(EMAX <= 126, "1 / scale must stay a normal number");
    if (amax_bits == 0u || amax_bits >= 0x7f800000u) return 1.f;
    int se = TOP - ((int)((amax_bits >> 23) & 0xffu) - 127);
    se = se > EMAX ? EMAX : (se < -100 ? -100 : se);
    return __int_as_float((unsigned)(se + 127) << 23);
}
template <int TOP, int EMAX = 100>
__device__ __forceinline__ float asd_split_scale(float amax) { return asd_split_scale_bits<TOP, EMAX>(__float_as_uint(amax)); }

// hi / lo of an already scaled value; of eight values times s
__device__ __forceinline__ void asd_split(float scaled, half_t& hi, half_t& lo) {
    hi = (half_t)scaled;
    lo = (half_t)(scaled - (float)hi);
}
__device__ __forceinline__ void asd_split8(const float (&x)[8], float s, half8& hi, half8& lo) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const float v = x[j] * s;       // asd_split written out: through it hipcc schedules field_mfma.hip's kernel differently (tools/asm_same.py)
        const half_t h = (half_t)v;
        hi[j] = h;
        lo[j] = (half_t)(v - (float)h);
    }
}

// acc += a . b as hi.hi + hi.lo + lo.hi, one overload per MFMA shape
__device__ __forceinline__ floatx4 asd_mma3(const half8 ah, const half8 al, const half8 bh, const half8 bl, floatx4 acc) {
    acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, bh, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, bl, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(al, bh, acc, 0, 0, 0);
    return acc;
}
__device__ __forceinline__ floatx16 asd_mma3(const half8 ah, const half8 al, const half8 bh, const half8 bl, floatx16 acc) {
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bh, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bl, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, bh, acc, 0, 0, 0);
    return acc;
}

// The 32x32 accumulator keeps a column in lanes l and l ^ 32: v_permlane32_swap exchanges the two halves of the wave on the vector pipe (no LDS
// round trip).  x: lanes 32-63 <-> y: lanes 0-31 ...
__device__ __forceinline__ void asd_half_swap(float& x, float& y) {
    const auto t = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(y), false, false);
    x = __uint_as_float(t[0]);
    y = __uint_as_float(t[1]);
}
// ... and the value of lane l ^ 32
__device__ __forceinline__ float asd_other_half(float v) {
    float x = v, y = v;
    asd_half_swap(x, y);
    return ((threadIdx.x >> 5) & 1) ? x : y;
}
