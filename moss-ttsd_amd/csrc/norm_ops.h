// The arithmetic of "residual add + RMSNorm" (modeling_qwen3.py:299-324, :59-64), one copy: resid_norm_kernel (layer.hip)
// and the kernels that fold its two halves into the GEMMs around it (gemm_fold.hip) call these, so a row gets the same
// bits from either.  A "group" is 8 consecutive elements of a row: what one resid_norm thread owns per 2048-wide chunk,
// one 16-byte unit of the X-fragment layout.
#pragma once
#include "common.h"

// Two fp32 values rounded to bf16 and packed, by the hardware's v_cvt_pk_bf16_f32: one instruction where pack2 (common.h)
// takes about twenty, which is what lets a GEMM block redo a whole tile's norm under its weight loads.  It is the same
// function as f2bf on every one of the 2^32 inputs, NaNs included (layer.hip: bf16_round_check_kernel compares them all;
// tests/test_bf16_round_gpu.py asserts that none differs).
typedef float f32x2_t __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint32_t pack2_rn(float lo, float hi) {
    const f32x2_t v = {lo, hi};
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, bf16x2_t));
}

// x' = bf16(x + bf16(y)) of two elements: the Linear's bf16 output added to the residual stream in bf16
__device__ __forceinline__ uint32_t resid_add2(uint32_t x2, float y0, float y1) {
    const uint32_t y2 = pack2_rn(y0, y1);
    return pack2_rn(bflo(x2) + bflo(y2), bfhi(x2) + bfhi(y2));
}
__device__ __forceinline__ u32x4_t resid_add8(const u32x4_t x, const float4 a, const float4 b) {
    u32x4_t g;
    g.x = resid_add2(x.x, a.x, a.y); g.y = resid_add2(x.y, a.z, a.w);
    g.z = resid_add2(x.z, b.x, b.y); g.w = resid_add2(x.w, b.z, b.w);
    return g;
}

__device__ __forceinline__ void group_unpack(const u32x4_t g, float (&v)[8]) {
    v[0] = bflo(g.x); v[1] = bfhi(g.x); v[2] = bflo(g.y); v[3] = bfhi(g.y);
    v[4] = bflo(g.z); v[5] = bfhi(g.z); v[6] = bflo(g.w); v[7] = bfhi(g.w);
}
// running sum of squares of a thread, continued over one group (elements in ascending order)
__device__ __forceinline__ float group_ss(float ss, const float (&v)[8]) {
#pragma unroll
    for (int j = 0; j < 8; ++j) ss += v[j] * v[j];
    return ss;
}
// the row's sum of squares from the wave sums of its four 64-thread segments, and the scale it gives
__device__ __forceinline__ float norm_total(float s0, float s1, float s2, float s3) { return s0 + s1 + s2 + s3; }
__device__ __forceinline__ float norm_inv(float tot, int H, float eps) { return 1.0f / sqrtf(tot / (float)H + eps); }
// bf16(w * bf16(x' * inv)) of two elements and of one group
__device__ __forceinline__ uint32_t pair_scale(uint32_t w2, float v0, float v1, float inv) {
    const uint32_t t = pack2_rn(v0 * inv, v1 * inv);
    return pack2_rn(bflo(w2) * bflo(t), bfhi(w2) * bfhi(t));
}
__device__ __forceinline__ u32x4_t group_scale(const u32x4_t w, const float (&v)[8], float inv) {
    u32x4_t y;
    y.x = pair_scale(w.x, v[0], v[1], inv);
    y.y = pair_scale(w.y, v[2], v[3], inv);
    y.z = pair_scale(w.z, v[4], v[5], inv);
    y.w = pair_scale(w.w, v[6], v[7], inv);
    return y;
}
