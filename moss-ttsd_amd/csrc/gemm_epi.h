// The epilogue of the one-row-tile decode GEMMs (gemm.hip, gemm_sealed.hip): one copy, so a column gets the same bits from either.
#pragma once
#include "launch.h"

// v: 4 consecutive columns n0.. of activation row `row`, summed over the block's waves
template <int EPI>
__device__ __forceinline__ void skinny_store(const float (&v)[4], int row, int n0, int ks, float* __restrict__ partial,
                                             uint16_t* __restrict__ out, int Npad, int n_valid) {
    if (EPI == EPI_PARTIAL) {
        *(float4*)(partial + ((size_t)ks * MTTS_PFCAP + row) * Npad + n0) = make_float4(v[0], v[1], v[2], v[3]);
    } else if (EPI == EPI_BF16) {
        uint16_t* o = out + (size_t)row * Npad + n0;
        if (n0 + 3 < n_valid) *(u32x2_t*)o = u32x2_t{pack2(v[0], v[1]), pack2(v[2], v[3])};
        else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (n0 + j < n_valid) o[j] = f2bf(v[j]);
        }
    } else {                                                   // SwiGLU, rounding points and layout of gemm_skinny_kernel
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            float g = rbf(v[2 * j]), u = rbf(v[2 * j + 1]);
            float a = rbf(g / (1.0f + expf(-g)));
            out[xpack_off(row, (n0 >> 1) + j, Npad >> 1)] = f2bf(a * u);
        }
    }
}
