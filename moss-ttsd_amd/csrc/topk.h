// Top-k selection shared by score.hip (forward(top_logprobs=k)) and gen_topk.hip (generate(top_logprobs=k)): the order
// "descending logit, ties by ascending column" as an unsigned compare, 64-bit (value, column) pairs, and a thread's sorted
// list of them in registers.  mtts/topk_spec.py states the order in numpy.
#pragma once
#include "common.h"

// f32_sortable: a monotone map of the floats onto uint32 (-0 counts as +0: the two compare equal, so the column decides).
__device__ __forceinline__ uint32_t f32_sortable(float v) {
    uint32_t u = __float_as_uint(v);
    u = u == 0x80000000u ? 0u : u;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float f32_unsortable(uint32_t s) { return __uint_as_float((s & 0x80000000u) ? (s ^ 0x80000000u) : ~s); }
// (value, column of the head) in 64 bits, the same order; 0 = nothing
__device__ __forceinline__ uint64_t topk_pair(uint32_t sortable, int col) { return ((uint64_t)sortable << 32) | (uint32_t)~(uint32_t)col; }
__device__ __forceinline__ int topk_pair_col(uint64_t c) { return c ? (int)~(uint32_t)c : -1; }
// max over the wave, in every lane (an order-free reduction, like wave_max)
__device__ __forceinline__ uint64_t wave_umax64(uint64_t v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const uint64_t o = ((uint64_t)(uint32_t)__shfl_xor((int)(v >> 32), d) << 32) | (uint32_t)__shfl_xor((int)(uint32_t)v, d);
        v = o > v ? o : v;
    }
    return v;
}
// A thread's KL best pairs, descending, in registers: every index is a compile-time constant.
template <int KL>
struct TopList {
    uint64_t v[KL];
    __device__ __forceinline__ void clear() {
#pragma unroll
        for (int j = 0; j < KL; ++j) v[j] = 0;
    }
    __device__ __forceinline__ uint64_t last() const { return v[KL - 1]; }
    __device__ __forceinline__ void insert(uint64_t c) {      // (c <= last() falls out again)
#pragma unroll
        for (int j = 0; j < KL; ++j) {
            const bool gt = c > v[j];
            const uint64_t t = gt ? v[j] : c;
            v[j] = gt ? c : v[j];
            c = t;
        }
    }
    __device__ __forceinline__ void pop_if(bool own) {
#pragma unroll
        for (int j = 0; j + 1 < KL; ++j) v[j] = own ? v[j + 1] : v[j];
        v[KL - 1] = own ? 0 : v[KL - 1];
    }
};

// list length of the kernels that keep a TopList: the smallest of 1, 4, 8, 16 that holds k (the result does not depend on it)
#define TOPK_DISPATCH(K, CALL)      \
    do {                            \
        if ((K) <= 1) { CALL(1); }  \
        else if ((K) <= 4) { CALL(4); } \
        else if ((K) <= 8) { CALL(8); } \
        else { CALL(16); }          \
    } while (0)
