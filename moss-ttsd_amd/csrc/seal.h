// The sealed 13-bit form of a lane's bf16 values: encoder and unpack, shared by the KV pages (attn.hip) and the decode
// weight streams (gemm_sealed.hip).  oracle/kv_seal_oracle.py is the executable specification.
#pragma once
#include "common.h"

// ---------------------------------------------------------------------------------------------------
// Sealed pages (common.h: MTTS_PKU).  A bf16 value is [sign | exponent 8 | mantissa 7]; over the 128 values one lane
// reads from a page (a K row; 32 tokens x 4 dims of V) the LOW byte (exponent bit 0 + mantissa) is incompressible, but
// the high byte without its sign (exponent bits 7..1) takes only a handful of distinct values.  A sealed page stores the
// low bytes, a 4-bit code per value (sign, index) and the lane's dictionary of up to 8 such bytes: 13 bits per value,
// exact.  Unpacking one 16-byte unit (8 values) is 12 VALU instructions: the dictionary look-up is a v_perm_b32 whose
// selector is the masked code word, the sign is and-ed back in, two more v_perm interleave high and low bytes.
// ---------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t u4c(const u32x4_t& v, int c) { return c == 0 ? v.x : c == 1 ? v.y : c == 2 ? v.z : v.w; }
// unit j (0..15, compile-time) of the lane's page from its 13 packed registers -> the 4 dwords of the bf16 form
__device__ __forceinline__ void pk_unit(const u32x4_t* pk, int j, uint32_t w[4]) {
    const uint32_t L0 = u4c(pk[j >> 1], 2 * (j & 1)), L1 = u4c(pk[j >> 1], 2 * (j & 1) + 1);
    const uint32_t N = u4c(pk[8 + (j >> 2)], j & 3);
    const uint32_t lo = pk[12].x, hi = pk[12].y;
    const uint32_t HA = ((N & 0x08080808u) << 4) | __builtin_amdgcn_perm(hi, lo, N & 0x07070707u);
    const uint32_t HB = (N & 0x80808080u) | __builtin_amdgcn_perm(hi, lo, (N >> 4) & 0x07070707u);
    w[0] = __builtin_amdgcn_perm(HA, L0, 0x05010400u);
    w[1] = __builtin_amdgcn_perm(HA, L0, 0x07030602u);
    w[2] = __builtin_amdgcn_perm(HB, L1, 0x05010400u);
    w[3] = __builtin_amdgcn_perm(HB, L1, 0x07030602u);
}

// i-th unit to request so that unit j's operands (low (j >> 1), nibbles 8 + (j >> 2), dictionary 12) are complete as
// early as possible: 12, 8, 0, 1, 9, 2, 3, 10, 4, 5, 11, 6, 7
__host__ __device__ constexpr int pk_order(int i) { return i == 0 ? 12 : (i - 1) % 3 == 0 ? 8 + (i - 1) / 3 : 2 * ((i - 1) / 3) + (i - 1) % 3 - 1; }
// One lane's share of a page (16 units of 16 B in registers) -> its sealed form (13 units); `spare` = third dword of unit 12.
// NT = the lane's 16-byte units: 16 (a page; a decode GEMM wave's 16 k-tiles) or 12 (down_proj's wave).  The 12-unit form is
// the 16-unit form of the lane's 96 values followed by 32 copies of its first value (no new high byte) with units 6, 7 and
// 11 dropped: NT / 2 low-byte units, NT / 4 nibble units and the dictionary unit, stored one after another.
template <int NT>
__device__ bool seal_encode(const u32x4_t (&v)[NT], u32x4_t* __restrict__ pk, uint32_t spare, bool unfit) {
    static_assert(NT == 16 || NT == 12, "a sealed group is 16 or 12 units");
    constexpr int DU = NT / 2 + NT / 4;                       // where the dictionary unit is stored
    unsigned long long b0 = 0ull, b1 = 0ull;                  // which of the 128 possible high bytes occur
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const uint32_t e = (u4c(v[j], c) >> (8 + 16 * h)) & 0x7fu;
                if (e & 64u) b1 |= 1ull << (e & 63u);
                else b0 |= 1ull << e;
            }
    const int n0 = __popcll(b0), n = n0 + __popcll(b1);
    if (n > 8 || unfit) {                                     // does not fit: readers take the bf16 page
        pk[DU * 64] = u32x4_t{0u, 0u, spare, 1u};
        return false;
    }
    unsigned long long dict = 0ull;                           // entry i = the i-th smallest high byte present
    {
        unsigned long long t0 = b0, t1 = b1;
        for (int i = 0; i < n; ++i) {
            uint32_t e;
            if (t0) { e = __ffsll((long long)t0) - 1; t0 &= t0 - 1; }
            else { e = 64 + __ffsll((long long)t1) - 1; t1 &= t1 - 1; }
            dict |= (unsigned long long)e << (8 * i);
        }
    }
    auto code = [&](uint32_t half) -> uint32_t {              // 16-bit value -> sign << 3 | rank of its high byte
        const uint32_t e = (half >> 8) & 0x7fu;
        const uint32_t rank = (e & 64u) ? n0 + __popcll(b1 & ((1ull << (e & 63u)) - 1ull)) : __popcll(b0 & ((1ull << e) - 1ull));
        return ((half >> 12) & 8u) | rank;
    };
    uint32_t lowp[2 * NT], nib[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        uint32_t N = 0u;
#pragma unroll
        for (int g = 0; g < 2; ++g) {                         // group A = dwords 0,1 of the unit, B = dwords 2,3
            uint32_t L = 0u;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const uint32_t half = (u4c(v[j], 2 * g + (k >> 1)) >> (16 * (k & 1))) & 0xffffu;
                L |= (half & 0xffu) << (8 * k);
                N |= code(half) << (8 * k + 4 * g);
            }
            lowp[2 * j + g] = L;
        }
        nib[j] = N;
    }
#pragma unroll
    for (int u = 0; u < NT / 2; ++u) pk[u * 64] = u32x4_t{lowp[4 * u], lowp[4 * u + 1], lowp[4 * u + 2], lowp[4 * u + 3]};
#pragma unroll
    for (int u = 0; u < NT / 4; ++u) pk[(NT / 2 + u) * 64] = u32x4_t{nib[4 * u], nib[4 * u + 1], nib[4 * u + 2], nib[4 * u + 3]};
    pk[DU * 64] = u32x4_t{(uint32_t)dict, (uint32_t)(dict >> 32), spare, 0u};
    return true;
}
// The plain form (the format hook; a packed weight array's groups): the lane's NT units as they are.
template <int NT = 16>
__device__ bool seal_lane(const u32x4_t* __restrict__ raw, u32x4_t* __restrict__ pk) {
    u32x4_t v[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) v[j] = raw[j * 64];
    return seal_encode(v, pk, 0u, false);
}
