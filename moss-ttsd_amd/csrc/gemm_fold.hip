// The seam o_proj -> post-attention RMSNorm -> gate/up of the one-row-tile decode step as two launches instead of three
// (DESIGN section 3).  The producer finishes o_proj's split-K sum itself, with the sum tree the split launch and
// resid_norm_kernel have between them, and writes the bf16 residual stream x'; the consumer is gemm_gateup48_kernel with the
// RMSNorm of x' as the prologue of its X operand, run while its weight tiles are in flight.  No fp32 slab reaches memory
// and every block reads the 128 KiB of x' that gate/up reads as X anyway.  The arithmetic is norm_ops.h's (shared with
// resid_norm_kernel) and gemm_epi.h's: the SwiGLU output has the bits of the three launches.
#include "launch.h"
#include "gemm_epi.h"
#include "norm_ops.h"

// ---------------------------------------------------------------------------------------------------
// Producer: x' = bf16(x + bf16(attn * Wo^T)) for one 32-row tile, K = KS * WAVES * KTW k-tiles, un-split.
// Today's tree per element: gemm_depth_kernel<8, 4, 0>'s wave (ks, w) multiplies k-tiles (ks * 8 + w) * 4 + 0..3 ascending
// into one accumulator, its block adds the 8 waves through LDS in wave order (slab ks), resid_norm_kernel adds the slabs as
// ((s0 + s1) + s2) + s3.  Here wave w owns those four k-tiles for every ks, in accumulators acc[ks]; each ks is reduced
// over the waves in wave order, and the lane that holds a column's four sums adds them in ks order, rounds, adds the
// residual and rounds (resid_add2).  x' goes out twice: row-major into the residual stream in place (an element belongs
// to one block) and in the X-fragment layout for the consumer.  Rows >= R are neither read from x nor stored.
// grid = N / 8, block = WAVES * 64: a block owns 8 columns, one register quad q of a weight tile (64 blocks of 32 columns
// were built and timed: 7.3 against 5.8 us).  The 16 lanes that hold the strip's weight rows load them
// and the rest repeat one of those addresses (the trick of gemm_gateup48_kernel's half tile: same cache lines, no branch
// in the load stream), which makes the other quads copies that are dropped.  One quad per (ks, wave) is 32 KiB of LDS in
// all: one barrier, then wave 0 adds the waves of every ks in wave order.  Every block reads the whole X.  All of a wave's
// loads are requested before its first product: KS * KTW X fragments, then KS * KTW weight tiles (32 loads of 16 bytes
// per lane), after the 8 bytes of residual its lane adds.
// ---------------------------------------------------------------------------------------------------
template <int WAVES, int KS, int KTW>
__global__ __launch_bounds__(WAVES * 64) void oproj_resid_kernel(
    const u32x4_t* __restrict__ Wp, const u32x4_t* __restrict__ Xp, int KT, uint16_t* __restrict__ x,
    uint16_t* __restrict__ x_packed, int R, int H) {
    __shared__ float red[WAVES][4 * KS][64];
    const int nt = blockIdx.x >> 2, q = blockIdx.x & 3;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    // the epilogue's element of this lane (wave 0): 4 columns of one row, in register quad q
    const int row = lane & 31, n0 = nt * 32 + 8 * q + 4 * (lane >> 5);
    const bool live = row < R;
    const u32x2_t xo = *(const u32x2_t*)(x + (size_t)(live ? row : 0) * H + n0);
    const int wl = (lane & 32) | (8 * q) | (lane & 7);
    u32x4_t a[KS][KTW], b[KS][KTW];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks)
#pragma unroll
        for (int u = 0; u < KTW; ++u) b[ks][u] = Xp[(size_t)((ks * WAVES + wave) * KTW + u) * 64 + lane];
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int ks = 0; ks < KS; ++ks)
#pragma unroll
        for (int u = 0; u < KTW; ++u) {
            a[ks][u] = __builtin_nontemporal_load(Wp + ((size_t)nt * KT + (ks * WAVES + wave) * KTW + u) * 64 + wl);
            __builtin_amdgcn_sched_barrier(0);                 // requests in the order of use
        }
    f32x16_t acc[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[ks][i] = 0.f;
#pragma unroll
        for (int u = 0; u < KTW; ++u)
            acc[ks] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(*(bf16x8_t*)&a[ks][u], *(bf16x8_t*)&b[ks][u], acc[ks], 0, 0, 0);
    }
#pragma unroll
    for (int ks = 0; ks < KS; ++ks)
#pragma unroll
        for (int j = 0; j < 4; ++j)
            red[wave][4 * ks + j][lane] = q == 0 ? acc[ks][j] : q == 1 ? acc[ks][4 + j] : q == 2 ? acc[ks][8 + j] : acc[ks][12 + j];
    __syncthreads();
    if (wave || !live) return;
    float v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        float s[KS];
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            float t = red[0][4 * ks + j][lane];
#pragma unroll
            for (int w = 1; w < WAVES; ++w) t += red[w][4 * ks + j][lane];
            s[ks] = t;
        }
        float t = s[0];
#pragma unroll
        for (int ks = 1; ks < KS; ++ks) t += s[ks];            // the slabs in the order k = 0, 1, 2, ...
        v[j] = t;
    }
    const u32x2_t o = {resid_add2(xo.x, v[0], v[1]), resid_add2(xo.y, v[2], v[3])};
    *(u32x2_t*)(x + (size_t)row * H + n0) = o;
    *(u32x2_t*)(x_packed + xpack_off(row, n0, H)) = o;         // half of a 16-byte group of the fragment layout
}

// ---------------------------------------------------------------------------------------------------
// Consumer: gemm_gateup48_kernel<8, 16> (gemm.hip: same blocks, tiles, loads, MFMA chain, LDS reduction and epilogue) whose
// X operand is x' and whose prologue is resid_norm_kernel's RMSNorm, replayed while the weight tiles are in flight:
//   * a lane's fragment of k-tile kt is the group of resid_norm thread t = 2 kt + (lane >> 5) of its row: the lane forms
//     that thread's sum of squares (group_ss) and leaves it in LDS as ss[row][t];
//   * wave w replays the block sum for rows 4w .. 4w+3: lane l of segment m takes ss[row][64 m + l], wave_sum gives the
//     segment's sum, norm_total and norm_inv the row's scale;
//   * every lane rewrites its fragments with group_scale, the norm weights coming from a copy in LDS (4 KiB, requested
//     before everything else so that the wait for it does not drain the weight stream).
// The ss rows alias the reduction buffer, which is not in use yet (rows padded to 257 floats: a wave writes 32 rows at
// once).  Requires KT == WAVES * KTW == 128 (H = 2048: 256 groups per row, one per resid_norm thread) and Npad % 96 == 0.
// All 32 rows of the tile are normalised, as gate/up multiplies all 32: the x' buffer holds a whole tile.
// ---------------------------------------------------------------------------------------------------
template <int WAVES, int KTW>
__global__ __launch_bounds__(WAVES * 64) void gemm_gateup48_norm_kernel(
    const u32x4_t* __restrict__ Wp, const u32x4_t* __restrict__ Xp, const u32x4_t* __restrict__ norm_w, float eps, int KT,
    uint16_t* __restrict__ out, int Npad) {
    static_assert(WAVES * KTW == 128 && WAVES == 8, "one resid_norm thread per group: 256 groups per row, 4 rows per wave");
    constexpr int SSP = 257;                                   // padded ss row
    __shared__ float red[WAVES][24][64];
    __shared__ u32x4_t nws[256];
    __shared__ float invs[32];
    static_assert(sizeof(float) * 32 * SSP <= sizeof(float) * WAVES * 24 * 64, "ss fits the reduction buffer");
    const int p = blockIdx.x >> 1, o = blockIdx.x & 1;
    const int tf = 3 * p + 2 * o, th = 3 * p + 1;              // whole tile, shared tile
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int kt0 = wave * KTW;
    const int hl = (((lane >> 4) & 1) == o) ? lane : (lane ^ 16);
    const u32x4_t* wp = Wp + ((size_t)tf * KT + kt0) * 64 + lane;
    const u32x4_t* hp = Wp + ((size_t)th * KT + kt0) * 64 + hl;
    const u32x4_t* xp = Xp + (size_t)kt0 * 64 + lane;
    const u32x4_t nwv = norm_w[threadIdx.x & 255];             // both halves of the block fetch the same 4 KiB: no branch
    u32x4_t a[KTW], h[KTW], b[KTW];
#pragma unroll
    for (int u = 0; u < KTW; ++u) b[u] = xp[(size_t)u * 64];
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int u = 0; u < KTW; ++u) {
        a[u] = __builtin_nontemporal_load(wp + (size_t)u * 64);
        h[u] = __builtin_nontemporal_load(hp + (size_t)u * 64);
        __builtin_amdgcn_sched_barrier(0);                     // requests in the order of use
    }
    // ---- the RMSNorm of x' ----
    float* ssb = &red[0][0][0];
    nws[threadIdx.x & 255] = nwv;
    {
        float* sp = ssb + (lane & 31) * SSP + 2 * kt0 + (lane >> 5);
#pragma unroll
        for (int u = 0; u < KTW; ++u) {
            float v[8];
            group_unpack(b[u], v);
            sp[2 * u] = group_ss(0.f, v);
        }
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float* sr = ssb + (4 * wave + i) * SSP + lane;
        const float s0 = wave_sum(sr[0]), s1 = wave_sum(sr[64]), s2 = wave_sum(sr[128]), s3 = wave_sum(sr[192]);
        const float inv = norm_inv(norm_total(s0, s1, s2, s3), KT * 16, eps);
        if (lane == 0) invs[4 * wave + i] = inv;
    }
    __syncthreads();
    {
        const float inv = invs[lane & 31];
        const u32x4_t* np = nws + 2 * kt0 + (lane >> 5);
#pragma unroll
        for (int u = 0; u < KTW; ++u) {
            // Register budget (48 weight tiles are in flight: 192 registers): the empty asm statements pin a fragment to its
            // four packed registers before and after it is rescaled.  Without them the compiler keeps all 16 fragments
            // unpacked since the sums of squares (128 registers instead of 64).
            asm volatile("" : "+v"(b[u]));
            float v[8];
            group_unpack(b[u], v);
            b[u] = group_scale(np[2 * u], v, inv);
            asm volatile("" : "+v"(b[u]));
        }
    }
    // ---- gemm_gateup48_kernel from here on (the ss rows were last read before the second barrier) ----
    f32x16_t acc, acch;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = acch[i] = 0.f;
#pragma unroll
    for (int u = 0; u < KTW; ++u) {
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(*(bf16x8_t*)&a[u], *(bf16x8_t*)&b[u], acc, 0, 0, 0);
        acch = __builtin_amdgcn_mfma_f32_32x32x16_bf16(*(bf16x8_t*)&h[u], *(bf16x8_t*)&b[u], acch, 0, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) red[wave][r][lane] = acc[r];
#pragma unroll
    for (int r = 0; r < 8; ++r) red[wave][16 + r][lane] = o ? acch[8 + r] : acch[r];   // quads 2o, 2o + 1 are ours
    __syncthreads();
    for (int q6 = wave; q6 < 6; q6 += WAVES) {                 // quads 0..3: whole tile; 4, 5: our half of the shared tile
        float v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float s = red[0][4 * q6 + j][lane];
#pragma unroll
            for (int w = 1; w < WAVES; ++w) s += red[w][4 * q6 + j][lane];
            v[j] = s;
        }
        const int nt = q6 < 4 ? tf : th, q = q6 < 4 ? q6 : 2 * o + (q6 - 4);
        skinny_store<EPI_SILU>(v, lane & 31, nt * 32 + 8 * q + 4 * (lane >> 5), 0, nullptr, out, Npad, Npad);
    }
}

// The pair takes the shapes its kernels are built for: o_proj as gemm_depth_kernel<8, 4, 0> with split-K 4 (K = 2048), gate/up
// as gemm_gateup48_kernel<8, 16> (K = H = 2048, 2 I % 96 == 0), depth-specialised kernels enabled in both plans.
bool fold_norm_shape(const GemmPlan& p_o, int K_o, const GemmPlan& p_gu, int H, int N_gu) {
    return p_o.depth && p_gu.depth && p_o.waves == 8 && p_o.ksplit == 4 && p_o.kt_per_wave == 4 && p_o.kt_per_split == 32 &&
           K_o == 2048 && p_gu.waves == 8 && p_gu.ksplit == 1 && p_gu.kt_per_wave == 16 && H == 2048 && N_gu > 0 && N_gu % 96 == 0;
}
static long long g_fold_launches = 0;       // launches of either kernel (test hook: mtts_debug_fold_norm_launches)
long long mtts_fold_norm_launches() { return g_fold_launches; }

// x [R][N] bf16 row-major += attn (packed, 32 x 2048) * Wo^T (packed [N][2048]), in place; x_packed [32][N] receives rows < R
void launch_oproj_resid(const void* Wp, const void* Xp, void* x, void* x_packed, int R, int N, hipStream_t st) {
    hipLaunchKernelGGL((oproj_resid_kernel<8, 4, 4>), dim3(N / 8), dim3(512), 0, st, (const u32x4_t*)Wp, (const u32x4_t*)Xp, 128,
                       (uint16_t*)x, (uint16_t*)x_packed, R, N);
    ++g_fold_launches;
}
// out (packed, 32 x Npad / 2) = SwiGLU(RMSNorm(x') * norm_w times Wgu^T): x_packed [32][2048], Wgu packed [Npad][2048]
void launch_gateup_norm(const void* Wp, const void* x_packed, const void* norm_w, float eps, void* out, int Npad, hipStream_t st) {
    hipLaunchKernelGGL((gemm_gateup48_norm_kernel<8, 16>), dim3(Npad / 48), dim3(512), 0, st, (const u32x4_t*)Wp,
                       (const u32x4_t*)x_packed, (const u32x4_t*)norm_w, eps, 128, (uint16_t*)out, Npad);
    ++g_fold_launches;
}
