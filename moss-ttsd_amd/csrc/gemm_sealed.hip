// Decode GEMMs that read their weights in the sealed 13-bit form (seal.h), and the sealer that makes that form at bind time.
//
// A packed weight array (common.h: wpack_off) is Wp[(nt * KT + kt) * 64 + lane], 16 bytes per lane: the KTW consecutive
// k-tiles a wave of the depth-specialised kernels owns (gemm.hip) are KTW KiB in a row, lane-indexed with unit stride 64 --
// a KV page's layout when KTW = 16 -- and a lane's 8 KTW values are one weight row over 8 KTW consecutive k.  Such a GROUP
// is sealed once, when the matrix is bound, into KTW / 2 low-byte units, KTW / 4 nibble units and the dictionary unit:
// 13 KiB instead of 16 (KTW = 16), 10 instead of 12 (down_proj's 12).  Ws[((nt * KT / KTW + c) * NU + unit) * 64 + lane].
//
// The kernels below are the twins of gemm_depth_kernel / gemm_gateup48_kernel / gemm_skinny_kernel<8, EPI_BF16, 1>: same
// grid, same wave -> k-tile assignment, products in the same ascending order into one accumulator, the same LDS sum in
// wave order and the same epilogue (gemm_epi.h).  pk_unit gives back the exact 4 dwords of the bf16 tile, so the results
// are the same bits.  A group with a lane that did not fit (more than 8 distinct high bytes) is flagged in its dictionary
// unit, which is requested first; its wave takes the bf16 tiles instead: requested the moment the ballot is known where
// the registers allow it (down_proj), in two halves behind the sealed units where they do not.  That path costs a launch
// that is one round trip long about what sealing saves it, hence the per-kind bounds of engine.h: WSEAL_MAX_UNSEALED.
#include "launch.h"
#include "gemm_epi.h"
#include "seal.h"

// a stored group: where unit u of the 16-unit form (0-7 low bytes, 8-11 nibbles, 12 dictionary) sits, and how many there are
template <int KTW> __host__ __device__ constexpr int su_pos(int u) { return u < 8 ? u : u < 12 ? KTW / 2 + (u - 8) : KTW / 2 + KTW / 4; }
template <int KTW> __host__ __device__ constexpr int su_count() { return KTW / 2 + KTW / 4 + 1; }

// ---- bind time ------------------------------------------------------------------------------------------------------
// grid = (KT / KTW, tiles), block 64: one group per wave, N-tiles nt0 .. nt0 + gridDim.y - 1
template <int KTW>
__global__ __launch_bounds__(64) void wseal_kernel(const u32x4_t* __restrict__ Wp, u32x4_t* __restrict__ Ws, int KT, int nt0) {
    const int nt = nt0 + blockIdx.y, c = blockIdx.x, lane = threadIdx.x;
    seal_lane<KTW>(Wp + ((size_t)nt * KT + (size_t)c * KTW) * 64 + lane,
                   Ws + ((size_t)nt * (KT / KTW) + c) * (su_count<KTW>() * 64) + lane);
}
// groups whose flag is set, from the dictionary units alone; grid = ceil(groups / 4), block 256; out = {groups, not sealed}
__global__ __launch_bounds__(256) void wseal_count_kernel(const u32x4_t* __restrict__ Ws, size_t groups, int nu,
                                                          unsigned long long* __restrict__ out) {
    const size_t g = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (g >= groups) return;
    const int lane = threadIdx.x & 63;
    const u32x4_t d = Ws[(g * nu + (nu - 1)) * 64 + lane];
    const bool bad = __ballot(d.w != 0u) != 0ull;
    if (lane == 0) {
        atomicAdd(out, 1ull);
        if (bad) atomicAdd(out + 1, 1ull);
    }
}

// ---- the readers ----------------------------------------------------------------------------------------------------
// the lane's sealed group into pk[] (indexed as the 16-unit form; the slots a 12-tile group does not have stay unused),
// requested in pk_order: the dictionary unit first, then every unit as early as its first product needs it
template <int KTW>
__device__ __forceinline__ void sealed_request(u32x4_t (&pk)[MTTS_PKU], const u32x4_t* __restrict__ g) {
#pragma unroll
    for (int i = 0; i < su_count<KTW>(); ++i) {
        pk[pk_order(i)] = __builtin_nontemporal_load(g + su_pos<KTW>(pk_order(i)) * 64);
        __builtin_amdgcn_sched_barrier(0);
    }
}
template <int KTW>
__device__ __forceinline__ void plain_request(u32x4_t (&a)[KTW], const u32x4_t* __restrict__ w) {
#pragma unroll
    for (int u = 0; u < KTW; ++u) {
        a[u] = __builtin_nontemporal_load(w + (size_t)u * 64);
        __builtin_amdgcn_sched_barrier(0);
    }
}
template <int KTW>
__device__ __forceinline__ f32x16_t sealed_chain(const u32x4_t (&pk)[MTTS_PKU], const u32x4_t (&b)[KTW], f32x16_t acc) {
#pragma unroll
    for (int u = 0; u < KTW; ++u) {
        uint32_t w[4];
        pk_unit(pk, u, w);
        const u32x4_t a = {w[0], w[1], w[2], w[3]};
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(*(const bf16x8_t*)&a, *(const bf16x8_t*)&b[u], acc, 0, 0, 0);
    }
    return acc;
}
template <int KTW>
__device__ __forceinline__ f32x16_t plain_chain(const u32x4_t (&a)[KTW], const u32x4_t (&b)[KTW], f32x16_t acc) {
#pragma unroll
    for (int u = 0; u < KTW; ++u)
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(*(const bf16x8_t*)&a[u], *(const bf16x8_t*)&b[u], acc, 0, 0, 0);
    return acc;
}
// a not-sealed group where other loads hold registers (a second group; the next tile's units): the wave's bf16 tiles in two
// halves, k ascending all the same -- two round trips for that wave, and no scratch
template <int KTW>
__device__ __forceinline__ f32x16_t plain_halves(const u32x4_t* __restrict__ w, const u32x4_t (&b)[KTW], f32x16_t acc) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        u32x4_t a[KTW / 2], bh[KTW / 2];
#pragma unroll
        for (int u = 0; u < KTW / 2; ++u) bh[u] = b[h * (KTW / 2) + u];
        plain_request<KTW / 2>(a, w + (size_t)h * (KTW / 2) * 64);
        acc = plain_chain<KTW / 2>(a, bh, acc);
        __builtin_amdgcn_sched_barrier(0);
    }
    return acc;
}
// The compiler sinks a load whose only readers sit behind a branch into that branch: the units would be requested after
// the flag is back, two round trips in a row.  The not-sealed path therefore "reads" them too (no instruction).
__device__ __forceinline__ void sealed_touch(const u32x4_t (&pk)[MTTS_PKU]) {
#pragma unroll
    for (int i = 0; i < MTTS_PKU; ++i) asm volatile("" ::"v"(pk[i]));
    __builtin_amdgcn_sched_barrier(0);
}
__device__ __forceinline__ f32x16_t zero16() {
    f32x16_t z;
#pragma unroll
    for (int i = 0; i < 16; ++i) z[i] = 0.f;
    return z;
}
template <int WAVES, int EPI>
__device__ __forceinline__ void reduce_store(float (&red)[WAVES][16][64], int wave, int lane, int nt, int ks, float* __restrict__ partial,
                                             uint16_t* __restrict__ out, int Npad, int n_valid) {
    for (int q = wave; q < 4; q += WAVES) {                    // q: register quad 4q..4q+3
        float v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float s = red[0][4 * q + j][lane];
#pragma unroll
            for (int w = 1; w < WAVES; ++w) s += red[w][4 * q + j][lane];
            v[j] = s;
        }
        skinny_store<EPI>(v, lane & 31, nt * 32 + 8 * q + 4 * (lane >> 5), ks, partial, out, Npad, n_valid);
    }
}

// gemm_depth_kernel's twin (down_proj: <8, 12, EPI_PARTIAL>; a head tile per block: <8, 16, EPI_BF16>).
// grid = (N/32, ksplit); block = WAVES*64; requires KT == ksplit * WAVES * KTW.
template <int WAVES, int KTW, int EPI>
__global__ __launch_bounds__(WAVES * 64) void depth_sealed_kernel(
    const u32x4_t* __restrict__ Ws, const u32x4_t* __restrict__ Wp, const u32x4_t* __restrict__ Xp, int KT, float* __restrict__ partial,
    uint16_t* __restrict__ out, int Npad, int n_valid) {
    __shared__ float red[WAVES][16][64];
    const int nt = blockIdx.x, ks = blockIdx.y;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int c = ks * WAVES + wave, kt0 = c * KTW;
    const u32x4_t* xp = Xp + (size_t)kt0 * 64 + lane;
    u32x4_t b[KTW], pk[MTTS_PKU];
#pragma unroll
    for (int u = 0; u < KTW; ++u) b[u] = xp[(size_t)u * 64];
    __builtin_amdgcn_sched_barrier(0);
    sealed_request<KTW>(pk, Ws + ((size_t)nt * (KT / KTW) + c) * (su_count<KTW>() * 64) + lane);
    f32x16_t acc = zero16();
    if (__builtin_expect(__ballot(pk[12].w != 0u) != 0ull, 0)) {           // a lane did not fit: this wave's bf16 tiles
        u32x4_t a[KTW];
        plain_request<KTW>(a, Wp + ((size_t)nt * KT + kt0) * 64 + lane);
        sealed_touch(pk);
        acc = plain_chain<KTW>(a, b, acc);
    } else acc = sealed_chain<KTW>(pk, b, acc);
#pragma unroll
    for (int r = 0; r < 16; ++r) red[wave][r][lane] = acc[r];
    __syncthreads();
    reduce_store<WAVES, EPI>(red, wave, lane, nt, ks, partial, out, Npad, n_valid);
}

// gemm_gateup48_kernel's twin: block b = 2p + o takes the whole tile 3p + 2o and its half of tile 3p + 1; the lanes that do
// not hold the half tile's rows repeat lane ^ 16 -- units are lane-indexed, dictionary included, so the trick carries over.
// Per wave: KTW X fragments, then the two groups' units.  Requires KT == WAVES * KTW and Npad % 96 == 0.
template <int WAVES, int KTW>
__global__ __launch_bounds__(WAVES * 64) void gateup48_sealed_kernel(
    const u32x4_t* __restrict__ Ws, const u32x4_t* __restrict__ Wp, const u32x4_t* __restrict__ Xp, int KT, uint16_t* __restrict__ out, int Npad) {
    __shared__ float red[WAVES][24][64];
    constexpr int NU = su_count<KTW>();
    const int p = blockIdx.x >> 1, o = blockIdx.x & 1;
    const int tf = 3 * p + 2 * o, th = 3 * p + 1;              // whole tile, shared tile
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int kt0 = wave * KTW;
    const int hl = (((lane >> 4) & 1) == o) ? lane : (lane ^ 16);
    const u32x4_t* xp = Xp + (size_t)kt0 * 64 + lane;
    u32x4_t b[KTW], pw[MTTS_PKU], ph[MTTS_PKU];
#pragma unroll
    for (int u = 0; u < KTW; ++u) b[u] = xp[(size_t)u * 64];
    __builtin_amdgcn_sched_barrier(0);
    sealed_request<KTW>(pw, Ws + ((size_t)tf * WAVES + wave) * (NU * 64) + lane);
    sealed_request<KTW>(ph, Ws + ((size_t)th * WAVES + wave) * (NU * 64) + hl);
    f32x16_t acc = zero16(), acch = zero16();
    if (__builtin_expect(__ballot((pw[12].w | ph[12].w) != 0u) != 0ull, 0)) {
        // One tile after the other and each in two halves, in the registers of the sealed units: no scratch, at the price of
        // four round trips for this wave (one request of 16 tiles per group was tried: with two groups' units and the X
        // fragments held, the register allocator spills).  It is why gate/up is not in the default dispatch.
        sealed_touch(pw);
        sealed_touch(ph);
        acc = plain_halves<KTW>(Wp + ((size_t)tf * KT + kt0) * 64 + lane, b, acc);
        acch = plain_halves<KTW>(Wp + ((size_t)th * KT + kt0) * 64 + hl, b, acch);
    } else {
#pragma unroll
        for (int u = 0; u < KTW; ++u) {
            uint32_t w[4], v[4];
            pk_unit(pw, u, w);
            pk_unit(ph, u, v);
            const u32x4_t a = {w[0], w[1], w[2], w[3]}, h = {v[0], v[1], v[2], v[3]};
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(*(const bf16x8_t*)&a, *(const bf16x8_t*)&b[u], acc, 0, 0, 0);
            acch = __builtin_amdgcn_mfma_f32_32x32x16_bf16(*(const bf16x8_t*)&h, *(const bf16x8_t*)&b[u], acch, 0, 0, 0);
        }
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

// The heads: one N-tile is computed exactly as by depth_sealed_kernel<8, 16, EPI_BF16>, but the grid of that kernel is ~19
// rounds deep (4 772 tiles at V0 = 152 697), every block re-reading its 128 KiB of X and paying its own ramp.  Here a
// block is persistent over the tiles blockIdx.x, + gridDim.x, ...: the wave's X fragments stay in registers, and tile
// t + 1's units are requested before tile t's products.  The LDS sum alternates between two buffers, one barrier a tile.
// grid = min(tiles, CUs); requires KT == WAVES * KTW.
template <int WAVES, int KTW, bool NEXT>
__device__ __forceinline__ void head_tile(float (&red)[WAVES][16][64], const u32x4_t (&b)[KTW], const u32x4_t (&pk)[MTTS_PKU],
                                          u32x4_t (&nx)[MTTS_PKU], const u32x4_t* __restrict__ Ws, const u32x4_t* __restrict__ Wp, int KT,
                                          int nt, int nt_next, int wave, int lane, uint16_t* __restrict__ out, int Npad, int n_valid) {
    const bool bad = __ballot(pk[12].w != 0u) != 0ull;
    if (NEXT) sealed_request<KTW>(nx, Ws + ((size_t)nt_next * WAVES + wave) * (su_count<KTW>() * 64) + lane);
    f32x16_t acc = zero16();
    if (__builtin_expect(bad, 0)) {
        sealed_touch(pk);                                      // (the next tile's units stay in flight behind them)
        acc = plain_halves<KTW>(Wp + ((size_t)nt * KT + (size_t)wave * KTW) * 64 + lane, b, acc);
    } else acc = sealed_chain<KTW>(pk, b, acc);
#pragma unroll
    for (int r = 0; r < 16; ++r) red[wave][r][lane] = acc[r];
    __syncthreads();
    reduce_store<WAVES, EPI_BF16>(red, wave, lane, nt, 0, nullptr, out, Npad, n_valid);
}
template <int WAVES, int KTW>
__global__ __launch_bounds__(WAVES * 64) void head_sealed_kernel(
    const u32x4_t* __restrict__ Ws, const u32x4_t* __restrict__ Wp, const u32x4_t* __restrict__ Xp, int KT, int ntiles,
    uint16_t* __restrict__ out, int Npad, int n_valid) {
    __shared__ float red[2][WAVES][16][64];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int stride = gridDim.x;
    int nt = blockIdx.x;
    if (nt >= ntiles) return;
    const u32x4_t* xp = Xp + (size_t)wave * KTW * 64 + lane;
    u32x4_t b[KTW], pa[MTTS_PKU], pb[MTTS_PKU];
#pragma unroll
    for (int u = 0; u < KTW; ++u) b[u] = xp[(size_t)u * 64];
    __builtin_amdgcn_sched_barrier(0);
    sealed_request<KTW>(pa, Ws + ((size_t)nt * WAVES + wave) * (su_count<KTW>() * 64) + lane);
    // two tiles a turn, the unit registers changing roles (no copies: a copy would wait for the units it moves)
    for (;;) {
        if (nt + stride >= ntiles) { head_tile<WAVES, KTW, false>(red[0], b, pa, pb, Ws, Wp, KT, nt, 0, wave, lane, out, Npad, n_valid); break; }
        head_tile<WAVES, KTW, true>(red[0], b, pa, pb, Ws, Wp, KT, nt, nt + stride, wave, lane, out, Npad, n_valid);
        nt += stride;
        if (nt + stride >= ntiles) { head_tile<WAVES, KTW, false>(red[1], b, pb, pa, Ws, Wp, KT, nt, 0, wave, lane, out, Npad, n_valid); break; }
        head_tile<WAVES, KTW, true>(red[1], b, pb, pa, Ws, Wp, KT, nt, nt + stride, wave, lane, out, Npad, n_valid);
        nt += stride;
    }
}

// ---- host side ------------------------------------------------------------------------------------------------------
size_t wseal_bytes(int Npad, int K, int ktw) {
    const int nu = ktw / 2 + ktw / 4 + 1;
    return (size_t)(Npad / 32) * (K / 16 / ktw) * nu * 1024;
}
bool wseal_shape(const GemmPlan& p, int K, int Npad, int epi) {
    const int KT = K / 16;
    if (p.waves != 8 || K % 16 || Npad % 32 || KT != p.ksplit * 8 * p.kt_per_wave || p.kt_per_split != 8 * p.kt_per_wave) return false;
    if (epi == EPI_PARTIAL) return p.kt_per_wave == 12;
    if (epi == EPI_SILU) return p.ksplit == 1 && p.kt_per_wave == 16 && Npad % 96 == 0;
    if (epi == EPI_BF16) return p.ksplit == 1 && p.kt_per_wave == 16;
    return false;
}
void launch_wseal(const void* Wp, void* Ws, int K, int ktw, int nt0, int ntiles, hipStream_t st) {
    const int KT = K / 16;
    if (ntiles < 1) return;
    for (int t = 0; t < ntiles; t += 32768) {                 // (gridDim.y is 16 bits)
        const dim3 grid(KT / ktw, std::min(ntiles - t, 32768));
        if (ktw == 16) hipLaunchKernelGGL((wseal_kernel<16>), grid, dim3(64), 0, st, (const u32x4_t*)Wp, (u32x4_t*)Ws, KT, nt0 + t);
        else hipLaunchKernelGGL((wseal_kernel<12>), grid, dim3(64), 0, st, (const u32x4_t*)Wp, (u32x4_t*)Ws, KT, nt0 + t);
    }
}
void launch_wseal_count(const void* Ws, int Npad, int K, int ktw, unsigned long long* out2, hipStream_t st) {
    const size_t groups = (size_t)(Npad / 32) * (K / 16 / ktw);
    hipLaunchKernelGGL(wseal_count_kernel, dim3((unsigned)((groups + 3) / 4)), dim3(256), 0, st, (const u32x4_t*)Ws, groups,
                       ktw / 2 + ktw / 4 + 1, out2);
}

static long long g_wseal_launches = 0;      // launches that took a sealed kernel (test hook: mtts_debug_wseal_launches)
long long mtts_wseal_launches() { return g_wseal_launches; }
static int head_grid(int ntiles) {
    static int cus = 0;
    if (!cus) {
        int dev = 0, n = 0;
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n < 1) n = 256;
        cus = n;
    }
    return std::min(ntiles, cus);
}
// The sealed twin of launch_gemm for the shapes wseal_shape accepts (one activation tile).  false: not such a call, nothing
// was launched and the caller runs launch_gemm.  head_form (EPI_BF16): 1 the persistent kernel on one block per CU, 0 one
// tile per block, n > 1 the persistent kernel on n blocks (tests: a block's tile loop at small N).
bool launch_gemm_sealed(int epi, int mb, const GemmPlan& p, const void* Ws, const void* Wp, const void* Xp, int K, int Npad,
                        int n_valid, float* partial, uint16_t* out, int head_form, hipStream_t st) {
    if (!Ws || !p.depth || mb > 1 || !wseal_shape(p, K, Npad, epi)) return false;
    const int KT = K / 16;
    if (epi == EPI_PARTIAL)
        hipLaunchKernelGGL((depth_sealed_kernel<8, 12, EPI_PARTIAL>), dim3(Npad / 32, p.ksplit), dim3(512), 0, st, (const u32x4_t*)Ws,
                           (const u32x4_t*)Wp, (const u32x4_t*)Xp, KT, partial, out, Npad, n_valid);
    else if (epi == EPI_SILU) {
        if (n_valid != Npad) return false;
        hipLaunchKernelGGL((gateup48_sealed_kernel<8, 16>), dim3(Npad / 48), dim3(512), 0, st, (const u32x4_t*)Ws, (const u32x4_t*)Wp,
                           (const u32x4_t*)Xp, KT, out, Npad);
    } else if (head_form)
        hipLaunchKernelGGL((head_sealed_kernel<8, 16>), dim3(head_form > 1 ? std::min(Npad / 32, head_form) : head_grid(Npad / 32)), dim3(512), 0, st, (const u32x4_t*)Ws,
                           (const u32x4_t*)Wp, (const u32x4_t*)Xp, KT, Npad / 32, out, Npad, n_valid);
    else
        hipLaunchKernelGGL((depth_sealed_kernel<8, 16, EPI_BF16>), dim3(Npad / 32, 1), dim3(512), 0, st, (const u32x4_t*)Ws,
                           (const u32x4_t*)Wp, (const u32x4_t*)Xp, KT, partial, out, Npad, n_valid);
    ++g_wseal_launches;
    mtts_gemm_depth_note();                  // a depth-specialised launch like its bf16 twin's (MTTS_GEMM_DEPTH=0 takes neither)
    return true;
}
