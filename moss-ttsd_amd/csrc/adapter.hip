// LoRA adapters merged into the engine's weights on the device (PEFT's merge_and_unload, per matrix):
//
//     acc = 0;  for j = 0 .. r-1 ascending:  acc = acc + B[n][j] * A[j][k]        (one IEEE multiply, one IEEE add: no fma)
//     merged[n][k] = round_model_dtype(W[n][k] + acc * scaling)
//
// with A = lora_A.weight [r][cols] and B = lora_B.weight [rows][r] in fp32.  (B A) * scaling in fp32 and one rounding of
// the fp32 sum is what PEFT computes for fp32 adapter weights on a half-precision base; the ascending order of the r-term
// sum is this project's choice, which makes the result a function of the inputs alone (mtts/adapters.py: merge_spec).
//
// lora_pack_kernel is pack_weight_kernel (gemm.hip) with the merge in front of the store: the base matrix is read once
// and the merged matrix is written once, straight into fragment order.  A block takes 32 source rows x 128 columns and
// walks r in chunks of 32: the chunk's B rows and A columns are staged in LDS, a thread keeps 2 x 8 sums (two 16-byte
// groups of one row) in registers.  lora_rows_f32_kernel does the same into the row-major fp32 copies of the fp32 / fp16
// engines.  Plain fp32 VALU: at r = 16 the merge is ~32 operations per weight, below the time the bytes take.
#include <hip/hip_fp16.h>

#include "launch.h"

#define LORA_JC 32        // adapter ranks staged per pass
#define LORA_KB 128       // columns per block: 8 k-tiles, two per wave
#define LORA_G 2          // 16-byte groups (8 columns) per thread

// The two operations of the definition: lora_mul / lora_add (common.h), one IEEE multiply and one IEEE add, never an fma
// (tests/test_adapter_isa_cpu.py).
// W + acc * scaling, rounded to the model dtype and held as fp32: mode 0 bf16, 1 fp32, 2 fp16 (MTTS_DTYPE_*; f32path.hip: r16)
__device__ __forceinline__ float lora_merge(float w, float acc, float scaling) { return lora_add(w, lora_mul(acc, scaling)); }
__device__ __forceinline__ float lora_round_f16(float v) { return __half2float(__float2half_rn(v)); }

// acc[g][i] = sum over j of B[row][j] * A[j][k(g) + i] for this thread's row (srow0 + tid % 32) and its LORA_G groups of 8
// columns, k(g) = k0 + (2 * wave + g) * 16 + 8 * ((tid / 32) & 1): the group a lane of the packed layout holds.
__device__ __forceinline__ void lora_block_acc(float (&acc)[LORA_G][8], const float* __restrict__ A, const float* __restrict__ B,
                                               int r, int rows, int cols, int srow0, int k0) {
    __shared__ __attribute__((aligned(16))) float sA[LORA_JC][LORA_KB];
    __shared__ float sB[32][LORA_JC + 1];                 // + 1: the 32 rows of a half wave fall on 32 banks
    const int tid = threadIdx.x, sr = tid & 31, kh = (tid >> 5) & 1, wv = tid >> 6;
#pragma unroll
    for (int g = 0; g < LORA_G; ++g)
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[g][i] = 0.f;
    for (int j0 = 0; j0 < r; j0 += LORA_JC) {
        const int jn = min(LORA_JC, r - j0);
        __syncthreads();                                  // the previous chunk has been read
        for (int idx = tid; idx < jn * (LORA_KB / 4); idx += 256) {
            const int jj = idx / (LORA_KB / 4), c = (idx % (LORA_KB / 4)) * 4, k = k0 + c;
            f32x4_t v = {0.f, 0.f, 0.f, 0.f};
            if (k < cols) v = *(const f32x4_t*)(A + (size_t)(j0 + jj) * cols + k);      // cols % 16 == 0: k + 3 < cols
            *(f32x4_t*)&sA[jj][c] = v;
        }
        for (int idx = tid; idx < 32 * LORA_JC; idx += 256) {
            const int rr = idx / LORA_JC, jj = idx % LORA_JC, srow = srow0 + rr;
            sB[rr][jj] = (srow < rows && jj < jn) ? B[(size_t)srow * r + j0 + jj] : 0.f;
        }
        __syncthreads();
#pragma unroll 4
        for (int jj = 0; jj < jn; ++jj) {
            const float b = sB[sr][jj];
#pragma unroll
            for (int g = 0; g < LORA_G; ++g) {
                const float* a = &sA[jj][(wv * LORA_G + g) * 16 + kh * 8];
                const f32x4_t a0 = *(const f32x4_t*)a, a1 = *(const f32x4_t*)(a + 4);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    acc[g][i] = lora_add(acc[g][i], lora_mul(b, a0[i]));
                    acc[g][4 + i] = lora_add(acc[g][4 + i], lora_mul(b, a1[i]));
                }
            }
        }
    }
}

// Source row s of the bf16 matrix `base` [rows][cols], merged, lands on packed row s * row_mul + row_off of `dst`
// (rows_pad rows in fragment order): pack_weight_kernel's placement.  Only the 16-byte groups of its source rows are
// written.  Grid: (ceil(cols / 128), ceil(rows / 32)).
__global__ __launch_bounds__(256) void lora_pack_kernel(const uint16_t* __restrict__ base, const float* __restrict__ A,
                                                        const float* __restrict__ B, int r, float scaling,
                                                        uint16_t* __restrict__ dst, int rows, int cols, int row_mul, int row_off) {
    const int tid = threadIdx.x, sr = tid & 31, kh = (tid >> 5) & 1, wv = tid >> 6;
    const int k0 = blockIdx.x * LORA_KB, srow0 = blockIdx.y * 32, srow = srow0 + sr;
    u32x4_t w[LORA_G];
#pragma unroll
    for (int g = 0; g < LORA_G; ++g) {                    // the base is in flight while the sums are formed
        const int k = k0 + (wv * LORA_G + g) * 16 + kh * 8;
        w[g] = u32x4_t{0u, 0u, 0u, 0u};
        if (srow < rows && k < cols) w[g] = *(const u32x4_t*)(base + (size_t)srow * cols + k);
    }
    float acc[LORA_G][8];
    lora_block_acc(acc, A, B, r, rows, cols, srow0, k0);
    if (srow >= rows) return;
    const int p = srow * row_mul + row_off;
#pragma unroll
    for (int g = 0; g < LORA_G; ++g) {
        const int k = k0 + (wv * LORA_G + g) * 16 + kh * 8;
        if (k >= cols) continue;
        u32x4_t o;
#pragma unroll
        for (int i = 0; i < 4; ++i)
            o[i] = pack2(lora_merge(bflo(w[g][i]), acc[g][2 * i], scaling), lora_merge(bfhi(w[g][i]), acc[g][2 * i + 1], scaling));
        *(u32x4_t*)(dst + wpack_off(p, k, cols >> 4)) = o;
    }
}

// The fp32 / fp16 engines: base and dst fp32 row-major [rows][cols] (h16: fp32 holding fp16 values, rounded as such).
__global__ __launch_bounds__(256) void lora_rows_f32_kernel(const float* __restrict__ base, const float* __restrict__ A,
                                                            const float* __restrict__ B, int r, float scaling,
                                                            float* __restrict__ dst, int rows, int cols, int h16) {
    const int tid = threadIdx.x, sr = tid & 31, kh = (tid >> 5) & 1, wv = tid >> 6;
    const int k0 = blockIdx.x * LORA_KB, srow0 = blockIdx.y * 32, srow = srow0 + sr;
    float acc[LORA_G][8];
    lora_block_acc(acc, A, B, r, rows, cols, srow0, k0);
    if (srow >= rows) return;
#pragma unroll
    for (int g = 0; g < LORA_G; ++g) {
        const int k = k0 + (wv * LORA_G + g) * 16 + kh * 8;
        if (k >= cols) continue;
        const size_t at = (size_t)srow * cols + k;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const f32x4_t w = *(const f32x4_t*)(base + at + 4 * h);
            f32x4_t o;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float v = lora_merge(w[i], acc[g][4 * h + i], scaling);
                o[i] = h16 ? lora_round_f16(v) : v;
            }
            *(f32x4_t*)(dst + at + 4 * h) = o;
        }
    }
}

void launch_lora_pack(const void* base, const float* A, const float* B, int r, float scaling, void* dst, int rows, int cols,
                      int row_mul, int row_off, hipStream_t st) {
    const dim3 grid((cols + LORA_KB - 1) / LORA_KB, (rows + 31) / 32);
    hipLaunchKernelGGL(lora_pack_kernel, grid, dim3(256), 0, st, (const uint16_t*)base, A, B, r, scaling, (uint16_t*)dst, rows, cols,
                       row_mul, row_off);
}
void launch_lora_rows_f32(const float* base, const float* A, const float* B, int r, float scaling, float* dst, int rows, int cols,
                          int h16, hipStream_t st) {
    const dim3 grid((cols + LORA_KB - 1) / LORA_KB, (rows + 31) / 32);
    hipLaunchKernelGGL(lora_rows_f32_kernel, grid, dim3(256), 0, st, base, A, B, r, scaling, dst, rows, cols, h16);
}
