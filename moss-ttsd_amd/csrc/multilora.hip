// Per-dialogue LoRA adapters, unmerged: the low-rank path as one more split-K slab.
//
// Every GEMM whose output an adapter changes and whose consumer is linear (q|k|v, o_proj, down_proj) leaves fp32 slabs
// [ksplit][MTTS_PFCAP][Npad] that the consumer sums in ascending order with a run-time ksplit.  lora_delta_kernel writes
// slab number `ksplit`: for the row's adapter (RowMeta.seq -> seq_adapter[seq] -> bank entry of this matrix)
//
//     t[j]    = sum over k of A[j][k] * x[k]          lane l of a wave takes k = 256 i + 4 l + c (i ascending, then c = 0..3)
//                                                     into one sum, one multiply and one add per term; the 64 lane sums go
//                                                     through the wave-sum tree (common.h: wave_sum, xor 32, 16, 8, 4, 2, 1)
//     y[n]    = (sum over j ascending of B[n][j] * t[j]) * scaling
//
// all fp32, every multiply and add one IEEE operation (no fma): mtts/adapters.py: delta_spec states it in numpy and the
// tests compare bit for bit.  A function of (x, A, B, scaling) alone: not of the rows of the pass, the grid, or decode
// against prefill.  A row without an adapter, an adapter without this matrix and the padding columns get +0.0f, so the
// consumer's sum of a base row is the one it had (s + 0 = s).
//
// gate/up ends in SwiGLU, which is not linear: in a pass that carries adapters its GEMM writes slab 0, the delta slab 1,
// and swiglu_slabs_kernel applies the epilogue of gemm.hip (EPI_SILU) to their sum.
//
// x is the packed activation the GEMM reads (xpack_off); a block stages its row as fp32 in LDS (K * 4 bytes), computes
// the t of every matrix its columns touch (four waves, four ranks per wave at a time, 16-byte loads of A), and then one
// column per thread.  The adapter matrices are read from L2 / MALL: 32 rows of one adapter re-read the same A and B.
#include "launch.h"

#define LD_COLS 1024      // columns of the slab per block

// the matrix column n belongs to, and its row in that matrix (-1: none)
__device__ __forceinline__ int lora_seg_of(const LoraJob& job, int n, int* row) {
    for (int s = 0; s < job.nseg; ++s) {
        const int d = n - job.seg[s].col0;
        if (d >= 0 && d % job.seg[s].mul == 0 && d / job.seg[s].mul < job.seg[s].ncols) { *row = d / job.seg[s].mul; return s; }
    }
    return -1;
}

// grid = (R, ceil(Npad / LD_COLS)), block 256, dynamic LDS K * 4 bytes.  `ents`: the bank at this layer, entry
// [adapter * job.ent_stride + seg.proj]; `slab`: slab [MTTS_PFCAP][Npad] to write.
__global__ __launch_bounds__(256) void lora_delta_kernel(const uint16_t* __restrict__ xp, const RowMeta* __restrict__ meta,
                                                         const int32_t* __restrict__ seq_adapter, const LoraEnt* __restrict__ ents,
                                                         LoraJob job, float* __restrict__ slab) {
    extern __shared__ __attribute__((aligned(16))) float xs[];          // the row, fp32
    __shared__ float ts[LORA_SEGS][MTTS_LORA_MAX_RANK];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int row = blockIdx.x, K = job.K, Npad = job.Npad;
    const int c0 = blockIdx.y * LD_COLS, c1 = min(c0 + LD_COLS, Npad);
    float* out = slab + (size_t)row * Npad;
    const int seq = meta[row].seq;
    const int ad = seq >= 0 ? seq_adapter[seq] : -1;
    // the matrices of this adapter that have columns in [c0, c1)
    LoraEnt ent[LORA_SEGS];
    bool any = false;
#pragma unroll
    for (int s = 0; s < LORA_SEGS; ++s) {
        ent[s] = LoraEnt{nullptr, nullptr, 0, 0.f};
        if (ad >= 0 && s < job.nseg) {
            const LoraSeg g = job.seg[s];
            const int first = g.col0 + (c0 > g.col0 ? (c0 - g.col0 + g.mul - 1) / g.mul * g.mul : 0);
            if (first < c1 && first <= g.col0 + (g.ncols - 1) * g.mul) ent[s] = ents[(size_t)ad * job.ent_stride + g.proj];
        }
        any |= ent[s].r > 0;
    }
    if (!any) {                                                     // (block-uniform)
        for (int n = c0 + tid; n < c1; n += 256) out[n] = 0.f;
        return;
    }
    for (int g = tid; g < (K >> 3); g += 256) {
        const u32x4_t v = *(const u32x4_t*)(xp + xpack_off(row, g * 8, K));
        *(f32x4_t*)&xs[g * 8] = f32x4_t{bflo(v.x), bfhi(v.x), bflo(v.y), bfhi(v.y)};
        *(f32x4_t*)&xs[g * 8 + 4] = f32x4_t{bflo(v.z), bfhi(v.z), bflo(v.w), bfhi(v.w)};
    }
    __syncthreads();
#pragma unroll
    for (int s = 0; s < LORA_SEGS; ++s) {
        const int r = ent[s].r;
        for (int j0 = wave * 4; j0 < r; j0 += 16) {                 // ranks j0 .. j0 + 3 of this wave, their loads interleaved
            const float* a[4];
            float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int u = 0; u < 4; ++u) a[u] = ent[s].A + (size_t)min(j0 + u, r - 1) * K;
            for (int k = 4 * lane; k < K; k += 256) {               // K % 4 == 0: k + 3 < K
                const f32x4_t xv = *(const f32x4_t*)&xs[k];
                f32x4_t av[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) av[u] = *(const f32x4_t*)(a[u] + k);
#pragma unroll
                for (int c = 0; c < 4; ++c)
#pragma unroll
                    for (int u = 0; u < 4; ++u) acc[u] = lora_add(acc[u], lora_mul(av[u][c], xv[c]));
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const float t = wave_sum(acc[u]);
                if (lane == 0 && j0 + u < r) ts[s][j0 + u] = t;
            }
        }
    }
    __syncthreads();
    for (int n = c0 + tid; n < c1; n += 256) {
        int brow = 0;
        const int s = lora_seg_of(job, n, &brow);
        float y = 0.f;
        if (s >= 0) {
            // (a select over the unrolled array keeps ent[] in registers)
            LoraEnt en = ent[0];
#pragma unroll
            for (int q = 1; q < LORA_SEGS; ++q) if (s == q) en = ent[q];
            if (en.r > 0) {
                const float* b = en.B + (size_t)brow * en.r;
                float acc = 0.f;
                for (int j = 0; j < en.r; ++j) acc = lora_add(acc, lora_mul(b[j], ts[s][j]));
                y = lora_mul(acc, en.scaling);
            }
        }
        out[n] = y;
    }
}

// SwiGLU on the sum of two gate/up slabs [MTTS_PFCAP][2 I] (columns interleaved gate, up, gate, up: the packed weight's
// rows), with the rounding points of the fused epilogue (gemm.hip: EPI_SILU): gate, up -> bf16; silu(gate) -> bf16;
// product -> bf16, written in the packed layout down_proj reads.  grid = (R, ceil(I / 2048)), block 256: 8 outputs
// (one 16-byte group of the packed row) per thread.
__global__ __launch_bounds__(256) void swiglu_slabs_kernel(const float* __restrict__ slab0, const float* __restrict__ slab1,
                                                           uint16_t* __restrict__ act, int I) {
    const int row = blockIdx.x, i0 = (blockIdx.y * 256 + threadIdx.x) * 8;
    if (i0 >= I) return;
    const size_t at = (size_t)row * 2 * I + 2 * i0;
    float o[8];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const f32x4_t a = *(const f32x4_t*)(slab0 + at + 4 * q), d = *(const f32x4_t*)(slab1 + at + 4 * q);
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            float g = rbf(a[2 * j] + d[2 * j]), u = rbf(a[2 * j + 1] + d[2 * j + 1]);
            float s = rbf(g / (1.0f + expf(-g)));
            o[2 * q + j] = s * u;
        }
    }
    *(u32x4_t*)(act + xpack_off(row, i0, I)) = u32x4_t{pack2(o[0], o[1]), pack2(o[2], o[3]), pack2(o[4], o[5]), pack2(o[6], o[7])};
}

void launch_lora_delta(const void* xp, const RowMeta* meta, const int32_t* seq_adapter, const LoraEnt* ents, const LoraJob& job,
                       float* slab, int R, hipStream_t st) {
    const dim3 grid(R, (job.Npad + LD_COLS - 1) / LD_COLS);
    hipLaunchKernelGGL(lora_delta_kernel, grid, dim3(256), (size_t)job.K * 4, st, (const uint16_t*)xp, meta,
                       seq_adapter, ents, job, slab);
}

void launch_swiglu_slabs(const float* slab0, const float* slab1, void* act_packed, int R, int I, hipStream_t st) {
    hipLaunchKernelGGL(swiglu_slabs_kernel, dim3(R, (I + 2047) / 2048), dim3(256), 0, st, slab0, slab1, (uint16_t*)act_packed, I);
}
