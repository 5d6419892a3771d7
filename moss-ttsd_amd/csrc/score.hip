// Teacher-forced scoring: log-probability of a given label under every head, at every row of a prefill pass.
//
// Replaces the labels branch of AsteroidTTSInstruct.forward (reference modeling_asteroid.py:382-410): per channel
// `logits = lm_heads[i](hidden_states)` (a bf16 tensor [rows, V_c]) and ForCausalLMLoss, which upcasts the logits to
// fp32 and takes cross_entropy = -log_softmax(logits)[label].  In training the reference gets the same number from Liger's
// fused linear cross-entropy without the logits tensor; this is its forward half: at 2048 rows the channel-0 logits
// would be 625 MB in bf16 and are never written.
//
// head_ce_kernel   the main loop of gemm_tile_kernel (common.h: tile_mainloop) over the head weights as the engine holds them; the
//                  epilogue keeps, per row and 128-column block, (max m, sum exp(l - m), the label's logit).
// ce_finish_kernel merges a row's blocks and writes logp = l_label - (m + log s).
// ce_rows_f32_kernel  the fp32 / fp16 engines: the same formula on a materialised chunk of fp32 logits.
//
// Rounding points: the fp32 accumulator (k ascending, one accumulator: no split-K, so a logit is the same number whatever
// the launch) -> bf16 (the lm_head output dtype) -> fp32; everything after is fp32.  A row's result is a function of the
// row and the head shape alone: the column partition depends on the vocabulary only, every merge has a fixed order, and
// there are no atomics.
#include <math.h>

#include "launch.h"

// weight of a partial (max m, sum s) inside a merged maximum M: exp(m - M), 0 for an empty partial (m = -inf, whatever M)
__device__ __forceinline__ float ce_scale(float m, float M) { return m == -INFINITY ? 0.f : expf(m - M); }

// grid = (segments * blocks_per_seg, ceil(rtiles / 4)); block = 256 (2 x 2 waves, 64 rows x 64 columns each).
// Wp: `segments` heads one after another, each tiles_per_seg 32-row tiles (head0: 1 segment; heads17: 7 of Vs_pad rows),
// columns >= n_valid of a head are padding.  labels[row * lab_stride + lab_off + seg] (< 0: none), rows < rtiles * 32.
// part[row][blockIdx.x] = (m, s, l_label or -inf, 0).
__global__ __launch_bounds__(256) void head_ce_kernel(
    const u32x4_t* __restrict__ Wp, const u32x4_t* __restrict__ Xp, int KT, int tiles_per_seg, int blocks_per_seg, int n_valid,
    int rtiles, const int32_t* __restrict__ labels, int lab_stride, int lab_off, float4* __restrict__ part) {
    __shared__ float4 red[2][2][32];                       // [row half of the block][row tile][row]: the odd waves' partials
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int seg = blockIdx.x / blocks_per_seg, cb = blockIdx.x - seg * blocks_per_seg;
    const int nt0 = cb * 4 + (wave & 1) * 2;               // first of this wave's two 32-column tiles, inside its head
    const int rt0 = blockIdx.y * 4 + (wave >> 1) * 2;      // first of its two 32-row tiles
    const bool live = nt0 < tiles_per_seg && rt0 < rtiles; // (a dead wave still meets the barrier, with an empty partial)
    const bool n1 = nt0 + 1 < tiles_per_seg, r1 = rt0 + 1 < rtiles;
    f32x16_t acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[a][b][i] = 0.f;
    if (live) {
        const size_t xtile = (size_t)KT * 64;
        const int gt0 = seg * tiles_per_seg + nt0;
        const u32x4_t* w0 = Wp + (size_t)gt0 * KT * 64 + lane;
        const u32x4_t* w1 = Wp + (size_t)(n1 ? gt0 + 1 : gt0) * KT * 64 + lane;
        const u32x4_t* x0 = Xp + (size_t)rt0 * xtile + lane;
        const u32x4_t* x1 = Xp + (size_t)(r1 ? rt0 + 1 : rt0) * xtile + lane;
        tile_mainloop(acc, w0, w1, x0, x1, KT);
    }
    // D[n][row]: the lane holds row = lane & 31 of row tile b and, of column tile a, n = (i & 3) + 8 * (i >> 2) + 4 * (lane >> 5):
    // 32 of the row's 128 columns; lane ^ 32 holds the other 32 of this wave's 64, the wave next to it (wave ^ 1) the rest.
    float pm[2], ps[2], pl[2];
#pragma unroll
    for (int b = 0; b < 2; ++b) {
        const bool rowlive = live && (b == 0 || r1);
        const int row = (rt0 + b) * 32 + (lane & 31);
        const int lab = rowlive ? labels[(size_t)row * lab_stride + lab_off + seg] : -1;
        float m = -INFINITY, l = -INFINITY;
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int col = (nt0 + a) * 32 + (i & 3) + 8 * (i >> 2) + 4 * (lane >> 5);
                const bool ok = rowlive && (a == 0 || n1) && col < n_valid;
                const float v = ok ? rbf(acc[a][b][i]) : -INFINITY;       // bf16 logit, widened; padding drops out
                acc[a][b][i] = v;
                m = fmaxf(m, v);
                if (col == lab) l = v;
            }
        const float mm = m == -INFINITY ? 0.f : m;                        // (all columns dropped: every term is exp(-inf) = 0)
        float s = 0.f;
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int i = 0; i < 16; ++i) s += expf(acc[a][b][i] - mm);
        const float M = max_xor32(m);
        s = add_xor32(s * ce_scale(m, M));
        pm[b] = M; ps[b] = s; pl[b] = max_xor32(l);
        if ((wave & 1) && lane < 32) red[wave >> 1][b][lane] = make_float4(pm[b], ps[b], pl[b], 0.f);
    }
    __syncthreads();
    if ((wave & 1) || lane >= 32 || !live) return;
    // the two waves of a row, lower columns first
#pragma unroll
    for (int b = 0; b < 2; ++b) {
        if (b && !r1) break;
        const float4 o = red[wave >> 1][b][lane];
        const float M = fmaxf(pm[b], o.x);
        const float s = ps[b] * ce_scale(pm[b], M) + o.y * ce_scale(o.x, M);
        const int row = (rt0 + b) * 32 + lane;
        part[(size_t)row * gridDim.x + blockIdx.x] = make_float4(M, s, fmaxf(pl[b], o.z), 0.f);
    }
}

// One wave per (row, head): lane j takes the head's column blocks j, j + 64, ... in ascending order, the 64 lane sums
// go through wave_sum's fixed tree.  The maximum and the label's logit (held by exactly one block) do not depend on an
// order.  grid = (rows, segments), block = 64.  logp[row * out_stride + out_off + seg]; NaN where the label is < 0.
__global__ __launch_bounds__(64) void ce_finish_kernel(const float4* __restrict__ part, int ncb, int blocks_per_seg,
                                                       const int32_t* __restrict__ labels, int lab_stride, int lab_off,
                                                       float* __restrict__ logp, int out_stride, int out_off) {
    const int row = blockIdx.x, seg = blockIdx.y, lane = threadIdx.x;
    float* out = logp + (size_t)row * out_stride + out_off + seg;
    if (labels[(size_t)row * lab_stride + lab_off + seg] < 0) {
        if (lane == 0) *out = __uint_as_float(0x7fc00000u);
        return;
    }
    const float4* p = part + (size_t)row * ncb + (size_t)seg * blocks_per_seg;
    float m = -INFINITY, l = -INFINITY;
    for (int i = lane; i < blocks_per_seg; i += 64) {
        const float4 t = p[i];
        m = fmaxf(m, t.x);
        l = fmaxf(l, t.z);
    }
    const float M = wave_max(m), L = wave_max(l);
    float s = 0.f;
    for (int i = lane; i < blocks_per_seg; i += 64) {
        const float4 t = p[i];
        s += t.y * expf(t.x - M);                          // (every block holds a valid column: t.x is finite)
    }
    const float S = wave_sum(s);
    if (lane == 0) *out = L - (M + logf(S));
}

// fp32 / fp16 engines: row r of `logits` [R][ldy] fp32 (n_valid columns; an fp16 engine's are fp16 values) -> the same
// formula.  Thread t sums columns t, t + 256, ... in ascending order; wave_sum, then the four waves in order.
// grid = R, block = 256.
__global__ __launch_bounds__(256) void ce_rows_f32_kernel(const float* __restrict__ logits, long ldy, int n_valid,
                                                          const int32_t* __restrict__ labels, int lab_stride, int lab_off,
                                                          float* __restrict__ logp, int out_stride, int out_off) {
    __shared__ float sh[4];
    const int row = blockIdx.x;
    float* out = logp + (size_t)row * out_stride + out_off;
    const int lab = labels[(size_t)row * lab_stride + lab_off];
    if (lab < 0) {
        if (threadIdx.x == 0) *out = __uint_as_float(0x7fc00000u);
        return;
    }
    const float* p = logits + (size_t)row * ldy;
    float m = -INFINITY;
    for (int i = threadIdx.x; i < n_valid; i += 256) m = fmaxf(m, p[i]);
    m = wave_max(m);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = m;
    __syncthreads();
    const float M = fmaxf(fmaxf(sh[0], sh[1]), fmaxf(sh[2], sh[3]));
    __syncthreads();
    float s = 0.f;
    for (int i = threadIdx.x; i < n_valid; i += 256) s += expf(p[i] - M);
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) *out = p[lab] - (M + logf(sh[0] + sh[1] + sh[2] + sh[3]));
}

size_t head_ce_part_elems(int rows, int n_valid, int segments) {
    return (size_t)round_up32(rows) * segments * head_ce_blocks(n_valid) * 4;
}

void launch_head_ce(const void* Wp, const void* Xp, int R, int K, int n_valid, int segments, const int32_t* labels, int lab_stride,
                    int lab_off, float* part, float* logp, int out_stride, int out_off, hipStream_t st) {
    const int KT = K / 16, tiles = (n_valid + 31) / 32, bps = head_ce_blocks(n_valid), rtiles = (R + 31) / 32;
    hipLaunchKernelGGL(head_ce_kernel, dim3(segments * bps, (rtiles + 3) / 4), dim3(256), 0, st, (const u32x4_t*)Wp,
                       (const u32x4_t*)Xp, KT, tiles, bps, n_valid, rtiles, labels, lab_stride, lab_off, (float4*)part);
    hipLaunchKernelGGL(ce_finish_kernel, dim3(R, segments), dim3(64), 0, st, (const float4*)part, segments * bps, bps, labels,
                       lab_stride, lab_off, logp, out_stride, out_off);
}

void launch_ce_rows_f32(const float* logits, long ldy, int R, int n_valid, const int32_t* labels, int lab_stride, int lab_off,
                        float* logp, int out_stride, int out_off, hipStream_t st) {
    hipLaunchKernelGGL(ce_rows_f32_kernel, dim3(R), dim3(256), 0, st, logits, ldy, n_valid, labels, lab_stride, lab_off, logp,
                       out_stride, out_off);
}
