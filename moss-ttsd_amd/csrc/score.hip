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
// head_topk_kernel / topk_finish_kernel / topk_rows_f32_kernel  the k most probable tokens of every row next to it (below).
//
// Rounding points: the fp32 accumulator (k ascending, one accumulator: no split-K, so a logit is the same number whatever
// the launch) -> bf16 (the lm_head output dtype) -> fp32; everything after is fp32.  A row's result is a function of the
// row and the head shape alone: the column partition depends on the vocabulary only, every merge has a fixed order, and
// there are no atomics.
#include <math.h>

#include "launch.h"
#include "topk.h"

// weight of a partial (max m, sum s) inside a merged maximum M: exp(m - M), 0 for an empty partial (m = -inf, whatever M)
__device__ __forceinline__ float ce_scale(float m, float M) { return m == -INFINITY ? 0.f : expf(m - M); }

// ---- top-k: the order "descending logit, ties by ascending column" as an unsigned compare (topk.h: f32_sortable, the 64-bit
// pairs, wave_umax64, TopList) ----------------------------------------------------------------------------------------
// A bf16 logit (the low 16 bits of its fp32 form are zero) and its column inside a 128-column block in one word: the larger
// key is the better candidate, and 0 is below every key of a valid column.
__device__ __forceinline__ uint32_t topk_key16(float v, int off) { return (f32_sortable(v) & 0xffff0000u) | (uint32_t)(127 - off); }
// the logit of a key (or of its upper half): a negative value's 16 dropped bits were ones in the sortable form
__device__ __forceinline__ float topk_key16_value(uint32_t key) { return f32_unsortable(key & 0x80000000u ? key & 0xffff0000u : key | 0xffffu); }
__device__ __forceinline__ uint32_t umax_xor32(uint32_t v) {
    const u32x2s_t t = __builtin_amdgcn_permlane32_swap(v, v, false, false);
    return max(t.x, t.y);
}
// grid = (segments * blocks_per_seg, ceil(rtiles / 4)); block = 256 (2 x 2 waves, 64 rows x 64 columns each).
// Wp: `segments` heads one after another, each tiles_per_seg 32-row tiles (head0: 1 segment; heads17: 7 of Vs_pad rows),
// columns >= n_valid of a head are padding.  labels[row * lab_stride + lab_off + seg] (< 0: none), rows < rtiles * 32.
// part[row][blockIdx.x] = (m, s, l_label or -inf, 0).
//
// TOPK (head_topk_kernel): the same main loop, rounding and (m, s, l_label) partials, and after them the block's k best
// columns of every row, as keys (topk_key16) in descending order: cand[(row * gridDim.x + blockIdx.x) * k + j], 0 where
// the block has fewer than k valid columns.  A wave first selects the k best of its own 64 columns: k rounds of a max
// over the lane's 32 keys, one exchange with lane ^ 32, and the winner (a key names its column, so exactly one register
// of one lane equals it) zeroed in place.  The two sorted lists of a row then meet in LDS behind the one barrier the
// partials already need, and the even wave merges them.
template <bool TOPK>
__device__ __forceinline__ void head_ce_body(
    const u32x4_t* __restrict__ Wp, const u32x4_t* __restrict__ Xp, int KT, int tiles_per_seg, int blocks_per_seg, int n_valid,
    int rtiles, const int32_t* __restrict__ labels, int lab_stride, int lab_off, float4* __restrict__ part, int k,
    uint32_t* __restrict__ cand) {
    __shared__ float4 red[2][2][32];                       // [row half of the block][row tile][row]: the odd waves' partials
    // TOPK: [row half][column half: the wave][row tile][rank][row], the waves' sorted lists
    __shared__ uint32_t wkeys[2][2][2][TOPK ? MTTS_SCORE_MAX_TOPK : 1][32];
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
        // TOPK: n_valid made opaque per row tile, so that the 32 "column is valid" lane masks are computed again for the
        // second tile and not kept in 64 scalar registers across the selection loop (they spilled there)
        int nvl = n_valid;
        if constexpr (TOPK) asm volatile("" : "+s"(nvl));
        const int row = (rt0 + b) * 32 + (lane & 31);
        const int lab = rowlive ? labels[(size_t)row * lab_stride + lab_off + seg] : -1;
        float m = -INFINITY, l = -INFINITY;
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int col = (nt0 + a) * 32 + (i & 3) + 8 * (i >> 2) + 4 * (lane >> 5);
                const bool ok = rowlive && (a == 0 || n1) && col < nvl;
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
        if constexpr (TOPK) {
            // the columns the reduction above kept, as one bound on the column inside the block (not 32 lane masks held
            // across the sum): off < nv
            const int nv = rowlive ? min(n_valid - cb * 128, (wave & 1) * 64 + (n1 ? 64 : 32)) : 0;
            uint32_t key[32];
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const int off = (wave & 1) * 64 + a * 32 + (i & 3) + 8 * (i >> 2) + 4 * (lane >> 5);     // column inside the block
                    key[a * 16 + i] = off < nv ? topk_key16(acc[a][b][i], off) : 0u;
                }
            for (int j = 0; j < k; ++j) {
                uint32_t w = 0;
#pragma unroll
                for (int c = 0; c < 32; ++c) w = max(w, key[c]);
                w = umax_xor32(w);
#pragma unroll
                for (int c = 0; c < 32; ++c) key[c] = key[c] == w ? 0u : key[c];
                if (lane < 32) wkeys[wave >> 1][wave & 1][b][j][lane] = w;
            }
        }
    }
    __syncthreads();
    if constexpr (TOPK) {
        // lane -> (row tile lane >> 5, row lane & 31) of the even wave: the wave's list and its neighbour's, both descending
        const int b = lane >> 5, rl = lane & 31;
        if (!(wave & 1) && live && (b == 0 || r1)) {
            const int row = (rt0 + b) * 32 + rl;
            uint32_t* out = cand + ((size_t)row * gridDim.x + blockIdx.x) * k;
            int ia = 0, ib = 0;
            uint32_t ka = wkeys[wave >> 1][0][b][0][rl], kb = wkeys[wave >> 1][1][b][0][rl];
            for (int j = 0; j < k; ++j) {
                const bool lo = ka >= kb;                      // (equal only when both lists have run out: 0)
                out[j] = lo ? ka : kb;
                if (lo) ka = ++ia < k ? wkeys[wave >> 1][0][b][ia][rl] : 0u;
                else kb = ++ib < k ? wkeys[wave >> 1][1][b][ib][rl] : 0u;
            }
        }
    }
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

__global__ __launch_bounds__(256) void head_ce_kernel(
    const u32x4_t* __restrict__ Wp, const u32x4_t* __restrict__ Xp, int KT, int tiles_per_seg, int blocks_per_seg, int n_valid,
    int rtiles, const int32_t* __restrict__ labels, int lab_stride, int lab_off, float4* __restrict__ part) {
    head_ce_body<false>(Wp, Xp, KT, tiles_per_seg, blocks_per_seg, n_valid, rtiles, labels, lab_stride, lab_off, part, 0, nullptr);
}

// 1 <= k <= MTTS_SCORE_MAX_TOPK; cand uint32 [rtiles * 32][gridDim.x][k]
__global__ __launch_bounds__(256) void head_topk_kernel(
    const u32x4_t* __restrict__ Wp, const u32x4_t* __restrict__ Xp, int KT, int tiles_per_seg, int blocks_per_seg, int n_valid,
    int rtiles, const int32_t* __restrict__ labels, int lab_stride, int lab_off, float4* __restrict__ part, int k,
    uint32_t* __restrict__ cand) {
    head_ce_body<true>(Wp, Xp, KT, tiles_per_seg, blocks_per_seg, n_valid, rtiles, labels, lab_stride, lab_off, part, k, cand);
}

// A row's (M, S) -- and the label's logit L -- from the partials of its head's blocks.  One wave: lane j takes the column
// blocks j, j + 64, ... in ascending order, the 64 lane sums go through wave_sum's fixed tree.  The maximum and the
// label's logit (held by exactly one block) do not depend on an order.
__device__ __forceinline__ void ce_merge_blocks(const float4* __restrict__ p, int blocks_per_seg, int lane, float& M, float& S, float& L) {
    float m = -INFINITY, l = -INFINITY;
    for (int i = lane; i < blocks_per_seg; i += 64) {
        const float4 t = p[i];
        m = fmaxf(m, t.x);
        l = fmaxf(l, t.z);
    }
    M = wave_max(m);
    L = wave_max(l);
    float s = 0.f;
    for (int i = lane; i < blocks_per_seg; i += 64) {
        const float4 t = p[i];
        s += t.y * expf(t.x - M);                          // (every block holds a valid column: t.x is finite)
    }
    S = wave_sum(s);
}

// One wave per (row, head).  grid = (rows, segments), block = 64.  logp[row * out_stride + out_off + seg]; NaN where the
// label is < 0.
__global__ __launch_bounds__(64) void ce_finish_kernel(const float4* __restrict__ part, int ncb, int blocks_per_seg,
                                                       const int32_t* __restrict__ labels, int lab_stride, int lab_off,
                                                       float* __restrict__ logp, int out_stride, int out_off) {
    const int row = blockIdx.x, seg = blockIdx.y, lane = threadIdx.x;
    float* out = logp + (size_t)row * out_stride + out_off + seg;
    if (labels[(size_t)row * lab_stride + lab_off + seg] < 0) {
        if (lane == 0) *out = __uint_as_float(0x7fc00000u);
        return;
    }
    float M, S, L;
    ce_merge_blocks(part + (size_t)row * ncb + (size_t)seg * blocks_per_seg, blocks_per_seg, lane, M, S, L);
    if (lane == 0) *out = L - (M + logf(S));
}

// One wave per (row, head): the row's k best out of its blocks' candidates.  Lane j reads the blocks j, j + 64, ... and
// keeps its own KL >= k best pairs (a block's list is descending: it is left at the first key that does not enter);
// then k rounds of: the best head of the 64 lists, which its one owner pops.  The result is the k largest pairs of a
// total order, whatever the order they were met in.  The log-probability is ce_finish_kernel's expression on the
// candidate's logit.  ids / logp [(row * out_stride + out_off + seg) * k + j].  grid = (rows, segments), block = 64.
template <int KL>
__global__ __launch_bounds__(64) void topk_finish_kernel(const float4* __restrict__ part, const uint32_t* __restrict__ cand, int ncb,
                                                         int blocks_per_seg, int k, int32_t* __restrict__ ids,
                                                         float* __restrict__ logp, int out_stride, int out_off) {
    const int row = blockIdx.x, seg = blockIdx.y, lane = threadIdx.x;
    const uint32_t* c = cand + ((size_t)row * ncb + (size_t)seg * blocks_per_seg) * k;
    TopList<KL> top;
    top.clear();
    for (int i = lane; i < blocks_per_seg; i += 64)
        for (int j = 0; j < k; ++j) {
            const uint32_t key = c[(size_t)i * k + j];
            const uint64_t pr = topk_pair(key & 0xffff0000u, i * 128 + 127 - (int)(key & 127u));
            if (key == 0 || pr <= top.last()) break;
            top.insert(pr);
        }
    float M, S, L;
    ce_merge_blocks(part + (size_t)row * ncb + (size_t)seg * blocks_per_seg, blocks_per_seg, lane, M, S, L);
    const size_t o = ((size_t)row * out_stride + out_off + seg) * k;
    for (int j = 0; j < k; ++j) {
        const uint64_t best = wave_umax64(top.v[0]);
        top.pop_if(best != 0 && top.v[0] == best);
        if (lane == 0) {
            ids[o + j] = topk_pair_col(best);
            logp[o + j] = best ? topk_key16_value((uint32_t)(best >> 32)) - (M + logf(S)) : __uint_as_float(0x7fc00000u);
        }
    }
}

// fp32 / fp16 engines: row r of `logits` [R][ldy] fp32 (n_valid columns; an fp16 engine's are fp16 values) -> (M, the four
// waves' sums in sh).  Thread t sums columns t, t + 256, ... in ascending order; wave_sum, then the four waves in order.
__device__ __forceinline__ float ce_row_f32_max_sums(const float* __restrict__ p, int n_valid, float (&sh)[4]) {
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
    return M;
}

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
    const float M = ce_row_f32_max_sums(p, n_valid, sh);
    if (threadIdx.x == 0) *out = p[lab] - (M + logf(sh[0] + sh[1] + sh[2] + sh[3]));
}

// The same rows' k best columns: thread t keeps the KL >= k best pairs of its columns t, t + 256, ...; k rounds of the best
// head of the 256 lists (wave, then the four waves through LDS), popped by its owner.  The log-probability is
// ce_rows_f32_kernel's expression on the winner's logit.  ids / logp [(row * out_stride + out_off) * k + j].
// grid = R, block = 256.
template <int KL>
__global__ __launch_bounds__(256) void topk_rows_f32_kernel(const float* __restrict__ logits, long ldy, int n_valid, int k,
                                                            int32_t* __restrict__ ids, float* __restrict__ logp, int out_stride,
                                                            int out_off) {
    __shared__ float sh[4];
    __shared__ uint64_t best4[4];
    const int row = blockIdx.x;
    const float* p = logits + (size_t)row * ldy;
    TopList<KL> top;
    top.clear();
    for (int i = threadIdx.x; i < n_valid; i += 256) {
        const uint64_t pr = topk_pair(f32_sortable(p[i]), i);
        if (pr > top.last()) top.insert(pr);
    }
    const float M = ce_row_f32_max_sums(p, n_valid, sh);
    const size_t o = ((size_t)row * out_stride + out_off) * k;
    for (int j = 0; j < k; ++j) {
        const uint64_t w = wave_umax64(top.v[0]);
        if ((threadIdx.x & 63) == 0) best4[threadIdx.x >> 6] = w;
        __syncthreads();
        const uint64_t a = best4[0] > best4[1] ? best4[0] : best4[1], b = best4[2] > best4[3] ? best4[2] : best4[3];
        const uint64_t best = a > b ? a : b;
        __syncthreads();
        top.pop_if(best != 0 && top.v[0] == best);
        if (threadIdx.x == 0) {
            const int col = topk_pair_col(best);
            ids[o + j] = col;
            logp[o + j] = best ? p[col] - (M + logf(sh[0] + sh[1] + sh[2] + sh[3])) : __uint_as_float(0x7fc00000u);
        }
    }
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

size_t head_topk_cand_elems(int rows, int n_valid, int segments, int k) {
    return (size_t)std::min(round_up32(rows), MTTS_SCORE_TOPK_ROWS) * segments * head_ce_blocks(n_valid) * k;
}

void launch_head_topk(const void* Wp, const void* Xp, int R, int K, int n_valid, int segments, const int32_t* labels, int lab_stride,
                      int lab_off, float* part, float* logp, int out_stride, int out_off, int k, uint32_t* cand, int32_t* top_ids,
                      float* top_logp, hipStream_t st) {
    const int KT = K / 16, tiles = (n_valid + 31) / 32, bps = head_ce_blocks(n_valid), ncb = segments * bps;
    for (int r0 = 0; r0 < R; r0 += MTTS_SCORE_TOPK_ROWS) {
        const int n = std::min(MTTS_SCORE_TOPK_ROWS, R - r0), rtiles = (n + 31) / 32;
        float4* p = (float4*)part + (size_t)r0 * ncb;
        const int32_t* lab = labels + (size_t)r0 * lab_stride;
        hipLaunchKernelGGL(head_topk_kernel, dim3(ncb, (rtiles + 3) / 4), dim3(256), 0, st, (const u32x4_t*)Wp,
                           (const u32x4_t*)Xp + (size_t)(r0 / 32) * KT * 64, KT, tiles, bps, n_valid, rtiles, lab, lab_stride, lab_off, p,
                           k, cand);
        if (logp)
            hipLaunchKernelGGL(ce_finish_kernel, dim3(n, segments), dim3(64), 0, st, (const float4*)p, ncb, bps, lab, lab_stride, lab_off,
                               logp + (size_t)r0 * out_stride, out_stride, out_off);
#define TOPK_FINISH(KL)                                                                                                          \
    hipLaunchKernelGGL(topk_finish_kernel<KL>, dim3(n, segments), dim3(64), 0, st, (const float4*)p, (const uint32_t*)cand, ncb, bps, \
                       k, top_ids + (size_t)r0 * out_stride * k, top_logp + (size_t)r0 * out_stride * k, out_stride, out_off)
        TOPK_DISPATCH(k, TOPK_FINISH);
#undef TOPK_FINISH
    }
}

void launch_topk_rows_f32(const float* logits, long ldy, int R, int n_valid, int k, int32_t* top_ids, float* top_logp, int out_stride,
                          int out_off, hipStream_t st) {
#define TOPK_ROWS(KL) \
    hipLaunchKernelGGL(topk_rows_f32_kernel<KL>, dim3(R), dim3(256), 0, st, logits, ldy, n_valid, k, top_ids, top_logp, out_stride, out_off)
    TOPK_DISPATCH(k, TOPK_ROWS);
#undef TOPK_ROWS
}

