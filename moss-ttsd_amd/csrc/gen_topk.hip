// generate(top_logprobs=k): the model's own distribution at the steps it sampled.
//
// The reference returns a step's logits rows under return_dict_in_generate=True, output_logits=True
// (modeling_asteroid.py:78,123-128,174-175: `next_token_logits` with the two hard-coded masks, before any processor).
// 8 x [B, V_c] per step are not kept here; this is their reduced form, per (row, channel) of a decode step:
//   logp       = log_softmax(L)[d], d = the sampler's raw decision (decisions[row][c]),
//   ids / tlp  = the first k tokens of L under (descending logit, ascending id; -0 = +0) and their log_softmax(L),
// L = the fp32 view of the logits row the step's forward wrote, masked id at -inf.  The kernels run between the sampler
// and update_kernel, while the row is still in L2, and write the step's row of the per-slot result buffers; update_kernel
// then puts NaN / -1 over the slots that are not model decisions, by the rule it applies to lp.
//
// gen_topk_slice_kernel   vocabulary > SAMP_CAND (channel 0): grid (SAMP_NS, rows), the slices of sample_scan_kernel.
//                         A slice leaves its k best pairs, its max m and sum exp(l - m).
// gen_topk_finish_kernel  grid (channels, rows): merges a row's slices in slice order, or (<= SAMP_CAND columns:
//                         channels 1..7) scans the row itself; writes logp, ids, tlp.
//
// Sums: a thread adds at most 19 terms in fp32 (ceil(152 697 / 32 / 256); 16 for a row one block scans); the 256 thread
// sums meet in fp64 through a fixed tree (lanes by xor 32..1, then the four waves in order), the 32 slice sums in fp64
// in slice order.  No atomics: a value is a function of the logits row and the decision alone.  Both outputs are the one
// expression (float)((double)l - (M + log S)), so tlp[j] is bit for bit the logp of a decision ids[j].
#include <math.h>

#include "launch.h"
#include "sample_ctx.h"
#include "topk.h"

#define GT_T 256

struct GenRow {
    LogitsPtr lg;
    int V, mask_id;
    int dec;               // index of the (row, channel) pair in `decisions`: row * 8 + channel in the engine, row on the per-kernel entry
    long out;              // result slot: (slot * gen_cap + the dialogue's step) * 8 + channel in the engine (the layout of the
                           // generated tokens), row on the per-kernel entry; < 0: the slot's storage is full, nothing is written
};

// single_vocab > 0: one logits matrix [rows][vocab] (the per-kernel entry); else the engine's row context (sample_ctx)
__device__ __forceinline__ bool gen_row(GenRow& r, int b, int c_in, const void* logits0, const void* logits17, int V0, int Vs,
                                        int Vs_pad, const MttsSamplerCfg* cfgs, const LoopState* ls, const SeqState* seqs,
                                        int single_vocab, int single_mask, int single_f32) {
    if (single_vocab > 0) {
        r.lg = LogitsPtr{(const char*)logits0 + (size_t)b * single_vocab * (single_f32 ? 4 : 2), single_f32};
        r.V = single_vocab; r.mask_id = single_mask; r.dec = b; r.out = b;
        return true;
    }
    SampleCtx x;
    if (!sample_ctx(x, b, c_in, (const uint16_t*)logits0, (const uint16_t*)logits17, V0, Vs, Vs_pad, nullptr, 0, cfgs, ls, seqs,
                    0, 0, 0, 0)) return false;
    r.lg = x.lg; r.V = x.V; r.mask_id = x.mask_id; r.dec = b * 8 + x.c;
    r.out = x.step < ls->gen_cap ? ((long)b * ls->gen_cap + x.step) * 8 + x.c : -1;      // (update_kernel retires such a row)
    return true;
}

// L[i]: the raw logit, widened; the masked id at -inf (modeling_asteroid.py:124-128)
__device__ __forceinline__ float raw_logit(LogitsPtr lg, int i, int mask_id) {
    if (i == mask_id) return -INFINITY;
    return lg.f32 ? ((const float*)lg.p)[i] : bf2f(((const uint16_t*)lg.p)[i]);
}

// sum of one double per thread over the block, in every thread: a fixed tree, whatever the launch
__device__ __forceinline__ double block_sum_f64(double v, double* shd) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) shd[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((shd[0] + shd[1]) + shd[2]) + shd[3];
}

// Columns [i0, i1) of the row, thread t taking i0 + t, i0 + t + 256, ...: its KL best pairs, the block's max M
// (-inf: no finite logit) and S = sum exp(l - M), both in every thread.
template <int KL>
__device__ __forceinline__ void scan_cols(const GenRow& r, int i0, int i1, TopList<KL>& top, float& M, double& S, float* shf,
                                          double* shd) {
    top.clear();
    float tm = -INFINITY;
    for (int i = i0 + (int)threadIdx.x; i < i1; i += GT_T) {
        const float v = raw_logit(r.lg, i, r.mask_id);
        tm = fmaxf(tm, v);
        const uint64_t pr = topk_pair(f32_sortable(v), i);
        if (pr > top.last()) top.insert(pr);
    }
    tm = wave_max(tm);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) shf[threadIdx.x >> 6] = tm;
    __syncthreads();
    M = fmaxf(fmaxf(shf[0], shf[1]), fmaxf(shf[2], shf[3]));
    // second pass over the columns (L2 resident): the thread's terms in fp32, ascending column
    float loc = 0.f;
    if (M > -INFINITY)
        for (int i = i0 + (int)threadIdx.x; i < i1; i += GT_T) loc += expf(raw_logit(r.lg, i, r.mask_id) - M);
    S = block_sum_f64((double)loc, shd);
}

// The best head of the block's 256 lists, popped by its one owner (a pair names its column); 0 when all are empty.
template <int KL>
__device__ __forceinline__ uint64_t block_pop_best(TopList<KL>& top, uint64_t* best4) {
    const uint64_t w = wave_umax64(top.v[0]);
    if ((threadIdx.x & 63) == 0) best4[threadIdx.x >> 6] = w;
    __syncthreads();
    const uint64_t a = best4[0] > best4[1] ? best4[0] : best4[1], b = best4[2] > best4[3] ? best4[2] : best4[3];
    const uint64_t best = a > b ? a : b;
    __syncthreads();
    top.pop_if(best != 0 && top.v[0] == best);
    return best;
}

// grid = (SAMP_NS, rows), block = GT_T.  1 <= k <= KL.
template <int KL>
__global__ __launch_bounds__(GT_T) void gen_topk_slice_kernel(
    const void* __restrict__ logits0, int V0, const MttsSamplerCfg* __restrict__ cfgs, const LoopState* __restrict__ ls,
    const SeqState* __restrict__ seqs, int k, GenTopkScratch sc, int single_vocab, int single_mask, int single_f32) {
    __shared__ float shf[GT_T / 64];
    __shared__ double shd[GT_T / 64];
    __shared__ uint64_t best4[GT_T / 64];
    const int b = blockIdx.y, slice = blockIdx.x;
    GenRow r;
    if (!gen_row(r, b, 0, logits0, nullptr, V0, 0, 0, cfgs, ls, seqs, single_vocab, single_mask, single_f32)) return;
    const int per = (r.V + SAMP_NS - 1) / SAMP_NS;
    const int i0 = min(r.V, slice * per), i1 = min(r.V, i0 + per);
    TopList<KL> top;
    float M;
    double S;
    scan_cols<KL>(r, i0, i1, top, M, S, shf, shd);
    const size_t o = (size_t)b * SAMP_NS + slice;
    if (threadIdx.x == 0) { sc.smax[o] = M; sc.ssum[o] = S; }
    for (int j = 0; j < k; ++j) {
        const uint64_t best = block_pop_best<KL>(top, best4);
        if (threadIdx.x == 0) sc.cand[o * k + j] = best;
    }
}

// grid = (channels, rows), block = GT_T.  out.logp[r.out], out.ids / out.tlp[r.out * k + j]: in the engine the step's row of
// the per-slot buffers themselves -- update_kernel, which runs next, puts NaN / -1 over the slots that are not decisions.
template <int KL>
__global__ __launch_bounds__(GT_T) void gen_topk_finish_kernel(
    const void* __restrict__ logits0, const void* __restrict__ logits17, int V0, int Vs, int Vs_pad,
    const MttsSamplerCfg* __restrict__ cfgs, const LoopState* __restrict__ ls, const SeqState* __restrict__ seqs,
    const int32_t* __restrict__ decisions, int k, GenTopkScratch sc, GenTopkOut out, int single_vocab, int single_mask,
    int single_f32) {
    __shared__ float shf[GT_T / 64];
    __shared__ double shd[GT_T / 64];
    __shared__ uint64_t best4[GT_T / 64];
    __shared__ double term[SAMP_NS];
    const int b = blockIdx.y, tid = threadIdx.x;
    GenRow r;
    if (!gen_row(r, b, blockIdx.x, logits0, logits17, V0, Vs, Vs_pad, cfgs, ls, seqs, single_vocab, single_mask, single_f32)) return;
    if (r.out < 0) return;
    TopList<KL> top;
    float M;
    double S = 0.0;
    if (r.V > SAMP_CAND) {
        // the row's slices: thread j < SAMP_NS holds slice j's list (already descending) and rescales its sum to the row's
        // maximum; thread 0 adds the 32 terms in slice order
        const size_t o = (size_t)b * SAMP_NS;
        top.clear();
        float m = -INFINITY;
        if (tid < SAMP_NS) {
            m = sc.smax[o + tid];
#pragma unroll
            for (int j = 0; j < KL; ++j) top.v[j] = j < k ? sc.cand[(o + tid) * k + j] : 0;
        }
        M = wave_max(m);                               // (wave 0 holds every slice; only its threads use M)
        if (tid < SAMP_NS) term[tid] = m > -INFINITY ? sc.ssum[o + tid] * exp((double)(m - M)) : 0.0;
        __syncthreads();
        if (tid == 0)
            for (int j = 0; j < SAMP_NS; ++j) S += term[j];
    } else {
        scan_cols<KL>(r, 0, r.V, top, M, S, shf, shd);
    }
    const double lz = (double)M + log(S);              // log sum exp(L)
    if (tid == 0) {
        const int d = decisions[r.dec];
        // (+ 0.0f: -0 reads as +0, as the order has it)
        out.logp[r.out] = (d >= 0 && d < r.V) ? (float)((double)(raw_logit(r.lg, d, r.mask_id) + 0.0f) - lz) : __uint_as_float(0x7fc00000u);
    }
    for (int j = 0; j < k; ++j) {
        const uint64_t best = block_pop_best<KL>(top, best4);
        if (tid == 0) {
            out.ids[r.out * k + j] = topk_pair_col(best);
            out.tlp[r.out * k + j] = best ? (float)((double)f32_unsortable((uint32_t)(best >> 32)) - lz) : __uint_as_float(0x7fc00000u);
        }
    }
}

void launch_gen_topk(const void* logits0, const void* logits17, int V0, int Vs, int Vs_pad, const MttsSamplerCfg* cfgs,
                     const LoopState* ls, const SeqState* seqs, const int32_t* decisions, int B, const GenTopkScratch& sc,
                     const GenTopkOut& out, hipStream_t st) {
    const int k = out.k;
#define GT_ENGINE(KL)                                                                                                           \
    do {                                                                                                                        \
        if (V0 > SAMP_CAND)                                                                                                     \
            hipLaunchKernelGGL(gen_topk_slice_kernel<KL>, dim3(SAMP_NS, B), dim3(GT_T), 0, st, logits0, V0, cfgs, ls, seqs, k, sc, \
                               0, 0, 0);                                                                                        \
        hipLaunchKernelGGL(gen_topk_finish_kernel<KL>, dim3(8, B), dim3(GT_T), 0, st, logits0, logits17, V0, Vs, Vs_pad, cfgs, ls, \
                           seqs, decisions, k, sc, out, 0, 0, 0);                                                               \
    } while (0)
    TOPK_DISPATCH(k, GT_ENGINE);
#undef GT_ENGINE
}

void launch_gen_topk_single(const void* logits, int is_f32, int rows, int vocab, int mask_id, const int32_t* decisions,
                            const GenTopkScratch& sc, const GenTopkOut& out, hipStream_t st) {
    const int k = out.k;
#define GT_SINGLE(KL)                                                                                                          \
    do {                                                                                                                       \
        if (vocab > SAMP_CAND)                                                                                                 \
            hipLaunchKernelGGL(gen_topk_slice_kernel<KL>, dim3(SAMP_NS, rows), dim3(GT_T), 0, st, logits, vocab,               \
                               (const MttsSamplerCfg*)nullptr, (const LoopState*)nullptr, (const SeqState*)nullptr, k, sc, vocab, \
                               mask_id, is_f32);                                                                               \
        hipLaunchKernelGGL(gen_topk_finish_kernel<KL>, dim3(1, rows), dim3(GT_T), 0, st, logits, (const void*)nullptr, vocab,  \
                           vocab, vocab, (const MttsSamplerCfg*)nullptr, (const LoopState*)nullptr, (const SeqState*)nullptr,  \
                           decisions, k, sc, out, vocab, mask_id, is_f32);                                                     \
    } while (0)
    TOPK_DISPATCH(k, GT_SINGLE);
#undef GT_SINGLE
}
