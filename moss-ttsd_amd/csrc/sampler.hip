// Multi-codebook sampler and the delay-pattern state machine of the decode loop.
//
// sample_kernel   : reference modeling_asteroid.py:123-138 (logit masks, HF
//                   RepetitionPenalty/Temperature/TopK/TopP processors in that
//                   order, then argmax or a multinomial draw).
// update_kernel   : reference modeling_asteroid.py:139-169 (EOS flush via
//                   needs_additional_steps, teacher forcing of the delayed prompt
//                   tail, finished-row padding, stopping criteria).  Also commits what the step keeps per decision:
//                   lp (output_scores) and, as update_kernel<true>, the NaN slots of gen_topk.hip's results (top_logprobs).
//
// Draw definition (torch.multinomial's stream cannot be reproduced): Philox4x32-10,
// key = seed, counter = (step, row, channel, 0), u = (x0 >> 8) * 2^-24; kept tokens
// are walked in descending score and the first whose running sum of
// exp(score - max) exceeds u * total is taken.  oracle/asteroid_oracle.py
// (sample_from_scores) states the same rule.
#include "launch.h"
#include "sample_ctx.h"       // LogitsPtr, SampleCtx, sample_ctx: shared with gen_topk.hip

__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                                              uint32_t k1, uint32_t* out) {
#pragma unroll
    for (int i = 0; i < 10; ++i) {
        uint64_t p0 = (uint64_t)0xD2511F53u * c0;
        uint64_t p1 = (uint64_t)0xCD9E8D57u * c2;
        uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0;
        uint32_t n1 = (uint32_t)p1;
        uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        uint32_t n3 = (uint32_t)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// order-preserving map fp32 -> uint32 (larger float = larger key)
__device__ __forceinline__ uint32_t fkey(float f) {
    uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// Processed score of token i (everything except top-k / top-p, which act on the set).  A token banned this step
// (x.ban: mtts_set_sampler_bans; null in a run without bans) is at -inf like the masked id, before penalty and temperature.
// Every sampler pass reads scores through here, so a row whose every token is banned is a row of -inf to all of them:
// the argmax merges keep the lowest id (0), no candidate is collected, and the kernels below give token 0 with lp NaN.
// A token whose bit is set in x.bias_w (mtts_set_sampler_bias; null in a run without finite rules) carries an additive term
// this step: one fp32 addition on the fp32 value of the raw logit, behind the masks and in front of the penalty, which
// therefore sees the sign of raw + term (HF's order: SequenceBias, then RepetitionPenalty).  The stored logits stay raw.
__device__ __forceinline__ float bias_term(const MttsBiasTable* __restrict__ t, int i) {
    int lo = 0, hi = min(t->n, MTTS_BIAS_RULES_MAX);
    while (lo < hi) {                   // the first entry with ids[k] >= i
        const int mid = (lo + hi) >> 1;
        if (t->ids[mid] < i) lo = mid + 1; else hi = mid;
    }
    return (lo < MTTS_BIAS_RULES_MAX && lo < t->n && t->ids[lo] == i) ? t->term[lo] : 0.f;
}
__device__ __forceinline__ float proc_score(const SampleCtx& x, int i) {
    if (i == x.mask_id) return -INFINITY;
    if (x.ban && (x.ban[i >> 5] >> (i & 31)) & 1u) return -INFINITY;
    float s = x.lg.f32 ? ((const float*)x.lg.p)[i] : bf2f(((const uint16_t*)x.lg.p)[i]);
    if (x.bias_w && (x.bias_w[i >> 5] >> (i & 31)) & 1u) s = s + bias_term(x.bias_t, i);
    if (x.penalty > 0.f && (x.bm[i >> 5] >> (i & 31)) & 1u) s = (s < 0.f) ? s * x.penalty : s / x.penalty;
    if (x.temp > 0.f) s = s / x.temp;
    return s;
}

// ---------------------------------------------------------------------------
// Sampler = three short kernels per step.
//   A sample_scan_kernel    (big vocab only, grid (NS,B)): per-slice argmax + 11-bit
//                            radix histogram of the processed scores (global, per row)
//   B sample_collect_kernel (big vocab only, grid (NS,B)): bin b0 that holds the k-th
//                            largest score; every token in bins >= b0 is appended to the
//                            row's candidate list (a superset of the top-k set)
//   C sample_final_kernel   (grid (8,B)): candidates -> LDS, bitonic sort by
//                            (score asc, id asc), exact top-k threshold, top-p cut on
//                            the ascending cumulative softmax, Philox draw.
// Channels 1..7 (1025 tokens) skip A/B: kernel C reads the logits straight into LDS.
// Draw order: kept tokens from the highest score down (ties: higher id first); the
// first whose running sum of exp(score - max) exceeds u * total wins.
// ---------------------------------------------------------------------------
#define SAMP_T 256

__device__ __forceinline__ void argmax_merge(float& bv, int& bi, float ov, int oi) {
    if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
}

// block-wide argmax (lowest index wins ties); result valid in every thread
__device__ __forceinline__ void block_argmax(float& bv, int& bi, float* shf, int* shi) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) argmax_merge(bv, bi, __shfl_xor(bv, o, 64), __shfl_xor(bi, o, 64));
    const int wid = threadIdx.x >> 6, nw = blockDim.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) { shf[wid] = bv; shi[wid] = bi; }
    __syncthreads();
    bv = shf[0]; bi = shi[0];
    for (int w = 1; w < nw; ++w) argmax_merge(bv, bi, shf[w], shi[w]);
    __syncthreads();
}

// block-wide exclusive prefix sum of one double per thread (NT threads); returns (exclusive, total).
// Sums run in fp64: a nucleus over the whole 152 k vocabulary has terms of 1e-5 of the total, and the draw must
// land on the same token as the oracle's fp64 cumulative sum.
template <int NT>
__device__ __forceinline__ double block_excl_scan(double v, double* sh, double& total) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    double inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        double t = __shfl_up(inc, o, 64);
        if (lane >= o) inc += t;
    }
    __syncthreads();
    if (lane == 63) sh[wid] = inc;
    __syncthreads();
    double base = 0.0, tot = 0.0;
    for (int w = 0; w < NT / 64; ++w) { if (w < wid) base += sh[w]; tot += sh[w]; }
    total = tot;
    __syncthreads();
    return base + inc - v;
}

// LP (output_scores): a greedy row's slices also leave sum exp(s - slice max), combined by sample_final_kernel.
template <bool LP>
__global__ __launch_bounds__(SAMP_T) void sample_scan_kernel(
    const uint16_t* __restrict__ logits0, int V0, const uint32_t* __restrict__ bitmaps, int bm_words,
    const MttsSamplerCfg* __restrict__ cfgs, const LoopState* __restrict__ ls, const SeqState* __restrict__ seqs,
    SampleScratch sc, int single_vocab,
    int single_mask, int single_step, int single_channel) {
    __shared__ uint32_t hist[2048];
    __shared__ float shf[SAMP_T / 64];
    __shared__ int shi[SAMP_T / 64];
    __shared__ double shd[SAMP_T / 64];
    const int b = blockIdx.y, slice = blockIdx.x, tid = threadIdx.x;
    SampleCtx x;
    if (!sample_ctx(x, b, 0, logits0, nullptr, V0, 0, 0, bitmaps, bm_words, cfgs, ls, seqs, single_vocab, single_mask,
                    single_step, single_channel, sc.ban, sc.bias_w, sc.bias_t, sc.ext)) return;
    const MttsSamplerCfg cfg = cfgs[x.c];
    const bool want_hist = cfg.do_sample && cfg.top_k > 0 && cfg.top_k < x.V;
    for (int i = tid; i < 2048; i += SAMP_T) hist[i] = 0;
    __syncthreads();
    const int per = (x.V + SAMP_NS - 1) / SAMP_NS;
    const int i0 = slice * per, i1 = min(x.V, i0 + per);
    float bv = -INFINITY;
    int bi = 0x7fffffff;
    for (int i = i0 + tid; i < i1; i += SAMP_T) {
        float s = proc_score(x, i);
        argmax_merge(bv, bi, s, i);
        if (want_hist) atomicAdd(&hist[fkey(s) >> 21], 1u);
    }
    block_argmax(bv, bi, shf, shi);
    if (tid == 0) { sc.slice_val[b * SAMP_NS + slice] = bv; sc.slice_idx[b * SAMP_NS + slice] = bi; }
    if (LP && !cfg.do_sample) {
        // second pass over the slice (L2 resident): at most 19 fp32 terms per thread, then fp64 in a fixed order
        float loc = 0.f;
        if (bv > -INFINITY)
            for (int i = i0 + tid; i < i1; i += SAMP_T) {
                const float s = proc_score(x, i);
                if (s > -INFINITY) loc += expf(s - bv);
            }
        double tot;
        (void)block_excl_scan<SAMP_T>((double)loc, shd, tot);
        if (tid == 0) sc.slice_sum[b * SAMP_NS + slice] = (float)tot;
    }
    if (want_hist)
        for (int i = tid; i < 2048; i += SAMP_T)
            if (hist[i]) atomicAdd(&sc.hist[(size_t)b * 2048 + i], hist[i]);
}

// ---- helpers of the full-vocabulary path (sample_full_kernel below; its first pass runs inside sample_collect_kernel)
#define SAMP_FT 1024
#define NUC_BINS 2048
#define NUC_SCALE 35184372088832.0          // 2^45
typedef unsigned long long u64;

struct NucSel {            // membership of the current candidate set, in (key, id) order
    uint32_t kmin;         // survivors of top-k: key >= kmin (and finite)
    uint32_t kp;           // kept by top-p: key > kp, or key == kp and id >= idp
    int idp;
    uint32_t kmax = 0xffffffffu;       // typical_p, the one stage that can cut from the top: key <= kmax
};
__device__ __forceinline__ float unfkey(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }
__device__ __forceinline__ bool nuc_in(const NucSel& z, uint32_t key, int id) {
    return key > 0x007fffffu /* fkey(-inf) */ && key >= z.kmin && key <= z.kmax && (key > z.kp || (key == z.kp && id >= z.idp));
}
__device__ __forceinline__ int nuc_bin(uint32_t key, float lo) {
    const int b = (int)((unfkey(key) - lo) * ((float)(NUC_BINS - 1) / 32.0f));      // monotone in the score
    return min(max(b, 0), NUC_BINS - 1);
}

__device__ __forceinline__ u64 nuc_q(uint32_t key, float smax) { return (u64)((double)expf(unfkey(key) - smax) * NUC_SCALE); }

// Pass A for tokens i0, i0 + step, ... < i1 of one row: processed score -> key + level-0 bin (scratch, read by every later
// pass) and the level-0 histogram in LDS (cnt / mass: 2048 entries each, zeroed by the caller).
__device__ __forceinline__ void nuc_pass_a(const SampleCtx& x, float smax, float lo, uint32_t* __restrict__ keys,
                                           uint16_t* __restrict__ bins, unsigned int* cnt, u64* mass, int i0, int i1, int step) {
    for (int i = i0; i < i1; i += step) {
        const float s = proc_score(x, i) + 0.0f;      // (-0 -> +0: one key per value)
        const uint32_t key = fkey(s);
        keys[i] = key;
        if (s > -INFINITY) {
            const int d = nuc_bin(key, lo);
            bins[i] = (uint16_t)d;
            atomicAdd(&cnt[d], 1u);
            atomicAdd(&mass[d], nuc_q(key, smax));
        } else bins[i] = 0xffffu;
    }
}


// Bin of the k-th largest score in a 2048-bin histogram of fkey(score) >> 21 (LDS or global), SAMP_T threads:
// thread t owns bins 8t..8t+7; suffix sums over lanes and waves locate the bin.  Result in every thread.
__device__ __forceinline__ int topk_bin(const uint32_t* hist, uint32_t k, uint32_t* wsum, int* sh_b0) {
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const uint32_t* h = hist + tid * 8;
    uint32_t cnt[8], mine = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) { cnt[j] = h[j]; mine += cnt[j]; }
    uint32_t suf = mine;                      // inclusive suffix sum over lanes >= lane
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        uint32_t t = __shfl_down(suf, o, 64);
        if (lane + o < 64) suf += t;
    }
    if (lane == 0) wsum[wid] = suf;
    if (tid == 0) *sh_b0 = 0;
    __syncthreads();
    uint32_t above_waves = 0;
    for (int w = wid + 1; w < SAMP_T / 64; ++w) above_waves += wsum[w];
    const uint32_t above = above_waves + suf - mine;      // scores in bins strictly above this thread's
    if (above < k && above + mine >= k) {
        uint32_t run = above;
        for (int j = 7; j >= 0; --j) {
            run += cnt[j];
            if (run >= k) { *sh_b0 = tid * 8 + j; break; }
        }
    }
    __syncthreads();
    return *sh_b0;
}

__global__ __launch_bounds__(SAMP_T) void sample_collect_kernel(
    const uint16_t* __restrict__ logits0, int V0, const uint32_t* __restrict__ bitmaps, int bm_words,
    const MttsSamplerCfg* __restrict__ cfgs, const LoopState* __restrict__ ls, const SeqState* __restrict__ seqs,
    SampleScratch sc, int full_cap, int single_vocab,
    int single_mask, int single_step, int single_channel) {
    __shared__ uint32_t wsum[SAMP_T / 64];
    __shared__ int sh_b0;
    const int b = blockIdx.y, slice = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    SampleCtx x;
    if (!sample_ctx(x, b, 0, logits0, nullptr, V0, 0, 0, bitmaps, bm_words, cfgs, ls, seqs, single_vocab, single_mask,
                    single_step, single_channel, sc.ban, sc.bias_w, sc.bias_t, sc.ext)) return;
    const MttsSamplerCfg cfg = cfgs[x.c];
    if (!cfg.do_sample) return;
    // no top-k (every finite score is a candidate) or a top_k beyond the candidate buffer: nothing to collect, the row
    // goes to the full-vocabulary kernel (the final kernel flags it when it sees more than SAMP_CAND candidates)
    if (!(cfg.top_k > 0 && cfg.top_k < x.V) || cfg.top_k > SAMP_CAND) {
        // ... whose first pass over the row (keys, level-0 bins, level-0 histogram) is done HERE, by the row's 32 blocks
        __shared__ unsigned int a_cnt[2048];
        __shared__ unsigned long long a_mass[2048];
        float smax = sc.slice_val[b * SAMP_NS + (lane & (SAMP_NS - 1))];
        smax = wave_max(smax);
        for (int i = tid; i < 2048; i += SAMP_T) { a_cnt[i] = 0; a_mass[i] = 0; }
        __syncthreads();
        const int per = (x.V + SAMP_NS - 1) / SAMP_NS;
        const int i0 = slice * per, i1 = min(x.V, i0 + per);
        nuc_pass_a(x, smax, smax - 32.0f, (uint32_t*)(sc.full_idx + (size_t)b * full_cap), (uint16_t*)(sc.full_val + (size_t)b * full_cap),
                   a_cnt, a_mass, i0 + tid, i1, SAMP_T);
        __syncthreads();
        for (int i = tid; i < 2048; i += SAMP_T)
            if (a_cnt[i]) { atomicAdd(&sc.nuc_cnt[(size_t)b * 2048 + i], a_cnt[i]); atomicAdd(&sc.nuc_mass[(size_t)b * 2048 + i], a_mass[i]); }
        if (slice == 0 && tid == 0) { sc.cand_n[b] = SAMP_CAND + 1; sc.overflow[b] = 2; }
        return;
    }
    const int b0 = topk_bin(sc.hist + (size_t)b * 2048, (uint32_t)cfg.top_k, wsum, &sh_b0);
    const uint32_t ninf_key = fkey(-INFINITY);
    const int per = (x.V + SAMP_NS - 1) / SAMP_NS;
    const int i0 = slice * per, i1 = min(x.V, i0 + per);
    for (int i = i0 + tid; i < i1; i += SAMP_T) {
        float s = proc_score(x, i);
        uint32_t key = fkey(s);
        if ((int)(key >> 21) >= b0 && key > ninf_key) {
            uint32_t slot = atomicAdd(&sc.cand_n[b], 1u);
            if (slot < SAMP_CAND) { sc.cand_val[(size_t)b * SAMP_CAND + slot] = s; sc.cand_idx[(size_t)b * SAMP_CAND + slot] = i; }
        }
    }
}

// ---- typical_p (HF TypicalLogitsWarper; mtts/warp_spec.py states the rule).  Over the kept set, with d_i = s_i - smax,
// e_i = exp(d_i) and p_i = e_i / tot: the surprisal is ln tot - d_i and the entropy H = ln tot - sum p_i d_i, so
// shift_i = |-ln p_i - H| = |d_i - dc| with dc = sum p_i d_i, the mean of d.  Both sampler paths take the shift as the
// fp32 value below: a function of the score alone (tokens of equal score stay or leave together), falling to the
// entropy crossing and rising after it as the score ascends, so "shift <= t" is an interval in score order.
__device__ __forceinline__ uint32_t typ_shift_bits(float d, double dc) { return __float_as_uint((float)fabs((double)d - dc)); }

// block-wide sum, the same bits in every thread; one barrier per call: consecutive calls alternate between the two rows of sh
template <int NT>
__device__ __forceinline__ double block_sum_alt(double v, double (*sh)[NT / 64], int it) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if ((threadIdx.x & 63) == 0) sh[it & 1][threadIdx.x >> 6] = v;
    __syncthreads();
    double s = 0.0;
#pragma unroll
    for (int w = 0; w < NT / 64; ++w) s += sh[it & 1][w];
    return s;
}

// In-block path: cval ascends over [first_keep, hi_keep).  t* = the smallest shift whose tokens {shift <= t*} hold typ of
// the mass, found by bisection on the shift's bit pattern (non-negative floats order as their bits): every thread keeps
// its run's (shift, e) in registers and a step costs one block sum.  The leavers are a prefix and a suffix of the range.
template <int NT>
__device__ void typical_cut(const float* __restrict__ cval, float smax, float typ, int& first_keep, int& hi_keep, double* shd) {
    constexpr int TPT = SAMP_CAND / NT;         // tokens per thread at most
    __shared__ double alt[2][NT / 64];
    const int tid = threadIdx.x;
    const int mk = hi_keep - first_keep;
    const int perf = (mk + NT - 1) / NT;
    const int a0 = first_keep + tid * perf, a1 = min(hi_keep, a0 + perf);
    float dd[TPT], ee[TPT];
    double loc = 0.0, loc1 = 0.0;
#pragma unroll
    for (int j = 0; j < TPT; ++j) {
        const bool on = j < perf && a0 + j < a1;
        dd[j] = on ? cval[a0 + j] - smax : 0.f;
        ee[j] = on ? expf(dd[j]) : 0.f;
        loc += (double)ee[j];
        loc1 += (double)ee[j] * (double)dd[j];
    }
    double tot, tot1;
    (void)block_excl_scan<NT>(loc, shd, tot);
    (void)block_excl_scan<NT>(loc1, shd, tot1);
    const double dc = tot1 / tot, need = (double)typ * tot;
    uint32_t sb[TPT];
#pragma unroll
    for (int j = 0; j < TPT; ++j) sb[j] = (j < perf && a0 + j < a1) ? typ_shift_bits(dd[j], dc) : 0xffffffffu;
    uint32_t lo = 0u, hi = 0x7f800000u;         // (at +inf every token is in: the mass is tot >= need)
    for (int it = 0; lo < hi; ++it) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        double m = 0.0;
#pragma unroll
        for (int j = 0; j < TPT; ++j) m += sb[j] <= mid ? (double)ee[j] : 0.0;
        if (block_sum_alt<NT>(m, alt, it) >= need) hi = mid; else lo = mid + 1;
    }
    int below = 0, above = 0;
#pragma unroll
    for (int j = 0; j < TPT; ++j)
        if (sb[j] != 0xffffffffu && sb[j] > lo) { if ((double)dd[j] < dc) ++below; else ++above; }
    double nb, na;
    (void)block_excl_scan<NT>((double)below, shd, nb);
    (void)block_excl_scan<NT>((double)above, shd, na);
    first_keep += (int)nb;
    hi_keep -= (int)na;
}

// Everything after the candidates are known: sort, HF top-k / top-p cuts, Philox draw.
// val/idx: n candidate (score, id) pairs (LDS for the fast path, global memory for the full-vocabulary path),
// capacity >= next_pow2(n).  NT threads.  Returns the chosen token in every thread; lp (may be null): thread 0's
// receives log(softmax over the kept set)[pick].  FL: the probability floors `fl` (mtts.h: MttsSamplerFloors) cut the kept
// set once more per active floor.  TY: typical_p `typ` (0: absent) runs between min_p and epsilon_cutoff and may cut the kept
// range from the top as well: [first_keep, hi_keep) from there on.
template <int NT, bool FL, bool TY>
__device__ int finish_sample(float* __restrict__ cval, int* __restrict__ cidx, int n, const MttsSamplerCfg& cfg, float smax,
                             uint32_t step, uint32_t b, uint32_t c, uint64_t seed, double* shd, int* sh_i, float* lp,
                             const MttsSamplerFloors& fl, float typ) {
    const int tid = threadIdx.x;
    // bitonic sort of P = next_pow2(n) slots by (score asc, id asc); padding sorts last
    int P = 1;
    while (P < n) P <<= 1;
    for (int i = n + tid; i < P; i += NT) { cval[i] = INFINITY; cidx[i] = 0x7fffffff; }
    __syncthreads();
    for (int kk = 2; kk <= P; kk <<= 1) {
        for (int j = kk >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < P; t += NT) {
                int ixj = t ^ j;
                if (ixj > t) {
                    bool up = ((t & kk) == 0);
                    float a = cval[t], bb = cval[ixj];
                    int ai = cidx[t], bi2 = cidx[ixj];
                    bool gt = (a > bb) || (a == bb && ai > bi2);
                    if (gt == up) { cval[t] = bb; cval[ixj] = a; cidx[t] = bi2; cidx[ixj] = ai; }
                }
            }
            __syncthreads();
        }
    }
    // top-k (HF TopKLogitsWarper): drop scores < k-th largest; ties with the k-th stay
    int f0 = 0;
    if (cfg.top_k > 0 && cfg.top_k < n) {
        const float thr = cval[n - cfg.top_k];
        int cnt = 0;
        for (int i = tid; i < n; i += NT) cnt += (cval[i] < thr) ? 1 : 0;
        double tot;
        (void)block_excl_scan<NT>((double)cnt, shd, tot);
        f0 = (int)tot;
    }
    // top-p (HF TopPLogitsWarper): ascending cumulative softmax over the survivors; drop cum <= 1-p,
    // always keep the last (most probable) one.  Thread t owns a contiguous run of the kept range.
    const int m = n - f0;                                  // survivors of top-k
    const int per = (m + NT - 1) / NT;
    int first_keep = f0;
    if (cfg.top_p > 0.f && cfg.top_p < 1.0f) {
        const int a0 = f0 + tid * per, a1 = min(n, a0 + per);
        double loc = 0.0;
        for (int i = a0; i < a1; ++i) loc += (double)expf(cval[i] - smax);
        double tot;
        double base = block_excl_scan<NT>(loc, shd, tot);
        int drop = 0;
        double run = base;
        for (int i = a0; i < a1; ++i) {
            run += (double)expf(cval[i] - smax);
            if (i < n - 1 && (float)(run / tot) <= cfg.one_minus_top_p) drop++;
        }
        double dtot;
        (void)block_excl_scan<NT>((double)drop, shd, dtot);
        first_keep = f0 + (int)dtot;          // cum is monotone: the dropped ones are a prefix
    }
    // probability floors (HF MinP / Epsilon / EtaLogitsWarper, in that order, each on the survivors of the last): a token
    // leaves iff its share of the kept mass is below the floor and its score below the maximum.  Scores ascend, so the
    // leavers are again a prefix of [first_keep, n)
    int hi_keep = n;            // the kept range is [first_keep, hi_keep); only typical_p lowers its top, cval[hi_keep - 1]
    float stop = smax;
    if constexpr (FL) {
        for (int w = 0; w < 3; ++w) {
            if constexpr (TY) {
                if (w == 1 && typ > 0.f) {
                    typical_cut<NT>(cval, smax, typ, first_keep, hi_keep, shd);
                    stop = cval[hi_keep - 1];
                }
            }
            const float fv = w == 0 ? fl.min_p : w == 1 ? fl.epsilon_cutoff : fl.eta_cutoff;
            if (!(fv > 0.f)) continue;
            const int mk = hi_keep - first_keep;
            const int perf = (mk + NT - 1) / NT;
            const int a0 = first_keep + tid * perf, a1 = min(hi_keep, a0 + perf);
            double loc = 0.0, loc1 = 0.0;
            for (int i = a0; i < a1; ++i) {
                const double d = (double)(cval[i] - smax), e = (double)expf(cval[i] - smax);
                loc += e;
                loc1 += e * d;
            }
            double tot, tot1 = 0.0;
            (void)block_excl_scan<NT>(loc, shd, tot);
            if (w == 2) (void)block_excl_scan<NT>(loc1, shd, tot1);
            // the floor as a mass: p_i < floor  <=>  e_i < floor * tot  (p_max = 1 / tot: the top token has e = 1)
            double thr;
            if (w == 0) thr = (double)fv;
            else if (w == 1) thr = (double)fv * tot;
            else {
                const double H = log(tot) - tot1 / tot;       // -sum p ln p, p = e / tot, ln p = (s - smax) - ln tot
                thr = fmin((double)fv, (double)fl.sqrt_eta_cutoff * exp(-H)) * tot;
            }
            int drop = 0;
            for (int i = a0; i < a1; ++i) drop += ((double)expf(cval[i] - smax) < thr && cval[i] < stop) ? 1 : 0;
            double dtot;
            (void)block_excl_scan<NT>((double)drop, shd, dtot);
            first_keep += (int)dtot;
        }
    }
    // draw: walk kept tokens from the top (position hi_keep-1 down to first_keep)
    const int nk = hi_keep - first_keep;
    const int perk = (nk + NT - 1) / NT;
    const int r0 = tid * perk, r1 = min(nk, r0 + perk);    // ranks from the top
    n = hi_keep;
    double loc = 0.0;
    for (int r = r0; r < r1; ++r) loc += (double)expf(cval[n - 1 - r] - smax);
    double tot;
    double base = block_excl_scan<NT>(loc, shd, tot);
    uint32_t rnd[4];
    philox4x32_10(step, b, c, 0u, (uint32_t)seed, (uint32_t)(seed >> 32), rnd);
    const double u = (double)((float)(rnd[0] >> 8) * (1.0f / 16777216.0f));
    const double target = u * tot;
    if (tid == 0) sh_i[1] = 0x7fffffff;
    __syncthreads();
    double run = base;
    for (int r = r0; r < r1; ++r) {
        run += (double)expf(cval[n - 1 - r] - smax);
        if (run > target) { atomicMin(&sh_i[1], r); break; }
    }
    __syncthreads();
    int r = sh_i[1];
    if (r >= nk) r = nk - 1;                    // u*tot rounding: fall back to the last kept token
    // output_scores: log-probability of the pick under the distribution it was drawn from (the kept set, total `tot`)
    if (lp && tid == 0) *lp = (float)((double)(cval[n - 1 - r] - smax) - log(tot));
    return cidx[n - 1 - r];
}

// The body of sample_final_kernel<LP, FL> (TY false) and of sample_final_typ_kernel<LP> (TY: typical_p per channel in
// `typical`, 0 = absent; `floors` may then be null).  A run without typical_p launches the kernels it launched before.
template <bool LP, bool FL, bool TY>
__device__ __forceinline__ void sample_final_body(
    const uint16_t* __restrict__ logits0, const uint16_t* __restrict__ logits17, int V0, int Vs, int Vs_pad,
    const uint32_t* __restrict__ bitmaps, int bm_words, const MttsSamplerCfg* __restrict__ cfgs,
    const LoopState* __restrict__ ls, const SeqState* __restrict__ seqs, uint64_t seed, int32_t* __restrict__ decisions,
    int32_t* __restrict__ err, const SampleScratch& sc, int big_channel0, int single_vocab, int single_mask, int single_step, int single_channel,
    const MttsSamplerFloors* __restrict__ floors, const float* __restrict__ typical) {
    __shared__ float cval[SAMP_CAND];
    __shared__ int cidx[SAMP_CAND];
    __shared__ float shf[SAMP_T / 64];
    __shared__ double shd[SAMP_T / 64];
    __shared__ int shi[SAMP_T / 64];
    __shared__ int sh_i[4];
    __shared__ uint32_t hist[2048];
    __shared__ uint32_t wsum[SAMP_T / 64];
    const int tid = threadIdx.x;
    const int b = blockIdx.y;
    SampleCtx x;
    if (!sample_ctx(x, b, blockIdx.x, logits0, logits17, V0, Vs, Vs_pad, bitmaps, bm_words, cfgs, ls, seqs, single_vocab,
                    single_mask, single_step, single_channel, sc.ban, sc.bias_w, sc.bias_t, sc.ext)) return;
    const MttsSamplerCfg cfg = cfgs[x.c];
    const bool big = single_vocab > 0 ? (single_vocab > SAMP_CAND) : (x.c == 0 && big_channel0);
    const int out_slot = b * 8 + x.c;
    int n = 0;
    float smax; int amax;
    if (big) {
        float bv = -INFINITY; int bi = 0x7fffffff;
        if (tid < SAMP_NS) { bv = sc.slice_val[b * SAMP_NS + tid]; bi = sc.slice_idx[b * SAMP_NS + tid]; }
        block_argmax(bv, bi, shf, shi);
        smax = bv; amax = bi;
        if (cfg.do_sample) {
            n = (int)sc.cand_n[b];
            const int nn = min(n, SAMP_CAND);
            for (int i = tid; i < nn; i += SAMP_T) { cval[i] = sc.cand_val[(size_t)b * SAMP_CAND + i]; cidx[i] = sc.cand_idx[(size_t)b * SAMP_CAND + i]; }
        }
        __syncthreads();
        // reset the per-row scratch for the next step
        for (int i = tid; i < 2048; i += SAMP_T) sc.hist[(size_t)b * 2048 + i] = 0;
        if (tid == 0) sc.cand_n[b] = 0;
    } else {
        // small vocabulary (channels 1..7): scores straight from the logits.  With top_k set, an LDS histogram
        // first finds the radix bin of the k-th largest score and only that bin and the ones above it are kept
        // (a superset of the top-k set, typically ~2k entries): the sort below then runs on 64-128 slots, not 2048.
        float bv = -INFINITY; int bi = 0x7fffffff;
        const bool prefilter = cfg.do_sample && cfg.top_k > 0 && cfg.top_k < x.V;
        if (tid == 0) sh_i[0] = 0;
        if (prefilter)
            for (int i = tid; i < 2048; i += SAMP_T) hist[i] = 0;
        __syncthreads();
        for (int i = tid; i < x.V; i += SAMP_T) {
            float s = proc_score(x, i);
            argmax_merge(bv, bi, s, i);
            if (prefilter) atomicAdd(&hist[fkey(s) >> 21], 1u);
            else if (cfg.do_sample && s > -INFINITY) {
                int slot = atomicAdd(&sh_i[0], 1);
                if (slot < SAMP_CAND) { cval[slot] = s; cidx[slot] = i; }
            }
        }
        if (prefilter) {
            __syncthreads();
            const int b0 = topk_bin(hist, (uint32_t)cfg.top_k, wsum, &sh_i[2]);
            const uint32_t ninf_key = fkey(-INFINITY);
            for (int i = tid; i < x.V; i += SAMP_T) {
                float s = proc_score(x, i);
                uint32_t key = fkey(s);
                if ((int)(key >> 21) >= b0 && key > ninf_key) {
                    int slot = atomicAdd(&sh_i[0], 1);
                    if (slot < SAMP_CAND) { cval[slot] = s; cidx[slot] = i; }
                }
            }
        }
        block_argmax(bv, bi, shf, shi);
        smax = bv; amax = bi;
        n = sh_i[0];
    }
    if (!cfg.do_sample) {
        if (tid == 0) decisions[out_slot] = amax;
        if (LP) {
            // greedy: lp = log_softmax over every finite processed score at the argmax = -log(sum exp(s - smax)).
            // -inf scores add nothing; an all -inf row (every token banned: smax = -inf, amax = 0) gives NaN, no trap.
            double tot = 0.0;
            if (big) {
                if (tid == 0)                    // the row's 32 (slice max, slice sum) pairs, in slice order
                    for (int j = 0; j < SAMP_NS; ++j) {
                        const float m = sc.slice_val[b * SAMP_NS + j];
                        if (m > -INFINITY) tot += (double)sc.slice_sum[b * SAMP_NS + j] * (double)expf(m - smax);
                    }
            } else {
                float loc = 0.f;
                if (smax > -INFINITY)
                    for (int i = tid; i < x.V; i += SAMP_T) {
                        const float s = proc_score(x, i);
                        if (s > -INFINITY) loc += expf(s - smax);
                    }
                (void)block_excl_scan<SAMP_T>((double)loc, shd, tot);
            }
            if (tid == 0) sc.lp[out_slot] = tot > 0.0 ? (float)(-log(tot)) : __uint_as_float(0x7fc00000u);
        }
        return;
    }
    if (n > SAMP_CAND || n == 0) {               // too many candidates: hand the row to the full-vocabulary kernel
        if (tid == 0) {
            decisions[out_slot] = amax;
            if (n > SAMP_CAND && sc.overflow[b] == 0) sc.overflow[b] = 1;
            // channel 0 with too many candidates: the full-vocabulary kernel overwrites this.  n == 0 (every score -inf:
            // every token of the row is banned, amax = 0) on ANY channel: token 0 and the NaN are final where nothing
            // follows; the full-vocabulary kernel finds no member either (n == 0 there) and writes the same pair
            if (LP) sc.lp[out_slot] = __uint_as_float(0x7fc00000u);
        }
        return;
    }
    float lpv = 0.f;
    MttsSamplerFloors fl{0.f, 0.f, 0.f, 0.f};
    if constexpr (FL) { if (!TY || floors) fl = floors[x.c]; }
    float typ = 0.f;
    if constexpr (TY) typ = typical[x.c];
    const int pick = finish_sample<SAMP_T, FL, TY>(cval, cidx, n, cfg, smax, (uint32_t)x.step, x.row_id, (uint32_t)x.c,
                                                   single_vocab > 0 ? seed : x.seed, shd, sh_i, LP ? &lpv : nullptr, fl, typ);
    if (tid == 0) {
        decisions[out_slot] = pick;
        if (LP) sc.lp[out_slot] = lpv;
    }
}

template <bool LP, bool FL>
__global__ __launch_bounds__(SAMP_T) void sample_final_kernel(
    const uint16_t* __restrict__ logits0, const uint16_t* __restrict__ logits17, int V0, int Vs, int Vs_pad,
    const uint32_t* __restrict__ bitmaps, int bm_words, const MttsSamplerCfg* __restrict__ cfgs,
    const LoopState* __restrict__ ls, const SeqState* __restrict__ seqs, uint64_t seed, int32_t* __restrict__ decisions,
    int32_t* __restrict__ err, SampleScratch sc, int big_channel0, int single_vocab, int single_mask, int single_step, int single_channel,
    const MttsSamplerFloors* __restrict__ floors) {
    sample_final_body<LP, FL, false>(logits0, logits17, V0, Vs, Vs_pad, bitmaps, bm_words, cfgs, ls, seqs, seed, decisions, err, sc,
                                     big_channel0, single_vocab, single_mask, single_step, single_channel, floors, nullptr);
}
template <bool LP>
__global__ __launch_bounds__(SAMP_T) void sample_final_typ_kernel(
    const uint16_t* __restrict__ logits0, const uint16_t* __restrict__ logits17, int V0, int Vs, int Vs_pad,
    const uint32_t* __restrict__ bitmaps, int bm_words, const MttsSamplerCfg* __restrict__ cfgs,
    const LoopState* __restrict__ ls, const SeqState* __restrict__ seqs, uint64_t seed, int32_t* __restrict__ decisions,
    int32_t* __restrict__ err, SampleScratch sc, int big_channel0, int single_vocab, int single_mask, int single_step, int single_channel,
    const MttsSamplerFloors* __restrict__ floors, const float* __restrict__ typical) {
    sample_final_body<LP, true, true>(logits0, logits17, V0, Vs, Vs_pad, bitmaps, bm_words, cfgs, ls, seqs, seed, decisions, err, sc,
                                      big_channel0, single_vocab, single_mask, single_step, single_channel, floors, typical);
}

// ---------------------------------------------------------------------------------------------------------------
// Full-vocabulary path (sampling without top_k, or a top_k beyond the candidate buffer): the same HF rules and the same
// draw as finish_sample, WITHOUT sorting the row.  In the order (score asc, id asc) every quantity the rules need is
// a position found by counting or by mass: the k-th largest score (top-k threshold), the longest prefix whose
// cumulative softmax mass is <= 1 - top_p, and the token at which the running mass from the top exceeds u * total.
// Each is located by radix selection: a 2048-bin histogram (count + mass) over a linear binning of the score, then the
// three digits (11 | 11 | 10 bits) of the order-preserving key inside the crossing bin, then -- among tokens of EQUAL
// score -- two 9-bit digits of the token id.  One 1024-thread block per row, ~11 passes over the row's keys (L2
// resident), against the 171 global-memory bitonic passes over 2^18 slots this replaces (17 ms -> tens of us).
// Masses are exact integers (exp(s - max) * 2^45, uint64): sums do not depend on the order of the LDS atomics, so the
// pick is reproducible; against the fp64 sums of the in-block path / the oracle they differ by < 1e-8 of the total.
// ---------------------------------------------------------------------------------------------------------------
struct NucShared {
    unsigned int cnt0[NUC_BINS];      // level-0 histogram (linear score bins) of the CURRENT candidate set
    u64 mass0[NUC_BINS];
    unsigned int cnt[NUC_BINS];       // digit histograms of the passes below
    u64 mass[NUC_BINS];
    u64 wm[SAMP_FT / 64];
    unsigned int wc[SAMP_FT / 64];
    int cross;
    unsigned int out_cnt, grp_cnt;
    u64 out_mass, grp_mass;
};
// member(i) for every token i of level-0 bin `binA`, the row's tokens spread over the block's threads.
// The bins are read 8 per 16-byte load, four loads in flight per thread (a load-test-loop pays one L2 round trip per
// token); almost every group holds no token of bin `binA` and leaves after one packed compare.
template <typename F>
__device__ __forceinline__ void nuc_scan_bin(const uint16_t* __restrict__ bins, int V, int binA, F member) {
    const int G = (V + 7) >> 3;                           // (bins[V .. 8G) hold 0xffff: sample_full_kernel pads them)
    const u32x4_t* bv = (const u32x4_t*)bins;
    const uint32_t pat = (uint32_t)binA * 0x00010001u;
    for (int g0 = threadIdx.x; g0 < G; g0 += SAMP_FT * 4) {
        u32x4_t w[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int g = g0 + u * SAMP_FT;
            w[u] = g < G ? bv[g] : u32x4_t{~0u, ~0u, ~0u, ~0u};
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int g = g0 + u * SAMP_FT;
            const uint32_t ww[4] = {w[u].x ^ pat, w[u].y ^ pat, w[u].z ^ pat, w[u].w ^ pat};
            uint32_t any = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) any |= (ww[k] - 0x00010001u) & ~ww[k] & 0x80008000u;    // a zero half-word somewhere?
            if (!any) continue;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if ((ww[k] & 0xffffu) == 0) member(8 * g + 2 * k);
                if ((ww[k] >> 16) == 0) member(8 * g + 2 * k + 1);
            }
        }
    }
}

// One digit pass over the row, restricted to the tokens of level-0 bin `binA` that are members of `z`.
// level 1..3: key digits (higher digits == `prefix`); 4, 5: id digits (9 bits each) of the tokens whose key == `prefix`.
__device__ void nuc_hist(NucShared& S, const uint32_t* __restrict__ keys, const uint16_t* __restrict__ bins, int V, const NucSel& z,
                         float smax, int level, int binA, uint32_t prefix, int idhi) {
    for (int i = threadIdx.x; i < NUC_BINS; i += SAMP_FT) { S.cnt[i] = 0; S.mass[i] = 0; }
    __syncthreads();
    auto member = [&](int i) {
        const uint32_t key = keys[i];
        if (!nuc_in(z, key, i)) return;
        int d;
        if (level == 1) d = key >> 21;
        else if (level == 2) { if ((key >> 21) != prefix) return; d = (key >> 10) & 2047; }
        else if (level == 3) { if ((key >> 10) != prefix) return; d = key & 1023; }
        else {
            if (key != prefix) return;
            if (level == 4) d = i >> 9;
            else { if ((i >> 9) != idhi) return; d = i & 511; }
        }
        atomicAdd(&S.cnt[d], 1u);
        if (level <= 3) atomicAdd(&S.mass[d], nuc_q(key, smax));
    };
    nuc_scan_bin(bins, V, binA, member);
    __syncthreads();
}

// Walk the bins of (cnt, mass) in ascending (asc) or descending order and find the first one at which `crossed(count so far
// incl. the bin, mass so far incl. the bin)` holds (it is monotone).  `bc` / `bm` = count / mass in front of the walk; on
// return they hold the totals in front of the crossing bin, S.grp_cnt / S.grp_mass that bin's own content.  Returns the
// bin, or -1 (then S.wc / S.wm hold the per-wave totals of the walk).
template <typename F>
__device__ int nuc_cross(NucShared& S, const unsigned int* cnt, const u64* mass, bool asc, unsigned int& bc, u64& bm, F crossed) {
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int p0 = 2 * tid, b0 = asc ? p0 : NUC_BINS - 1 - p0, b1 = asc ? p0 + 1 : NUC_BINS - 2 - p0;
    const unsigned int c0 = cnt[b0], c1 = cnt[b1];
    const u64 m0 = mass[b0], m1 = mass[b1];
    unsigned int ic = c0 + c1;
    u64 im = m0 + m1;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned int tc = __shfl_up(ic, o, 64);
        const u64 tm = __shfl_up(im, o, 64);
        if (lane >= o) { ic += tc; im += tm; }
    }
    if (tid == 0) S.cross = 0x7fffffff;
    __syncthreads();
    if (lane == 63) { S.wc[wid] = ic; S.wm[wid] = im; }
    __syncthreads();
    unsigned int ec = bc + ic - (c0 + c1);
    u64 em = bm + im - (m0 + m1);
    for (int w = 0; w < wid; ++w) { ec += S.wc[w]; em += S.wm[w]; }
    const bool x0 = (c0 > 0) && crossed(ec + c0, em + m0);
    const bool x1 = (c1 > 0) && crossed(ec + c0 + c1, em + m0 + m1);
    if (x0) atomicMin(&S.cross, p0);
    else if (x1) atomicMin(&S.cross, p0 + 1);
    __syncthreads();
    const int px = S.cross;
    if (px == p0) { S.out_cnt = ec; S.out_mass = em; S.grp_cnt = c0; S.grp_mass = m0; }
    if (px == p0 + 1) { S.out_cnt = ec + c0; S.out_mass = em + m0; S.grp_cnt = c1; S.grp_mass = m1; }
    __syncthreads();
    if (px == 0x7fffffff) return -1;
    bc = S.out_cnt;
    bm = S.out_mass;
    return asc ? px : NUC_BINS - 1 - px;
}

// Locate the crossing of `crossed` down to one key value.  false: the walk never crosses.  Else `key` = the score group (all
// member tokens of that key), bc / bm = what lies in front of the group, gc / gm = the group's count / mass; binA = its level-0
// bin, c_bin / m_bin = what lies in front of that bin.
template <typename F>
__device__ bool nuc_select_key(NucShared& S, const uint32_t* keys, const uint16_t* bins, int V, const NucSel& z, float smax, bool asc,
                               unsigned int& bc, u64& bm, F crossed, uint32_t& key, unsigned int& gc, u64& gm, int& binA,
                               unsigned int& c_bin, u64& m_bin) {
    binA = nuc_cross(S, S.cnt0, S.mass0, asc, bc, bm, crossed);
    if (binA < 0) return false;
    c_bin = bc;
    m_bin = bm;
    nuc_hist(S, keys, bins, V, z, smax, 1, binA, 0, 0);
    const int d1 = nuc_cross(S, S.cnt, S.mass, asc, bc, bm, crossed);
    nuc_hist(S, keys, bins, V, z, smax, 2, binA, (uint32_t)d1, 0);
    const int d2 = nuc_cross(S, S.cnt, S.mass, asc, bc, bm, crossed);
    nuc_hist(S, keys, bins, V, z, smax, 3, binA, ((uint32_t)d1 << 11) | (uint32_t)d2, 0);
    const int d3 = nuc_cross(S, S.cnt, S.mass, asc, bc, bm, crossed);
    key = ((uint32_t)d1 << 21) | ((uint32_t)d2 << 10) | (uint32_t)d3;
    gc = S.grp_cnt;
    gm = S.grp_mass;
    return true;
}

// Among the member tokens of key `key` (level-0 bin binA): the id at rank `rank` (0-based) in ascending / descending id order.
__device__ int nuc_select_id(NucShared& S, const uint32_t* keys, const uint16_t* bins, int V, const NucSel& z, float smax, int binA,
                             uint32_t key, bool asc, unsigned int rank) {
    unsigned int bc = 0;
    u64 bm = 0;
    auto by_rank = [rank](unsigned int c, u64) { return c > rank; };
    nuc_hist(S, keys, bins, V, z, smax, 4, binA, key, 0);
    const int hi = nuc_cross(S, S.cnt, S.mass, asc, bc, bm, by_rank);
    nuc_hist(S, keys, bins, V, z, smax, 5, binA, key, hi);
    const int low = nuc_cross(S, S.cnt, S.mass, asc, bc, bm, by_rank);
    return (hi << 9) | low;
}

// The level-0 histogram after `dc` tokens / `dm` mass have left from the bottom of the order, the last of them inside bin
// binA (c_bin / m_bin = what lay in front of that bin).
__device__ void nuc_drop_prefix(NucShared& S, int binA, unsigned int dc, u64 dm, unsigned int c_bin, u64 m_bin) {
    __syncthreads();
    for (int i = threadIdx.x; i < binA; i += SAMP_FT) { S.cnt0[i] = 0; S.mass0[i] = 0; }
    if (threadIdx.x == 0) { S.cnt0[binA] -= dc - c_bin; S.mass0[binA] -= dm - m_bin; }
    __syncthreads();
}

// ---- probability floors (mtts.h: MttsSamplerFloors) on the full-vocabulary path.  A floor is a mass per token, so the
// cut is a key threshold: the smallest key whose expf(score - smax) reaches `thr` (never above the maximum's own key,
// which stays whatever the floor says); every member below it leaves.
// ktop: the key of the kept set's top, fkey(smax) until typical_p has cut from above.
__device__ __forceinline__ uint32_t nuc_floor_key(double thr, float smax, uint32_t ktop) {
    uint32_t lo = 0x00800000u /* fkey(-FLT_MAX) */, hi = ktop;
    while (lo < hi) {                                       // smallest key in [lo, hi] that stays; hi always does
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if ((double)expf(unfkey(mid) - smax) < thr) lo = mid + 1; else hi = mid;
    }
    return lo;
}
// The members of `z` below key `kthr` leave: z, n, tot and the level-0 histogram afterwards describe the survivors.
__device__ void nuc_floor_cut(NucShared& S, const uint32_t* __restrict__ keys, const uint16_t* __restrict__ bins, int V, NucSel& z,
                              float smax, uint32_t kthr, unsigned int& n, u64& tot) {
    // bins ascend with the score: those below binA leave whole (a threshold under the binned window lies in bin 0)
    const int binA = kthr < fkey(smax - 32.0f) ? 0 : nuc_bin(kthr, smax - 32.0f);
    __syncthreads();
    if (threadIdx.x == 0) { S.out_cnt = 0; S.out_mass = 0; S.grp_cnt = 0; S.grp_mass = 0; }
    __syncthreads();
    for (int i = threadIdx.x; i < binA; i += SAMP_FT)
        if (S.cnt0[i]) { atomicAdd(&S.out_cnt, S.cnt0[i]); atomicAdd(&S.out_mass, S.mass0[i]); }
    nuc_scan_bin(bins, V, binA, [&](int i) {
        const uint32_t key = keys[i];
        if (nuc_in(z, key, i) && key < kthr) { atomicAdd(&S.grp_cnt, 1u); atomicAdd(&S.grp_mass, nuc_q(key, smax)); }
    });
    __syncthreads();
    const unsigned int c_bin = S.out_cnt, dc = c_bin + S.grp_cnt;
    const u64 m_bin = S.out_mass, dm = m_bin + S.grp_mass;
    if (dc == 0) return;                                    // (uniform: every thread read the same totals)
    z.kmin = max(z.kmin, kthr);                             // (a top-p group that was partly dropped lies below kthr or stays as it is)
    n -= dc;
    tot -= dm;
    nuc_drop_prefix(S, binA, dc, dm, c_bin, m_bin);
}
// sum over the members of exp(s - smax) * (s - smax), for the entropy of eta_cutoff: one pass over the row's keys, four
// loads in flight; per-thread fp64 sums in index order, then lanes and waves in a fixed order (run-to-run identical)
__device__ double nuc_entropy_sum(NucShared& S, const uint32_t* __restrict__ keys, int V, const NucSel& z, float smax) {
    double loc = 0.0;
    for (int i0 = threadIdx.x; i0 < V; i0 += SAMP_FT * 4) {
        uint32_t k[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) { const int i = i0 + u * SAMP_FT; k[u] = i < V ? keys[i] : 0u; }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int i = i0 + u * SAMP_FT;
            if (i < V && nuc_in(z, k[u], i)) {
                const float d = unfkey(k[u]) - smax;
                loc += (double)expf(d) * (double)d;
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) loc += __shfl_xor(loc, o, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) S.wm[threadIdx.x >> 6] = (u64)__double_as_longlong(loc);
    __syncthreads();
    double sum = 0.0;
    for (int w = 0; w < SAMP_FT / 64; ++w) sum += __longlong_as_double((long long)S.wm[w]);
    __syncthreads();
    return sum;
}

// ---- typical_p on the full-vocabulary path (typ_shift_bits above: the rule and the shift both paths use)
// f(key, id) for every member of `z`, the row's keys spread over the block's threads, four loads in flight
template <typename F>
__device__ __forceinline__ void nuc_each_member(const uint32_t* __restrict__ keys, int V, const NucSel& z, F f) {
    for (int i0 = threadIdx.x; i0 < V; i0 += SAMP_FT * 4) {
        uint32_t k[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) { const int i = i0 + u * SAMP_FT; k[u] = i < V ? keys[i] : 0u; }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int i = i0 + u * SAMP_FT;
            if (i < V && nuc_in(z, k[u], i)) f(k[u], i);
        }
    }
}
// The members of `z` above key `kceil` leave: the mirror image of nuc_floor_cut.
__device__ void nuc_ceil_cut(NucShared& S, const uint32_t* __restrict__ keys, const uint16_t* __restrict__ bins, int V, NucSel& z,
                             float smax, uint32_t kceil, unsigned int& n, u64& tot) {
    const int binB = kceil < fkey(smax - 32.0f) ? 0 : nuc_bin(kceil, smax - 32.0f);      // the bins above it leave whole
    __syncthreads();
    if (threadIdx.x == 0) { S.out_cnt = 0; S.out_mass = 0; S.grp_cnt = 0; S.grp_mass = 0; }
    __syncthreads();
    for (int i = binB + 1 + threadIdx.x; i < NUC_BINS; i += SAMP_FT)
        if (S.cnt0[i]) { atomicAdd(&S.out_cnt, S.cnt0[i]); atomicAdd(&S.out_mass, S.mass0[i]); }
    nuc_scan_bin(bins, V, binB, [&](int i) {
        const uint32_t key = keys[i];
        if (nuc_in(z, key, i) && key > kceil) { atomicAdd(&S.grp_cnt, 1u); atomicAdd(&S.grp_mass, nuc_q(key, smax)); }
    });
    __syncthreads();
    const unsigned int gc = S.grp_cnt, dc = S.out_cnt + gc;
    const u64 gm = S.grp_mass, dm = S.out_mass + gm;
    z.kmax = min(z.kmax, kceil);
    if (dc == 0) return;                                    // (uniform: every thread read the same totals)
    n -= dc;
    tot -= dm;
    __syncthreads();
    for (int i = binB + 1 + threadIdx.x; i < NUC_BINS; i += SAMP_FT) { S.cnt0[i] = 0; S.mass0[i] = 0; }
    if (threadIdx.x == 0) { S.cnt0[binB] -= gc; S.mass0[binB] -= gm; }
    __syncthreads();
}
// the largest key among the members: the top of the kept set once typical_p has cut from above
__device__ uint32_t nuc_top_key(NucShared& S, const uint32_t* __restrict__ keys, int V, const NucSel& z) {
    uint32_t m = 0;
    nuc_each_member(keys, V, z, [&](uint32_t key, int) { m = max(m, key); });
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, o, 64));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) S.wc[threadIdx.x >> 6] = m;
    __syncthreads();
    uint32_t r = 0;
    for (int w = 0; w < SAMP_FT / 64; ++w) r = max(r, S.wc[w]);
    __syncthreads();
    return r;
}
__device__ __forceinline__ int typ_lin_bin(uint32_t sb) { return (int)fminf(__uint_as_float(sb) * 64.0f, (float)(NUC_BINS - 1)); }
// t* is a selection by mass in ascending shift order, and the shift is a function of the key once dc is known: the count-
// and-mass radix selection of this path on a derived key -- a linear binning of the shift (monotone in it, so the order by
// (bin, shift bits) is the order by shift), then the three digits (11 | 11 | 10 bits) of the shift's bit pattern inside
// the crossing bin.  Masses stay nuc_q of the SCORE key: exact integers, order-free.  One pass over the row's keys per
// level and one for the mean.  The kept keys are then the interval [klo, khi] around the crossing, found without memory
// traffic by bisection on the key; what lies below and above it leaves through nuc_floor_cut / nuc_ceil_cut.
__device__ void nuc_typical_cut(NucShared& S, const uint32_t* __restrict__ keys, const uint16_t* __restrict__ bins, int V, NucSel& z,
                                float smax, float typ, unsigned int& n, u64& tot) {
    const double dc = nuc_entropy_sum(S, keys, V, z, smax) / ((double)tot / NUC_SCALE);
    const double need = (double)typ * (double)tot;
    auto reached = [need](unsigned int, u64 m) { return (double)m >= need; };
    unsigned int bc = 0;
    u64 bm = 0;
    int binT = 0;
    uint32_t prefix = 0, tb = 0x7f800000u;                  // (no crossing, which the exact masses rule out: everything stays)
    for (int level = 0; level < 4; ++level) {
        for (int i = threadIdx.x; i < NUC_BINS; i += SAMP_FT) { S.cnt[i] = 0; S.mass[i] = 0; }
        __syncthreads();
        nuc_each_member(keys, V, z, [&](uint32_t key, int) {
            const uint32_t sb = typ_shift_bits(unfkey(key) - smax, dc);
            int d = typ_lin_bin(sb);
            if (level > 0) {
                if (d != binT) return;
                if (level == 1) d = sb >> 21;
                else if (level == 2) { if ((sb >> 21) != prefix) return; d = (sb >> 10) & 2047; }
                else { if ((sb >> 10) != prefix) return; d = sb & 1023; }
            }
            atomicAdd(&S.cnt[d], 1u);
            atomicAdd(&S.mass[d], nuc_q(key, smax));
        });
        __syncthreads();
        const int dg = nuc_cross(S, S.cnt, S.mass, true, bc, bm, reached);
        if (dg < 0) break;                                  // (uniform)
        if (level == 0) binT = dg;
        else if (level == 1) prefix = (uint32_t)dg;
        else if (level == 2) prefix = (prefix << 11) | (uint32_t)dg;
        else tb = (prefix << 10) | (uint32_t)dg;
    }
    const uint32_t kbot = 0x00800000u /* fkey(-FLT_MAX) */, ktop = fkey(smax);
    auto below = [&](uint32_t key) { return (double)(unfkey(key) - smax) <= dc; };
    auto in = [&](uint32_t key) { return typ_shift_bits(unfkey(key) - smax, dc) <= tb; };
    uint32_t lo = kbot, hi = ktop;                          // kc: the largest key at or below the crossing (kbot is)
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo + 1) >> 1);
        if (below(mid)) lo = mid; else hi = mid - 1;
    }
    const uint32_t kc = lo;
    uint32_t klo = kc + 1, khi = kc;                        // the shift falls over [kbot, kc] and rises over (kc, ktop]
    if (in(kc)) {
        lo = kbot; hi = kc;
        while (lo < hi) {
            const uint32_t mid = lo + ((hi - lo) >> 1);
            if (in(mid)) hi = mid; else lo = mid + 1;
        }
        klo = lo;
    }
    if (kc < ktop && in(kc + 1)) {
        lo = kc + 1; hi = ktop;
        while (lo < hi) {
            const uint32_t mid = lo + ((hi - lo + 1) >> 1);
            if (in(mid)) lo = mid; else hi = mid - 1;
        }
        khi = lo;
    }
    nuc_floor_cut(S, keys, bins, V, z, smax, klo, n, tot);
    nuc_ceil_cut(S, keys, bins, V, z, smax, khi, n, tot);
}

// The body of sample_full_kernel<FL> (TY false) and of sample_full_typ_kernel (TY: typical_p per channel in `typical`,
// 0 = absent; `floors` may then be null).
template <bool FL, bool TY>
__device__ __forceinline__ void sample_full_body(
    const uint16_t* __restrict__ logits0, int V0, const uint32_t* __restrict__ bitmaps, int bm_words,
    const MttsSamplerCfg* __restrict__ cfgs, const LoopState* __restrict__ ls, const SeqState* __restrict__ seqs,
    uint64_t seed, int32_t* __restrict__ decisions, const SampleScratch& sc, int full_cap, int emit_lp, int single_vocab, int single_mask,
    int single_step, int single_channel, const MttsSamplerFloors* __restrict__ floors, const float* __restrict__ typical) {
    __shared__ NucShared S;
    __shared__ float shf[SAMP_FT / 64];
    __shared__ int shi[SAMP_FT / 64];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int flag = sc.overflow[b];
    if (!flag) return;
    SampleCtx x;
    if (!sample_ctx(x, b, 0, logits0, nullptr, V0, 0, 0, bitmaps, bm_words, cfgs, ls, seqs, single_vocab, single_mask,
                    single_step, single_channel, sc.ban, sc.bias_w, sc.bias_t, sc.ext)) return;
    const MttsSamplerCfg cfg = cfgs[x.c];
    uint16_t* bins = (uint16_t*)(sc.full_val + (size_t)b * full_cap);  // level-0 bin of every token (0xffff: -inf)
    uint32_t* keys = (uint32_t*)(sc.full_idx + (size_t)b * full_cap);  // order-preserving key of every processed score
    float bv = -INFINITY; int bi = 0x7fffffff;
    if (tid < SAMP_NS) { bv = sc.slice_val[b * SAMP_NS + tid]; bi = sc.slice_idx[b * SAMP_NS + tid]; }
    block_argmax(bv, bi, shf, shi);
    const float smax = bv;
    const float lo = smax - 32.0f;
    const int V = x.V;
    // ---- level-0 histogram: left by the collect kernel's 32 blocks per row (flag 2), or built here (a row that overflowed
    // the candidate buffer although its top_k fits: many tokens tie with the k-th score)
    if (flag == 2) {
        unsigned int* gc_ = sc.nuc_cnt + (size_t)b * NUC_BINS;
        u64* gm_ = sc.nuc_mass + (size_t)b * NUC_BINS;
        for (int i = tid; i < NUC_BINS; i += SAMP_FT) { S.cnt0[i] = gc_[i]; S.mass0[i] = gm_[i]; gc_[i] = 0; gm_[i] = 0; }
        __syncthreads();
    } else {
        for (int i = tid; i < NUC_BINS; i += SAMP_FT) { S.cnt0[i] = 0; S.mass0[i] = 0; }
        __syncthreads();
        nuc_pass_a(x, smax, lo, keys, bins, S.cnt0, S.mass0, tid, V, SAMP_FT);
        __syncthreads();
    }
    if (tid < 8 && V + tid < ((V + 7) & ~7)) bins[V + tid] = 0xffffu;   // the digit passes read the bins 8 at a time
    __syncthreads();
    unsigned int n = 0;
    u64 tot = 0;
    {
        unsigned int bc = 0; u64 bm = 0;
        auto never = [](unsigned int, u64) { return false; };
        (void)nuc_cross(S, S.cnt0, S.mass0, true, bc, bm, never);      // no crossing: the walk's per-wave sums are the totals
        for (int w = 0; w < SAMP_FT / 64; ++w) { n += S.wc[w]; tot += S.wm[w]; }
        __syncthreads();
    }
    int pick = bi;          // n == 0 (every token banned: all keys are -inf's): the argmax of a row of -inf, token 0, lp NaN
    if (n > 0) {
        NucSel z{0u, 0u, 0};
        int binA; unsigned int c_bin; u64 m_bin;
        // ---- top-k (HF TopKLogitsWarper): scores below the k-th largest go; ties with it stay
        if (cfg.top_k > 0 && (unsigned int)cfg.top_k < n) {
            const unsigned int idx0 = n - (unsigned int)cfg.top_k;       // ascending position of the k-th largest
            unsigned int bc = 0, gc; u64 bm = 0, gm; uint32_t kk;
            auto at = [idx0](unsigned int c, u64) { return c > idx0; };
            nuc_select_key(S, keys, bins, V, z, smax, true, bc, bm, at, kk, gc, gm, binA, c_bin, m_bin);
            z.kmin = kk;
            n -= bc;                                        // everything in front of the threshold's group is dropped
            tot -= bm;
            nuc_drop_prefix(S, binA, bc, bm, c_bin, m_bin);
        }
        // ---- top-p (HF TopPLogitsWarper): longest ascending prefix with cumulative softmax <= 1 - top_p goes
        if (cfg.top_p > 0.f && cfg.top_p < 1.0f) {
            const double dtot = (double)tot;
            const float omp = cfg.one_minus_top_p;
            auto beyond = [dtot, omp](unsigned int, u64 m) { return !((float)((double)m / dtot) <= omp); };
            unsigned int bc = 0, gc; u64 bm = 0, gm; uint32_t kp;
            if (nuc_select_key(S, keys, bins, V, z, smax, true, bc, bm, beyond, kp, gc, gm, binA, c_bin, m_bin)) {
                // tokens of equal score leave in ascending id order: t of the group's gc go (t < gc: the group crosses)
                const u64 q = gm / gc;
                unsigned int t = 0, hi = gc;                // largest t with cum(bm + t q) <= 1 - p
                while (t < hi) {
                    const unsigned int mid = (t + hi + 1) >> 1;
                    if (!beyond(0u, bm + (u64)mid * q)) t = mid; else hi = mid - 1;
                }
                int idp = 0;
                if (t > 0) idp = nuc_select_id(S, keys, bins, V, z, smax, binA, kp, true, t);      // the (t+1)-th smallest id stays
                z.kp = kp;
                z.idp = idp;
                n -= bc + t;
                tot -= bm + (u64)t * q;
                nuc_drop_prefix(S, binA, bc + t, bm + (u64)t * q, c_bin, m_bin);
            }
        }
        // ---- probability floors (HF MinP / Epsilon / EtaLogitsWarper), each on the survivors of the stage before it
        if constexpr (FL) {
            MttsSamplerFloors fl{0.f, 0.f, 0.f, 0.f};
            if (!TY || floors) fl = floors[x.c];
            uint32_t ktop = fkey(smax);
            // as a mass per token: p_i < floor  <=>  exp(s_i - smax) < floor * total  (p_max = 1 / total)
            if (fl.min_p > 0.f) nuc_floor_cut(S, keys, bins, V, z, smax, nuc_floor_key((double)fl.min_p, smax, ktop), n, tot);
            if constexpr (TY) {
                const float typ = typical[x.c];
                if (typ > 0.f) {
                    nuc_typical_cut(S, keys, bins, V, z, smax, typ, n, tot);
                    // the floors that follow never drop a token at the maximum of what is left
                    if (fl.epsilon_cutoff > 0.f || fl.eta_cutoff > 0.f) ktop = nuc_top_key(S, keys, V, z);
                }
            }
            if (fl.epsilon_cutoff > 0.f)
                nuc_floor_cut(S, keys, bins, V, z, smax, nuc_floor_key((double)fl.epsilon_cutoff * ((double)tot / NUC_SCALE), smax, ktop), n, tot);
            if (fl.eta_cutoff > 0.f) {
                const double t = (double)tot / NUC_SCALE;
                const double H = log(t) - nuc_entropy_sum(S, keys, V, z, smax) / t;
                const double eta = fmin((double)fl.eta_cutoff, (double)fl.sqrt_eta_cutoff * exp(-H));
                nuc_floor_cut(S, keys, bins, V, z, smax, nuc_floor_key(eta * t, smax, ktop), n, tot);
            }
        }
        // ---- draw: walk the kept tokens from the top; the first whose running mass exceeds u * total
        uint32_t rnd[4];
        const uint64_t sd = single_vocab > 0 ? seed : x.seed;
        philox4x32_10((uint32_t)x.step, x.row_id, (uint32_t)x.c, 0u, (uint32_t)sd, (uint32_t)(sd >> 32), rnd);
        const double u = (double)((float)(rnd[0] >> 8) * (1.0f / 16777216.0f));
        const double target = u * ((double)tot / NUC_SCALE);
        auto past = [target](unsigned int, u64 m) { return (double)m / NUC_SCALE > target; };
        unsigned int bc = 0, gc; u64 bm = 0, gm; uint32_t kd;
        if (nuc_select_key(S, keys, bins, V, z, smax, false, bc, bm, past, kd, gc, gm, binA, c_bin, m_bin)) {
            const u64 q = gm / gc;
            unsigned int j = 1, hi = gc;                    // smallest j with mass(bm + j q) past the target (ties: higher id first)
            while (j < hi) {
                const unsigned int mid = (j + hi) >> 1;
                if (past(0u, bm + (u64)mid * q)) hi = mid; else j = mid + 1;
            }
            pick = nuc_select_id(S, keys, bins, V, z, smax, binA, kd, false, j - 1);
        }
    }
    if (tid == 0) {
        decisions[b * 8 + x.c] = pick;
        sc.overflow[b] = 0;
        // output_scores: the pick's own score over the exact integer mass of the kept set (the pick's quantised mass would
        // carry only a few significant bits for an unlikely token)
        if (emit_lp)
            sc.lp[b * 8 + x.c] = n > 0 ? (float)((double)(unfkey(keys[pick]) - smax) - log((double)tot / NUC_SCALE))
                                       : __uint_as_float(0x7fc00000u);
    }
}
template <bool FL>
__global__ __launch_bounds__(SAMP_FT) void sample_full_kernel(
    const uint16_t* __restrict__ logits0, int V0, const uint32_t* __restrict__ bitmaps, int bm_words,
    const MttsSamplerCfg* __restrict__ cfgs, const LoopState* __restrict__ ls, const SeqState* __restrict__ seqs,
    uint64_t seed, int32_t* __restrict__ decisions, SampleScratch sc, int full_cap, int emit_lp, int single_vocab, int single_mask,
    int single_step, int single_channel, const MttsSamplerFloors* __restrict__ floors) {
    sample_full_body<FL, false>(logits0, V0, bitmaps, bm_words, cfgs, ls, seqs, seed, decisions, sc, full_cap, emit_lp, single_vocab,
                                single_mask, single_step, single_channel, floors, nullptr);
}
__global__ __launch_bounds__(SAMP_FT) void sample_full_typ_kernel(
    const uint16_t* __restrict__ logits0, int V0, const uint32_t* __restrict__ bitmaps, int bm_words,
    const MttsSamplerCfg* __restrict__ cfgs, const LoopState* __restrict__ ls, const SeqState* __restrict__ seqs,
    uint64_t seed, int32_t* __restrict__ decisions, SampleScratch sc, int full_cap, int emit_lp, int single_vocab, int single_mask,
    int single_step, int single_channel, const MttsSamplerFloors* __restrict__ floors, const float* __restrict__ typical) {
    sample_full_body<true, true>(logits0, V0, bitmaps, bm_words, cfgs, ls, seqs, seed, decisions, sc, full_cap, emit_lp, single_vocab,
                                 single_mask, single_step, single_channel, floors, typical);
}

// One block; thread b handles sequence slot b.  Restates modeling_asteroid.py:139-169 with a per-dialogue clock.
// gen / dec_log / forced: [slot][gen_cap][8]; tf_tail: [slot][7][8] = tf_inputs[:, base_length + s, :].
// GT (generate(top_logprobs=k)): gen_topk.hip has written this step's row of gt.logp / gt.ids / gt.tlp for every evaluated
// dialogue; this instantiation puts NaN / -1 over the slots that are not decisions.  The plain one does not look at `gt`.
template <bool GT>
__global__ void update_kernel(const int32_t* __restrict__ decisions, int32_t* __restrict__ dec_log,
                              const int32_t* __restrict__ forced, const int32_t* __restrict__ tf_tail,
                              int32_t* __restrict__ gen, int32_t* __restrict__ cur_tokens,
                              SeqState* __restrict__ seqs, RowMeta* __restrict__ meta, uint32_t* __restrict__ bitmaps,
                              int bm_words, LoopState* __restrict__ ls, int eos, int spad, int sp_lo, int sp_hi,
                              const float* __restrict__ lp_in, float* __restrict__ lp_out, GenTopkOut gt) {
    __shared__ int any_unfinished;
    if (ls->done) return;
    const int b = threadIdx.x, B = ls->B;
    const int cap = ls->gen_cap;
    if (b == 0) any_unfinished = 0;
    __syncthreads();
    if (b < B) {
        SeqState s = seqs[b];
        if (!s.active || s.step >= cap) {
            meta[b].seq = -1;
            if (s.active && s.step >= cap) { s.active = 0; s.unfinished = 0; seqs[b] = s; }
        } else {
            const int step = s.step;
            int tok[8];
            // The reference evaluates EVERY row of a static batch at every step (finished ones too) and tests their
            // channel-0 pick for "not a speech token" (:140-141) before it overwrites the row with padding (:155-158).
            // A row that was finished by max_length (needs_additional_steps still -1) is thereby resurrected for a
            // 7-step flush as soon as its pick is a non-speech token (`unfinished | nas > 0`, :168), while the rest of
            // the batch is still running.  Such rows are kept in the forward pass (active == 2); rows finished by EOS
            // have nas == 0, can never come back, and are skipped for good.
            const bool linger = s.active == 2;
#pragma unroll
            for (int c = 0; c < 8; ++c) tok[c] = (s.unfinished || linger) ? decisions[b * 8 + c] : 0;
            const size_t slot = ((size_t)b * cap + step) * 8;
            const bool as_draw = forced && ls->forced_draw;
            if (as_draw) {          // the log keeps the raw draws; the reference's history drives the state machine
                // (mode 2, tests of chained resurrections: the forced row is also the raw draw of a cut-off row that
                //  the reference keeps evaluating -- a real reference run does not record those draws)
                const bool take = s.unfinished != 0 || (linger && ls->forced_draw == 2);
#pragma unroll
                for (int c = 0; c < 8; ++c) {
                    dec_log[slot + c] = tok[c];
                    const int f = forced[slot + c];
                    if (f >= 0 && take) tok[c] = f;
                }
            }
            // :140-141
            const bool speech = tok[0] >= sp_lo && tok[0] < sp_hi;
            if ((s.unfinished || linger) && !speech && s.nas < 0) s.nas = 7;
            // :143-145 teacher forcing of the delayed prompt tail (first 7 steps)
            if (step < 7) {
#pragma unroll
                for (int c = 0; c < 8; ++c)
                    if (c >= step + 1) tok[c] = tf_tail[(b * 7 + step) * 8 + c];
            }
            // :148-153 EOS flush
            if (s.nas > 0 && s.nas < 7) {
                tok[0] = eos;
#pragma unroll
                for (int c = 1; c < 8; ++c)
                    if (s.nas < 8 - c) tok[c] = spad;
            }
            // :155-158 finished rows
            if (!s.unfinished) {
                tok[0] = eos;
#pragma unroll
                for (int c = 1; c < 8; ++c) tok[c] = spad;
            }
            // output_scores (lp_out [slot][gen_cap][8], laid out like gen): the sampler's log-probability where the appended
            // token is the model's decision, NaN where teacher forcing, the EOS flush or finished-row padding replaced it.
            // The rule is the one applied to tok[] above; the replay hook (forced) has no part in it.
            const bool flush = s.nas > 0 && s.nas < 7;
            auto used = [&](int c) { return s.unfinished && !(step < 7 && c >= step + 1) && !(flush && (c == 0 || s.nas < 8 - c)); };
            if (lp_out) {
#pragma unroll
                for (int c = 0; c < 8; ++c) lp_out[slot + c] = used(c) ? lp_in[b * 8 + c] : __uint_as_float(0x7fc00000u);
            }
            // top_logprobs ([slot][gen_cap][8] and [slot][gen_cap][8][k]): the same rule.  Only an evaluated row has values to
            // cover (the buffers start as NaN / -1), and on most steps every slot of it is a decision: nothing to do
            if constexpr (GT) {
                if (s.unfinished || linger) {
#pragma unroll
                    for (int c = 0; c < 8; ++c)
                        if (!used(c)) {
                            gt.logp[slot + c] = __uint_as_float(0x7fc00000u);
                            for (int j = 0; j < gt.k; ++j) {
                                gt.ids[(slot + c) * gt.k + j] = -1;
                                gt.tlp[(slot + c) * gt.k + j] = __uint_as_float(0x7fc00000u);
                            }
                        }
                }
            }
            if (dec_log && !as_draw) {
#pragma unroll
                for (int c = 0; c < 8; ++c) dec_log[slot + c] = tok[c];
            }
            if (forced && !as_draw) {
#pragma unroll
                for (int c = 0; c < 8; ++c) {
                    int f = forced[slot + c];
                    if (f >= 0) tok[c] = f;
                }
            }
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                gen[slot + c] = tok[c];
                cur_tokens[b * 8 + c] = tok[c];
                uint32_t* bm = bitmaps + ((size_t)b * 8 + c) * bm_words;
                bm[tok[c] >> 5] |= 1u << (tok[c] & 31);       // history for the repetition penalty
            }
            // :165-168
            if (s.nas > 0) s.nas -= 1;
            const int new_len = s.base_length + step + 1;
            const bool stopping = (new_len >= s.max_length) || (tok[0] == eos) || (s.nas == 0);
            s.unfinished = (s.unfinished && !stopping) ? 1 : 0;
            if (s.nas > 0) s.unfinished = 1;
            s.step = step + 1;
            if (ls->continuous) {
                if (!s.unfinished) s.active = 0;                     // scheduler mode: the slot is free again
            } else {
                s.active = (!s.unfinished && s.nas < 0) ? 2 : 1;     // static batch: finished at max_length, may come back
            }
            // the forward that follows appends this token to the cache at position kv_len
            meta[b].seq = (s.unfinished || s.active == 2) ? b : -1;
            meta[b].pos = s.kv_len;
            meta[b].last = 1;
            s.kv_len += 1;
            seqs[b] = s;
            if (s.unfinished) atomicOr(&any_unfinished, 1);
        }
    }
    __syncthreads();
    if (b == 0) {
        ls->step = ls->step + 1;
        if (!any_unfinished) ls->done = 1;
    }
}

// ---------------------------------------------------------------------------------------------------------------
// The split step (mtts_step_begin / mtts_step_sample / mtts_step_finish): generate(logits_processor=, stopping_criteria=,
// streamer=).  The step pauses between the heads and the sampler: scores_materialize_kernel hands the caller the rows HF's
// built-in processors leave (reference modeling_asteroid.py:123-129 up to the caller's own list), the sampler kernels above
// then run on what the caller made of them (SampleScratch::ext), step_tokens_kernel shows the appended tokens, and
// stop_rows_kernel applies the caller's stopping criteria (:166-168).
//
// scores_materialize_kernel: grid (8, B) (the unit-test entry: (1, rows)), the gate of the sampler (sample_ctx).  The value
// of token i is proc_score with x.temp = 0 -- the function every sampler pass reads through, so the row cannot drift from
// what the unsplit step samples from; the sampler's only operation left on it is the division by the temperature, on the
// same fp32 value.  Four tokens per thread and store: 16-byte vector stores, no atomics; the row's pad columns get -inf.
#define MAT_T 256
__global__ __launch_bounds__(MAT_T) void scores_materialize_kernel(
    const uint16_t* __restrict__ logits0, const uint16_t* __restrict__ logits17, int V0, int Vs, int Vs_pad,
    const uint32_t* __restrict__ bitmaps, int bm_words, const MttsSamplerCfg* __restrict__ cfgs, const LoopState* __restrict__ ls,
    const SeqState* __restrict__ seqs, SampleScratch sc, float* __restrict__ out0, float* __restrict__ out17, int single_vocab,
    int single_mask, int single_step, int single_channel) {
    const int b = blockIdx.y, tid = threadIdx.x;
    SampleCtx x;
    if (!sample_ctx(x, b, blockIdx.x, logits0, logits17, V0, Vs, Vs_pad, bitmaps, bm_words, cfgs, ls, seqs, single_vocab, single_mask,
                    single_step, single_channel, sc.ban, sc.bias_w, sc.bias_t)) return;
    x.temp = 0.f;
    float* out;
    int ld;                            // the row's length with its padding: a multiple of 32, so every 16-byte store stays inside
    if (single_vocab > 0) { ld = (x.V + 31) & ~31; out = out0 + (size_t)b * ld; }
    else if (x.c == 0) { ld = (V0 + 31) & ~31; out = out0 + (size_t)b * ld; }
    else { ld = Vs_pad; out = out17 + ((size_t)b * 7 + (x.c - 1)) * Vs_pad; }
    for (int i = tid * 4; i < ld; i += MAT_T * 4) {
        f32x4_t v;
        v.x = i < x.V ? proc_score(x, i) : -INFINITY;
        v.y = i + 1 < x.V ? proc_score(x, i + 1) : -INFINITY;
        v.z = i + 2 < x.V ? proc_score(x, i + 2) : -INFINITY;
        v.w = i + 3 < x.V ? proc_score(x, i + 3) : -INFINITY;
        *(f32x4_t*)(out + i) = v;
    }
}
void launch_scores_materialize(const void* logits0, const void* logits17, int V0, int Vs, int Vs_pad, const uint32_t* bitmaps, int bm_words,
                               const MttsSamplerCfg* cfgs, const LoopState* ls, const SeqState* seqs, int B, const SampleScratch& sc,
                               float* out0, float* out17, hipStream_t st) {
    hipLaunchKernelGGL(scores_materialize_kernel, dim3(8, B), dim3(MAT_T), 0, st, (const uint16_t*)logits0, (const uint16_t*)logits17, V0, Vs,
                       Vs_pad, bitmaps, bm_words, cfgs, ls, seqs, sc, out0, out17, 0, 0, 0, 0);
}
void launch_scores_materialize_single(const void* logits, int rows, int vocab, const uint32_t* bitmap, int bm_words, const MttsSamplerCfg* cfgs8,
                                      int mask_id, int step, int channel, const SampleScratch& sc, float* out, hipStream_t st) {
    hipLaunchKernelGGL(scores_materialize_kernel, dim3(1, rows), dim3(MAT_T), 0, st, (const uint16_t*)logits, (const uint16_t*)nullptr, vocab,
                       vocab, vocab, bitmap, bm_words, cfgs8, (const LoopState*)nullptr, (const SeqState*)nullptr, sc, out, (float*)nullptr,
                       vocab, mask_id, step, channel);
}

// One block; thread b handles sequence slot b: the tokens update_kernel has just appended, widened for a LongTensor.
__global__ void step_tokens_kernel(const int32_t* __restrict__ cur_tokens, int64_t* __restrict__ tokens, const LoopState* __restrict__ ls) {
    const int b = threadIdx.x;
    if (b >= ls->B) return;
#pragma unroll
    for (int c = 0; c < 8; ++c) tokens[b * 8 + c] = (int64_t)cur_tokens[b * 8 + c];
}
void launch_step_tokens(const int32_t* cur_tokens, int64_t* tokens, const LoopState* ls, hipStream_t st) {
    hipLaunchKernelGGL(step_tokens_kernel, dim3(1), dim3(MTTS_RCAP), 0, st, cur_tokens, tokens, ls);
}

// One block; thread b handles sequence slot b, behind update_kernel of the same step.  Reference modeling_asteroid.py:166-168:
// unfinished &= ~stop, then a row with needs_additional_steps > 0 stays unfinished.  update_kernel has applied the built-in
// criteria (max_length, EOS, the end of a flush) already, so what is left is to finish the rows the caller stopped: like a
// row max_length finished, a static batch keeps evaluating it (active == 2; its needs_additional_steps is < 0 here, since a
// row with 0 is finished and one with > 0 is exempt), the scheduler frees its slot.
__global__ void stop_rows_kernel(const StopMask stop, SeqState* __restrict__ seqs, RowMeta* __restrict__ meta,
                                 LoopState* __restrict__ ls) {
    __shared__ int any_unfinished;
    if (ls->done) return;
    const int b = threadIdx.x, B = ls->B;
    if (b == 0) any_unfinished = 0;
    __syncthreads();
    if (b < B) {
        SeqState s = seqs[b];
        if (s.active && s.unfinished && stop.row[b] && s.nas <= 0) {
            s.unfinished = 0;
            s.active = ls->continuous ? 0 : 2;
            meta[b].seq = s.active == 2 ? b : -1;
            seqs[b] = s;
        }
        if (s.active && s.unfinished) atomicOr(&any_unfinished, 1);
    }
    __syncthreads();
    if (b == 0 && !any_unfinished) ls->done = 1;
}
void launch_stop_rows(const StopMask& stop, SeqState* seqs, RowMeta* meta, LoopState* ls, hipStream_t st) {
    hipLaunchKernelGGL(stop_rows_kernel, dim3(1), dim3(MTTS_RCAP), 0, st, stop, seqs, meta, ls);
}

// ---------------------------------------------------------------------------------------------------------------
// Hard bans (mtts_set_sampler_bans; launch.h: launch_ban).  One block per (row, channel) the sampler is about to evaluate
// rewrites that pair's ban words: first the run's static bitmap of the channel (suppress_tokens) with eos while the
// row's step is below min_new_tokens + 7 -- an overwrite, so it is also the per-step clear -- then, behind a barrier, HF's
// NoRepeatNGram rule: the last n-1 tokens of the history are block-uniform (LDS); every thread tests a strided range of
// window starts, leaves a window at its first unequal token, and ORs the follower of a matching one in.  OR is order-free,
// so the words are the same bits run to run.  The history is the prompt's slots (hist, staged by the host) followed by
// the row's generated tokens (gen, appended by update_kernel): the stream that sets bits in the repetition-penalty bitmap.
// single_vocab > 0: the unit-test entry, hist [rows][hist_cap] of one channel with lengths single_lens.
#define BAN_T 256
__global__ __launch_bounds__(BAN_T) void ban_kernel(
    uint32_t* __restrict__ ban, const uint32_t* __restrict__ stat, const uint32_t* __restrict__ begin, int words,
    const BanCfg* __restrict__ cfgs, const int32_t* __restrict__ hist, int hist_cap, const int32_t* __restrict__ gen, int V0, int Vs, int eos,
    const LoopState* __restrict__ ls, const SeqState* __restrict__ seqs, const int32_t* __restrict__ single_lens, int single_vocab) {
    __shared__ int32_t suf[MTTS_NGRAM_MAX];
    const uint32_t* bp = nullptr;       // begin_suppress_tokens of the channel, at its one step
    const int b = blockIdx.y, tid = threadIdx.x;
    int V, base, glen, hs;
    const int32_t *hp, *gp;
    const uint32_t* sp;
    uint32_t* out;
    BanCfg cfg;
    bool eos_on;
    if (single_vocab > 0) {
        V = single_vocab; cfg = cfgs[0];
        base = min(max(single_lens[b], 0), hist_cap); glen = 0; hs = 1;
        hp = hist + (size_t)b * hist_cap; gp = nullptr;
        out = ban + (size_t)b * ((V + 31) >> 5); sp = stat;
        eos_on = cfg.eos_below != 0;
    } else {
        if (ls->done) return;
        const SeqState sq = seqs[b];
        if (!sq.active || !(sq.unfinished || sq.active == 2)) return;       // the rows sample_ctx evaluates
        const int c = blockIdx.x;
        V = c == 0 ? V0 : Vs; cfg = cfgs[c];
        base = sq.base_length; glen = min(sq.step, ls->gen_cap); hs = 8;
        if (base > hist_cap) cfg.ngram = 0;         // (the host refuses such a prompt: nothing past the row is ever read)
        hp = hist + (size_t)b * hist_cap * 8 + c; gp = gen + (size_t)b * ls->gen_cap * 8 + c;
        out = ban + ((size_t)b * 8 + c) * words; sp = stat + (size_t)c * words;
        eos_on = sq.step < cfg.eos_below || base + sq.step < cfg.min_length;         // min_new_tokens; min_length against len(h)
        if (begin && sq.step == 7) bp = begin + (size_t)c * words;                  // len(h) == base + 7, HF's begin_index
    }
    const int nw = (V + 31) >> 5;                   // (<= words; bits at and above V are never set)
    for (int w = tid; w < nw; w += BAN_T) {
        uint32_t v = sp[w];
        if (bp) v |= bp[w];
        if (eos_on && eos >= 0 && eos < V && (eos >> 5) == w) v |= 1u << (eos & 31);
        out[w] = v;
    }
    const int n = cfg.ngram, len = base + glen;
    if (n <= 0 || len < n) return;                  // (block-uniform)
    const auto h = [&](int i) { return i < base ? hp[(size_t)i * hs] : gp[(size_t)(i - base) * hs]; };
    if (tid < n - 1) suf[tid] = h(len - n + 1 + tid);
    __syncthreads();                                // the static words are written, the suffix is in LDS
    for (int j = tid; j <= len - n; j += BAN_T) {
        int k = 0;
        while (k < n - 1 && h(j + k) == suf[k]) ++k;
        if (k == n - 1) {
            const int t = h(j + n - 1);
            if (t >= 0 && t < V) atomicOr(&out[t >> 5], 1u << (t & 31));
        }
    }
}
static long long g_ban_launches = 0;        // launches of ban_kernel (test hook: mtts_debug_ban_launches)
long long mtts_ban_launches() { return g_ban_launches; }
void launch_ban(uint32_t* ban, const uint32_t* stat, const uint32_t* begin, int words, const BanCfg* cfgs, const int32_t* hist, int hist_cap,
                const int32_t* gen, int V0, int Vs, int eos, const LoopState* ls, const SeqState* seqs, int B, hipStream_t st) {
    ++g_ban_launches;
    hipLaunchKernelGGL(ban_kernel, dim3(8, B), dim3(BAN_T), 0, st, ban, stat, begin, words, cfgs, hist, hist_cap, gen, V0, Vs, eos, ls, seqs,
                       (const int32_t*)nullptr, 0);
}
void launch_ban_single(uint32_t* ban, const uint32_t* stat, const BanCfg* cfg1, const int32_t* hist, const int32_t* lens, int rows,
                       int cap, int vocab, int eos, hipStream_t st) {
    ++g_ban_launches;
    hipLaunchKernelGGL(ban_kernel, dim3(1, rows), dim3(BAN_T), 0, st, ban, stat, (const uint32_t*)nullptr, (vocab + 31) >> 5, cfg1, hist, cap,
                       (const int32_t*)nullptr, vocab, vocab, eos, (const LoopState*)nullptr, (const SeqState*)nullptr, lens, vocab);
}

// ---------------------------------------------------------------------------------------------------------------
// Sequence rules (mtts_set_sampler_bias; launch.h: launch_bias), behind ban_kernel in the step graph.  One block per (row,
// channel) the sampler is about to evaluate.  All threads rewrite the pair's bias words from the channel's static words
// (the single-token finite rules, staged by the host) -- an overwrite, so it is also the per-step clear.  Meanwhile lane
// r of the first wave tests rule r: a rule of L > 1 tokens matches when the history holds L tokens (HF skips a rule longer
// than its context) and its last L-1 are the rule's prefix; one of a single token always; the history is indexed as in ban_kernel.  Behind the barrier the same wave ORs the last
// token of every matching -inf rule into the pair's ban words, the bit of every finite hit into its bias words, and builds
// the table: the first hit of a token (in rule order) is its leader, which sums the token's chain -- its own beta, then
// the beta of every later hit of the token, one fp32 addition each, the order in which the host laid the rules out -- and
// writes (id, term) at the rank of its id among the leaders.  One lane per token, a fixed order, no float atomics: words
// and table are the same bits run to run.  OR into the ban words is order-free.
// single_vocab > 0: the unit-test entry, hist [rows][hist_cap] of one channel with lengths single_lens.
#define BIAS_T 256
static_assert(BIAS_RULES == 64 && BIAS_RULES == MTTS_BIAS_RULES_MAX && BIAS_RULE_LEN == MTTS_BIAS_RULE_LEN_MAX, "one rule per lane of a wave");
__global__ __launch_bounds__(BIAS_T) void bias_kernel(
    uint32_t* __restrict__ ban, uint32_t* __restrict__ bias_w, const uint32_t* __restrict__ bias_stat, MttsBiasTable* __restrict__ tabs,
    int words, const BiasRules* __restrict__ rules, const int32_t* __restrict__ hist, int hist_cap, const int32_t* __restrict__ gen,
    int V0, int Vs, const LoopState* __restrict__ ls, const SeqState* __restrict__ seqs, const int32_t* __restrict__ single_lens,
    int single_vocab) {
    __shared__ int32_t s_tok[BIAS_RULES];
    __shared__ float s_beta[BIAS_RULES];
    __shared__ int32_t s_hit[BIAS_RULES];           // 0: no hit, 1: a finite one, 2: a ban
    __shared__ int32_t s_lead[BIAS_RULES];
    const int b = blockIdx.y, tid = threadIdx.x;
    int V, base, glen, hs;
    const int32_t *hp, *gp;
    const uint32_t* sp;
    uint32_t *banw, *outw;
    MttsBiasTable* tab;
    const BiasRules* R;
    if (single_vocab > 0) {
        V = single_vocab; R = rules;
        base = min(max(single_lens[b], 0), hist_cap); glen = 0; hs = 1;
        hp = hist + (size_t)b * hist_cap; gp = nullptr;
        const size_t row = (size_t)b * ((V + 31) >> 5);
        banw = ban ? ban + row : nullptr; outw = bias_w ? bias_w + row : nullptr; sp = bias_stat;
        tab = tabs ? tabs + b : nullptr;
    } else {
        if (ls->done) return;
        const SeqState sq = seqs[b];
        if (!sq.active || !(sq.unfinished || sq.active == 2)) return;       // the rows sample_ctx evaluates
        const int c = blockIdx.x;
        V = c == 0 ? V0 : Vs; R = rules + c;
        base = sq.base_length; glen = min(sq.step, ls->gen_cap); hs = 8;
        hp = hist ? hist + (size_t)b * hist_cap * 8 + c : nullptr; gp = gen + (size_t)b * ls->gen_cap * 8 + c;
        if (base > hist_cap) hp = nullptr;          // (the host refuses such a prompt: nothing past the row is ever read)
        const size_t pair = (size_t)b * 8 + c;
        banw = ban ? ban + pair * words : nullptr; outw = bias_w ? bias_w + pair * words : nullptr;
        sp = bias_stat ? bias_stat + (size_t)c * words : nullptr;
        tab = tabs ? tabs + pair : nullptr;
    }
    const int nw = (V + 31) >> 5;                   // (<= words; bits at and above V are never set)
    if (outw)
        for (int w = tid; w < nw; w += BIAS_T) outw[w] = sp ? sp[w] : 0u;
    const int len = base + glen, nr = min(max(R->n, 0), BIAS_RULES);
    int tok = -1, hit = 0;
    float beta = 0.f;
    if (tid < BIAS_RULES) {
        if (tid < nr) {
            const int L = min(max(R->len[tid], 1), BIAS_RULE_LEN);
            tok = R->ids[tid][L - 1]; beta = R->beta[tid];
            bool m = tok >= 0 && tok < V && (L == 1 || (len >= L && (hp || len - (L - 1) >= base)));
            for (int k = 0; m && k < L - 1; ++k) {
                const int i = len - (L - 1) + k;
                m = (i < base ? hp[(size_t)i * hs] : gp[(size_t)(i - base) * hs]) == R->ids[tid][k];
            }
            if (m) hit = beta == -INFINITY ? 2 : 1;
        }
        s_tok[tid] = tok; s_beta[tid] = beta; s_hit[tid] = hit;
    }
    __syncthreads();                                // the static words are written, the hits are in LDS
    bool lead = false;
    if (tid < BIAS_RULES) {
        if (hit == 2 && banw) atomicOr(&banw[tok >> 5], 1u << (tok & 31));
        if (hit == 1 && outw) {
            atomicOr(&outw[tok >> 5], 1u << (tok & 31));
            lead = true;
            for (int r = 0; r < tid; ++r) lead = lead && !(s_hit[r] == 1 && s_tok[r] == tok);
        }
        s_lead[tid] = lead ? 1 : 0;
    }
    __syncthreads();
    if (tid < BIAS_RULES && tab) {
        if (lead) {
            float term = beta;
            int rank = 0;
            for (int r = 0; r < nr; ++r) {
                if (r > tid && s_hit[r] == 1 && s_tok[r] == tok) term = term + s_beta[r];
                rank += (s_lead[r] && s_tok[r] < tok) ? 1 : 0;
            }
            tab->ids[rank] = tok; tab->term[rank] = term;
        }
        const int n = __popcll(__ballot(lead));
        if (tid == 0) tab->n = n;
    }
}
static long long g_bias_launches = 0;       // launches of bias_kernel (test hook: mtts_debug_bias_launches)
long long mtts_bias_launches() { return g_bias_launches; }
void launch_bias(uint32_t* ban, uint32_t* bias_w, const uint32_t* bias_stat, MttsBiasTable* tabs, int words, const BiasRules* rules,
                 const int32_t* hist, int hist_cap, const int32_t* gen, int V0, int Vs, const LoopState* ls, const SeqState* seqs,
                 int B, hipStream_t st) {
    ++g_bias_launches;
    hipLaunchKernelGGL(bias_kernel, dim3(8, B), dim3(BIAS_T), 0, st, ban, bias_w, bias_stat, tabs, words, rules, hist, hist_cap, gen, V0, Vs,
                       ls, seqs, (const int32_t*)nullptr, 0);
}
void launch_bias_single(uint32_t* ban, uint32_t* bias_w, const uint32_t* bias_stat, MttsBiasTable* tabs, const BiasRules* rules1,
                        const int32_t* hist, const int32_t* lens, int rows, int cap, int vocab, hipStream_t st) {
    ++g_bias_launches;
    hipLaunchKernelGGL(bias_kernel, dim3(1, rows), dim3(BIAS_T), 0, st, ban, bias_w, bias_stat, tabs, (vocab + 31) >> 5, rules1, hist, cap,
                       (const int32_t*)nullptr, vocab, vocab, (const LoopState*)nullptr, (const SeqState*)nullptr, lens, vocab);
}

static SampleScratch g_dummy_scratch;
// emit_lp (output_scores): the LP instantiations of the scan / final kernels; off, the step runs the plain ones.
// floors (mtts_set_sampler_floors; device, 8 entries): the FL instantiations of the final / full kernels; null, the plain ones.
// typical (mtts_set_sampler_typical; device, 8 floats): the *_typ_kernel pair, which takes both tables (floors may be null
// there); null, the launches above, as before typical_p existed.
template <bool LP, bool FL>
static void launch_final(dim3 grid, hipStream_t st, const void* logits0, const void* logits17, int V0, int Vs, int Vs_pad,
                         const uint32_t* bitmaps, int bm_words, const MttsSamplerCfg* cfgs, const LoopState* ls, const SeqState* seqs,
                         uint64_t seed, int32_t* decisions, int32_t* err, const SampleScratch& sc, int big0, int single_vocab,
                         int single_mask, int single_step, int single_channel, const MttsSamplerFloors* floors, const float* typical) {
    if (typical) {
        hipLaunchKernelGGL((sample_final_typ_kernel<LP>), grid, dim3(SAMP_T), 0, st, (const uint16_t*)logits0, (const uint16_t*)logits17,
                           V0, Vs, Vs_pad, bitmaps, bm_words, cfgs, ls, seqs, seed, decisions, err, sc, big0, single_vocab, single_mask,
                           single_step, single_channel, floors, typical);
        return;
    }
    hipLaunchKernelGGL((sample_final_kernel<LP, FL>), grid, dim3(SAMP_T), 0, st, (const uint16_t*)logits0, (const uint16_t*)logits17,
                       V0, Vs, Vs_pad, bitmaps, bm_words, cfgs, ls, seqs, seed, decisions, err, sc, big0, single_vocab, single_mask,
                       single_step, single_channel, floors);
}
#define LAUNCH_FINAL(...)                                                                                              \
    do {                                                                                                               \
        if (floors) { if (emit_lp) launch_final<true, true>(__VA_ARGS__); else launch_final<false, true>(__VA_ARGS__); } \
        else { if (emit_lp) launch_final<true, false>(__VA_ARGS__); else launch_final<false, false>(__VA_ARGS__); }      \
    } while (0)
void launch_sample(const void* logits0, const void* logits17, int V0, int Vs, int Vs_pad, const uint32_t* bitmaps, int bm_words,
                   const MttsSamplerCfg* cfgs, const LoopState* ls, const SeqState* seqs, uint64_t seed, int32_t* decisions,
                   int32_t* err, int B, const SampleScratch& sc, int ch0_sampled, int full_cap, int emit_lp,
                   const MttsSamplerFloors* floors, const float* typical, hipStream_t st) {
    const int big0 = V0 > SAMP_CAND ? 1 : 0;
    if (big0) {
        hipLaunchKernelGGL(emit_lp ? sample_scan_kernel<true> : sample_scan_kernel<false>, dim3(SAMP_NS, B), dim3(SAMP_T), 0, st,
                           (const uint16_t*)logits0, V0, bitmaps, bm_words, cfgs, ls, seqs, sc, 0, 0, 0, 0);
        if (ch0_sampled)
            hipLaunchKernelGGL(sample_collect_kernel, dim3(SAMP_NS, B), dim3(SAMP_T), 0, st, (const uint16_t*)logits0, V0,
                               bitmaps, bm_words, cfgs, ls, seqs, sc, full_cap, 0, 0, 0, 0);
    }
    LAUNCH_FINAL(dim3(8, B), st, logits0, logits17, V0, Vs, Vs_pad, bitmaps, bm_words, cfgs, ls, seqs, seed, decisions, err, sc, big0,
                 0, 0, 0, 0, floors, typical);
    if (big0 && ch0_sampled && typical)
        hipLaunchKernelGGL(sample_full_typ_kernel, dim3(B), dim3(SAMP_FT), 0, st, (const uint16_t*)logits0, V0, bitmaps, bm_words, cfgs,
                           ls, seqs, seed, decisions, sc, full_cap, emit_lp, 0, 0, 0, 0, floors, typical);
    else if (big0 && ch0_sampled)
        hipLaunchKernelGGL(floors ? sample_full_kernel<true> : sample_full_kernel<false>, dim3(B), dim3(SAMP_FT), 0, st,
                           (const uint16_t*)logits0, V0, bitmaps, bm_words, cfgs, ls, seqs, seed, decisions, sc, full_cap, emit_lp,
                           0, 0, 0, 0, floors);
}
void launch_sample_single(const void* logits, int rows, int vocab, const uint32_t* bitmap, int bm_words,
                          const MttsSamplerCfg* cfgs8, int mask_id, uint64_t seed, int step, int channel,
                          int32_t* decisions, int32_t* err, const SampleScratch& sc, int full_cap, int emit_lp,
                          const MttsSamplerFloors* floors, const float* typical, hipStream_t st) {
    if (vocab > SAMP_CAND) {
        hipLaunchKernelGGL(emit_lp ? sample_scan_kernel<true> : sample_scan_kernel<false>, dim3(SAMP_NS, rows), dim3(SAMP_T), 0, st,
                           (const uint16_t*)logits, vocab, bitmap, bm_words, cfgs8, (const LoopState*)nullptr,
                           (const SeqState*)nullptr, sc, vocab, mask_id, step, channel);
        hipLaunchKernelGGL(sample_collect_kernel, dim3(SAMP_NS, rows), dim3(SAMP_T), 0, st, (const uint16_t*)logits, vocab,
                           bitmap, bm_words, cfgs8, (const LoopState*)nullptr, (const SeqState*)nullptr, sc, full_cap, vocab, mask_id, step, channel);
    }
    LAUNCH_FINAL(dim3(1, rows), st, logits, nullptr, vocab, vocab, vocab, bitmap, bm_words, cfgs8, (const LoopState*)nullptr,
                 (const SeqState*)nullptr, seed, decisions, err, sc, 1, vocab, mask_id, step, channel, floors, typical);
    if (vocab > SAMP_CAND && typical)
        hipLaunchKernelGGL(sample_full_typ_kernel, dim3(rows), dim3(SAMP_FT), 0, st, (const uint16_t*)logits, vocab, bitmap, bm_words,
                           cfgs8, (const LoopState*)nullptr, (const SeqState*)nullptr, seed, decisions, sc, full_cap, emit_lp, vocab,
                           mask_id, step, channel, floors, typical);
    else if (vocab > SAMP_CAND)
        hipLaunchKernelGGL(floors ? sample_full_kernel<true> : sample_full_kernel<false>, dim3(rows), dim3(SAMP_FT), 0, st,
                           (const uint16_t*)logits, vocab, bitmap, bm_words, cfgs8, (const LoopState*)nullptr, (const SeqState*)nullptr,
                           seed, decisions, sc, full_cap, emit_lp, vocab, mask_id, step, channel, floors);
}
#undef LAUNCH_FINAL
void launch_update(const int32_t* decisions, int32_t* dec_log, const int32_t* forced, const int32_t* tf_tail,
                   int32_t* gen, int32_t* cur_tokens, SeqState* seqs, RowMeta* meta, uint32_t* bitmaps, int bm_words,
                   LoopState* ls, int eos, int spad, int sp_lo, int sp_hi, const float* lp_in, float* lp_out, const GenTopkOut& gt,
                   hipStream_t st) {
    hipLaunchKernelGGL(gt.k ? update_kernel<true> : update_kernel<false>, dim3(1), dim3(MTTS_RCAP), 0, st, decisions, dec_log, forced,
                       tf_tail, gen, cur_tokens, seqs, meta, bitmaps, bm_words, ls, eos, spad, sp_lo, sp_hi, lp_in, lp_out, gt);
}

// Un-shift the delay pattern on the device (reference generation_utils.py:416-425):
// codes[c][b][f - first] = gen[f + c][b][c] (- speech offset on channel 0), frames first..first+n-1.
__global__ void export_codes_kernel(const int32_t* __restrict__ gen, int64_t* __restrict__ codes, int B, int first, int n,
                                    int speech_offset, int clamp_hi, int cap) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= 8 * B * n) return;
    const int t = i % n, b = (i / n) % B, c = i / (n * B);
    int v = gen[((size_t)b * cap + (first + t + c)) * 8 + c];
    if (c == 0) v -= speech_offset;
    v = min(max(v, 0), clamp_hi);          // flushed / padded frames carry 1024 or EOS: keep the gather in range
    codes[i] = v;
}
void launch_export_codes(const int32_t* gen, int64_t* codes, int B, int first, int n, int speech_offset, int clamp_hi,
                         int cap, hipStream_t st) {
    int total = 8 * B * n;
    hipLaunchKernelGGL(export_codes_kernel, dim3((total + 255) / 256), dim3(256), 0, st, gen, codes, B, first, n,
                       speech_offset, clamp_hi, cap);
}
