// Host-side interface of the kernel files: the structs that cross between host and device code, and the one prototype
// of every launcher that one .hip defines and another calls.  Included by the defining file as well as by its callers,
// so a prototype or a layout cannot drift.  (common.h holds the device helpers and the structs kernels take as arguments.)
#pragma once
#include <type_traits>

#include "../../include/mtts.h"
#include "common.h"
#include "kvpool.h"          // PageEdits (launch_set_pages) and the KV page pool that fills it: HIP-free

// ---- gemm.hip -------------------------------------------------------------------------------------------------------
enum { EPI_PARTIAL = 0, EPI_BF16 = 1, EPI_SILU = 2,
       EPI_SILU_RM = 3 };      // SwiGLU, row-major bf16 [rows][N/2] output (gemv_small_kernel only)
struct GemmPlan {
    int waves, ksplit, kt_per_split, kt_per_wave;
    int depth;      // 1: launch_gemm may take a depth-specialised kernel where the shape has one (0: MTTS_GEMM_DEPTH=0)
};
GemmPlan mtts_plan_gemm(int Npad, int K, int want_ksplit);
GemmPlan mtts_plan_gemm_forced(int Npad, int K, int ksplit, int waves);
void launch_gemm(int epi, int mb, const GemmPlan& p, const void* Wp, const void* Xp, int K, int Npad, int n_valid,
                 float* partial, uint16_t* out, hipStream_t st);
int mtts_gemm_form(int epi, int mb, const GemmPlan& p, int K, int Npad, int n_valid);      // GEMM_SKINNY / GEMM_DEPTH / GEMM_GATEUP48 (shapes.h) of that call
int mtts_tile_ksplit(int Npad, int K, int R);
void launch_gemm_tile(int epi, int R, int ksplit, const void* Wp, const void* Xp, int K, int Npad, int n_valid,
                      float* partial, uint16_t* out, hipStream_t st);
int mtts_small_lds_bytes(const GemmPlan& p, int K, int pro);
void launch_gemv_small(int epi, int pro, const GemmPlan& p, const void* Wp, int K, int Npad, int n_valid, float* partial,
                       uint16_t* out, const SmallPro& pr, hipStream_t st);
long long mtts_gemm_depth_launches();
void mtts_gemm_depth_note();
void launch_pack_weight(const void* src, void* dst, int rows, int cols, int rows_pad, int row_mul, int row_off, hipStream_t st);
void launch_pack_rows(const void* src, void* dst, int R, int K, int tiles, hipStream_t st);
void launch_reduce_partial_bf16(const float* partial, void* out, int ksplit, int Npad, int n_valid, int R, hipStream_t st);

// ---- gemm_sealed.hip ------------------------------------------------------------------------------------------------
// The sealed twin of a packed weight array, for the decode shapes whose waves own 16 or 12 k-tiles (gate/up, the heads;
// down_proj).  wseal_shape: the plan / shape is one the sealed kernels take, and kt_per_wave is its group size.
// (the kinds: WSEAL_GU, WSEAL_DOWN, WSEAL_HEAD0, WSEAL_HEADS in shapes.h)
bool wseal_shape(const GemmPlan& p, int K, int Npad, int epi);
size_t wseal_bytes(int Npad, int K, int ktw);
void launch_wseal(const void* Wp, void* Ws, int K, int ktw, int nt0, int ntiles, hipStream_t st);     // N-tiles nt0 .. nt0 + ntiles - 1
void launch_wseal_count(const void* Ws, int Npad, int K, int ktw, unsigned long long* out2, hipStream_t st);   // out2 += {groups, not sealed}
bool launch_gemm_sealed(int epi, int mb, const GemmPlan& p, const void* Ws, const void* Wp, const void* Xp, int K, int Npad,
                        int n_valid, float* partial, uint16_t* out, int head_form, hipStream_t st);
long long mtts_wseal_launches();

// ---- gemm_fold.hip --------------------------------------------------------------------------------------------------
// o_proj -> post-attention RMSNorm -> gate/up of a one-row-tile decode step as two launches: the first finishes the
// residual stream x' (row-major in place, and in the X-fragment layout), the second normalises it in its X prologue.
bool fold_norm_shape(const GemmPlan& p_o, int K_o, const GemmPlan& p_gu, int H, int N_gu);      // the pair takes these two GEMMs
void launch_oproj_resid(const void* Wp, const void* Xp, void* x, void* x_packed, int R, int N, hipStream_t st);
void launch_gateup_norm(const void* Wp, const void* x_packed, const void* norm_w, float eps, void* out, int Npad, hipStream_t st);
long long mtts_fold_norm_launches();

// ---- layer.hip ------------------------------------------------------------------------------------------------------
void launch_embed_norm(const int32_t* tokens, const RowMeta* meta, const uint16_t* const* tables, const void* norm_w,
                       void* x, void* xn_packed, int R, int H, float eps, hipStream_t st);
void launch_resid_norm(const float* partial, int ksplit, int Npad, void* x, const void* norm_w, void* xn_packed,
                       void* hlast, const RowMeta* meta, int R, int H, float eps, hipStream_t st);
void launch_qkv_post(const float* partial, int ksplit, int Npad, const RowMeta* meta, const void* qnw, const void* knw,
                     const void* cosb, const void* sinb, void* qbuf, void* kcache, void* vcache,
                     const int32_t* page_table, int max_pages, int total_pages, int R, int nq, int nkv, float eps,
                     hipStream_t st);
void launch_rmsnorm_rows(const void* x, const void* w, void* y, int rows, int n, float eps, hipStream_t st);
void launch_fill_random_bf16(void* p, size_t n, uint32_t seed, hipStream_t st);
void launch_set_pages(int32_t* table, const PageEdits& ed, hipStream_t st);
void launch_fork(void* kc, void* vc, size_t layer_bytes, size_t head_bytes, int blk_bytes, int L, int nkv, const ForkJob& job,
                 hipStream_t st);
void launch_pack_kv_pages(const void* K, const void* V, void* kcache, void* vcache, const int32_t* page_table, const int32_t* lens,
                          int S, int Lmax, int nkv, int max_pages, int total_pages, hipStream_t st);
void launch_bf16_to_f32(const void* a, float* b, size_t n, hipStream_t st);
void launch_unpack_rows(const void* packed, void* out, int R, int K, hipStream_t st);
void launch_bf16_round_check(unsigned long long* cnt2, hipStream_t st);      // cnt2 += {non-NaN, NaN} inputs on which pack2_rn != f2bf

// ---- attn.hip -------------------------------------------------------------------------------------------------------
// One launch_attn call = one phase: scores / P.V / combine for decode-style rows (one dialogue per row), the same three
// for prefill tiles (32 consecutive positions of one dialogue), or ATTN_ALL = the three decode phases in one call.
// (mtts_k_attn_bench takes the number across the ABI: the values stay.)
enum AttnPhase { ATTN_ALL = 0, ATTN_SCORES = 1, ATTN_PV = 2, ATTN_COMBINE = 3,
                 ATTN_ROW = 4,       // the three decode phases as one launch, one block per (row, kv head): needs `fuse`
                 ATTN_PF_SCORES = 11, ATTN_PF_PV = 12, ATTN_PF_COMBINE = 13 };
int launch_attn(const void* qbuf, void* kcache, void* vcache, const int32_t* page_table,
                const RowMeta* meta, void* scores, float* stats, float* opart, void* out_packed, int R,
                int pages_bound, int max_pages, int total_pages, int nchunks_max, int nq, int nkv, float scale,
                const QkvFuse* fuse, AttnPhase phase, hipStream_t st, const KvPack* pack = nullptr);
bool attn_row_fits(int G, const QkvFuse* fuse, const KvPack* pack, int pages_bound);   // ATTN_ROW can take this launch
int attn_row_prepare();                  // once per device before the first ATTN_ROW launch (raises the kernels' LDS limit to the device's; -1: refused)
int attn_row_lds_limit();                // bytes of dynamic LDS an ATTN_ROW block may take (0 before attn_row_prepare)
long long mtts_attn_row_launches();      // ATTN_ROW launches issued by this process (captures count once)
void launch_kv_seal_rows(const void* kcache, const void* vcache, void* kpack, void* vpack, const int32_t* page_table,
                         const RowMeta* meta, int R, int max_pages, int total_pages, int nkv, int L, unsigned long long* cnt, hipStream_t st);
void launch_kv_seal_all(const void* kcache, const void* vcache, void* kpack, void* vpack, int total_pages, int nkv, int L,
                        unsigned long long* cnt, hipStream_t st);
void launch_kv_seal_pages(const void* raw, void* pk, int npages, int as_k, hipStream_t st);
void launch_kv_pack_count(const void* kpack, const void* vpack, const int32_t* page_table, const int32_t* complete, int B, int max_pages,
                          int total_pages, int nkv, int L, unsigned long long* out, hipStream_t st);

// ---- sampler.hip ----------------------------------------------------------------------------------------------------
struct SeqState {           // one per sequence slot, device resident.  Every dialogue carries its own clock so
                            // that slots can be refilled while others are mid-flight (continuous batching).
    int32_t nas;            // needs_additional_steps
    int32_t unfinished;
    int32_t kv_len;         // real tokens already in the KV cache
    int32_t step;           // decode steps this dialogue has run (= rows it generated)
    int32_t base_length;    // T-7 (padded slots) of its prompt
    int32_t max_length;     // HF max_length in padded slots
    int32_t row_id;         // Philox counter word 1 (batch row index in mtts_generate, 0 for scheduled dialogues)
    int32_t active;         // slot holds a dialogue that still steps
    uint64_t seed;          // Philox key
};

struct LoopState {          // one per engine, device resident
    int32_t step;           // decode steps executed so far by the engine
    int32_t done;           // no active row is unfinished
    int32_t continuous;     // 1: a finished row leaves the batch at once (scheduler); 0: it keeps emitting the
                            //    reference's finished-row padding until the whole batch is done (mtts_generate)
    int32_t B;
    int32_t error;          // sticky device-side error
    int32_t gen_cap;        // rows of generated-token storage per slot
    int32_t forced_draw;    // forced replay: 1 (2: cut-off rows too) = the forced row replaces the step's raw draw BEFORE the state machine
                            //    (replay of a sampled reference run); 0 = it replaces the state machine's output
    int32_t logits_f32;     // the logits buffers hold fp32 (MTTS_DTYPE_F32 engine) instead of bf16
};
// both are memcpy'd between host and device
static_assert(sizeof(SeqState) == 40 && std::is_trivially_copyable<SeqState>::value, "SeqState layout");
static_assert(sizeof(LoopState) == 32 && std::is_trivially_copyable<LoopState>::value, "LoopState layout");

#define SAMP_CAND 4096
#define SAMP_NS 32
struct SampleScratch {
    uint32_t* hist = nullptr;        // [32][2048]
    float* slice_val = nullptr;      // [32][SAMP_NS]
    int32_t* slice_idx = nullptr;    // [32][SAMP_NS]
    float* cand_val = nullptr;       // [32][SAMP_CAND]
    int32_t* cand_idx = nullptr;     // [32][SAMP_CAND]
    uint32_t* cand_n = nullptr;      // [rows]
    int32_t* overflow = nullptr;     // [rows] set by the final kernel when a row needs the full-vocabulary path
    float* full_val = nullptr;       // [rows][full_cap]   full-vocabulary path: level-0 bin (uint16) of every token
    int32_t* full_idx = nullptr;     // [rows][full_cap]   full-vocabulary path: key of every token
    uint32_t* nuc_cnt = nullptr;     // [rows][2048] level-0 histogram (count) left by the collect kernel for the full-vocabulary kernel
    unsigned long long* nuc_mass = nullptr;   // [rows][2048] ... and mass (exp(s - max) * 2^45, exact integer sums)
    // the next two exist only once output_scores was asked for (null otherwise; only the LP kernels touch them)
    float* slice_sum = nullptr;      // [rows][SAMP_NS] output_scores, greedy channel 0: sum of exp(s - slice_val) over the slice (its max IS slice_val)
    float* lp = nullptr;             // [rows][8] output_scores: log-probability of decisions[row][c], read by update_kernel
    // not scratch, but it travels with it to every sampler kernel: this step's banned tokens (mtts_set_sampler_bans), laid out
    // like the history bitmaps ([slot][8][bm_words]; the single-matrix entry: [rows][ceil(vocab / 32)]).  Null: no bans
    const uint32_t* ban = nullptr;
    // the same for this step's additive terms (mtts_set_sampler_bias): bias_w one bit per token that carries a term, in the
    // ban words' layout; bias_t the (id, term) table of each pair ([slot][8]; the single-matrix entry: [rows]).  Both null:
    // no finite rule
    const uint32_t* bias_w = nullptr;
    const MttsBiasTable* bias_t = nullptr;
    // externally scored rows (the split step: mtts_step_begin / mtts_step_finish): the logits pointers the sampler kernels get
    // are fp32 rows in the logits' layout that already carry masks, bans, terms and penalty (sample_ctx.h)
    int ext = 0;
};
void launch_sample(const void* logits0, const void* logits17, int V0, int Vs, int Vs_pad, const uint32_t* bitmaps,
                   int bm_words, const MttsSamplerCfg* cfgs, const LoopState* ls, const SeqState* seqs, uint64_t seed,
                   int32_t* decisions, int32_t* err, int B, const SampleScratch& sc, int ch0_sampled, int full_cap,
                   int emit_lp, const MttsSamplerFloors* floors /* device, 8 entries; null: no floors */,
                   const float* typical /* device, 8 entries (0: absent); null: no typical_p */, hipStream_t st);
void launch_sample_single(const void* logits, int rows, int vocab, const uint32_t* bitmap, int bm_words,
                          const MttsSamplerCfg* cfgs8, int mask_id, uint64_t seed, int step, int channel,
                          int32_t* decisions, int32_t* err, const SampleScratch& sc, int full_cap, int emit_lp,
                          const MttsSamplerFloors* floors8, const float* typical8, hipStream_t st);
// The ban kernel of a decode step (mtts_set_sampler_bans; sampler.hip: ban_kernel), one block per (row, channel) the
// sampler evaluates: ban[row][c][words] = stat[c][words], plus eos while the row's step < cfgs[c].eos_below, plus -- where
// cfgs[c].ngram = n > 0 -- the follower of every earlier occurrence of the history's last n-1 tokens.  The history of
// (row, c) is hist[row][0 .. base_length)[c] followed by gen[row][0 .. step)[c].
// min_length (mtts_set_sampler_bias) rides along: eos is also banned while base_length + step < cfgs[c].min_length, and
// begin ([8][words], or null) is a second static bitmap ORed in at the one step == 7, HF's begin_index.
struct BanCfg { int32_t ngram, eos_below, min_length; };      // eos_below = min_new_tokens + 7, or 0; min_length or 0
void launch_ban(uint32_t* ban, const uint32_t* stat, const uint32_t* begin, int words, const BanCfg* cfgs, const int32_t* hist, int hist_cap,
                const int32_t* gen, int V0, int Vs, int eos, const LoopState* ls, const SeqState* seqs, int B, hipStream_t st);
// one channel on bare histories hist [rows][cap], lens [rows]: ban [rows][ceil(vocab / 32)]; cfg1: one device BanCfg
// (eos_below != 0: eos banned); stat [ceil(vocab / 32)]
void launch_ban_single(uint32_t* ban, const uint32_t* stat, const BanCfg* cfg1, const int32_t* hist, const int32_t* lens, int rows,
                       int cap, int vocab, int eos, hipStream_t st);
long long mtts_ban_launches();
// The rule kernel of a decode step (mtts_set_sampler_bias; sampler.hip: bias_kernel), behind launch_ban and ahead of the
// sampler, one block per (row, channel) the sampler evaluates: rules[c] against the tail of the pair's history (hist /
// gen as for launch_ban; hist may be null when no rule is longer than one token).  The last token of every matching -inf
// rule is ORed into ban (null: the run has no -inf rule).  bias_w / tabs (both null: the run has no finite rule):
// bias_w[row][c][words] = bias_stat[c][words] plus the bit of every finite hit, tabs[row][c] the pair's (id, term) table.
void launch_bias(uint32_t* ban, uint32_t* bias_w, const uint32_t* bias_stat, MttsBiasTable* tabs, int words, const BiasRules* rules,
                 const int32_t* hist, int hist_cap, const int32_t* gen, int V0, int Vs, const LoopState* ls, const SeqState* seqs,
                 int B, hipStream_t st);
// one channel on bare histories: rules1 one device BiasRules, bias_stat [ceil(vocab / 32)]; ban / bias_w [rows][ceil(vocab / 32)], tabs [rows]
void launch_bias_single(uint32_t* ban, uint32_t* bias_w, const uint32_t* bias_stat, MttsBiasTable* tabs, const BiasRules* rules1,
                        const int32_t* hist, const int32_t* lens, int rows, int cap, int vocab, hipStream_t st);
long long mtts_bias_launches();
// generate(top_logprobs=k): where a step's results go.  In the engine the per-slot buffers, laid out like gen: logp
// [slot][gen_cap][8], ids / tlp [slot][gen_cap][8][k]; gen_topk_finish_kernel writes the step's row of every evaluated
// dialogue, update_kernel<true> then puts NaN / -1 over the slots that are not model decisions, by the rule it applies
// to lp.  k == 0: off, update_kernel<false> runs and looks at nothing here.
struct GenTopkOut {
    int32_t k = 0;
    float* logp = nullptr;
    int32_t* ids = nullptr;
    float* tlp = nullptr;
};
void launch_update(const int32_t* decisions, int32_t* dec_log, const int32_t* forced, const int32_t* tf_tail,
                   int32_t* gen, int32_t* cur_tokens, SeqState* seqs, RowMeta* meta, uint32_t* bitmaps, int bm_words,
                   LoopState* ls, int eos, int spad, int sp_lo, int sp_hi, const float* lp_in, float* lp_out,
                   const GenTopkOut& gt, hipStream_t st);
// The split step (mtts_step_begin / mtts_step_sample / mtts_step_finish; sampler.hip).
// launch_scores_materialize: one block per (row, channel) the sampler would evaluate this step writes that pair's processed
// scores in front of the warpers -- proc_score without the temperature: masks, bans (sc.ban), terms (sc.bias_w / sc.bias_t),
// repetition penalty -- as fp32 into out0 [B][V0 padded to 32] / out17 [B][7][Vs_pad]; the pad columns get -inf, rows the
// sampler skips are left untouched.  The sampler then runs on those buffers with sc.ext = 1.
void launch_scores_materialize(const void* logits0, const void* logits17, int V0, int Vs, int Vs_pad, const uint32_t* bitmaps, int bm_words,
                               const MttsSamplerCfg* cfgs, const LoopState* ls, const SeqState* seqs, int B, const SampleScratch& sc,
                               float* out0, float* out17, hipStream_t st);
// one logits matrix [rows][vocab] of bf16 bits -> out [rows][vocab padded to 32] (sc.ban / sc.bias_w / sc.bias_t: per row)
void launch_scores_materialize_single(const void* logits, int rows, int vocab, const uint32_t* bitmap, int bm_words, const MttsSamplerCfg* cfgs8,
                                      int mask_id, int step, int channel, const SampleScratch& sc, float* out, hipStream_t st);
// tokens [B][8] int64 = the tokens update_kernel appended this step (cur_tokens); rows at and above ls->B are left alone
void launch_step_tokens(const int32_t* cur_tokens, int64_t* tokens, const LoopState* ls, hipStream_t st);
// The caller's stopping criteria (reference modeling_asteroid.py:166-168), behind update_kernel: a row whose byte of stop
// is set and that is unfinished outside an EOS flush (needs_additional_steps <= 0) becomes a finished row -- it emits
// (eos, speech_pad x 7) from the next step on and, in a static batch, is still evaluated like a row max_length finished
// (active == 2: the reference may resurrect it for a flush); a row inside its flush stays unfinished.  ls->done is recomputed.
struct StopMask { uint8_t row[MTTS_RCAP]; };      // one byte per sequence slot, passed by value
void launch_stop_rows(const StopMask& stop, SeqState* seqs, RowMeta* meta, LoopState* ls, hipStream_t st);
void launch_export_codes(const int32_t* gen, int64_t* codes, int B, int first, int n, int speech_offset, int clamp_hi,
                         int cap, hipStream_t st);

// ---- gen_topk.hip ---------------------------------------------------------------------------------------------------
// generate(top_logprobs=k): per (row, channel) of a decode step, on the RAW logits row with the two hard-coded masks
// applied (no penalty, temperature, top-k, top-p): logp[row][c] = log_softmax(L)[decisions[row][c]], and ids / tlp
// [row][c][j], j < k, the first k tokens of L in the order of topk.h with their log_softmax(L).  A vocabulary above
// SAMP_CAND goes through one pass over the row's SAMP_NS slices (gen_topk_slice_kernel) and a merge in slice order; a
// smaller one is scanned by the finish block itself.  Rows the sampler does not evaluate are left alone (their slots keep
// the NaN / -1 the buffers start with).
struct GenTopkScratch {                  // exists only once a run asked for top_logprobs
    unsigned long long* cand = nullptr;  // [rows][SAMP_NS][kcap] a slice's best (value, id) pairs, descending, 0 = none (stride: the run's k)
    float* smax = nullptr;               // [rows][SAMP_NS] max of the slice's logits (-inf: nothing finite)
    double* ssum = nullptr;              // [rows][SAMP_NS] sum of exp(l - smax) over the slice
    int kcap = 0;
};
void launch_gen_topk(const void* logits0, const void* logits17, int V0, int Vs, int Vs_pad, const MttsSamplerCfg* cfgs,
                     const LoopState* ls, const SeqState* seqs, const int32_t* decisions, int B, const GenTopkScratch& sc,
                     const GenTopkOut& out, hipStream_t st);
// one logits matrix [rows][vocab] (bf16 bits or fp32), decisions [rows]; out.logp [rows], out.ids / out.tlp [rows][k]
void launch_gen_topk_single(const void* logits, int is_f32, int rows, int vocab, int mask_id, const int32_t* decisions,
                            const GenTopkScratch& sc, const GenTopkOut& out, hipStream_t st);

// ---- f32path.hip ----------------------------------------------------------------------------------------------------
#define MTTS_PF32CAP 256       // rows of a prefill pass in the fp32 engine (bounds its fp32 score scratch)
void launch_f32_embed_norm(const int32_t* tokens, const RowMeta* meta, const float* const* tables, const float* norm_w, float* x,
                           float* xn, int R, int H, float eps, int h16, hipStream_t st);
void launch_f32_resid_norm(const float* y, float* x, const float* norm_w, float* xn, float* hlast, const RowMeta* meta, int R,
                           int H, float eps, int h16, hipStream_t st);
void launch_f32_linear(const float* W, const float* X, float* Y, int R, int N, int K, long ldy, int h16, bool gemv, hipStream_t st);
void launch_f32_qkv_post(const float* qkv, int ldq, const RowMeta* meta, const float* qnw, const float* knw, const float* cosb,
                         const float* sinb, float* qbuf, float* kcache, float* vcache, const int32_t* page_table, int max_pages,
                         int total_pages, int R, int nq, int nkv, float eps, int h16, hipStream_t st);
void launch_f32_attn(const float* qbuf, const float* kcache, const float* vcache, const int32_t* page_table, const RowMeta* meta,
                     float* scores, float* out, int R, int max_pages, int total_pages, int nq, int nkv, float scale, int Lmax,
                     int h16, hipStream_t st);
void launch_f32_swiglu(const float* gu, float* act, int R, int I, int h16, hipStream_t st);

// ---- score.hip ------------------------------------------------------------------------------------------------------
// Teacher-forced scoring (mtts_score).  A head of n_valid columns is cut into blocks of 128 columns (4 MFMA tiles): a
// function of the vocabulary alone.  launch_head_ce: packed head weights (`segments` heads of round_up(n_valid, 32) rows
// one after another) x packed activations of R rows -> logp[row * out_stride + out_off + seg] = log_softmax(bf16 logits
// of head seg)[labels[row * lab_stride + lab_off + seg]], NaN where that label is < 0.  labels must hold round_up(R, 32)
// rows, `part` head_ce_part_elems(R, n_valid, segments) floats.
static inline int round_up32(int a) { return (a + 31) / 32 * 32; }
static inline int head_ce_blocks(int n_valid) { return ((n_valid + 31) / 32 + 3) / 4; }
size_t head_ce_part_elems(int rows, int n_valid, int segments);
void launch_head_ce(const void* Wp, const void* Xp, int R, int K, int n_valid, int segments, const int32_t* labels, int lab_stride,
                    int lab_off, float* part, float* logp, int out_stride, int out_off, hipStream_t st);
// the same on R rows of materialised fp32 logits [R][ldy] of one head (fp32 / fp16 engines)
void launch_ce_rows_f32(const float* logits, long ldy, int R, int n_valid, const int32_t* labels, int lab_stride, int lab_off,
                        float* logp, int out_stride, int out_off, hipStream_t st);
// Top-k next to it (mtts_score_topk), 1 <= k <= MTTS_SCORE_MAX_TOPK: top_ids / top_logp [(row * out_stride + out_off + seg)
// * k + j], j = 0..k-1 = the k columns with the largest logit, descending, ties by ascending column, and their
// log-probabilities; `logp` as launch_head_ce fills it, or null (labels must still be readable: < 0 everywhere then).
// The rows go through head_topk_kernel MTTS_SCORE_TOPK_ROWS at a time, so that `cand` -- every block's k candidates --
// stays at head_topk_cand_elems(R, n_valid, segments, k) words.
size_t head_topk_cand_elems(int rows, int n_valid, int segments, int k);
void launch_head_topk(const void* Wp, const void* Xp, int R, int K, int n_valid, int segments, const int32_t* labels, int lab_stride,
                      int lab_off, float* part, float* logp, int out_stride, int out_off, int k, uint32_t* cand, int32_t* top_ids,
                      float* top_logp, hipStream_t st);
void launch_topk_rows_f32(const float* logits, long ldy, int R, int n_valid, int k, int32_t* top_ids, float* top_logp, int out_stride,
                          int out_off, hipStream_t st);

// ---- adapter.hip ----------------------------------------------------------------------------------------------------
// A LoRA adapter merged into a projection weight: merged = round(W + ((B A), r terms summed in ascending order) * scaling),
// A fp32 [r][cols], B fp32 [rows][r], 1 <= r, cols % 16 == 0, every pointer 16-byte aligned.  launch_lora_pack: W bf16
// row-major -> the packed buffer, with launch_pack_weight's placement (source row s on packed row s * row_mul + row_off,
// only the groups of its source rows written).  launch_lora_rows_f32: W and dst fp32 row-major (h16: fp16 rounding).
void launch_lora_pack(const void* base, const float* A, const float* B, int r, float scaling, void* dst, int rows, int cols,
                      int row_mul, int row_off, hipStream_t st);
void launch_lora_rows_f32(const float* base, const float* A, const float* B, int r, float scaling, float* dst, int rows, int cols,
                          int h16, hipStream_t st);

// ---- multilora.hip --------------------------------------------------------------------------------------------------
// Unmerged per-row adapters: the delta scaling * B (A x) of a row's adapter as one more split-K slab of a GEMM, and the
// SwiGLU epilogue on the sum of two gate/up slabs.  One bank entry per (adapter, layer, projection): A fp32 [r][in],
// B fp32 [out][r], r = 0: the adapter does not target the matrix.  A job names the matrices whose outputs share one slab:
// matrix row i of segment s is slab column col0 + mul * i (q|k|v one after another; gate and up interleaved).
#define LORA_SEGS 3
#define LORA_MAX_K 16000       // row length a delta block can stage (fp32, in LDS)
struct LoraEnt { const float* A; const float* B; int32_t r; float scaling; };
struct LoraSeg { int32_t col0, ncols, mul, proj; };      // proj: entry of the layer (0..6: q k v o gate up down)
struct LoraJob { int32_t nseg, Npad, K, ent_stride; LoraSeg seg[LORA_SEGS]; };
static_assert(sizeof(LoraEnt) == 24 && std::is_trivially_copyable<LoraEnt>::value, "LoraEnt is memcpy'd to the device");
// rows [0, R) x columns [0, Npad) of `slab` ([MTTS_PFCAP][Npad]) are written, nothing else; xp: packed activations of
// row length job.K (% 16 == 0, <= LORA_MAX_K); ents: the bank at this layer, entry [adapter * job.ent_stride + proj]
void launch_lora_delta(const void* xp, const RowMeta* meta, const int32_t* seq_adapter, const LoraEnt* ents, const LoraJob& job,
                       float* slab, int R, hipStream_t st);
// act (packed, row length I) = SwiGLU(slab0 + slab1), slabs [MTTS_PFCAP][2 I] with gate / up columns interleaved; I % 8 == 0
void launch_swiglu_slabs(const float* slab0, const float* slab1, void* act_packed, int R, int I, hipStream_t st);

// ---- codec.hip / codec_fused.hip ------------------------------------------------------------------------------------
void mtts_gemm_f32_exact(hipStream_t st, const float* A, const float* W, float* C, int M, int N, int K, long ldc);
void launch_split_pack_w2perm(hipStream_t st, const float* w2, uint16_t* hi, uint16_t* lo);
void launch_vocos_pw_fused(hipStream_t st, const uint16_t* xn_planes, long x_plane_elems, const uint16_t* w1_planes, const float* b1,
                           const uint16_t* w2perm_planes, long w_plane_elems, const float* b2, const float* gamma, float* h, int M);
