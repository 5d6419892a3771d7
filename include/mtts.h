/*
 * mtts.h -- C ABI of libmtts.so, the MI355X-native engine under the
 * MOSS-TTSD hot path (AsteroidTTSInstruct decode + XY_Tokenizer decode).
 *
 * The reference has no FFI of its own: its boundary is the Python surface
 *   model.generate(input_ids[B,T,8], attention_mask[B,T])   generation_utils.py:406-409
 *   CustomMixin._sample                                      modeling_asteroid.py:53-197
 *   AsteroidTTSInstruct.forward (inference branch)           modeling_asteroid.py:337-380,411-426
 *   spt.decode(codes_list)                                   XY_Tokenizer/xy_tokenizer/model.py:195-256
 * Each entry point below names the reference code it replaces.  The Python
 * mirror of that surface (moss-ttsd_amd/modeling_asteroid.py etc.) binds these
 * symbols with ctypes; INTEGRATION.md shows the stub a maintainer would add.
 *
 * Conventions: extern "C"; plain pointers and sizes; every `dev_` pointer is
 * device memory of the engine's GPU (caller-owned: torch tensors); `host_`
 * pointers are host memory; `stream` is a hipStream_t passed as void* (NULL =
 * default stream).  Every function returns 0 on success or a negative
 * MTTS_E* code; mtts_last_error() gives the message of the calling thread's
 * last failure.  One engine = one device; an engine is not thread-safe.
 * No C++ exception crosses this boundary.
 */
#ifndef MTTS_H
#define MTTS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MTTS_OK 0
#define MTTS_EINVAL (-1)      /* bad argument / unsupported shape */
#define MTTS_EHIP (-2)        /* HIP runtime error */
#define MTTS_ENOMEM (-3)      /* KV page pool or workspace exhausted */
#define MTTS_ESTATE (-4)      /* call sequence error (e.g. decode before prefill) */

#define MTTS_CHANNELS 8

/* Fields of AsteroidTTSConfig / Qwen3Config the path reads
 * (modeling_asteroid.py:17-28; transformers Qwen3Config). */
typedef struct MttsConfig {
    int32_t vocab_size;            /* channel-0 vocabulary */
    int32_t hidden_size;
    int32_t intermediate_size;
    int32_t num_hidden_layers;
    int32_t num_attention_heads;
    int32_t num_key_value_heads;
    int32_t head_dim;              /* must be 128 */
    int32_t channels;              /* must be 8 */
    int32_t speech_vocab_size;     /* 1025 */
    int32_t speech_pad_token;      /* 1024 */
    int32_t speech_range_lo;       /* speech_token_range[0] */
    int32_t speech_range_hi;       /* speech_token_range[1] */
    int32_t eos_token_id;
    int32_t max_position;          /* rows in the RoPE table */
    float rms_norm_eps;
    int32_t max_batch;             /* sequences resident at once (1..128: up to 4 MFMA row tiles share each weight stream) */
    int32_t max_seq_len;           /* real tokens one sequence may reach (width of a page-table row) */
    int32_t kv_pool_pages;         /* 64-token KV pages in the pool shared by all sequences; 0 = max_batch x pages(max_seq_len),
                                      i.e. every slot can reach max_seq_len at once.  A smaller pool serves short dialogues
                                      with less memory: pages are taken on demand and returned when a dialogue finishes */
    int32_t dtype;                 /* MTTS_DTYPE_BF16 (0, the reference default) or MTTS_DTYPE_F32 (`inference.py --dtype fp32`,
                                      inference.py:27-40): fp32 weights, arithmetic, K/V pages and logits -- the strict-parity mode */
} MttsConfig;
#define MTTS_DTYPE_BF16 0
#define MTTS_DTYPE_F32 1
#define MTTS_DTYPE_F16 2   /* `--dtype fp16`: the MTTS_DTYPE_F32 kernels with an fp16 rounding point wherever the reference's fp16
                              run materialises a tensor; weights / RoPE tables are bound as fp32 tensors holding fp16 values */

/* generation_config.layers[i] / do_samples[i] (modeling_asteroid.py:95-106).
 * A field <= 0 (or top_k == 0) means "processor absent". */
typedef struct MttsSamplerCfg {
    int32_t do_sample;
    int32_t top_k;
    float top_p;
    float one_minus_top_p;   /* (float)(1.0 - (double)top_p): HF compares cum <= 1 - top_p with the scalar cast to fp32 */
    float temperature;
    float repetition_penalty;
} MttsSamplerCfg;

/* The probability floors of one channel (mtts_set_sampler_floors): HF's MinPLogitsWarper, EpsilonLogitsWarper and
 * EtaLogitsWarper.  They run in that order after repetition penalty, temperature, top-k and top-p, each on the
 * survivors K of the one before it.  With e_i = exp(s_i - smax), tot = sum over K of e_i and p_i = e_i / tot:
 *   min_p           floor = min_p * p_max, p_max = 1 / tot
 *   epsilon_cutoff  floor = epsilon
 *   eta_cutoff      floor = min(eta, sqrt(eta) * exp(-H)), H = -sum over K of p_i ln p_i
 * Token i leaves iff p_i < floor and s_i < smax (HF's min_tokens_to_keep = 1: a token at the maximum never leaves).
 * A field of 0 means "warper absent", as in MttsSamplerCfg.  A greedy channel applies none. */
typedef struct MttsSamplerFloors {
    float min_p;             /* 0..1 */
    float epsilon_cutoff;    /* 0 <= . < 1 */
    float eta_cutoff;        /* 0 <= . < 1 */
    float sqrt_eta_cutoff;   /* sqrt(eta_cutoff) in fp32, computed by the caller as torch.sqrt of the fp32 scalar gives it */
} MttsSamplerFloors;

/* The hard bans of one channel (mtts_set_sampler_bans): HF's NoRepeatNGramLogitsProcessor, MinNewTokensLengthLogitsProcessor
 * and SuppressTokensLogitsProcessor.  All three only put tokens at -inf, and -inf survives penalty and temperature, so
 * the order among the processors does not matter: a banned token has processed score -inf, everything else is as without
 * bans.  They are processors, not warpers: a greedy channel applies them too.  With h the channel's history at decode step
 * g (every left-padded prompt slot and every appended token: the stream the repetition penalty sees), the banned set is
 *   no_repeat_ngram_size n   every h[j+n-1] with h[j : j+n-1] == h[len(h)-n+1 :], 0 <= j <= len(h)-n  (n = 1: all of h)
 *   suppress                 every listed id inside the channel's vocabulary (others are ignored)
 *   min_new_tokens m         eos_token_id while g < m + 7 (HF counts from the full prompt width, delay tail included)
 * A field of 0 means "processor absent".  mtts/ban_spec.py states the same rule in numpy. */
#define MTTS_NGRAM_MAX 16
typedef struct MttsSamplerBans {
    int32_t no_repeat_ngram_size;    /* 0..MTTS_NGRAM_MAX */
    int32_t min_new_tokens;          /* >= 0 */
    int32_t n_suppress;              /* entries of suppress */
    const int32_t* suppress;         /* ids >= 0; read during the call only */
} MttsSamplerBans;

/* The sequence rules and step-conditioned bans of one channel (mtts_set_sampler_bias): HF's SequenceBiasLogitsProcessor,
 * NoBadWordsLogitsProcessor, MinLengthLogitsProcessor and SuppressTokensAtBeginLogitsProcessor.  With h the channel's history
 * at decode step g as MttsSamplerBans defines it, len(h) = base + g:
 *   rule (t_1..t_L, beta)   L = 1: token t_1 always carries beta.  L > 1: t_L carries beta at a step where len(h) >= L and
 *                           the last L-1 tokens of h are t_1..t_{L-1} (HF skips a rule longer than its context, so a
 *                           history of exactly L-1 tokens does not fire it).  A token's term is an fp32 chain: its single-token
 *                           beta (0 without one), then the beta of every matching longer rule in the order of rule_len,
 *                           each addition in fp32.  The processed score is penalty(raw + term) / temperature: one fp32
 *                           addition on the fp32 value of the raw logit, behind the two hard-coded masks (-inf stays
 *                           -inf) and in front of the repetition penalty, HF's order.  beta = -inf (bad_words_ids): a
 *                           matching rule bans t_L this step, with everything MttsSamplerBans says about a banned token.
 *                           A rule with an id outside the channel's vocabulary is ignored on that channel.
 *   min_length m            eos_token_id is banned while len(h) < m.
 *   begin_suppress          the listed ids inside the vocabulary are banned at the one step with len(h) = base + 7: HF's
 *                           begin_index is the full prompt width, delay tail included.
 * A field of 0 means "processor absent".  mtts/bias_spec.py states the same rule in numpy. */
#define MTTS_BIAS_RULES_MAX 64       /* rules per channel */
#define MTTS_BIAS_RULE_LEN_MAX 16    /* tokens per rule */
typedef struct MttsSamplerBias {
    int32_t n_rules;                 /* 0..MTTS_BIAS_RULES_MAX */
    int32_t min_length;              /* >= 0 */
    int32_t n_begin_suppress;        /* entries of begin_suppress */
    const int32_t* rule_len;         /* [n_rules], each 1..MTTS_BIAS_RULE_LEN_MAX; read during the call only, like the next three */
    const int32_t* rule_ids;         /* the rules' ids one rule after another, sum(rule_len) entries, each >= 0 */
    const float* rule_bias;          /* [n_rules]: beta; -inf is a ban, +inf and NaN are refused */
    const int32_t* begin_suppress;   /* ids >= 0 */
} MttsSamplerBias;
/* The terms of one (row, channel) pair at one step, as the rule kernel leaves them for the sampler: the n tokens that carry
 * a finite term this step, ascending by id, each with its chain's sum. */
typedef struct MttsBiasTable {
    int32_t n;
    int32_t ids[MTTS_BIAS_RULES_MAX];
    float term[MTTS_BIAS_RULES_MAX];
} MttsBiasTable;

typedef struct MttsEngine MttsEngine;

const char* mtts_last_error(void);
int32_t mtts_version(void);

/* ---- engine lifetime ---------------------------------------------------- */
int32_t mtts_engine_create(const MttsConfig* cfg, int32_t device, MttsEngine** out);
int32_t mtts_engine_destroy(MttsEngine* e);

/* Weight binding: state-dict name (reference naming, e.g.
 * "model.language_model.layers.3.self_attn.q_proj.weight",
 * "model.embedding_list.0.weight", "model.language_model.norm.weight") ->
 * bf16 row-major device tensor.  The engine re-lays the matrix out into its
 * MFMA-fragment order in its own memory; the caller's tensor may be freed
 * after the call returns (stream-ordered).  Replaces from_pretrained's
 * parameter materialisation (generation_utils.py:18). */
int32_t mtts_bind_weight(MttsEngine* e, const char* name, const void* dev_bf16,
                         int64_t rows, int64_t cols, void* stream);
/* (an MTTS_DTYPE_F32 engine takes fp32 row-major tensors through the same calls: dev_bf16 / dev_cos_bf16 / dev_sin_bf16
 * then point to floats, and the engine keeps plain copies) */
/* mtts_bind_weight with a LoRA adapter merged into the matrix (PEFT merge_and_unload, reference finetune/finetune.py:237,
 * per matrix and on the device): behaves as mtts_bind_weight(name, merged), where for dev_base W [rows][cols] in the
 * engine's weight format, dev_lora_a = lora_A.weight fp32 [r][cols] and dev_lora_b = lora_B.weight fp32 [rows][r]
 *     acc = 0;  for j = 0 .. r-1 ascending: acc = acc + B[n][j] * A[j][k]      (fp32, one multiply and one add: no fma)
 *     merged[n][k] = round_to_model_dtype(W[n][k] + acc * scaling)             (bf16 / fp16 RNE; none for fp32)
 * scaling = lora_alpha / r, or lora_alpha / sqrt(r) with use_rslora, computed by the caller.  The merged matrix goes
 * straight into the engine's layout (csrc/adapter.hip); no row-major merged copy exists.  `name` must be one of the seven
 * projection weights of a layer (q/k/v/o_proj, gate/up/down_proj).  MTTS_EINVAL: any other name, a shape other than the
 * weight's, r outside 1..256, a pointer that is not 16-byte aligned.  MTTS_ESTATE: a run is open (the rule of
 * mtts_set_output_scores); the weights are then as they were.  Like mtts_bind_weight it writes the engine's arrays in
 * place: captured step graphs hold addresses, not values, and stay valid.
 * Stream-ordered: the three tensors may be freed once `stream` has passed the call. */
int32_t mtts_bind_weight_lora(MttsEngine* e, const char* name, const void* dev_base, int64_t rows, int64_t cols,
                              const float* dev_lora_a, const float* dev_lora_b, int32_t r, float scaling, void* stream);
/* ---- resident adapters, one per dialogue (PEFT: load_adapter(path, adapter_name=...) + generate(adapter_names=[...])) ----
 * Up to MTTS_MAX_ADAPTERS LoRA adapters stay resident UNMERGED next to whatever weights are bound, and every row of a run
 * names the one it runs with (-1: none).  For a row with adapter a, every targeted projection computes
 *     y = W x + scaling * B (A x)
 * where W x is the engine's GEMM, untouched, and the low-rank term is added in fp32 before the Linear's output is rounded:
 * it is delivered as one more split-K slab of the GEMM (csrc/multilora.hip).  Its arithmetic is a function of
 * (x, A, B, scaling) alone, stated in numpy as mtts.adapters.delta_spec: a row's tokens and logits do not depend on what
 * shares its batch, and a row without an adapter computes what it computes on an engine with an empty bank.  (Against
 * the MERGED adapter of mtts_bind_weight_lora the results differ by the bf16 rounding of the merged weight.)
 * mtts_adapter_load: one matrix pair of adapter `adapter` (0 .. MTTS_MAX_ADAPTERS-1) for the projection weight `name`
 * ([rows][cols], as mtts_bind_weight_lora names it): dev_lora_a fp32 [r][cols], dev_lora_b fp32 [rows][r], 16-byte
 * aligned, copied into engine-owned memory on `stream` (drained before the call returns); a pair loaded before for the
 * same matrix is replaced.  Matrices an adapter never loads are not targeted.  mtts_adapter_clear frees an adapter.
 * Both: MTTS_ESTATE while a run is open (the rule of mtts_bind_weight_lora).
 * MTTS_EINVAL, with the offending value in mtts_last_error: an index outside the bank, a name that is not a projection
 * weight of a layer, a shape other than the weight's, r outside 1..MTTS_LORA_MAX_RANK, and an MTTS_DTYPE_F32 / _F16
 * engine (the bank exists on the bf16 engine only).  The engine takes no memory for any of this before the first
 * mtts_adapter_load (then: the bank's tables, one more split-K slab and the two unfused gate/up slabs). */
#define MTTS_MAX_ADAPTERS 16
#define MTTS_LORA_MAX_RANK 64
int32_t mtts_adapter_load(MttsEngine* e, int32_t adapter, const char* name, const float* dev_lora_a, const float* dev_lora_b,
                          int64_t rows, int64_t cols, int32_t r, float scaling, void* stream);
int32_t mtts_adapter_clear(MttsEngine* e, int32_t adapter);
/* The adapter of each row of the NEXT mtts_begin / mtts_generate (consumed by it, failures included, like
 * mtts_set_row_ids; default: none): host_ids int32 [n], n = that call's B, -1 = no adapter.  With takes it is given per
 * PROMPT and a prompt's takes inherit it (they share its KV pages, which depend on the adapter).  That call returns
 * MTTS_EINVAL for n != B or an id that names an empty adapter.  mtts_score does not take adapters: with a list pending it
 * returns MTTS_ESTATE and the list stays pending (score per adapter with mtts_bind_weight_lora). */
int32_t mtts_set_row_adapters(MttsEngine* e, const int32_t* host_ids, int32_t n);
/* Scheduler mode: the adapter (-1: none) of the next mtts_slot_submit* into `slot` (consumed by it, failures included;
 * default none).  mtts_slot_fork gives the take its source's adapter.  MTTS_EINVAL at the submit when it names an empty
 * adapter. */
int32_t mtts_set_slot_adapter(MttsEngine* e, int32_t slot, int32_t adapter);
/* RoPE table cos|sin, bf16 [max_position][64] each, computed by the host the
 * way Qwen3RotaryEmbedding does (fp32 -> bf16). */
int32_t mtts_bind_rope(MttsEngine* e, const void* dev_cos_bf16, const void* dev_sin_bf16,
                       int32_t rows, void* stream);
int32_t mtts_weights_ready(MttsEngine* e);   /* 0 when every tensor is bound */

/* ---- generation (replaces model.generate -> CustomMixin._sample) --------- */
/* host_input_ids int64 [B,T,8], host_attention_mask uint8 [B,T] (left padded,
 * 1 = real).  max_length = HF generation_config.max_length (T + max_new_tokens).
 * sampler[8], seed: sampling stream (Philox4x32-10).
 * Prefills the first T-7 slots, then runs the decode loop on the device until
 * every row is finished.  out: host_out_ids int64 [B, out_capacity, 8] receives
 * [B, T-7+G, 8]; *out_len = T-7+G.  G can exceed max_length - (T-7), exactly as in the reference
 * (modeling_asteroid.py:140-141,165-168): a dialogue whose EOS falls within 7 steps of max_length still runs its
 * delay-pattern flush, and while it does, a row that was cut off by max_length is resurrected for a flush of its own
 * as soon as its channel-0 pick is not a speech token (up to 14 steps past max_length); resurrections can chain, each
 * further row adding up to 6 steps, so size out_capacity as max_length + 6 * B + 8.  The engine has room for the whole
 * chain where max_seq_len allows and for 14 steps at least; a chain that outruns the room returns MTTS_ESTATE.
 * host_forced (verification hook, may be NULL): int64 [B, forced_len, 8] full
 * sequences; when given, every step's own decision is written to
 * host_decisions int64 [G,B,8] and the forced row is appended instead. */
int32_t mtts_generate(MttsEngine* e, const int64_t* host_input_ids, const uint8_t* host_attention_mask,
                      int32_t B, int32_t T, int32_t max_length,
                      const MttsSamplerCfg* sampler, uint64_t seed,
                      int64_t* host_out_ids, int32_t out_capacity, int32_t* out_len,
                      const int64_t* host_forced, int32_t forced_len, int64_t* host_decisions,
                      void* stream);

/* Step-level API (bench + tests): same state as mtts_generate, driven by the host. */
int32_t mtts_begin(MttsEngine* e, const int64_t* host_input_ids, const uint8_t* host_attention_mask,
                   int32_t B, int32_t T, int32_t max_length,
                   const MttsSamplerCfg* sampler, uint64_t seed, void* stream);   /* prefill */
int32_t mtts_step(MttsEngine* e, int32_t n_steps, void* stream);   /* n x (sample+update, forward); async */
int32_t mtts_sync_state(MttsEngine* e, int32_t* steps_done, int32_t* all_finished, void* stream);
int32_t mtts_read_generated(MttsEngine* e, int64_t* host_gen, int32_t capacity_steps, int32_t* n_steps);
/* ---- the split step: the caller's per-step hooks (HF generate(logits_processor=, stopping_criteria=, streamer=); reference
 * modeling_asteroid.py:109,129,161-168) ----
 * One decode step of a run started with mtts_begin, in halves with the caller in between; all calls are stream-ordered on
 * `stream` and return without waiting.  They replace one mtts_step(e, 1) and may alternate with mtts_step between steps.
 * mtts_step_begin: everything in front of the sampler.  For every (row, channel) the sampler would evaluate this step the
 * processed scores in front of the warpers are written as fp32: the two hard-coded masks, the bans and sequence rules of
 * the run (-inf / an added term) and the repetition penalty; no temperature.  dev_scores0: [rows of the run][vocab_size
 * padded to 32], channel 0; dev_scores17: [rows][7][speech_vocab_size padded to 32], channels 1..7; both device memory of
 * the caller, 16-byte aligned, alive until mtts_step_finish returns.  Pad columns get -inf; rows the sampler skips
 * (finished rows that cannot come back) are left untouched and never read.
 * mtts_step_sample: the sampler on those buffers as the caller left them -- temperature, top-k, top-p, min_p, typical_p and
 * the cutoffs, argmax or the Philox draw, output_scores as the log-softmax over the kept set; top_logprobs still reads the
 * raw logits -- then the state machine.  A row of -inf gives token 0 with a NaN score.  dev_tokens (device int64
 * [rows][8], or NULL): the tokens the step appended, padding and flushes included.
 * mtts_step_finish: host_stop (one byte per row, or NULL) is the caller's stopping criteria for the rows as they stand
 * after this step's tokens: a stopped row is finished (reference :166-168; a row inside its EOS flush finishes the flush
 * first) and emits (eos, speech_pad x 7) from the next step on; then the KV page bookkeeping and the forward pass.  Called
 * right after mtts_step_begin it runs mtts_step_sample itself.
 * MTTS_ESTATE: no run, a scheduler run (mtts_sched_open), a call out of order, no step left; mtts_step refuses while a
 * split step is in flight.  A run that never calls these launches, allocates and captures what it always did. */
int32_t mtts_step_begin(MttsEngine* e, float* dev_scores0, float* dev_scores17, void* stream);
int32_t mtts_step_sample(MttsEngine* e, int64_t* dev_tokens, void* stream);
int32_t mtts_step_finish(MttsEngine* e, const uint8_t* host_stop, void* stream);
/* ---- output_scores: per-token log-probabilities (HF generate(output_scores=True) reduced to what
 * compute_transition_scores(sequences, scores, normalize_logits=True) returns: one float per decision) ----
 * lp[g][r][c] = log_softmax(S)[d]: S = the channel's processed score row of step g (hard-coded masks, repetition penalty,
 * temperature, top-k, top-p; filtered tokens at -inf: modeling_asteroid.py:123-138 `next_token_scores`), d = the sampler's
 * own raw decision for the slot.  On a sampled channel that is the log-probability with which the engine drew d (the kept
 * set renormalised); on a greedy channel the log-softmax over all finite processed scores (a greedy channel applies no
 * top-k / top-p).  A slot whose appended token is NOT a model decision holds NaN: the teacher-forced channels c > step of
 * the first 7 steps, channels replaced by the EOS flush, finished-row padding, rows not evaluated.  The rule is the state
 * machine's; in the forced replay modes lp is still taken at the engine's own decision.  Full score rows (8 x [B,V_c] per
 * step) are not materialised.  Values are run-to-run bit-identical and do not depend on what else shares the batch.
 * mtts_set_output_scores: sticky switch (default off), read by the next mtts_begin / mtts_generate / mtts_sched_open; off,
 * the step is unchanged and no buffer exists.  MTTS_ESTATE when changed while a run is open (rows still unfinished on the
 * device); setting the value it already has always succeeds.  A run the caller has abandoned mid-flight counts as open: end
 * it first with mtts_sched_open (an empty scheduler run: no slot is occupied, so nothing is open), then set the switch
 * and begin.
 * mtts_read_scores: host_lp float [capacity_steps][rows][8], the row space and step range of mtts_read_generated;
 * MTTS_ESTATE when the run was started with scores off.  mtts_slot_read_scores: scheduler mode, host_rows float [steps][8],
 * like mtts_slot_read. */
int32_t mtts_set_output_scores(MttsEngine* e, int32_t on);
int32_t mtts_read_scores(MttsEngine* e, float* host_lp, int32_t capacity_steps, int32_t* n_steps);
int32_t mtts_slot_read_scores(MttsEngine* e, int32_t slot, float* host_rows, int32_t capacity_steps, int32_t* n_steps);
/* ---- top_logprobs of a generation: the model's own distribution at every decision (HF generate(output_logits=True)
 * reduced to the chosen token and the k most probable ones; what mtts_score_topk is to a prompt) ----
 * For step g, row r, channel c: L = the logits row the step's forward wrote, upcast to fp32, with the two hard-coded masks
 * applied (modeling_asteroid.py:124-128 `next_token_logits`) and NO repetition penalty, temperature, top-k or top-p;
 * d = the sampler's raw decision, the d of mtts_set_output_scores.
 *   logp[g][r][c]        = log_softmax(L)[d]
 *   top_ids[g][r][c][j], top_logp[g][r][c][j], j < k: the first k tokens of L by descending logit, ties by ascending id
 *                          (-0 = +0), and their log_softmax(L)
 * top_logp[..., j] is bit for bit the logp of a decision top_ids[..., j]; the first k' entries do not depend on k.  A slot
 * whose appended token is not a model decision holds NaN (ids: -1): exactly the slots where mtts_read_scores holds NaN,
 * and in the forced replay modes the values are taken at the engine's own decision, as there.  Sums run in a fixed order
 * without atomics: values are run-to-run bit-identical, the same under graph replay and stream launches, and a function
 * of (prompt, seed, row id) alone -- an evicted and re-run dialogue, a forked take (mtts_slot_fork copies nothing: values
 * start at the first generated step) and a queued take reproduce them.  Switching it on changes no token and no lp.
 * mtts_set_top_logprobs: sticky, k = 0 off (default) or 1..MTTS_SCORE_MAX_TOPK, else MTTS_EINVAL; read by the next
 * mtts_begin / mtts_generate / mtts_sched_open; MTTS_ESTATE (setting unchanged) while a run is open, the rule of
 * mtts_set_output_scores, of which it is independent.  Off, the step launches what it launched before and neither the
 * scratch nor the buffers exist; they are allocated by the first run that asks and again when k changes.
 * mtts_read_top_logprobs: host_logp float [capacity_steps][rows][8], host_top_ids int32 and host_top_logp float
 * [capacity_steps][rows][8][k], the row space and step range of mtts_read_generated; MTTS_ESTATE when the run was started
 * with k = 0.  mtts_slot_read_top_logprobs: scheduler mode, [steps][8] and [steps][8][k], like mtts_slot_read_scores. */
int32_t mtts_set_top_logprobs(MttsEngine* e, int32_t k);
int32_t mtts_read_top_logprobs(MttsEngine* e, float* host_logp, int32_t* host_top_ids, float* host_top_logp,
                               int32_t capacity_steps, int32_t* n_steps);
int32_t mtts_slot_read_top_logprobs(MttsEngine* e, int32_t slot, float* host_logp, int32_t* host_top_ids, float* host_top_logp,
                                    int32_t capacity_steps, int32_t* n_steps);
/* ---- teacher-forced scoring: the labels branch of AsteroidTTSInstruct.forward (modeling_asteroid.py:382-410: per channel
 * lm_heads[i](hidden_states) and ForCausalLMLoss) reduced to one float per label; what inference engines call prompt
 * log-probabilities.  host_input_ids int64 [B,T,8], host_attention_mask uint8 [B,T], host_labels int64 [B,T,8] (-100 =
 * ignore), host_logp float [B,T,8] (out).  The HF shift applies: logp[b][t][c] = log_softmax(logits_c(h[b][t-1]))[labels[b][t][c]]
 * for t >= 1, with logits_c in the model dtype upcast to fp32 (transformers ForCausalLMLoss); NaN at t = 0, at ignored
 * labels and at padding (the convention of mtts_read_scores).  The caller reduces: loss_all[c] = -mean of the non-NaN
 * logp[..., c].  Sequences are RIGHT-padded or unpadded (each mask row ones, then zeros, as causal-LM collators produce):
 * real token i sits at position i, the reference's arange(T) positions when forward gets no position_ids.  The logits are
 * never materialised (bf16 engine: fused head GEMM + log-sum-exp, csrc/score.hip); a value is run-to-run bit-identical
 * and does not depend on what else shares the batch.  The KV pages the call takes are back in the pool when it returns
 * and no state of a generation survives or is needed: mtts_begin afterwards behaves as if the call had not happened.
 * Synchronous: `stream` is drained before it returns, on success and on failure, the device page table included.
 * MTTS_EINVAL: a left-padded (or otherwise not ones-then-zeros) mask row, a label other than -100 at a
 * masked position or outside [0, V_c), a token out of range, B > max_batch, T > max_seq_len; MTTS_ESTATE: a run is open
 * (the rule of mtts_set_output_scores); MTTS_ENOMEM: the pool cannot hold the batch (reported before any launch). */
int32_t mtts_score(MttsEngine* e, const int64_t* host_input_ids, const uint8_t* host_attention_mask,
                   const int64_t* host_labels, int32_t B, int32_t T, float* host_logp, void* stream);
/* The same call that also returns, for every slot mtts_score can score (1 <= t < len_b, every channel c), the k most
 * probable tokens of the distribution the label is scored under: host_top_ids int32 [B,T,8,k] and host_top_logp float
 * [B,T,8,k], entry j = 0..k-1 in descending order of the logit, ties by ascending id (bf16 logits tie often); id -1 and
 * NaN at t = 0, at padding and past a row's last token.  Labels play no part in it: a slot whose label is -100 is filled
 * like any other, and host_labels may be NULL (then host_logp must be NULL too and is not written; otherwise both are
 * given and host_logp is exactly what mtts_score writes).  host_top_logp[..., j] is bit for bit what mtts_score returns
 * at that slot for the label host_top_ids[..., j], and the first k' entries of a call with k are the entries of a call
 * with k' < k.  1 <= k <= MTTS_SCORE_MAX_TOPK, else MTTS_EINVAL; every other precondition, error code and guarantee is
 * mtts_score's (synchronous, pages handed back, MTTS_ESTATE with a run open or an adapter list pending).  The logits are
 * not materialised on a bf16 engine: the k best columns of each 128-column block are selected in the head GEMM's
 * epilogue and merged per row.  Besides the staged results (8 x k ids and floats per staged row) those candidates are
 * the one buffer the call adds, allocated by the first such call and bounded whatever the batch and k: 4 bytes x
 * MTTS_SCORE_TOPK_ROWS rows x the 128-column blocks of head 0 (the speech heads reuse it) x 16 = 39 MB at 152 697
 * columns -- a prefill pass goes through the heads MTTS_SCORE_TOPK_ROWS rows at a time. */
#define MTTS_SCORE_MAX_TOPK 16
#define MTTS_SCORE_TOPK_ROWS 512
int32_t mtts_score_topk(MttsEngine* e, const int64_t* host_input_ids, const uint8_t* host_attention_mask,
                        const int64_t* host_labels, int32_t B, int32_t T, float* host_logp, int32_t k,
                        int32_t* host_top_ids, float* host_top_logp, void* stream);
/* last forward's logits: bf16 bits, channel 0 [B,vocab_size], channels 1..7 [7,B,speech_vocab_size] */
int32_t mtts_read_logits(MttsEngine* e, uint16_t* host_logits0, uint16_t* host_logits17, void* stream);
/* the same for an MTTS_DTYPE_F32 engine: fp32 logits */
int32_t mtts_read_logits_f32(MttsEngine* e, float* host_logits0, float* host_logits17, void* stream);
/* ---- continuous batching: slots are refilled while other dialogues are mid-flight ---------
 * mtts_sched_open: B empty slots, gen_cap rows of token storage each.  mtts_slot_submit: prefill ONE delay-shifted
 * prompt (host int64 [T][8], no padding) into an empty slot; its Philox stream is (seed; step, 0, channel).
 * mtts_step advances every occupied slot; a finished dialogue leaves the batch at once.  mtts_slot_states:
 * int32 [B][4] = (active, unfinished, rows generated, tokens cached).  mtts_slot_read: its rows int64 [steps][8]. */
int32_t mtts_sched_open(MttsEngine* e, int32_t B, int32_t gen_cap, const MttsSamplerCfg* sampler, void* stream);
int32_t mtts_slot_submit(MttsEngine* e, int32_t slot, const int64_t* host_ids, int32_t T, int32_t max_length, uint64_t seed,
                         void* stream);
/* the same with an explicit Philox row id: the dialogue draws from (seed; step, row_id, channel) -- what row `row_id` of a
 * static batch with that seed draws (mtts_slot_submit = row_id 0) */
int32_t mtts_slot_submit_row(MttsEngine* e, int32_t slot, const int64_t* host_ids, int32_t T, int32_t max_length, uint64_t seed,
                             int32_t row_id, void* stream);
/* Philox row ids of the rows of the NEXT mtts_begin / mtts_generate (consumed by it, failures included; default 0..B-1): one rank's share of
 * a sharded batch draws what its rows would draw inside the whole batch (host_row_ids int32 [n], n = that call's B). */
int32_t mtts_set_row_ids(MttsEngine* e, const int32_t* host_row_ids, int32_t n);
/* Takes per prompt of the NEXT mtts_begin / mtts_generate (consumed by it, failures included; default 1): HF
 * generate(num_return_sequences=n) with sampling (GenerationMixin._expand_inputs_for_generation repeat-interleaves the
 * batch).  B stays the number of prompts; the run has B*n rows, row b*n+j is take j of prompt b, and every per-row buffer
 * of the run is in that row space (output ids, mtts_set_row_ids, mtts_read_generated / _logits / _seq_state,
 * mtts_export_codes).  Only the B prompts are prefilled; the takes share their complete prompt pages (one owner count per
 * KV page) and copy the partially filled last one.  The tokens equal those of the repeat-interleaved batch.
 * MTTS_EINVAL: B*n > max_batch, or n > 1 with host_forced (the replay hook has no takes). */
int32_t mtts_set_takes(MttsEngine* e, int32_t n);
/* Probability floors of the NEXT run only (one-shot, like mtts_set_takes: consumed by the next mtts_begin, mtts_generate or
 * mtts_sched_open, failures included; a run that does not ask for floors never inherits them): floors[c] is channel c's
 * MttsSamplerFloors, applied where that run's sampler[c].do_sample is set.  NULL: none.  They act inside the sampler, on the
 * kept set top-k / top-p leave: the draw rule (descending score, ties by higher id, the same Philox key) and every other
 * output are as without them, lp of mtts_set_output_scores is the log-softmax over the final kept set, and
 * mtts_set_top_logprobs, which describes the raw distribution, does not see them.  A run whose floors are all zero on its
 * sampled channels launches what a run without floors launches.
 * MTTS_EINVAL, naming the channel: min_p outside [0, 1], epsilon_cutoff or eta_cutoff outside [0, 1) (NaN included). */
int32_t mtts_set_sampler_floors(MttsEngine* e, const MttsSamplerFloors floors[8] /* NULL: none */);
/* Hard bans of the NEXT run only (one-shot like mtts_set_sampler_floors: consumed by the next mtts_begin, mtts_generate or
 * mtts_sched_open, failures included): bans[c] is channel c's MttsSamplerBans, applied whether the channel samples or not.
 * NULL: none.  A banned token has processed score -inf in every sampler kernel; lp of mtts_set_output_scores is the
 * log-softmax over what survives, bans included, and mtts_set_top_logprobs, which describes the raw distribution, does not
 * see them.  A row whose every token is banned gives token 0 with lp NaN, on greedy and sampled channels alike.  A run with
 * a ban launches one more kernel per decode step, ahead of the sampler, which rewrites the per-(row, channel) ban words:
 * the static part (suppress, eos while the step is below min_new_tokens + 7), then the followers of every earlier
 * occurrence of the history's last n-1 tokens.  The history and ban buffers exist only once a run asked for them; a
 * run without bans launches what it launched before and allocates nothing.  With an n-gram ban a prompt may have at most
 * max_seq_len slots (padding included).
 * MTTS_EINVAL, naming the channel: no_repeat_ngram_size outside [0, MTTS_NGRAM_MAX], min_new_tokens < 0, n_suppress < 0 or
 * without a list, a negative id. */
int32_t mtts_set_sampler_bans(MttsEngine* e, const MttsSamplerBans bans[8] /* NULL: none */);
/* typical_p of the NEXT run only (one-shot like mtts_set_sampler_floors: consumed by the next mtts_begin, mtts_generate or
 * mtts_sched_open, failures included): typical_p[c] is channel c's mass for HF's TypicalLogitsWarper (locally typical
 * sampling), applied where that run's sampler[c].do_sample is set.  It runs in HF's place, after min_p and before
 * epsilon_cutoff.  Over the set K kept so far, with p = softmax over K, H = -sum p_i ln p_i and shift_i = |-ln p_i - H|:
 * t* is the smallest shift whose tokens {shift_i <= t*} hold at least typical_p of the mass, and token i stays iff
 * shift_i <= t*.  Tokens of equal score stay or leave together; the kept set is an interval in score order whose top need
 * not be the row's maximum -- the one warper that can remove the most probable token.  epsilon_cutoff and eta_cutoff then
 * never drop a token at the maximum of that interval, the draw walks it from its top down, and lp is the log-softmax over
 * the final set.  0 and 1 mean "absent" (HF adds the warper for typical_p < 1); a run without a typical_p on a sampled
 * channel launches what it launched before.  mtts/warp_spec.py states the rule in numpy.
 * MTTS_EINVAL, naming the channel, and nothing is left pending: a typical_p that is neither 0 nor 1 nor strictly inside
 * (0, 1), NaN included. */
int32_t mtts_set_sampler_typical(MttsEngine* e, const float typical_p[8] /* NULL: none; 0 or 1: absent */);
/* Launches of the ban kernel by this process so far (engine steps and mtts_k_ngram_ban). */
int64_t mtts_debug_ban_launches(void);
/* Sequence rules, min_length and begin_suppress_tokens of the NEXT run only (one-shot like mtts_set_sampler_bans: consumed by
 * the next mtts_begin, mtts_generate or mtts_sched_open, failures included): bias[c] is channel c's MttsSamplerBias, applied
 * whether the channel samples or not.  NULL: none.  The lists are copied during the call.  lp of mtts_set_output_scores is
 * the log-softmax over the final kept set of the biased, processed scores; mtts_set_top_logprobs, which describes the raw
 * distribution, sees neither term nor ban.  A run with a rule launches one more kernel per decode step, behind the ban kernel
 * and ahead of the sampler: one block per (row, channel), whose first wave tests every rule's prefix against the tail of
 * the history, ORs the last token of each matching -inf rule into the pair's ban words, and -- in a run with a finite beta --
 * rewrites the pair's bias words (a bitmap in the ban words' layout, from the channel's single-token rules) and its
 * MttsBiasTable, from which the sampler's score function adds the term of a token whose bit is set.  No float atomics: the
 * chain is summed in rule order by one lane per token, so words and tables are the same bits run to run and under graph
 * replay.  A -inf rule, min_length or begin_suppress turn the ban path on (eos under min_length and the begin list are
 * step-conditioned static bans of the ban kernel).  Rules longer than one token need the prompt history of the n-gram
 * ban: a prompt may then have at most max_seq_len slots (padding included).  Every buffer exists only once a run asked for
 * it; a run that sets none of this launches and allocates what it did before.
 * MTTS_EINVAL, naming the channel, and nothing is left pending: n_rules outside [0, MTTS_BIAS_RULES_MAX], a rule length
 * outside [1, MTTS_BIAS_RULE_LEN_MAX], a negative id, a beta that is NaN or +inf, min_length < 0, a count without its list. */
int32_t mtts_set_sampler_bias(MttsEngine* e, const MttsSamplerBias bias[8] /* NULL: none */);
/* Launches of the rule kernel by this process so far (engine steps and mtts_k_seq_bias). */
int64_t mtts_debug_bias_launches(void);
/* Scheduler mode: start a take of the dialogue just submitted to src_slot in the empty dst_slot: same prompt (its
 * complete KV pages shared, the partially filled last one copied), drawing from (seed; step, row_id, channel).  The take's
 * tokens equal those of mtts_slot_submit_row(dst_slot, the same prompt, seed, row_id).  Stream-ordered on `stream`.
 * MTTS_ESTATE: src_slot was not submitted since the last mtts_step, or dst_slot is occupied; MTTS_ENOMEM: the prompt ends
 * mid-page and no page is free for the copy. */
int32_t mtts_slot_fork(MttsEngine* e, int32_t src_slot, int32_t dst_slot, uint64_t seed, int32_t row_id, void* stream);
int32_t mtts_slot_states(MttsEngine* e, int32_t* host_state, void* stream);
int32_t mtts_slot_read(MttsEngine* e, int32_t slot, int64_t* host_rows, int32_t capacity_steps, int32_t* n_steps);
int32_t mtts_read_seq_state(MttsEngine* e, int32_t* host_nas, int32_t* host_unfinished, int32_t* host_kv_len, void* stream);
/* Evict the dialogue in `slot` (scheduler mode): it leaves the batch now and its KV pages return to the pool; the host
 * re-submits it later (tokens are a function of prompt and seed only, so the re-run reproduces them).  Used when
 * mtts_step reports MTTS_ENOMEM: the pool cannot grow every resident dialogue by another page. */
int32_t mtts_slot_evict(MttsEngine* e, int32_t slot, void* stream);
/* KV pool occupancy: pages in the pool, pages free, pages per page-table row. */
int32_t mtts_kv_pool_state(MttsEngine* e, int32_t* total_pages, int32_t* free_pages, int32_t* max_pages_per_seq);
/* host_table int32 [max_batch][max_pages_per_seq] (the device page table as the host tracks it), host_n_pages int32 [max_batch]. */
int32_t mtts_read_page_table(MttsEngine* e, int32_t* host_table, int32_t* host_n_pages);
/* Forced replay mode of mtts_generate's verification hook: 0 (default) the forced row replaces the state machine's
 * output (replay of a greedy run); 1 it replaces the step's raw draw before the state machine, host_decisions receives
 * the raw draws (replay of a SAMPLED reference run: the state follows the reference's history); 2 = as 1, and the forced
 * row is also the raw draw of rows that max_length has cut off and that the reference keeps evaluating
 * (modeling_asteroid.py:140-141: tests that script chained finished-row resurrections). */
int32_t mtts_set_forced_mode(MttsEngine* e, int32_t as_draw);
/* verification hook: the page table as the device holds it once everything queued on `stream` has run
 * (host_table int32 [max_batch][max_pages_per_seq]); compare with mtts_read_page_table. */
int32_t mtts_debug_read_device_page_table(MttsEngine* e, int32_t* host_table, void* stream);
/* Frames first..first+n-1 as codec codes int64 [8][B][n] on the device (delay pattern undone, generation_utils.py:416-425);
 * `stream` must be ordered after the steps that produced frame first+n+6. */
int32_t mtts_export_codes(MttsEngine* e, int32_t first, int32_t n, int64_t* dev_codes, void* stream);
/* name of / time spent in the dominant decode kernel since the last reset, measured with hipEvents
 * on the launch stream (bench.py's roofline leg). */
/* which: 0 attention scores, 1 P.V, 2 GEMM, 3 whole decode step, 4 the scoring kernels of mtts_score (head_ce_kernel +
 * ce_finish_kernel, one entry per prefill pass; with top-k: head_topk_kernel, ce_finish_kernel and topk_finish_kernel). */
int32_t mtts_profile_enable(MttsEngine* e, int32_t on);
int32_t mtts_profile_read(MttsEngine* e, int32_t which, double* total_ms, int64_t* launches, int64_t* bytes);

/* measurement hooks (bench / profiling only, never on the product path) */
int32_t mtts_debug_set_kv_len(MttsEngine* e, int32_t kv_len);   /* also fills the KV pages with pseudo-random bf16 */
/* sealed KV pages (csrc/attn.hip kv_seal): out6 = {complete K pages of the live dialogues x kv heads x
 * layers, of which NOT sealed (a lane's 128 values held more than 8 distinct high bytes: read as bf16), the same for V,
 * number of layers whose K reads / V reads currently take the sealed pages (the read policy switches a layer back to bf16
 * reads when more than 1 in 8 of its pages did not seal)}.  MTTS_ESTATE when the engine keeps none (fp32 / fp16 engines,
 * MTTS_KV_PACK=0). */
int32_t mtts_debug_kv_pack_stats(MttsEngine* e, int64_t* out6);
/* How a step chooses its kernels (csrc/stepplan.h): the plan of the decode step the engine would run now
 * at `pages_bound` KV pages -- its current rows, run options and read policies -- as text into buf[cap], NUL-terminated,
 * one line per distinct launch group in issue order ("attn[0..27]: row sealed", "down: depth sealed", ...).
 * MTTS_EINVAL when `cap` is too small. */
int32_t mtts_debug_step_plan(MttsEngine* e, int32_t pages_bound, char* buf, int32_t cap);
/* train of `iters` launches of one decode attention pass (1 scores, 2 P.V, 3 combine, 0 = the three in a row, 4 = the
 * whole-row kernel that does all three in one launch) at the current state; when the product would
 * run the fused q/k/v epilogue at this size the train does too and overwrites the current position's K/V rows:
 * call it only when no further step follows */
int32_t mtts_k_attn_bench(MttsEngine* e, int32_t phase, int32_t iters, float* avg_ms, int64_t* bytes_per_launch);
/* waves > 0: skinny decode GEMM (32 rows) with that decomposition; waves < 0: the tiled prefill GEMM on -waves rows */
int32_t mtts_k_gemm_bench(int32_t N, int32_t K, int32_t epi, int32_t ksplit, int32_t waves, int32_t copies,
                          int32_t iters, float* avg_us);

/* Sealed weight streams (csrc/gemm_sealed.hip): gate/up, down_proj and the heads also exist in the sealed
 * 13-bit form and the one-row-tile decode GEMMs read that.  out12 = per kind (gate/up, down_proj, head 0, heads 1-7):
 * {groups, groups NOT sealed (a lane held more than 8 distinct high bytes: its wave reads the bf16 tiles), 1 if the
 * kind's decode GEMMs currently read the twin}.  Runs mtts_weights_ready (the counts are taken there, after a bind).
 * MTTS_ESTATE when the engine keeps no twins (fp32 / fp16 engines, MTTS_W_SEAL=0, MTTS_GEMM_DEPTH=0). */
int32_t mtts_debug_wseal_stats(MttsEngine* e, int64_t* out12);
/* number of GEMM launches of this process that took a sealed kernel (they also count as depth-specialised launches,
 * mtts_debug_gemm_depth_launches below); under graph replay a launch counts once, when it is captured */
int64_t mtts_debug_wseal_launches(void);
/* mtts_k_gemm_bench's launch train on `copies` packed copies of W [N][K] bf16 row-major (NULL: a constant), 32 rows, 8
 * waves, split-K as given: sealed != 0 the sealed kernel on the copies' twins (head_form, epi 1 only: 1 the persistent
 * kernel, 0 one tile per block), 0 launch_gemm on the bf16 copies.  epi 0 partial / 1 bf16 / 2 SwiGLU; only the shapes
 * the sealed kernels take.  out2 (may be NULL) = {groups, groups not sealed} of one copy. */
int32_t mtts_k_gemm_sealed_bench(const void* dev_w, int32_t N, int32_t K, int32_t epi, int32_t ksplit, int32_t copies,
                                 int32_t iters, int32_t sealed, int32_t head_form, float* avg_us, int64_t* out2);

/* ---- per-kernel entry points (unit tests; device pointers) ---------------- */
/* The bind-time sealer: a packed weight array of `ntiles` N-tiles ([ntiles][K/16][64 lanes][16 B]) -> its sealed twin
 * [ntiles][K/16/ktw][13 or 10 units][64][16 B], groups of ktw = 16 or 12 k-tiles.  A 16-tile group is a page of
 * mtts_k_kv_seal's plain form; a 12-tile group is the 16-unit form of the lane's 96 values followed by 32 copies of its
 * first value, units 0-5, 8-10 and 12 kept (oracle/kv_seal_oracle.py is the specification of both). */
int32_t mtts_k_wseal(const void* dev_packed, int32_t ntiles, int32_t K, int32_t ktw, void* dev_sealed, void* stream);
/* One decode GEMM of 1 <= M <= 32 rows, W [N][K] and X [M][K] bf16 row-major, packed and sealed by the hook, through the
 * sealed kernel (sealed != 0) or through launch_gemm on the same packed array (0).  dev_out receives the kernel's raw
 * output, which starts as 0xa5 bytes: epi 0 fp32 [ksplit][32][Npad]; 1 bf16 [32][Npad] (columns >= N keep the sentinel);
 * 2 bf16 32 * Npad / 2 in the X-fragment layout (Npad = N rounded up to 32).  out2 (may be NULL) as above. */
int32_t mtts_k_gemm_sealed(const void* dev_w, const void* dev_x, void* dev_out, int32_t M, int32_t N, int32_t K, int32_t epi,
                           int32_t ksplit, int32_t sealed, int32_t head_form, int64_t* out2, void* stream);
/* Y[M,N] = X[M,K] * W[N,K]^T, bf16 in, fp32 accumulate, bf16 out.  M <= 128: skinny decode kernel; 128 < M <= 512:
 * tiled prefill kernel. */
int32_t mtts_k_gemm_bf16(const void* dev_w, const void* dev_x, void* dev_y,
                         int32_t M, int32_t N, int32_t K, int32_t ksplit, void* stream);
/* number of GEMM launches of this process that took a depth-specialised kernel (gemm_depth_kernel / gemm_gateup48_kernel,
 * or one of their sealed twins) instead of gemm_skinny_kernel; under graph replay a launch counts once, when it is captured (tests: did the dispatch fire) */
int64_t mtts_debug_gemm_depth_launches(void);
/* number of launches of this process that took one of gemm_fold.hip's kernels (the o_proj that finishes the residual
 * stream, the gate/up that normalises it: MTTS_FOLD_NORM); counted like the above */
int64_t mtts_debug_fold_norm_launches(void);
/* oproj_resid_kernel alone: dev_x bf16 [R][N] += bf16(dev_attn [R][2048] * dev_wo [N][2048]^T), in place, with o_proj's
 * split-K 4 sum tree and resid_norm_kernel's two roundings; dev_x_packed (bf16, 32 * N, the X-fragment layout of one
 * 32-row tile) receives the same rows, the rest of it keeps what the caller put there.  1 <= R <= 32, N % 32 == 0. */
int32_t mtts_k_oproj_resid(const void* dev_wo, const void* dev_attn, void* dev_x, void* dev_x_packed, int32_t R, int32_t N,
                           void* stream);
/* The pair at H = 2048: the producer as above (N = 2048), then gemm_gateup48_norm_kernel on dev_wgu [N_gu][2048] (gate
 * and up rows interleaved, N_gu % 96 == 0) with dev_norm_w bf16 [2048].  Out: dev_x updated in place, dev_y bf16
 * [R][N_gu / 2] row-major = the SwiGLU output. */
int32_t mtts_k_fold_pair(const void* dev_wo, const void* dev_attn, void* dev_x, const void* dev_norm_w, const void* dev_wgu,
                         float eps, int32_t R, int32_t N_gu, void* dev_y, void* stream);
/* pack2_rn (csrc/norm_ops.h: v_cvt_pk_bf16_f32, what resid_norm_kernel and the kernels of gemm_fold.hip round with) against
 * f2bf (csrc/common.h) on all 2^32 fp32 bit patterns: out2 = {inputs that are not NaN on which they differ, NaN inputs on
 * which they differ}.  Both must be 0 (tests/test_bf16_round_gpu.py). */
int32_t mtts_k_bf16_round_check(int64_t* out2, void* stream);
/* launch trains of the seam at H = 2048 over `copies` rotating copies of both weight arrays: mode 0 the three launches
 * (o_proj split-K 4, resid_norm, gate/up), 1 producer + consumer, 10 .. 14 one of those five launches alone; avg_us = one
 * pass through the seam (tools/fold_norm_ab.py) */
int32_t mtts_k_fold_bench(int32_t N_gu, int32_t copies, int32_t iters, int32_t mode, float* avg_us);
/* number of whole-row decode attention launches (attn_row_kernel) of this process; counted like the above */
int64_t mtts_debug_attn_row_launches(void);
/* Test hook: the attention section of one decode layer (fused q/k/v epilogue, scores, P.V, sum of the chunk partials) on
 * given qkv slabs, path 0 = the two-pass kernels + combine, 1 = the whole-row kernel.  dev_slabs fp32 [ksplit][R][(nq +
 * 2 nkv) * 128]; dev_k / dev_v bf16 [R][Lmax][nkv][128] = the tokens already cached (row r: host_lens[r] - 1 of them;
 * host_lens[r] = its length with the new token, 0 = idle row); dev_cos / dev_sin bf16 [Lmax][64]; sealed != 0: complete
 * pages are read in their sealed form.  Out: dev_out bf16 [32][nq*128] (X-fragment layout), the bf16 pools after the
 * launch dev_kcache / dev_vcache [nkv][R*pages][64*128] and (sealed, may be NULL) the sealed pools [nkv][R*pages][13*64*16 B]. */
int32_t mtts_k_attn_section(const float* dev_slabs, int32_t ksplit, const void* dev_qnw, const void* dev_knw, const void* dev_cos,
                            const void* dev_sin, float eps, const void* dev_k, const void* dev_v, const int32_t* host_lens,
                            const int32_t* host_page_table, int32_t R, int32_t Lmax, int32_t nq, int32_t nkv, int32_t sealed,
                            int32_t path, void* dev_out, void* dev_kcache, void* dev_vcache, void* dev_kpack, void* dev_vpack,
                            void* stream);
/* Test hook: the attention section of one PREFILL pass (qkv_post_kernel over many rows of a dialogue, attn_prefill_scores /
 * attn_prefill_pv on 32-row tiles, attn_combine with the prefill chunking) for B dialogues, launched as the engine's
 * prefill launches it (tests/test_attn_prefill_gpu.py).  Dialogue b has host_cached[b] tokens cached (a multiple of 32,
 * 0 <= cached < lens <= Lmax) and the pass carries its tokens cached[b] .. lens[b]-1; every dialogue starts on a 32-row
 * tile boundary (the filler rows are idle), M = sum_b round_up(lens[b] - cached[b], 32) <= 2048, and the hook pads the pass
 * to a multiple of 128 rows with idle tiles.  dev_slabs fp32 [ksplit][M][(nq + 2 nkv) * 128], 1 <= ksplit <= 8; dev_k /
 * dev_v bf16 [B][Lmax][nkv][128]: ALL Lmax tokens go into the pools before the pass (the cached prefix, and whatever the
 * caller wants behind a dialogue's end); dev_cos / dev_sin bf16 [Lmax][64]; host_page_table int32 [B][ceil(Lmax/64)] as
 * in mtts_k_paged_attn_decode.  The q, scores, statistics and chunk-partial scratch starts as 0xff bytes (NaN).
 * Out: dev_out bf16 [M][nq*128] row-major (idle rows: zeros), dev_q bf16 [M][nq][128] (idle rows: 0xff bytes), the bf16
 * pools after the pass dev_kcache / dev_vcache [nkv][B*pages][64*128].  MTTS_EINVAL, with nothing written: a cached
 * that is not a multiple of 32 or not below lens, lens > Lmax, nq % nkv != 0 or a group size other than 1, 2, 4, M > 2048,
 * a page table that is not a permutation.  Synchronous. */
int32_t mtts_k_attn_prefill(const float* dev_slabs, int32_t ksplit, const void* dev_qnw, const void* dev_knw, const void* dev_cos,
                            const void* dev_sin, float eps, const void* dev_k, const void* dev_v, const int32_t* host_lens,
                            const int32_t* host_cached, const int32_t* host_page_table, int32_t B, int32_t Lmax, int32_t nq,
                            int32_t nkv, void* dev_out, void* dev_q, void* dev_kcache, void* dev_vcache, void* stream);
/* The decode path's gate/up GEMM with its SwiGLU epilogue: W[N,K] holds gate and up rows interleaved (row 2i = gate i,
 * row 2i+1 = up i), Y[M,N/2] = bf16(bf16(silu(bf16(gate))) * bf16(up)), row-major.  M <= 128, N % 32 == 0, no split-K.
 * Like mtts_k_gemm_bf16 and mtts_k_gemm_bench it reads MTTS_GEMM_DEPTH on every call (0: gemm_skinny_kernel only). */
int32_t mtts_k_gemm_swiglu_bf16(const void* dev_w, const void* dev_x, void* dev_y,
                                int32_t M, int32_t N, int32_t K, void* stream);
/* RMSNorm (Qwen3RMSNorm, modeling_qwen3.py:59-64): x,w bf16 -> y bf16, rows x n.  Runs rmsnorm_rows_kernel, a
 * test-only entry point that the engine never launches; the kernels the engine runs are reached through
 * mtts_k_embed_norm, mtts_k_resid_norm and mtts_k_gemv_small (tests/test_layer_kernels_gpu.py). */
int32_t mtts_k_rmsnorm(const void* dev_x, const void* dev_w, void* dev_y,
                       int32_t rows, int32_t n, float eps, void* stream);
/* ---- the layer kernels the engine launches, one launch each (tests/test_layer_kernels_gpu.py) ----
 * epi / pro below are the launchers' numbers: epi 0 = fp32 split-K slabs (reduced to bf16 by the hook), 1 = bf16
 * row-major with row stride round_up(N, 32), 2 = SwiGLU into the fragment layout, 3 = SwiGLU row-major (small kernel);
 * pro 1 = residual + slabs + RMSNorm, 2 = sum of the P.V chunk partials, 3 = row-major activations.
 *
 * embed_norm_kernel on R rows: host_tokens int32 [R][8], host_seq int32 [R] (< 0 = idle row), host_tables = 8 device
 * pointers to bf16 [host_vocab[c]][H], dev_norm_w bf16 [H].  Out: dev_x bf16 [R][H] (the residual stream) and dev_xn
 * bf16 [R][H] (the normalised rows, unpacked from the fragment layout).  H % 16 == 0, H <= 8192, 1 <= R <= 2048. */
int32_t mtts_k_embed_norm(const int32_t* host_tokens, const int32_t* host_seq, const void* const* host_tables,
                          const int32_t* host_vocab, const void* dev_norm_w, int32_t R, int32_t H, float eps,
                          void* dev_x, void* dev_xn, void* stream);
/* resid_norm_kernel on R rows: dev_slabs fp32 [ksplit][R][Npad] (Npad = round_up(H, 32)), dev_x bf16 [R][H] updated in
 * place, host_seq / host_last int32 [R] (seq < 0 = idle row, seq < nseq).  Out: dev_xn bf16 [R][H] row-major, and
 * dev_hlast bf16 [nseq][H]: row seq[r] receives the xn row of every row r with last[r] != 0, the rest keeps what the
 * caller put there. */
int32_t mtts_k_resid_norm(const float* dev_slabs, int32_t ksplit, int32_t Npad, void* dev_x, const void* dev_norm_w,
                          const int32_t* host_seq, const int32_t* host_last, int32_t R, int32_t H, int32_t nseq, float eps,
                          void* dev_xn, void* dev_hlast, void* stream);
/* One launch of gemv_small_kernel (decode of 1..4 dialogues) with (epi, pro) in the pairs the engine uses: (0,1) (0,2)
 * (0,3) (3,1) (1,1).  dev_w bf16 [N][K] row-major; the plan is the engine's GEMM planner on round_up(N, 32), K and
 * want_ksplit (which must be 1 unless epi == 0); MTTS_EINVAL when the prologue's LDS exceeds the budget the engine allows.
 * pro 1: dev_x_in bf16 [rows][K], dev_slabs fp32 [slab_ksplit][rows][round_up(K, 32)] (slab_ksplit 0: none), dev_norm_w
 *        bf16 [K]; dev_x_out bf16 [rows][K] receives x' (may be NULL; must not be dev_x_in).
 * pro 2: K = nq * 128, dev_opart fp32 [rows][nq][nchunks_max][128], host_seq / host_pos int32 [rows] (seq < 0 = idle
 *        row; a row sums its first ceil(ceil((pos + 1) / 64) / 8) chunks).
 * pro 3: dev_xrows bf16 [rows][K].
 * Out dev_y bf16: epi 0 [rows][N] (slabs reduced), epi 1 [rows][round_up(N, 32)] (columns < N written), epi 3
 * [rows][N / 2] (N % 32 == 0).  With epi 1 / 3 and for dev_x_out the kernel writes the caller's buffers itself: whatever
 * it must not write keeps its content.  out_plan (may be NULL) receives {waves per block, ksplit} of the launch. */
int32_t mtts_k_gemv_small(int32_t epi, int32_t pro, const void* dev_w, int32_t rows, int32_t N, int32_t K, int32_t want_ksplit,
                          const void* dev_x_in, const float* dev_slabs, int32_t slab_ksplit, const void* dev_norm_w, float eps,
                          void* dev_x_out, const float* dev_opart, const int32_t* host_seq, const int32_t* host_pos, int32_t nq,
                          int32_t nchunks_max, const void* dev_xrows, void* dev_y, int32_t* out_plan, void* stream);
/* gemm_tile_kernel (every prefill pass) on 1 <= M <= 2048 rows, whatever M is: epi 0, Y[M,N] as mtts_k_gemm_bf16
 * (ksplit 0 = the kernel's own choice), or epi 2, Y[M,N/2] as mtts_k_gemm_swiglu_bf16 (ksplit 0 or 1). */
int32_t mtts_k_gemm_tile(int32_t epi, const void* dev_w, const void* dev_x, void* dev_y, int32_t M, int32_t N, int32_t K,
                         int32_t ksplit, void* stream);
/* q/k/v epilogue of one new token per row (per-head q/k RMSNorm, RoPE, K/V page write: transformers modeling_qwen3.py
 * :148-170,251-259): dev_qkv bf16 [R][(nq+2*nkv)*128] = the q|k|v Linear outputs, host_pos int32 [R], norm weights bf16
 * [128], RoPE tables bf16 [rows][64].  Out (bf16): dev_q [R][nq][128], dev_k / dev_v [R][nkv][128] as read back from the
 * cache pages they were written to. */
int32_t mtts_k_rope_kvwrite(const void* dev_qkv, const int32_t* host_pos, const void* dev_qnorm, const void* dev_knorm,
                            const void* dev_cos, const void* dev_sin, int32_t R, int32_t nq, int32_t nkv, float eps,
                            void* dev_q, void* dev_k, void* dev_v, void* stream);
/* Decode attention, one query token per row, over a paged KV cache (eager_attention_forward, modeling_qwen3.py:185-208,
 * with its three bf16 rounding points): dev_q bf16 [R][nq][128]; dev_k / dev_v bf16 [R][Lmax][nkv][128] (row r holds
 * host_lens[r] tokens, the query is the last one); host_page_table int32 [R][ceil(Lmax/64)] = any permutation of the
 * pool's page numbers (NULL: consecutive).  dev_out bf16 [R][nq*128].  R <= 32. */
int32_t mtts_k_paged_attn_decode(const void* dev_q, const void* dev_k, const void* dev_v, const int32_t* host_lens,
                                 const int32_t* host_page_table, int32_t R, int32_t Lmax, int32_t nq, int32_t nkv,
                                 void* dev_out, void* stream);
/* The sealed page format on its own: dev_pages = npages x 16 KiB (a page as the cache holds it: [16 units][64 lanes][16 B]),
 * dev_sealed = npages x 13 KiB ([13 units][64 lanes][16 B]: units 0-7 the low bytes of the lane's 128 values in order,
 * 8-11 one code nibble per value (byte 4j+k: low nibble = value 8j+k, high nibble = value 8j+4+k; code = sign << 3 | index),
 * unit 12 = 8 dictionary bytes ((bf16 >> 8) & 0x7f, ascending), a 32-bit spare, a 32-bit flag: != 0 = the lane did not fit
 * and the rest of its sealed data is undefined).  Lossless: value = sign << 15 | dictionary[index] << 8 | low byte.
 * as_k = 0: the values as they are.  as_k = 1 (K pages: lane = token, value i = dim i): dim d is first divided
 * by 2^s[d], s[d] = (rounded mean of the non-zero exponent fields of dim d over the page's 64 tokens) - 125 (0 for an
 * all-zero dim; clamped to -127..127), lane l keeps s[2l], s[2l+1] as int8 in the low 16 bits of its spare; k = stored value
 * x 2^s[d] exactly (a lane with a denormal, inf / NaN or an exponent that would leave 1..254 is flagged instead).
 * as_k = 2 (V pages: lane = 32 * sub + dl, value 8 it + 2 c + h = token 4 it + 2 sub + h, dim 4 dl + c): token t is first
 * divided by 2^s[t], s[t] = (rounded mean of the non-zero exponent fields of token t's 128 values) - (the smallest such
 * mean of the page), rounded down to even, 0..126 (0 for an all-zero token); lane t keeps s[t] in the low byte of its spare; the same flags. */
int32_t mtts_k_kv_seal(const void* dev_pages, int32_t npages, void* dev_sealed, int32_t as_k, void* stream);
/* The scoring kernels on their own (mtts_score: lm_heads[i] + ForCausalLMLoss per token, modeling_asteroid.py:398-399):
 * dev_w bf16 [N,K] row-major, dev_x bf16 [M,K], host_labels int32 [M * segments] (< 0 = ignore), dev_logp float
 * [M * segments] = log_softmax over the first n_valid columns of bf16(X W^T) at the label, NaN where ignored.
 * segments == 1: one head, n_valid <= N (rows n_valid..N-1 of W are padding the kernel must drop).  segments > 1: the
 * speech-head layout, N = segments * n_valid, head s = rows [s * n_valid, (s + 1) * n_valid), each padded to a multiple
 * of 32 rows in the packed matrix; labels and logp are [M][segments].  M <= 2048, K % 16 == 0. */
int32_t mtts_k_head_ce(const void* dev_w, const void* dev_x, const int32_t* host_labels, int32_t M, int32_t N, int32_t K,
                       int32_t n_valid, int32_t segments, float* dev_logp, void* stream);
/* The top-k kernels of mtts_score_topk on the same operands, launched as the engine launches them (head_topk_kernel in
 * chunks of MTTS_SCORE_TOPK_ROWS rows, topk_finish_kernel): dev_ids int32 and dev_logp float [M * segments * k], entry
 * [(row * segments + s) * k + j].  1 <= k <= MTTS_SCORE_MAX_TOPK and k <= n_valid, else MTTS_EINVAL. */
int32_t mtts_k_head_topk(const void* dev_w, const void* dev_x, int32_t M, int32_t N, int32_t K, int32_t n_valid,
                         int32_t segments, int32_t k, int32_t* dev_ids, float* dev_logp, void* stream);
/* The adapter-merge kernels the engine runs (mtts_bind_weight_lora), into a caller-supplied buffer.  dtype 0: dev_base bf16
 * [rows][cols] -> dev_out packed bf16 [rows_pad][cols] in fragment order, source row s on packed row s * row_mul + row_off;
 * only the 16-byte groups of those rows are written (the rest of dev_out keeps what it held).  dtype 1 / 2: dev_base fp32
 * [rows][cols] -> dev_out fp32 [rows][cols] row-major (2: rounded to fp16 values); the placement arguments are not used.
 * cols % 16 == 0, 1 <= r <= 256, rows_pad % 32 == 0 and (rows - 1) * row_mul + row_off < rows_pad.  Synchronous. */
int32_t mtts_k_lora_pack(const void* dev_base, int32_t rows, int32_t cols, const float* dev_lora_a, const float* dev_lora_b,
                         int32_t r, float scaling, int32_t rows_pad, int32_t row_mul, int32_t row_off, int32_t dtype,
                         void* dev_out, void* stream);
/* The per-row adapter kernels (csrc/multilora.hip) as the engine launches them, on caller buffers.  Synchronous.
 * mtts_k_lora_delta: dev_x bf16 [R][K] row-major (packed by the hook like an activation buffer), R <= 2048, K % 16 == 0.
 * The slab holds the outputs of nseg <= 3 matrices: host_segs int32 [nseg][3] = (col0, ncols, mul), row i of matrix s at
 * column col0 + mul * i; columns of no matrix (up to Npad, % 32 == 0) are padding.  Adapter a's pair for matrix s:
 * host_a / host_b [n_adapters][nseg] device pointers (fp32 [r][K] and [ncols][r]; NULL with r 0: not targeted), host_r and
 * host_scaling [n_adapters][nseg]; host_row_adapter int32 [R]: -1 a row without adapter, -2 an idle row (RowMeta.seq -1).
 * dev_slabs float [..][2048][Npad], the GEMMs' slab stride: slab `ks` gets rows [0, R) x columns [0, Npad) written
 * (mtts.adapters.delta_spec, +0.0 where there is no delta) and nothing else is touched.
 * mtts_k_swiglu_slabs: gate/up as a pass with adapters runs it, on the operands of mtts_k_gemm_swiglu_bf16: the GEMM
 * writes fp32 slab 0 (copied to dev_slab0_out float [M][N] when not NULL), dev_delta float [M][N] (NULL: zeros) is slab 1,
 * swiglu_slabs_kernel -> dev_y bf16 [M][N/2]. */
int32_t mtts_k_lora_delta(const void* dev_x, int32_t R, int32_t K, int32_t Npad, int32_t nseg, const int32_t* host_segs,
                          int32_t n_adapters, const void* const* host_a, const void* const* host_b, const int32_t* host_r,
                          const float* host_scaling, const int32_t* host_row_adapter, float* dev_slabs, int32_t ks, void* stream);
int32_t mtts_k_swiglu_slabs(const void* dev_w, const void* dev_x, const float* dev_delta, void* dev_y, float* dev_slab0_out,
                            int32_t M, int32_t N, int32_t K, void* stream);
/* One sampler call on fp32-from-bf16 logits (HF processors + engine draw). */
int32_t mtts_k_sample(const void* dev_logits_bf16, int32_t rows, int32_t vocab,
                      const void* dev_history_bitmap, const MttsSamplerCfg* cfg,
                      int32_t mask_id, uint64_t seed, int32_t step, int32_t channel,
                      int32_t* dev_tokens, void* stream);
/* The same call that also leaves the log-probability of each row's token (see mtts_set_output_scores) in dev_logp float [rows]. */
int32_t mtts_k_sample_scores(const void* dev_logits_bf16, int32_t rows, int32_t vocab,
                             const void* dev_history_bitmap, const MttsSamplerCfg* cfg,
                             int32_t mask_id, uint64_t seed, int32_t step, int32_t channel,
                             int32_t* dev_tokens, float* dev_logp, void* stream);
/* The same call with the channel's probability floors (mtts_set_sampler_floors; the same value checks).  floors NULL or
 * all zero: the kernels without floors run, bit for bit mtts_k_sample_scores.  dev_logp may be NULL (tokens only). */
int32_t mtts_k_sample_floors(const void* dev_logits_bf16, int32_t rows, int32_t vocab,
                             const void* dev_history_bitmap, const MttsSamplerCfg* cfg,
                             int32_t mask_id, uint64_t seed, int32_t step, int32_t channel,
                             int32_t* dev_tokens, float* dev_logp, const MttsSamplerFloors* floors, void* stream);
/* The same call with a ban bitmap (mtts_set_sampler_bans): dev_ban uint32 [rows][ceil(vocab / 32)], bit i of a row set =
 * token i at -inf.  NULL: the plain call, bit for bit (an all-zero bitmap gives the same results). */
int32_t mtts_k_sample_bans(const void* dev_logits_bf16, int32_t rows, int32_t vocab,
                           const void* dev_history_bitmap, const MttsSamplerCfg* cfg,
                           int32_t mask_id, uint64_t seed, int32_t step, int32_t channel,
                           int32_t* dev_tokens, float* dev_logp, const MttsSamplerFloors* floors, const void* dev_ban,
                           void* stream);
/* The same call with the channel's typical_p (mtts_set_sampler_typical; the same value check).  0 or 1: bit for bit
 * mtts_k_sample_bans, the same kernels. */
int32_t mtts_k_sample_typical(const void* dev_logits_bf16, int32_t rows, int32_t vocab,
                              const void* dev_history_bitmap, const MttsSamplerCfg* cfg,
                              int32_t mask_id, uint64_t seed, int32_t step, int32_t channel,
                              int32_t* dev_tokens, float* dev_logp, const MttsSamplerFloors* floors, const void* dev_ban,
                              float typical_p, void* stream);
/* The ban kernel of a decode step on bare histories, launched as the engine launches it (one block per row): dev_hist
 * int32 [rows][cap], dev_lens int32 [rows] (each 0..cap), n = no_repeat_ngram_size (0..MTTS_NGRAM_MAX; 0: static bans
 * only, no scan), host_static n_static ids (suppress; those outside [0, vocab) are ignored), eos_id banned when eos_on.
 * dev_ban uint32 [rows][ceil(vocab / 32)] is overwritten: whatever it held before the call is gone, bits >= vocab are 0. */
int32_t mtts_k_ngram_ban(const int32_t* dev_hist, const int32_t* dev_lens, int32_t rows, int32_t cap, int32_t n,
                         const int32_t* host_static, int32_t n_static, int32_t vocab, int32_t eos_id, int32_t eos_on,
                         void* dev_ban, void* stream);
/* The rule kernel of a decode step (mtts_set_sampler_bias) on bare histories of one channel, launched as the engine launches
 * it (one block per row): dev_hist / dev_lens as for mtts_k_ngram_ban, host_rules ONE channel's settings (its rules only;
 * the same value checks; rules with an id outside [0, vocab) are ignored).  dev_ban uint32 [rows][ceil(vocab / 32)] keeps
 * what it holds and gains the last token of every matching -inf rule (NULL: allowed when no rule is -inf).  dev_bias_words,
 * the same shape, and dev_bias_tab [rows] are overwritten: whatever they held is gone (both NULL: the -inf rules only). */
int32_t mtts_k_seq_bias(const int32_t* dev_hist, const int32_t* dev_lens, int32_t rows, int32_t cap,
                        const MttsSamplerBias* host_rules, int32_t vocab, void* dev_ban, void* dev_bias_words,
                        MttsBiasTable* dev_bias_tab, void* stream);
/* mtts_k_sample_typical with the bias inputs the rule kernel leaves: dev_bias_words uint32 [rows][ceil(vocab / 32)], bit i of
 * a row set = token i carries the term dev_bias_tab[row] lists for it.  Both NULL: mtts_k_sample_typical bit for bit, the
 * same kernels reading no bias word. */
int32_t mtts_k_sample_bias(const void* dev_logits_bf16, int32_t rows, int32_t vocab,
                           const void* dev_history_bitmap, const MttsSamplerCfg* cfg,
                           int32_t mask_id, uint64_t seed, int32_t step, int32_t channel,
                           int32_t* dev_tokens, float* dev_logp, const MttsSamplerFloors* floors, const void* dev_ban,
                           float typical_p, const void* dev_bias_words, const MttsBiasTable* dev_bias_tab, void* stream);
/* scores_materialize_kernel of the split step (mtts_step_begin) on one logits matrix, launched as the engine launches it
 * (one block per row): dev_scores float [rows][vocab padded to 32] receives, per token, what mtts_k_sample_bias would sample
 * from in front of the temperature -- mask_id, dev_ban and the terms at their places, the repetition penalty of `cfg`
 * where the history bitmap has the token's bit -- and -inf in the pad columns.  dev_ban, dev_bias_words / dev_bias_tab as
 * above, each NULL for none; dev_history_bitmap may be NULL (no penalty). */
int32_t mtts_k_scores_materialize(const void* dev_logits_bf16, int32_t rows, int32_t vocab, const void* dev_history_bitmap,
                                  const MttsSamplerCfg* cfg, int32_t mask_id, int32_t step, int32_t channel, const void* dev_ban,
                                  const void* dev_bias_words, const MttsBiasTable* dev_bias_tab, float* dev_scores, void* stream);
/* The kernels of mtts_set_top_logprobs on bare logits, launched as the engine launches them (the slice pass and the merge
 * when vocab > 4096, the single-block path otherwise): dev_logits [rows][vocab] bf16 bits, or fp32 when is_f32; mask_id
 * the one id at -inf (-1: none); dev_decisions int32 [rows].  dev_logp float [rows] = log_softmax(L)[decision],
 * dev_top_ids int32 and dev_top_logp float [rows][k].  rows <= 128, 1 <= k <= MTTS_SCORE_MAX_TOPK and k <= vocab,
 * else MTTS_EINVAL; a decision outside [0, vocab) gives NaN in dev_logp.  Synchronous. */
int32_t mtts_k_gen_topk(const void* dev_logits, int32_t is_f32, int32_t rows, int32_t vocab, int32_t mask_id,
                        const int32_t* dev_decisions, int32_t k, float* dev_logp, int32_t* dev_top_ids, float* dev_top_logp,
                        void* stream);

/* ======================================================================================
 * XY_Tokenizer decode path (codes -> 24 kHz waveform), fp32.
 * Replaces XY_Tokenizer.inference_detokenize (XY_Tokenizer/xy_tokenizer/model.py:104-128);
 * the 30 s-window / 20 s-stride scheduling of XY_Tokenizer.decode (model.py:195-256) stays
 * in the host mirror, which calls mtts_codec_detokenize once per window batch.
 * ====================================================================================== */
typedef struct MttsCodecConfig {       /* decode-side fields of xy_tokenizer_config.yaml */
    int32_t nq, codebook_size, rvq_dim, quant_out_dim;
    int32_t adapter_layers, adapter_dim, adapter_heads, adapter_ffn, adapter_max_pos;
    int32_t up_stride;
    int32_t dec_layers, dec_dim, dec_heads, dec_ffn, dec_max_pos, mel_bins;
    int32_t voc_dim, voc_inter, voc_layers, n_fft, hop;
    /* encode side (voice-clone prompts) */
    int32_t mel_n_fft, mel_hop, mel_frames;
    int32_t enc_layers, enc_dim, enc_heads, enc_ffn, enc_max_pos;
    int32_t sem_adapter_layers, pre_rvq_layers, down_pool;
} MttsCodecConfig;

typedef struct MttsCodec MttsCodec;
const char* mtts_codec_last_error(void);
int32_t mtts_codec_create(const MttsCodecConfig* cfg, int32_t device, MttsCodec** out);
int32_t mtts_codec_destroy(MttsCodec* c);
/* Bind one fp32 tensor by role name (role <- reference state-dict key and the
 * re-layout applied); the engine copies it. */
int32_t mtts_codec_bind(MttsCodec* c, const char* role, const float* dev_f32, int64_t n, void* stream);
/* dev_codes int64 [nq][B][T] (T <= 375), host_lens int32 [B]; dev_wav f32 [B][T*1920]. Synchronous. */
int32_t mtts_codec_detokenize(MttsCodec* c, const int64_t* dev_codes, const int32_t* host_lens, int32_t B, int32_t T,
                              float* dev_wav, void* stream);
/* Enqueue-only form (overlap with the decode loop on another stream); mtts_codec_check() synchronises and
 * reports a code index outside the codebook. */
int32_t mtts_codec_detokenize_async(MttsCodec* c, const int64_t* dev_codes, const int32_t* host_lens, int32_t B, int32_t T,
                                    float* dev_wav, void* stream);
int32_t mtts_codec_check(MttsCodec* c, void* stream);
/* Encode one chunk (<= 30 s of 16 kHz audio) per row.  Replaces XY_Tokenizer.inference_tokenize
 * (XY_Tokenizer/xy_tokenizer/model.py:55-101), log-mel included.  dev_wav f32 [B][nsamp] zero padded,
 * host_lens int32 [B]; dev_codes int64 [nq][B][375]; host_code_lens int32 [B] (out).  Synchronous. */
int32_t mtts_codec_tokenize(MttsCodec* c, const float* dev_wav, const int32_t* host_lens, int32_t B, int32_t nsamp,
                            int64_t* dev_codes, int32_t* host_code_lens, void* stream);
/* unit test: C[M,N] = act(A[M,K] * W[N,K]^T + bias); act 0 none, 1 GELU(erf); act | 0x100: the decode direction's
 * bf16x3 kernel instead of the exact-f32 MFMA */
int32_t mtts_k_gemm_f32(const float* dev_a, const float* dev_w, const float* dev_bias, float* dev_c,
                        int32_t M, int32_t N, int32_t K, int32_t act, void* stream);
/* Tuning hook: time the decoder's pre-split bf16x3 GEMM (gemm_b3t_kernel) alone on synthetic operands.
 * flags: 1 GELU | 2 gamma | 4 residual | 8 fragment-packed output (the decoder uses 0, 4, 6, 9); tile_code 0 = the
 * production choice for the shape, else NA NB U OCC as decimal digits.  No reference counterpart. */
int32_t mtts_k_gemm_planes_bench(int32_t M, int32_t N, int32_t K, int32_t flags, int32_t tile_code, int32_t iters,
                                 float* avg_us, int32_t* code_used);

/* ---- unit test: the codec's kernels, one launch function of the engine each -------------------------------------
 * All buffers are caller-owned device memory unless named host_*; scratch is allocated and freed inside; every entry
 * returns after the stream is idle.  "Planes" are bf16 hi / lo planes in MFMA-fragment order (element (r, k) of a
 * matrix with rows of K elements at ((r/32) 32 K + ((k/16) 64 + r%32 + 32 ((k%16)/8)) 8 + k%8); hi plane first, the lo
 * plane pad32(rows) * K elements further, pad32(r) = r rounded up to 32).
 *
 * Attention of one transformer layer, head dim 64: qkv f32 [B][T][3 d], d = 64 heads; host_lens int32 [B], each 0 .. T.
 * mode 0: S = q k^T / 8 (exact f32), masked softmax, P V in three launches; 1: the fused kernel; 2: K / V packed once,
 * then the fused kernel on the planes.  A valid query (t < len) attends to keys < len, a padded one uniformly to all T.
 * att: f32 [B][T][d], or with planes != 0 (modes 1, 2) planes of B T rows x d, in a buffer of pad32(B T) d floats. */
int32_t mtts_k_codec_attn(const float* dev_qkv, const int32_t* host_lens, float* dev_att, int32_t B, int32_t T, int32_t heads,
                          int32_t mode, int32_t planes, void* stream);
/* The pre-split bf16x3 GEMM (gemm_b3t_kernel) through the engine's argument builder: rows row0 .. row0 + M - 1 of
 * C = epi(A W^T).  A f32 [R][K] and W f32 [N][K] are split and packed here, R = plane_rows, or M when plane_rows = 0
 * (then row0 = 0).  flags: 1 GELU | 2 * gamma | 4 + residual | 8 plane output, one of 0, 4, 6, 9, with gamma / res null
 * exactly when their flag is clear; epilogue order + bias (may be null), GELU, * gamma, + res.  C and res: f32 [R][ldc];
 * with flag 8 C holds planes of R rows x N.  Needs K % 64 = 0, N % 4 = 0, row0 % 32 = 0, plane_rows >= row0 + M,
 * ldc % 4 = 0, ldc >= N, and for plane output ldc = N, N % 16 = 0.  tile: 0 = the production choice, else NA NB U OCC
 * as decimal digits; nt_out: nontemporal stores of the GELU planes, as MTTS_CODEC_NT_OUT. */
int32_t mtts_k_codec_gemm_planes(const float* dev_a, const float* dev_w, const float* dev_bias, const float* dev_gamma,
                                 const float* dev_res, float* dev_c, int32_t M, int32_t N, int32_t K, int32_t ldc, int32_t flags,
                                 int32_t tile, int32_t row0, int32_t plane_rows, int32_t nt_out, void* stream);
/* The fused Vocos pointwise pair: h[M][512] += gamma * (W2 GELU(W1 xn + b1) + b2), xn f32 [M][512], W1 [4096][512],
 * W2 [512][4096]; xn and both weights are split and packed here (W2 in the kernel's permuted K order). */
int32_t mtts_k_codec_vocos_pw(const float* dev_xn, const float* dev_w1, const float* dev_b1, const float* dev_w2,
                              const float* dev_b2, const float* dev_gamma, float* dev_h, int32_t M, void* stream);
/* layernorm_kernel: y[r][0..C) = LN(x[r]) w + b over C <= 1024 channels, row stride ldy >= C.  host_lens (may be null):
 * int32 [rows / T]; row r with r % T >= lens[r / T] is written as zeros.  planes != 0: planes of rows x C instead of
 * fp32 (ldy = C, C % 16 = 0), in a buffer of pad32(rows) C floats. */
int32_t mtts_k_codec_layernorm(const float* dev_x, const float* dev_w, const float* dev_b, float* dev_y, int32_t rows, int32_t C,
                               float eps, const int32_t* host_lens, int32_t T, int32_t ldy, int32_t planes, void* stream);
/* layernorm_wide_kernel: one block per row, any C; y f32 [rows][C]. */
int32_t mtts_k_codec_layernorm_wide(const float* dev_x, const float* dev_w, const float* dev_b, float* dev_y, int32_t rows,
                                    int32_t C, float eps, void* stream);
/* Depthwise Conv1d(k = 7, pad 3) per window + bias + LayerNorm: h f32 [B][T][C], dw [7][C].  kernel: 0 = the kernel
 * for any C <= 1024, 4 / 8 = the C = 512 kernel with that many rows per wave.  y: f32 [B T][C], or with planes != 0
 * planes of B T rows x C (C % 16 = 0) in a buffer of pad32(B T) C floats. */
int32_t mtts_k_codec_dwconv_ln(const float* dev_h, const float* dev_dw, const float* dev_dwb, const float* dev_lw,
                               const float* dev_lb, float* dev_y, int32_t B, int32_t T, int32_t C, float eps, int32_t kernel,
                               int32_t planes, void* stream);
/* softmax_mask_kernel in place on S f32 [B][heads][T][ldT], ldT % 16 = 0, ldT >= T: masking as mtts_k_codec_attn,
 * columns T .. ldT - 1 are written as zeros.  The kernel takes its loop branch when ldT > 2048. */
int32_t mtts_k_codec_softmax_mask(float* dev_s, const int32_t* host_lens, int32_t B, int32_t heads, int32_t T, int32_t ldT,
                                  void* stream);
/* One RVQ stage of the encoder: per row (b, t) with t < lens[b], code = argmin_j (|r|^2 - 2 dot[row][j]) + cc[j], first
 * index on ties, and residual[row] -= cb[code]; other rows keep their residual and get the code of dot = |r|^2 = 0.
 * dot f32 [B T][K], cb [K][D], cc [K], residual [B T][D] (in / out), codes int64 [B T] (out). */
int32_t mtts_k_codec_vq_argmin_update(const float* dev_dot, const float* dev_cb, const float* dev_cc, float* dev_residual,
                                      int64_t* dev_codes, const int32_t* host_lens, int32_t B, int32_t T, int32_t K, int32_t D,
                                      void* stream);
/* The exact-f32 GEMM in its general form: for z < batch, zo = z / batch_inner, zi = z % batch_inner,
 * C_z[m][n] = ((sum_k A_z[m][k] W_z[..]) + bias[n]) * scale -> GELU(erf) if act -> * gamma[n] -> + res[m' ][n], with
 * W_z[n][k] (b_kn = 0) or W_z[k][n] (b_kn = 1), m' = m % res_rows (res_rows = 0: m), X_z = X + zo s_o + zi s_i and
 * host strides = {sAo, sAi, sWo, sWi, sCo, sCi}.  bias, gamma, res may be null.  lda, ldw and the A / W strides must be
 * multiples of 4 (16-byte loads). */
int32_t mtts_k_codec_gemm_f32_ex(const float* dev_a, const float* dev_w, float* dev_c, const float* dev_bias,
                                 const float* dev_gamma, const float* dev_res, int32_t M, int32_t N, int32_t K, int32_t b_kn,
                                 int64_t lda, int64_t ldw, int64_t ldc, int64_t ldres, int32_t res_rows, int32_t act, float scale,
                                 int32_t batch, int32_t batch_inner, const int64_t* host_strides, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MTTS_H */
