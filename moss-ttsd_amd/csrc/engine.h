// What engine.hip (engine object, C ABI of the product path) and hooks.hip (per-kernel test / bench entry points)
// share: the engine's definition, error reporting, and the owner of device memory.  Only these two files include it.
// The HIP-free host code sits apart, where a CPU test can include it: kvpool.h (the KV page pool; through launch.h),
// staging.h (prompt staging; engine.hip, and hooks.hip for the static ban bitmap), stepplan.h (how a pass chooses its kernels) and runstate.h (the options a
// run starts with, the addresses a captured step holds, the captured steps; both included here) -- besides those includers
// only tests/host/pool_stage_main.cpp, tests/host/step_plan_main.cpp and tests/host/run_state_main.cpp.
//
// Device memory after mtts_engine_create: every mem.release, and every mem.get, targets either a member of StepBufs
// (runstate.h; MttsEngine::bufs) -- which is part of what a captured step is found by, so no reallocation has to remember
// the captured steps -- or a buffer whose address no launch of a decode step carries, and says so where it does: the
// prefill staging, the sc_* scoring buffers, an adapter's matrices (a step finds those through the table in bufs.d_bank).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "launch.h"
#include "runstate.h"
#include "stepplan.h"

static_assert(RUN_EINVAL == MTTS_EINVAL, "runstate.h reports with MTTS_EINVAL");

// ---- errors -------------------------------------------------------------------
#define MTTS_LOCAL __attribute__((visibility("hidden")))
extern MTTS_LOCAL thread_local char g_err[512];          // engine.hip; mtts_last_error() of the calling thread
// int fail(int code, const char* fmt, ...): declared by kvpool.h (the pool reports through it), defined in engine.hip
#define HIPCHK(x)                                                                          \
    do {                                                                                   \
        hipError_t _e = (x);                                                               \
        if (_e != hipSuccess) return fail(MTTS_EHIP, "%s: %s (%s:%d)", #x, hipGetErrorString(_e), __FILE__, __LINE__); \
    } while (0)
#define TRY(x)             \
    do {                   \
        int _r = (x);      \
        if (_r) return _r; \
    } while (0)

static inline int round_up(int a, int b) { return (a + b - 1) / b * b; }
static inline hipStream_t S(void* s) { return (hipStream_t)s; }
// Sealed weight streams, MTTS_W_SEAL=1: a kind's decode GEMMs read the twin while at most this share of its groups did not
// seal (gate/up, down_proj, head 0, heads 1-7).  A group that did not seal costs its wave more round trips in kernels that
// are one round trip long, so the bounds are small; each is the largest share at which the sealed launch train still beat
// the bf16 one by more than the spread of both (profiles/wseal_ab.json).  gate/up did not beat it at the
// share Gaussian weights have (1 group in 3 072): negative = never, and no twin is kept for it.
static const double WSEAL_MAX_UNSEALED[4] = {-1.0, 1.0 / 512, 1.0 / 8, 1.0 / 64};

template <typename T>
static int dalloc(T** p, size_t n, bool zero = true) {
    HIPCHK(hipMalloc((void**)p, n * sizeof(T)));
    if (zero) HIPCHK(hipMemset(*p, 0, n * sizeof(T)));
    return 0;
}

// Owner of device and pinned host memory (the engine's, or a test hook's): what it handed out is freed when it dies,
// or earlier by release().  The first free that does not succeed is kept, so that a double or stale free is reported
// (mtts_engine_destroy) instead of passing silently.
struct DevBufs {
    struct Buf { void* p; bool pinned; };
    std::vector<Buf> bufs;
    std::string free_error;
    DevBufs() = default;
    DevBufs(const DevBufs&) = delete;
    DevBufs& operator=(const DevBufs&) = delete;
    ~DevBufs() { free_all(); }
    template <typename T>
    int get(T** out, size_t n, bool zero = true) {
        TRY(dalloc(out, n, zero));
        bufs.push_back({(void*)*out, false});
        return 0;
    }
    template <typename T>
    int get_pinned(T** out, size_t n) {             // zeroed
        HIPCHK(hipHostMalloc((void**)out, n * sizeof(T)));
        bufs.push_back({(void*)*out, true});
        memset((void*)*out, 0, n * sizeof(T));
        return 0;
    }
    // free now (a buffer that is being reallocated); null is fine, a pointer this owner does not hold is an error
    template <typename T>
    void release(T*& p) {
        if (!p) return;
        auto it = std::find_if(bufs.begin(), bufs.end(), [&](const Buf& b) { return b.p == (void*)p; });
        if (it == bufs.end()) note(hipErrorInvalidValue, (void*)p);
        else { free_one(*it); bufs.erase(it); }
        p = nullptr;
    }
    void free_all() {
        for (const Buf& b : bufs) free_one(b);
        bufs.clear();
    }
private:
    void free_one(const Buf& b) {
        const hipError_t r = b.pinned ? hipHostFree(b.p) : hipFree(b.p);
        if (r != hipSuccess) note(r, b.p);
    }
    void note(hipError_t r, void* p) {
        if (!free_error.empty()) return;
        char msg[160];
        snprintf(msg, sizeof(msg), "freeing %p: %s", p, hipGetErrorString(r));
        free_error = msg;
    }
};

// ---- sampler scratch (sampler.hip: SampleScratch) --------------------------------------------------------------
static inline int full_cap_for(int vocab) { int p = 1; while (p < vocab) p <<= 1; return vocab > SAMP_CAND ? p : 0; }
static inline int alloc_scratch(DevBufs& m, SampleScratch& sc, int rows, int vocab) {
    const int fc = full_cap_for(vocab);
    TRY(m.get(&sc.overflow, (size_t)rows));
    if (fc) {            // full-vocabulary path (sampling without top_k): per token a key and a level-0 bin, per row the level-0 histogram
        TRY(m.get(&sc.full_val, (size_t)rows * fc, false));
        TRY(m.get(&sc.full_idx, (size_t)rows * fc, false));
        TRY(m.get(&sc.nuc_cnt, (size_t)rows * 2048));
        TRY(m.get(&sc.nuc_mass, (size_t)rows * 2048));
    }
    TRY(m.get(&sc.hist, (size_t)rows * 2048));
    TRY(m.get(&sc.slice_val, (size_t)rows * SAMP_NS));
    TRY(m.get(&sc.slice_idx, (size_t)rows * SAMP_NS));
    TRY(m.get(&sc.cand_val, (size_t)rows * SAMP_CAND));
    TRY(m.get(&sc.cand_idx, (size_t)rows * SAMP_CAND));
    TRY(m.get(&sc.cand_n, (size_t)rows));
    return 0;
}

// ---- the engine ------------------------------------------------------------------------------------------------
struct Layer {
    void *wqkv = nullptr, *wo = nullptr, *wgu = nullptr, *wd = nullptr;     // packed
    void *wgu_s = nullptr, *wd_s = nullptr;                                 // their sealed twins (gemm_sealed.hip), or null
    void *ln_in = nullptr, *ln_post = nullptr, *qn = nullptr, *kn = nullptr; // bf16 vectors
    int bound = 0;
};

enum { PROF_SCORES = 0, PROF_PV = 1, PROF_GEMM = 2, PROF_STEP = 3,
       PROF_CE = 4,          // mtts_score: head_ce_kernel + ce_finish_kernel of a pass (both launches of the 8 heads); mtts_score_topk: its kernels
       PROF_N = 5 };

struct MttsEngine {
    DevBufs mem;                        // owns every device / pinned pointer below
    MttsConfig cfg;
    int device = 0;
    int H, I, L, nq, nkv, V0, Vs, Vs_pad, V0_pad, qkv_rows;
    std::vector<Layer> layers;
    void* emb[8] = {nullptr};          // row-major tables (gather)
    void* head0 = nullptr;             // packed [V0_pad][H]
    void* heads17 = nullptr;           // packed [7*Vs_pad][H]
    void* final_norm = nullptr;
    int emb_bound = 0, norm_bound = 0;
    const uint16_t** d_tables = nullptr;
    // plans
    GemmPlan p_qkv, p_o, p_gu, p_d, p_h0, p_h17;
    // workspaces
    // (the qkv / o_proj / down_proj split-K slabs `partial` are in bufs: the first adapter load widens them)
    float* partial2 = nullptr;          // small-batch path: o_proj / down_proj slabs (the qkv slabs stay in `partial`)
    void *x2 = nullptr, *act_rm = nullptr;   // small-batch path: second residual buffer (ping-pong), row-major SwiGLU output
    // how a pass chooses its kernels (stepplan.h): the switches of the environment as read at creation (attn_row and
    // kv_pack go to 0 there when the device refuses what they need), and what is fixed from then on
    StepKnobs knobs;
    StepCaps caps;
    void* xres_p = nullptr;             // gemm_fold.hip: the x' o_proj hands to gate/up, one 32-row tile in the X-fragment layout
    // Sealed weight streams (gemm_sealed.hip): gate/up, down_proj and the heads also exist in the sealed
    // 13-bit form, made by every bind of such a matrix on the bind's stream, and the one-row-tile decode GEMMs read that
    // instead of the bf16 array.  MTTS_W_SEAL: 0 never (no twin is allocated), 1 per matrix kind by the share of groups that
    // did not seal (counted at mtts_weights_ready after a bind; WSEAL_MAX_UNSEALED above), 2 whenever the shape fits.
    void *head0_s = nullptr, *heads17_s = nullptr;
    int wseal_ktw[WSEAL_KINDS] = {0, 0, 0, 0};      // k-tiles per sealed group of each kind (0: the kind has no twin)
    bool wseal_dirty = false;           // a matrix with a twin was bound since the last count
    char wseal_on[WSEAL_KINDS] = {0, 0, 0, 0};      // the kind's decode GEMMs read the twin (decided at mtts_weights_ready)
    unsigned long long *d_wseal_cnt = nullptr, *h_wseal_cnt = nullptr;     // per kind {groups, groups not sealed}
    void *x = nullptr, *xn = nullptr, *attn_p = nullptr, *act_p = nullptr, *qbuf = nullptr, *hlast = nullptr, *xh = nullptr;
    void *logits0 = nullptr, *logits17 = nullptr, *join_logits0 = nullptr, *join_logits17 = nullptr;
    void* scores = nullptr;
    float *stats = nullptr, *opart = nullptr;
    // kv
    void *kcache = nullptr, *vcache = nullptr;
    size_t layer_stride = 0;           // elements per layer in each cache
    int total_pages = 0, max_pages = 0, nchunks_max = 0;
    int32_t* d_page_table = nullptr;
    // KV page pool (kvpool.h): pages are handed out on demand as a dialogue's length crosses a page boundary and come back
    // when it finishes; max_pages / total_pages above are its sizes, set once beside it (kernel arguments)
    KvPool pool;
    std::vector<char> slot_live;        // host's view: the slot holds a dialogue that may still step
    int forced_draw = 0;
    PendingRun pending;                 // what the mtts_set_* calls left for the next run (runstate.h)
    StepBufs bufs;                      // every address a decode step reads that can change after creation (runstate.h)
    int takes = 1;                      // of the current static run: row b*takes+j is take j of prompt b
    // ---- MTTS_DTYPE_F32 engine (f32path.hip): plain fp32 copies of everything, no packed layouts ----
    bool f32 = false;
    int h16 = 0;                        // MTTS_DTYPE_F16: the fp32 engine with fp16 rounding points (f32path.hip: r16)
    struct LayerF32 { float *wqkv = nullptr, *wo = nullptr, *wgu = nullptr, *wd = nullptr, *ln_in = nullptr, *ln_post = nullptr, *qn = nullptr, *kn = nullptr; };
    std::vector<LayerF32> lf;
    float* embf[8] = {nullptr};
    const float** d_tables_f = nullptr;
    float* final_norm_f = nullptr;
    float *kcache_f = nullptr, *vcache_f = nullptr;
    float *xf = nullptr, *xnf = nullptr, *qkvf = nullptr, *qbuf_f = nullptr, *attnf = nullptr, *yf = nullptr, *guf = nullptr,
          *actf = nullptr, *hlast_f = nullptr, *scores_f = nullptr;
    // generation state
    SeqState* d_seqs = nullptr;
    RowMeta* d_meta = nullptr;          // decode rows
    LoopState* d_ls = nullptr;
    LoopState* h_ls = nullptr;          // pinned mirror
    SeqState* h_seqs = nullptr;         // pinned mirror of d_seqs (mtts_sync_state)
    int32_t *d_decisions = nullptr, *d_cur = nullptr, *d_tf = nullptr;
    uint32_t* d_bitmaps = nullptr;
    int bm_words = 0;
    MttsSamplerCfg* d_scfg = nullptr;
    MttsSamplerFloors* d_floors = nullptr;      // [8], allocated with the engine: a captured step may hold the address
    int floors_on = 0;                  // of the current run: a sampled channel has a probability floor (mtts_set_sampler_floors)
    float* d_typical = nullptr;         // [8] typical_p per channel (0: absent), allocated with the engine like d_floors
    int typical_on = 0;                 // of the current run: a sampled channel has a typical_p (mtts_set_sampler_typical)
    BanCfg* d_bancfg = nullptr;         // [8], allocated with the engine like d_floors (launch.h: launch_ban)
    int bans_on = 0;                    // of the current run: a channel has a hard ban (mtts_set_sampler_bans; the buffers are in bufs)
    int ban_ngram_on = 0;               // ... an n-gram ban: submits stage the prompt's slots into bufs.d_hist
    int ban_begin_on = 0;               // ... begin_suppress_tokens (mtts_set_sampler_bias): bufs.d_ban_begin appears
    int bias_on = 0, bias_terms = 0;    // of the current run: a channel has a sequence rule / a finite one (mtts_set_sampler_bias)
    int hist_on = 0;                    // ban_ngram_on, or a rule longer than one token: the prompt history is staged
    SampleScratch sscr;                 // (its slice_sum / lp / ban stay null here: bufs holds them)
    int ch0_sampled = 0;
    // output_scores: per-token log-probabilities (bufs.d_lp, laid out like bufs.d_gen)
    int scores_on = 0;                  // of the current run
    bool run_open = false;              // a run has begun and has not been seen to end (mtts_set_output_scores)
    // top_logprobs (gen_topk.hip): raw log-probability of every decision and the k most probable tokens (bufs.d_gt_*)
    int topk_on = 0;                    // k of the current run (0: off)
    // teacher-forced scoring (mtts_score; score.hip): allocated by the first call, grown by later ones; no decode step reads any of it
    int32_t* d_sc_labels = nullptr;     // [staged rows][8]: the label of the row's NEXT position, -100 = none
    float* d_sc_logp = nullptr;         // [staged rows][8]
    size_t sc_cap_rows = 0;
    float* sc_part = nullptr;           // bf16 engine: (m, s, l_label) per row of a pass and 128-column block, head 0 then heads 1..7
    float* sc_logits = nullptr;         // fp32 / fp16 engines: fp32 logits of SCORE_F32_ROWS rows of one head
    // mtts_score_topk only: allocated by the first such call
    int32_t* d_sc_top_ids = nullptr;    // [staged rows][8][k]
    float* d_sc_top_logp = nullptr;
    size_t sc_top_cap = 0;              // elements of each
    uint32_t* sc_cand = nullptr;        // bf16 engine: every block's k candidate keys of MTTS_SCORE_TOPK_ROWS rows of one head launch
    // resident adapters, one per dialogue (mtts_adapter_load; multilora.hip): no device memory before the first load
    std::vector<LoraEnt> bank;          // host copy of bufs.d_bank [MTTS_MAX_ADAPTERS][L * 7]; r == 0: the adapter has no pair for the matrix
    int bank_pairs[MTTS_MAX_ADAPTERS] = {0};     // matrix pairs each adapter holds (0: the adapter is empty)
    // bufs.d_seq_adapter [MTTS_RCAP]: adapter of the dialogue in each sequence slot (-1: none); kernels go RowMeta.seq -> there
    std::vector<int32_t> seq_adapter = std::vector<int32_t>(MTTS_RCAP, -1);          // the host's copy
    int32_t* d_pf_tokens = nullptr;     // prefill staging: grows with the prompts; read by prefill passes, never by a decode step
    RowMeta* d_pf_meta = nullptr;
    size_t pf_cap_rows = 0;
    // current run
    int B = 0, T = 0, base_length = 0, max_length = 0, max_steps = 0, steps_issued = 0;
    bool continuous = false;
    std::vector<int> join_step;         // engine step at which each slot's dialogue joined
    std::vector<int> n_real;
    int max_real = 0;
    uint64_t seed = 0;
    bool began = false, has_forced = false;
    // the split step (mtts_step_begin / mtts_step_sample / mtts_step_finish): which half comes next, and what the halves share
    int split_phase = 0;                // 0: between steps; 1: mtts_step_begin has run; 2: mtts_step_sample has run
    float *split_scores0 = nullptr, *split_scores17 = nullptr;     // the caller's score rows of the step in flight
    // decode-step graphs: one captured step per (plan, KV page bound, bufs), replayed by mtts_step
    struct DestroyExec { void operator()(hipGraphExec_t g) const { hipGraphExecDestroy(g); } };
    StepGraphs<hipGraphExec_t, DestroyExec> graphs;
    hipStream_t cap_stream = nullptr;
    // sealed KV pages (attn.hip: kv_seal): every COMPLETE page also kept in a lossless 13-bit form the decode attention
    // reads instead of the bf16 page (MTTS_KV_PACK=0: off, no second pool)
    void *kpack = nullptr, *vpack = nullptr;
    size_t pk_layer_stride = 0;         // bytes per layer of a sealed pool
    // read policy: a page that did not seal costs a wasted sealed read + the bf16 read (29 units instead of 16), so a
    // layer whose K (or V) pages stop sealing (more than 1 in 8 since mtts_begin) goes back to bf16 reads; the sealer
    // counts per layer {K sealed, K not, V sealed, V not}, mtts_sync_state looks at the counts (MTTS_KV_PACK=2: no policy)
    unsigned long long *d_seal_cnt = nullptr, *h_seal_cnt = nullptr;
    std::vector<char> pack_k_on, pack_v_on;
    // profiling
    bool prof = false;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev[PROF_N];
    int64_t prof_bytes[PROF_N] = {0, 0, 0, 0, 0};
};

// a decode step of the current run carries adapters: a row of it has one
static inline bool rows_carry_adapters(const MttsEngine* e) {
    for (int b = 0; b < e->B; ++b)
        if (e->seq_adapter[b] >= 0) return true;
    return false;
}
// What plan_step is asked about a pass of R rows: the run's options and the two read policies as they stand now.  The
// only place that gathers one.
static inline StepState step_state(const MttsEngine* e, int heads, int R, int pages_bound, bool lora, bool split = false) {
    StepState s;
    s.heads = heads; s.B = e->B; s.R = R; s.pages_bound = pages_bound; s.lora = lora;
    s.forced = e->has_forced; s.ch0_sampled = e->ch0_sampled != 0; s.scores_on = e->scores_on != 0; s.floors_on = e->floors_on != 0; s.typical_on = e->typical_on != 0;
    s.bans_on = e->bans_on != 0; s.bias_on = e->bias_on != 0; s.bias_terms = e->bias_terms != 0;
    s.topk = e->topk_on; s.split = split;
    for (int k = 0; k < WSEAL_KINDS; ++k) s.wseal_on[k] = e->wseal_on[k] != 0;
    if (e->kpack) s.pack_k_on = e->pack_k_on.data();
    if (e->vpack) s.pack_v_on = e->pack_v_on.data();
    return s;
}
// the plan of the decode step the engine would run now at this page bound
// (split: the step issued in halves, mtts_step_begin / mtts_step_finish)
static inline StepPlan decode_plan(const MttsEngine* e, int pages_bound, bool split = false) {
    return plan_step(e->knobs, e->caps, step_state(e, 1, round_up(e->B, 32), pages_bound, rows_carry_adapters(e), split));
}

// layer n's sealed pools, each null where the plan says bf16 pages
static inline KvPack layer_pack(const MttsEngine* e, const StepPlan& plan, int n) {
    const LayerPlan& l = plan.layers[n];
    return KvPack{l.k_sealed ? (uint8_t*)e->kpack + e->pk_layer_stride * n : nullptr,
                  l.v_sealed ? (uint8_t*)e->vpack + e->pk_layer_stride * n : nullptr};
}
