// How a pass chooses its kernels.  plan_step is a pure function of three structs -- the switches read from the environment
// (StepKnobs), what is fixed once the engine exists (StepCaps) and what varies from pass to pass (StepState) -- and its
// result says everything the engine branches on: forward_rows, forward_small and attend_layer (engine.hip) execute a
// StepPlan and hold no policy of their own.  The plan of a decode step is also the key of its captured graph: two steps
// replay the same graph exactly when their plans compare equal, so a path that joins the plan cannot be forgotten in the key.
// No HIP in here: engine.h includes it (and runstate.h, whose cache of captured steps holds plans), and so does
// tests/host/step_plan_main.cpp, which runs it on the CPU.
#pragma once
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "shapes.h"

// ---- the switches ---------------------------------------------------------------------------------------------------
// MTTS_FOLD_NORM: the one-row-tile decode step runs o_proj -> post-attention norm -> gate/up as the two launches of
// gemm_fold.hip instead of three (same bits).
#define MTTS_FOLD_NORM_DEFAULT 0
struct StepKnobs {
    int small_rows = SMALL_RP;      // MTTS_SMALL_ROWS: decode batches up to this many dialogues take the small-batch path (0 = off)
    int fuse_qkv_max = 2560;        // MTTS_FUSE_QKV_MAX: q/k/v epilogue inside the attention kernels while rows x KV pages <= this
                                    // (32 rows x 80 pages: wins at 32 x 64, loses at 64 x 64)
    int pack_min_work = 512;        // MTTS_KV_PACK_MIN: sealed KV reads from this many rows x KV pages up.  Below it the passes are
                                    // latency-bound and the unpack sits on the critical path (B=1 at 2 k: +4 %; break-even at
                                    // 8 rows x 64 pages, -6 % at 16 x 64: profiles/r03_kv_pack_ab.txt)
    int attn_row = 1;               // MTTS_ATTN_ROW: whole-row decode attention 0 never, 1 by the shape (attn_row_auto), 2 whenever it fits
    int pf_mfma_pages = 0;          // MTTS_PREFILL_MFMA_PAGES: prefill attention on the tile-sharing MFMA kernels from this many KV
                                    // pages up (0 = always; a dialogue's numerics must not depend on its batch)
    int gemm_depth = 1;             // MTTS_GEMM_DEPTH=0: every decode GEMM runs gemm_skinny_kernel (no sealed reads, no fold either)
    int fold_norm = MTTS_FOLD_NORM_DEFAULT;
    int w_seal = 1;                 // MTTS_W_SEAL: sealed weight streams 0 never, 1 per kind by the share of groups that sealed, 2 whenever the shape fits
    int w_seal_head = 1;            // MTTS_W_SEAL_HEAD: the heads' sealed kernel 1 persistent over N-tiles, 0 one tile per block (a tuning aid)
    int kv_pack = 1;                // MTTS_KV_PACK: sealed KV pages 0 off (no second pool), 1 with the per-layer read policy, 2 without it
    bool use_graphs = true;         // MTTS_GRAPHS=0: every step is launched on the stream
};
static inline StepKnobs step_knobs_from_env() {
    StepKnobs k;
    const auto clamp = [](const char* g, int lo, int hi) { return std::min(std::max(atoi(g), lo), hi); };
    if (const char* g = getenv("MTTS_GRAPHS")) k.use_graphs = atoi(g) != 0;
    if (const char* g = getenv("MTTS_FUSE_QKV_MAX")) k.fuse_qkv_max = atoi(g);
    if (const char* g = getenv("MTTS_KV_PACK")) k.kv_pack = atoi(g);
    if (const char* g = getenv("MTTS_KV_PACK_MIN")) k.pack_min_work = atoi(g);
    if (const char* g = getenv("MTTS_PREFILL_MFMA_PAGES")) k.pf_mfma_pages = atoi(g);
    if (const char* g = getenv("MTTS_ATTN_ROW")) k.attn_row = clamp(g, 0, 2);
    if (const char* g = getenv("MTTS_SMALL_ROWS")) k.small_rows = clamp(g, 0, SMALL_RP);
    if (const char* g = getenv("MTTS_GEMM_DEPTH")) k.gemm_depth = atoi(g) != 0;
    if (const char* g = getenv("MTTS_FOLD_NORM")) k.fold_norm = atoi(g) != 0;
    if (const char* g = getenv("MTTS_W_SEAL")) k.w_seal = clamp(g, 0, 2);
    if (const char* g = getenv("MTTS_W_SEAL_HEAD")) k.w_seal_head = atoi(g) != 0;
    return k;
}
// the two that the per-kernel hooks (hooks.hip) read per call
static inline int fold_norm_env() { return step_knobs_from_env().fold_norm; }
static inline int gemm_depth_env() { return step_knobs_from_env().gemm_depth; }

// ---- what is fixed once the engine exists ---------------------------------------------------------------------------
enum { GEMM_QKV = 0, GEMM_O = 1, GEMM_GU = 2, GEMM_DOWN = 3, GEMM_HEAD0 = 4, GEMM_HEADS = 5,
       GEMM_GU_SLAB = 6,            // gate/up writing a slab instead of running its SwiGLU epilogue (a pass with adapters)
       GEMM_KINDS = 7 };
struct StepCaps {
    int G = 1, nkv = 1, L = 0;      // q heads per kv head, kv heads, layers
    int n_cus = 0;                  // compute units of the device
    bool f32 = false;               // the fp32 / fp16 engine: the plan says F32 and nothing more
    bool small_fits = false;        // the small-batch kernels' LDS holds this model's rows
    bool fold_shape = false;        // fold_norm_shape of the engine's o_proj and gate/up plans
    int row_lds_limit = 0;          // dynamic LDS an attn_row_kernel block may take (0: attn_row_prepare failed, or MTTS_ATTN_ROW=0)
    bool wseal_kind[WSEAL_KINDS] = {false, false, false, false};    // the kind has a sealed twin
    int gemm_form[GEMM_KINDS] = {0, 0, 0, 0, 0, 0, 0};              // the kernel launch_gemm gives each GEMM at one row tile (describe() names it)
};

// ---- what varies ------------------------------------------------------------------------------------------------------
struct StepState {
    int heads = 1;                  // 0 none, 1 decode (rows are dialogues), 2 end of a prefill
    int B = 0, R = 0;               // dialogues of the run, rows of the pass
    int pages_bound = 0;
    bool lora = false;              // a row of the pass has an adapter
    bool forced = false, ch0_sampled = false, scores_on = false;     // the sampler's variants (decode)
    bool floors_on = false;         // a sampled channel of the run has a probability floor (mtts_set_sampler_floors)
    bool typical_on = false;        // a sampled channel of the run has a typical_p (mtts_set_sampler_typical)
    bool bans_on = false;           // a channel of the run has a hard ban (mtts_set_sampler_bans, or a -inf rule, min_length or
                                    // begin_suppress_tokens of mtts_set_sampler_bias): ban_kernel runs ahead of the sampler
    bool bias_on = false;           // a channel has a sequence rule (mtts_set_sampler_bias): bias_kernel runs behind ban_kernel
    bool bias_terms = false;        // ... a finite one: the sampler reads the bias words and tables
    int topk = 0;
    bool split = false;             // the step is issued in halves with the caller in between (mtts_step_begin / mtts_step_finish):
                                    // the sampler reads the caller's fp32 score rows
    bool wseal_on[WSEAL_KINDS] = {false, false, false, false};       // the weight policy: the kind's decode GEMMs read the twin
    const char* pack_k_on = nullptr;    // [L] the KV read policy per layer; null: the engine keeps no sealed pages
    const char* pack_v_on = nullptr;
};

// ---- the plan ---------------------------------------------------------------------------------------------------------
enum StepPath { PATH_F32 = 0, PATH_SMALL = 1, PATH_ROWS = 2 };
enum AttnForm { ATTN_FORM_ROW = 0,            // one launch: attn_row_kernel, the q/k/v epilogue inside
                ATTN_FORM_TWO_PASS_FUSED = 1, // scores, P.V (and the combine, which the small path leaves to o_proj), epilogue inside
                ATTN_FORM_TWO_PASS_EPILOGUE = 2,   // launch_qkv_post, then the same
                ATTN_FORM_PREFILL_MFMA = 3 }; // launch_qkv_post, then the tile-sharing prefill kernels
struct LayerPlan {
    AttnForm attn;
    bool k_sealed, v_sealed;        // the layer's attention reads complete K / V pages in their sealed form
    bool operator==(const LayerPlan& o) const { return attn == o.attn && k_sealed == o.k_sealed && v_sealed == o.v_sealed; }
};
struct StepPlan {
    StepPath path = PATH_ROWS;
    int heads = 1, B = 0, R = 0;
    int mb = 1, hmb = 1;            // activation row tiles that share a weight stream: the layers', the heads'
    bool tiled = false;             // prefill passes: the tiled GEMM, its split-K a function of the shape only
    bool lora = false, fold = false;
    bool sealed[WSEAL_KINDS] = {false, false, false, false};        // the GEMM reads the sealed twin
    bool head_persistent = false;   // ... the heads through the persistent kernel
    std::vector<LayerPlan> layers;  // empty on the F32 path
    bool forced = false, ch0_sampled = false, scores_on = false, floors_on = false, typical_on = false, bans_on = false, bias_on = false, bias_terms = false;
    int topk = 0;
    bool split = false;             // issued in halves (mtts_step_begin / mtts_step_finish): never the unsplit step's captured graph
    int gemm_form[GEMM_KINDS] = {0, 0, 0, 0, 0, 0, 0};              // for describe(): a function of the fields above and the caps
    bool operator==(const StepPlan& o) const {
        return path == o.path && heads == o.heads && B == o.B && R == o.R && mb == o.mb && hmb == o.hmb && tiled == o.tiled &&
               lora == o.lora && fold == o.fold && std::equal(sealed, sealed + WSEAL_KINDS, o.sealed) &&
               head_persistent == o.head_persistent && layers == o.layers && forced == o.forced && ch0_sampled == o.ch0_sampled &&
               scores_on == o.scores_on && floors_on == o.floors_on && typical_on == o.typical_on && bans_on == o.bans_on && bias_on == o.bias_on && bias_terms == o.bias_terms && topk == o.topk && split == o.split && std::equal(gemm_form, gemm_form + GEMM_KINDS, o.gemm_form);
    }
    bool operator!=(const StepPlan& o) const { return !(*this == o); }
};

// MTTS_ATTN_ROW=1: the shapes at which one block per (row, kv head) beats the two-pass kernels -- a function of the shape
// only (both paths give the same bits, so it may depend on the batch): the blocks have to fill the machine.  No bound on
// the context: at 32 rows it wins from 3 pages (most waves idle) to 8 k (profiles/attn_row_ab.json), and the LDS ends it
static inline bool attn_row_auto(int rows, int nkv, int n_cus) { return n_cus > 0 && rows * nkv >= n_cus; }

static inline StepPlan plan_step(const StepKnobs& k, const StepCaps& c, const StepState& s) {
    StepPlan p;
    const bool decode = s.heads == 1;
    p.heads = s.heads; p.B = s.B; p.R = s.R;
    if (decode) { p.forced = s.forced; p.ch0_sampled = s.ch0_sampled; p.scores_on = s.scores_on; p.floors_on = s.floors_on; p.typical_on = s.typical_on; p.bans_on = s.bans_on; p.bias_on = s.bias_on; p.bias_terms = s.bias_on && s.bias_terms; p.topk = s.topk; p.split = s.split; }
    if (c.f32) { p.path = PATH_F32; return p; }
    // decode steps of a few dialogues: six launches per layer whose prologues redo the small kernels' work.  The small path
    // has no slabs for an adapter's delta; its arithmetic is the general path's, so nothing depends on which one runs
    const bool small = decode && !s.lora && s.B <= k.small_rows && c.small_fits;
    p.path = small ? PATH_SMALL : PATH_ROWS;
    const int work = s.B * s.pages_bound;
    // the q/k/v epilogue inside the attention kernels (decode rows, one dialogue each) where it pays: every attention block
    // repeats the q epilogue, which costs more than the saved launch once rows x pages is large.  Prefill passes need
    // every K/V row of the pass in the cache before any of its attention runs, so they keep the launch
    const bool fused = decode && work <= k.fuse_qkv_max;
    // decode rows read complete pages in their sealed form where the layer's read policy says so; prefill tiles share
    // their K/V pages and may complete a page themselves: bf16 pages
    const bool pack = decode && work >= k.pack_min_work;
    const bool row_shape = !small && decode && k.attn_row != 0 && (k.attn_row == 2 || attn_row_auto(s.B, c.nkv, c.n_cus));
    p.layers.resize(c.L);
    for (int n = 0; n < c.L; ++n) {
        LayerPlan& l = p.layers[n];
        l.k_sealed = pack && s.pack_k_on && s.pack_k_on[n];
        l.v_sealed = pack && s.pack_v_on && s.pack_v_on[n];
        // the whole-row kernel takes K and V pages in the same form and a page bound whose LDS fits one block
        const bool row = row_shape && l.k_sealed == l.v_sealed && attn_row_lds_bytes(c.G, l.k_sealed, s.pages_bound) <= c.row_lds_limit;
        l.attn = row ? ATTN_FORM_ROW : fused ? ATTN_FORM_TWO_PASS_FUSED :
                 (!decode && s.pages_bound >= k.pf_mfma_pages) ? ATTN_FORM_PREFILL_MFMA : ATTN_FORM_TWO_PASS_EPILOGUE;
    }
    if (small) return p;
    p.mb = (s.R + 31) / 32;
    p.hmb = s.heads == 2 ? (s.B + 31) / 32 : p.mb;
    p.tiled = !decode;
    p.lora = s.lora;
    // one row tile without adapters: the GEMM reads its sealed twin where the weight policy says so (same bits).  The
    // sealed kernels are depth-specialised ones: MTTS_GEMM_DEPTH=0 switches them off as well
    const auto sealed = [&](int kind, int tiles) { return !s.lora && tiles == 1 && k.gemm_depth && c.wseal_kind[kind] && s.wseal_on[kind]; };
    p.sealed[WSEAL_GU] = !p.tiled && sealed(WSEAL_GU, p.mb);
    p.sealed[WSEAL_DOWN] = !p.tiled && sealed(WSEAL_DOWN, p.mb);
    p.sealed[WSEAL_HEAD0] = s.heads != 0 && sealed(WSEAL_HEAD0, p.hmb);
    p.sealed[WSEAL_HEADS] = s.heads != 0 && sealed(WSEAL_HEADS, p.hmb);
    p.head_persistent = (p.sealed[WSEAL_HEAD0] || p.sealed[WSEAL_HEADS]) && k.w_seal_head;
    // decode rows in one row tile, no adapter row: o_proj -> post-attention norm -> gate/up as gemm_fold.hip's two launches
    // where both GEMMs have the shape those kernels are built for and gate/up does not read its twin
    p.fold = k.fold_norm && decode && p.mb == 1 && !s.lora && k.gemm_depth && !s.wseal_on[WSEAL_GU] && c.fold_shape;
    for (int g = 0; g < GEMM_KINDS; ++g) {
        const int tiles = (g == GEMM_HEAD0 || g == GEMM_HEADS) ? p.hmb : p.mb;
        p.gemm_form[g] = tiles == 1 ? c.gemm_form[g] : GEMM_SKINNY;
    }
    return p;
}

// One line of text per distinct launch group, in issue order (the tests and mtts_debug_step_plan read it).  The first line
// is the pass, the second (decode) the sampler; a layer line stands for that launch in every layer.
static inline std::string describe(const StepPlan& p) {
    static const char* const paths[] = {"f32", "small", "rows"};
    static const char* const forms[] = {"skinny", "depth", "gateup48"};
    static const char* const attn[] = {"row", "two_pass fused", "two_pass epilogue", "prefill mfma"};
    char buf[160];
    snprintf(buf, sizeof(buf), "pass: %s B=%d R=%d heads=%d layers=%d\n", paths[p.path], p.B, p.R, p.heads, (int)p.layers.size());
    std::string out = buf;
    if (p.heads == 1) {
        snprintf(buf, sizeof(buf), "sample:%s%s%s%s%s%s%s topk=%d%s\n", p.ch0_sampled ? " ch0_sampled" : " ch0_greedy", p.scores_on ? " scores" : "",
                 p.floors_on ? " floors" : "", p.typical_on ? " typical" : "", p.bans_on ? " bans" : "", p.bias_terms ? " bias" : p.bias_on ? " rules" : "", p.forced ? " forced" : "", p.topk, p.split ? " split" : "");
        out += buf;
    }
    if (p.path == PATH_F32) return out;
    const auto gemm = [&](const char* name, int g, int tiles, bool sealed, const char* more) {
        std::string s = std::string(name) + ": ";
        if (p.path == PATH_SMALL) s += "small";
        else if (p.tiled && g != GEMM_HEAD0 && g != GEMM_HEADS) s += "tile";
        else {
            if (sealed) s += p.gemm_form[g] == GEMM_SKINNY ? "sealed" : std::string(forms[p.gemm_form[g]]) + " sealed";     // (the twin of that kernel)
            else s += forms[p.gemm_form[g]];
            if (tiles > 1) s += " x" + std::to_string(tiles);
        }
        return s + more + "\n";
    };
    const char* lora = p.lora ? " +lora" : "";
    out += gemm("qkv", GEMM_QKV, p.mb, false, lora);
    for (size_t a = 0; a < p.layers.size();) {
        size_t b = a;
        while (b + 1 < p.layers.size() && p.layers[b + 1] == p.layers[a]) ++b;
        const LayerPlan& l = p.layers[a];
        snprintf(buf, sizeof(buf), "attn[%d..%d]: %s%s\n", (int)a, (int)b, attn[l.attn],
                 l.k_sealed && l.v_sealed ? " sealed" : l.k_sealed ? " k_sealed" : l.v_sealed ? " v_sealed" : "");
        out += buf;
        a = b + 1;
    }
    if (p.fold) out += "o_proj+gate_up: fold\n";
    else {
        out += gemm("o_proj", GEMM_O, p.mb, false, lora);
        out += gemm("gate_up", p.lora ? GEMM_GU_SLAB : GEMM_GU, p.mb, p.sealed[WSEAL_GU], p.lora ? " slab +lora" : "");
    }
    out += gemm("down", GEMM_DOWN, p.mb, p.sealed[WSEAL_DOWN], lora);
    if (p.heads) {
        out += gemm("head0", GEMM_HEAD0, p.hmb, p.sealed[WSEAL_HEAD0], p.sealed[WSEAL_HEAD0] && p.head_persistent ? " persistent" : "");
        out += gemm("heads1_7", GEMM_HEADS, p.hmb, p.sealed[WSEAL_HEADS], p.sealed[WSEAL_HEADS] && p.head_persistent ? " persistent" : "");
    }
    return out;
}
