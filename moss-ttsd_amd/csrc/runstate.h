// What a run is started with, and what a captured decode step holds on to.  Three small types, each of which keeps a rule
// that engine.hip used to keep by hand:
//   PendingRun / RunOptions   the settings of the mtts_set_* calls.  The one-shot ones leave the engine in one place
//                             (take), before anything can fail, so "consumed by the next begin, failures included" holds
//                             for every one of them; the sticky ones are copied.
//   StepBufs                  every device address a decode step reads that can change after mtts_engine_create, with
//                             whatever bounds the step's indexing into it.
//   StepGraphs                the captured steps, found by (plan, KV page bound, StepBufs): a step captured with buffers
//                             that have since been reallocated is never found again, and is destroyed by the next insert.
// No HIP in here: engine.h includes it, and so does tests/host/run_state_main.cpp, which runs it on the CPU.
#pragma once
#include <cmath>
#include <cstring>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../include/mtts.h"       // MttsSamplerFloors, MttsSamplerBans, MttsSamplerBias (plain C, no HIP)
#include "stepplan.h"

// defined by whoever includes this (engine.hip; the CPU test), as for kvpool.h
__attribute__((visibility("hidden"), format(printf, 2, 3))) int fail(int code, const char* fmt, ...);
static const int RUN_EINVAL = -1;       // MTTS_EINVAL of include/mtts.h (engine.h checks that it is)

// The hard bans of a run (mtts_set_sampler_bans), owned: the caller's suppress lists are copied when they are set.
struct ChannelBans {
    int ngram = 0, min_new = 0;         // no_repeat_ngram_size, min_new_tokens; 0: absent
    std::vector<int32_t> suppress;
    bool any() const { return ngram > 0 || min_new > 0 || !suppress.empty(); }
};
struct RunBans {
    std::vector<ChannelBans> ch;        // per channel; empty: none
    bool any() const { for (const ChannelBans& c : ch) if (c.any()) return true; return false; }
    bool ngram() const { for (const ChannelBans& c : ch) if (c.ngram > 0) return true; return false; }
};

// The sequence rules and step-conditioned bans of a run (mtts_set_sampler_bias), owned like the bans.
struct ChannelBias {
    std::vector<int32_t> len, ids;      // rule r: the next len[r] entries of ids
    std::vector<float> beta;            // -inf: a ban (bad_words_ids)
    int min_length = 0;                 // 0: absent
    std::vector<int32_t> begin;         // begin_suppress_tokens
    bool any() const { return !len.empty() || min_length > 0 || !begin.empty(); }
};
struct RunBias {
    std::vector<ChannelBias> ch;        // per channel; empty: none
    bool any() const { for (const ChannelBias& c : ch) if (c.any()) return true; return false; }
    bool rules() const { for (const ChannelBias& c : ch) if (!c.len.empty()) return true; return false; }          // the rule kernel runs
    bool finite() const { for (const ChannelBias& c : ch) for (float v : c.beta) if (v > -INFINITY) return true; return false; }   // the sampler adds terms
    bool bans() const {                 // the ban path is on: a -inf rule, min_length, begin_suppress_tokens
        for (const ChannelBias& c : ch) {
            if (c.min_length > 0 || !c.begin.empty()) return true;
            for (float v : c.beta) if (!(v > -INFINITY)) return true;
        }
        return false;
    }
    bool begin() const { for (const ChannelBias& c : ch) if (!c.begin.empty()) return true; return false; }
    bool history() const { for (const ChannelBias& c : ch) for (int32_t l : c.len) if (l > 1) return true; return false; }    // a rule reads the history
};

// ---- the options of one static run ----------------------------------------------------------------------------------
struct RunOptions {
    int B = 0;                          // prompts of the call
    int takes = 1;                      // rows per prompt: row b*takes+j is take j of prompt b
    std::vector<int32_t> row_ids;       // Philox row id per row; empty: 0..rows-1
    std::vector<int32_t> row_adapters;  // adapter per PROMPT (its takes share its KV pages and so its adapter); empty: none
    std::vector<MttsSamplerFloors> floors;      // per channel (mtts_set_sampler_floors); empty: none
    std::vector<float> typical;         // typical_p per channel (mtts_set_sampler_typical), 0: absent; empty: none
    RunBans bans;                       // per channel (mtts_set_sampler_bans); empty: none
    RunBias bias;                       // per channel (mtts_set_sampler_bias); empty: none
    int output_scores = 0, top_logprobs = 0;
    int rows() const { return B * takes; }
    int row_id(int r) const { return row_ids.empty() ? r : row_ids[r]; }
    int row_adapter(int r) const { return row_adapters.empty() ? -1 : row_adapters[r / takes]; }
    // the sizes, before anything is indexed by them; forced: the call is a forced replay (mtts_generate with host_forced)
    int check(int max_batch, bool forced) const {
        if (forced && takes > 1) return fail(RUN_EINVAL, "forced replay (reference fixtures) has no takes: %d takes per prompt", takes);
        if (!row_adapters.empty() && (int)row_adapters.size() != B)
            return fail(RUN_EINVAL, "mtts_set_row_adapters gave %d ids, the batch has %d prompts", (int)row_adapters.size(), B);
        if (B < 1 || B > max_batch || rows() > max_batch) return fail(RUN_EINVAL, "batch %d x %d takes exceeds max_batch %d", B, takes, max_batch);
        if (!row_ids.empty() && (int)row_ids.size() != rows())
            return fail(RUN_EINVAL, "mtts_set_row_ids gave %d ids, the batch has %d rows", (int)row_ids.size(), rows());
        return 0;
    }
};

// What the mtts_set_* calls leave for the next run.  They validate and store; nothing else in the engine reads these.
class PendingRun {
    int takes = 1;
    std::vector<int32_t> row_ids, row_adapters;
    std::vector<int32_t> slot_adapter = std::vector<int32_t>(MTTS_RCAP, -1);    // scheduler mode: of the slot's next submit
    std::vector<MttsSamplerFloors> floors;
    std::vector<float> typical;
    RunBans bans;
    RunBias bias;
public:
    int output_scores = 0, top_logprobs = 0;        // sticky: every run reads them, none resets them
    void set_takes(int n) { takes = n; }
    void set_row_ids(const int32_t* ids, int n) { row_ids.assign(ids, ids + n); }
    void set_row_adapters(const int32_t* ids, int n) { row_adapters.assign(ids, ids + n); }
    void set_slot_adapter(int slot, int id) { slot_adapter[slot] = id; }
    // checked here, where every other size and value of a run's options is: the channel is named
    int set_floors(const MttsSamplerFloors* f) {
        floors.clear();
        for (int c = 0; f && c < MTTS_CHANNELS; ++c) {
            if (!(f[c].min_p >= 0.f && f[c].min_p <= 1.f)) return fail(RUN_EINVAL, "channel %d: min_p %g is outside [0, 1]", c, (double)f[c].min_p);
            if (!(f[c].epsilon_cutoff >= 0.f && f[c].epsilon_cutoff < 1.f))
                return fail(RUN_EINVAL, "channel %d: epsilon_cutoff %g is outside [0, 1)", c, (double)f[c].epsilon_cutoff);
            if (!(f[c].eta_cutoff >= 0.f && f[c].eta_cutoff < 1.f)) return fail(RUN_EINVAL, "channel %d: eta_cutoff %g is outside [0, 1)", c, (double)f[c].eta_cutoff);
        }
        if (f) floors.assign(f, f + MTTS_CHANNELS);
        return 0;
    }
    // typical_p per channel: 0 or 1 mean "absent" (HF adds the warper for typical_p < 1) and are stored as 0; anything else
    // lies strictly inside (0, 1), as HF's constructor demands.  A refused call leaves none behind
    int set_typical(const float* t) {
        typical.clear();
        if (!t) return 0;
        std::vector<float> v(MTTS_CHANNELS, 0.f);
        for (int c = 0; c < MTTS_CHANNELS; ++c) {
            if (t[c] == 0.f || t[c] == 1.f) continue;
            if (!(t[c] > 0.f && t[c] < 1.f)) return fail(RUN_EINVAL, "channel %d: typical_p %g is outside (0, 1)", c, (double)t[c]);
            v[c] = t[c];
        }
        typical.swap(v);
        return 0;
    }
    // the same for the bans; a refused call leaves none behind
    int set_bans(const MttsSamplerBans* b) {
        bans.ch.clear();
        if (!b) return 0;
        std::vector<ChannelBans> ch(MTTS_CHANNELS);
        for (int c = 0; c < MTTS_CHANNELS; ++c) {
            if (b[c].no_repeat_ngram_size < 0 || b[c].no_repeat_ngram_size > MTTS_NGRAM_MAX)
                return fail(RUN_EINVAL, "channel %d: no_repeat_ngram_size %d is outside [0, %d]", c, b[c].no_repeat_ngram_size, MTTS_NGRAM_MAX);
            if (b[c].min_new_tokens < 0) return fail(RUN_EINVAL, "channel %d: min_new_tokens %d is negative", c, b[c].min_new_tokens);
            if (b[c].n_suppress < 0 || (b[c].n_suppress > 0 && !b[c].suppress))
                return fail(RUN_EINVAL, "channel %d: suppress_tokens: %d ids and %s list", c, b[c].n_suppress, b[c].suppress ? "a" : "no");
            for (int i = 0; i < b[c].n_suppress; ++i)
                if (b[c].suppress[i] < 0) return fail(RUN_EINVAL, "channel %d: suppress_tokens holds the negative id %d", c, b[c].suppress[i]);
            ch[c].ngram = b[c].no_repeat_ngram_size;
            ch[c].min_new = b[c].min_new_tokens;
            if (b[c].n_suppress > 0) ch[c].suppress.assign(b[c].suppress, b[c].suppress + b[c].n_suppress);
        }
        bans.ch.swap(ch);
        return 0;
    }
    // the same for the sequence rules, min_length and begin_suppress_tokens; a refused call leaves none behind
    int set_bias(const MttsSamplerBias* b) {
        bias.ch.clear();
        if (!b) return 0;
        std::vector<ChannelBias> ch(MTTS_CHANNELS);
        for (int c = 0; c < MTTS_CHANNELS; ++c) {
            const MttsSamplerBias& s = b[c];
            if (s.n_rules < 0 || s.n_rules > MTTS_BIAS_RULES_MAX)
                return fail(RUN_EINVAL, "channel %d: %d sequence_bias / bad_words_ids rules, at most %d", c, s.n_rules, MTTS_BIAS_RULES_MAX);
            if (s.n_rules > 0 && (!s.rule_len || !s.rule_ids || !s.rule_bias)) return fail(RUN_EINVAL, "channel %d: %d rules and a list missing", c, s.n_rules);
            if (s.min_length < 0) return fail(RUN_EINVAL, "channel %d: min_length %d is negative", c, s.min_length);
            if (s.n_begin_suppress < 0 || (s.n_begin_suppress > 0 && !s.begin_suppress))
                return fail(RUN_EINVAL, "channel %d: begin_suppress_tokens: %d ids and %s list", c, s.n_begin_suppress, s.begin_suppress ? "a" : "no");
            size_t total = 0;
            for (int r = 0; r < s.n_rules; ++r) {
                if (s.rule_len[r] < 1 || s.rule_len[r] > MTTS_BIAS_RULE_LEN_MAX)
                    return fail(RUN_EINVAL, "channel %d: rule %d has %d tokens, a rule has 1 to %d", c, r, s.rule_len[r], MTTS_BIAS_RULE_LEN_MAX);
                if (!(s.rule_bias[r] < INFINITY)) return fail(RUN_EINVAL, "channel %d: rule %d has the bias %g (NaN and +inf are refused)", c, r, (double)s.rule_bias[r]);
                for (int k = 0; k < s.rule_len[r]; ++k)
                    if (s.rule_ids[total + k] < 0) return fail(RUN_EINVAL, "channel %d: rule %d holds the negative id %d", c, r, s.rule_ids[total + k]);
                total += (size_t)s.rule_len[r];
            }
            for (int i = 0; i < s.n_begin_suppress; ++i)
                if (s.begin_suppress[i] < 0) return fail(RUN_EINVAL, "channel %d: begin_suppress_tokens holds the negative id %d", c, s.begin_suppress[i]);
            if (s.n_rules > 0) {
                ch[c].len.assign(s.rule_len, s.rule_len + s.n_rules);
                ch[c].beta.assign(s.rule_bias, s.rule_bias + s.n_rules);
                ch[c].ids.assign(s.rule_ids, s.rule_ids + total);
            }
            ch[c].min_length = s.min_length;
            if (s.n_begin_suppress > 0) ch[c].begin.assign(s.begin_suppress, s.begin_suppress + s.n_begin_suppress);
        }
        bias.ch.swap(ch);
        return 0;
    }
    bool has_row_adapters() const { return !row_adapters.empty(); }
    // mtts_begin / mtts_generate with B prompts: the one-shots move out and are back at their defaults, whatever the call
    // does next (RunOptions::check included)
    RunOptions take(int B) {
        RunOptions o;
        o.B = B; o.takes = takes; o.output_scores = output_scores; o.top_logprobs = top_logprobs;
        o.row_ids.swap(row_ids);
        o.row_adapters.swap(row_adapters);
        o.floors = take_floors();
        o.typical = take_typical();
        o.bans = take_bans();
        o.bias = take_bias();
        takes = 1;
        return o;
    }
    // mtts_sched_open: a scheduler run takes no other one-shot
    std::vector<MttsSamplerFloors> take_floors() { return std::exchange(floors, {}); }
    std::vector<float> take_typical() { return std::exchange(typical, {}); }
    RunBans take_bans() { return std::exchange(bans, RunBans()); }
    RunBias take_bias() { return std::exchange(bias, RunBias()); }
    // mtts_slot_submit* into `slot`: the same for that slot's adapter
    int take_slot_adapter(int slot) { return std::exchange(slot_adapter[slot], -1); }
};

// ---- the addresses a captured step holds ----------------------------------------------------------------------------
// A step graph bakes in its launches' arguments.  Everything allocated by mtts_engine_create lives as long as the engine;
// what is allocated or reallocated later and read by a decode step (step_body, forward_rows, forward_small, attend_layer,
// forward_rows_f32 of engine.hip) is here, beside the sizes that bound the step's indexing into it -- an allocator may hand
// the old address out again for another size.  Not here, though a step passes it: the run's seed.  launch_sample takes it
// by value for the single-matrix test entry (sampler.hip: single_vocab > 0); a step's rows draw with SeqState.seed, which
// lives in device memory, so a replayed step does not depend on the value it was captured with.
struct LoraEnt;
struct StepBufs {
    int32_t *d_gen = nullptr, *d_declog = nullptr, *d_forced = nullptr;    // [slot][gen_cap][8]: tokens, decision log, forced rows
    float* d_lp = nullptr;                  // output_scores [slot][gen_cap][8]; exists once a run asked for it
    float *sscr_slice_sum = nullptr, *sscr_lp = nullptr;        // ... and the sampler's scratch for it (SampleScratch), sized by max_batch
    float* d_gt_logp = nullptr;             // top_logprobs [slot][gen_cap][8], and [slot][gen_cap][8][gt_stride]:
    int32_t* d_gt_ids = nullptr;
    float* d_gt_tlp = nullptr;
    unsigned long long* gt_cand = nullptr;  // ... and its scratch (GenTopkScratch), which holds gt_scr_cap candidates per slice
    float* gt_smax = nullptr;
    double* gt_ssum = nullptr;
    uint16_t *rope_cos = nullptr, *rope_sin = nullptr;          // [rope_rows][64] (mtts_bind_rope): the bf16 engine's,
    float *rope_cos_f = nullptr, *rope_sin_f = nullptr;         // the fp32 / fp16 engine's
    float* partial = nullptr;               // split-K slabs: widened by the first mtts_adapter_load, with which the next two appear
    LoraEnt* d_bank = nullptr;
    int32_t* d_seq_adapter = nullptr;
    // hard bans (mtts_set_sampler_bans); all three exist once a run asked for a ban, d_hist once one asked for an n-gram ban
    uint32_t* d_ban = nullptr;              // [slot][8][ban_words]: the step's banned tokens, rewritten by ban_kernel every step
    uint32_t* d_ban_static = nullptr;       // [8][ban_words]: the run's suppress_tokens per channel
    int32_t* d_hist = nullptr;              // [slot][hist_cap][8]: the prompt's slots, padding included (the generated ones are d_gen)
    // sequence rules (mtts_set_sampler_bias); each exists once a run asked for what it serves
    uint32_t* d_ban_begin = nullptr;        // [8][ban_words]: begin_suppress_tokens per channel, ORed in by ban_kernel at its one step
    BiasRules* d_bias_rules = nullptr;      // [8]: the run's rules per channel, flattened (any rule)
    uint32_t* d_bias_w = nullptr;           // [slot][8][ban_words]: the step's tokens with a term, rewritten by bias_kernel every step (a finite rule)
    uint32_t* d_bias_static = nullptr;      // [8][ban_words]: the single-token finite rules per channel
    MttsBiasTable* d_bias_tab = nullptr;    // [slot][8]: the step's (id, term) tables
    int gen_cap = 0;                        // steps a slot's rows hold
    int gt_stride = 0, gt_scr_cap = 0;      // innermost stride of d_gt_ids / d_gt_tlp; of gt_cand
    int rope_rows = 0;
    int hist_cap = 0, ban_words = 0;        // prompt slots a row of d_hist holds; words per (slot, channel) of d_ban
    // every byte takes part (no padding: the assertion below), so a new member cannot be left out of the comparison
    bool operator==(const StepBufs& o) const { return memcmp(this, &o, sizeof(StepBufs)) == 0; }
    bool operator!=(const StepBufs& o) const { return !(*this == o); }
};
static_assert(std::has_unique_object_representations<StepBufs>::value, "StepBufs is compared (and swept by its test) bytewise: no padding");

// ---- the captured steps ---------------------------------------------------------------------------------------------
// Exec: the handle of a captured step (hipGraphExec_t; an int on the CPU); Destroy: what frees one.
template <typename Exec, typename Destroy>
class StepGraphs {
    struct Entry { StepPlan plan; int pages; StepBufs bufs; Exec exec; };
    std::vector<Entry> entries;
    Destroy destroy;
public:
    enum { CAP = 256 };
    explicit StepGraphs(Destroy d = Destroy()) : destroy(d) {}
    StepGraphs(const StepGraphs&) = delete;
    StepGraphs& operator=(const StepGraphs&) = delete;
    ~StepGraphs() { clear(); }
    size_t size() const { return entries.size(); }
    const Exec* find(const StepPlan& plan, int pages, const StepBufs& bufs) const {
        for (const Entry& g : entries)
            if (g.pages == pages && g.bufs == bufs && g.plan == plan) return &g.exec;
        return nullptr;
    }
    // Steps captured with other buffers hold addresses that are dead by now (the engine has one StepBufs at a time): they
    // go first.  Then the cap: a run whose plans keep changing starts over instead of growing without bound.
    void insert(StepPlan plan, int pages, const StepBufs& bufs, Exec exec) {
        size_t keep = 0;
        for (size_t i = 0; i < entries.size(); ++i) {
            if (entries[i].bufs != bufs) destroy(entries[i].exec);
            else { if (keep != i) entries[keep] = std::move(entries[i]); ++keep; }
        }
        entries.erase(entries.begin() + keep, entries.end());
        if (entries.size() >= CAP) clear();
        entries.push_back(Entry{std::move(plan), pages, bufs, exec});
    }
    void clear() {
        for (Entry& g : entries) destroy(g.exec);
        entries.clear();
    }
};
