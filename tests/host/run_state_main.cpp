// Stand-alone host program for tests/test_run_state_cpu.py: csrc/runstate.h on the CPU, nothing of HIP.  One case per run:
// `run_state_main <case>` ends with "ok <case>", exit status 0; a check that does not hold prints itself and exits 1.
// Built with -fsanitize=address,undefined: a leaked or twice-destroyed graph handle is the sanitizer's finding.
//   options    PendingRun::take after each set_* alone and combined, the sticky switches, a take whose check fails
//   sizes      RunOptions::check: every size mismatch and its message
//   slots      the one-shot adapter of a slot
//   key        StepGraphs<int*>: a hit needs plan, pages and bufs all equal; every byte of StepBufs takes part
//   stale      insert with new bufs destroys exactly the stale entries, once each; clear destroys the rest
//   cap        the 257th insert empties first
#include <climits>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <string>

#include "../../moss-ttsd_amd/csrc/runstate.h"

static char g_err[512] = "";
int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

#define CHECK(c)                                                          \
    do {                                                                  \
        if (!(c)) {                                                       \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);         \
            exit(1);                                                      \
        }                                                                 \
    } while (0)

// the one-shot options of `o` are the defaults
static bool one_shots_default(const RunOptions& o) { return o.takes == 1 && o.row_ids.empty() && o.row_adapters.empty(); }

static void options() {
    const int32_t ids[6] = {9, 8, 7, 6, 5, 4}, ad[3] = {2, -1, 0};
    PendingRun p;
    CHECK(one_shots_default(p.take(3)) && !p.has_row_adapters());
    // each alone: the take has it, the next take does not
    p.set_takes(2);
    RunOptions o = p.take(3);
    CHECK(o.B == 3 && o.takes == 2 && o.rows() == 6 && o.row_ids.empty() && o.row_adapters.empty() && o.check(8, false) == 0);
    CHECK(o.row_id(4) == 4 && o.row_adapter(4) == -1);
    CHECK(one_shots_default(p.take(3)));
    p.set_row_ids(ids, 3);
    o = p.take(3);
    CHECK(o.takes == 1 && o.row_ids == std::vector<int32_t>({9, 8, 7}) && o.row_adapters.empty() && o.check(8, false) == 0 && o.row_id(2) == 7);
    CHECK(one_shots_default(p.take(3)));
    p.set_row_adapters(ad, 3);
    CHECK(p.has_row_adapters());
    o = p.take(3);
    CHECK(!p.has_row_adapters() && o.takes == 1 && o.row_ids.empty() && o.row_adapters == std::vector<int32_t>({2, -1, 0}) && o.check(8, false) == 0);
    CHECK(one_shots_default(p.take(3)));
    p.set_row_adapters(ad, 0);                         // an empty list is no list
    CHECK(!p.has_row_adapters());
    // combined, with the sticky switches: those stay, through any number of takes
    p.output_scores = 1; p.top_logprobs = 5;
    p.set_takes(2); p.set_row_ids(ids, 6); p.set_row_adapters(ad, 3);
    o = p.take(3);
    CHECK(o.takes == 2 && o.row_ids.size() == 6 && o.row_adapters.size() == 3 && o.output_scores == 1 && o.top_logprobs == 5 && o.check(6, false) == 0);
    CHECK(o.row_id(5) == 4 && o.row_adapter(0) == 2 && o.row_adapter(1) == 2 && o.row_adapter(2) == -1 && o.row_adapter(5) == 0);   // a prompt's takes share its adapter
    o = p.take(3);
    CHECK(one_shots_default(o) && o.output_scores == 1 && o.top_logprobs == 5 && p.output_scores == 1 && p.top_logprobs == 5);
    // a take whose check fails has consumed them all the same
    p.set_takes(4); p.set_row_ids(ids, 5); p.set_row_adapters(ad, 2);
    o = p.take(3);
    CHECK(o.check(128, false) != 0);
    o = p.take(3);
    CHECK(one_shots_default(o) && !p.has_row_adapters() && o.check(128, false) == 0 && o.output_scores == 1 && o.top_logprobs == 5);
}

static void sizes() {
    const int32_t v[8] = {0, 1, 2, 3, 4, 5, 6, 7};
    const auto msg = [&](int takes, int n_ids, int n_ad, int B, int max_batch, bool forced) {
        PendingRun p;
        p.set_takes(takes); p.set_row_ids(v, n_ids); p.set_row_adapters(v, n_ad);
        g_err[0] = 0;
        const int rc = p.take(B).check(max_batch, forced);
        CHECK((rc == 0) == (g_err[0] == 0) && (rc == 0 || rc == RUN_EINVAL));
        return std::string(g_err);
    };
    CHECK(msg(2, 8, 4, 4, 8, false).empty());
    CHECK(msg(1, 0, 0, 8, 8, true).empty());
    CHECK(msg(2, 0, 0, 2, 8, true) == "forced replay (reference fixtures) has no takes: 2 takes per prompt");
    CHECK(msg(1, 0, 3, 4, 8, false) == "mtts_set_row_adapters gave 3 ids, the batch has 4 prompts");
    CHECK(msg(2, 0, 8, 4, 8, false) == "mtts_set_row_adapters gave 8 ids, the batch has 4 prompts");       // per prompt, not per row
    CHECK(msg(1, 0, 0, 0, 8, false) == "batch 0 x 1 takes exceeds max_batch 8");
    CHECK(msg(1, 0, 0, 9, 8, false) == "batch 9 x 1 takes exceeds max_batch 8");
    CHECK(msg(3, 0, 0, 3, 8, false) == "batch 3 x 3 takes exceeds max_batch 8");
    CHECK(msg(128, 0, 0, INT_MAX, 128, false) == "batch 2147483647 x 128 takes exceeds max_batch 128");   // (no product is formed)
    CHECK(msg(1, 0, 0, -5, 8, false) == "batch -5 x 1 takes exceeds max_batch 8");
    CHECK(msg(2, 4, 0, 4, 8, false) == "mtts_set_row_ids gave 4 ids, the batch has 8 rows");
    CHECK(msg(1, 5, 0, 4, 8, false) == "mtts_set_row_ids gave 5 ids, the batch has 4 rows");
    // the order the engine has always reported in: replay, adapters, batch, ids
    CHECK(msg(2, 1, 1, 9, 8, true).rfind("forced replay", 0) == 0);
    CHECK(msg(2, 1, 1, 9, 8, false).rfind("mtts_set_row_adapters", 0) == 0);
    CHECK(msg(2, 1, 0, 9, 8, false).rfind("batch 9", 0) == 0);
}

static void slots() {
    PendingRun p;
    for (int s = 0; s < MTTS_RCAP; ++s) CHECK(p.take_slot_adapter(s) == -1);
    p.set_slot_adapter(0, 3); p.set_slot_adapter(5, 0); p.set_slot_adapter(MTTS_RCAP - 1, 15);
    CHECK(p.take_slot_adapter(5) == 0 && p.take_slot_adapter(5) == -1);          // once
    CHECK(p.take_slot_adapter(4) == -1 && p.take_slot_adapter(6) == -1);
    p.take(2);                                                                   // a static run's take leaves the slots alone
    CHECK(p.take_slot_adapter(0) == 3 && p.take_slot_adapter(MTTS_RCAP - 1) == 15);
    for (int s = 0; s < MTTS_RCAP; ++s) CHECK(p.take_slot_adapter(s) == -1);
    p.set_slot_adapter(7, 2); p.set_slot_adapter(7, -1);
    CHECK(p.take_slot_adapter(7) == -1);
}

// ---- the graph cache: handles are heap ints, so a handle that is never destroyed leaks and one destroyed twice is a
// double free -- both the sanitizer's to report; `destroyed` keeps the order for the cases to look at
static std::vector<int> destroyed;
struct Destroy {
    void operator()(int* h) const { destroyed.push_back(*h); delete h; }
};
typedef StepGraphs<int*, Destroy> Graphs;

static StepPlan plan_of(int B, int topk) {
    StepKnobs k; StepCaps c; StepState s;
    c.L = 2; c.n_cus = 256; c.nkv = 8;
    s.B = B; s.R = 32; s.pages_bound = 8; s.topk = topk;
    return plan_step(k, c, s);
}
// a StepBufs whose every byte is set and differs from its neighbours'
static StepBufs some_bufs(unsigned salt) {
    StepBufs b;
    unsigned char raw[sizeof(StepBufs)];
    for (size_t i = 0; i < sizeof(raw); ++i) raw[i] = (unsigned char)(i * 7 + salt);
    memcpy(&b, raw, sizeof(raw));
    return b;
}

static void key() {
    Graphs g;
    const StepBufs b = some_bufs(1);
    const StepPlan p = plan_of(2, 0);
    CHECK(!g.find(p, 8, b));
    g.insert(p, 8, b, new int(1));
    CHECK(g.find(p, 8, b) && **g.find(p, 8, b) == 1 && g.size() == 1);
    CHECK(g.find(plan_of(2, 0), 8, some_bufs(1)));                // by value, not by identity
    CHECK(!g.find(p, 16, b) && !g.find(plan_of(3, 0), 8, b) && !g.find(plan_of(2, 4), 8, b));
    // one differing pointer or int misses: every byte of StepBufs, which has no padding, so every member is swept
    static_assert(std::has_unique_object_representations<StepBufs>::value, "the sweep below covers members only without padding");
    for (size_t i = 0; i < sizeof(StepBufs); ++i) {
        StepBufs c = b;
        unsigned char byte;
        memcpy(&byte, (const char*)&c + i, 1);
        byte ^= 0x10;
        memcpy((char*)&c + i, &byte, 1);
        CHECK(c != b && !(c == b) && !g.find(p, 8, c));
    }
    // ... and by name, the members a reallocation changes
    const auto miss = [&](void (*edit)(StepBufs&)) { StepBufs c = b; edit(c); return !g.find(p, 8, c); };
    CHECK(miss([](StepBufs& c) { c.d_gen = nullptr; }) && miss([](StepBufs& c) { c.d_declog = nullptr; }) && miss([](StepBufs& c) { c.d_forced = nullptr; }));
    CHECK(miss([](StepBufs& c) { c.d_lp = nullptr; }) && miss([](StepBufs& c) { c.sscr_lp = nullptr; }) && miss([](StepBufs& c) { c.sscr_slice_sum = nullptr; }));
    CHECK(miss([](StepBufs& c) { c.d_gt_logp = nullptr; }) && miss([](StepBufs& c) { c.d_gt_ids = nullptr; }) && miss([](StepBufs& c) { c.d_gt_tlp = nullptr; }));
    CHECK(miss([](StepBufs& c) { c.gt_cand = nullptr; }) && miss([](StepBufs& c) { c.gt_smax = nullptr; }) && miss([](StepBufs& c) { c.gt_ssum = nullptr; }));
    CHECK(miss([](StepBufs& c) { c.rope_cos = nullptr; }) && miss([](StepBufs& c) { c.rope_sin = nullptr; }) && miss([](StepBufs& c) { c.rope_cos_f = nullptr; }) &&
          miss([](StepBufs& c) { c.rope_sin_f = nullptr; }));
    CHECK(miss([](StepBufs& c) { c.partial = nullptr; }) && miss([](StepBufs& c) { c.d_bank = nullptr; }) && miss([](StepBufs& c) { c.d_seq_adapter = nullptr; }));
    CHECK(miss([](StepBufs& c) { c.gen_cap ^= 1; }) && miss([](StepBufs& c) { c.gt_stride ^= 1; }) && miss([](StepBufs& c) { c.gt_scr_cap ^= 1; }) &&
          miss([](StepBufs& c) { c.rope_rows ^= 1; }));
    CHECK(StepBufs() == StepBufs() && destroyed.empty());
    g.clear();
    CHECK(destroyed == std::vector<int>({1}) && g.size() == 0 && !g.find(p, 8, b));
}

static void stale() {
    StepBufs a = some_bufs(1), b = a;
    b.gen_cap ^= 1;                                                // the same addresses handed out again for another size
    {
        Graphs g;
        for (int i = 0; i < 3; ++i) g.insert(plan_of(2, 0), 8 * (i + 1), a, new int(i));
        CHECK(g.size() == 3 && destroyed.empty());
        g.insert(plan_of(2, 0), 8, a, new int(3));                // same bufs (another plan would be the usual reason): nothing goes
        CHECK(g.size() == 4 && destroyed.empty());
        g.insert(plan_of(2, 0), 8, b, new int(4));                // new bufs: the four stale ones go, once each, in order
        CHECK(g.size() == 1 && destroyed == std::vector<int>({0, 1, 2, 3}));
        CHECK(!g.find(plan_of(2, 0), 8, a) && **g.find(plan_of(2, 0), 8, b) == 4);
        g.insert(plan_of(2, 0), 16, b, new int(5));
        g.insert(plan_of(2, 0), 8, a, new int(6));                // and back: the address alone would have matched entry 0..3
        CHECK(g.size() == 1 && destroyed == std::vector<int>({0, 1, 2, 3, 4, 5}) && **g.find(plan_of(2, 0), 8, a) == 6);
        g.insert(plan_of(2, 0), 16, a, new int(7));
        g.clear();
        CHECK(g.size() == 0 && destroyed == std::vector<int>({0, 1, 2, 3, 4, 5, 6, 7}));
        g.clear();
        CHECK(destroyed.size() == 8);
        g.insert(plan_of(2, 0), 8, a, new int(8));                // what is left when the cache dies goes with it
    }
    CHECK(destroyed.size() == 9 && destroyed.back() == 8);
}

static void cap() {
    Graphs g;
    const StepBufs b = some_bufs(2);
    const StepPlan p = plan_of(2, 0);
    for (int i = 0; i < Graphs::CAP; ++i) g.insert(p, i, b, new int(i));
    CHECK(g.size() == (size_t)Graphs::CAP && Graphs::CAP == 256 && destroyed.empty());
    for (int i = 0; i < Graphs::CAP; ++i) CHECK(**g.find(p, i, b) == i);
    g.insert(p, 256, b, new int(256));
    CHECK(g.size() == 1 && destroyed.size() == 256 && **g.find(p, 256, b) == 256 && !g.find(p, 0, b));
    for (int i = 0; i < 256; ++i) CHECK(destroyed[i] == i);
    g.clear();
    CHECK(destroyed.size() == 257);
}

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    const std::string what = argv[1];
    if (what == "options") options();
    else if (what == "sizes") sizes();
    else if (what == "slots") slots();
    else if (what == "key") key();
    else if (what == "stale") stale();
    else if (what == "cap") cap();
    else return 2;
    printf("ok %s\n", what.c_str());
    return 0;
}
