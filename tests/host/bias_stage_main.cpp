// Stand-alone host program for tests/test_sampler_bias_cpu.py: the host half of the sequence rules (mtts_set_sampler_bias) on
// the CPU, nothing of HIP -- csrc/staging.h (stage_bias_rules), csrc/runstate.h (PendingRun::set_bias, StepBufs) and
// csrc/stepplan.h (bias_on / bias_terms).  One case per run: `bias_stage_main <case>` ends with "ok <case>", exit status 0;
// a check that does not hold prints itself and exits 1.  Built with -fsanitize=address,undefined.
//   rules      stage_bias_rules: rules inside the vocabulary only, the single-token ones first, the static bias words
//   bias       PendingRun::set_bias: validation with the channel named, the lists copied, one-shot through take() and take_bias()
//   plan       bias_on / bias_terms travel from StepState into the plan and take part in its equality and its text
//   bufs       the new StepBufs members take part in the bytewise comparison
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <string>

#include "../../moss-ttsd_amd/csrc/staging.h"
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

static const float NINF = -INFINITY;

static void rules() {
    // six rules: a 2-token one, a single, a 3-token one with an id outside 1025, a -inf single, a single at V-1, a 16-token one
    std::vector<int32_t> len = {2, 1, 3, 1, 1, 16}, ids = {7, 9, 5, 3, 1030, 4, 14, 1024};
    for (int k = 0; k < 16; ++k) ids.push_back(100 + k);
    const std::vector<float> beta = {0.25f, 0.1f, 2.f, NINF, -1.5f, 3.f};
    const int V = 1025, words = (V + 31) / 32;
    BiasRules r;
    memset(&r, 0x5a, sizeof(r));
    std::vector<uint32_t> stat(words, 0xdeadbeefu);
    CHECK(stage_bias_rules(len.data(), ids.data(), beta.data(), 6, V, words, &r, stat.data()) == 5);
    // singles first (5, 14 at -inf, 1024), then (7, 9) and the 16-token rule; (3, 1030, 4) is gone
    CHECK(r.n == 5 && r.len[0] == 1 && r.len[1] == 1 && r.len[2] == 1 && r.len[3] == 2 && r.len[4] == 16);
    CHECK(r.ids[0][0] == 5 && r.ids[1][0] == 14 && r.ids[2][0] == 1024 && r.ids[3][0] == 7 && r.ids[3][1] == 9 && r.ids[4][15] == 115);
    CHECK(r.beta[0] == 0.1f && r.beta[1] == NINF && r.beta[2] == -1.5f && r.beta[3] == 0.25f && r.beta[4] == 3.f);
    for (int i = 0; i < words * 32; ++i) CHECK((((stat[i >> 5] >> (i & 31)) & 1u) != 0) == (i == 5 || i == 1024));    // finite singles only
    CHECK(stat[32] == 1u);
    // the same list on 152 697 tokens keeps all six; no static words wanted
    CHECK(stage_bias_rules(len.data(), ids.data(), beta.data(), 6, 152697, 4772, &r, nullptr) == 6 && r.len[3] == 2 && r.len[4] == 3 && r.ids[4][1] == 1030);
    // none: an empty table, clear words
    CHECK(stage_bias_rules(nullptr, nullptr, nullptr, 0, V, words, &r, stat.data()) == 0 && r.n == 0);
    for (uint32_t w : stat) CHECK(w == 0u);
    // 64 rules of 16 tokens fill the table to its last entry
    std::vector<int32_t> l64(64, 16), i64(64 * 16);
    std::vector<float> b64(64, 1.f);
    for (int i = 0; i < 64 * 16; ++i) i64[i] = i;
    CHECK(stage_bias_rules(l64.data(), i64.data(), b64.data(), 64, 152697, 4772, &r, nullptr) == 64 && r.ids[63][15] == 1023);
}

static void bias() {
    const int32_t len[] = {1, 2}, ids[] = {5, 7, 9}, beg[] = {3, 2000};
    const float beta[] = {0.5f, NINF};
    MttsSamplerBias b[8];
    for (int c = 0; c < 8; ++c) b[c] = MttsSamplerBias{c < 2 ? 2 : 0, c == 1 ? 40 : 0, c == 7 ? 2 : 0, len, ids, beta, c == 7 ? beg : nullptr};
    PendingRun p;
    CHECK(!p.take(2).bias.any() && p.take_bias().ch.empty());
    CHECK(p.set_bias(b) == 0);
    RunOptions o = p.take(2);
    CHECK(o.bias.ch.size() == 8 && o.bias.any() && o.bias.rules() && o.bias.finite() && o.bias.bans() && o.bias.history() && o.bias.begin());
    CHECK(o.bias.ch[0].len == std::vector<int32_t>({1, 2}) && o.bias.ch[0].ids == std::vector<int32_t>({5, 7, 9}) && o.bias.ch[1].min_length == 40 &&
          o.bias.ch[7].begin == std::vector<int32_t>({3, 2000}) && o.bias.ch[7].len.empty() && o.bias.ch[0].beta[1] == NINF);
    CHECK(p.take(2).bias.ch.empty());                       // one-shot
    CHECK(p.set_bias(b) == 0);
    CHECK(p.take_bias().ch.size() == 8 && p.take_bias().ch.empty() && p.take(1).bias.ch.empty());   // the scheduler's take, once
    CHECK(p.set_bias(b) == 0 && p.set_bias(nullptr) == 0 && p.take(1).bias.ch.empty());            // NULL: none
    // the lists are copied when they are set
    {
        std::vector<int32_t> l = {1}, i = {4};
        std::vector<float> f = {0.25f};
        MttsSamplerBias t[8] = {};
        t[4] = MttsSamplerBias{1, 0, 0, l.data(), i.data(), f.data(), nullptr};
        CHECK(p.set_bias(t) == 0);
        l[0] = 9; i[0] = 99; f[0] = 9.f;
    }
    o = p.take(1);
    CHECK(o.bias.rules() && o.bias.finite() && !o.bias.bans() && !o.bias.history() && !o.bias.begin() && o.bias.ch[4].ids == std::vector<int32_t>({4}) &&
          o.bias.ch[4].beta[0] == 0.25f);
    // what each setting turns on
    {
        MttsSamplerBias t[8] = {};
        const int32_t l1[] = {1}, i1[] = {4};
        t[2] = MttsSamplerBias{1, 0, 0, l1, i1, &NINF, nullptr};
        CHECK(p.set_bias(t) == 0);
        o = p.take(1);
        CHECK(o.bias.rules() && !o.bias.finite() && o.bias.bans() && !o.bias.history());
        MttsSamplerBias m[8] = {};
        m[0].min_length = 3;
        CHECK(p.set_bias(m) == 0);
        o = p.take(1);
        CHECK(o.bias.any() && !o.bias.rules() && !o.bias.finite() && o.bias.bans());
        MttsSamplerBias z[8] = {};
        CHECK(p.set_bias(z) == 0);
        o = p.take(1);
        CHECK(o.bias.ch.size() == 8 && !o.bias.any() && !o.bias.bans() && !o.bias.rules());
    }
    // refusals name the channel and leave nothing pending
    const auto refused = [&](int c, MttsSamplerBias bad, const char* text) {
        MttsSamplerBias t[8];
        for (int i = 0; i < 8; ++i) t[i] = b[i];
        t[c] = bad;
        CHECK(p.set_bias(b) == 0);
        g_err[0] = 0;
        CHECK(p.set_bias(t) == RUN_EINVAL);
        if (std::string(g_err) != text) printf("got: %s\n", g_err);
        CHECK(std::string(g_err) == text);
        CHECK(p.take(1).bias.ch.empty());
    };
    const int32_t l17[] = {17}, l0[] = {0}, neg[] = {4, -1}, l2[] = {2};
    const float inf = INFINITY, nan = NAN, one = 1.f;
    refused(3, MttsSamplerBias{65, 0, 0, len, ids, beta, nullptr}, "channel 3: 65 sequence_bias / bad_words_ids rules, at most 64");
    refused(0, MttsSamplerBias{-1, 0, 0, len, ids, beta, nullptr}, "channel 0: -1 sequence_bias / bad_words_ids rules, at most 64");
    refused(6, MttsSamplerBias{1, 0, 0, l17, ids, &one, nullptr}, "channel 6: rule 0 has 17 tokens, a rule has 1 to 16");
    refused(6, MttsSamplerBias{1, 0, 0, l0, ids, &one, nullptr}, "channel 6: rule 0 has 0 tokens, a rule has 1 to 16");
    refused(5, MttsSamplerBias{1, 0, 0, l2, neg, &one, nullptr}, "channel 5: rule 0 holds the negative id -1");
    refused(4, MttsSamplerBias{1, 0, 0, len, ids, &inf, nullptr}, "channel 4: rule 0 has the bias inf (NaN and +inf are refused)");
    refused(4, MttsSamplerBias{1, 0, 0, len, ids, &nan, nullptr}, "channel 4: rule 0 has the bias nan (NaN and +inf are refused)");
    refused(2, MttsSamplerBias{1, 0, 0, len, nullptr, &one, nullptr}, "channel 2: 1 rules and a list missing");
    refused(7, MttsSamplerBias{0, -2, 0, nullptr, nullptr, nullptr, nullptr}, "channel 7: min_length -2 is negative");
    refused(1, MttsSamplerBias{0, 0, 2, nullptr, nullptr, nullptr, nullptr}, "channel 1: begin_suppress_tokens: 2 ids and no list");
    refused(1, MttsSamplerBias{0, 0, 2, nullptr, nullptr, nullptr, neg}, "channel 1: begin_suppress_tokens holds the negative id -1");
}

static void plan() {
    StepKnobs k;
    StepCaps c;
    c.f32 = true;                       // the plan says F32 and nothing more: the sampler's flags alone
    StepState s;
    s.B = 2; s.R = 2;
    const StepPlan none = plan_step(k, c, s);
    CHECK(!none.bias_on && !none.bias_terms && describe(none).find("bias") == std::string::npos && describe(none).find("rules") == std::string::npos);
    s.bias_on = true;
    const StepPlan rules_only = plan_step(k, c, s);
    s.bias_terms = true;
    const StepPlan terms = plan_step(k, c, s);
    CHECK(rules_only.bias_on && !rules_only.bias_terms && terms.bias_on && terms.bias_terms);
    CHECK(none != rules_only && rules_only != terms && none != terms && terms == plan_step(k, c, s));
    CHECK(describe(rules_only).find(" rules") != std::string::npos && describe(terms).find(" bias") != std::string::npos);
    s.bias_on = false;                  // terms without rules is no state of a run
    CHECK(plan_step(k, c, s) == none);
    s.heads = 2; s.bias_on = true;      // a prefill pass samples nothing
    CHECK(!plan_step(k, c, s).bias_on);
}

static void bufs() {
    static_assert(std::has_unique_object_representations<StepBufs>::value, "no padding");
    const StepBufs a;
    const auto differs = [&](void (*edit)(StepBufs&)) { StepBufs c = a; edit(c); return c != a; };
    CHECK(differs([](StepBufs& c) { c.d_ban_begin = (uint32_t*)8; }) && differs([](StepBufs& c) { c.d_bias_rules = (BiasRules*)8; }) &&
          differs([](StepBufs& c) { c.d_bias_w = (uint32_t*)8; }) && differs([](StepBufs& c) { c.d_bias_static = (uint32_t*)8; }) &&
          differs([](StepBufs& c) { c.d_bias_tab = (MttsBiasTable*)8; }));
    CHECK(a.d_ban_begin == nullptr && a.d_bias_rules == nullptr && a.d_bias_w == nullptr && a.d_bias_static == nullptr && a.d_bias_tab == nullptr);
    static_assert(sizeof(MttsBiasTable) == 4 + 8 * MTTS_BIAS_RULES_MAX && BIAS_RULES == MTTS_BIAS_RULES_MAX && BIAS_RULE_LEN == MTTS_BIAS_RULE_LEN_MAX, "");
}

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    const std::string what = argv[1];
    if (what == "rules") rules();
    else if (what == "bias") bias();
    else if (what == "plan") plan();
    else if (what == "bufs") bufs();
    else return 2;
    printf("ok %s\n", what.c_str());
    return 0;
}
