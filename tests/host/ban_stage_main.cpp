// Stand-alone host program for tests/test_sampler_bans_cpu.py: the host half of the hard bans (mtts_set_sampler_bans) on
// the CPU, nothing of HIP -- csrc/staging.h (stage_history, stage_ban_static) and csrc/runstate.h (PendingRun::set_bans,
// StepBufs).  One case per run: `ban_stage_main <case>` ends with "ok <case>", exit status 0; a check that does not hold
// prints itself and exits 1.  Built with -fsanitize=address,undefined.
//   history    stage_history is the token stream stage_bitmap sets bits from, a left-padded row included
//   static     stage_ban_static: ids inside the vocabulary only, the last word's bits at and above V stay 0
//   bans       PendingRun::set_bans: validation with the channel named, one-shot through take() and take_bans()
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

static void history() {
    // a left-padded prompt row of 9 slots: 3 padded slots (whatever the caller left there, out-of-table values included),
    // then 6 real ones; channel 0 over 200 tokens, the others over 40
    const int n = 9, words = 7;         // 7 * 32 = 224 >= 200
    std::vector<int64_t> toks((size_t)n * 8);
    for (int t = 0; t < n; ++t)
        for (int c = 0; c < 8; ++c) toks[(size_t)t * 8 + c] = t < 3 ? (c == 0 ? 199 : 39) : (c == 0 ? 100 + 7 * t : (5 * t + c) % 40);
    toks[0 * 8 + 2] = -5;                       // padded slots are not range-checked: skipped by the bitmap, -1 in the history
    toks[1 * 8 + 3] = (int64_t)1 << 40;
    toks[2 * 8 + 4] = 223;                      // inside the table though outside the vocabulary: both keep it
    std::vector<int32_t> hist((size_t)n * 8, 77);
    stage_history(toks.data(), n, hist.data());
    std::vector<uint32_t> bm((size_t)8 * words, 0u), from_hist((size_t)8 * words, 0u);
    stage_bitmap(toks.data(), n, words, bm.data());
    for (int t = 0; t < n; ++t)
        for (int c = 0; c < 8; ++c) {
            const int32_t h = hist[(size_t)t * 8 + c];
            const int64_t tk = toks[(size_t)t * 8 + c];
            CHECK(h == ((tk >= 0 && tk <= INT32_MAX) ? (int32_t)tk : -1));
            if (h >= 0 && h < words * 32) from_hist[(size_t)c * words + (h >> 5)] |= 1u << (h & 31);
        }
    CHECK(hist[2] == -1 && hist[8 + 3] == -1 && hist[16 + 4] == 223 && hist[0] == 199 && hist[3 * 8] == 121);
    CHECK(bm == from_hist);                     // the same stream: the bits of the history are the bitmap's
    stage_history(toks.data(), 0, nullptr);     // an empty prompt part touches nothing
}

static void statics() {
    const int32_t ids[] = {3, 17, 1000, 1024, 1030, 5000, 152000, 3};
    const int V = 1025, words = (V + 31) / 32;  // 33 words, the last holds token 1024 alone
    std::vector<uint32_t> bm(words, 0xdeadbeefu);
    stage_ban_static(ids, 8, V, words, bm.data());
    for (int i = 0; i < words * 32; ++i) {
        const bool want = i == 3 || i == 17 || i == 1000 || i == 1024;
        CHECK((((bm[i >> 5] >> (i & 31)) & 1u) != 0) == want);
    }
    CHECK(bm[32] == 1u);                        // bits at and above V stay 0
    std::vector<uint32_t> big(4772, 1u);
    stage_ban_static(ids, 8, 152697, 4772, big.data());
    int set = 0;
    for (uint32_t w : big) set += __builtin_popcount(w);
    CHECK(set == 7 && ((big[152000 >> 5] >> (152000 & 31)) & 1u));
    stage_ban_static(nullptr, 0, V, words, bm.data());     // none: all clear (the overwrite is the clear)
    for (uint32_t w : bm) CHECK(w == 0u);
}

static void bans() {
    const int32_t sup[] = {5, 9, 2000};
    MttsSamplerBans b[8];
    for (int c = 0; c < 8; ++c) b[c] = MttsSamplerBans{c == 0 ? 3 : 2, c == 1 ? 5 : 0, c < 2 ? 3 : 0, c < 2 ? sup : nullptr};
    PendingRun p;
    CHECK(!p.take(2).bans.any() && p.take_bans().ch.empty());
    CHECK(p.set_bans(b) == 0);
    RunOptions o = p.take(2);
    CHECK(o.bans.ch.size() == 8 && o.bans.any() && o.bans.ngram() && o.bans.ch[0].ngram == 3 && o.bans.ch[1].min_new == 5 &&
          o.bans.ch[1].suppress == std::vector<int32_t>({5, 9, 2000}) && o.bans.ch[7].suppress.empty() && o.bans.ch[7].ngram == 2);
    CHECK(p.take(2).bans.ch.empty());                       // one-shot
    CHECK(p.set_bans(b) == 0);
    CHECK(p.take_bans().ch.size() == 8 && p.take_bans().ch.empty() && p.take(1).bans.ch.empty());   // the scheduler's take, once
    CHECK(p.set_bans(b) == 0 && p.set_bans(nullptr) == 0 && p.take(1).bans.ch.empty());            // NULL: none
    // the lists are copied when they are set
    {
        std::vector<int32_t> tmp = {1, 2};
        MttsSamplerBans t[8] = {};
        t[4] = MttsSamplerBans{0, 0, 2, tmp.data()};
        CHECK(p.set_bans(t) == 0);
        tmp.assign(2, 99);
    }
    o = p.take(1);
    CHECK(o.bans.any() && !o.bans.ngram() && o.bans.ch[4].suppress == std::vector<int32_t>({1, 2}));
    // static-only and all-zero tables
    MttsSamplerBans z[8] = {};
    CHECK(p.set_bans(z) == 0);
    o = p.take(1);
    CHECK(o.bans.ch.size() == 8 && !o.bans.any() && !o.bans.ngram());
    // refusals name the channel and leave nothing pending
    const auto refused = [&](int c, MttsSamplerBans bad, const char* text) {
        MttsSamplerBans t[8];
        for (int i = 0; i < 8; ++i) t[i] = b[i];
        t[c] = bad;
        CHECK(p.set_bans(b) == 0);
        g_err[0] = 0;
        CHECK(p.set_bans(t) == RUN_EINVAL);
        CHECK(std::string(g_err) == text);
        CHECK(p.take(1).bans.ch.empty());
    };
    const int32_t neg[] = {4, -1};
    refused(3, MttsSamplerBans{17, 0, 0, nullptr}, "channel 3: no_repeat_ngram_size 17 is outside [0, 16]");
    refused(0, MttsSamplerBans{-1, 0, 0, nullptr}, "channel 0: no_repeat_ngram_size -1 is outside [0, 16]");
    refused(7, MttsSamplerBans{0, -2, 0, nullptr}, "channel 7: min_new_tokens -2 is negative");
    refused(5, MttsSamplerBans{0, 0, 2, neg}, "channel 5: suppress_tokens holds the negative id -1");
    refused(2, MttsSamplerBans{0, 0, 2, nullptr}, "channel 2: suppress_tokens: 2 ids and no list");
    refused(2, MttsSamplerBans{0, 0, -1, sup}, "channel 2: suppress_tokens: -1 ids and a list");
    MttsSamplerBans top[8] = {};
    top[6].no_repeat_ngram_size = MTTS_NGRAM_MAX;
    CHECK(p.set_bans(top) == 0 && p.take(1).bans.ch[6].ngram == 16);
}

static void bufs() {
    static_assert(std::has_unique_object_representations<StepBufs>::value, "no padding");
    const StepBufs a;
    const auto differs = [&](void (*edit)(StepBufs&)) { StepBufs c = a; edit(c); return c != a; };
    CHECK(differs([](StepBufs& c) { c.d_ban = (uint32_t*)8; }) && differs([](StepBufs& c) { c.d_ban_static = (uint32_t*)8; }) &&
          differs([](StepBufs& c) { c.d_hist = (int32_t*)8; }) && differs([](StepBufs& c) { c.hist_cap ^= 1; }) &&
          differs([](StepBufs& c) { c.ban_words ^= 1; }));
    CHECK(a.d_ban == nullptr && a.d_ban_static == nullptr && a.d_hist == nullptr && a.hist_cap == 0 && a.ban_words == 0);
}

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    const std::string what = argv[1];
    if (what == "history") history();
    else if (what == "static") statics();
    else if (what == "bans") bans();
    else if (what == "bufs") bufs();
    else return 2;
    printf("ok %s\n", what.c_str());
    return 0;
}
