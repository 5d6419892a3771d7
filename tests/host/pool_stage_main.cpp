// The engine's HIP-free host code on the CPU: the KV page pool (csrc/kvpool.h) and the prompt stager (csrc/staging.h).
// One case per run: `pool_stage_main <case>` prints what it found and ends with "ok <case>", exit status 0; a check that
// does not hold prints itself and exits 1.  tests/test_host_pool_cpu.py builds this with the sanitizers and drives it.
// The "device table" is a vector that only the ship callback writes, one (idx, val) of a batch at a time; every pool
// case ends by comparing it with the pool's own table over the owned entries.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <string>

#include "../../include/mtts.h"
#include "../../moss-ttsd_amd/csrc/kvpool.h"
#include "../../moss-ttsd_amd/csrc/staging.h"

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

// ---- the device side of the pool: a table and the batches that reached it --------------------------------------------
struct Device {
    std::vector<int32_t> table;
    std::vector<PageEdits> batches;
    explicit Device(size_t n) : table(n, -1) {}
    auto ship() {
        return [this](const PageEdits& ed) -> int {
            CHECK(ed.n >= 1 && ed.n <= 31);
            std::set<int32_t> seen;
            for (int i = 0; i < ed.n; ++i) {
                CHECK(seen.insert(ed.idx[i]).second);                     // one batch never carries an index twice
                CHECK(ed.idx[i] >= 0 && (size_t)ed.idx[i] < table.size());
                table[ed.idx[i]] = ed.val[i];
            }
            batches.push_back(ed);
            return 0;
        };
    }
};
// the mirror equals the host table over the owned entries, and nothing is pending
static void check_mirror(const KvPool& p, const Device& d, int slots, int max_pages) {
    CHECK(p.pending().n == 0);
    for (int b = 0; b < slots; ++b)
        for (int i = 0; i < p.pages_of(b); ++i) CHECK(d.table[(size_t)b * max_pages + i] == p.entry(b, i));
}
// every page is in at most `most` rows, and free + distinct owned = total
static void check_pages(const KvPool& p, int slots, int total, int most) {
    std::vector<int> rows(total, 0);
    for (int b = 0; b < slots; ++b)
        for (int i = 0; i < p.pages_of(b); ++i) {
            CHECK(p.entry(b, i) >= 0 && p.entry(b, i) < total);
            rows[p.entry(b, i)]++;
        }
    int owned = 0;
    for (int32_t f : p.free_list()) CHECK(f >= 0 && f < total && rows[f] == 0);
    for (int r : rows) { CHECK(r <= most); owned += r > 0; }
    CHECK(owned + p.free_count() == total);
    CHECK(std::set<int32_t>(p.free_list().begin(), p.free_list().end()).size() == p.free_list().size());
}

static void pool_order() {
    KvPool p;
    Device d(9);
    p.init(9, 9, 1, 512, nullptr);
    CHECK(p.free_count() == 9);
    CHECK(p.grow(0, 9, d.ship()) == 0 && p.flush(d.ship()) == 0);
    for (int i = 0; i < 9; ++i) CHECK(p.entry(0, i) == i);
    check_mirror(p, d, 1, 9);
    const uint64_t seed = 17;
    KvPool q;
    Device dq(40);
    q.init(40, 40, 1, 2496, &seed);
    CHECK(q.grow(0, 40, dq.ship()) == 0 && q.flush(dq.ship()) == 0);
    check_mirror(q, dq, 1, 40);
    check_pages(q, 1, 40, 1);
    printf("order");
    for (int i = 0; i < 40; ++i) printf(" %d", q.entry(0, i));
    printf("\n");
}

static void pool_batches() {
    KvPool p;
    Device d(80);
    p.init(80, 80, 1, 5056, nullptr);
    CHECK(p.grow(0, 70, d.ship()) == 0);
    CHECK(d.batches.size() == 2 && p.pending().n == 8);                   // 31 + 31 went out on the way
    CHECK(p.flush(d.ship()) == 0);
    CHECK(d.batches.size() == 3 && p.pages_of(0) == 70 && p.free_count() == 10);
    check_mirror(p, d, 1, 80);
    check_pages(p, 1, 80, 1);
    printf("batches %zu\n", d.batches.size());
}

// tests/test_robustness_gpu.py: test_page_table_consistent_after_enomem_recovery, on the host
static void pool_dry() {
    const int slots = 4, total = 9, mp = 8;
    KvPool p;
    Device d((size_t)slots * mp);
    p.init(total, mp, slots, 448, nullptr);
    CHECK(p.grow(0, 5, d.ship()) == 0);
    const std::vector<int32_t> free_before = p.free_list();
    const int rc = p.grow(1, 5, d.ship());                                // runs dry at its fifth page
    CHECK(rc == MTTS_ENOMEM && strstr(g_err, "KV page pool exhausted (9 pages of 64 tokens): slot 1 needs page 4"));
    CHECK(p.pages_of(0) == 5 && p.pages_of(1) == 4 && p.free_count() == 0);      // nothing is taken back
    CHECK(free_before.size() == 4 && d.batches.empty() && p.pending().n == 9);    // (the state a failed mtts_begin leaves)
    p.release_all();
    CHECK(p.free_count() == total && p.pending().n == 0);
    for (int b = 0; b < 3; ++b) CHECK(p.grow(b, 2, d.ship()) == 0);
    CHECK(p.flush(d.ship()) == 0);
    // no batch carries an edit from before the release: every shipped index is an entry its slot owns now, with its value
    for (const PageEdits& ed : d.batches)
        for (int i = 0; i < ed.n; ++i) {
            const int b = ed.idx[i] / mp, at = ed.idx[i] % mp;
            CHECK(b < 3 && at < p.pages_of(b) && p.entry(b, at) == ed.val[i]);
        }
    check_mirror(p, d, slots, mp);
    check_pages(p, slots, total, 1);                                      // no page is in two rows
    CHECK(p.free_count() == 3);
    printf("free %d\n", p.free_count());
}

static void pool_wide() {
    KvPool p;
    Device d(2 * 6);
    p.init(20, 6, 2, 320, nullptr);
    CHECK(p.grow(0, 2, d.ship()) == 0);
    const std::vector<int32_t> free_before = p.free_list(), counts_before = p.counts();
    CHECK(p.grow(1, 7, d.ship()) == MTTS_ENOMEM);
    CHECK(p.free_list() == free_before && p.counts() == counts_before);
    CHECK(p.flush(d.ship()) == 0);
    check_mirror(p, d, 2, 6);
    printf("error %s\n", g_err);
}

static void pool_shares() {
    const int slots = 3, total = 8, mp = 4;
    KvPool p;
    Device d((size_t)slots * mp);
    p.init(total, mp, slots, 192, nullptr);
    CHECK(p.grow(0, 3, d.ship()) == 0);
    for (int dst = 1; dst <= 2; ++dst) {
        CHECK(p.share(0, dst, 2, d.ship()) == 0);
        CHECK(p.grow(dst, 3, d.ship()) == 0);                             // a private third page
    }
    CHECK(p.flush(d.ship()) == 0);
    for (int dst = 1; dst <= 2; ++dst) {
        CHECK(p.entry(dst, 0) == p.entry(0, 0) && p.entry(dst, 1) == p.entry(0, 1));
        CHECK(p.entry(dst, 2) != p.entry(0, 2));
    }
    CHECK(p.entry(1, 2) != p.entry(2, 2) && p.free_count() == total - 5);
    check_mirror(p, d, slots, mp);
    check_pages(p, slots, total, 3);
    const int32_t s0 = p.entry(0, 0), s1 = p.entry(0, 1);
    p.release(0);                                                         // the source first: the shared pages stay out
    CHECK(p.free_count() == total - 4);
    for (int32_t f : p.free_list()) CHECK(f != s0 && f != s1);
    p.release(1);
    for (int32_t f : p.free_list()) CHECK(f != s0 && f != s1);
    p.release(2);
    CHECK(p.free_count() == total);
    check_pages(p, slots, total, 0);                                      // every page is back exactly once
    check_mirror(p, d, slots, mp);
    // a share that was never shipped goes with its slot
    CHECK(p.grow(0, 3, d.ship()) == 0 && p.flush(d.ship()) == 0);
    CHECK(p.share(0, 1, 2, d.ship()) == 0 && p.pending().n == 2);
    p.release(1);
    for (int i = 0; i < p.pending().n; ++i) CHECK(p.pending().idx[i] / mp != 1);
    CHECK(p.pending().n == 0 && p.pages_of(1) == 0 && p.free_count() == total - 3);
    check_mirror(p, d, slots, mp);
    check_pages(p, slots, total, 1);
    printf("free %d\n", p.free_count());
}

// mtts_score's borrow: rows 0..2 still list pages of an ended run, the free list is in a shuffled state
static void pool_borrow() {
    const int slots = 4, total = 24, mp = 6;
    const uint64_t seed = 5;
    KvPool p;
    Device d((size_t)slots * mp);
    p.init(total, mp, slots, 320, &seed);
    const int ended[4] = {2, 3, 1, 2}, scored[3] = {4, 1, 2};
    for (int b = 0; b < slots; ++b) CHECK(p.grow(b, ended[b], d.ship()) == 0);
    p.release(3);                                                         // (a finished row gave its pages back out of order)
    CHECK(p.flush(d.ship()) == 0);
    const std::vector<int32_t> free0 = p.free_list(), counts0 = p.counts();
    std::vector<int32_t> owned0, mirror0;
    for (int b = 0; b < slots; ++b)
        for (int i = 0; i < p.pages_of(b); ++i) { owned0.push_back(p.entry(b, i)); mirror0.push_back(d.table[(size_t)b * mp + i]); }
    const KvPool::Kept kept = p.set_aside(3);
    for (int b = 0; b < 3; ++b) CHECK(p.pages_of(b) == 0 && (int)kept[b].size() == ended[b]);
    CHECK(p.free_list() == free0);                                        // set aside, not released
    for (int b = 0; b < 3; ++b) CHECK(p.grow(b, scored[b], d.ship()) == 0);
    CHECK(p.flush(d.ship()) == 0);
    check_mirror(p, d, slots, mp);
    for (int b = 0; b < 3; ++b)                                           // the borrowed pages are none of the kept ones
        for (int i = 0; i < p.pages_of(b); ++i)
            for (const auto& k : kept) for (int32_t page : k) CHECK(p.entry(b, i) != page);
    CHECK(p.restore(kept, d.ship()) == 0);
    CHECK(p.free_list() == free0 && p.counts() == counts0);               // element for element
    std::vector<int32_t> owned1, mirror1;
    for (int b = 0; b < slots; ++b)
        for (int i = 0; i < p.pages_of(b); ++i) { owned1.push_back(p.entry(b, i)); mirror1.push_back(d.table[(size_t)b * mp + i]); }
    CHECK(owned1 == owned0 && mirror1 == mirror0);
    check_mirror(p, d, slots, mp);
    check_pages(p, slots, total, 1);
    printf("free %d\n", p.free_count());
}

// ---- the stager ------------------------------------------------------------------------------------------------------
static const int V0 = 300, VS = 100;
static std::vector<int64_t> tokens(int n, int salt) {                     // [n][8], inside the vocabularies
    std::vector<int64_t> t((size_t)n * 8);
    for (int i = 0; i < n; ++i)
        for (int c = 0; c < 8; ++c) t[(size_t)i * 8 + c] = (i * 7 + c * 13 + salt) % (c == 0 ? V0 : VS);
    return t;
}
static void check_filler(const StagedRows& sr, size_t r) {
    CHECK(sr.metas[r].seq == -1 && sr.metas[r].pos == 0 && sr.metas[r].last == 0 && sr.metas[r].pad == 0);
    for (int c = 0; c < 8; ++c) {
        CHECK(sr.toks[r * 8 + c] == 0);
        if (!sr.labs.empty()) CHECK(sr.labs[r * 8 + c] == -100);
    }
}

static void stage_lengths() {
    const int lens[5] = {1, 31, 32, 33, 65};
    const size_t want0[5] = {0, 32, 64, 96, 160};
    std::vector<std::vector<int64_t>> t;
    for (int b = 0; b < 5; ++b) t.push_back(tokens(lens[b], b));
    for (int last = 0; last < 2; ++last) {
        std::vector<StageSeq> seqs;
        for (int b = 0; b < 5; ++b) seqs.push_back(StageSeq{t[b].data(), lens[b], 10 + b, last != 0, nullptr});
        StagedRows sr;
        CHECK(stage_rows(seqs, V0, VS, false, &sr) == 0);
        CHECK(sr.Mpad == 256 && sr.toks.size() == 256 * 8 && sr.metas.size() == 256 && sr.labs.empty());
        std::vector<char> real(sr.Mpad, 0);
        int lasts = 0;
        for (int b = 0; b < 5; ++b) {
            CHECK(sr.row0[b] == want0[b]);
            for (int i = 0; i < lens[b]; ++i) {
                const size_t r = sr.row0[b] + i;
                real[r] = 1;
                CHECK(sr.metas[r].seq == 10 + b && sr.metas[r].pos == i && sr.metas[r].pad == 0);
                CHECK(sr.metas[r].last == (last && i == lens[b] - 1 ? 1 : 0));
                lasts += sr.metas[r].last;
                for (int c = 0; c < 8; ++c) CHECK(sr.toks[r * 8 + c] == t[b][(size_t)i * 8 + c]);
            }
        }
        CHECK(lasts == (last ? 5 : 0));
        for (size_t r = 0; r < sr.Mpad; ++r)
            if (!real[r]) check_filler(sr, r);
    }
    printf("mpad 256\n");
}

static void stage_one() {
    const std::vector<int64_t> t = tokens(1, 3);
    StagedRows sr;
    CHECK(stage_rows({StageSeq{t.data(), 1, 0, true, nullptr}}, V0, VS, false, &sr) == 0);
    CHECK(sr.Mpad == 128 && sr.row0[0] == 0 && sr.metas[0].seq == 0 && sr.metas[0].last == 1);
    for (size_t r = 1; r < sr.Mpad; ++r) check_filler(sr, r);
    StagedRows none;                                                      // no sequence at all is still one whole pass
    CHECK(stage_rows({}, V0, VS, true, &none) == 0 && none.Mpad == 128);
    for (size_t r = 0; r < none.Mpad; ++r) check_filler(none, r);
    printf("mpad %zu\n", sr.Mpad);
}

static void stage_labels() {
    const int T = 6, lens[2] = {5, 3};
    const std::vector<int64_t> ids = tokens(2 * T, 1);                    // [2][T][8], right-padded
    std::vector<int64_t> labels((size_t)2 * T * 8, -100);
    for (int b = 0; b < 2; ++b)
        for (int i = 0; i < lens[b]; ++i)
            for (int c = 0; c < 8; ++c) labels[((size_t)b * T + i) * 8 + c] = 1000 * b + 10 * i + c;
    std::vector<StageSeq> seqs;
    for (int b = 0; b < 2; ++b) seqs.push_back(StageSeq{ids.data() + (size_t)b * T * 8, lens[b], b, false, labels.data() + (size_t)b * T * 8});
    StagedRows sr;
    CHECK(stage_rows(seqs, V0, VS, true, &sr) == 0);
    CHECK(sr.Mpad == 128 && sr.labs.size() == 128 * 8 && sr.row0[0] == 0 && sr.row0[1] == 32);
    std::vector<char> real(sr.Mpad, 0);
    for (int b = 0; b < 2; ++b)
        for (int i = 0; i < lens[b]; ++i) {
            const size_t r = sr.row0[b] + i;
            real[r] = 1;
            CHECK(sr.metas[r].seq == b && sr.metas[r].pos == i && sr.metas[r].last == 0);
            for (int c = 0; c < 8; ++c) CHECK(sr.labs[r * 8 + c] == (i + 1 < lens[b] ? 1000 * b + 10 * (i + 1) + c : -100));
        }
    for (size_t r = 0; r < sr.Mpad; ++r)
        if (!real[r]) check_filler(sr, r);
    printf("labels ok\n");
}

// every refusal prints "<name>: <code>: <message>"
static void refused(const char* name, int rc) {
    CHECK(rc == MTTS_EINVAL);
    printf("%s: %d: %s\n", name, rc, g_err);
}
static void stage_refusals() {
    const struct { const char* name; int row, ch; int64_t tok; } bad[3] = {{"negative", 2, 3, -1}, {"speech", 0, 5, VS}, {"text", 4, 0, V0}};
    for (const auto& b : bad) {
        std::vector<int64_t> t = tokens(5, 0);
        t[(size_t)b.row * 8 + b.ch] = b.tok;
        StagedRows sr;
        refused(b.name, stage_rows({StageSeq{t.data(), 5, 0, true, nullptr}}, V0, VS, false, &sr));
    }
    int out = -1;
    const uint8_t hole[6] = {0, 1, 1, 0, 1, 1}, zeros[6] = {0, 0, 0, 0, 0, 0}, left[6] = {0, 0, 1, 1, 1, 1}, right[6] = {1, 1, 1, 0, 0, 0};
    refused("left hole", mask_left_padded(hole, 6, 2, &out));
    refused("left empty", mask_left_padded(zeros, 6, 1, &out));
    refused("right left-padded", mask_ones_then_zeros(left, 6, 3, &out));
    const uint8_t rhole[6] = {1, 1, 0, 1, 0, 0};
    refused("right hole", mask_ones_then_zeros(rhole, 6, 4, &out));
    CHECK(out == -1);                                                     // a refusal writes nothing
    CHECK(mask_left_padded(left, 6, 0, &out) == 0 && out == 2);
    CHECK(mask_ones_then_zeros(right, 6, 0, &out) == 0 && out == 3);
    CHECK(mask_ones_then_zeros(zeros, 6, 0, &out) == 0 && out == 0);
    std::vector<int64_t> tail = tokens(7, 2);
    tail[3 * 8 + 6] = VS;
    int32_t tf[56];
    refused("tail", stage_tail(tail.data(), V0, VS, " (delayed tail)", tf));
}

static void stage_bitmap_tail() {
    const int T = 11, base = 4, words = (V0 + 31) / 32;
    std::vector<int64_t> ids = tokens(T, 5);
    ids[0 * 8 + 2] = 1000000;                                             // padded slots are not range-checked: outside the
    ids[1 * 8 + 0] = -1;                                                  // table means skipped, not reported
    ids[2 * 8 + 7] = (int64_t)words * 32;
    ids[3 * 8 + 1] = (int64_t)words * 32 - 1;                             // the table's last bit
    std::vector<uint32_t> bm((size_t)8 * words, 0u), want((size_t)8 * words, 0u);
    stage_bitmap(ids.data(), base, words, bm.data());
    int bits = 0;
    for (int t = 0; t < base; ++t)
        for (int c = 0; c < 8; ++c) {
            const int64_t tk = ids[(size_t)t * 8 + c];
            if (tk < 0 || tk >= (int64_t)words * 32) continue;
            uint32_t& w = want[(size_t)c * words + tk / 32];
            bits += !(w >> (tk % 32) & 1u);
            w |= 1u << (tk % 32);
        }
    CHECK(bm == want && bits > 0 && (want[(size_t)1 * words + words - 1] >> 31 & 1u));
    int32_t tf[56];
    CHECK(stage_tail(ids.data() + (size_t)base * 8, V0, VS, "", tf) == 0);
    for (int s = 0; s < 7; ++s)
        for (int c = 0; c < 8; ++c) CHECK(tf[s * 8 + c] == ids[(size_t)(base + s) * 8 + c]);
    printf("bits %d\n", bits);
}

int main(int argc, char** argv) {
    const struct { const char* name; void (*run)(); } cases[] = {
        {"pool_order", pool_order}, {"pool_batches", pool_batches}, {"pool_dry", pool_dry}, {"pool_wide", pool_wide},
        {"pool_shares", pool_shares}, {"pool_borrow", pool_borrow}, {"stage_lengths", stage_lengths}, {"stage_one", stage_one},
        {"stage_labels", stage_labels}, {"stage_refusals", stage_refusals}, {"stage_bitmap_tail", stage_bitmap_tail}};
    for (const auto& c : cases)
        if (argc == 2 && !strcmp(argv[1], c.name)) {
            c.run();
            printf("ok %s\n", c.name);
            return 0;
        }
    printf("usage: pool_stage_main <case>\n");
    return 2;
}
