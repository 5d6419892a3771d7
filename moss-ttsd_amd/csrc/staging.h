// Prompt staging, the host half: attention masks read, tokens range-checked and laid out as the rows of a prefill pass,
// history bitmaps and teacher-forcing tails built.  Pure host code, no HIP: engine.hip includes it (mtts_begin /
// mtts_generate, mtts_slot_submit and mtts_score stage through it and upload the result), and so does
// tests/host/pool_stage_main.cpp, which runs it on the CPU under the sanitizers.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "kvpool.h"          // fail(), MTTS_EINVAL; shapes.h: RowMeta, MTTS_MAXR, MTTS_RCAP

// attention_mask of a generation prompt: the left-padded form rpadding() produces (generation_utils.py:221-237) over the
// first `base` = T-7 slots -> *pad = the padded slots in front
static inline int mask_left_padded(const uint8_t* m, int base, int row, int* pad) {
    int p = 0;
    while (p < base && !m[p]) ++p;
    for (int t = p; t < base; ++t)
        if (!m[t]) return fail(MTTS_EINVAL, "attention_mask of row %d is not left-padded", row);
    if (p >= base) return fail(MTTS_EINVAL, "row %d has no real token in the first T-7 slots", row);
    *pad = p;
    return 0;
}
// attention_mask of a scored row: ones, then zeros (real token i sits at position i, the reference's arange(T) positions)
// -> *len = the ones
static inline int mask_ones_then_zeros(const uint8_t* m, int T, int row, int* len) {
    int n = 0;
    while (n < T && m[n]) ++n;
    for (int t = n; t < T; ++t)
        if (m[t]) {
            if (n == 0) return fail(MTTS_EINVAL, "attention_mask of row %d is left-padded: mtts_score takes right-padded or unpadded rows (ones, then zeros)", row);
            return fail(MTTS_EINVAL, "attention_mask of row %d is not ones followed by zeros (right-padded or unpadded rows only)", row);
        }
    *len = n;
    return 0;
}

struct StageSeq {
    const int64_t* toks;     // [n][8]
    int n;
    int slot;                // sequence slot (page-table row) its rows name
    bool last;               // its last row wants logits
    const int64_t* labels;   // [n][8] or null
};
struct StagedRows {
    std::vector<int32_t> toks, labs;     // [Mpad][8]; labs only when asked for
    std::vector<RowMeta> metas;          // [Mpad]
    std::vector<size_t> row0;            // first row of each sequence
    size_t Mpad = 0;
};
// The rows of a prefill: every sequence starts on a 32-row tile boundary, so that a tile holds consecutive positions of
// one sequence (the prefill attention kernels share K/V pages across a tile); filler rows are idle; the total is a whole
// number of MTTS_RCAP rows, at least one.  with_labs: the row of position i carries labels[i + 1] (the HF shift), the last
// position of a sequence and the fillers carry -100.  Tokens must lie inside their channel's vocabulary.
static inline int stage_rows(const std::vector<StageSeq>& seqs, int V0, int Vs, bool with_labs, StagedRows* out) {
    size_t Mtot = 0;
    for (const StageSeq& s : seqs) Mtot += ((size_t)s.n + MTTS_MAXR - 1) / MTTS_MAXR * MTTS_MAXR;
    const size_t Mpad = out->Mpad = std::max<size_t>((Mtot + MTTS_RCAP - 1) / MTTS_RCAP * MTTS_RCAP, MTTS_RCAP);
    out->toks.assign(Mpad * 8, 0);
    out->labs.assign(with_labs ? Mpad * 8 : 0, -100);
    out->metas.assign(Mpad, RowMeta{-1, 0, 0, 0});
    out->row0.assign(seqs.size(), 0);
    size_t r = 0;
    for (size_t b = 0; b < seqs.size(); r = (r + MTTS_MAXR - 1) / MTTS_MAXR * MTTS_MAXR, ++b) {
        const StageSeq& s = seqs[b];
        out->row0[b] = r;
        for (int i = 0; i < s.n; ++i, ++r) {
            for (int c = 0; c < 8; ++c) {
                const int64_t t = s.toks[(size_t)i * 8 + c];
                if (t < 0 || t >= (c == 0 ? V0 : Vs)) return fail(MTTS_EINVAL, "token %lld out of range on channel %d", (long long)t, c);
                out->toks[r * 8 + c] = (int32_t)t;
                if (with_labs && s.labels && i + 1 < s.n) out->labs[r * 8 + c] = (int32_t)s.labels[(size_t)(i + 1) * 8 + c];
            }
            out->metas[r] = RowMeta{s.slot, i, s.last && i == s.n - 1 ? 1 : 0, 0};
        }
    }
    return 0;
}

// history bitmap of one row, bm [8][bm_words], from `n` prompt slots [n][8] (HF repetition penalty sees the whole channel
// incl. pads: modeling_asteroid.py:129).  Padded slots are not range-checked: a value outside the table is skipped.
static inline void stage_bitmap(const int64_t* toks, int n, int bm_words, uint32_t* bm) {
    for (int t = 0; t < n; ++t)
        for (int c = 0; c < 8; ++c) {
            const int64_t tk = toks[(size_t)t * 8 + c];
            if (tk >= 0 && tk < (int64_t)bm_words * 32) bm[(size_t)c * bm_words + (tk >> 5)] |= 1u << (tk & 31);
        }
}
// history of one row for the n-gram ban (mtts_set_sampler_bans), hist [n][8], from the same `n` prompt slots: the token
// stream the bitmap above is built from, in order.  Padded slots are not range-checked here either: a value no int32
// token can equal is kept as -1 (it matches nothing a channel can emit and bans nothing).
static inline void stage_history(const int64_t* toks, int n, int32_t* hist) {
    for (size_t i = 0; i < (size_t)n * 8; ++i) hist[i] = (toks[i] >= 0 && toks[i] <= INT32_MAX) ? (int32_t)toks[i] : -1;
}
// the static bans of one channel, bm [words] (words * 32 >= V): the listed ids inside [0, V); the others are ignored, as
// HF's isin(arange(V), ids) ignores them -- one list meets eight vocabularies
static inline void stage_ban_static(const int32_t* ids, int n, int V, int words, uint32_t* bm) {
    std::fill(bm, bm + words, 0u);
    for (int i = 0; i < n; ++i)
        if (ids[i] >= 0 && ids[i] < V) bm[ids[i] >> 5] |= 1u << (ids[i] & 31);
}
// the sequence rules of one channel (mtts_set_sampler_bias) as the rule kernel reads them: n rules, rule r = the next len[r]
// entries of ids with beta[r].  A rule with an id outside [0, V) is dropped -- it can never match or land on this channel,
// and one list meets eight vocabularies.  The single-token rules go first and the longer ones follow in the caller's order:
// a token's chain starts from its single-token value, as HF's starts from length_1_bias.  bias_stat [words] (null: not
// wanted): the bits of the single-token finite rules, the static part of the bias words.  The caller has checked the
// counts and lengths (PendingRun::set_bias); -> the rules kept
static inline int stage_bias_rules(const int32_t* len, const int32_t* ids, const float* beta, int n, int V, int words, BiasRules* out,
                                   uint32_t* bias_stat) {
    *out = BiasRules();
    if (bias_stat) std::fill(bias_stat, bias_stat + words, 0u);
    for (int pass = 0; pass < 2; ++pass) {          // 0: the single-token rules, 1: the others
        const int32_t* p = ids;
        for (int r = 0; r < n; p += len[r], ++r) {
            if ((len[r] == 1) != (pass == 0) || out->n >= BIAS_RULES || len[r] < 1 || len[r] > BIAS_RULE_LEN) continue;
            bool inside = true;
            for (int k = 0; k < len[r]; ++k) inside = inside && p[k] >= 0 && p[k] < V;
            if (!inside) continue;
            const int o = out->n++;
            out->len[o] = len[r]; out->beta[o] = beta[r];
            std::copy(p, p + len[r], out->ids[o]);
            if (bias_stat && len[r] == 1 && beta[r] > -INFINITY) bias_stat[p[0] >> 5] |= 1u << (p[0] & 31);
        }
    }
    return out->n;
}
// teacher-forcing tail tf_inputs[:, base+s, :] for s = 0..6 (modeling_asteroid.py:143-145): `toks` = those 7 slots,
// tf [7][8]; `note` ends the message of a token outside its vocabulary
static inline int stage_tail(const int64_t* toks, int V0, int Vs, const char* note, int32_t* tf) {
    for (int s = 0; s < 7; ++s)
        for (int c = 0; c < 8; ++c) {
            const int64_t tk = toks[(size_t)s * 8 + c];
            if (tk < 0 || tk >= (c == 0 ? V0 : Vs)) return fail(MTTS_EINVAL, "token %lld out of range on channel %d%s", (long long)tk, c, note);
            tf[s * 8 + c] = (int32_t)tk;
        }
    return 0;
}
