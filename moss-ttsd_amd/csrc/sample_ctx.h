// The row context of the decode-step kernels that read a step's logits (sampler.hip, gen_topk.hip): which logits row a
// (row, channel) pair reads, its vocabulary, and the reference's two hard-coded masks.  One definition, so the sampler
// and generate(top_logprobs=k) cannot disagree about the row they look at.
#pragma once
#include "launch.h"

struct LogitsPtr { const void* p; int f32; };     // one row of logits: bf16 bit patterns, or fp32 in the fp32 engine

struct SampleCtx {         // resolved per (row, channel)
    LogitsPtr lg;
    const uint32_t* bm;
    const uint32_t* ban;   // this step's banned tokens, one bit each (mtts_set_sampler_bans); null: the run has none
    const uint32_t* bias_w;        // this step's tokens with an additive term, one bit each (mtts_set_sampler_bias); null: none
    const MttsBiasTable* bias_t;   // ... and their terms, ascending by id
    int V, mask_id, step, c;
    float penalty, temp;
    uint64_t seed;
    uint32_t row_id;
};

__device__ __forceinline__ bool sample_ctx(SampleCtx& x, int b, int c_in, const uint16_t* logits0,
                                           const uint16_t* logits17, int V0, int Vs, int Vs_pad,
                                           const uint32_t* bitmaps, int bm_words, const MttsSamplerCfg* cfgs,
                                           const LoopState* ls, const SeqState* seqs, int single_vocab, int single_mask,
                                           int single_step, int single_channel, const uint32_t* bans = nullptr,
                                           const uint32_t* bias_w = nullptr, const MttsBiasTable* bias_t = nullptr, int ext = 0) {
    if (single_vocab > 0) {            // unit-test entry: one logits matrix [rows][vocab]
        x.c = single_channel; x.step = single_step; x.V = single_vocab; x.mask_id = single_mask;
        x.seed = 0; x.row_id = (uint32_t)b;
        x.lg = ext ? LogitsPtr{(const float*)logits0 + (size_t)b * x.V, 1} : LogitsPtr{logits0 + (size_t)b * x.V, 0};
        x.bm = bitmaps ? bitmaps + (size_t)b * bm_words : nullptr;
        x.ban = bans ? bans + (size_t)b * ((x.V + 31) >> 5) : nullptr;       // unit-test entry: [rows][ceil(vocab / 32)]
        x.bias_w = bias_w ? bias_w + (size_t)b * ((x.V + 31) >> 5) : nullptr;
        x.bias_t = bias_w ? bias_t + b : nullptr;
    } else {
        if (ls->done) return false;
        const SeqState sq = seqs[b];
        // finished rows get padding from the state machine; a row that finished AT max_length without a flush behind it
        // (active == 2) is still evaluated, as in the reference: see update_kernel
        if (!sq.active || !(sq.unfinished || sq.active == 2)) return false;
        x.c = c_in; x.step = sq.step;
        x.seed = sq.seed; x.row_id = (uint32_t)sq.row_id;
        x.V = (x.c == 0) ? V0 : Vs;
        {
            // channel-0 rows are padded to a multiple of 32 tokens (aligned rows: the head GEMM stores 8 bytes per lane)
            const size_t off = (x.c == 0) ? (size_t)b * ((V0 + 31) & ~31) : ((size_t)b * 7 + (x.c - 1)) * Vs_pad;
            const char* base = (const char*)((x.c == 0) ? logits0 : logits17);
            const int f32 = ext ? 1 : ls->logits_f32;
            x.lg = LogitsPtr{base + off * (f32 ? 4 : 2), f32};
        }
        // modeling_asteroid.py:124-128 (hard-coded ids 1024 / 152694 as in the reference)
        x.mask_id = -1;
        if (x.c != 0 && x.step >= x.c) x.mask_id = 1024;
        if (x.c == 0 && x.step <= 6) x.mask_id = 152694;
        x.bm = bitmaps ? bitmaps + ((size_t)b * 8 + x.c) * bm_words : nullptr;
        x.ban = bans ? bans + ((size_t)b * 8 + x.c) * bm_words : nullptr;    // laid out like the history bitmaps
        x.bias_w = bias_w ? bias_w + ((size_t)b * 8 + x.c) * bm_words : nullptr;
        x.bias_t = bias_w ? bias_t + ((size_t)b * 8 + x.c) : nullptr;
    }
    const MttsSamplerCfg cfg = cfgs[x.c];
    x.penalty = (x.bm && cfg.repetition_penalty > 0.f) ? cfg.repetition_penalty : 0.f;
    x.temp = cfg.temperature;
    // externally scored rows (mtts_step_begin / mtts_step_finish): logits0 / logits17 are the caller's fp32 buffers in the
    // layout above, holding what scores_materialize_kernel wrote and the caller's processors left -- the masks, the bans,
    // the terms and the penalty are in them already; the temperature and everything behind it are still to come
    if (ext) { x.mask_id = -1; x.ban = nullptr; x.bias_w = nullptr; x.bias_t = nullptr; x.penalty = 0.f; }
    return true;
}
