// The sizes and the row descriptor that the HIP-free host headers (kvpool.h, staging.h, stepplan.h) share with the kernels.
// No HIP in here: common.h includes it for the device side.
#pragma once
#include <stdint.h>

#define MTTS_MAXR 32          // rows per MFMA N-tile (one activation fragment tile)
#define MTTS_RCAP 128         // dialogue slots; rows of a decode pass (up to 4 activation tiles share one weight stream)
#define MTTS_PFCAP 2048       // rows of a prefill pass (tiled GEMM); also the row stride of the split-K slabs
#define MTTS_PAGE 64          // tokens per KV page
#define ATT_PB 8              // KV pages per pass-B chunk, decode rows (4 waves x 2 pages)
#define ATT_PF 2              // KV pages per pass-B chunk, prefill tiles (one wave)
#define SMALL_RP 4            // rows of the small-batch decode path (common.h: SmallPro)

// Per-row metadata of one forward pass.
struct RowMeta {
    int32_t seq;     // sequence slot (page-table row), -1 = inactive row
    int32_t pos;     // position of this token = its index among the sequence's real tokens
    int32_t last;    // 1 if logits are wanted for this row
    int32_t pad;
};

// One channel's sequence rules (mtts_set_sampler_bias) as the rule kernel reads them (sampler.hip: bias_kernel), flattened
// by the host (staging.h: stage_bias_rules): the single-token rules first, then the longer ones in the caller's order, so
// a token's fp32 chain is the rules' order.  Rule r is ids[r][0 .. len[r]), its last id the token that carries beta[r].
#define BIAS_RULES 64         // MTTS_BIAS_RULES_MAX of include/mtts.h (sampler.hip checks that it is)
#define BIAS_RULE_LEN 16      // MTTS_BIAS_RULE_LEN_MAX
struct BiasRules {
    int32_t n;
    int32_t len[BIAS_RULES];
    float beta[BIAS_RULES];
    int32_t ids[BIAS_RULES][BIAS_RULE_LEN];
};

// The weight kinds that also exist as a sealed twin (gemm_sealed.hip)
enum { WSEAL_GU = 0, WSEAL_DOWN = 1, WSEAL_HEAD0 = 2, WSEAL_HEADS = 3, WSEAL_KINDS = 4 };

// The kernel launch_gemm gives a decode GEMM (gemm.hip: mtts_gemm_form)
enum { GEMM_SKINNY = 0, GEMM_DEPTH = 1, GEMM_GATEUP48 = 2 };

// ---- block shapes of the decode attention kernels (attn.hip) and the LDS of the whole-row one -------------------------
#ifndef PV_WAVES
#define PV_WAVES 4            // waves per pass-B block (ATT_PB / PV_WAVES pages each)
#endif
#ifndef ROW_WAVES
#define ROW_WAVES 12          // waves per whole-row block: 3 per SIMD, at most 168 registers each (the sealed-page bodies take
                              // 138-152; 16 waves would have to fit 128, spill, and lose: profiles/attn_row_ab.json; 8 is no faster)
#endif
// Dynamic LDS of an attn_row_kernel block: q, the new K / V rows, the per-wave rescaled q and probability pairs, then per
// page of the launch's bound G x (8 B of pairs + 128 B of scores) and per chunk 4 x G x 512 B of item vectors.  The launch
// (attn.hip) and the step planner (stepplan.h: "the row kernel fits") both ask here.
static inline int attn_row_lds_bytes(int G, bool pk, int pages_bound) {
    const int nch = (pages_bound + ATT_PB - 1) / ATT_PB;
    return G * 256 + 512 + (pk ? ROW_WAVES * G * 256 : 0) + ROW_WAVES * G * 128 + G * pages_bound * (8 + 128) + PV_WAVES * nch * G * 512;
}
