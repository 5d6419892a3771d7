// The sizes and the row descriptor that the HIP-free host headers (kvpool.h, staging.h) share with the kernels.
// No HIP in here: common.h includes it for the device side.
#pragma once
#include <stdint.h>

#define MTTS_MAXR 32          // rows per MFMA N-tile (one activation fragment tile)
#define MTTS_RCAP 128         // dialogue slots; rows of a decode pass (up to 4 activation tiles share one weight stream)
#define MTTS_PFCAP 2048       // rows of a prefill pass (tiled GEMM); also the row stride of the split-K slabs
#define MTTS_PAGE 64          // tokens per KV page

// Per-row metadata of one forward pass.
struct RowMeta {
    int32_t seq;     // sequence slot (page-table row), -1 = inactive row
    int32_t pos;     // position of this token = its index among the sequence's real tokens
    int32_t last;    // 1 if logits are wanted for this row
    int32_t pad;
};
