// Per-kernel entry points of libmtts.so for the unit tests, and the measurement / debug hooks of bench.py and the tools
// (mtts_k_*, mtts_debug_*: include/mtts.h).  None of them is on the product path.  A hook's device buffers live in a
// DevBufs of its own: freed on every return path.
#include "engine.h"
#include "staging.h"        // stage_ban_static (mtts_k_ngram_ban)

int32_t mtts_k_gemm_bf16(const void* w, const void* x, void* y, int32_t M, int32_t N, int32_t K, int32_t ksplit, void* stream) {
    if (!w || !x || !y || M < 1 || M > MTTS_PFCAP || K % 16 || N < 1) return fail(MTTS_EINVAL, "gemm: need 1<=M<=MTTS_PFCAP, K%%16==0");
    hipStream_t st = S(stream);
    int Npad = round_up(N, 32);
    void *wp = nullptr, *xp = nullptr;
    float* part = nullptr;
    GemmPlan p = mtts_plan_gemm(Npad, K, ksplit);
    p.depth = gemm_depth_env();
    DevBufs hb;
    TRY(hb.get((uint16_t**)&wp, (size_t)Npad * K));
    // M <= 128: skinny kernel (decode); above: tiled kernel (prefill), ksplit as given or its own choice
    const bool tiled = M > MTTS_RCAP;
    const int ks = tiled ? (ksplit > 0 ? ksplit : mtts_tile_ksplit(Npad, K, M)) : p.ksplit;
    TRY(hb.get((uint16_t**)&xp, (size_t)MTTS_PFCAP * K));
    TRY(hb.get(&part, (size_t)ks * MTTS_PFCAP * Npad));
    launch_pack_weight(w, wp, N, K, Npad, 1, 0, st);
    const int tiles = (M + 31) / 32;
    launch_pack_rows(x, xp, M, K, tiles == 3 ? 4 : tiles, st);
    if (tiled) launch_gemm_tile(EPI_PARTIAL, M, ks, wp, xp, K, Npad, Npad, part, nullptr, st);
    else launch_gemm(EPI_PARTIAL, tiles, p, wp, xp, K, Npad, Npad, part, nullptr, st);
    launch_reduce_partial_bf16(part, y, ks, Npad, N, M, st);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(st));
    return MTTS_OK;
}

int64_t mtts_debug_gemm_depth_launches(void) { return (int64_t)mtts_gemm_depth_launches(); }
int32_t mtts_k_gemm_swiglu_bf16(const void* w, const void* x, void* y, int32_t M, int32_t N, int32_t K, void* stream) {
    if (!w || !x || !y || M < 1 || M > MTTS_RCAP || K % 16 || N < 32 || N % 32) return fail(MTTS_EINVAL, "gemm_swiglu: need 1<=M<=128, K%%16==0, N%%32==0");
    hipStream_t st = S(stream);
    void *wp = nullptr, *xp = nullptr, *op = nullptr;
    GemmPlan p = mtts_plan_gemm(N, K, 1);          // as the engine plans gate/up: no split-K
    p.depth = gemm_depth_env();
    DevBufs hb;
    const int tiles = (M + 31) / 32, tp = tiles == 3 ? 4 : tiles;
    TRY(hb.get((uint16_t**)&wp, (size_t)N * K));
    TRY(hb.get((uint16_t**)&xp, (size_t)tp * 32 * K));
    TRY(hb.get((uint16_t**)&op, (size_t)tp * 32 * (N / 2)));
    launch_pack_weight(w, wp, N, K, N, 1, 0, st);
    launch_pack_rows(x, xp, M, K, tp, st);
    launch_gemm(EPI_SILU, tiles, p, wp, xp, K, N, N, nullptr, (uint16_t*)op, st);
    launch_unpack_rows(op, y, M, N / 2, st);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(st));
    return MTTS_OK;
}

// The scoring kernels (score.hip) on a row-major head and activation: packed with the engine's pack launchers (heads of
// n_valid rows at multiples of round_up(n_valid, 32), like heads17), then head_ce_kernel + ce_finish_kernel.
int32_t mtts_k_head_ce(const void* w, const void* x, const int32_t* host_labels, int32_t M, int32_t N, int32_t K, int32_t n_valid,
                       int32_t segments, float* dev_logp, void* stream) {
    if (!w || !x || !host_labels || !dev_logp || M < 1 || M > MTTS_PFCAP || K < 16 || K % 16 || n_valid < 1 || segments < 1 ||
        (segments == 1 ? n_valid > N : N != segments * n_valid))
        return fail(MTTS_EINVAL, "head_ce: need 1<=M<=MTTS_PFCAP, K%%16==0, n_valid<=N (one head) or N==segments*n_valid");
    for (int i = 0; i < M * segments; ++i)
        if (host_labels[i] >= n_valid) return fail(MTTS_EINVAL, "head_ce: label %d outside [0, %d)", host_labels[i], n_valid);
    hipStream_t st = S(stream);
    const int seg_pad = round_up(segments == 1 ? N : n_valid, 32), Mpad = round_up(M, 32);
    uint16_t *wp = nullptr, *xp = nullptr;
    int32_t* lab = nullptr;
    float* part = nullptr;
    DevBufs hb;
    TRY(hb.get(&wp, (size_t)segments * seg_pad * K));
    TRY(hb.get(&xp, (size_t)Mpad * K));
    TRY(hb.get(&lab, (size_t)Mpad * segments, false));
    TRY(hb.get(&part, head_ce_part_elems(M, n_valid, segments), false));
    std::vector<int32_t> hl((size_t)Mpad * segments, -100);
    std::copy(host_labels, host_labels + (size_t)M * segments, hl.begin());
    HIPCHK(hipMemcpyAsync(lab, hl.data(), hl.size() * 4, hipMemcpyHostToDevice, st));
    if (segments == 1) launch_pack_weight(w, wp, N, K, seg_pad, 1, 0, st);
    else
        for (int s = 0; s < segments; ++s)
            launch_pack_weight((const uint16_t*)w + (size_t)s * n_valid * K, wp, n_valid, K, segments * seg_pad, 1, s * seg_pad, st);
    launch_pack_rows(x, xp, M, K, Mpad / 32, st);
    launch_head_ce(wp, xp, M, K, n_valid, segments, lab, segments, 0, part, dev_logp, segments, 0, st);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(st));
    return MTTS_OK;
}

// The same packing, then head_topk_kernel + topk_finish_kernel through the engine's launcher (no labels: every one -100).
int32_t mtts_k_head_topk(const void* w, const void* x, int32_t M, int32_t N, int32_t K, int32_t n_valid, int32_t segments, int32_t k,
                         int32_t* dev_ids, float* dev_logp, void* stream) {
    if (!w || !x || !dev_ids || !dev_logp || M < 1 || M > MTTS_PFCAP || K < 16 || K % 16 || n_valid < 1 || segments < 1 ||
        (segments == 1 ? n_valid > N : N != segments * n_valid))
        return fail(MTTS_EINVAL, "head_topk: need 1<=M<=MTTS_PFCAP, K%%16==0, n_valid<=N (one head) or N==segments*n_valid");
    if (k < 1 || k > MTTS_SCORE_MAX_TOPK || k > n_valid)
        return fail(MTTS_EINVAL, "head_topk: k %d outside 1..min(%d, n_valid %d)", k, MTTS_SCORE_MAX_TOPK, n_valid);
    hipStream_t st = S(stream);
    const int seg_pad = round_up(segments == 1 ? N : n_valid, 32), Mpad = round_up(M, 32);
    uint16_t *wp = nullptr, *xp = nullptr;
    int32_t* lab = nullptr;
    float* part = nullptr;
    uint32_t* cand = nullptr;
    DevBufs hb;
    TRY(hb.get(&wp, (size_t)segments * seg_pad * K));
    TRY(hb.get(&xp, (size_t)Mpad * K));
    TRY(hb.get(&lab, (size_t)Mpad * segments, false));
    TRY(hb.get(&part, head_ce_part_elems(M, n_valid, segments), false));
    TRY(hb.get(&cand, head_topk_cand_elems(M, n_valid, segments, k), false));
    HIPCHK(hipMemsetAsync(lab, 0xff, (size_t)Mpad * segments * 4, st));                    // -1: no label
    if (segments == 1) launch_pack_weight(w, wp, N, K, seg_pad, 1, 0, st);
    else
        for (int s = 0; s < segments; ++s)
            launch_pack_weight((const uint16_t*)w + (size_t)s * n_valid * K, wp, n_valid, K, segments * seg_pad, 1, s * seg_pad, st);
    launch_pack_rows(x, xp, M, K, Mpad / 32, st);
    launch_head_topk(wp, xp, M, K, n_valid, segments, lab, segments, 0, part, nullptr, segments, 0, k, cand, dev_ids, dev_logp, st);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(st));
    return MTTS_OK;
}

int32_t mtts_k_lora_pack(const void* base, int32_t rows, int32_t cols, const float* lora_a, const float* lora_b, int32_t r, float scaling,
                         int32_t rows_pad, int32_t row_mul, int32_t row_off, int32_t dtype, void* out, void* stream) {
    if (!base || !lora_a || !lora_b || !out || rows < 1 || cols < 16 || cols % 16 || r < 1 || r > 256 || dtype < 0 || dtype > 2)
        return fail(MTTS_EINVAL, "lora_pack: need rows >= 1, cols %% 16 == 0, 1 <= r <= 256, dtype 0..2");
    if (((uintptr_t)base | (uintptr_t)lora_a | (uintptr_t)lora_b | (uintptr_t)out) & 15) return fail(MTTS_EINVAL, "lora_pack: pointers must be 16-byte aligned");
    if (dtype == 0 && (rows_pad < 32 || rows_pad % 32 || row_mul < 1 || row_off < 0 || (int64_t)(rows - 1) * row_mul + row_off >= rows_pad))
        return fail(MTTS_EINVAL, "lora_pack: rows_pad %% 32 == 0 and (rows - 1) * row_mul + row_off < rows_pad");
    hipStream_t st = S(stream);
    if (dtype == 0) launch_lora_pack(base, lora_a, lora_b, r, scaling, out, rows, cols, row_mul, row_off, st);
    else launch_lora_rows_f32((const float*)base, lora_a, lora_b, r, scaling, (float*)out, rows, cols, dtype == 2, st);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(st));
    return MTTS_OK;
}

int32_t mtts_k_lora_delta(const void* dev_x, int32_t R, int32_t K, int32_t Npad, int32_t nseg, const int32_t* host_segs,
                          int32_t n_adapters, const void* const* host_a, const void* const* host_b, const int32_t* host_r,
                          const float* host_scaling, const int32_t* host_row_adapter, float* dev_slabs, int32_t ks, void* stream) {
    if (!dev_x || !host_segs || !host_a || !host_b || !host_r || !host_scaling || !host_row_adapter || !dev_slabs)
        return fail(MTTS_EINVAL, "lora_delta: null argument");
    if (R < 1 || R > MTTS_PFCAP || K < 16 || K % 16 || K > LORA_MAX_K || Npad < 32 || Npad % 32 || nseg < 1 || nseg > LORA_SEGS ||
        n_adapters < 1 || n_adapters > MTTS_MAX_ADAPTERS || ks < 0)
        return fail(MTTS_EINVAL, "lora_delta: need 1<=R<=%d, K%%16==0, K<=%d, Npad%%32==0, 1<=nseg<=%d, 1<=n_adapters<=%d", MTTS_PFCAP,
                    LORA_MAX_K, LORA_SEGS, MTTS_MAX_ADAPTERS);
    LoraJob job{};
    job.nseg = nseg; job.Npad = Npad; job.K = K; job.ent_stride = nseg;
    for (int s = 0; s < nseg; ++s) {
        const int32_t* g = host_segs + 3 * s;
        if (g[0] < 0 || g[1] < 1 || g[2] < 1 || (int64_t)g[0] + (int64_t)(g[1] - 1) * g[2] >= Npad)
            return fail(MTTS_EINVAL, "lora_delta: matrix %d (col0 %d, ncols %d, mul %d) does not fit %d columns", s, g[0], g[1], g[2], Npad);
        job.seg[s] = LoraSeg{g[0], g[1], g[2], s};
    }
    std::vector<LoraEnt> ents((size_t)n_adapters * nseg);
    for (size_t i = 0; i < ents.size(); ++i) {
        if (host_r[i] < 0 || host_r[i] > MTTS_LORA_MAX_RANK || (host_r[i] && (!host_a[i] || !host_b[i])))
            return fail(MTTS_EINVAL, "lora_delta: entry %zu: rank %d outside 0..%d, or a null matrix", i, host_r[i], MTTS_LORA_MAX_RANK);
        if (((uintptr_t)host_a[i] | (uintptr_t)host_b[i]) & 15) return fail(MTTS_EINVAL, "lora_delta: matrices must be 16-byte aligned");
        ents[i] = LoraEnt{(const float*)host_a[i], (const float*)host_b[i], host_r[i], host_scaling[i]};
    }
    std::vector<RowMeta> metas(R);
    std::vector<int32_t> sa(R);
    for (int r = 0; r < R; ++r) {
        const int a = host_row_adapter[r];
        if (a < -2 || a >= n_adapters) return fail(MTTS_EINVAL, "lora_delta: row %d names adapter %d of %d", r, a, n_adapters);
        metas[r] = RowMeta{a == -2 ? -1 : r, 0, 0, 0};
        sa[r] = a < 0 ? -1 : a;
    }
    hipStream_t st = S(stream);
    DevBufs hb;
    uint16_t* xp = nullptr;
    LoraEnt* d_ents = nullptr;
    RowMeta* d_meta = nullptr;
    int32_t* d_sa = nullptr;
    const int tiles = (R + 31) / 32;
    TRY(hb.get(&xp, (size_t)tiles * 32 * K));
    TRY(hb.get(&d_ents, ents.size(), false));
    TRY(hb.get(&d_meta, (size_t)R, false));
    TRY(hb.get(&d_sa, (size_t)R, false));
    HIPCHK(hipMemcpyAsync(d_ents, ents.data(), ents.size() * sizeof(LoraEnt), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_meta, metas.data(), metas.size() * sizeof(RowMeta), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_sa, sa.data(), sa.size() * 4, hipMemcpyHostToDevice, st));
    launch_pack_rows(dev_x, xp, R, K, tiles, st);
    launch_lora_delta(xp, d_meta, d_sa, d_ents, job, dev_slabs + (size_t)ks * MTTS_PFCAP * Npad, R, st);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(st));
    return MTTS_OK;
}

int32_t mtts_k_swiglu_slabs(const void* w, const void* x, const float* dev_delta, void* y, float* dev_slab0_out, int32_t M, int32_t N,
                            int32_t K, void* stream) {
    if (!w || !x || !y || M < 1 || M > MTTS_RCAP || K % 16 || N < 32 || N % 32) return fail(MTTS_EINVAL, "swiglu_slabs: need 1<=M<=128, K%%16==0, N%%32==0");
    hipStream_t st = S(stream);
    void *wp = nullptr, *xp = nullptr, *op = nullptr;
    float* part = nullptr;
    GemmPlan p = mtts_plan_gemm(N, K, 1);          // as the engine plans gate/up: no split-K
    p.depth = gemm_depth_env();
    DevBufs hb;
    const int tiles = (M + 31) / 32, tp = tiles == 3 ? 4 : tiles;
    TRY(hb.get((uint16_t**)&wp, (size_t)N * K));
    TRY(hb.get((uint16_t**)&xp, (size_t)tp * 32 * K));
    TRY(hb.get((uint16_t**)&op, (size_t)tp * 32 * (N / 2)));
    TRY(hb.get(&part, (size_t)2 * MTTS_PFCAP * N));
    float* slab1 = part + (size_t)MTTS_PFCAP * N;
    launch_pack_weight(w, wp, N, K, N, 1, 0, st);
    launch_pack_rows(x, xp, M, K, tp, st);
    launch_gemm(EPI_PARTIAL, tiles, p, wp, xp, K, N, N, part, nullptr, st);
    if (dev_delta) HIPCHK(hipMemcpyAsync(slab1, dev_delta, (size_t)M * N * 4, hipMemcpyDeviceToDevice, st));
    launch_swiglu_slabs(part, slab1, op, tiles * 32, N / 2, st);
    launch_unpack_rows(op, y, M, N / 2, st);
    if (dev_slab0_out) HIPCHK(hipMemcpyAsync(dev_slab0_out, part, (size_t)M * N * 4, hipMemcpyDeviceToDevice, st));
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(st));
    return MTTS_OK;
}

int32_t mtts_k_rmsnorm(const void* x, const void* w, void* y, int32_t rows, int32_t n, float eps, void* stream) {
    if (!x || !w || !y || rows < 1 || n < 1) return fail(MTTS_EINVAL, "rmsnorm: bad argument");
    launch_rmsnorm_rows(x, w, y, rows, n, eps, S(stream));
    HIPCHK(hipGetLastError());
    return MTTS_OK;
}

// ---- the layer kernels the engine launches, one launch each (tests/test_layer_kernels_gpu.py) -------------------------
// Every launch goes through the launcher the engine calls (launch.h); a shape a kernel does not take is refused.

// split-K slabs [ksplit][R][Npad] of a caller -> a buffer with the kernels' slab stride (MTTS_PFCAP rows)
static int stage_slabs(DevBufs& hb, const float* dev_slabs, int ksplit, int R, int Npad, float** out, hipStream_t st) {
    TRY(hb.get(out, (size_t)ksplit * MTTS_PFCAP * Npad, false));
    for (int k = 0; k < ksplit; ++k)
        HIPCHK(hipMemcpyAsync(*out + (size_t)k * MTTS_PFCAP * Npad, dev_slabs + (size_t)k * R * Npad, (size_t)R * Npad * 4, hipMemcpyDeviceToDevice, st));
    return 0;
}

int32_t mtts_k_embed_norm(const int32_t* host_tokens, const int32_t* host_seq, const void* const* host_tables,
                          const int32_t* host_vocab, const void* dev_norm_w, int32_t R, int32_t H, float eps,
                          void* dev_x, void* dev_xn, void* stream) {
    if (!host_tokens || !host_seq || !host_tables || !host_vocab || !dev_norm_w || !dev_x || !dev_xn || R < 1 || R > MTTS_PFCAP ||
        H < 16 || H % 16 || H > 8192)
        return fail(MTTS_EINVAL, "embed_norm: need 1<=R<=MTTS_PFCAP, H%%16==0, H<=8192");
    for (int c = 0; c < 8; ++c)
        if (!host_tables[c] || host_vocab[c] < 1) return fail(MTTS_EINVAL, "embed_norm: table %d missing or empty", c);
    for (int r = 0; r < R; ++r)
        for (int c = 0; c < 8; ++c)
            if (host_seq[r] >= 0 && (host_tokens[r * 8 + c] < 0 || host_tokens[r * 8 + c] >= host_vocab[c]))
                return fail(MTTS_EINVAL, "embed_norm: row %d channel %d: token %d outside [0, %d)", r, c, host_tokens[r * 8 + c], host_vocab[c]);
    hipStream_t st = S(stream);
    int32_t* tok = nullptr; RowMeta* meta = nullptr; const uint16_t** tabs = nullptr; uint16_t* xnp = nullptr;
    DevBufs hb;
    TRY(hb.get(&tok, (size_t)R * 8)); TRY(hb.get(&meta, R)); TRY(hb.get(&tabs, 8));
    TRY(hb.get(&xnp, (size_t)round_up(R, 32) * H));
    std::vector<RowMeta> hm(R);
    for (int r = 0; r < R; ++r) hm[r] = RowMeta{host_seq[r] < 0 ? -1 : host_seq[r], 0, 0, 0};
    HIPCHK(hipMemcpyAsync(tok, host_tokens, (size_t)R * 8 * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(meta, hm.data(), R * sizeof(RowMeta), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(tabs, host_tables, 8 * sizeof(void*), hipMemcpyHostToDevice, st));
    launch_embed_norm(tok, meta, tabs, dev_norm_w, dev_x, xnp, R, H, eps, st);
    launch_unpack_rows(xnp, dev_xn, R, H, st);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(st));
    return MTTS_OK;
}

int32_t mtts_k_resid_norm(const float* dev_slabs, int32_t ksplit, int32_t Npad, void* dev_x, const void* dev_norm_w,
                          const int32_t* host_seq, const int32_t* host_last, int32_t R, int32_t H, int32_t nseq, float eps,
                          void* dev_xn, void* dev_hlast, void* stream) {
    if (!dev_slabs || !dev_x || !dev_norm_w || !host_seq || !host_last || !dev_xn || !dev_hlast || R < 1 || R > MTTS_PFCAP || H < 16 ||
        H % 16 || H > 8192 || Npad != round_up(H, 32) || ksplit < 1 || ksplit > 16 || nseq < 1)
        return fail(MTTS_EINVAL, "resid_norm: need 1<=R<=MTTS_PFCAP, H%%16==0, H<=8192, Npad==round_up(H,32), 1<=ksplit<=16");
    for (int r = 0; r < R; ++r)
        if (host_seq[r] >= nseq) return fail(MTTS_EINVAL, "resid_norm: row %d: sequence %d outside [0, %d)", r, host_seq[r], nseq);
    hipStream_t st = S(stream);
    float* slabs = nullptr; RowMeta* meta = nullptr; uint16_t* xnp = nullptr;
    DevBufs hb;
    TRY(stage_slabs(hb, dev_slabs, ksplit, R, Npad, &slabs, st));
    TRY(hb.get(&meta, R));
    TRY(hb.get(&xnp, (size_t)round_up(R, 32) * H));
    std::vector<RowMeta> hm(R);
    for (int r = 0; r < R; ++r) hm[r] = RowMeta{host_seq[r] < 0 ? -1 : host_seq[r], 0, host_last[r] ? 1 : 0, 0};
    HIPCHK(hipMemcpyAsync(meta, hm.data(), R * sizeof(RowMeta), hipMemcpyHostToDevice, st));
    launch_resid_norm(slabs, ksplit, Npad, dev_x, dev_norm_w, xnp, dev_hlast, meta, R, H, eps, st);
    launch_unpack_rows(xnp, dev_xn, R, H, st);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(st));
    return MTTS_OK;
}

int32_t mtts_k_gemv_small(int32_t epi, int32_t pro, const void* dev_w, int32_t rows, int32_t N, int32_t K, int32_t want_ksplit,
                          const void* dev_x_in, const float* dev_slabs, int32_t slab_ksplit, const void* dev_norm_w, float eps,
                          void* dev_x_out, const float* dev_opart, const int32_t* host_seq, const int32_t* host_pos, int32_t nq,
                          int32_t nchunks_max, const void* dev_xrows, void* dev_y, int32_t* out_plan, void* stream) {
    const bool pair = (epi == EPI_PARTIAL && (pro == PRO_NORM || pro == PRO_COMBINE || pro == PRO_ROWS)) ||
                      ((epi == EPI_SILU_RM || epi == EPI_BF16) && pro == PRO_NORM);
    if (!pair) return fail(MTTS_EINVAL, "gemv_small: (epi %d, pro %d) is not a pair the decode step uses", epi, pro);
    if (!dev_w || !dev_y || rows < 1 || rows > SMALL_RP || N < 1 || K < 16 || K % 16)
        return fail(MTTS_EINVAL, "gemv_small: need 1<=rows<=%d, N>=1, K%%16==0", SMALL_RP);
    if (epi == EPI_SILU_RM && N % 32) return fail(MTTS_EINVAL, "gemv_small: the SwiGLU epilogue needs N%%32==0");
    if (epi != EPI_PARTIAL && want_ksplit != 1) return fail(MTTS_EINVAL, "gemv_small: only the fp32 slab epilogue takes a split-K");
    if (want_ksplit < 0 || want_ksplit > 16 || want_ksplit > K / 16) return fail(MTTS_EINVAL, "gemv_small: split-K %d outside 0..min(16, K/16)", want_ksplit);
    const int Npad = round_up(N, 32), Kp = round_up(K, 32);
    if (pro == PRO_NORM) {
        if (!dev_x_in || !dev_norm_w || dev_x_in == dev_x_out || slab_ksplit < 0 || slab_ksplit > 16 || (slab_ksplit && !dev_slabs))
            return fail(MTTS_EINVAL, "gemv_small: norm prologue needs x_in != x_out, norm_w, 0<=slab_ksplit<=16 slabs");
    } else if (pro == PRO_COMBINE) {
        if (!dev_opart || !host_seq || !host_pos || nq < 1 || K != nq * MTTS_HD || nchunks_max < 1)
            return fail(MTTS_EINVAL, "gemv_small: combine prologue needs opart, seq, pos, K==nq*128, nchunks_max>=1");
        for (int r = 0; r < rows; ++r) {
            if (host_seq[r] < 0) continue;
            const int npages = host_pos[r] < 0 ? -1 : host_pos[r] / MTTS_PAGE + 1;
            if (npages < 0 || (npages + ATT_PB - 1) / ATT_PB > nchunks_max)
                return fail(MTTS_EINVAL, "gemv_small: row %d: position %d needs more than %d chunks", r, host_pos[r], nchunks_max);
        }
    } else if (!dev_xrows) return fail(MTTS_EINVAL, "gemv_small: rows prologue needs xrows");
    const GemmPlan p0 = mtts_plan_gemm(Npad, K, want_ksplit);
    if (mtts_small_lds_bytes(p0, K, pro) > 64 * 1024 - 33 * 1024)                     // the budget of the engine's small_path_fits
        return fail(MTTS_EINVAL, "gemv_small: the prologue's %d bytes of LDS exceed the small path's budget", mtts_small_lds_bytes(p0, K, pro));
    hipStream_t st = S(stream);
    uint16_t* wp = nullptr; float *part = nullptr, *slabs = nullptr; RowMeta* meta = nullptr;
    DevBufs hb;
    TRY(hb.get(&wp, (size_t)Npad * K));
    launch_pack_weight(dev_w, wp, N, K, Npad, 1, 0, st);
    SmallPro pr{};
    pr.rows = rows; pr.eps = eps;
    if (pro == PRO_NORM) {
        if (slab_ksplit) TRY(stage_slabs(hb, dev_slabs, slab_ksplit, rows, Kp, &slabs, st));
        pr.x_in = (const uint16_t*)dev_x_in; pr.x_out = (uint16_t*)dev_x_out; pr.slabs = slabs; pr.ksplit = slab_ksplit; pr.slab_npad = Kp;
        pr.norm_w = (const uint16_t*)dev_norm_w;
    } else if (pro == PRO_COMBINE) {
        TRY(hb.get(&meta, SMALL_RP));
        std::vector<RowMeta> hm(SMALL_RP, RowMeta{-1, 0, 0, 0});
        for (int r = 0; r < rows; ++r)
            if (host_seq[r] >= 0) hm[r] = RowMeta{host_seq[r], host_pos[r], 1, 0};
        HIPCHK(hipMemcpyAsync(meta, hm.data(), hm.size() * sizeof(RowMeta), hipMemcpyHostToDevice, st));
        pr.opart = dev_opart; pr.meta = meta; pr.nchunks_max = nchunks_max; pr.nq = nq; pr.pages_per_chunk = ATT_PB;
    } else pr.xrows = (const uint16_t*)dev_xrows;
    if (epi == EPI_PARTIAL) {
        // the slabs start as NaN: an element of a live row that the kernel leaves out shows in the reduced output
        TRY(hb.get(&part, (size_t)p0.ksplit * MTTS_PFCAP * Npad, false));
        for (int k = 0; k < p0.ksplit; ++k) HIPCHK(hipMemsetAsync(part + (size_t)k * MTTS_PFCAP * Npad, 0xff, (size_t)SMALL_RP * Npad * 4, st));
    }
    launch_gemv_small(epi, pro, p0, wp, K, Npad, N, part, epi == EPI_PARTIAL ? nullptr : (uint16_t*)dev_y, pr, st);
    if (epi == EPI_PARTIAL) launch_reduce_partial_bf16(part, dev_y, p0.ksplit, Npad, N, rows, st);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(st));
    if (out_plan) { out_plan[0] = std::max(p0.waves, 4); out_plan[1] = p0.ksplit; }
    return MTTS_OK;
}

int32_t mtts_k_gemm_tile(int32_t epi, const void* dev_w, const void* dev_x, void* dev_y, int32_t M, int32_t N, int32_t K,
                         int32_t ksplit, void* stream) {
    if ((epi != EPI_PARTIAL && epi != EPI_SILU) || !dev_w || !dev_x || !dev_y || M < 1 || M > MTTS_PFCAP || N < 1 || K < 16 || K % 16)
        return fail(MTTS_EINVAL, "gemm_tile: need epi 0 or 2, 1<=M<=MTTS_PFCAP, N>=1, K%%16==0");
    if (epi == EPI_SILU && (N % 32 || ksplit < 0 || ksplit > 1)) return fail(MTTS_EINVAL, "gemm_tile: the SwiGLU epilogue needs N%%32==0 and no split-K");
    if (ksplit < 0 || ksplit > 16 || ksplit > K / 16) return fail(MTTS_EINVAL, "gemm_tile: split-K %d outside 0..min(16, K/16)", ksplit);
    hipStream_t st = S(stream);
    const int Npad = round_up(N, 32), tiles = (M + 31) / 32;
    const int ks = epi == EPI_SILU ? 1 : (ksplit > 0 ? ksplit : mtts_tile_ksplit(Npad, K, M));
    uint16_t *wp = nullptr, *xp = nullptr, *op = nullptr;
    float* part = nullptr;
    DevBufs hb;
    TRY(hb.get(&wp, (size_t)Npad * K));
    TRY(hb.get(&xp, (size_t)tiles * 32 * K));
    launch_pack_weight(dev_w, wp, N, K, Npad, 1, 0, st);
    launch_pack_rows(dev_x, xp, M, K, tiles, st);
    if (epi == EPI_PARTIAL) {
        TRY(hb.get(&part, (size_t)ks * MTTS_PFCAP * Npad));
        launch_gemm_tile(EPI_PARTIAL, M, ks, wp, xp, K, Npad, Npad, part, nullptr, st);
        launch_reduce_partial_bf16(part, dev_y, ks, Npad, N, M, st);
    } else {
        TRY(hb.get(&op, (size_t)tiles * 32 * (N / 2)));
        launch_gemm_tile(EPI_SILU, M, 1, wp, xp, K, N, N, nullptr, op, st);
        launch_unpack_rows(op, dev_y, M, N / 2, st);
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(st));
    return MTTS_OK;
}

static int k_sample(const void* logits, int32_t rows, int32_t vocab, const void* bitmap, const MttsSamplerCfg* cfg,
                    int32_t mask_id, uint64_t seed, int32_t step, int32_t channel, int32_t* dev_tokens, float* dev_logp,
                    const MttsSamplerFloors* floors, const void* ban, float typical_p, void* stream, const void* bias_w = nullptr,
                    const MttsBiasTable* bias_t = nullptr) {
    if ((bias_w == nullptr) != (bias_t == nullptr)) return fail(MTTS_EINVAL, "sample: bias words and bias tables come together");
    if (!logits || !cfg || !dev_tokens || rows < 1 || vocab < 1 || channel < 0 || channel > 7) return fail(MTTS_EINVAL, "sample: bad argument");
    hipStream_t st = S(stream);
    MttsSamplerCfg h[8];
    for (int i = 0; i < 8; ++i) h[i] = *cfg;
    MttsSamplerCfg* d = nullptr;
    int32_t *err = nullptr, *dec = nullptr;
    if (rows > MTTS_RCAP) return fail(MTTS_EINVAL, "sample: at most 128 rows");
    DevBufs hb;
    TRY(hb.get(&d, 8));
    TRY(hb.get(&err, 1));
    TRY(hb.get(&dec, (size_t)rows * 8));
    HIPCHK(hipMemcpy(d, h, sizeof(h), hipMemcpyHostToDevice));
    // floors: checked like mtts_set_sampler_floors checks them; none, all zero or a greedy cfg: the kernels without floors
    MttsSamplerFloors* dfl = nullptr;
    if (floors) {
        MttsSamplerFloors hf[8];
        for (int i = 0; i < 8; ++i) hf[i] = *floors;
        PendingRun chk;
        TRY(chk.set_floors(hf));
        if (cfg->do_sample && (floors->min_p > 0.f || floors->epsilon_cutoff > 0.f || floors->eta_cutoff > 0.f)) {
            TRY(hb.get(&dfl, 8));
            HIPCHK(hipMemcpy(dfl, hf, sizeof(hf), hipMemcpyHostToDevice));
        }
    }
    // typical_p: checked like mtts_set_sampler_typical checks it; 0, 1 or a greedy cfg: the kernels without it
    float* dty = nullptr;
    {
        float ht[8];
        for (int i = 0; i < 8; ++i) ht[i] = typical_p;
        PendingRun chk;
        TRY(chk.set_typical(ht));
        if (cfg->do_sample && typical_p > 0.f && typical_p < 1.f) {
            TRY(hb.get(&dty, 8));
            HIPCHK(hipMemcpy(dty, ht, sizeof(ht), hipMemcpyHostToDevice));
        }
    }
    SampleScratch sc;
    TRY(alloc_scratch(hb, sc, rows, vocab));
    sc.ban = (const uint32_t*)ban;   // [rows][ceil(vocab / 32)], or null: the same kernels, which then read no ban word
    sc.bias_w = (const uint32_t*)bias_w; sc.bias_t = bias_t;    // the same for the additive terms: [rows][ceil(vocab / 32)], [rows]
    if (dev_logp) {                  // output_scores scratch
        TRY(hb.get(&sc.slice_sum, (size_t)rows * SAMP_NS));
        TRY(hb.get(&sc.lp, (size_t)rows * 8));
    }
    launch_sample_single(logits, rows, vocab, (const uint32_t*)bitmap, (vocab + 31) / 32, d, mask_id, seed, step, channel, dec, err, sc,
                         full_cap_for(vocab), dev_logp ? 1 : 0, dfl, dty, st);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(st));
    std::vector<int32_t> hd((size_t)rows * 8);
    int32_t herr = 0;
    HIPCHK(hipMemcpy(hd.data(), dec, hd.size() * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(&herr, err, 4, hipMemcpyDeviceToHost));
    std::vector<int32_t> outv(rows);
    for (int r = 0; r < rows; ++r) outv[r] = hd[(size_t)r * 8 + channel];
    HIPCHK(hipMemcpy(dev_tokens, outv.data(), rows * 4, hipMemcpyHostToDevice));
    if (dev_logp) {
        std::vector<float> hl((size_t)rows * 8), outl(rows);
        HIPCHK(hipMemcpy(hl.data(), sc.lp, hl.size() * 4, hipMemcpyDeviceToHost));
        for (int r = 0; r < rows; ++r) outl[r] = hl[(size_t)r * 8 + channel];
        HIPCHK(hipMemcpy(dev_logp, outl.data(), rows * 4, hipMemcpyHostToDevice));
    }
    if (herr) return fail(MTTS_EINVAL, "sample: more than 4096 candidate tokens");
    return MTTS_OK;
}

int32_t mtts_k_sample(const void* logits, int32_t rows, int32_t vocab, const void* bitmap, const MttsSamplerCfg* cfg,
                      int32_t mask_id, uint64_t seed, int32_t step, int32_t channel, int32_t* dev_tokens, void* stream) {
    return k_sample(logits, rows, vocab, bitmap, cfg, mask_id, seed, step, channel, dev_tokens, nullptr, nullptr, nullptr, 0.f, stream);
}

int32_t mtts_k_sample_scores(const void* logits, int32_t rows, int32_t vocab, const void* bitmap, const MttsSamplerCfg* cfg,
                             int32_t mask_id, uint64_t seed, int32_t step, int32_t channel, int32_t* dev_tokens, float* dev_logp,
                             void* stream) {
    if (!dev_logp) return fail(MTTS_EINVAL, "sample: null dev_logp");
    return k_sample(logits, rows, vocab, bitmap, cfg, mask_id, seed, step, channel, dev_tokens, dev_logp, nullptr, nullptr, 0.f, stream);
}

int32_t mtts_k_sample_floors(const void* logits, int32_t rows, int32_t vocab, const void* bitmap, const MttsSamplerCfg* cfg,
                             int32_t mask_id, uint64_t seed, int32_t step, int32_t channel, int32_t* dev_tokens, float* dev_logp,
                             const MttsSamplerFloors* floors, void* stream) {
    return k_sample(logits, rows, vocab, bitmap, cfg, mask_id, seed, step, channel, dev_tokens, dev_logp, floors, nullptr, 0.f, stream);
}

int32_t mtts_k_sample_bans(const void* logits, int32_t rows, int32_t vocab, const void* bitmap, const MttsSamplerCfg* cfg,
                           int32_t mask_id, uint64_t seed, int32_t step, int32_t channel, int32_t* dev_tokens, float* dev_logp,
                           const MttsSamplerFloors* floors, const void* dev_ban, void* stream) {
    return k_sample(logits, rows, vocab, bitmap, cfg, mask_id, seed, step, channel, dev_tokens, dev_logp, floors, dev_ban, 0.f, stream);
}

int32_t mtts_k_sample_typical(const void* logits, int32_t rows, int32_t vocab, const void* bitmap, const MttsSamplerCfg* cfg,
                              int32_t mask_id, uint64_t seed, int32_t step, int32_t channel, int32_t* dev_tokens, float* dev_logp,
                              const MttsSamplerFloors* floors, const void* dev_ban, float typical_p, void* stream) {
    return k_sample(logits, rows, vocab, bitmap, cfg, mask_id, seed, step, channel, dev_tokens, dev_logp, floors, dev_ban, typical_p, stream);
}

int32_t mtts_k_sample_bias(const void* logits, int32_t rows, int32_t vocab, const void* bitmap, const MttsSamplerCfg* cfg,
                           int32_t mask_id, uint64_t seed, int32_t step, int32_t channel, int32_t* dev_tokens, float* dev_logp,
                           const MttsSamplerFloors* floors, const void* dev_ban, float typical_p, const void* dev_bias_words,
                           const MttsBiasTable* dev_bias_tab, void* stream) {
    return k_sample(logits, rows, vocab, bitmap, cfg, mask_id, seed, step, channel, dev_tokens, dev_logp, floors, dev_ban, typical_p, stream,
                    dev_bias_words, dev_bias_tab);
}

// scores_materialize_kernel of the split step (sampler.hip) on one logits matrix.
int32_t mtts_k_scores_materialize(const void* logits, int32_t rows, int32_t vocab, const void* bitmap, const MttsSamplerCfg* cfg,
                                  int32_t mask_id, int32_t step, int32_t channel, const void* dev_ban, const void* dev_bias_words,
                                  const MttsBiasTable* dev_bias_tab, float* dev_scores, void* stream) {
    if (!logits || !cfg || !dev_scores || rows < 1 || rows > MTTS_RCAP || vocab < 1 || channel < 0 || channel > 7 || mask_id >= vocab)
        return fail(MTTS_EINVAL, "scores_materialize: bad argument");
    if ((dev_bias_words == nullptr) != (dev_bias_tab == nullptr)) return fail(MTTS_EINVAL, "scores_materialize: bias words and bias tables come together");
    if ((uintptr_t)dev_scores & 15) return fail(MTTS_EINVAL, "scores_materialize: dev_scores is not 16-byte aligned");
    hipStream_t st = S(stream);
    MttsSamplerCfg h[8];
    for (int i = 0; i < 8; ++i) h[i] = *cfg;
    DevBufs hb;
    MttsSamplerCfg* d = nullptr;
    TRY(hb.get(&d, 8));
    HIPCHK(hipMemcpy(d, h, sizeof(h), hipMemcpyHostToDevice));
    SampleScratch sc;
    sc.ban = (const uint32_t*)dev_ban;
    sc.bias_w = (const uint32_t*)dev_bias_words; sc.bias_t = dev_bias_tab;
    launch_scores_materialize_single(logits, rows, vocab, (const uint32_t*)bitmap, (vocab + 31) / 32, d, mask_id, step, channel, sc, dev_scores, st);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(st));
    return MTTS_OK;
}

// The ban kernel of a decode step (sampler.hip: ban_kernel) on bare histories of one channel.
int32_t mtts_k_ngram_ban(const int32_t* dev_hist, const int32_t* dev_lens, int32_t rows, int32_t cap, int32_t n,
                         const int32_t* host_static, int32_t n_static, int32_t vocab, int32_t eos_id, int32_t eos_on,
                         void* dev_ban, void* stream) {
    if (!dev_lens || !dev_ban || rows < 1 || rows > MTTS_RCAP || cap < 0 || (cap > 0 && !dev_hist) || vocab < 1 || n_static < 0 ||
        (n_static > 0 && !host_static))
        return fail(MTTS_EINVAL, "ngram_ban: bad argument");
    // the settings, checked like mtts_set_sampler_bans checks them
    MttsSamplerBans hbans[8];
    for (int i = 0; i < 8; ++i) hbans[i] = MttsSamplerBans{n, 0, n_static, host_static};
    PendingRun chk;
    TRY(chk.set_bans(hbans));
    hipStream_t st = S(stream);
    HIPCHK(hipStreamSynchronize(st));
    std::vector<int32_t> lens(rows);
    HIPCHK(hipMemcpy(lens.data(), dev_lens, (size_t)rows * 4, hipMemcpyDeviceToHost));
    for (int r = 0; r < rows; ++r)
        if (lens[r] < 0 || lens[r] > cap) return fail(MTTS_EINVAL, "ngram_ban: row %d has length %d, the histories hold %d", r, lens[r], cap);
    const int words = (vocab + 31) / 32;
    std::vector<uint32_t> stat(words);
    stage_ban_static(host_static, n_static, vocab, words, stat.data());
    const BanCfg hc{n, eos_on ? 1 : 0};
    DevBufs hb;
    BanCfg* dc = nullptr;
    uint32_t* ds = nullptr;
    TRY(hb.get(&dc, 1));
    TRY(hb.get(&ds, (size_t)words));
    HIPCHK(hipMemcpy(dc, &hc, sizeof(hc), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(ds, stat.data(), stat.size() * 4, hipMemcpyHostToDevice));
    launch_ban_single((uint32_t*)dev_ban, ds, dc, dev_hist, dev_lens, rows, cap, vocab, eos_id, st);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(st));
    return MTTS_OK;
}
int64_t mtts_debug_ban_launches(void) { return (int64_t)mtts_ban_launches(); }

// The rule kernel of a decode step (sampler.hip: bias_kernel) on bare histories of one channel.
int32_t mtts_k_seq_bias(const int32_t* dev_hist, const int32_t* dev_lens, int32_t rows, int32_t cap, const MttsSamplerBias* host_rules,
                        int32_t vocab, void* dev_ban, void* dev_bias_words, MttsBiasTable* dev_bias_tab, void* stream) {
    if (!dev_lens || !host_rules || rows < 1 || rows > MTTS_RCAP || cap < 0 || (cap > 0 && !dev_hist) || vocab < 1 ||
        (dev_bias_words == nullptr) != (dev_bias_tab == nullptr))
        return fail(MTTS_EINVAL, "seq_bias: bad argument");
    // the settings, checked like mtts_set_sampler_bias checks them
    MttsSamplerBias hb8[8];
    for (int i = 0; i < 8; ++i) hb8[i] = *host_rules;
    PendingRun chk;
    TRY(chk.set_bias(hb8));
    const RunBias rb = chk.take_bias();
    const ChannelBias& cb = rb.ch[0];
    bool ninf = false, fin = false;
    for (float v : cb.beta) { ninf = ninf || !(v > -INFINITY); fin = fin || v > -INFINITY; }
    if (ninf && !dev_ban) return fail(MTTS_EINVAL, "seq_bias: a -inf rule and no ban words");
    if (fin && !dev_bias_words) return fail(MTTS_EINVAL, "seq_bias: a finite rule and no bias words");
    hipStream_t st = S(stream);
    HIPCHK(hipStreamSynchronize(st));
    std::vector<int32_t> lens(rows);
    HIPCHK(hipMemcpy(lens.data(), dev_lens, (size_t)rows * 4, hipMemcpyDeviceToHost));
    for (int r = 0; r < rows; ++r)
        if (lens[r] < 0 || lens[r] > cap) return fail(MTTS_EINVAL, "seq_bias: row %d has length %d, the histories hold %d", r, lens[r], cap);
    const int words = (vocab + 31) / 32;
    BiasRules hr;
    std::vector<uint32_t> stat(words);
    stage_bias_rules(cb.len.data(), cb.ids.data(), cb.beta.data(), (int)cb.len.size(), vocab, words, &hr, stat.data());
    DevBufs hb;
    BiasRules* dr = nullptr;
    uint32_t* ds = nullptr;
    TRY(hb.get(&dr, 1));
    TRY(hb.get(&ds, (size_t)words));
    HIPCHK(hipMemcpy(dr, &hr, sizeof(hr), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(ds, stat.data(), stat.size() * 4, hipMemcpyHostToDevice));
    launch_bias_single((uint32_t*)dev_ban, (uint32_t*)dev_bias_words, ds, dev_bias_tab, dr, dev_hist, dev_lens, rows, cap, vocab, st);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(st));
    return MTTS_OK;
}
int64_t mtts_debug_bias_launches(void) { return (int64_t)mtts_bias_launches(); }

// The top_logprobs kernels of a decode step (gen_topk.hip) on bare logits, with a scratch of their own.
int32_t mtts_k_gen_topk(const void* dev_logits, int32_t is_f32, int32_t rows, int32_t vocab, int32_t mask_id,
                        const int32_t* dev_decisions, int32_t k, float* dev_logp, int32_t* dev_top_ids, float* dev_top_logp,
                        void* stream) {
    if (!dev_logits || !dev_decisions || !dev_logp || !dev_top_ids || !dev_top_logp) return fail(MTTS_EINVAL, "gen_topk: null argument");
    if (rows < 1 || rows > MTTS_RCAP || vocab < 1 || k < 1 || k > MTTS_SCORE_MAX_TOPK || k > vocab || mask_id >= vocab)
        return fail(MTTS_EINVAL, "gen_topk: rows 1..%d, 1 <= k <= min(%d, vocab), mask_id < vocab", MTTS_RCAP, MTTS_SCORE_MAX_TOPK);
    hipStream_t st = S(stream);
    DevBufs hb;
    GenTopkScratch sc;
    TRY(hb.get(&sc.cand, (size_t)rows * SAMP_NS * k));
    TRY(hb.get(&sc.smax, (size_t)rows * SAMP_NS));
    TRY(hb.get(&sc.ssum, (size_t)rows * SAMP_NS));
    sc.kcap = k;
    launch_gen_topk_single(dev_logits, is_f32 ? 1 : 0, rows, vocab, mask_id, dev_decisions, sc, GenTopkOut{k, dev_logp, dev_top_ids, dev_top_logp}, st);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(st));
    return MTTS_OK;
}

// ---- per-kernel entry points for attention and RoPE / cache write (unit tests) ----------------------------------------

// q/k/v epilogue of one token per row (qkv_post_kernel): dev_qkv bf16 [R][(nq+2*nkv)*128] = the three Linears' outputs,
// host_pos int32 [R] positions, dev_qnorm / dev_knorm bf16 [128], dev_cos / dev_sin bf16 [rope_rows][64].
// Outputs bf16: dev_q [R][nq][128] (normed + rotated), dev_k [R][nkv][128] (normed + rotated, read back from the K page it was
// written to), dev_v [R][nkv][128] (read back from the V page).  Every row is its own sequence (page table = one page each).
int32_t mtts_k_rope_kvwrite(const void* dev_qkv, const int32_t* host_pos, const void* dev_qnorm, const void* dev_knorm,
                            const void* dev_cos, const void* dev_sin, int32_t R, int32_t nq, int32_t nkv, float eps,
                            void* dev_q, void* dev_k, void* dev_v, void* stream) {
    if (!dev_qkv || !host_pos || !dev_q || !dev_k || !dev_v || R < 1 || R > MTTS_RCAP || nq < 1 || nkv < 1) return fail(MTTS_EINVAL, "rope_kvwrite: bad argument");
    hipStream_t st = S(stream);
    const int N = (nq + 2 * nkv) * MTTS_HD;
    int maxpos = 0;
    for (int r = 0; r < R; ++r) { if (host_pos[r] < 0) return fail(MTTS_EINVAL, "negative position"); maxpos = std::max(maxpos, host_pos[r]); }
    const int max_pages = maxpos / MTTS_PAGE + 1, total_pages = R * max_pages;
    float* slab = nullptr; RowMeta* meta = nullptr; int32_t* pt = nullptr; uint16_t *kc = nullptr, *vc = nullptr;
    DevBufs hb;
    TRY(hb.get(&slab, (size_t)MTTS_PFCAP * N));
    TRY(hb.get(&meta, R)); TRY(hb.get(&pt, (size_t)R * max_pages));
    TRY(hb.get(&kc, (size_t)total_pages * nkv * MTTS_PAGE * MTTS_HD)); TRY(hb.get(&vc, (size_t)total_pages * nkv * MTTS_PAGE * MTTS_HD));
    std::vector<RowMeta> hm(R);
    std::vector<int32_t> hpt((size_t)R * max_pages);
    for (int r = 0; r < R; ++r) { hm[r] = RowMeta{r, host_pos[r], 1, 0}; for (int p = 0; p < max_pages; ++p) hpt[(size_t)r * max_pages + p] = r * max_pages + p; }
    HIPCHK(hipMemcpy(meta, hm.data(), R * sizeof(RowMeta), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(pt, hpt.data(), hpt.size() * 4, hipMemcpyHostToDevice));
    launch_bf16_to_f32(dev_qkv, slab, (size_t)R * N, st);
    launch_qkv_post(slab, 1, N, meta, dev_qnorm, dev_knorm, dev_cos, dev_sin, dev_q, kc, vc, pt, max_pages, total_pages, R, nq, nkv, eps, st);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(st));
    // read the written K / V rows back out of their pages
    std::vector<uint16_t> hk((size_t)total_pages * nkv * MTTS_PAGE * MTTS_HD), hv(hk.size()), ok((size_t)R * nkv * MTTS_HD), ov(ok.size());
    HIPCHK(hipMemcpy(hk.data(), kc, hk.size() * 2, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(hv.data(), vc, hv.size() * 2, hipMemcpyDeviceToHost));
    for (int r = 0; r < R; ++r)
        for (int h = 0; h < nkv; ++h)
            for (int d = 0; d < MTTS_HD; ++d) {
                const int page = r * max_pages + host_pos[r] / MTTS_PAGE, t = host_pos[r] % MTTS_PAGE;
                const size_t base = ((size_t)h * total_pages + page) * (MTTS_PAGE * MTTS_HD);
                ok[((size_t)r * nkv + h) * MTTS_HD + d] = hk[base + (((d >> 3) * 64) + t) * 8 + (d & 7)];
                ov[((size_t)r * nkv + h) * MTTS_HD + d] = hv[base + ((size_t)(t >> 1) * MTTS_HD + d) * 2 + (t & 1)];
            }
    HIPCHK(hipMemcpy(dev_k, ok.data(), ok.size() * 2, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(dev_v, ov.data(), ov.size() * 2, hipMemcpyHostToDevice));
    return MTTS_OK;
}

// Decode attention of one query token per row over a paged cache (attn_scores / attn_pv / attn_combine, the launches of
// a decode step): dev_q bf16 [R][nq][128]; dev_k / dev_v bf16 [R][Lmax][nkv][128] row-major (row r uses its first
// host_lens[r] tokens; its query sits at position host_lens[r]-1); host_page_table int32 [R][pages] with
// pages = ceil(Lmax/64): any permutation of 0..R*pages-1 (NULL = consecutive).  dev_out bf16 [R][nq*128].
int32_t mtts_k_paged_attn_decode(const void* dev_q, const void* dev_k, const void* dev_v, const int32_t* host_lens,
                                 const int32_t* host_page_table, int32_t R, int32_t Lmax, int32_t nq, int32_t nkv,
                                 void* dev_out, void* stream) {
    if (!dev_q || !dev_k || !dev_v || !host_lens || !dev_out || R < 1 || R > MTTS_MAXR || Lmax < 1 || nq < 1 || nkv < 1 || nq % nkv)
        return fail(MTTS_EINVAL, "paged_attn_decode: bad argument (1..32 rows)");
    hipStream_t st = S(stream);
    const int max_pages = pages_for(Lmax), total_pages = R * max_pages, nch = (max_pages + ATT_PB - 1) / ATT_PB;
    std::vector<int32_t> hpt((size_t)R * max_pages);
    std::vector<char> seen(total_pages, 0);
    for (size_t i = 0; i < hpt.size(); ++i) {
        hpt[i] = host_page_table ? host_page_table[i] : (int32_t)i;
        if (hpt[i] < 0 || hpt[i] >= total_pages || seen[hpt[i]]) return fail(MTTS_EINVAL, "page table must be a permutation of 0..%d", total_pages - 1);
        seen[hpt[i]] = 1;
    }
    std::vector<RowMeta> hm(MTTS_MAXR, RowMeta{-1, 0, 0, 0});
    int pages_bound = 1;
    for (int r = 0; r < R; ++r) {
        if (host_lens[r] < 1 || host_lens[r] > Lmax) return fail(MTTS_EINVAL, "row %d: length %d outside 1..%d", r, host_lens[r], Lmax);
        hm[r] = RowMeta{r, host_lens[r] - 1, 1, 0};
        pages_bound = std::max(pages_bound, pages_for(host_lens[r]));
    }
    RowMeta* meta = nullptr; int32_t *pt = nullptr, *lens = nullptr; uint16_t *kc = nullptr, *vc = nullptr, *scores = nullptr, *outp = nullptr;
    float *stats = nullptr, *opart = nullptr;
    const size_t cache_n = (size_t)total_pages * nkv * MTTS_PAGE * MTTS_HD;
    DevBufs hb;
    TRY(hb.get(&meta, MTTS_MAXR)); TRY(hb.get(&pt, hpt.size())); TRY(hb.get(&lens, R));
    TRY(hb.get(&kc, cache_n)); TRY(hb.get(&vc, cache_n));
    TRY(hb.get(&scores, (size_t)MTTS_MAXR * nq * max_pages * MTTS_PAGE));
    TRY(hb.get(&stats, (size_t)MTTS_MAXR * nq * max_pages * 2));
    TRY(hb.get(&opart, (size_t)MTTS_MAXR * nq * nch * MTTS_HD));
    TRY(hb.get(&outp, (size_t)MTTS_MAXR * nq * MTTS_HD));
    HIPCHK(hipMemcpy(meta, hm.data(), hm.size() * sizeof(RowMeta), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(pt, hpt.data(), hpt.size() * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(lens, host_lens, R * 4, hipMemcpyHostToDevice));
    launch_pack_kv_pages(dev_k, dev_v, kc, vc, pt, lens, R, Lmax, nkv, max_pages, total_pages, st);
    // like the engine: complete pages are read in their sealed form unless MTTS_KV_PACK=0
    KvPack pk{nullptr, nullptr};
    const char* g = getenv("MTTS_KV_PACK");
    if (!g || atoi(g) != 0) {
        uint8_t *kp = nullptr, *vp = nullptr;
        const size_t pk_n = (size_t)total_pages * nkv * MTTS_PKU * 64 * 16;
        TRY(hb.get(&kp, pk_n)); TRY(hb.get(&vp, pk_n));
        launch_kv_seal_all(kc, vc, kp, vp, total_pages, nkv, 1, nullptr, st);
        pk = KvPack{kp, vp};
    }
    const float scale = 1.0f / sqrtf((float)MTTS_HD);
    if (launch_attn(dev_q, kc, vc, pt, meta, scores, stats, opart, outp, MTTS_MAXR, pages_bound, max_pages, total_pages, nch, nq, nkv,
                    scale, nullptr, ATTN_ALL, st, pk.k ? &pk : nullptr))
        return fail(MTTS_EINVAL, "attention group size not built (1, 2, 4)");
    launch_unpack_rows(outp, dev_out, R, nq * MTTS_HD, st);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(st));
    return MTTS_OK;
}

// Test hook: the attention section of one decode layer -- q/k/v epilogue, scores, P.V, sum of the chunk partials -- on
// given qkv slabs, through either path: `path` 0 = attn_scores + attn_pv + attn_combine (fused epilogue), 1 = the
// whole-row kernel (ATTN_ROW).  dev_slabs fp32 [ksplit][R][Npad], Npad = (nq + 2 nkv) * 128: the qkv GEMM's split-K
// partials of the rows' new token; dev_k / dev_v bf16 [R][Lmax][nkv][128]: the tokens already cached (row r: its first
// host_lens[r] - 1; host_lens[r] = its length WITH the new token, 0 = an idle row); dev_cos / dev_sin bf16 [Lmax][64];
// host_page_table as in mtts_k_paged_attn_decode.  `sealed` != 0: every page is also sealed and complete pages are read
// in that form.  Out: dev_out bf16 [32][nq*128] in the X-fragment layout (as the o_proj GEMM reads it), the bf16 pools
// dev_kcache / dev_vcache [nkv][R * pages][64 * 128] after the launch (with the new K / V rows) and, when sealed and not
// null, the sealed pools dev_kpack / dev_vpack [nkv][R * pages][13 * 64 * 16 B].
int32_t mtts_k_attn_section(const float* dev_slabs, int32_t ksplit, const void* dev_qnw, const void* dev_knw, const void* dev_cos,
                            const void* dev_sin, float eps, const void* dev_k, const void* dev_v, const int32_t* host_lens,
                            const int32_t* host_page_table, int32_t R, int32_t Lmax, int32_t nq, int32_t nkv, int32_t sealed,
                            int32_t path, void* dev_out, void* dev_kcache, void* dev_vcache, void* dev_kpack, void* dev_vpack,
                            void* stream) {
    if (!dev_slabs || !dev_qnw || !dev_knw || !dev_cos || !dev_sin || !dev_k || !dev_v || !host_lens || !dev_out || !dev_kcache ||
        !dev_vcache || R < 1 || R > MTTS_MAXR || Lmax < 1 || nq < 1 || nkv < 1 || nq % nkv || ksplit < 1 || (path != 0 && path != 1))
        return fail(MTTS_EINVAL, "attn_section: bad argument (1..32 rows, path 0 or 1)");
    hipStream_t st = S(stream);
    const int max_pages = pages_for(Lmax), total_pages = R * max_pages, nch = (max_pages + ATT_PB - 1) / ATT_PB;
    const int Npad = (nq + 2 * nkv) * MTTS_HD;
    std::vector<int32_t> hpt((size_t)R * max_pages);
    std::vector<char> seen(total_pages, 0);
    for (size_t i = 0; i < hpt.size(); ++i) {
        hpt[i] = host_page_table ? host_page_table[i] : (int32_t)i;
        if (hpt[i] < 0 || hpt[i] >= total_pages || seen[hpt[i]]) return fail(MTTS_EINVAL, "page table must be a permutation of 0..%d", total_pages - 1);
        seen[hpt[i]] = 1;
    }
    std::vector<RowMeta> hm(MTTS_MAXR, RowMeta{-1, 0, 0, 0});
    std::vector<int32_t> cached(R, 0);
    int pages_bound = 1;
    for (int r = 0; r < R; ++r) {
        if (host_lens[r] < 0 || host_lens[r] > Lmax) return fail(MTTS_EINVAL, "row %d: length %d outside 0..%d", r, host_lens[r], Lmax);
        if (!host_lens[r]) continue;
        hm[r] = RowMeta{r, host_lens[r] - 1, 1, 0};
        cached[r] = host_lens[r] - 1;
        pages_bound = std::max(pages_bound, pages_for(host_lens[r]));
    }
    pages_bound = std::min(round_up(pages_bound, ATT_PB), max_pages);      // as a captured decode step sizes its launches
    RowMeta* meta = nullptr; int32_t *pt = nullptr, *lens = nullptr; uint16_t *kc = nullptr, *vc = nullptr, *scores = nullptr, *outp = nullptr;
    float *stats = nullptr, *opart = nullptr, *slabs = nullptr;
    uint8_t *kp = nullptr, *vp = nullptr;
    const size_t cache_n = (size_t)total_pages * nkv * MTTS_PAGE * MTTS_HD, pk_n = (size_t)total_pages * nkv * MTTS_PKU * 64 * 16;
    DevBufs hb;
    TRY(hb.get(&meta, MTTS_MAXR)); TRY(hb.get(&pt, hpt.size())); TRY(hb.get(&lens, R));
    TRY(hb.get(&kc, cache_n)); TRY(hb.get(&vc, cache_n));
    TRY(hb.get(&scores, (size_t)MTTS_MAXR * nq * max_pages * MTTS_PAGE));
    TRY(hb.get(&stats, (size_t)MTTS_MAXR * nq * max_pages * 2));
    TRY(hb.get(&opart, (size_t)MTTS_MAXR * nq * nch * MTTS_HD));
    TRY(hb.get(&outp, (size_t)MTTS_MAXR * nq * MTTS_HD));
    TRY(hb.get(&slabs, (size_t)ksplit * MTTS_PFCAP * Npad, false));        // (the kernels' slab stride is MTTS_PFCAP rows)
    HIPCHK(hipMemcpyAsync(meta, hm.data(), hm.size() * sizeof(RowMeta), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(pt, hpt.data(), hpt.size() * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(lens, cached.data(), R * 4, hipMemcpyHostToDevice, st));
    for (int k = 0; k < ksplit; ++k)
        HIPCHK(hipMemcpyAsync(slabs + (size_t)k * MTTS_PFCAP * Npad, dev_slabs + (size_t)k * R * Npad, (size_t)R * Npad * 4, hipMemcpyDeviceToDevice, st));
    launch_pack_kv_pages(dev_k, dev_v, kc, vc, pt, lens, R, Lmax, nkv, max_pages, total_pages, st);
    KvPack pk{nullptr, nullptr};
    if (sealed) {
        TRY(hb.get(&kp, pk_n)); TRY(hb.get(&vp, pk_n));
        launch_kv_seal_all(kc, vc, kp, vp, total_pages, nkv, 1, nullptr, st);
        pk = KvPack{kp, vp};
    }
    const QkvFuse fz{slabs, ksplit, Npad, (const uint16_t*)dev_qnw, (const uint16_t*)dev_knw, (const uint16_t*)dev_cos, (const uint16_t*)dev_sin, eps};
    const float scale = 1.0f / sqrtf((float)MTTS_HD);
    if (path == 1) {
        if (attn_row_prepare()) return fail(MTTS_EINVAL, "attn_row_kernel: the dynamic LDS limit could not be raised");
        if (!attn_row_fits(nq / nkv, &fz, sealed ? &pk : nullptr, pages_bound)) return fail(MTTS_EINVAL, "attn_section: the whole-row kernel does not take this shape");
    }
    if (const int rc = launch_attn(nullptr, kc, vc, pt, meta, scores, stats, opart, outp, MTTS_MAXR, pages_bound, max_pages, total_pages, nch,
                                   nq, nkv, scale, &fz, path == 1 ? ATTN_ROW : ATTN_ALL, st, sealed ? &pk : nullptr))
        return fail(MTTS_EINVAL, rc == -2 ? "attn_section: the whole-row kernel does not take this shape" : "attention group size not built (1, 2, 4)");
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(dev_out, outp, (size_t)MTTS_MAXR * nq * MTTS_HD * 2, hipMemcpyDeviceToDevice, st));
    HIPCHK(hipMemcpyAsync(dev_kcache, kc, cache_n * 2, hipMemcpyDeviceToDevice, st));
    HIPCHK(hipMemcpyAsync(dev_vcache, vc, cache_n * 2, hipMemcpyDeviceToDevice, st));
    if (sealed && dev_kpack) HIPCHK(hipMemcpyAsync(dev_kpack, kp, pk_n, hipMemcpyDeviceToDevice, st));
    if (sealed && dev_vpack) HIPCHK(hipMemcpyAsync(dev_vpack, vp, pk_n, hipMemcpyDeviceToDevice, st));
    HIPCHK(hipStreamSynchronize(st));
    return MTTS_OK;
}
int64_t mtts_debug_attn_row_launches(void) { return (int64_t)mtts_attn_row_launches(); }

// Test hook: the attention section of one PREFILL pass (tests/test_attn_prefill_gpu.py) -- qkv_post_kernel over many rows
// of one dialogue, attn_prefill_scores_kernel, attn_prefill_pv_kernel and attn_combine_kernel with the prefill chunking
// (ATT_PF pages) -- for B dialogues on caller buffers.  Dialogue b has host_cached[b] tokens in its pages already (a
// multiple of 32, 0 <= cached < lens <= Lmax: the state at the start of a later pass of a long prompt) and the pass
// carries its tokens cached[b] .. lens[b] - 1.  The rows are staged as mtts_begin stages them (engine.hip):
//     for (int b = 0; b < B; r = (r + MTTS_MAXR - 1) / MTTS_MAXR * MTTS_MAXR, ++b)
//         for (int i = 0; i < e->n_real[b * takes]; ++i, ++r) ... metas[r] = RowMeta{b * takes, i, i == n_real - 1 ? 1 : 0, 0};
// every dialogue on a 32-row tile boundary, filler rows RowMeta{-1, 0, 0, 0}, the pass padded to a multiple of MTTS_RCAP
// rows (`size_t Mpad = (Mtot + MTTS_RCAP - 1) / MTTS_RCAP * MTTS_RCAP`) with wholly idle tiles, pages_bound =
// max_b ceil(lens[b] / 64) (`prefill_staged(e, sr.Mpad, pages_for(e->max_real), ...)`).  The launches are
// attend_layer's for prefill == true, fused == false, sealed == false (engine.hip), with nchunks_max the engine's
// `e->nchunks_max = (e->max_pages + ATT_PB - 1) / ATT_PB`:
//     launch_qkv_post(e->partial, ks_qkv, e->qkv_rows, d_meta, l.qn, l.kn, e->rope_cos, e->rope_sin, e->qbuf,
//                     kc, vc, e->d_page_table, e->max_pages, e->total_pages, R, e->nq, e->nkv, eps, st);
//     for (int i = 0; i < nphases; ++i)            // prefill_ph[3] = {ATTN_PF_SCORES, ATTN_PF_PV, ATTN_PF_COMBINE}
//         launch_attn(e->qbuf, kc, vc, e->d_page_table, d_meta, e->scores, e->stats, e->opart, e->attn_p, R,
//                     pages_bound, e->max_pages, e->total_pages, e->nchunks_max, e->nq, e->nkv, scale,
//                     fused ? &fz : nullptr, (prefill ? prefill_ph : decode_ph)[i], st, pkp);
// dev_slabs fp32 [ksplit][M][Npad], Npad = (nq + 2 nkv) * 128, M = sum_b round_up(lens[b] - cached[b], 32) <= MTTS_PFCAP,
// copied into the kernels' slab stride (MTTS_PFCAP rows); dev_k / dev_v bf16 [B][Lmax][nkv][128]: ALL Lmax tokens of every
// dialogue are packed into the pools before the pass, so the caller decides what lies behind a dialogue's end; dev_cos /
// dev_sin bf16 [Lmax][64]; host_page_table as in mtts_k_paged_attn_decode.  qbuf, scores, stats, opart (and the slab rows
// the caller does not give) start as 0xff bytes (NaN): a slot the kernels may load but must not use shows in the result.
// Out: dev_out bf16 [M][nq*128] row-major, dev_q bf16 [M][nq][128] (idle rows: the 0xff fill), the bf16 pools after the
// pass dev_kcache / dev_vcache [nkv][B * pages][64 * 128].
int32_t mtts_k_attn_prefill(const float* dev_slabs, int32_t ksplit, const void* dev_qnw, const void* dev_knw, const void* dev_cos,
                            const void* dev_sin, float eps, const void* dev_k, const void* dev_v, const int32_t* host_lens,
                            const int32_t* host_cached, const int32_t* host_page_table, int32_t B, int32_t Lmax, int32_t nq,
                            int32_t nkv, void* dev_out, void* dev_q, void* dev_kcache, void* dev_vcache, void* stream) {
    if (!dev_slabs || !dev_qnw || !dev_knw || !dev_cos || !dev_sin || !dev_k || !dev_v || !host_lens || !host_cached || !dev_out ||
        !dev_q || !dev_kcache || !dev_vcache || B < 1 || B > MTTS_RCAP || Lmax < 1 || nq < 1 || nkv < 1 || nq % nkv || ksplit < 1 || ksplit > 8)
        return fail(MTTS_EINVAL, "attn_prefill: bad argument (1..%d dialogues, nq %% nkv == 0, 1 <= ksplit <= 8)", MTTS_RCAP);
    if (const int G = nq / nkv; G != 1 && G != 2 && G != 4) return fail(MTTS_EINVAL, "attention group size not built (1, 2, 4)");
    const int max_pages = pages_for(Lmax), total_pages = B * max_pages, nch = (max_pages + ATT_PB - 1) / ATT_PB;
    const int nch_pf = (max_pages + ATT_PF - 1) / ATT_PF, Npad = (nq + 2 * nkv) * MTTS_HD;
    int64_t M = 0;
    int pages_bound = 1;
    for (int b = 0; b < B; ++b) {
        const int n = host_lens[b], c = host_cached[b];
        if (c < 0 || c % MTTS_MAXR || c >= n || n > Lmax)
            return fail(MTTS_EINVAL, "attn_prefill: dialogue %d: need cached %% 32 == 0 and 0 <= cached (%d) < lens (%d) <= Lmax (%d)", b, c, n, Lmax);
        M += round_up(n - c, MTTS_MAXR);
        pages_bound = std::max(pages_bound, pages_for(n));
    }
    if (M > MTTS_PFCAP) return fail(MTTS_EINVAL, "attn_prefill: %lld staged rows, a pass holds %d", (long long)M, MTTS_PFCAP);
    std::vector<int32_t> hpt((size_t)total_pages);
    std::vector<char> seen(total_pages, 0);
    for (size_t i = 0; i < hpt.size(); ++i) {
        hpt[i] = host_page_table ? host_page_table[i] : (int32_t)i;
        if (hpt[i] < 0 || hpt[i] >= total_pages || seen[hpt[i]]) return fail(MTTS_EINVAL, "page table must be a permutation of 0..%d", total_pages - 1);
        seen[hpt[i]] = 1;
    }
    const int R = round_up((int)M, MTTS_RCAP);
    std::vector<RowMeta> hm(R, RowMeta{-1, 0, 0, 0});
    {
        int r = 0;
        for (int b = 0; b < B; r = round_up(r, MTTS_MAXR), ++b)
            for (int i = host_cached[b]; i < host_lens[b]; ++i, ++r) hm[r] = RowMeta{b, i, i == host_lens[b] - 1 ? 1 : 0, 0};
    }
    hipStream_t st = S(stream);
    RowMeta* meta = nullptr; int32_t *pt = nullptr, *lens = nullptr; uint16_t *kc = nullptr, *vc = nullptr, *qbuf = nullptr, *scores = nullptr, *outp = nullptr;
    float *stats = nullptr, *opart = nullptr, *slabs = nullptr;
    const size_t cache_n = (size_t)total_pages * nkv * MTTS_PAGE * MTTS_HD;
    const size_t q_n = (size_t)R * nq * MTTS_HD, sc_n = (size_t)R * nq * max_pages * MTTS_PAGE, st_n = (size_t)R * nq * max_pages * 2;
    const size_t op_n = (size_t)R * nq * nch_pf * MTTS_HD, sl_n = (size_t)ksplit * MTTS_PFCAP * Npad;
    DevBufs hb;
    TRY(hb.get(&meta, (size_t)R, false)); TRY(hb.get(&pt, hpt.size(), false)); TRY(hb.get(&lens, (size_t)B, false));
    TRY(hb.get(&kc, cache_n)); TRY(hb.get(&vc, cache_n));
    TRY(hb.get(&qbuf, q_n, false)); TRY(hb.get(&scores, sc_n, false)); TRY(hb.get(&stats, st_n, false)); TRY(hb.get(&opart, op_n, false));
    TRY(hb.get(&outp, q_n, false)); TRY(hb.get(&slabs, sl_n, false));
    HIPCHK(hipMemsetAsync(qbuf, 0xff, q_n * 2, st)); HIPCHK(hipMemsetAsync(scores, 0xff, sc_n * 2, st));
    HIPCHK(hipMemsetAsync(stats, 0xff, st_n * 4, st)); HIPCHK(hipMemsetAsync(opart, 0xff, op_n * 4, st));
    HIPCHK(hipMemsetAsync(outp, 0xff, q_n * 2, st)); HIPCHK(hipMemsetAsync(slabs, 0xff, sl_n * 4, st));
    std::vector<int32_t> full(B, Lmax);
    HIPCHK(hipMemcpyAsync(meta, hm.data(), hm.size() * sizeof(RowMeta), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(pt, hpt.data(), hpt.size() * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(lens, full.data(), (size_t)B * 4, hipMemcpyHostToDevice, st));
    for (int k = 0; k < ksplit; ++k)
        HIPCHK(hipMemcpyAsync(slabs + (size_t)k * MTTS_PFCAP * Npad, dev_slabs + (size_t)k * M * Npad, (size_t)M * Npad * 4, hipMemcpyDeviceToDevice, st));
    launch_pack_kv_pages(dev_k, dev_v, kc, vc, pt, lens, B, Lmax, nkv, max_pages, total_pages, st);
    const float scale = 1.0f / sqrtf((float)MTTS_HD);
    launch_qkv_post(slabs, ksplit, Npad, meta, dev_qnw, dev_knw, dev_cos, dev_sin, qbuf, kc, vc, pt, max_pages, total_pages, R, nq, nkv, eps, st);
    static const AttnPhase prefill_ph[3] = {ATTN_PF_SCORES, ATTN_PF_PV, ATTN_PF_COMBINE};
    for (int i = 0; i < 3; ++i)
        if (launch_attn(qbuf, kc, vc, pt, meta, scores, stats, opart, outp, R, pages_bound, max_pages, total_pages, nch, nq, nkv, scale,
                        nullptr, prefill_ph[i], st, nullptr))
            return fail(MTTS_EINVAL, "attention group size not built (1, 2, 4)");
    launch_unpack_rows(outp, dev_out, (int)M, nq * MTTS_HD, st);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(dev_q, qbuf, (size_t)M * nq * MTTS_HD * 2, hipMemcpyDeviceToDevice, st));
    HIPCHK(hipMemcpyAsync(dev_kcache, kc, cache_n * 2, hipMemcpyDeviceToDevice, st));
    HIPCHK(hipMemcpyAsync(dev_vcache, vc, cache_n * 2, hipMemcpyDeviceToDevice, st));
    HIPCHK(hipStreamSynchronize(st));
    return MTTS_OK;
}

// Test hook for the sealed page format (attn.hip: seal_lane): `npages` bf16 pages of 16 KiB -> sealed pages of 13 KiB.
int32_t mtts_k_kv_seal(const void* dev_pages, int32_t npages, void* dev_sealed, int32_t as_k, void* stream) {
    if (!dev_pages || !dev_sealed || npages < 1) return fail(MTTS_EINVAL, "kv_seal: bad argument");
    launch_kv_seal_pages(dev_pages, dev_sealed, npages, as_k, S(stream));
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(S(stream)));
    return MTTS_OK;
}

// Debug hook: out6 = {complete K pages of the live sequences (x kv heads x layers), of which not sealed (a lane did not
// fit: read as bf16), the same two numbers for V, layers whose K / V reads currently use the sealed pages}.
// MTTS_ESTATE when the engine runs without sealed pages.
int32_t mtts_debug_kv_pack_stats(MttsEngine* e, int64_t* out6) {
    if (!e || !out6) return fail(MTTS_EINVAL, "null argument");
    if (!e->kpack) return fail(MTTS_ESTATE, "the engine keeps no sealed pages (fp32 / fp16 engine, or MTTS_KV_PACK=0)");
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipDeviceSynchronize());
    std::vector<SeqState> ss(MTTS_RCAP);
    HIPCHK(hipMemcpy(ss.data(), e->d_seqs, ss.size() * sizeof(SeqState), hipMemcpyDeviceToHost));
    std::vector<int32_t> complete(e->B, 0);
    for (int b = 0; b < e->B; ++b)
        if (e->slot_live[b]) complete[b] = std::min(ss[b].kv_len >> 6, e->pool.pages_of(b));
    DevBufs hb;
    int32_t* dc = nullptr; unsigned long long* dout = nullptr;
    TRY(hb.get(&dc, e->B)); TRY(hb.get(&dout, 4));
    HIPCHK(hipMemcpy(dc, complete.data(), e->B * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemset(dout, 0, 32));
    launch_kv_pack_count(e->kpack, e->vpack, e->d_page_table, dc, e->B, e->max_pages, e->total_pages, e->nkv, e->L, dout, nullptr);
    HIPCHK(hipGetLastError());
    unsigned long long h[4];
    HIPCHK(hipMemcpy(h, dout, 32, hipMemcpyDeviceToHost));
    for (int i = 0; i < 4; ++i) out6[i] = (int64_t)h[i];
    out6[4] = out6[5] = 0;
    for (int n = 0; n < e->L; ++n) { out6[4] += e->pack_k_on[n]; out6[5] += e->pack_v_on[n]; }
    return MTTS_OK;
}

// Measurement hook (bench/profiling only): pretend every live sequence already holds `kv_len` tokens.
// The cache content is whatever the pages hold; used to reach a long context without replaying it
// when collecting PMC counters.
int32_t mtts_debug_set_kv_len(MttsEngine* e, int32_t kv_len) {
    if (!e || !e->began) return fail(MTTS_ESTATE, "mtts_begin has not run");
    if (e->f32) return fail(MTTS_EINVAL, "measurement hook of the bf16 engine");
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipDeviceSynchronize());
    const int cap = std::min(e->max_pages * MTTS_PAGE, e->bufs.rope_rows);          // positions the pages and the RoPE table hold
    const int limit = cap - MTTS_PAGE;
    if (kv_len < 1 || kv_len > limit) return fail(MTTS_EINVAL, "kv_len %d outside 1..%d", kv_len, limit);
    e->max_steps = std::min(e->max_steps, e->steps_issued + cap - kv_len);   // stay inside the pages and the RoPE table
    std::vector<SeqState> ss(MTTS_RCAP);
    HIPCHK(hipMemcpy(ss.data(), e->d_seqs, ss.size() * sizeof(SeqState), hipMemcpyDeviceToHost));
    for (int b = 0; b < e->B; ++b) { ss[b].kv_len = kv_len; e->n_real[b] = kv_len - e->steps_issued; }
    e->max_real = kv_len - e->steps_issued;
    HIPCHK(hipMemcpy(e->d_seqs, ss.data(), ss.size() * sizeof(SeqState), hipMemcpyHostToDevice));
    launch_fill_random_bf16(e->kcache, e->layer_stride * e->L, 0x1234u, nullptr);
    launch_fill_random_bf16(e->vcache, e->layer_stride * e->L, 0x9876u, nullptr);
    if (e->kpack) launch_kv_seal_all(e->kcache, e->vcache, e->kpack, e->vpack, e->total_pages, e->nkv, e->L, nullptr, nullptr);
    HIPCHK(hipDeviceSynchronize());
    return MTTS_OK;
}

// Measurement hook: `iters` back-to-back launches of one attention pass (phase 1 = scores, 2 = PV, 3 = combine of the
// two-pass kernels; 0 = those three in a row; 4 = the whole-row kernel, whatever MTTS_ATTN_ROW says) at the
// engine's CURRENT decode state, cycling over the layers' caches; average duration from two HIP events on the
// launch stream.  (Events around a single launch also time the launch gap, which rocprof's kernel duration
// does not; a train of launches does not have that bias.)
int32_t mtts_k_attn_bench(MttsEngine* e, int32_t phase, int32_t iters, float* avg_ms, int64_t* bytes_per_launch) {
    if (!e || !e->began || phase < ATTN_ALL || phase > ATTN_ROW || iters < 1 || !avg_ms) return fail(MTTS_EINVAL, "attn_bench: bad argument");
    if (e->f32) return fail(MTTS_EINVAL, "measurement hook of the bf16 engine");
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipDeviceSynchronize());
    const float scale = 1.0f / sqrtf((float)MTTS_HD);
    const int R = round_up(e->B, 32);
    const int len_bound = e->max_real + e->steps_issued + 1;
    const int pages_bound = pages_for(len_bound);
    const StepPlan plan = decode_plan(e, pages_bound);      // the step's sealed reads per layer
    if (phase == ATTN_ROW) {
        if (attn_row_prepare()) return fail(MTTS_EINVAL, "attn_row_kernel: the dynamic LDS limit could not be raised");
        const QkvFuse f0{e->bufs.partial, e->p_qkv.ksplit, e->qkv_rows, nullptr, nullptr, nullptr, nullptr, 0.f};
        for (int n = 0; n < e->L; ++n) {
            const KvPack pk = layer_pack(e, plan, n);
            if (!attn_row_fits(e->nq / e->nkv, &f0, (pk.k || pk.v) ? &pk : nullptr, pages_bound))
                return fail(MTTS_EINVAL, "attn_bench: the whole-row kernel does not take this shape");
        }
    }
    hipEvent_t e0, e1;
    hipEventCreate(&e0); hipEventCreate(&e1);
    auto run = [&](int n) {
        for (int i = 0; i < n; ++i) {
            const int layer = i % e->L;
            uint16_t* kc = (uint16_t*)e->kcache + e->layer_stride * layer;
            uint16_t* vc = (uint16_t*)e->vcache + e->layer_stride * layer;
            // the product's decode launch: q/k/v epilogue fused (the slabs are whatever the last step left there)
            const QkvFuse fz{e->bufs.partial, e->p_qkv.ksplit, e->qkv_rows, (const uint16_t*)e->layers[layer].qn,
                             (const uint16_t*)e->layers[layer].kn, e->bufs.rope_cos, e->bufs.rope_sin, e->cfg.rms_norm_eps};
            const KvPack pk = layer_pack(e, plan, layer);
            launch_attn(e->qbuf, kc, vc, e->d_page_table, e->d_meta, e->scores, e->stats, e->opart, e->attn_p, R, pages_bound,
                        e->max_pages, e->total_pages, e->nchunks_max, e->nq, e->nkv, scale, (phase == ATTN_ROW || e->B * pages_bound <= e->knobs.fuse_qkv_max) ? &fz : nullptr, (AttnPhase)phase, nullptr,
                        (pk.k || pk.v) ? &pk : nullptr);
        }
    };
    run(e->L);                               // warm-up
    hipEventRecord(e0, nullptr);
    run(iters);
    hipEventRecord(e1, nullptr);
    HIPCHK(hipEventSynchronize(e1));
    float ms = 0;
    hipEventElapsedTime(&ms, e0, e1);
    *avg_ms = ms / iters;
    if (bytes_per_launch) {
        std::vector<RowMeta> m(MTTS_RCAP);
        HIPCHK(hipMemcpy(m.data(), e->d_meta, m.size() * sizeof(RowMeta), hipMemcpyDeviceToHost));
        int64_t tok = 0;
        for (int b = 0; b < R; ++b) if (m[b].seq >= 0) tok += m[b].pos + 1;
        // K, V or both; the combine reads neither
        *bytes_per_launch = phase == ATTN_COMBINE ? 0 : tok * e->nkv * MTTS_HD * 2 * ((phase == ATTN_ALL || phase == ATTN_ROW) ? 2 : 1);
    }
    hipEventDestroy(e0); hipEventDestroy(e1);
    return MTTS_OK;
}

// Tuning hook (not part of the product path): average time of one skinny-GEMM launch over `copies`
// distinct weight buffers (so that no launch finds its weights in L2 / Infinity Cache).
int32_t mtts_k_gemm_bench(int32_t N, int32_t K, int32_t epi, int32_t ksplit, int32_t waves, int32_t copies,
                                     int32_t iters, float* avg_us) {
    if (N % 32 || K % 16 || copies < 1 || iters < 1 || !avg_us) return fail(MTTS_EINVAL, "gemm_bench: bad argument");
    // waves < 0: the tiled prefill kernel on -waves rows (<= MTTS_PFCAP), split-K as given
    const int tile_rows = waves < 0 ? -waves : 0;
    if (tile_rows > MTTS_PFCAP) return fail(MTTS_EINVAL, "gemm_bench: at most MTTS_PFCAP rows");
    GemmPlan p = (ksplit > 0 && waves > 0) ? mtts_plan_gemm_forced(N, K, ksplit, waves) : mtts_plan_gemm(N, K, tile_rows ? std::max(ksplit, 1) : ksplit);
    if (tile_rows) p.ksplit = std::max(ksplit, 1);
    p.depth = gemm_depth_env();
    DevBufs hb;
    std::vector<uint16_t*> w(copies, nullptr);
    for (auto& q : w) { TRY(hb.get(&q, (size_t)N * K, false)); HIPCHK(hipMemset(q, 0x3c, (size_t)N * K * 2)); }
    uint16_t *x = nullptr, *out = nullptr;
    float* part = nullptr;
    TRY(hb.get(&x, (size_t)MTTS_PFCAP * K, false));
    HIPCHK(hipMemset(x, 0x3c, (size_t)MTTS_PFCAP * K * 2));
    TRY(hb.get(&out, (size_t)MTTS_PFCAP * N));
    TRY(hb.get(&part, (size_t)p.ksplit * MTTS_PFCAP * N));
    hipEvent_t e0, e1;
    hipEventCreate(&e0); hipEventCreate(&e1);
    auto go = [&](int i) {
        if (tile_rows) launch_gemm_tile(epi, tile_rows, p.ksplit, w[i % copies], x, K, N, N, part, out, nullptr);
        else launch_gemm(epi, 1, p, w[i % copies], x, K, N, N, part, out, nullptr);
    };
    for (int i = 0; i < copies; ++i) go(i);
    HIPCHK(hipDeviceSynchronize());
    hipEventRecord(e0, nullptr);
    for (int i = 0; i < iters; ++i) go(i);
    hipEventRecord(e1, nullptr);
    HIPCHK(hipEventSynchronize(e1));
    float ms = 0;
    hipEventElapsedTime(&ms, e0, e1);
    *avg_us = ms * 1000.f / iters;
    hipEventDestroy(e0); hipEventDestroy(e1);
    return MTTS_OK;
}

// ---- o_proj -> post-attention norm -> gate/up as two launches (gemm_fold.hip) ----------------------------------------------
int64_t mtts_debug_fold_norm_launches(void) { return (int64_t)mtts_fold_norm_launches(); }

static int fold_hook_args(const char* who, int R, int N) {
    if (R < 1 || R > 32 || N < 32 || N % 32) return fail(MTTS_EINVAL, "%s: need 1<=R<=32, N%%32==0 (K is 2048)", who);
    return MTTS_OK;
}

// The producer alone: x [R][N] += attn [R][2048] * Wo [N][2048]^T (all bf16 row-major), in place, and the packed copy.
int32_t mtts_k_oproj_resid(const void* dev_wo, const void* dev_attn, void* dev_x, void* dev_x_packed, int32_t R, int32_t N,
                           void* stream) {
    if (!dev_wo || !dev_attn || !dev_x || !dev_x_packed) return fail(MTTS_EINVAL, "oproj_resid: null argument");
    TRY(fold_hook_args("oproj_resid", R, N));
    hipStream_t st = S(stream);
    const int K = 2048;
    uint16_t *wp = nullptr, *ap = nullptr;
    DevBufs hb;
    TRY(hb.get(&wp, (size_t)N * K));
    TRY(hb.get(&ap, (size_t)32 * K));
    launch_pack_weight(dev_wo, wp, N, K, N, 1, 0, st);
    launch_pack_rows(dev_attn, ap, R, K, 1, st);
    launch_oproj_resid(wp, ap, dev_x, dev_x_packed, R, N, st);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(st));
    return MTTS_OK;
}

// The pair: the producer as above with N = H = 2048, then gate/up with the norm prologue on Wgu [N_gu][2048] (gate and up
// rows interleaved, N_gu % 96 == 0).  The hook's x' tile starts as zeros (rows >= R stay zero: the consumer reads all 32).
int32_t mtts_k_fold_pair(const void* dev_wo, const void* dev_attn, void* dev_x, const void* dev_norm_w, const void* dev_wgu,
                         float eps, int32_t R, int32_t N_gu, void* dev_y, void* stream) {
    if (!dev_wo || !dev_attn || !dev_x || !dev_norm_w || !dev_wgu || !dev_y) return fail(MTTS_EINVAL, "fold_pair: null argument");
    const int H = 2048, K = 2048;
    TRY(fold_hook_args("fold_pair", R, H));
    const GemmPlan p_o = mtts_plan_gemm(H, K, 0), p_gu = mtts_plan_gemm(N_gu > 0 ? N_gu : 32, H, 1);
    if (N_gu < 96 || N_gu % 96) return fail(MTTS_EINVAL, "fold_pair: gate/up needs N %% 96 == 0");
    if (!fold_norm_shape(p_o, K, p_gu, H, N_gu)) return fail(MTTS_EINVAL, "fold_pair: the planner does not give these GEMMs the shapes the pair is built for");
    hipStream_t st = S(stream);
    uint16_t *wp = nullptr, *ap = nullptr, *gp = nullptr, *xp = nullptr, *op = nullptr;
    DevBufs hb;
    TRY(hb.get(&wp, (size_t)H * K));
    TRY(hb.get(&ap, (size_t)32 * K));
    TRY(hb.get(&gp, (size_t)N_gu * H));
    TRY(hb.get(&xp, (size_t)32 * H));
    TRY(hb.get(&op, (size_t)32 * (N_gu / 2)));
    launch_pack_weight(dev_wo, wp, H, K, H, 1, 0, st);
    launch_pack_rows(dev_attn, ap, R, K, 1, st);
    launch_pack_weight(dev_wgu, gp, N_gu, H, N_gu, 1, 0, st);
    launch_oproj_resid(wp, ap, dev_x, xp, R, H, st);
    launch_gateup_norm(gp, xp, dev_norm_w, eps, op, N_gu, st);
    launch_unpack_rows(op, dev_y, R, N_gu / 2, st);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(st));
    return MTTS_OK;
}

// Measurement hook: launch trains of the seam at H = K = 2048 over `copies` rotating copies of both weight arrays (every
// value 0x3c3c).  mode 0: o_proj (split-K 4) + resid_norm + gate/up, the three launches; 1: producer + consumer; 10 .. 14: one
// launch of the above alone (o_proj, resid_norm, gate/up, producer, consumer).  avg_us is the time of one pass through the
// seam.  (The residual stream keeps adding the same bf16 increment and stops growing once that falls below half an ulp: it stays finite.)
int32_t mtts_k_fold_bench(int32_t N_gu, int32_t copies, int32_t iters, int32_t mode, float* avg_us) {
    const int H = 2048, K = 2048;
    if (copies < 1 || iters < 1 || mode < 0 || (mode > 1 && mode < 10) || mode > 14 || !avg_us) return fail(MTTS_EINVAL, "fold_bench: bad argument");
    GemmPlan p_o = mtts_plan_gemm(H, K, 0), p_gu = mtts_plan_gemm(N_gu > 0 ? N_gu : 32, H, 1);
    p_o.depth = p_gu.depth = 1;
    if (N_gu < 96 || N_gu % 96) return fail(MTTS_EINVAL, "fold_bench: gate/up needs N %% 96 == 0");
    if (!fold_norm_shape(p_o, K, p_gu, H, N_gu)) return fail(MTTS_EINVAL, "fold_bench: the planner does not give these GEMMs the shapes the pair is built for");
    DevBufs hb;
    std::vector<uint16_t*> wo(copies, nullptr), wgu(copies, nullptr);
    for (int c = 0; c < copies; ++c) {
        TRY(hb.get(&wo[c], (size_t)H * K, false)); HIPCHK(hipMemset(wo[c], 0x3c, (size_t)H * K * 2));
        TRY(hb.get(&wgu[c], (size_t)N_gu * H, false)); HIPCHK(hipMemset(wgu[c], 0x3c, (size_t)N_gu * H * 2));
    }
    uint16_t *attn = nullptr, *x = nullptr, *xn = nullptr, *xp = nullptr, *act = nullptr, *nw = nullptr;
    float* part = nullptr;
    RowMeta* meta = nullptr;
    TRY(hb.get(&attn, (size_t)32 * K, false)); HIPCHK(hipMemset(attn, 0x3c, (size_t)32 * K * 2));
    TRY(hb.get(&x, (size_t)32 * H));
    TRY(hb.get(&xn, (size_t)32 * H));
    TRY(hb.get(&xp, (size_t)32 * H));
    TRY(hb.get(&act, (size_t)32 * (N_gu / 2)));
    TRY(hb.get(&nw, (size_t)H, false)); HIPCHK(hipMemset(nw, 0x3c, (size_t)H * 2));
    TRY(hb.get(&part, (size_t)p_o.ksplit * MTTS_PFCAP * H));
    TRY(hb.get(&meta, 32));
    const float eps = 1e-6f;
    auto go = [&](int i) {
        const int c = i % copies;
        if (mode == 0 || mode == 10) launch_gemm(EPI_PARTIAL, 1, p_o, wo[c], attn, K, H, H, part, nullptr, nullptr);
        if (mode == 0 || mode == 11) launch_resid_norm(part, p_o.ksplit, H, x, nw, xn, nullptr, meta, 32, H, eps, nullptr);
        if (mode == 0 || mode == 12) launch_gemm(EPI_SILU, 1, p_gu, wgu[c], xn, H, N_gu, N_gu, nullptr, act, nullptr);
        if (mode == 1 || mode == 13) launch_oproj_resid(wo[c], attn, x, xp, 32, H, nullptr);
        if (mode == 1 || mode == 14) launch_gateup_norm(wgu[c], xp, nw, eps, act, N_gu, nullptr);
    };
    for (int i = 0; i < copies; ++i) go(i);
    HIPCHK(hipDeviceSynchronize());
    hipEvent_t e0, e1;
    hipEventCreate(&e0); hipEventCreate(&e1);
    hipEventRecord(e0, nullptr);
    for (int i = 0; i < iters; ++i) go(i);
    hipEventRecord(e1, nullptr);
    const hipError_t waited = hipEventSynchronize(e1);
    float ms = 0;
    if (waited == hipSuccess) hipEventElapsedTime(&ms, e0, e1);
    hipEventDestroy(e0); hipEventDestroy(e1);           // on the error path too
    HIPCHK(waited);
    *avg_us = ms * 1000.f / iters;
    HIPCHK(hipGetLastError());
    return MTTS_OK;
}

// pack2_rn (norm_ops.h: the hardware's fp32 -> bf16 conversion) against f2bf (common.h) on all 2^32 inputs:
// out2 = {inputs that are not NaN on which they differ, NaN inputs on which they differ}
int32_t mtts_k_bf16_round_check(int64_t* out2, void* stream) {
    if (!out2) return fail(MTTS_EINVAL, "bf16_round_check: null argument");
    hipStream_t st = S(stream);
    unsigned long long* cnt = nullptr;
    DevBufs hb;
    TRY(hb.get(&cnt, 2));
    launch_bf16_round_check(cnt, st);
    HIPCHK(hipGetLastError());
    unsigned long long h[2] = {0, 0};
    HIPCHK(hipMemcpyAsync(h, cnt, 16, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    out2[0] = (int64_t)h[0]; out2[1] = (int64_t)h[1];
    return MTTS_OK;
}

// describe() (stepplan.h) of the decode step the engine would run now at this KV page bound -- its current rows, run
// options and read policies -- as text into buf[cap], NUL-terminated; MTTS_EINVAL when it does not fit
int32_t mtts_debug_step_plan(MttsEngine* e, int32_t pages_bound, char* buf, int32_t cap) {
    if (!e || !buf || cap < 1 || pages_bound < 1) return fail(MTTS_EINVAL, "step_plan: bad argument");
    const std::string text = describe(decode_plan(e, pages_bound));
    if ((size_t)cap <= text.size()) return fail(MTTS_EINVAL, "step_plan: %d bytes needed, %d given", (int)text.size() + 1, cap);
    memcpy(buf, text.c_str(), text.size() + 1);
    return MTTS_OK;
}

// ---- sealed weight streams (gemm_sealed.hip) ----------------------------------------------------------------------------
int64_t mtts_debug_wseal_launches(void) { return (int64_t)mtts_wseal_launches(); }

// out12 = per kind (gate/up, down_proj, head 0, heads 1-7): {groups, groups not sealed, 1 if the decode GEMMs read the twin},
// as of the last mtts_weights_ready (which this call runs: MTTS_ESTATE from it when a tensor is missing)
int32_t mtts_debug_wseal_stats(MttsEngine* e, int64_t* out12) {
    if (!e || !out12) return fail(MTTS_EINVAL, "null argument");
    if (!e->d_wseal_cnt) return fail(MTTS_ESTATE, "the engine keeps no sealed weights (fp32 / fp16 engine, MTTS_W_SEAL=0 or MTTS_GEMM_DEPTH=0)");
    TRY(mtts_weights_ready(e));
    for (int k = 0; k < WSEAL_KINDS; ++k) {
        out12[3 * k] = (int64_t)e->h_wseal_cnt[2 * k];
        out12[3 * k + 1] = (int64_t)e->h_wseal_cnt[2 * k + 1];
        out12[3 * k + 2] = e->wseal_on[k];
    }
    return MTTS_OK;
}

// The bind-time sealer on a packed weight array of `ntiles` N-tiles: groups of ktw (16 or 12) k-tiles -> 13 or 10 units each.
int32_t mtts_k_wseal(const void* dev_packed, int32_t ntiles, int32_t K, int32_t ktw, void* dev_sealed, void* stream) {
    if (!dev_packed || !dev_sealed || ntiles < 1 || (ktw != 16 && ktw != 12) || K < 16 * ktw || K % (16 * ktw))
        return fail(MTTS_EINVAL, "wseal: need ktw 16 or 12 and K a multiple of 16 ktw");
    launch_wseal(dev_packed, dev_sealed, K, ktw, 0, ntiles, S(stream));
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(S(stream)));
    return MTTS_OK;
}

static int wseal_hook_plan(int epi, int N, int K, int ksplit, GemmPlan* p, int* Npad) {
    if (epi != EPI_PARTIAL && epi != EPI_BF16 && epi != EPI_SILU) return fail(MTTS_EINVAL, "gemm_sealed: epi 0 (partial), 1 (bf16) or 2 (SwiGLU)");
    if (N < 1 || K < 16 || K % 16 || ksplit < 1) return fail(MTTS_EINVAL, "gemm_sealed: bad shape");
    *Npad = round_up(N, 32);
    *p = mtts_plan_gemm_forced(*Npad, K, ksplit, 8);
    if (!wseal_shape(*p, K, *Npad, epi)) return fail(MTTS_EINVAL, "gemm_sealed: not a shape the sealed kernels take (8 waves of 16 k-tiles, or 12 with split-K; SwiGLU: N %% 96 == 0)");
    if (epi == EPI_SILU && N != *Npad) return fail(MTTS_EINVAL, "gemm_sealed: SwiGLU takes whole tiles");
    return MTTS_OK;
}

// One decode GEMM of 1 <= M <= 32 rows through the sealed kernel (sealed != 0; head_form as launch_gemm_sealed) or through
// launch_gemm on the same packed array (sealed == 0): W [N][K] and X [M][K] bf16 row-major.  dev_out receives the kernel's
// raw output, which starts as 0xa5 bytes: epi 0 fp32 [ksplit][32][Npad]; 1 bf16 [32][Npad] (columns >= N keep the sentinel);
// 2 bf16 32 * Npad / 2 in the X-fragment layout.  out2 = {groups, groups not sealed}.
int32_t mtts_k_gemm_sealed(const void* dev_w, const void* dev_x, void* dev_out, int32_t M, int32_t N, int32_t K, int32_t epi,
                           int32_t ksplit, int32_t sealed, int32_t head_form, int64_t* out2, void* stream) {
    if (!dev_w || !dev_x || !dev_out || M < 1 || M > 32) return fail(MTTS_EINVAL, "gemm_sealed: null argument or M outside 1..32");
    GemmPlan p;
    int Npad = 0;
    TRY(wseal_hook_plan(epi, N, K, ksplit, &p, &Npad));
    hipStream_t st = S(stream);
    DevBufs hb;
    uint16_t *wp = nullptr, *xp = nullptr, *out = nullptr;
    uint8_t* ws = nullptr;
    float* part = nullptr;
    unsigned long long* cnt = nullptr;
    const int ktw = p.kt_per_wave;
    TRY(hb.get(&wp, (size_t)Npad * K));
    TRY(hb.get(&ws, wseal_bytes(Npad, K, ktw)));
    TRY(hb.get(&xp, (size_t)32 * K));
    TRY(hb.get(&out, (size_t)32 * Npad, false));
    TRY(hb.get(&cnt, 2));
    if (epi == EPI_PARTIAL) {
        TRY(hb.get(&part, (size_t)ksplit * MTTS_PFCAP * Npad, false));
        HIPCHK(hipMemsetAsync(part, 0xa5, (size_t)ksplit * MTTS_PFCAP * Npad * 4, st));
    }
    HIPCHK(hipMemsetAsync(out, 0xa5, (size_t)32 * Npad * 2, st));
    launch_pack_weight(dev_w, wp, N, K, Npad, 1, 0, st);
    launch_wseal(wp, ws, K, ktw, 0, Npad / 32, st);
    launch_wseal_count(ws, Npad, K, ktw, cnt, st);
    launch_pack_rows(dev_x, xp, M, K, 1, st);
    if (sealed) {
        if (!launch_gemm_sealed(epi, 1, p, ws, wp, xp, K, Npad, N, part, out, head_form, st)) return fail(MTTS_EINVAL, "gemm_sealed: the sealed launch was refused");
    } else launch_gemm(epi, 1, p, wp, xp, K, Npad, N, part, out, st);
    HIPCHK(hipGetLastError());
    if (epi == EPI_PARTIAL) {
        for (int ks = 0; ks < ksplit; ++ks)
            HIPCHK(hipMemcpyAsync((float*)dev_out + (size_t)ks * 32 * Npad, part + (size_t)ks * MTTS_PFCAP * Npad, (size_t)32 * Npad * 4, hipMemcpyDeviceToDevice, st));
    } else HIPCHK(hipMemcpyAsync(dev_out, out, (size_t)32 * (epi == EPI_SILU ? Npad / 2 : Npad) * 2, hipMemcpyDeviceToDevice, st));
    unsigned long long h[2] = {0, 0};
    HIPCHK(hipMemcpyAsync(h, cnt, 16, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (out2) { out2[0] = (int64_t)h[0]; out2[1] = (int64_t)h[1]; }
    return MTTS_OK;
}

// Measurement hook: mtts_k_gemm_bench's launch train over `copies` packed copies of W [N][K] (dev_w null: every value
// 0x3c3c), sealed != 0 through the sealed kernel and its twins, else through launch_gemm on the bf16 arrays.
int32_t mtts_k_gemm_sealed_bench(const void* dev_w, int32_t N, int32_t K, int32_t epi, int32_t ksplit, int32_t copies, int32_t iters,
                                 int32_t sealed, int32_t head_form, float* avg_us, int64_t* out2) {
    if (copies < 1 || iters < 1 || !avg_us) return fail(MTTS_EINVAL, "gemm_sealed_bench: bad argument");
    GemmPlan p;
    int Npad = 0;
    TRY(wseal_hook_plan(epi, N, K, ksplit, &p, &Npad));
    DevBufs hb;
    const int ktw = p.kt_per_wave;
    std::vector<uint16_t*> w(copies, nullptr);
    std::vector<uint8_t*> ws(copies, nullptr);
    unsigned long long* cnt = nullptr;
    TRY(hb.get(&cnt, 2));
    for (int c = 0; c < copies; ++c) {
        TRY(hb.get(&w[c], (size_t)Npad * K));
        if (dev_w) launch_pack_weight(dev_w, w[c], N, K, Npad, 1, 0, nullptr);
        else HIPCHK(hipMemset(w[c], 0x3c, (size_t)Npad * K * 2));
        TRY(hb.get(&ws[c], wseal_bytes(Npad, K, ktw)));
        launch_wseal(w[c], ws[c], K, ktw, 0, Npad / 32, nullptr);
    }
    launch_wseal_count(ws[0], Npad, K, ktw, cnt, nullptr);
    uint16_t *x = nullptr, *out = nullptr;
    float* part = nullptr;
    TRY(hb.get(&x, (size_t)32 * K, false));
    HIPCHK(hipMemset(x, 0x3c, (size_t)32 * K * 2));
    TRY(hb.get(&out, (size_t)32 * Npad));
    if (epi == EPI_PARTIAL) TRY(hb.get(&part, (size_t)ksplit * MTTS_PFCAP * Npad));
    HIPCHK(hipGetLastError());
    bool refused = false;
    auto go = [&](int i) {
        if (!sealed) launch_gemm(epi, 1, p, w[i % copies], x, K, Npad, N, part, out, nullptr);
        else if (!launch_gemm_sealed(epi, 1, p, ws[i % copies], w[i % copies], x, K, Npad, N, part, out, head_form, nullptr)) refused = true;
    };
    for (int i = 0; i < copies; ++i) go(i);
    HIPCHK(hipDeviceSynchronize());
    if (refused) return fail(MTTS_EINVAL, "gemm_sealed_bench: the sealed launch was refused");
    hipEvent_t e0, e1;
    hipEventCreate(&e0); hipEventCreate(&e1);
    hipEventRecord(e0, nullptr);
    for (int i = 0; i < iters; ++i) go(i);
    hipEventRecord(e1, nullptr);
    HIPCHK(hipEventSynchronize(e1));
    float ms = 0;
    hipEventElapsedTime(&ms, e0, e1);
    *avg_us = ms * 1000.f / iters;
    hipEventDestroy(e0); hipEventDestroy(e1);
    unsigned long long h[2] = {0, 0};
    HIPCHK(hipMemcpy(h, cnt, 16, hipMemcpyDeviceToHost));
    if (out2) { out2[0] = (int64_t)h[0]; out2[1] = (int64_t)h[1]; }
    HIPCHK(hipGetLastError());
    return MTTS_OK;
}
