// Host side of libmtts.so: engine object, weight binding, KV page pool, the
// prefill / decode-step orchestration and the C ABI of include/mtts.h.
//
// Mirrors (file:line in /root/reference):
//   AsteroidTTSInstruct.forward inference branch   modeling_asteroid.py:337-380,411-426
//   AsteroidTTSInstruct.forward labels branch      modeling_asteroid.py:382-410 (mtts_score; kernels: score.hip)
//   AsteroidTTSModel._prepare_multi_modal_inputs    modeling_asteroid.py:235-250
//   CustomMixin._sample                             modeling_asteroid.py:83-169
// and, third-party, transformers Qwen3Model.forward (models/qwen3/modeling_qwen3.py).
#include "engine.h"
#include "staging.h"

#define FLUSH_STEPS 7          // a dialogue whose EOS falls within 7 steps of max_length still runs its delay-pattern flush (modeling_asteroid.py:165-168)
#define LINGER_STEPS 14        // static batch: a row finished BY max_length can be resurrected for a flush while another row's flush is still running (sampler.hip: update_kernel), so a batch runs up to 6 + 8 steps past max_length after ONE resurrection
// Resurrections chain: a resurrected row's own 7-step flush keeps the batch alive, and every step of it re-tests the other
// cut-off rows (modeling_asteroid.py:140-141,168), so each further row can add up to 6 more steps: 6 * B + 8 bounds the run.
// Storage (token rows, KV pages, RoPE rows) is sized for that bound where the engine's max_seq_len leaves room, and for
// LINGER_STEPS at least; a chain that outruns the room is reported (MTTS_ESTATE), never truncated silently.
static inline int linger_bound(int B) { return 6 * B + 8; }

thread_local char g_err[512] = "";
int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

const char* mtts_last_error(void) { return g_err; }
int32_t mtts_version(void) { return 202; }

// ---- KV page pool (kvpool.h) ---------------------------------------------------------------------------------------
// How the pool's table edits reach the device: as launch arguments of a one-wave kernel on the caller's stream, ordered
// with the steps around it, and no host buffer has to outlive the call
static auto ship_on(MttsEngine* e, hipStream_t st) {
    return [e, st](const PageEdits& ed) -> int {
        launch_set_pages(e->d_page_table, ed, st);
        HIPCHK(hipGetLastError());
        return 0;
    };
}

// ---- MTTS_DTYPE_F32 engine: allocation, binding, forward (kernels: f32path.hip) -------------------------------------
static int create_f32(MttsEngine* e) {
    const size_t H = e->H, I = e->I, D = MTTS_HD;
    e->lf.resize(e->L);
    for (auto& l : e->lf) {
        TRY(e->mem.get(&l.wqkv, (size_t)e->qkv_rows * H, false));
        TRY(e->mem.get(&l.wo, H * e->nq * D, false));
        TRY(e->mem.get(&l.wgu, 2 * I * H, false));
        TRY(e->mem.get(&l.wd, H * I, false));
        TRY(e->mem.get(&l.ln_in, H)); TRY(e->mem.get(&l.ln_post, H)); TRY(e->mem.get(&l.qn, D)); TRY(e->mem.get(&l.kn, D));
    }
    TRY(e->mem.get(&e->embf[0], (size_t)e->V0 * H, false));
    for (int ch = 1; ch < 8; ++ch) TRY(e->mem.get(&e->embf[ch], (size_t)e->Vs * H, false));
    TRY(e->mem.get(&e->final_norm_f, H));
    TRY(e->mem.get(&e->d_tables_f, 8));
    HIPCHK(hipMemcpy((void*)e->d_tables_f, e->embf, 8 * sizeof(void*), hipMemcpyHostToDevice));
    const size_t P = MTTS_PF32CAP;
    TRY(e->mem.get(&e->xf, P * H)); TRY(e->mem.get(&e->xnf, P * H)); TRY(e->mem.get(&e->yf, P * H));
    TRY(e->mem.get(&e->qkvf, P * e->qkv_rows)); TRY(e->mem.get(&e->qbuf_f, P * e->nq * D)); TRY(e->mem.get(&e->attnf, P * e->nq * D));
    TRY(e->mem.get(&e->guf, P * 2 * I)); TRY(e->mem.get(&e->actf, P * I));
    TRY(e->mem.get(&e->hlast_f, (size_t)MTTS_RCAP * H));
    TRY(e->mem.get((float**)&e->logits0, (size_t)MTTS_RCAP * e->V0_pad));
    TRY(e->mem.get((float**)&e->logits17, (size_t)MTTS_RCAP * 7 * e->Vs_pad));
    return 0;
}

static int forward_rows_f32(MttsEngine* e, const int32_t* d_tokens, const RowMeta* d_meta, int R, int heads, hipStream_t st) {
    const int H = e->H, I = e->I, nq = e->nq, nkv = e->nkv;
    const float eps = e->cfg.rms_norm_eps, scale = 1.0f / sqrtf((float)MTTS_HD);
    const int Lmax = e->max_pages * MTTS_PAGE, h16 = e->h16;
    const bool dec = heads == 1;                       // decode rows: GEMV in groups of 8 (batch-independent numerics)
    launch_f32_embed_norm(d_tokens, d_meta, e->d_tables_f, e->lf[0].ln_in, e->xf, e->xnf, R, H, eps, h16, st);
    for (int n = 0; n < e->L; ++n) {
        auto& l = e->lf[n];
        float* kc = e->kcache_f + e->layer_stride * n;
        float* vc = e->vcache_f + e->layer_stride * n;
        launch_f32_linear(l.wqkv, e->xnf, e->qkvf, R, e->qkv_rows, H, e->qkv_rows, h16, dec, st);
        launch_f32_qkv_post(e->qkvf, e->qkv_rows, d_meta, l.qn, l.kn, e->bufs.rope_cos_f, e->bufs.rope_sin_f, e->qbuf_f, kc, vc,
                            e->d_page_table, e->max_pages, e->total_pages, R, nq, nkv, eps, h16, st);
        launch_f32_attn(e->qbuf_f, kc, vc, e->d_page_table, d_meta, e->scores_f, e->attnf, R, e->max_pages, e->total_pages, nq,
                        nkv, scale, Lmax, h16, st);
        launch_f32_linear(l.wo, e->attnf, e->yf, R, H, nq * MTTS_HD, H, h16, dec, st);
        launch_f32_resid_norm(e->yf, e->xf, l.ln_post, e->xnf, nullptr, d_meta, R, H, eps, h16, st);
        launch_f32_linear(l.wgu, e->xnf, e->guf, R, 2 * I, H, 2 * I, h16, dec, st);
        launch_f32_swiglu(e->guf, e->actf, R, I, h16, st);
        launch_f32_linear(l.wd, e->actf, e->yf, R, H, I, H, h16, dec, st);
        const bool lastl = n == e->L - 1;
        launch_f32_resid_norm(e->yf, e->xf, lastl ? e->final_norm_f : e->lf[n + 1].ln_in, e->xnf, lastl ? e->hlast_f : nullptr,
                              d_meta, R, H, eps, h16, st);
    }
    if (heads) {
        // decode rows are the dialogues themselves (row b = slot b); after a prefill the last tokens' states are in hlast
        const float* xin = heads == 1 ? e->xnf : e->hlast_f;
        launch_f32_linear(e->embf[0], xin, (float*)e->logits0, e->B, e->V0, H, e->V0_pad, h16, true, st);
        for (int c = 1; c < 8; ++c)
            launch_f32_linear(e->embf[c], xin, (float*)e->logits17 + (size_t)(c - 1) * e->Vs_pad, e->B, e->Vs, H, 7 * e->Vs_pad, h16, true, st);
    }
    HIPCHK(hipGetLastError());
    return MTTS_OK;
}

// the small-batch kernels' LDS holds this model's rows (StepCaps.small_fits)
static bool small_path_fits(MttsEngine* e) {
    const int H = e->H;
    if (H > 8192 || H % 8 || e->I % 8) return false;
    const int lim = 64 * 1024 - 33 * 1024;            // default dynamic-LDS budget next to the kernel's static 32.1 KiB
    return mtts_small_lds_bytes(e->p_qkv, H, PRO_NORM) <= lim && mtts_small_lds_bytes(e->p_d, e->I, PRO_ROWS) <= lim &&
           mtts_small_lds_bytes(e->p_o, e->nq * MTTS_HD, PRO_COMBINE) <= lim;
}

int32_t mtts_engine_create(const MttsConfig* c, int32_t device, MttsEngine** out) {
    if (!c || !out) return fail(MTTS_EINVAL, "null argument");
    if (c->head_dim != MTTS_HD) return fail(MTTS_EINVAL, "head_dim must be 128 (got %d)", c->head_dim);
    if (c->channels != 8) return fail(MTTS_EINVAL, "channels must be 8");
    if (c->hidden_size % 16 || c->intermediate_size % 16) return fail(MTTS_EINVAL, "hidden/intermediate must be multiples of 16");
    if (c->hidden_size > 8192) return fail(MTTS_EINVAL, "hidden_size > 8192 not built (resid_norm keeps a row in registers)");
    if (c->num_attention_heads % c->num_key_value_heads) return fail(MTTS_EINVAL, "bad GQA ratio");
    int G = c->num_attention_heads / c->num_key_value_heads;
    if (G != 1 && G != 2 && G != 4) return fail(MTTS_EINVAL, "GQA group %d not built (1,2,4)", G);
    if (c->max_batch < 1 || c->max_batch > MTTS_RCAP) return fail(MTTS_EINVAL, "max_batch must be 1..128");
    if (c->vocab_size <= 152694 || c->speech_vocab_size <= 1024)
        return fail(MTTS_EINVAL, "vocab too small for the reference's hard-coded mask ids 152694 / 1024");
    if (c->dtype != MTTS_DTYPE_BF16 && c->dtype != MTTS_DTYPE_F32 && c->dtype != MTTS_DTYPE_F16)
        return fail(MTTS_EINVAL, "dtype %d not built (bf16 = 0, fp32 = 1, fp16 = 2)", c->dtype);
    if (c->kv_pool_pages < 0) return fail(MTTS_EINVAL, "kv_pool_pages must be >= 0");
    HIPCHK(hipSetDevice(device));
    // a failure from here on destroys the half-built engine; the message stays that of the failure
    struct Destroy {
        void operator()(MttsEngine* p) const {
            const std::string keep = g_err;
            mtts_engine_destroy(p);
            snprintf(g_err, sizeof(g_err), "%s", keep.c_str());
        }
    };
    std::unique_ptr<MttsEngine, Destroy> holder(new MttsEngine());
    MttsEngine* e = holder.get();
    DevBufs& m = e->mem;
    e->cfg = *c;
    e->device = device;
    StepKnobs& kn = e->knobs;
    StepCaps& caps = e->caps;
    kn = step_knobs_from_env();
    HIPCHK(hipDeviceGetAttribute(&caps.n_cus, hipDeviceAttributeMultiprocessorCount, device));
    if (kn.attn_row && attn_row_prepare()) {       // auto goes on without the row kernel; asking for it outright is an error
        if (kn.attn_row == 2) return fail(MTTS_EINVAL, "attn_row_kernel: the dynamic LDS limit could not be raised");
        kn.attn_row = 0;
    }
    caps.row_lds_limit = kn.attn_row ? attn_row_lds_limit() : 0;
    e->H = c->hidden_size; e->I = c->intermediate_size; e->L = c->num_hidden_layers;
    e->nq = c->num_attention_heads; e->nkv = c->num_key_value_heads;
    e->V0 = c->vocab_size; e->Vs = c->speech_vocab_size;
    e->V0_pad = round_up(e->V0, 32); e->Vs_pad = round_up(e->Vs, 32);
    e->qkv_rows = (e->nq + 2 * e->nkv) * MTTS_HD;
    e->layers.resize(e->L);
    const int H = e->H, I = e->I;
    e->f32 = c->dtype != MTTS_DTYPE_BF16;
    e->h16 = c->dtype == MTTS_DTYPE_F16;
    if (e->f32) TRY(create_f32(e));
    // packed weights (zeroed: padding rows must be zero)
    if (!e->f32) {
        for (auto& l : e->layers) {
            TRY(m.get((uint16_t**)&l.wqkv, (size_t)e->qkv_rows * H));
            TRY(m.get((uint16_t**)&l.wo, (size_t)H * e->nq * MTTS_HD));
            TRY(m.get((uint16_t**)&l.wgu, (size_t)2 * I * H));
            TRY(m.get((uint16_t**)&l.wd, (size_t)round_up(H, 32) * I));
            TRY(m.get((uint16_t**)&l.ln_in, (size_t)H));
            TRY(m.get((uint16_t**)&l.ln_post, (size_t)H));
            TRY(m.get((uint16_t**)&l.qn, (size_t)MTTS_HD));
            TRY(m.get((uint16_t**)&l.kn, (size_t)MTTS_HD));
        }
        TRY(m.get((uint16_t**)&e->emb[0], (size_t)e->V0 * H, false));
        for (int ch = 1; ch < 8; ++ch) TRY(m.get((uint16_t**)&e->emb[ch], (size_t)e->Vs * H, false));
        TRY(m.get((uint16_t**)&e->head0, (size_t)e->V0_pad * H));
        TRY(m.get((uint16_t**)&e->heads17, (size_t)7 * e->Vs_pad * H));
        TRY(m.get((uint16_t**)&e->final_norm, (size_t)H));
        TRY(m.get(&e->d_tables, 8));
        HIPCHK(hipMemcpy((void*)e->d_tables, e->emb, 8 * sizeof(void*), hipMemcpyHostToDevice));
    }
    // plans
    e->p_qkv = mtts_plan_gemm(e->qkv_rows, H, 0);
    e->p_o = mtts_plan_gemm(round_up(H, 32), e->nq * MTTS_HD, 0);
    e->p_gu = mtts_plan_gemm(2 * I, H, 1);
    e->p_d = mtts_plan_gemm(round_up(H, 32), I, 0);
    e->p_h0 = mtts_plan_gemm(e->V0_pad, H, 1);
    e->p_h17 = mtts_plan_gemm(7 * e->Vs_pad, H, 1);
    for (GemmPlan* p : {&e->p_qkv, &e->p_o, &e->p_gu, &e->p_d, &e->p_h0, &e->p_h17}) p->depth = kn.gemm_depth;
    // sealed twins of gate/up, down_proj and the heads, where the decode plan is one the sealed kernels take (they are
    // depth-specialised kernels: MTTS_GEMM_DEPTH=0 switches them off as well)
    if (!e->f32 && kn.w_seal && kn.gemm_depth) {
        const int Hp = round_up(H, 32);
        const auto wanted = [&](int kind) { return kn.w_seal == 2 || WSEAL_MAX_UNSEALED[kind] >= 0.0; };
        if (wanted(WSEAL_GU) && wseal_shape(e->p_gu, H, 2 * I, EPI_SILU)) e->wseal_ktw[WSEAL_GU] = e->p_gu.kt_per_wave;
        if (wanted(WSEAL_DOWN) && wseal_shape(e->p_d, I, Hp, EPI_PARTIAL)) e->wseal_ktw[WSEAL_DOWN] = e->p_d.kt_per_wave;
        if (wanted(WSEAL_HEAD0) && wseal_shape(e->p_h0, H, e->V0_pad, EPI_BF16)) e->wseal_ktw[WSEAL_HEAD0] = e->p_h0.kt_per_wave;
        if (wanted(WSEAL_HEADS) && wseal_shape(e->p_h17, H, 7 * e->Vs_pad, EPI_BF16)) e->wseal_ktw[WSEAL_HEADS] = e->p_h17.kt_per_wave;
        for (auto& l : e->layers) {
            if (e->wseal_ktw[WSEAL_GU]) TRY(m.get((uint8_t**)&l.wgu_s, wseal_bytes(2 * I, H, e->wseal_ktw[WSEAL_GU])));
            if (e->wseal_ktw[WSEAL_DOWN]) TRY(m.get((uint8_t**)&l.wd_s, wseal_bytes(Hp, I, e->wseal_ktw[WSEAL_DOWN])));
        }
        if (e->wseal_ktw[WSEAL_HEAD0]) TRY(m.get((uint8_t**)&e->head0_s, wseal_bytes(e->V0_pad, H, e->wseal_ktw[WSEAL_HEAD0])));
        if (e->wseal_ktw[WSEAL_HEADS]) TRY(m.get((uint8_t**)&e->heads17_s, wseal_bytes(7 * e->Vs_pad, H, e->wseal_ktw[WSEAL_HEADS])));
        TRY(m.get(&e->d_wseal_cnt, (size_t)WSEAL_KINDS * 2));
        TRY(m.get_pinned(&e->h_wseal_cnt, (size_t)WSEAL_KINDS * 2));
        // the zeroed twins are the sealed form of the zeroed bf16 arrays (padding rows, a matrix not yet bound)
        e->wseal_dirty = true;
    }
    // what plan_step (stepplan.h) needs to know of this engine, fixed from here on
    {
        const int Hp = round_up(H, 32), QD = e->nq * MTTS_HD;
        caps.G = G; caps.nkv = e->nkv; caps.L = e->L; caps.f32 = e->f32;
        caps.small_fits = small_path_fits(e);
        caps.fold_shape = fold_norm_shape(e->p_o, QD, e->p_gu, H, 2 * I);
        for (int k = 0; k < WSEAL_KINDS; ++k) caps.wseal_kind[k] = e->wseal_ktw[k] != 0;
        caps.gemm_form[GEMM_QKV] = mtts_gemm_form(EPI_PARTIAL, 1, e->p_qkv, H, e->qkv_rows, e->qkv_rows);
        caps.gemm_form[GEMM_O] = mtts_gemm_form(EPI_PARTIAL, 1, e->p_o, QD, Hp, Hp);
        caps.gemm_form[GEMM_GU] = mtts_gemm_form(EPI_SILU, 1, e->p_gu, H, 2 * I, 2 * I);
        caps.gemm_form[GEMM_GU_SLAB] = mtts_gemm_form(EPI_PARTIAL, 1, e->p_gu, H, 2 * I, 2 * I);
        caps.gemm_form[GEMM_DOWN] = mtts_gemm_form(EPI_PARTIAL, 1, e->p_d, I, Hp, Hp);
        caps.gemm_form[GEMM_HEAD0] = mtts_gemm_form(EPI_BF16, 1, e->p_h0, H, e->V0_pad, e->V0);
        caps.gemm_form[GEMM_HEADS] = mtts_gemm_form(EPI_BF16, 1, e->p_h17, H, 7 * e->Vs_pad, 7 * e->Vs_pad);
    }
    // activations hold a whole prefill pass (MTTS_PFCAP rows); split-K slabs: up to 8 of [MTTS_PFCAP][Npad] fp32
    size_t pmax = (size_t)8 * std::max(e->qkv_rows, round_up(H, 32));
    if (!e->f32) {
        TRY(m.get(&e->bufs.partial, pmax * MTTS_PFCAP));
        TRY(m.get(&e->partial2, (size_t)8 * round_up(H, 32) * MTTS_PFCAP));
        TRY(m.get((uint16_t**)&e->x2, (size_t)MTTS_MAXR * H));
        TRY(m.get((uint16_t**)&e->act_rm, (size_t)MTTS_MAXR * I));
        TRY(m.get((uint16_t**)&e->x, (size_t)MTTS_PFCAP * H));
        TRY(m.get((uint16_t**)&e->xn, (size_t)MTTS_PFCAP * H));
        TRY(m.get((uint16_t**)&e->xres_p, (size_t)32 * H));
        TRY(m.get((uint16_t**)&e->xh, (size_t)MTTS_RCAP * H));
        TRY(m.get((uint16_t**)&e->hlast, (size_t)MTTS_RCAP * H));
        TRY(m.get((uint16_t**)&e->attn_p, (size_t)MTTS_PFCAP * e->nq * MTTS_HD));
        TRY(m.get((uint16_t**)&e->act_p, (size_t)MTTS_PFCAP * I));
        TRY(m.get((uint16_t**)&e->qbuf, (size_t)MTTS_PFCAP * e->nq * MTTS_HD));
        TRY(m.get((uint16_t**)&e->logits0, (size_t)MTTS_RCAP * e->V0_pad));        // channel-0 rows padded to 32 tokens
        TRY(m.get((uint16_t**)&e->logits17, (size_t)MTTS_RCAP * 7 * e->Vs_pad));
        TRY(m.get((uint16_t**)&e->join_logits0, (size_t)MTTS_MAXR * e->V0_pad));
        TRY(m.get((uint16_t**)&e->join_logits17, (size_t)MTTS_MAXR * 7 * e->Vs_pad));
    }
    // KV pool
    e->max_pages = pages_for(c->max_seq_len) + 1;
    e->total_pages = c->kv_pool_pages > 0 ? c->kv_pool_pages : e->max_pages * c->max_batch;
    e->nchunks_max = (e->max_pages + ATT_PB - 1) / ATT_PB;
    e->layer_stride = (size_t)e->total_pages * e->nkv * MTTS_PAGE * MTTS_HD;
    if (e->f32) {
        TRY(m.get(&e->kcache_f, e->layer_stride * e->L));
        TRY(m.get(&e->vcache_f, e->layer_stride * e->L));
        TRY(m.get(&e->scores_f, (size_t)MTTS_PF32CAP * e->nq * e->max_pages * MTTS_PAGE, false));
    } else {
        // Invariant: the pools are zeroed here and afterwards only ever hold values a kernel wrote (K / V rows, finite
        // unless the model's own activations are not).  attn_prefill_pv_kernel relies on it: it multiplies the tokens behind
        // a row's position by an exact 0 on the matrix cores, which hides any finite stale value but not a NaN or an inf
        // (tests/test_attn_prefill_gpu.py: test_stale_pages_behind_a_dialogues_end_reach_nothing).
        TRY(m.get((uint16_t**)&e->kcache, e->layer_stride * e->L));
        TRY(m.get((uint16_t**)&e->vcache, e->layer_stride * e->L));
        if (kn.kv_pack) {
            // the second pool is an optimisation: when the card cannot hold it beside everything else (a very large
            // kv_pool_pages), the engine runs on bf16 pages alone instead of failing
            e->pk_layer_stride = (size_t)e->total_pages * e->nkv * MTTS_PKU * 64 * 16;
            size_t free_b = 0, total_b = 0;
            const size_t need = 2 * e->pk_layer_stride * e->L;
            if (hipMemGetInfo(&free_b, &total_b) != hipSuccess || need + ((size_t)8 << 30) > free_b) {
                fprintf(stderr, "mtts: sealed KV pages off: %.1f GB needed, %.1f GB free (8 GB kept for the run)\n", need / 1e9, free_b / 1e9);
                kn.kv_pack = 0;
            }
        }
        if (kn.kv_pack) {
            TRY(m.get((uint8_t**)&e->kpack, e->pk_layer_stride * e->L));
            TRY(m.get((uint8_t**)&e->vpack, e->pk_layer_stride * e->L));
            TRY(m.get(&e->d_seal_cnt, (size_t)e->L * 4));
            TRY(m.get_pinned(&e->h_seal_cnt, (size_t)e->L * 4));
            e->pack_k_on.assign(e->L, 1);
            e->pack_v_on.assign(e->L, 1);
        }
    }
    TRY(m.get(&e->d_page_table, (size_t)c->max_batch * e->max_pages));
    e->slot_live.assign(c->max_batch, 0);
    const char* shuffle = getenv("MTTS_PAGE_SHUFFLE");      // test hook: page tables become arbitrary permutations
    const uint64_t shuffle_seed = shuffle ? (uint64_t)atoll(shuffle) : 0;
    e->pool.init(e->total_pages, e->max_pages, c->max_batch, c->max_seq_len, shuffle ? &shuffle_seed : nullptr);
    if (!e->f32) {
        TRY(m.get((uint16_t**)&e->scores, (size_t)MTTS_PFCAP * e->nq * e->max_pages * MTTS_PAGE));
        TRY(m.get(&e->stats, (size_t)MTTS_PFCAP * e->nq * e->max_pages * 2));
        TRY(m.get(&e->opart, (size_t)MTTS_PFCAP * e->nq * ((e->max_pages + ATT_PF - 1) / ATT_PF) * MTTS_HD));   // prefill chunking is the finer one
    }
    // state
    TRY(m.get(&e->d_seqs, MTTS_RCAP));
    TRY(m.get(&e->d_meta, MTTS_RCAP));
    TRY(m.get(&e->d_ls, 1));
    TRY(m.get_pinned(&e->h_ls, 1));
    TRY(m.get_pinned(&e->h_seqs, MTTS_RCAP));
    TRY(m.get(&e->d_decisions, MTTS_RCAP * 8));
    TRY(m.get(&e->d_cur, MTTS_RCAP * 8));
    TRY(m.get(&e->d_tf, MTTS_RCAP * 7 * 8));
    e->bm_words = (e->V0 + 31) / 32;
    TRY(m.get(&e->d_bitmaps, (size_t)MTTS_RCAP * 8 * e->bm_words));
    TRY(m.get(&e->d_scfg, 8));
    TRY(m.get(&e->d_floors, 8));
    TRY(m.get(&e->d_typical, 8));
    TRY(m.get(&e->d_bancfg, 8));
    TRY(alloc_scratch(m, e->sscr, c->max_batch, e->V0));
    *out = holder.release();
    return MTTS_OK;
}

int32_t mtts_engine_destroy(MttsEngine* e) {
    if (!e) return MTTS_OK;
    hipSetDevice(e->device);
    hipDeviceSynchronize();
    e->graphs.clear();
    if (e->cap_stream) hipStreamDestroy(e->cap_stream);
    for (int w = 0; w < PROF_N; ++w) for (auto& pr : e->ev[w]) { hipEventDestroy(pr.first); hipEventDestroy(pr.second); }
    e->mem.free_all();
    const std::string err = e->mem.free_error;
    delete e;
    return err.empty() ? MTTS_OK : fail(MTTS_EHIP, "mtts_engine_destroy: %s", err.c_str());
}

// ---- weight binding ---------------------------------------------------------------------------------------------
// Where a state-dict tensor goes.  The bf16 engine keeps vectors and embedding tables as plain copies and matrices in
// MFMA-fragment order (launch_pack_weight); the fp32 engine keeps plain row-major copies (q|k|v rows one after another,
// gate rows then up rows).
struct WeightSlot {
    int64_t rows = 0, cols = 0;      // expected shape; cols == 1: a vector, given as [n], [n,1] or [1,n]
    void* copy_to = nullptr;         // bf16: plain copy (vectors, embedding tables)
    void* pack_to = nullptr;         // bf16: packed matrix [rows_pad][cols], source row r at row_mul * r + row_off
    int rows_pad = 0, row_mul = 1, row_off = 0;
    float* f32_to = nullptr;         // fp32: plain copy, starting at row f32_row
    int64_t f32_row = 0;
    int* bound = nullptr;            // mask that records the binding; null: a name that is accepted and ignored
    int bit = 0;
    bool proj = false;               // one of a layer's seven projection matrices (what a LoRA adapter may target)
    int layer = -1, proj_idx = -1;   // ... and which: layer, 0..6 = q k v o gate up down (the adapter bank's order)
    void* seal_to = nullptr;         // bf16: the packed matrix's sealed twin (gemm_sealed.hip), re-made by every bind ...
    int seal_ktw = 0, seal_nt0 = 0, seal_nt = 0;     // ... for the N-tiles the source rows land in
};
// after a bind wrote w.pack_to: the same stream re-seals the tiles it touched; the counts are taken at mtts_weights_ready
static void reseal(MttsEngine* e, const WeightSlot& w, hipStream_t st) {
    if (!w.seal_to) return;
    launch_wseal(w.pack_to, w.seal_to, (int)w.cols, w.seal_ktw, w.seal_nt0, w.seal_nt, st);
    e->wseal_dirty = true;
}

static int resolve_weight(MttsEngine* e, const char* name_c, WeightSlot& w) {
    const std::string name(name_c);
    const int64_t H = e->H, I = e->I, D = MTTS_HD, Hp = round_up(e->H, 32), QD = e->nq * D, KD = e->nkv * D;
    int ch = -1;
    if (sscanf(name_c, "model.embedding_list.%d.weight", &ch) == 1 && name.size() > 7 && name.compare(name.size() - 7, 7, ".weight") == 0) {
        if (ch < 0 || ch > 7) return fail(MTTS_EINVAL, "bad channel in %s", name_c);
        w.rows = ch == 0 ? e->V0 : e->Vs; w.cols = H;
        w.copy_to = e->emb[ch]; w.f32_to = e->embf[ch];
        // the head is tied to the embedding (modeling_asteroid.py:315-317)
        w.pack_to = ch == 0 ? e->head0 : e->heads17;
        w.rows_pad = ch == 0 ? e->V0_pad : 7 * e->Vs_pad;
        w.row_off = ch == 0 ? 0 : (ch - 1) * e->Vs_pad;
        w.seal_to = ch == 0 ? e->head0_s : e->heads17_s;
        w.seal_ktw = e->wseal_ktw[ch == 0 ? WSEAL_HEAD0 : WSEAL_HEADS];
        w.seal_nt0 = w.row_off / 32; w.seal_nt = (ch == 0 ? e->V0_pad : e->Vs_pad) / 32;
        w.bound = &e->emb_bound; w.bit = 1 << ch;
        return MTTS_OK;
    }
    if (name == "model.language_model.norm.weight") {
        w.rows = H; w.cols = 1; w.copy_to = e->final_norm; w.f32_to = e->final_norm_f; w.bound = &e->norm_bound; w.bit = 1;
        return MTTS_OK;
    }
    if (name.find("lm_heads.") == 0 || name == "model.language_model.embed_tokens.weight") return MTTS_OK;  // tied / unused
    int n = -1;
    char rest[128];
    if (sscanf(name_c, "model.language_model.layers.%d.%127s", &n, rest) != 2) return fail(MTTS_EINVAL, "unknown tensor %s", name_c);
    if (n < 0 || n >= e->L) return fail(MTTS_EINVAL, "layer index out of range in %s", name_c);
    Layer& l = e->layers[n];
    const MttsEngine::LayerF32 f = e->f32 ? e->lf[n] : MttsEngine::LayerF32{};
    const struct { const char* name; int64_t rows, cols; void* bf; float* f32; int rows_pad, row_mul, row_off; int64_t f32_row; } t[] = {
        {"input_layernorm.weight", H, 1, l.ln_in, f.ln_in, 0, 1, 0, 0},
        {"post_attention_layernorm.weight", H, 1, l.ln_post, f.ln_post, 0, 1, 0, 0},
        {"self_attn.q_norm.weight", D, 1, l.qn, f.qn, 0, 1, 0, 0},
        {"self_attn.k_norm.weight", D, 1, l.kn, f.kn, 0, 1, 0, 0},
        {"self_attn.q_proj.weight", QD, H, l.wqkv, f.wqkv, e->qkv_rows, 1, 0, 0},
        {"self_attn.k_proj.weight", KD, H, l.wqkv, f.wqkv, e->qkv_rows, 1, (int)QD, QD},
        {"self_attn.v_proj.weight", KD, H, l.wqkv, f.wqkv, e->qkv_rows, 1, (int)(QD + KD), QD + KD},
        {"self_attn.o_proj.weight", H, QD, l.wo, f.wo, (int)Hp, 1, 0, 0},
        {"mlp.gate_proj.weight", I, H, l.wgu, f.wgu, (int)(2 * I), 2, 0, 0},
        {"mlp.up_proj.weight", I, H, l.wgu, f.wgu, (int)(2 * I), 2, 1, I},
        {"mlp.down_proj.weight", H, I, l.wd, f.wd, (int)Hp, 1, 0, 0},
    };
    for (int i = 0; i < 11; ++i)
        if (!strcmp(rest, t[i].name)) {
            w.rows = t[i].rows; w.cols = t[i].cols;
            (t[i].cols == 1 ? w.copy_to : w.pack_to) = t[i].bf;
            w.rows_pad = t[i].rows_pad; w.row_mul = t[i].row_mul; w.row_off = t[i].row_off;
            w.f32_to = t[i].f32; w.f32_row = t[i].f32_row;
            w.bound = &l.bound; w.bit = 1 << i;       // a complete layer has all 11 bits: 2047 (mtts_weights_ready)
            w.proj = t[i].cols != 1;
            w.layer = n; w.proj_idx = i - 4;
            if (t[i].bf == l.wgu) { w.seal_to = l.wgu_s; w.seal_ktw = e->wseal_ktw[WSEAL_GU]; }      // (gate and up rows interleave: every tile)
            if (t[i].bf == l.wd) { w.seal_to = l.wd_s; w.seal_ktw = e->wseal_ktw[WSEAL_DOWN]; }
            w.seal_nt0 = 0; w.seal_nt = w.rows_pad / 32;
            return MTTS_OK;
        }
    return fail(MTTS_EINVAL, "unknown tensor %s", name_c);
}

int32_t mtts_bind_weight(MttsEngine* e, const char* name_c, const void* src, int64_t rows, int64_t cols, void* stream) {
    if (!e || !name_c || !src) return fail(MTTS_EINVAL, "null argument");
    HIPCHK(hipSetDevice(e->device));
    hipStream_t st = S(stream);
    WeightSlot w;
    TRY(resolve_weight(e, name_c, w));
    if (!w.bound) return MTTS_OK;
    const bool shape_ok = w.cols == 1 ? (rows == w.rows && cols == 1) || (rows == 1 && cols == w.rows) : rows == w.rows && cols == w.cols;
    if (!shape_ok)
        return fail(MTTS_EINVAL, "%s: expected [%lld,%lld] got [%lld,%lld]", name_c, (long long)w.rows, (long long)w.cols, (long long)rows, (long long)cols);
    const size_t n = (size_t)w.rows * w.cols;
    if (e->f32) {
        HIPCHK(hipMemcpyAsync(w.f32_to + w.f32_row * w.cols, src, n * 4, hipMemcpyDeviceToDevice, st));
    } else {
        if (w.copy_to) HIPCHK(hipMemcpyAsync(w.copy_to, src, n * 2, hipMemcpyDeviceToDevice, st));
        if (w.pack_to) launch_pack_weight(src, w.pack_to, (int)w.rows, (int)w.cols, w.rows_pad, w.row_mul, w.row_off, st);
        reseal(e, w, st);
        HIPCHK(hipGetLastError());
    }
    *w.bound |= w.bit;
    return MTTS_OK;
}

// mtts_bind_weight with a LoRA adapter merged into the matrix on its way into the engine's layout (csrc/adapter.hip).
static int run_still_open(MttsEngine* e, bool* open);
int32_t mtts_bind_weight_lora(MttsEngine* e, const char* name_c, const void* base, int64_t rows, int64_t cols, const float* lora_a,
                              const float* lora_b, int32_t r, float scaling, void* stream) {
    if (!e || !name_c || !base || !lora_a || !lora_b) return fail(MTTS_EINVAL, "null argument");
    if (r < 1 || r > 256) return fail(MTTS_EINVAL, "%s: adapter rank %d outside 1..256", name_c, r);
    if (((uintptr_t)base | (uintptr_t)lora_a | (uintptr_t)lora_b) & 15) return fail(MTTS_EINVAL, "%s: tensors must be 16-byte aligned", name_c);
    HIPCHK(hipSetDevice(e->device));
    WeightSlot w;
    TRY(resolve_weight(e, name_c, w));
    if (!w.proj) return fail(MTTS_EINVAL, "%s is not a projection weight of a layer: an adapter cannot target it", name_c);
    if (rows != w.rows || cols != w.cols)
        return fail(MTTS_EINVAL, "%s: expected [%lld,%lld] got [%lld,%lld]", name_c, (long long)w.rows, (long long)w.cols, (long long)rows, (long long)cols);
    bool open = false;
    TRY(run_still_open(e, &open));
    if (open) return fail(MTTS_ESTATE, "weights cannot change while a run is open (the rule of mtts_set_output_scores)");
    hipStream_t st = S(stream);
    if (e->f32)
        launch_lora_rows_f32((const float*)base, lora_a, lora_b, r, scaling, w.f32_to + w.f32_row * w.cols, (int)w.rows, (int)w.cols,
                             e->h16 ? 1 : 0, st);
    else {
        launch_lora_pack(base, lora_a, lora_b, r, scaling, w.pack_to, (int)w.rows, (int)w.cols, w.row_mul, w.row_off, st);
        reseal(e, w, st);
    }
    HIPCHK(hipGetLastError());
    *w.bound |= w.bit;
    return MTTS_OK;
}

// ---- resident adapters, one per dialogue (kernels: multilora.hip) ---------------------------------------------------
// split-K slabs of a pass with adapters: one slab more than the 8 a GEMM may write, and gate/up's two slabs of 2 I columns
// (mtts_engine_create sizes the buffer for the 8 slabs of an engine without a bank)
static size_t bank_partial_elems(const MttsEngine* e) {
    const size_t lin = std::max(e->qkv_rows, round_up(e->H, 32));
    return std::max(9 * lin, (size_t)4 * e->I) * MTTS_PFCAP;
}
static int bank_check(MttsEngine* e, int adapter, const char* what) {
    if (e->f32) return fail(MTTS_EINVAL, "%s: resident adapters exist on the bf16 engine only (this one is %s); merge one with mtts_bind_weight_lora", what, e->h16 ? "fp16" : "fp32");
    if (adapter < 0 || adapter >= MTTS_MAX_ADAPTERS) return fail(MTTS_EINVAL, "%s: adapter index %d outside 0..%d", what, adapter, MTTS_MAX_ADAPTERS - 1);
    bool open = false;
    TRY(run_still_open(e, &open));
    if (open) return fail(MTTS_ESTATE, "%s: the adapter bank cannot change while a run is open (the rule of mtts_bind_weight_lora)", what);
    return MTTS_OK;
}
// an id a row or a slot may carry: -1, or an adapter that holds at least one pair
static int adapter_id_check(MttsEngine* e, int id, const char* what, int at) {
    if (id == -1) return MTTS_OK;
    if (id < -1 || id >= MTTS_MAX_ADAPTERS) return fail(MTTS_EINVAL, "%s %d: adapter id %d outside -1..%d", what, at, id, MTTS_MAX_ADAPTERS - 1);
    if (!e->bank_pairs[id]) return fail(MTTS_EINVAL, "%s %d: adapter %d is empty (mtts_adapter_load)", what, at, id);
    return MTTS_OK;
}
static int bank_upload(MttsEngine* e, size_t first, size_t n, hipStream_t st) {
    HIPCHK(hipMemcpyAsync(e->bufs.d_bank + first, e->bank.data() + first, n * sizeof(LoraEnt), hipMemcpyHostToDevice, st));
    HIPCHK(hipStreamSynchronize(st));
    return MTTS_OK;
}

int32_t mtts_adapter_load(MttsEngine* e, int32_t adapter, const char* name_c, const float* lora_a, const float* lora_b, int64_t rows,
                          int64_t cols, int32_t r, float scaling, void* stream) {
    if (!e || !name_c || !lora_a || !lora_b) return fail(MTTS_EINVAL, "null argument");
    HIPCHK(hipSetDevice(e->device));
    TRY(bank_check(e, adapter, "mtts_adapter_load"));
    if (r < 1 || r > MTTS_LORA_MAX_RANK) return fail(MTTS_EINVAL, "%s: adapter rank %d outside 1..%d", name_c, r, MTTS_LORA_MAX_RANK);
    if (((uintptr_t)lora_a | (uintptr_t)lora_b) & 15) return fail(MTTS_EINVAL, "%s: tensors must be 16-byte aligned", name_c);
    WeightSlot w;
    TRY(resolve_weight(e, name_c, w));
    if (!w.proj) return fail(MTTS_EINVAL, "%s is not a projection weight of a layer: an adapter cannot target it", name_c);
    if (rows != w.rows || cols != w.cols)
        return fail(MTTS_EINVAL, "%s: expected [%lld,%lld] got [%lld,%lld]", name_c, (long long)w.rows, (long long)w.cols, (long long)rows, (long long)cols);
    if (cols > LORA_MAX_K) return fail(MTTS_EINVAL, "%s: rows of %lld elements, the delta kernel stages at most %d", name_c, (long long)cols, LORA_MAX_K);
    hipStream_t st = S(stream);
    const size_t per = (size_t)e->L * 7;
    if (!e->bufs.d_bank) {           // the first load: the bank's tables, the per-slot ids, and room for the extra slabs
        HIPCHK(hipDeviceSynchronize());
        // all three or none: a failure gives back what it took and leaves the engine as it was, so the load can be retried
        float* wider = nullptr;
        int32_t* ids = nullptr;
        LoraEnt* tab = nullptr;
        int rc = e->mem.get(&wider, bank_partial_elems(e));
        if (!rc) rc = e->mem.get(&ids, MTTS_RCAP, false);
        if (!rc) rc = e->mem.get(&tab, MTTS_MAX_ADAPTERS * per);
        if (!rc && hipMemset(ids, 0xff, MTTS_RCAP * sizeof(int32_t)) != hipSuccess) rc = fail(MTTS_EHIP, "mtts_adapter_load: hipMemset of the per-slot adapter ids failed");
        if (rc) { e->mem.release(wider); e->mem.release(ids); e->mem.release(tab); return rc; }
        e->mem.release(e->bufs.partial);
        e->bufs.partial = wider;
        e->bufs.d_seq_adapter = ids;
        e->bank.assign(MTTS_MAX_ADAPTERS * per, LoraEnt{nullptr, nullptr, 0, 0.f});
        e->bufs.d_bank = tab;
    }
    float *a = nullptr, *b = nullptr;      // (no launch carries a pair's addresses: a step finds them through the table in bufs.d_bank)
    TRY(e->mem.get(&a, (size_t)r * cols, false));
    if (const int rc = e->mem.get(&b, (size_t)rows * r, false)) { e->mem.release(a); return rc; }
    if (hipMemcpyAsync(a, lora_a, (size_t)r * cols * 4, hipMemcpyDeviceToDevice, st) != hipSuccess ||
        hipMemcpyAsync(b, lora_b, (size_t)rows * r * 4, hipMemcpyDeviceToDevice, st) != hipSuccess) {
        e->mem.release(a); e->mem.release(b);
        return fail(MTTS_EHIP, "%s: copying the adapter matrices failed", name_c);
    }
    const size_t at = adapter * per + (size_t)w.layer * 7 + w.proj_idx;
    LoraEnt& ent = e->bank[at];
    if (ent.r) {                // replaced: nothing in flight reads the old pair (no run is open, the stream is drained below)
        HIPCHK(hipDeviceSynchronize());
        float *oa = const_cast<float*>(ent.A), *ob = const_cast<float*>(ent.B);
        e->mem.release(oa); e->mem.release(ob);
    } else e->bank_pairs[adapter]++;
    ent = LoraEnt{a, b, r, scaling};
    return bank_upload(e, at, 1, st);
}

int32_t mtts_adapter_clear(MttsEngine* e, int32_t adapter) {
    if (!e) return fail(MTTS_EINVAL, "null engine");
    HIPCHK(hipSetDevice(e->device));
    TRY(bank_check(e, adapter, "mtts_adapter_clear"));
    if (!e->bufs.d_bank || !e->bank_pairs[adapter]) return MTTS_OK;
    HIPCHK(hipDeviceSynchronize());
    const size_t per = (size_t)e->L * 7;
    for (size_t i = adapter * per; i < (adapter + 1) * per; ++i) {
        float *oa = const_cast<float*>(e->bank[i].A), *ob = const_cast<float*>(e->bank[i].B);
        e->mem.release(oa); e->mem.release(ob);
        e->bank[i] = LoraEnt{nullptr, nullptr, 0, 0.f};
    }
    e->bank_pairs[adapter] = 0;
    return bank_upload(e, adapter * per, per, nullptr);
}

int32_t mtts_set_row_adapters(MttsEngine* e, const int32_t* host_ids, int32_t n) {
    if (!e || (n > 0 && !host_ids) || n < 0 || n > MTTS_RCAP) return fail(MTTS_EINVAL, "set_row_adapters: bad argument");
    if (e->f32) return fail(MTTS_EINVAL, "mtts_set_row_adapters: resident adapters exist on the bf16 engine only (this one is %s)", e->h16 ? "fp16" : "fp32");
    e->pending.set_row_adapters(host_ids, n);
    return MTTS_OK;
}

int32_t mtts_set_slot_adapter(MttsEngine* e, int32_t slot, int32_t adapter) {
    if (!e) return fail(MTTS_EINVAL, "null engine");
    if (e->f32) return fail(MTTS_EINVAL, "mtts_set_slot_adapter: resident adapters exist on the bf16 engine only (this one is %s)", e->h16 ? "fp16" : "fp32");
    if (slot < 0 || slot >= MTTS_RCAP) return fail(MTTS_EINVAL, "set_slot_adapter: slot %d out of range", slot);
    if (adapter < -1 || adapter >= MTTS_MAX_ADAPTERS) return fail(MTTS_EINVAL, "set_slot_adapter: adapter id %d outside -1..%d", adapter, MTTS_MAX_ADAPTERS - 1);
    e->pending.set_slot_adapter(slot, adapter);
    return MTTS_OK;
}
// the adapter of the dialogue in `slot` from now on: the host's copy now, the device's on `st`
static int set_seq_adapter(MttsEngine* e, int slot, int id, hipStream_t st) {
    e->seq_adapter[slot] = id;
    if (e->bufs.d_seq_adapter) HIPCHK(hipMemcpyAsync(e->bufs.d_seq_adapter + slot, &e->seq_adapter[slot], sizeof(int32_t), hipMemcpyHostToDevice, st));
    return MTTS_OK;
}
template <typename T>
static int bind_rope_tables(MttsEngine* e, T*& c, T*& s, const void* cosb, const void* sinb, int rows, hipStream_t st) {
    e->mem.release(c);
    e->mem.release(s);
    TRY(e->mem.get(&c, (size_t)rows * 64, false));
    TRY(e->mem.get(&s, (size_t)rows * 64, false));
    HIPCHK(hipMemcpyAsync(c, cosb, (size_t)rows * 64 * sizeof(T), hipMemcpyDeviceToDevice, st));
    HIPCHK(hipMemcpyAsync(s, sinb, (size_t)rows * 64 * sizeof(T), hipMemcpyDeviceToDevice, st));
    e->bufs.rope_rows = rows;
    return MTTS_OK;
}
int32_t mtts_bind_rope(MttsEngine* e, const void* cosb, const void* sinb, int32_t rows, void* stream) {
    if (!e || !cosb || !sinb || rows < 1) return fail(MTTS_EINVAL, "bad rope table");
    HIPCHK(hipSetDevice(e->device));
    // fp32 engine: fp32 tables [rows][64], as Qwen3RotaryEmbedding leaves them before the cast to the model dtype
    if (e->f32) return bind_rope_tables(e, e->bufs.rope_cos_f, e->bufs.rope_sin_f, cosb, sinb, rows, S(stream));
    return bind_rope_tables(e, e->bufs.rope_cos, e->bufs.rope_sin, cosb, sinb, rows, S(stream));
}

// Sealed weight streams: after a bind, count every kind's groups and those that did not seal (from the twins' dictionary
// units; the binds' streams are drained first) and decide which kinds the decode GEMMs read sealed.  Nothing per step.
static int wseal_policy(MttsEngine* e) {
    if (!e->wseal_dirty || !e->d_wseal_cnt) return MTTS_OK;
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemsetAsync(e->d_wseal_cnt, 0, WSEAL_KINDS * 2 * sizeof(unsigned long long), nullptr));
    const int H = e->H, I = e->I, Hp = round_up(H, 32);
    for (auto& l : e->layers) {
        if (l.wgu_s) launch_wseal_count(l.wgu_s, 2 * I, H, e->wseal_ktw[WSEAL_GU], e->d_wseal_cnt + 2 * WSEAL_GU, nullptr);
        if (l.wd_s) launch_wseal_count(l.wd_s, Hp, I, e->wseal_ktw[WSEAL_DOWN], e->d_wseal_cnt + 2 * WSEAL_DOWN, nullptr);
    }
    if (e->head0_s) launch_wseal_count(e->head0_s, e->V0_pad, H, e->wseal_ktw[WSEAL_HEAD0], e->d_wseal_cnt + 2 * WSEAL_HEAD0, nullptr);
    if (e->heads17_s) launch_wseal_count(e->heads17_s, 7 * e->Vs_pad, H, e->wseal_ktw[WSEAL_HEADS], e->d_wseal_cnt + 2 * WSEAL_HEADS, nullptr);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(e->h_wseal_cnt, e->d_wseal_cnt, WSEAL_KINDS * 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, nullptr));
    HIPCHK(hipStreamSynchronize(nullptr));
    for (int k = 0; k < WSEAL_KINDS; ++k) {      // (a changed choice changes the steps' plans: their old graphs no longer match)
        const unsigned long long groups = e->h_wseal_cnt[2 * k], bad = e->h_wseal_cnt[2 * k + 1];
        e->wseal_on[k] = e->wseal_ktw[k] && groups && (e->knobs.w_seal == 2 || (double)bad <= WSEAL_MAX_UNSEALED[k] * (double)groups);
    }
    e->wseal_dirty = false;
    return MTTS_OK;
}

int32_t mtts_weights_ready(MttsEngine* e) {
    if (!e) return fail(MTTS_EINVAL, "null engine");
    if (e->emb_bound != 0xff) return fail(MTTS_ESTATE, "embedding tables missing (mask %x)", e->emb_bound);
    if (!e->norm_bound) return fail(MTTS_ESTATE, "final norm missing");
    if (!e->bufs.rope_rows) return fail(MTTS_ESTATE, "rope table missing");
    for (int n = 0; n < e->L; ++n)
        if (e->layers[n].bound != 2047) return fail(MTTS_ESTATE, "layer %d incomplete (mask %x)", n, e->layers[n].bound);
    return wseal_policy(e);
}

// ---- profiling helpers ------------------------------------------------------------
static void prof_begin(MttsEngine* e, int which, hipStream_t st, hipEvent_t* a) {
    if (!e->prof) return;
    hipEvent_t s0, s1;
    hipEventCreate(&s0); hipEventCreate(&s1);
    hipEventRecord(s0, st);
    e->ev[which].push_back({s0, s1});
    *a = s1;
}
static void prof_end(MttsEngine* e, hipStream_t st, hipEvent_t a) {
    if (!e->prof) return;
    hipEventRecord(a, st);
}

// a new run: sealed reads everywhere, counts from zero (steps whose plan this changes no longer match their old graphs)
static int pack_policy_reset(MttsEngine* e, hipStream_t st) {
    if (!e->d_seal_cnt) return 0;
    HIPCHK(hipMemsetAsync(e->d_seal_cnt, 0, (size_t)e->L * 4 * sizeof(unsigned long long), st));
    e->pack_k_on.assign(e->L, 1);
    e->pack_v_on.assign(e->L, 1);
    return 0;
}
// The attention section of layer n, after its qkv GEMM left `ks_qkv` slabs in `partial`, in the form the plan gives the
// layer: the whole section as one launch, or the q/k/v epilogue (a launch of its own, or fused into the attention kernels)
// and then scores, P.V and -- except on the small path, which leaves it to its o_proj prologue -- the combine.
static int attend_layer(MttsEngine* e, const StepPlan& plan, int n, const RowMeta* d_meta, int R, int pages_bound, int ks_qkv,
                        hipStream_t st, int64_t kv_tokens_hint) {
    static const AttnPhase decode_ph[3] = {ATTN_SCORES, ATTN_PV, ATTN_COMBINE}, prefill_ph[3] = {ATTN_PF_SCORES, ATTN_PF_PV, ATTN_PF_COMBINE};
    Layer& l = e->layers[n];
    const AttnForm form = plan.layers[n].attn;
    const float eps = e->cfg.rms_norm_eps, scale = 1.0f / sqrtf((float)MTTS_HD);
    uint16_t* kc = (uint16_t*)e->kcache + e->layer_stride * n;
    uint16_t* vc = (uint16_t*)e->vcache + e->layer_stride * n;
    const QkvFuse fz{e->bufs.partial, ks_qkv, e->qkv_rows, (const uint16_t*)l.qn, (const uint16_t*)l.kn, e->bufs.rope_cos, e->bufs.rope_sin, eps};
    const KvPack pk = layer_pack(e, plan, n);
    const KvPack* pkp = (pk.k || pk.v) ? &pk : nullptr;
    // one launch (the q/k/v epilogue is always inside), timed under the scores slot with the K + V bytes
    if (form == ATTN_FORM_ROW) {
        hipEvent_t ev = nullptr;
        prof_begin(e, PROF_SCORES, st, &ev);
        if (const int rc = launch_attn(e->qbuf, kc, vc, e->d_page_table, d_meta, e->scores, e->stats, e->opart, e->attn_p, R, pages_bound,
                                       e->max_pages, e->total_pages, e->nchunks_max, e->nq, e->nkv, scale, &fz, ATTN_ROW, st, pkp))
            return fail(MTTS_EINVAL, rc == -2 ? "the whole-row attention kernel does not take this launch" : "attention group size not built");
        prof_end(e, st, ev);
        if (e->prof) e->prof_bytes[PROF_SCORES] += 2 * kv_tokens_hint * e->nkv * MTTS_HD * 2;
        return 0;
    }
    const bool fused = form == ATTN_FORM_TWO_PASS_FUSED;
    const AttnPhase* ph = form == ATTN_FORM_PREFILL_MFMA ? prefill_ph : decode_ph;
    const int nphases = plan.path == PATH_SMALL ? 2 : 3;
    if (!fused)
        launch_qkv_post(e->bufs.partial, ks_qkv, e->qkv_rows, d_meta, l.qn, l.kn, e->bufs.rope_cos, e->bufs.rope_sin, e->qbuf,
                        kc, vc, e->d_page_table, e->max_pages, e->total_pages, R, e->nq, e->nkv, eps, st);
    for (int i = 0; i < nphases; ++i) {
        hipEvent_t ev = nullptr;
        if (i < 2) prof_begin(e, i == 0 ? PROF_SCORES : PROF_PV, st, &ev);
        if (launch_attn(e->qbuf, kc, vc, e->d_page_table, d_meta, e->scores, e->stats, e->opart, e->attn_p, R,
                        pages_bound, e->max_pages, e->total_pages, e->nchunks_max, e->nq, e->nkv, scale,
                        fused ? &fz : nullptr, ph[i], st, pkp))
            return fail(MTTS_EINVAL, "attention group size not built");
        if (i < 2) prof_end(e, st, ev);
    }
    if (e->prof) {   // algorithmic bytes: one K (or V) row of 128 bf16 per kv head per cached token
        e->prof_bytes[PROF_SCORES] += kv_tokens_hint * e->nkv * MTTS_HD * 2;
        e->prof_bytes[PROF_PV] += kv_tokens_hint * e->nkv * MTTS_HD * 2;
    }
    return 0;
}
// rows whose token completed a KV page: seal it (all layers)
static void seal_completed_pages(MttsEngine* e, const RowMeta* d_meta, int R, hipStream_t st) {
    if (e->kpack)
        launch_kv_seal_rows(e->kcache, e->vcache, e->kpack, e->vpack, e->d_page_table, d_meta, R, e->max_pages, e->total_pages, e->nkv, e->L, e->d_seal_cnt, st);
}

// ---- decode step for 1..SMALL_RP dialogues: six launches per layer instead of nine ---------------------------------
// qkv GEMM [prologue: residual + slabs + input norm] -> scores -> P.V -> o_proj [prologue: chunk sum] ->
// gate/up + SwiGLU [prologue: residual + slabs + post-attention norm] -> down_proj; the heads take the final norm as
// their prologue.  The residual stream alternates between two buffers (a prologue's block (0,0) writes x' while the
// other blocks still read x); the qkv slabs live in `partial` (the fused attention epilogue reads them), the o_proj /
// down_proj slabs in `partial2`.  Same arithmetic as forward_rows, operation for operation.
static int forward_small(MttsEngine* e, const StepPlan& plan, const RowMeta* d_meta, int pages_bound, hipStream_t st, int64_t kv_tokens_hint) {
    const int H = e->H, I = e->I, nq = e->nq, Hp = round_up(H, 32), R = MTTS_MAXR;
    const float eps = e->cfg.rms_norm_eps;
    uint16_t* xa = (uint16_t*)e->x;                    // embed_norm has left the embedding sum here
    uint16_t* xb = (uint16_t*)e->x2;
    SmallPro base{};
    base.rows = plan.B; base.eps = eps; base.slab_npad = Hp;
    for (int n = 0; n < e->L; ++n) {
        Layer& l = e->layers[n];
        SmallPro pq = base;                            // input norm (+ the previous layer's down_proj slabs)
        pq.x_in = xa; pq.x_out = xb; pq.slabs = e->partial2; pq.ksplit = n ? e->p_d.ksplit : 0; pq.norm_w = (const uint16_t*)l.ln_in;
        launch_gemv_small(EPI_PARTIAL, PRO_NORM, e->p_qkv, l.wqkv, H, e->qkv_rows, e->qkv_rows, e->bufs.partial, nullptr, pq, st);
        TRY(attend_layer(e, plan, n, d_meta, R, pages_bound, e->p_qkv.ksplit, st, kv_tokens_hint));
        SmallPro po = base;                            // o_proj: the chunk partials of P.V are summed in its prologue
        po.opart = e->opart; po.meta = d_meta; po.nchunks_max = e->nchunks_max; po.nq = nq; po.pages_per_chunk = ATT_PB;
        launch_gemv_small(EPI_PARTIAL, PRO_COMBINE, e->p_o, l.wo, nq * MTTS_HD, Hp, Hp, e->partial2, nullptr, po, st);
        SmallPro pg = base;                            // post-attention norm (+ the o_proj slabs)
        pg.x_in = xb; pg.x_out = xa; pg.slabs = e->partial2; pg.ksplit = e->p_o.ksplit; pg.norm_w = (const uint16_t*)l.ln_post;
        launch_gemv_small(EPI_SILU_RM, PRO_NORM, e->p_gu, l.wgu, H, 2 * I, 2 * I, nullptr, (uint16_t*)e->act_rm, pg, st);
        SmallPro pd = base;
        pd.xrows = (const uint16_t*)e->act_rm;
        launch_gemv_small(EPI_PARTIAL, PRO_ROWS, e->p_d, l.wd, I, Hp, Hp, e->partial2, nullptr, pd, st);
    }
    seal_completed_pages(e, d_meta, R, st);
    SmallPro ph = base;                                // final norm (+ the last down_proj slabs) in front of the 8 heads
    ph.x_in = xa; ph.x_out = nullptr; ph.slabs = e->partial2; ph.ksplit = e->p_d.ksplit; ph.norm_w = (const uint16_t*)e->final_norm;
    // (same plan as the general path: a different K partition over the waves would change the fp32 sums, and with them
    //  the bit-identity of a dialogue's logits across batch sizes; 4 waves would be 1 % faster at B=1)
    launch_gemv_small(EPI_BF16, PRO_NORM, e->p_h0, e->head0, H, e->V0_pad, e->V0, nullptr, (uint16_t*)e->logits0, ph, st);
    launch_gemv_small(EPI_BF16, PRO_NORM, e->p_h17, e->heads17, H, 7 * e->Vs_pad, 7 * e->Vs_pad, nullptr, (uint16_t*)e->logits17, ph, st);
    HIPCHK(hipGetLastError());
    return MTTS_OK;
}

// One GEMM of forward_rows on `tiles` activation row tiles, by the plan's choice for it: the tiled kernel with `ks`
// k-splits (prefill passes), the sealed twin `Ws`, or launch_gemm, which picks among its kernels by the shape.  A sealed
// launch that the launcher refuses is an error, never a silent bf16 launch.  It cannot happen today: plan_step asks only
// at one row tile without adapters and for a kind whose policy is on; wseal_on[k] implies wseal_ktw[k] (wseal_policy),
// which implies a twin, wseal_shape of this very GemmPlan and gemm_depth (mtts_engine_create) -- all the launcher checks.
static int run_gemm(int epi, bool tiled, int R, int ks, bool sealed, int head_form, const GemmPlan& p, const void* Ws, const void* Wp,
                    const void* Xp, int K, int Npad, int n_valid, float* partial, uint16_t* out, hipStream_t st) {
    const int mb = (R + 31) / 32;
    if (tiled) launch_gemm_tile(epi, R, ks, Wp, Xp, K, Npad, n_valid, partial, out, st);
    else if (!sealed) launch_gemm(epi, mb, p, Wp, Xp, K, Npad, n_valid, partial, out, st);
    else if (!launch_gemm_sealed(epi, mb, p, Ws, Wp, Xp, K, Npad, n_valid, partial, out, head_form, st))
        return fail(MTTS_ESTATE, "the plan asks for a sealed weight read that the launcher does not take (K %d, N %d, %d row tiles)", K, Npad, mb);
    return 0;
}

// ---- one forward pass: plan.R rows = decode rows (<= MTTS_RCAP, one dialogue each) or a prefill pass (<= MTTS_PFCAP) ----
// plan.heads: 0 none, 1 from xn (rows are sequences: decode), 2 from hlast (end of prefill)
// plan.lora: a row of the pass has an adapter (mtts_set_row_adapters / mtts_set_slot_adapter).  The GEMMs, norms and attention
// kernels are then the same launches with the same arguments, except that after the qkv, o_proj and down_proj GEMMs the
// adapters' delta goes into the slab behind the GEMM's last one and the consumer sums one slab more, and that gate/up
// writes a slab instead of running its SwiGLU epilogue (delta into slab 1, swiglu_slabs_kernel on the sum).
// Which launches: plan_step (stepplan.h).  Nothing below decides.
static int forward_rows(MttsEngine* e, const StepPlan& plan, const int32_t* d_tokens, const RowMeta* d_meta, int pages_bound,
                        hipStream_t st, int64_t kv_tokens_hint) {
    const int H = e->H, I = e->I, nq = e->nq, nkv = e->nkv, R = plan.R, mb = plan.mb;
    const float eps = e->cfg.rms_norm_eps;
    const int Hp = round_up(H, 32);
    const bool tiled = plan.tiled, lora = plan.lora;
    if (plan.path == PATH_F32) return forward_rows_f32(e, d_tokens, d_meta, plan.heads == 1 ? plan.B : R, plan.heads, st);
    launch_embed_norm(d_tokens, d_meta, e->d_tables, e->layers[0].ln_in, e->x, e->xn, R, H, eps, st);
    if (plan.path == PATH_SMALL) return forward_small(e, plan, d_meta, pages_bound, st, kv_tokens_hint);
    if (lora && !e->bufs.d_bank) return fail(MTTS_ESTATE, "a pass with adapters on an engine without a bank");
    const int QD = nq * MTTS_HD, KD = nkv * MTTS_HD, EL = e->L * 7;
    const LoraJob j_qkv{3, e->qkv_rows, H, EL, {{0, QD, 1, 0}, {QD, KD, 1, 1}, {QD + KD, KD, 1, 2}}};
    const LoraJob j_o{1, Hp, QD, EL, {{0, H, 1, 3}}}, j_gu{2, 2 * I, H, EL, {{0, I, 2, 4}, {1, I, 2, 5}}}, j_d{1, Hp, I, EL, {{0, H, 1, 6}}};
    // prefill passes take the tiled GEMM with a split-K that depends on the shape only (chosen for a 1024-row pass: good
    // from one dialogue's prompt up to a full pass): a prompt's hidden states then do not depend on how many rows (other
    // dialogues) share its pass
    const int ks_qkv = tiled ? mtts_tile_ksplit(e->qkv_rows, H, 1024) : e->p_qkv.ksplit;
    const int ks_o = tiled ? mtts_tile_ksplit(Hp, QD, 1024) : e->p_o.ksplit;
    const int ks_d = tiled ? mtts_tile_ksplit(Hp, I, 1024) : e->p_d.ksplit;
    const int ex = lora ? 1 : 0;                     // slabs the consumers sum beyond the GEMM's
    // gate/up: the same plan with or without adapters (p_gu; one k-split of the tile GEMM), so slab 0 holds the sums
    // the fused epilogue would have rounded
    const int gu_epi = lora ? EPI_PARTIAL : EPI_SILU;
    float* gu_slab = lora ? e->bufs.partial : nullptr;
    for (int n = 0; n < e->L; ++n) {
        Layer& l = e->layers[n];
        // the adapters' delta of this layer's matrices in `job`, for the rows in `xp`, into slab `ks` of the partial buffer
        auto delta = [&](const LoraJob& job, const void* xp, int ks) {
            launch_lora_delta(xp, d_meta, e->bufs.d_seq_adapter, e->bufs.d_bank + (size_t)n * 7, job, e->bufs.partial + (size_t)ks * MTTS_PFCAP * job.Npad, R, st);
        };
        TRY(run_gemm(EPI_PARTIAL, tiled, R, ks_qkv, false, 0, e->p_qkv, nullptr, l.wqkv, e->xn, H, e->qkv_rows, e->qkv_rows, e->bufs.partial, nullptr, st));
        if (lora) delta(j_qkv, e->xn, ks_qkv);
        TRY(attend_layer(e, plan, n, d_meta, R, pages_bound, ks_qkv + ex, st, kv_tokens_hint));
        if (plan.fold) {
            // o_proj leaves no slabs: it finishes x' (rows < R), gate/up normalises it.  Both buffers hold a whole tile; rows >= R
            // of xres_p keep zeros or the x' of an earlier, larger batch (finite), which gate/up normalises and multiplies like the
            // stale xn rows of the three launches: nothing reads the result rows >= R
            launch_oproj_resid(l.wo, e->attn_p, e->x, e->xres_p, R, Hp, st);
            launch_gateup_norm(l.wgu, e->xres_p, l.ln_post, eps, e->act_p, 2 * I, st);
        } else {
            TRY(run_gemm(EPI_PARTIAL, tiled, R, ks_o, false, 0, e->p_o, nullptr, l.wo, e->attn_p, QD, Hp, Hp, e->bufs.partial, nullptr, st));
            if (lora) delta(j_o, e->attn_p, ks_o);
            launch_resid_norm(e->bufs.partial, ks_o + ex, Hp, e->x, l.ln_post, e->xn, nullptr, d_meta, R, H, eps, st);
            TRY(run_gemm(gu_epi, tiled, R, 1, plan.sealed[WSEAL_GU], 0, e->p_gu, l.wgu_s, l.wgu, e->xn, H, 2 * I, 2 * I, gu_slab, (uint16_t*)e->act_p, st));
        }
        if (lora) {
            delta(j_gu, e->xn, 1);
            launch_swiglu_slabs(e->bufs.partial, e->bufs.partial + (size_t)MTTS_PFCAP * 2 * I, e->act_p, mb * 32, I, st);
        }
        TRY(run_gemm(EPI_PARTIAL, tiled, R, ks_d, plan.sealed[WSEAL_DOWN], 0, e->p_d, l.wd_s, l.wd, e->act_p, I, Hp, Hp, e->bufs.partial, nullptr, st));
        if (lora) delta(j_d, e->act_p, ks_d);
        const bool lastl = (n == e->L - 1);
        const void* nw = lastl ? e->final_norm : e->layers[n + 1].ln_in;
        launch_resid_norm(e->bufs.partial, ks_d + ex, Hp, e->x, nw, e->xn, lastl ? e->hlast : nullptr, d_meta, R, H, eps, st);
    }
    seal_completed_pages(e, d_meta, R, st);
    if (plan.heads) {
        const void* xin = e->xn;
        if (plan.heads == 2) {                         // the dialogues' last rows, packed into tiles of their own
            launch_pack_rows(e->hlast, e->xh, plan.B, H, plan.hmb, st);
            xin = e->xh;
        }
        const int hr = plan.hmb * 32, form = plan.head_persistent ? 1 : 0;
        TRY(run_gemm(EPI_BF16, false, hr, 0, plan.sealed[WSEAL_HEAD0], form, e->p_h0, e->head0_s, e->head0, xin, H, e->V0_pad, e->V0, nullptr, (uint16_t*)e->logits0, st));
        TRY(run_gemm(EPI_BF16, false, hr, 0, plan.sealed[WSEAL_HEADS], form, e->p_h17, e->heads17_s, e->heads17, xin, H, 7 * e->Vs_pad, 7 * e->Vs_pad, nullptr, (uint16_t*)e->logits17, st));
    }
    HIPCHK(hipGetLastError());
    return MTTS_OK;
}
// a pass that is not a decode step: R staged rows, heads 0 or 2
static int forward_staged(MttsEngine* e, const int32_t* d_tokens, const RowMeta* d_meta, int R, int pages_bound, int heads, bool lora, hipStream_t st) {
    return forward_rows(e, plan_step(e->knobs, e->caps, step_state(e, heads, R, pages_bound, lora)), d_tokens, d_meta, pages_bound, st, 0);
}

// prefill of the first `Mpad` staged rows in passes of up to MTTS_PFCAP (a multiple of MTTS_RCAP each); K/V of a pass are
// written before its attention runs.  `last_heads`: the heads argument of the last pass.
static int prefill_staged(MttsEngine* e, size_t Mpad, int pages_bound, int last_heads, bool lora, hipStream_t st) {
    const size_t pfcap = e->f32 ? MTTS_PF32CAP : MTTS_PFCAP;
    for (size_t off = 0; off < Mpad; off += pfcap) {
        const int rows = (int)std::min<size_t>(pfcap, Mpad - off);
        TRY(forward_staged(e, e->d_pf_tokens + off * 8, e->d_pf_meta + off, rows, pages_bound, off + rows >= Mpad ? last_heads : 0, lora, st));
    }
    return 0;
}

// The per-slot stores of the run that starts now, [slot][gen_cap][width] each (e->scores_on and e->topk_on are the run's):
// generated tokens, decision log and forced rows always; output_scores and top_logprobs only once a run asked for them,
// with the sampler's scratch for them.  A store that exists has the shape (bufs.gen_cap, bufs.gt_stride): when either changes,
// what it shapes is released here and comes back when next wanted.  The optional ones start every run as NaN / -1 (0xff
// bytes) in every slot, filled on `st` in the order below.
static int start_outputs(MttsEngine* e, int steps, hipStream_t st) {
    StepBufs& b = e->bufs;
    DevBufs& m = e->mem;
    const int k = e->topk_on, rows = e->cfg.max_batch;
    const bool scores = e->scores_on != 0, grown = steps > b.gen_cap, restrided = k && k != b.gt_stride;
    if (grown) b.gen_cap = steps;
    if (restrided) b.gt_stride = k;
    if (scores && !b.sscr_lp) {
        TRY(m.get(&b.sscr_slice_sum, (size_t)rows * SAMP_NS));
        TRY(m.get(&b.sscr_lp, (size_t)rows * 8));
    }
    if (k > b.gt_scr_cap) {
        m.release(b.gt_cand); m.release(b.gt_smax); m.release(b.gt_ssum);
        b.gt_scr_cap = 0;
        TRY(m.get(&b.gt_cand, (size_t)rows * SAMP_NS * k));
        TRY(m.get(&b.gt_smax, (size_t)rows * SAMP_NS));
        TRY(m.get(&b.gt_ssum, (size_t)rows * SAMP_NS));
        b.gt_scr_cap = k;
    }
    // one row per store: inner width 8 or 8 k, wanted by this run, zeroed when allocated, 0xff-filled when the run starts
    const auto store = [&](auto*& p, bool per_k, bool wanted, bool zeroed, bool filled) -> int {
        const size_t n = (size_t)rows * b.gen_cap * 8 * (per_k ? k : 1);
        if (grown || (per_k && restrided)) m.release(p);
        if (wanted && !p) TRY(m.get(&p, n, zeroed));
        if (wanted && filled) HIPCHK(hipMemsetAsync(p, 0xff, n * sizeof(*p), st));
        return 0;
    };
    TRY(store(b.d_gen, false, true, true, false));
    TRY(store(b.d_declog, false, true, true, false));
    TRY(store(b.d_forced, false, true, false, false));
    TRY(store(b.d_lp, false, scores, false, true));
    TRY(store(b.d_gt_logp, false, k > 0, false, true));
    TRY(store(b.d_gt_ids, true, k > 0, false, true));
    TRY(store(b.d_gt_tlp, true, k > 0, false, true));
    return 0;
}

// The hard bans of the run that starts now (mtts_set_sampler_bans): the per-channel settings and static bitmaps go up, and
// the buffers the ban kernel works on appear with the first run that asks -- the ban words and static bitmaps with any
// ban, the prompt history with an n-gram ban.  They are members of bufs and keep their size, so nothing is released here.
// A run without bans touches and allocates nothing.  Returns with `st` drained when it copied.
// The same for mtts_set_sampler_bias, which shares the ban path: a -inf rule, min_length or begin_suppress_tokens turn it on
// (min_length travels in BanCfg, the begin list in a second static bitmap), a rule longer than one token needs the prompt
// history.  The flattened rules appear with the first run that has a rule; the bias words, their static part and the
// tables with the first that has a finite one.
static int start_bans(MttsEngine* e, const RunBans& bans, const RunBias& bias, hipStream_t st) {
    StepBufs& b = e->bufs;
    e->bans_on = (bans.any() || bias.bans()) ? 1 : 0;
    e->ban_ngram_on = bans.ngram() ? 1 : 0;
    e->ban_begin_on = bias.begin() ? 1 : 0;
    e->bias_on = bias.rules() ? 1 : 0;
    e->bias_terms = bias.finite() ? 1 : 0;
    e->hist_on = (e->ban_ngram_on || bias.history()) ? 1 : 0;
    if (!e->bans_on && !e->bias_on) return 0;
    const int rows = e->cfg.max_batch, words = e->bm_words;
    if (e->bans_on && !b.d_ban) {
        TRY(e->mem.get(&b.d_ban, (size_t)rows * 8 * words));
        TRY(e->mem.get(&b.d_ban_static, (size_t)8 * words));
    }
    if (e->ban_begin_on && !b.d_ban_begin) TRY(e->mem.get(&b.d_ban_begin, (size_t)8 * words));
    if (e->bias_on && !b.d_bias_rules) TRY(e->mem.get(&b.d_bias_rules, 8));
    if (e->bias_terms && !b.d_bias_w) {
        TRY(e->mem.get(&b.d_bias_w, (size_t)rows * 8 * words));
        TRY(e->mem.get(&b.d_bias_static, (size_t)8 * words));
        TRY(e->mem.get(&b.d_bias_tab, (size_t)rows * 8));
    }
    b.ban_words = words;
    if (e->hist_on && !b.d_hist) {
        TRY(e->mem.get(&b.d_hist, (size_t)rows * e->cfg.max_seq_len * 8));
        b.hist_cap = e->cfg.max_seq_len;
    }
    const ChannelBans no_bans;
    const ChannelBias no_bias;
    if (e->bans_on) {
        BanCfg cfg[8];
        // (once the begin bitmap exists every run with bans restages it, empty included: a captured step holds its address)
        const bool has_begin = b.d_ban_begin != nullptr;
        std::vector<uint32_t> stat((size_t)8 * words, 0u), begin(has_begin ? (size_t)8 * words : 0, 0u);
        for (int c = 0; c < 8; ++c) {
            const ChannelBans& cb = bans.ch.empty() ? no_bans : bans.ch[c];
            const ChannelBias& ci = bias.ch.empty() ? no_bias : bias.ch[c];
            const int V = c == 0 ? e->V0 : e->Vs;
            cfg[c] = BanCfg{cb.ngram, cb.min_new > 0 ? cb.min_new + 7 : 0, ci.min_length};
            stage_ban_static(cb.suppress.data(), (int)cb.suppress.size(), V, words, stat.data() + (size_t)c * words);
            if (has_begin) stage_ban_static(ci.begin.data(), (int)ci.begin.size(), V, words, begin.data() + (size_t)c * words);
        }
        HIPCHK(hipMemcpyAsync(e->d_bancfg, cfg, sizeof(cfg), hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(b.d_ban_static, stat.data(), stat.size() * 4, hipMemcpyHostToDevice, st));
        if (has_begin) HIPCHK(hipMemcpyAsync(b.d_ban_begin, begin.data(), begin.size() * 4, hipMemcpyHostToDevice, st));
        HIPCHK(hipStreamSynchronize(st));
    }
    if (e->bias_on) {
        std::vector<BiasRules> rules(8);
        std::vector<uint32_t> stat(e->bias_terms ? (size_t)8 * words : 0, 0u);
        for (int c = 0; c < 8; ++c) {
            const ChannelBias& ci = bias.ch[c];
            stage_bias_rules(ci.len.data(), ci.ids.data(), ci.beta.data(), (int)ci.len.size(), c == 0 ? e->V0 : e->Vs, words, &rules[c],
                             e->bias_terms ? stat.data() + (size_t)c * words : nullptr);
        }
        HIPCHK(hipMemcpyAsync(b.d_bias_rules, rules.data(), rules.size() * sizeof(BiasRules), hipMemcpyHostToDevice, st));
        if (e->bias_terms) HIPCHK(hipMemcpyAsync(b.d_bias_static, stat.data(), stat.size() * 4, hipMemcpyHostToDevice, st));
        HIPCHK(hipStreamSynchronize(st));
    }
    return 0;
}
static const char* hist_user(const MttsEngine* e) { return e->ban_ngram_on ? "no_repeat_ngram_size" : "sequence_bias / bad_words_ids"; }
// the prompt slots [n][8] of the dialogue in `slot`, for the n-gram ban and the rules longer than one token: into its row of bufs.d_hist.  on_stream: on `st`,
// which the caller drains before `host` dies (mtts_begin); else synchronously (mtts_slot_submit)
static int upload_history(MttsEngine* e, int slot, const int64_t* toks, int n, std::vector<int32_t>& host, bool on_stream, hipStream_t st) {
    if (n > e->bufs.hist_cap)
        return fail(MTTS_EINVAL, "%s: the prompt has %d slots (padding included), the history holds max_seq_len = %d", hist_user(e), n, e->bufs.hist_cap);
    host.resize((size_t)n * 8);
    stage_history(toks, n, host.data());
    int32_t* dst = e->bufs.d_hist + (size_t)slot * e->bufs.hist_cap * 8;
    if (on_stream) HIPCHK(hipMemcpyAsync(dst, host.data(), host.size() * 4, hipMemcpyHostToDevice, st));
    else HIPCHK(hipMemcpy(dst, host.data(), host.size() * 4, hipMemcpyHostToDevice));
    return 0;
}

// staged rows (staging.h) into the prefill staging, which grows to hold them.  on_stream: asynchronously on `st`, which
// the caller drains before `sr` dies (mtts_begin, mtts_score); else synchronously (mtts_slot_submit)
static int upload_staged(MttsEngine* e, const StagedRows& sr, bool on_stream, hipStream_t st) {
    if (sr.Mpad > e->pf_cap_rows) {       // (prefill passes read the staging, no decode step does)
        e->mem.release(e->d_pf_tokens); e->mem.release(e->d_pf_meta);
        e->pf_cap_rows = 0;
        TRY(e->mem.get(&e->d_pf_tokens, sr.Mpad * 8, false));
        TRY(e->mem.get(&e->d_pf_meta, sr.Mpad, false));
        e->pf_cap_rows = sr.Mpad;
    }
    const size_t tb = sr.Mpad * 8 * 4, mb = sr.Mpad * sizeof(RowMeta);
    if (on_stream) {
        HIPCHK(hipMemcpyAsync(e->d_pf_tokens, sr.toks.data(), tb, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(e->d_pf_meta, sr.metas.data(), mb, hipMemcpyHostToDevice, st));
    } else {
        HIPCHK(hipMemcpy(e->d_pf_tokens, sr.toks.data(), tb, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(e->d_pf_meta, sr.metas.data(), mb, hipMemcpyHostToDevice));
    }
    return 0;
}

// A new run starts from `seqs` (MTTS_RCAP slots; the idle ones as IDLE_SEQ) with every decode row idle, the loop state at
// step 0, the run's sampler settings (floors, typical: per channel, or empty) and clean sampler scratch.  Returns with `st` drained.
static const SeqState IDLE_SEQ{-1, 0, 0, 0, 0, 0, 0, 0, 0};
static int reset_run_state(MttsEngine* e, const std::vector<SeqState>& seqs, bool continuous, const MttsSamplerCfg* sampler,
                           const std::vector<MttsSamplerFloors>& floors, const std::vector<float>& typical, hipStream_t st) {
    HIPCHK(hipMemcpyAsync(e->d_seqs, seqs.data(), seqs.size() * sizeof(SeqState), hipMemcpyHostToDevice, st));
    if (continuous) e->forced_draw = 0;
    LoopState ls{0, 0, continuous ? 1 : 0, e->B, 0, e->bufs.gen_cap, e->forced_draw, e->f32 ? 1 : 0};
    e->continuous = continuous;
    e->join_step.assign(MTTS_RCAP, 0);
    HIPCHK(hipMemcpyAsync(e->d_ls, &ls, sizeof(ls), hipMemcpyHostToDevice, st));
    *e->h_ls = ls;
    std::vector<RowMeta> dm(MTTS_RCAP, RowMeta{-1, 0, 0, 0});
    HIPCHK(hipMemcpyAsync(e->d_meta, dm.data(), dm.size() * sizeof(RowMeta), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(e->d_scfg, sampler, 8 * sizeof(MttsSamplerCfg), hipMemcpyHostToDevice, st));
    e->ch0_sampled = sampler[0].do_sample ? 1 : 0;
    // probability floors: on when a channel that samples has one (a greedy channel applies none); off, the step is the
    // one a run without floors launches and nothing reads the table
    e->floors_on = 0;
    for (size_t c = 0; c < floors.size(); ++c)
        if (sampler[c].do_sample && (floors[c].min_p > 0.f || floors[c].epsilon_cutoff > 0.f || floors[c].eta_cutoff > 0.f)) e->floors_on = 1;
    // typical_p: the same, per sampled channel; its kernels read both tables, so the floors go up (as zeros) with it
    float typ[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    e->typical_on = 0;
    for (size_t c = 0; c < typical.size(); ++c)
        if (sampler[c].do_sample && typical[c] > 0.f) { typ[c] = typical[c]; e->typical_on = 1; }
    MttsSamplerFloors fl[8] = {};
    for (size_t c = 0; c < floors.size(); ++c) fl[c] = floors[c];
    if (e->floors_on || e->typical_on) HIPCHK(hipMemcpyAsync(e->d_floors, fl, sizeof(fl), hipMemcpyHostToDevice, st));
    if (e->typical_on) HIPCHK(hipMemcpyAsync(e->d_typical, typ, sizeof(typ), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(e->sscr.hist, 0, (size_t)e->cfg.max_batch * 2048 * 4, st));
    HIPCHK(hipMemsetAsync(e->sscr.cand_n, 0, (size_t)e->cfg.max_batch * 4, st));
    HIPCHK(hipMemsetAsync(e->sscr.overflow, 0, (size_t)e->cfg.max_batch * 4, st));
    HIPCHK(hipStreamSynchronize(st));   // the host arrays (the callers' too) may go out of scope
    return 0;
}

// One launch of fork_kernel (layer.hip): the page pairs already in `job`, plus for its row pairs the rows of the logits
// and, with `state_rows`, of the history bitmaps and the teacher-forcing tail.
static int launch_fork_job(MttsEngine* e, ForkJob& job, bool state_rows, hipStream_t st) {
    const int ew = e->f32 ? 4 : 2;                     // logits element bytes
    job.narr = 0;
    auto arr = [&](void* base, size_t stride, size_t bytes) {
        job.base[job.narr] = (uint8_t*)base; job.stride[job.narr] = (int64_t)stride; job.bytes[job.narr++] = (int64_t)bytes;
    };
    arr(e->logits0, (size_t)e->V0_pad * ew, (size_t)e->V0_pad * ew);
    arr(e->logits17, (size_t)7 * e->Vs_pad * ew, (size_t)7 * e->Vs_pad * ew);
    if (state_rows) {
        arr(e->d_bitmaps, (size_t)8 * e->bm_words * 4, (size_t)8 * e->bm_words * 4);
        arr(e->d_tf, (size_t)7 * 8 * 4, (size_t)7 * 8 * 4);
    }
    for (int i = 0; i < job.np; ++i)
        if (job.psrc[i] < 0 || job.psrc[i] >= e->total_pages || job.pdst[i] < 0 || job.pdst[i] >= e->total_pages)
            return fail(MTTS_EINVAL, "fork: page outside the pool");
    for (int i = 0; i < job.nr; ++i)
        if (job.rsrc[i] < 0 || job.rsrc[i] >= e->cfg.max_batch || job.rdst[i] < 0 || job.rdst[i] >= e->cfg.max_batch)
            return fail(MTTS_EINVAL, "fork: row outside the batch");
    const size_t blk = (size_t)MTTS_PAGE * MTTS_HD * (e->f32 ? 4 : 2), layer = e->layer_stride * (e->f32 ? 4 : 2);
    void* kc = e->f32 ? (void*)e->kcache_f : e->kcache;
    void* vc = e->f32 ? (void*)e->vcache_f : e->vcache;
    launch_fork(kc, vc, layer, (size_t)e->total_pages * blk, (int)blk, e->L, e->nkv, job, st);
    HIPCHK(hipGetLastError());
    return 0;
}

// ---- begin: parse prompt, allocate pages, prefill --------------------------------------
static int begin_run(MttsEngine* e, const int64_t* ids, const uint8_t* mask, int32_t B, int32_t T, int32_t max_length,
                     const MttsSamplerCfg* sampler, uint64_t seed, const RunOptions& opt, void* stream) {
    if (!ids || !mask || !sampler) return fail(MTTS_EINVAL, "null argument");
    TRY(mtts_weights_ready(e));
    HIPCHK(hipSetDevice(e->device));
    hipStream_t st = S(stream);
    // one adapter id per prompt (mtts_set_row_adapters); none given: no row has one
    bool lora = false;
    for (size_t b = 0; b < opt.row_adapters.size(); ++b) {
        TRY(adapter_id_check(e, opt.row_adapters[b], "row", (int)b));
        lora |= opt.row_adapters[b] >= 0;
    }
    // takes: row b*takes+j is take j of prompt b; only the B prompts are prefilled (into rows b*takes), the other takes
    // share their complete prompt pages and get a copy of the rest (fork_kernel)
    const int takes = opt.takes, R = opt.rows();
    if (T < 8) return fail(MTTS_EINVAL, "T must be >= 8 (delay pattern adds 7 slots)");
    const int base = T - 7;
    if (max_length <= base) return fail(MTTS_EINVAL, "max_length %d leaves no room to generate (prompt slots %d)", max_length, base);
    // a dialogue whose EOS falls within 7 steps of max_length keeps stepping until its flush is through
    // (`unfinished | needs_additional_steps > 0`, modeling_asteroid.py:165-168)
    int max_steps = max_length - base + LINGER_STEPS;          // the least the engine must have room for; widened below
    e->B = R; e->T = T; e->base_length = base; e->max_length = max_length; e->takes = takes;
    e->seed = seed; e->steps_issued = 0; e->has_forced = false; e->split_phase = 0;
    e->n_real.assign(R, 0);
    e->max_real = 0;
    std::vector<StageSeq> seqs(B);     // prompt b: its real tokens, into row b*takes; the last one's logits start the run
    for (int b = 0; b < B; ++b) {
        int p = 0;
        TRY(mask_left_padded(mask + (size_t)b * T, base, b, &p));
        seqs[b] = StageSeq{ids + ((size_t)b * T + p) * 8, base - p, b * takes, true, nullptr};
        for (int j = 0; j < takes; ++j) e->n_real[b * takes + j] = base - p;
        e->max_real = std::max(e->max_real, base - p);
    }
    // pages: every earlier run has been synchronised by its caller or is ordered before us on `st`; the prompts'
    // pages are taken now, the rest on demand as the dialogues grow (issue_steps)
    e->pool.release_all();             // (also the edits a failed run left queued: they belong to released pages)
    for (int b = 0; b < e->cfg.max_batch; ++b) e->slot_live[b] = b < R;
    TRY(pack_policy_reset(e, st));
    const auto ship = ship_on(e, st);
    ForkJob fork;
    fork.np = 0; fork.nr = 0;
    for (int b = 0; b < B; ++b) {
        const int src = b * takes, len = e->n_real[src], full = len / MTTS_PAGE;
        const int need = pages_for(len + max_steps);
        if (need > e->max_pages) return fail(MTTS_ENOMEM, "row %d needs %d KV pages, a sequence holds at most %d (max_seq_len %d)", src, need, e->max_pages, e->cfg.max_seq_len);
        TRY(e->pool.grow(src, pages_for(len), ship));
        for (int j = 1; j < takes; ++j) {
            const int dst = src + j;
            TRY(e->pool.share(src, dst, full, ship));
            if (len % MTTS_PAGE) {
                TRY(e->pool.grow(dst, full + 1, ship));
                fork.psrc[fork.np] = e->pool.entry(src, full);
                fork.pdst[fork.np++] = e->pool.entry(dst, full);
            }
            fork.rsrc[fork.nr] = src;
            fork.rdst[fork.nr++] = dst;
        }
    }
    TRY(e->pool.flush(ship));
    if (e->max_real + max_steps > e->bufs.rope_rows)
        return fail(MTTS_EINVAL, "rope table has %d rows, need %d", e->bufs.rope_rows, e->max_real + max_steps);
    // room for chained resurrections (linger_bound) as far as the page-table width and the RoPE table allow
    max_steps = std::max(max_steps, std::min(max_length - base + linger_bound(R),
                                             std::min(e->max_pages * MTTS_PAGE, e->bufs.rope_rows) - e->max_real));
    e->max_steps = max_steps;
    // generation buffers
    e->scores_on = opt.output_scores; e->topk_on = opt.top_logprobs;
    TRY(start_outputs(e, max_steps, st));
    TRY(start_bans(e, opt.bans, opt.bias, st));
    if (e->hist_on && base > e->bufs.hist_cap)
        return fail(MTTS_EINVAL, "%s: the prompt has %d slots (padding included), the history holds max_seq_len = %d", hist_user(e), base, e->bufs.hist_cap);
    StagedRows sr;
    TRY(stage_rows(seqs, e->V0, e->Vs, false, &sr));
    {
        // every row's history bitmap (over all the padded slots of its prompt), teacher-forcing tail and state: all the
        // host work that can refuse the call comes before the first copy, so no copy is left reading a vector that died
        std::vector<uint32_t> bm((size_t)MTTS_RCAP * 8 * e->bm_words, 0u);
        std::vector<int32_t> tf((size_t)MTTS_RCAP * 7 * 8, 0);
        for (int rw = 0; rw < R; ++rw) {
            const int64_t* prompt = ids + (size_t)(rw / takes) * T * 8;
            stage_bitmap(prompt, base, e->bm_words, bm.data() + (size_t)rw * 8 * e->bm_words);
            TRY(stage_tail(prompt + (size_t)base * 8, e->V0, e->Vs, " (delayed tail)", tf.data() + (size_t)rw * 7 * 8));
        }
        std::vector<SeqState> ss(MTTS_RCAP, IDLE_SEQ);
        for (int b = 0; b < R; ++b) ss[b] = SeqState{-1, 1, e->n_real[b], 0, base, max_length, opt.row_id(b), 1, seed};
        // n-gram ban: every row's prompt slots, the stream the bitmap was built from (a prompt's takes start from the same)
        std::vector<std::vector<int32_t>> hist(e->hist_on ? B : 0);
        for (int rw = 0; e->hist_on && rw < R; ++rw) {
            std::vector<int32_t>& hb = hist[rw / takes];
            if (rw % takes == 0) TRY(upload_history(e, rw, ids + (size_t)(rw / takes) * T * 8, base, hb, true, st));
            else HIPCHK(hipMemcpyAsync(e->bufs.d_hist + (size_t)rw * e->bufs.hist_cap * 8, hb.data(), hb.size() * 4, hipMemcpyHostToDevice, st));
        }
        TRY(upload_staged(e, sr, true, st));
        HIPCHK(hipMemcpyAsync(e->d_bitmaps, bm.data(), bm.size() * 4, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(e->d_tf, tf.data(), tf.size() * 4, hipMemcpyHostToDevice, st));
        // the rows' adapters: a prompt's takes share its KV pages and so its adapter
        for (int b = 0; b < MTTS_RCAP; ++b) e->seq_adapter[b] = b < R ? opt.row_adapter(b) : -1;
        if (e->bufs.d_seq_adapter) HIPCHK(hipMemcpyAsync(e->bufs.d_seq_adapter, e->seq_adapter.data(), MTTS_RCAP * sizeof(int32_t), hipMemcpyHostToDevice, st));
        TRY(reset_run_state(e, ss, false, sampler, opt.floors, opt.typical, st));   // drains st: the host vectors above go out of scope
    }
    TRY(prefill_staged(e, sr.Mpad, pages_for(e->max_real), 2, lora, st));
    // takes: the partially filled last prompt page of each source row into its takes' private pages, and the source
    // row's logits into theirs (bitmaps, teacher-forcing tails and states were uploaded for every row above)
    if (fork.nr) TRY(launch_fork_job(e, fork, false, st));
    e->began = true;
    e->run_open = true;
    return MTTS_OK;
}

int32_t mtts_set_takes(MttsEngine* e, int32_t n) {
    if (!e) return fail(MTTS_EINVAL, "null engine");
    if (n < 1 || n > MTTS_RCAP) return fail(MTTS_EINVAL, "takes must be 1..%d (got %d)", MTTS_RCAP, n);
    e->pending.set_takes(n);
    return MTTS_OK;
}
int32_t mtts_set_sampler_floors(MttsEngine* e, const MttsSamplerFloors* floors) {
    if (!e) return fail(MTTS_EINVAL, "null engine");
    return e->pending.set_floors(floors);
}
int32_t mtts_set_sampler_typical(MttsEngine* e, const float* typical_p) {
    if (!e) return fail(MTTS_EINVAL, "null engine");
    return e->pending.set_typical(typical_p);
}
int32_t mtts_set_sampler_bans(MttsEngine* e, const MttsSamplerBans* bans) {
    if (!e) return fail(MTTS_EINVAL, "null engine");
    return e->pending.set_bans(bans);
}
int32_t mtts_set_sampler_bias(MttsEngine* e, const MttsSamplerBias* bias) {
    if (!e) return fail(MTTS_EINVAL, "null engine");
    return e->pending.set_bias(bias);
}
// The options of the mtts_begin / mtts_generate that starts now: out of the engine first -- so the one-shot ones are
// consumed whatever the call does next -- and then checked.
static int take_options(MttsEngine* e, int B, bool forced, RunOptions* opt) {
    *opt = e->pending.take(B);
    return opt->check(e->cfg.max_batch, forced);
}

int32_t mtts_begin(MttsEngine* e, const int64_t* ids, const uint8_t* mask, int32_t B, int32_t T, int32_t max_length,
                   const MttsSamplerCfg* sampler, uint64_t seed, void* stream) {
    if (!e) return fail(MTTS_EINVAL, "null argument");
    RunOptions opt;
    TRY(take_options(e, B, false, &opt));
    return begin_run(e, ids, mask, B, T, max_length, sampler, seed, opt, stream);
}

// One decode step: sample from the previous logits, advance the per-dialogue state machine, run the stack.
// Nothing in it depends on the host (step counters, lengths and the stop flag live on the device), so the same
// launches repeat until the KV page bound grows: they are captured once per bound into a hipGraph and replayed --
// a dependent kernel costs ~1.5 us inside a graph against ~2.9 us launched on a stream (tools/latency_probe.hip).
// The plan (decode_plan) says which launches; it is also what a captured step is found by.
// The three parts below are what the split step (mtts_step_begin / mtts_step_sample / mtts_step_finish) issues one by one.
// step_front: this step's ban words and rule tables; -> the sampler's scratch with what they wrote
static SampleScratch step_front(MttsEngine* e, const StepPlan& plan, hipStream_t st) {
    const StepBufs& b = e->bufs;
    SampleScratch sscr = e->sscr;
    sscr.slice_sum = b.sscr_slice_sum; sscr.lp = b.sscr_lp;
    if (plan.bans_on) {                  // this step's banned tokens, from the history as the last update_kernel left it
        launch_ban(b.d_ban, b.d_ban_static, b.d_ban_begin, b.ban_words, e->d_bancfg, b.d_hist, b.hist_cap, b.d_gen, e->V0, e->Vs, e->cfg.eos_token_id,
                   e->d_ls, e->d_seqs, plan.B, st);
        sscr.ban = b.d_ban;
    }
    if (plan.bias_on) {                  // the rules against the same history: -inf hits into the ban words, finite ones into words and tables
        launch_bias(plan.bans_on ? b.d_ban : nullptr, plan.bias_terms ? b.d_bias_w : nullptr, b.d_bias_static, plan.bias_terms ? b.d_bias_tab : nullptr,
                    b.ban_words, b.d_bias_rules, b.d_hist, b.hist_cap, b.d_gen, e->V0, e->Vs, e->d_ls, e->d_seqs, plan.B, st);
        if (plan.bias_terms) { sscr.bias_w = b.d_bias_w; sscr.bias_t = b.d_bias_tab; }
    }
    return sscr;
}
// step_decide: the sampler on score rows l0 / l17 (the heads' logits; the split step: the caller's fp32 rows, sscr.ext), then
// top_logprobs on the heads' logits and the state machine
static void step_decide(MttsEngine* e, const StepPlan& plan, const SampleScratch& sscr, const void* l0, const void* l17, hipStream_t st) {
    const StepBufs& b = e->bufs;
    launch_sample(l0, l17, e->V0, e->Vs, e->Vs_pad, e->d_bitmaps, e->bm_words, e->d_scfg, e->d_ls,
                  e->d_seqs, e->seed, e->d_decisions, &e->d_ls->error, plan.B, sscr, plan.ch0_sampled,
                  full_cap_for(e->V0), plan.scores_on, (plan.floors_on || plan.typical_on) ? e->d_floors : nullptr,
                  plan.typical_on ? e->d_typical : nullptr, st);
    GenTopkOut gt;                       // top_logprobs: the raw distribution at the decisions just written, into this step's row
    if (plan.topk) {
        gt = GenTopkOut{plan.topk, b.d_gt_logp, b.d_gt_ids, b.d_gt_tlp};
        launch_gen_topk(e->logits0, e->logits17, e->V0, e->Vs, e->Vs_pad, e->d_scfg, e->d_ls, e->d_seqs, e->d_decisions, plan.B,
                        GenTopkScratch{b.gt_cand, b.gt_smax, b.gt_ssum, b.gt_scr_cap}, gt, st);
    }
    launch_update(e->d_decisions, b.d_declog, plan.forced ? b.d_forced : nullptr, e->d_tf, b.d_gen, e->d_cur,
                  e->d_seqs, e->d_meta, e->d_bitmaps, e->bm_words, e->d_ls, e->cfg.eos_token_id,
                  e->cfg.speech_pad_token, e->cfg.speech_range_lo, e->cfg.speech_range_hi,
                  plan.scores_on ? b.sscr_lp : nullptr, plan.scores_on ? b.d_lp : nullptr, gt, st);
}
static int step_body(MttsEngine* e, const StepPlan& plan, int pages_bound, hipStream_t st, int64_t kvtok) {
    const SampleScratch sscr = step_front(e, plan, st);
    step_decide(e, plan, sscr, e->logits0, e->logits17, st);
    return forward_rows(e, plan, e->d_cur, e->d_meta, pages_bound, st, kvtok);
}

static int step_graph(MttsEngine* e, int pages, hipGraphExec_t* out) {
    StepPlan plan = decode_plan(e, pages);
    if (const hipGraphExec_t* hit = e->graphs.find(plan, pages, e->bufs)) {
        *out = *hit;
        return MTTS_OK;
    }
    if (!e->cap_stream) HIPCHK(hipStreamCreateWithFlags(&e->cap_stream, hipStreamNonBlocking));
    hipGraph_t g = nullptr;
    HIPCHK(hipStreamBeginCapture(e->cap_stream, hipStreamCaptureModeRelaxed));
    int rc = step_body(e, plan, pages, e->cap_stream, 0);
    hipError_t ce = hipStreamEndCapture(e->cap_stream, &g);
    if (rc) { if (g) hipGraphDestroy(g); return rc; }
    HIPCHK(ce);
    hipGraphExec_t exec = nullptr;
    hipError_t ie = hipGraphInstantiate(&exec, g, nullptr, nullptr, 0);
    hipGraphDestroy(g);
    HIPCHK(ie);
    e->graphs.insert(std::move(plan), pages, e->bufs, exec);
    *out = exec;
    return MTTS_OK;
}

// The step about to be issued appends one token per live dialogue at position n_real + steps_issued: take its page if that
// crosses a page boundary (the host's view of "live" lags the device by at most one poll: a dialogue that has just
// finished may get one page it never writes, returned with the others).  -> the step's KV page bound
static int step_pages(MttsEngine* e, hipStream_t st, int* pages_bound) {
    int len_bound = 1;
    const auto ship = ship_on(e, st);
    for (int b = 0; b < e->B; ++b) {
        if (!e->slot_live[b]) continue;
        const int len = e->n_real[b] + e->steps_issued + 1;
        len_bound = std::max(len_bound, len);
        TRY(e->pool.grow(b, pages_for(len), ship));
    }
    TRY(e->pool.flush(ship));
    *pages_bound = pages_for(len_bound);
    return MTTS_OK;
}

static int issue_steps(MttsEngine* e, int n, hipStream_t st) {
    for (int i = 0; i < n; ++i) {
        if (e->steps_issued >= e->max_steps) break;
        int pages_bound = 0;
        TRY(step_pages(e, st, &pages_bound));
        if (e->knobs.use_graphs && !e->prof) {
            // the attention grids are sized by the page bound: round it up to a whole pass-B chunk so that one
            // graph serves ATT_PB pages (512 steps); blocks past a row's last page exit at once
            hipGraphExec_t exec = nullptr;
            TRY(step_graph(e, std::min(round_up(pages_bound, ATT_PB), e->max_pages), &exec));
            HIPCHK(hipGraphLaunch(exec, st));
        } else {
            hipEvent_t ev = nullptr;
            prof_begin(e, PROF_STEP, st, &ev);
            // rough KV token count for the profile's byte figure: every row at its current length
            int64_t kvtok = 0;
            for (int b = 0; b < e->B; ++b) if (e->slot_live[b]) kvtok += e->n_real[b] + e->steps_issued + 1;
            TRY(step_body(e, decode_plan(e, pages_bound), pages_bound, st, kvtok));
            prof_end(e, st, ev);
        }
        e->steps_issued++;
    }
    return MTTS_OK;
}

int32_t mtts_step(MttsEngine* e, int32_t n_steps, void* stream) {
    if (!e || !e->began) return fail(MTTS_ESTATE, "mtts_begin has not run");
    if (e->split_phase) return fail(MTTS_ESTATE, "mtts_step in the middle of a split step: mtts_step_finish first");
    HIPCHK(hipSetDevice(e->device));
    return issue_steps(e, n_steps, S(stream));
}

// ---- the split step: generate(logits_processor=, stopping_criteria=, streamer=) ------------------------------------------
// One decode step in up to three calls with the caller in between (include/mtts.h).  The launches are those of step_body,
// in its order, on the caller's stream: a split step is never captured, and its plan carries `split`, so it is never taken
// for a captured unsplit step either.
static int split_check(MttsEngine* e, const char* who) {
    if (!e || !e->began) return fail(MTTS_ESTATE, "%s: mtts_begin has not run", who);
    if (e->continuous) return fail(MTTS_ESTATE, "%s: the scheduler's steps are not split (mtts_sched_open is running)", who);
    return MTTS_OK;
}
int32_t mtts_step_begin(MttsEngine* e, float* dev_scores0, float* dev_scores17, void* stream) {
    TRY(split_check(e, "mtts_step_begin"));
    if (e->split_phase) return fail(MTTS_ESTATE, "mtts_step_begin: a split step is in flight, mtts_step_finish first");
    if (!dev_scores0 || !dev_scores17 || ((uintptr_t)dev_scores0 & 15) || ((uintptr_t)dev_scores17 & 15))
        return fail(MTTS_EINVAL, "mtts_step_begin: the score buffers are null or not 16-byte aligned");
    if (e->steps_issued >= e->max_steps) return fail(MTTS_ESTATE, "mtts_step_begin: the run has no step left (%d issued)", e->steps_issued);
    HIPCHK(hipSetDevice(e->device));
    hipStream_t st = S(stream);
    const StepPlan plan = decode_plan(e, 1, true);      // (the page bound plays no part in front of the forward pass)
    const SampleScratch sscr = step_front(e, plan, st);
    launch_scores_materialize(e->logits0, e->logits17, e->V0, e->Vs, e->Vs_pad, e->d_bitmaps, e->bm_words, e->d_scfg, e->d_ls, e->d_seqs,
                              plan.B, sscr, dev_scores0, dev_scores17, st);
    HIPCHK(hipGetLastError());
    e->split_scores0 = dev_scores0; e->split_scores17 = dev_scores17;
    e->split_phase = 1;
    return MTTS_OK;
}
int32_t mtts_step_sample(MttsEngine* e, int64_t* dev_tokens, void* stream) {
    TRY(split_check(e, "mtts_step_sample"));
    if (e->split_phase != 1) return fail(MTTS_ESTATE, "mtts_step_sample: mtts_step_begin has not run for this step");
    HIPCHK(hipSetDevice(e->device));
    hipStream_t st = S(stream);
    const StepPlan plan = decode_plan(e, 1, true);
    SampleScratch sscr = e->sscr;       // no ban words, no terms: the rows carry them
    sscr.slice_sum = e->bufs.sscr_slice_sum; sscr.lp = e->bufs.sscr_lp;
    sscr.ext = 1;
    step_decide(e, plan, sscr, e->split_scores0, e->split_scores17, st);
    if (dev_tokens) launch_step_tokens(e->d_cur, dev_tokens, e->d_ls, st);
    HIPCHK(hipGetLastError());
    e->split_phase = 2;
    return MTTS_OK;
}
int32_t mtts_step_finish(MttsEngine* e, const uint8_t* host_stop, void* stream) {
    TRY(split_check(e, "mtts_step_finish"));
    if (!e->split_phase) return fail(MTTS_ESTATE, "mtts_step_finish: mtts_step_begin has not run for this step");
    if (e->split_phase == 1) TRY(mtts_step_sample(e, nullptr, stream));
    HIPCHK(hipSetDevice(e->device));
    hipStream_t st = S(stream);
    if (host_stop) {
        StopMask m;                     // (travels as a kernel argument: no copy to order, no buffer to keep)
        memset(m.row, 0, sizeof(m.row));
        memcpy(m.row, host_stop, (size_t)e->B);
        launch_stop_rows(m, e->d_seqs, e->d_meta, e->d_ls, st);
    }
    int pages_bound = 0;
    TRY(step_pages(e, st, &pages_bound));
    int64_t kvtok = 0;
    for (int b = 0; b < e->B; ++b) if (e->slot_live[b]) kvtok += e->n_real[b] + e->steps_issued + 1;
    TRY(forward_rows(e, decode_plan(e, pages_bound, true), e->d_cur, e->d_meta, pages_bound, st, kvtok));
    e->steps_issued++;
    e->split_phase = 0;
    return MTTS_OK;
}

int32_t mtts_sync_state(MttsEngine* e, int32_t* steps_done, int32_t* all_finished, void* stream) {
    if (!e || !e->began) return fail(MTTS_ESTATE, "mtts_begin has not run");
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipMemcpyAsync(e->h_ls, e->d_ls, sizeof(LoopState), hipMemcpyDeviceToHost, S(stream)));
    // (both copies ride the caller's stream into pinned memory: no null-stream copy that would serialise with the codec leg)
    if (!e->continuous) HIPCHK(hipMemcpyAsync(e->h_seqs, e->d_seqs, e->B * sizeof(SeqState), hipMemcpyDeviceToHost, S(stream)));
    if (e->d_seal_cnt) HIPCHK(hipMemcpyAsync(e->h_seal_cnt, e->d_seal_cnt, (size_t)e->L * 4 * sizeof(unsigned long long), hipMemcpyDeviceToHost, S(stream)));
    HIPCHK(hipStreamSynchronize(S(stream)));
    if (e->d_seal_cnt && e->knobs.kv_pack == 1) {    // the read policy per layer; the next step's plan follows it, and with it its graph
        for (int n = 0; n < e->L; ++n) {
            const unsigned long long* c = e->h_seal_cnt + (size_t)n * 4;
            e->pack_k_on[n] = c[0] + c[1] < 16 || c[1] * 8 <= c[0] + c[1];
            e->pack_v_on[n] = c[2] + c[3] < 16 || c[3] * 8 <= c[2] + c[3];
        }
    }
    if (e->h_ls->error) return fail(MTTS_EINVAL, "device sampler error %d: more than 4096 candidate tokens (set top_k so that the k-th score's radix bin holds <= 4096 tokens)", e->h_ls->error);
    if (!e->continuous) {
        // static batch (mtts_generate semantics): a finished row only emits padding from here on and never touches
        // its KV pages again; everything issued so far has completed, so its pages go back to the pool
        const SeqState* ss = e->h_seqs;
        for (int b = 0; b < e->B; ++b)
            if (e->slot_live[b] && ss[b].step > 0 && !ss[b].unfinished && ss[b].active != 2) { e->slot_live[b] = 0; e->pool.release(b); }
    }
    if (steps_done) *steps_done = e->h_ls->step;
    if (all_finished) *all_finished = e->h_ls->done;
    if (e->h_ls->done && !e->continuous) e->run_open = false;
    return MTTS_OK;
}

// `nslots` slots from `slot0` of a device array [slot][gen_cap][w] -> host [step][slot - slot0][w] (w = 8, or 8 k: top_logprobs)
template <typename Src, typename Dst>
static int read_slots(MttsEngine* e, const Src* d_src, int slot0, int nslots, int steps, Dst* host, int w = 8) {
    std::vector<Src> tmp((size_t)std::max(steps, 1) * w);
    for (int b = 0; b < nslots; ++b) {
        if (steps) HIPCHK(hipMemcpy(tmp.data(), d_src + (size_t)(slot0 + b) * e->bufs.gen_cap * w, (size_t)steps * w * sizeof(Src), hipMemcpyDeviceToHost));
        for (int s = 0; s < steps; ++s)
            for (int c = 0; c < w; ++c) host[((size_t)s * nslots + b) * w + c] = tmp[(size_t)s * w + c];
    }
    return MTTS_OK;
}
// every row of the run, all steps so far
template <typename Src, typename Dst>
static int read_rows(MttsEngine* e, const Src* d_src, Dst* host, int capacity_steps, int* n_steps, int w = 8) {
    const int steps = e->h_ls->step;
    if (steps > capacity_steps) return fail(MTTS_EINVAL, "output buffer holds %d steps, need %d", capacity_steps, steps);
    TRY(read_slots(e, d_src, 0, e->B, steps, host, w));
    if (n_steps) *n_steps = steps;
    return MTTS_OK;
}
// one slot of a scheduler run, the steps its dialogue has run
template <typename Src, typename Dst>
static int slot_read(MttsEngine* e, const Src* d_src, int slot, Dst* host_rows, int capacity_steps, int* n_steps, int w = 8) {
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipDeviceSynchronize());
    SeqState cur;
    HIPCHK(hipMemcpy(&cur, e->d_seqs + slot, sizeof(cur), hipMemcpyDeviceToHost));
    if (cur.step > capacity_steps) return fail(MTTS_EINVAL, "buffer holds %d steps, need %d", capacity_steps, cur.step);
    TRY(read_slots(e, d_src, slot, 1, cur.step, host_rows, w));
    if (n_steps) *n_steps = cur.step;
    return MTTS_OK;
}
// last forward's logits (T = the engine's logits element): channel 0 [B][V0], channels 1..7 [7][B][Vs]
template <typename T>
static int read_logits(MttsEngine* e, T* l0, T* l17, void* stream) {
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipStreamSynchronize(S(stream)));
    if (l0) HIPCHK(hipMemcpy2D(l0, (size_t)e->V0 * sizeof(T), e->logits0, (size_t)e->V0_pad * sizeof(T), (size_t)e->V0 * sizeof(T), e->B, hipMemcpyDeviceToHost));
    if (l17) {
        std::vector<T> tmp((size_t)MTTS_RCAP * 7 * e->Vs_pad);
        HIPCHK(hipMemcpy(tmp.data(), e->logits17, tmp.size() * sizeof(T), hipMemcpyDeviceToHost));
        for (int c = 0; c < 7; ++c)
            for (int b = 0; b < e->B; ++b)
                memcpy(l17 + ((size_t)c * e->B + b) * e->Vs, tmp.data() + ((size_t)b * 7 + c) * e->Vs_pad, (size_t)e->Vs * sizeof(T));
    }
    return MTTS_OK;
}

int32_t mtts_read_generated(MttsEngine* e, int64_t* host_gen, int32_t capacity_steps, int32_t* n_steps) {
    if (!e || !e->began || !host_gen) return fail(MTTS_ESTATE, "nothing generated");
    HIPCHK(hipSetDevice(e->device));
    TRY(mtts_sync_state(e, nullptr, nullptr, nullptr));
    return read_rows(e, e->bufs.d_gen, host_gen, capacity_steps, n_steps);
}

// A run counts as open until the device says it has ended: every row finished / every slot empty.  -> *open.
static int run_still_open(MttsEngine* e, bool* open) {
    *open = false;
    if (!e->run_open) return MTTS_OK;
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipDeviceSynchronize());
    LoopState ls;
    std::vector<SeqState> ss(MTTS_RCAP);
    HIPCHK(hipMemcpy(&ls, e->d_ls, sizeof(ls), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(ss.data(), e->d_seqs, ss.size() * sizeof(SeqState), hipMemcpyDeviceToHost));
    bool live = false;
    for (int b = 0; b < e->B; ++b) live |= ss[b].active != 0;
    if (live && !ls.done) *open = true;
    else e->run_open = false;
    return MTTS_OK;
}

int32_t mtts_set_output_scores(MttsEngine* e, int32_t on) {
    if (!e) return fail(MTTS_EINVAL, "null engine");
    on = on ? 1 : 0;
    if (on == e->pending.output_scores) return MTTS_OK;
    bool open = false;
    TRY(run_still_open(e, &open));
    if (open) return fail(MTTS_ESTATE, "output_scores cannot change while a run is open (it is read when a run begins)");
    e->pending.output_scores = on;
    return MTTS_OK;
}

// host_lp float [capacity_steps][rows][8]: row space and step range of mtts_read_generated
int32_t mtts_read_scores(MttsEngine* e, float* host_lp, int32_t capacity_steps, int32_t* n_steps) {
    if (!e || !e->began || !host_lp) return fail(MTTS_ESTATE, "nothing generated");
    if (!e->scores_on) return fail(MTTS_ESTATE, "the run was started with output_scores off (mtts_set_output_scores)");
    HIPCHK(hipSetDevice(e->device));
    TRY(mtts_sync_state(e, nullptr, nullptr, nullptr));
    return read_rows(e, e->bufs.d_lp, host_lp, capacity_steps, n_steps);
}

int32_t mtts_set_top_logprobs(MttsEngine* e, int32_t k) {
    if (!e) return fail(MTTS_EINVAL, "null engine");
    if (k < 0 || k > MTTS_SCORE_MAX_TOPK) return fail(MTTS_EINVAL, "top_logprobs must be 0 (off) or 1..%d (got %d)", MTTS_SCORE_MAX_TOPK, k);
    if (k == e->pending.top_logprobs) return MTTS_OK;
    bool open = false;
    TRY(run_still_open(e, &open));
    if (open) return fail(MTTS_ESTATE, "top_logprobs cannot change while a run is open (it is read when a run begins)");
    e->pending.top_logprobs = k;
    return MTTS_OK;
}

// host_logp float [capacity_steps][rows][8], host_top_ids int32 / host_top_logp float [capacity_steps][rows][8][k]
int32_t mtts_read_top_logprobs(MttsEngine* e, float* host_logp, int32_t* host_top_ids, float* host_top_logp, int32_t capacity_steps,
                               int32_t* n_steps) {
    if (!e || !e->began || !host_logp || !host_top_ids || !host_top_logp) return fail(MTTS_ESTATE, "nothing generated");
    if (!e->topk_on) return fail(MTTS_ESTATE, "the run was started with top_logprobs off (mtts_set_top_logprobs)");
    HIPCHK(hipSetDevice(e->device));
    TRY(mtts_sync_state(e, nullptr, nullptr, nullptr));
    TRY(read_rows(e, e->bufs.d_gt_logp, host_logp, capacity_steps, n_steps));
    TRY(read_rows(e, e->bufs.d_gt_ids, host_top_ids, capacity_steps, n_steps, 8 * e->topk_on));
    return read_rows(e, e->bufs.d_gt_tlp, host_top_logp, capacity_steps, n_steps, 8 * e->topk_on);
}

// ---- teacher-forced scoring (the labels branch of AsteroidTTSInstruct.forward, modeling_asteroid.py:382-410) ---------
#define SCORE_F32_ROWS 64      // fp32 / fp16 engines: rows whose logits of one head are materialised at a time (64 x 152 704 x 4 B = 37 MiB)

// While a scoring pass runs, completed KV pages are not sealed: no decode follows that would read the sealed form, and
// the seal counters steer the read policy of generation runs.
struct NoSeal {
    MttsEngine* e; void* k;
    explicit NoSeal(MttsEngine* e_) : e(e_), k(e_->kpack) { e->kpack = nullptr; }
    ~NoSeal() { e->kpack = k; }
};

// heads + log-softmax + label pick on the `rows` final-normed rows the pass has just left in xn (bf16: packed) / xnf
// k > 0 (mtts_score_topk): the k best tokens of every row and head as well, top_ids / top_logp [rows][8][k]; logp null
// when the call has no labels (`labels` is then -100 throughout)
static int score_pass(MttsEngine* e, const int32_t* labels, float* logp, int rows, hipStream_t st, int k = 0, int32_t* top_ids = nullptr,
                      float* top_logp = nullptr) {
    const int H = e->H;
    if (!e->f32) {
        float* part17 = e->sc_part + head_ce_part_elems(MTTS_PFCAP, e->V0, 1);
        hipEvent_t ev = nullptr;
        prof_begin(e, PROF_CE, st, &ev);
        if (k > 0) {
            launch_head_topk(e->head0, e->xn, rows, H, e->V0, 1, labels, 8, 0, e->sc_part, logp, 8, 0, k, e->sc_cand, top_ids, top_logp, st);
            launch_head_topk(e->heads17, e->xn, rows, H, e->Vs, 7, labels, 8, 1, part17, logp, 8, 1, k, e->sc_cand, top_ids, top_logp, st);
        } else {
            launch_head_ce(e->head0, e->xn, rows, H, e->V0, 1, labels, 8, 0, e->sc_part, logp, 8, 0, st);
            launch_head_ce(e->heads17, e->xn, rows, H, e->Vs, 7, labels, 8, 1, part17, logp, 8, 1, st);
        }
        prof_end(e, st, ev);
        if (e->prof) e->prof_bytes[PROF_CE] += ((int64_t)e->V0_pad + 7 * e->Vs_pad) * H * 2;       // one read of the heads
    } else {
        for (int r0 = 0; r0 < rows; r0 += SCORE_F32_ROWS) {
            const int n = std::min(SCORE_F32_ROWS, rows - r0);
            for (int c = 0; c < 8; ++c) {
                const int V = c == 0 ? e->V0 : e->Vs;
                launch_f32_linear(e->embf[c], e->xnf + (size_t)r0 * H, e->sc_logits, n, V, H, e->V0_pad, e->h16, false, st);
                if (logp) launch_ce_rows_f32(e->sc_logits, e->V0_pad, n, V, labels + (size_t)r0 * 8, 8, c, logp + (size_t)r0 * 8, 8, c, st);
                if (k > 0)
                    launch_topk_rows_f32(e->sc_logits, e->V0_pad, n, V, k, top_ids + (size_t)r0 * 8 * k, top_logp + (size_t)r0 * 8 * k, 8, c, st);
            }
        }
    }
    HIPCHK(hipGetLastError());
    return MTTS_OK;
}

// mtts_score (k = 0: labels and host_logp given) and mtts_score_topk (k >= 1: labels and host_logp both given or both null)
static int32_t score_call(MttsEngine* e, const int64_t* ids, const uint8_t* mask, const int64_t* labels, int32_t B, int32_t T,
                          float* host_logp, int32_t k, int32_t* host_top_ids, float* host_top_logp, void* stream) {
    if (!e || !ids || !mask) return fail(MTTS_EINVAL, "null argument");
    TRY(mtts_weights_ready(e));
    HIPCHK(hipSetDevice(e->device));
    hipStream_t st = S(stream);
    if (B < 1 || B > e->cfg.max_batch) return fail(MTTS_EINVAL, "batch %d outside 1..max_batch %d", B, e->cfg.max_batch);
    if (T < 1 || T > e->cfg.max_seq_len) return fail(MTTS_EINVAL, "T %d outside 1..max_seq_len %d", T, e->cfg.max_seq_len);
    if (T > e->bufs.rope_rows) return fail(MTTS_EINVAL, "rope table has %d rows, need %d", e->bufs.rope_rows, T);
    if (e->pending.has_row_adapters())
        return fail(MTTS_ESTATE, "mtts_score takes no per-row adapters and a mtts_set_row_adapters list is pending (it stays so): score an adapter merged, with mtts_bind_weight_lora");
    bool open = false;
    TRY(run_still_open(e, &open));
    if (open) return fail(MTTS_ESTATE, "mtts_score while a run is open: its rows still own KV pages and the activation buffers");
    // sequence b = the ones of mask row b (real token i sits at position i), staged for page-table row b
    std::vector<StageSeq> seqs(B);
    std::vector<int> len(B, 0);
    size_t need = 0;
    for (int b = 0; b < B; ++b) {
        TRY(mask_ones_then_zeros(mask + (size_t)b * T, T, b, &len[b]));
        seqs[b] = StageSeq{ids + (size_t)b * T * 8, len[b], b, false, labels ? labels + (size_t)b * T * 8 : nullptr};
        need += (size_t)pages_for(len[b]);
    }
    const int max_len = *std::max_element(len.begin(), len.end());
    for (int b = 0; labels && b < B; ++b)
        for (int t = 0; t < T; ++t)
            for (int c = 0; c < 8; ++c) {
                const int64_t V = c == 0 ? e->V0 : e->Vs, lb = labels[((size_t)b * T + t) * 8 + c];
                if (lb == -100) continue;
                if (t >= len[b]) return fail(MTTS_EINVAL, "label %lld at a masked position (row %d, position %d, channel %d)", (long long)lb, b, t, c);
                if (lb < 0 || lb >= V) return fail(MTTS_EINVAL, "label %lld outside [0, %lld) on channel %d", (long long)lb, (long long)V, c);
            }
    StagedRows sr;
    TRY(stage_rows(seqs, e->V0, e->Vs, true, &sr));
    const size_t Mpad = sr.Mpad;
    const std::vector<size_t>& row0 = sr.row0;
    // pages: the need is checked against the pool before anything is launched
    if (need > (size_t)e->pool.free_count())
        return fail(MTTS_ENOMEM, "scoring needs %zu KV pages, the pool has %zu free (%d pages of %d tokens)", need, (size_t)e->pool.free_count(), e->total_pages, MTTS_PAGE);
    if (Mpad > e->sc_cap_rows) {       // (the sc_* buffers below: read by scoring passes, never by a decode step)
        e->mem.release(e->d_sc_labels); e->mem.release(e->d_sc_logp);
        e->sc_cap_rows = 0;
        TRY(e->mem.get(&e->d_sc_labels, Mpad * 8, false));
        TRY(e->mem.get(&e->d_sc_logp, Mpad * 8, false));
        e->sc_cap_rows = Mpad;
    }
    if (!e->f32 && !e->sc_part)
        TRY(e->mem.get(&e->sc_part, head_ce_part_elems(MTTS_PFCAP, e->V0, 1) + head_ce_part_elems(MTTS_PFCAP, e->Vs, 7), false));
    if (e->f32 && !e->sc_logits) TRY(e->mem.get(&e->sc_logits, (size_t)SCORE_F32_ROWS * e->V0_pad, false));
    if (k > 0) {                       // top-k only: the staged results, and on the bf16 engine the blocks' candidates (head 0's is the larger need)
        if (Mpad * 8 * k > e->sc_top_cap) {
            e->mem.release(e->d_sc_top_ids); e->mem.release(e->d_sc_top_logp);
            e->sc_top_cap = 0;
            TRY(e->mem.get(&e->d_sc_top_ids, Mpad * 8 * k, false));
            TRY(e->mem.get(&e->d_sc_top_logp, Mpad * 8 * k, false));
            e->sc_top_cap = Mpad * 8 * k;
        }
        if (!e->f32 && !e->sc_cand)
            TRY(e->mem.get(&e->sc_cand, std::max(head_topk_cand_elems(MTTS_PFCAP, e->V0, 1, MTTS_SCORE_MAX_TOPK),
                                                 head_topk_cand_elems(MTTS_PFCAP, e->Vs, 7, MTTS_SCORE_MAX_TOPK)), false));
    }
    // Sequence b borrows page-table row b.  The last run has ended, but a row may still list pages of it (they go back
    // with the next mtts_begin): those entries are set aside and put back, and the borrowed pages return to the free
    // list in the reverse of the order they were taken in, so the pool -- counts and page numbering -- is as before.
    struct Borrow {
        MttsEngine* e; hipStream_t st;
        KvPool::Kept kept;
        Borrow(MttsEngine* e_, int B_, hipStream_t st_) : e(e_), st(st_), kept(e_->pool.set_aside(B_)) {}
        // Every return path: first wait for what was enqueued (launches that touch the borrowed pages, copies from the
        // caller's host vectors), then give the pages back, restore the rows and wait for the device table to follow.
        int end() {
            if (done) return rc;
            done = true;
            auto note = [&](int r) { if (!rc) rc = r; };
            if (hipStreamSynchronize(st) != hipSuccess) note(fail(MTTS_EHIP, "mtts_score: the stream failed while the pass ran"));
            note(e->pool.restore(kept, ship_on(e, st)));
            if (hipStreamSynchronize(st) != hipSuccess) note(fail(MTTS_EHIP, "mtts_score: restoring the page table failed"));
            return rc;
        }
        ~Borrow() {                    // (an error return: the error that caused it is the one reported)
            const std::string keep = g_err;
            end();
            snprintf(g_err, sizeof(g_err), "%s", keep.c_str());
        }
        bool done = false; int rc = 0;
    } borrow(e, B, st);
    const auto ship = ship_on(e, st);
    for (int b = 0; b < B; ++b) TRY(e->pool.grow(b, pages_for(len[b]), ship));
    TRY(e->pool.flush(ship));
    TRY(upload_staged(e, sr, true, st));
    HIPCHK(hipMemcpyAsync(e->d_sc_labels, sr.labs.data(), Mpad * 8 * 4, hipMemcpyHostToDevice, st));
    {
        NoSeal ns(e);
        const size_t pfcap = e->f32 ? MTTS_PF32CAP : MTTS_PFCAP;
        const int pages_bound = std::max(1, pages_for(max_len));
        for (size_t off = 0; off < Mpad; off += pfcap) {
            const int rows = (int)std::min<size_t>(pfcap, Mpad - off);
            TRY(forward_staged(e, e->d_pf_tokens + off * 8, e->d_pf_meta + off, rows, pages_bound, 0, false, st));
            if (k > 0)
                TRY(score_pass(e, e->d_sc_labels + off * 8, labels ? e->d_sc_logp + off * 8 : nullptr, rows, st, k,
                               e->d_sc_top_ids + off * 8 * k, e->d_sc_top_logp + off * 8 * k));
            else TRY(score_pass(e, e->d_sc_labels + off * 8, e->d_sc_logp + off * 8, rows, st));
        }
    }
    std::vector<float> lp(labels ? Mpad * 8 : 0), tlp(Mpad * 8 * k);
    std::vector<int32_t> tid(Mpad * 8 * k);
    if (labels) HIPCHK(hipMemcpyAsync(lp.data(), e->d_sc_logp, Mpad * 8 * sizeof(float), hipMemcpyDeviceToHost, st));
    if (k > 0) {
        HIPCHK(hipMemcpyAsync(tid.data(), e->d_sc_top_ids, tid.size() * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(tlp.data(), e->d_sc_top_logp, tlp.size() * sizeof(float), hipMemcpyDeviceToHost, st));
    }
    TRY(borrow.end());                 // drains st: the copies have landed, the pool and both page tables are as before
    // logp[b][t] = what the row of position t - 1 computed; NaN at t = 0, at ignored labels and at padding
    const float nanv = __builtin_nanf("");
    if (labels) {
        for (size_t i = 0; i < (size_t)B * T * 8; ++i) host_logp[i] = nanv;
        for (int b = 0; b < B; ++b)
            for (int t = 1; t < len[b]; ++t)
                memcpy(host_logp + ((size_t)b * T + t) * 8, lp.data() + (row0[b] + t - 1) * 8, 8 * sizeof(float));
    }
    if (k > 0) {                       // the same slots, whatever their label; -1 / NaN elsewhere
        for (size_t i = 0; i < (size_t)B * T * 8 * k; ++i) { host_top_ids[i] = -1; host_top_logp[i] = nanv; }
        for (int b = 0; b < B; ++b)
            for (int t = 1; t < len[b]; ++t) {
                memcpy(host_top_ids + ((size_t)b * T + t) * 8 * k, tid.data() + (row0[b] + t - 1) * 8 * k, (size_t)8 * k * sizeof(int32_t));
                memcpy(host_top_logp + ((size_t)b * T + t) * 8 * k, tlp.data() + (row0[b] + t - 1) * 8 * k, (size_t)8 * k * sizeof(float));
            }
    }
    return MTTS_OK;
}

int32_t mtts_score(MttsEngine* e, const int64_t* ids, const uint8_t* mask, const int64_t* labels, int32_t B, int32_t T,
                   float* host_logp, void* stream) {
    if (!labels || !host_logp) return fail(MTTS_EINVAL, "null argument");
    return score_call(e, ids, mask, labels, B, T, host_logp, 0, nullptr, nullptr, stream);
}

int32_t mtts_score_topk(MttsEngine* e, const int64_t* ids, const uint8_t* mask, const int64_t* labels, int32_t B, int32_t T,
                        float* host_logp, int32_t k, int32_t* host_top_ids, float* host_top_logp, void* stream) {
    if (!host_top_ids || !host_top_logp) return fail(MTTS_EINVAL, "null argument");
    if (!labels != !host_logp) return fail(MTTS_EINVAL, "mtts_score_topk: host_labels and host_logp are given together or both null");
    if (k < 1 || k > MTTS_SCORE_MAX_TOPK) return fail(MTTS_EINVAL, "mtts_score_topk: k %d outside 1..%d", k, MTTS_SCORE_MAX_TOPK);
    return score_call(e, ids, mask, labels, B, T, host_logp, k, host_top_ids, host_top_logp, stream);
}

int32_t mtts_read_logits_f32(MttsEngine* e, float* l0, float* l17, void* stream) {
    if (!e || !e->began) return fail(MTTS_ESTATE, "mtts_begin has not run");
    if (!e->f32) return fail(MTTS_ESTATE, "bf16 engine: use mtts_read_logits");
    return read_logits(e, l0, l17, stream);
}

int32_t mtts_read_logits(MttsEngine* e, uint16_t* l0, uint16_t* l17, void* stream) {
    if (!e || !e->began) return fail(MTTS_ESTATE, "mtts_begin has not run");
    if (e->f32) return fail(MTTS_ESTATE, "fp32 engine: use mtts_read_logits_f32");
    return read_logits(e, l0, l17, stream);
}

int32_t mtts_generate(MttsEngine* e, const int64_t* ids, const uint8_t* mask, int32_t B, int32_t T, int32_t max_length,
                      const MttsSamplerCfg* sampler, uint64_t seed, int64_t* out, int32_t out_capacity, int32_t* out_len,
                      const int64_t* forced, int32_t forced_len, int64_t* decisions, void* stream) {
    if (!e) return fail(MTTS_EINVAL, "null argument");
    RunOptions opt;
    TRY(take_options(e, B, forced != nullptr, &opt));
    if (!out || !out_len) return fail(MTTS_EINVAL, "null output");
    TRY(begin_run(e, ids, mask, B, T, max_length, sampler, seed, opt, stream));
    hipStream_t st = S(stream);
    const int takes = opt.takes;
    const int base = e->base_length;
    const int R = e->B;
    if (forced) {
        if (!decisions) return fail(MTTS_EINVAL, "forced replay needs host_decisions");
        std::vector<int32_t> f((size_t)e->cfg.max_batch * e->bufs.gen_cap * 8, -1);
        for (int s = 0; s < e->max_steps && base + s < forced_len; ++s)
            for (int b = 0; b < B; ++b)
                for (int c = 0; c < 8; ++c) {
                    int64_t tk = forced[((size_t)b * forced_len + base + s) * 8 + c];
                    if (tk < 0 || tk >= (c == 0 ? e->V0 : e->Vs)) return fail(MTTS_EINVAL, "forced token %lld out of range on channel %d", (long long)tk, c);
                    f[((size_t)b * e->bufs.gen_cap + s) * 8 + c] = (int32_t)tk;
                }
        HIPCHK(hipMemcpy(e->bufs.d_forced, f.data(), f.size() * 4, hipMemcpyHostToDevice));
        e->has_forced = true;
        e->max_steps = std::min(e->max_steps, forced_len - base);
    }
    // run ahead of the device in small batches; once every dialogue has finished the device marks all rows idle and
    // the steps still in flight do no attention and change no state
    int done = 0, steps = 0;
    while (!done && e->steps_issued < e->max_steps) {
        TRY(issue_steps(e, 8, st));
        TRY(mtts_sync_state(e, &steps, &done, stream));
    }
    TRY(mtts_sync_state(e, &steps, &done, stream));
    if (!forced && !done)
        return fail(MTTS_ESTATE, "the batch is still flushing after %d steps (%d past max_length): chained finished-row "
                    "resurrections (modeling_asteroid.py:140-141,168) outran the room max_seq_len %d leaves; raise it by %d",
                    steps, steps - (max_length - base), e->cfg.max_seq_len, linger_bound(R) - LINGER_STEPS);
    const int total = base + steps;
    if (total > out_capacity) return fail(MTTS_EINVAL, "out_capacity %d < %d", out_capacity, total);
    std::vector<int64_t> gen((size_t)std::max(steps, 1) * R * 8);
    int ns = 0;
    TRY(read_rows(e, e->bufs.d_gen, gen.data(), steps, &ns));
    for (int b = 0; b < R; ++b) {
        const int p = b / takes;       // the row's prompt
        for (int t = 0; t < base; ++t)
            for (int c = 0; c < 8; ++c) out[((size_t)b * out_capacity + t) * 8 + c] = ids[((size_t)p * T + t) * 8 + c];
        for (int s = 0; s < steps; ++s)
            for (int c = 0; c < 8; ++c) out[((size_t)b * out_capacity + base + s) * 8 + c] = gen[((size_t)s * R + b) * 8 + c];
    }
    if (decisions) TRY(read_rows(e, e->bufs.d_declog, decisions, steps, &ns));
    *out_len = total;
    e->run_open = false;               // (a forced replay may stop before every row has finished)
    return MTTS_OK;
}

// Per-sequence loop state (needs_additional_steps, unfinished, tokens in the KV cache) after the steps issued so far.
int32_t mtts_read_seq_state(MttsEngine* e, int32_t* host_nas, int32_t* host_unfinished, int32_t* host_kv_len, void* stream) {
    if (!e || !e->began) return fail(MTTS_ESTATE, "mtts_begin has not run");
    HIPCHK(hipSetDevice(e->device));
    std::vector<SeqState> ss(MTTS_RCAP);
    HIPCHK(hipMemcpyAsync(ss.data(), e->d_seqs, ss.size() * sizeof(SeqState), hipMemcpyDeviceToHost, S(stream)));
    HIPCHK(hipStreamSynchronize(S(stream)));
    for (int b = 0; b < e->B; ++b) {
        if (host_nas) host_nas[b] = ss[b].nas;
        if (host_unfinished) host_unfinished[b] = ss[b].unfinished;
        if (host_kv_len) host_kv_len[b] = ss[b].kv_len;
    }
    return MTTS_OK;
}

// ---- continuous batching: per-slot dialogues ---------------------------------------------------------
// mtts_sched_open(e, B, sampler): B slots, all empty.  mtts_slot_submit(): prefill ONE dialogue into an empty slot
// while the others keep their state.  mtts_step() then advances every occupied slot by one frame; a dialogue that
// finishes leaves the batch at once (no finished-row padding) and its slot can be refilled.
int32_t mtts_sched_open(MttsEngine* e, int32_t B, int32_t gen_cap, const MttsSamplerCfg* sampler, void* stream) {
    if (!e) return fail(MTTS_EINVAL, "null argument");
    const std::vector<float> typical = e->pending.take_typical();
    const std::vector<MttsSamplerFloors> floors = e->pending.take_floors();     // the one-shots leave first: consumed whatever follows
    const RunBans bans = e->pending.take_bans();
    const RunBias bias = e->pending.take_bias();
    if (!sampler) return fail(MTTS_EINVAL, "null argument");
    TRY(mtts_weights_ready(e));
    HIPCHK(hipSetDevice(e->device));
    hipStream_t st = S(stream);
    if (B < 1 || B > e->cfg.max_batch) return fail(MTTS_EINVAL, "batch %d exceeds max_batch %d", B, e->cfg.max_batch);
    if (gen_cap < 8) return fail(MTTS_EINVAL, "gen_cap too small");
    e->scores_on = e->pending.output_scores; e->topk_on = e->pending.top_logprobs;      // the sticky switches only
    TRY(start_outputs(e, gen_cap, st));
    TRY(start_bans(e, bans, bias, st));
    e->B = B; e->steps_issued = 0; e->has_forced = false; e->continuous = true; e->split_phase = 0;
    e->max_steps = 1 << 30;
    e->n_real.assign(B, 0);
    e->max_real = 0;
    HIPCHK(hipStreamSynchronize(st));
    e->pool.release_all();
    std::fill(e->slot_live.begin(), e->slot_live.end(), 0);
    TRY(pack_policy_reset(e, st));
    std::fill(e->seq_adapter.begin(), e->seq_adapter.end(), -1);
    if (e->bufs.d_seq_adapter) HIPCHK(hipMemsetAsync(e->bufs.d_seq_adapter, 0xff, MTTS_RCAP * sizeof(int32_t), st));
    TRY(reset_run_state(e, std::vector<SeqState>(MTTS_RCAP, IDLE_SEQ), true, sampler, floors, typical, st));
    e->began = true;
    e->run_open = true;
    return MTTS_OK;
}

// host_ids int64 [T][8] (one delay-shifted prompt, no padding), max_length in its own padded-slot units (T + max_new).
int32_t mtts_slot_submit(MttsEngine* e, int32_t slot, const int64_t* ids, int32_t T, int32_t max_length, uint64_t seed,
                         void* stream) {
    return mtts_slot_submit_row(e, slot, ids, T, max_length, seed, 0, stream);
}

// Philox row ids for the rows of the NEXT mtts_begin / mtts_generate (consumed by it): row b draws from counter
// (step, host_row_ids[b], channel, 0).  Default 0..B-1.  Lets one rank's share of a sharded batch, or one chunk of a
// large one, draw exactly what its rows would draw inside the whole batch.
int32_t mtts_set_row_ids(MttsEngine* e, const int32_t* host_row_ids, int32_t n) {
    if (!e || (n > 0 && !host_row_ids) || n < 0 || n > MTTS_RCAP) return fail(MTTS_EINVAL, "set_row_ids: bad argument");
    e->pending.set_row_ids(host_row_ids, n);
    return MTTS_OK;
}

int32_t mtts_slot_submit_row(MttsEngine* e, int32_t slot, const int64_t* ids, int32_t T, int32_t max_length, uint64_t seed,
                             int32_t row_id, void* stream) {
    if (!e || !e->began || !e->continuous || !ids) return fail(MTTS_ESTATE, "mtts_sched_open has not run");
    HIPCHK(hipSetDevice(e->device));
    hipStream_t st = S(stream);
    if (slot < 0 || slot >= e->B) return fail(MTTS_EINVAL, "slot %d out of range", slot);
    const int adapter = e->pending.take_slot_adapter(slot);     // mtts_set_slot_adapter: consumed by this call, whatever its outcome
    TRY(adapter_id_check(e, adapter, "slot", slot));
    if (T < 8) return fail(MTTS_EINVAL, "T must be >= 8");
    const int base = T - 7, n = base;
    if (max_length <= base) return fail(MTTS_EINVAL, "max_length leaves no room to generate");
    const int max_new = max_length - base + FLUSH_STEPS;      // incl. a delay-pattern flush that starts at max_length
    if (max_new > e->bufs.gen_cap) return fail(MTTS_EINVAL, "dialogue may run %d steps, slot storage holds %d", max_new, e->bufs.gen_cap);
    if (pages_for(n + max_new) > e->max_pages) return fail(MTTS_ENOMEM, "dialogue needs more KV pages than a sequence may hold");
    if (n + max_new > e->bufs.rope_rows) return fail(MTTS_EINVAL, "rope table too short");
    HIPCHK(hipStreamSynchronize(st));
    {   // the slot must be empty
        SeqState cur;
        HIPCHK(hipMemcpy(&cur, e->d_seqs + slot, sizeof(cur), hipMemcpyDeviceToHost));
        if (cur.active) return fail(MTTS_ESTATE, "slot %d is occupied", slot);
    }
    // admission: the prompt's pages plus the page its first step may open must be free now
    if (e->slot_live[slot]) { e->slot_live[slot] = 0; e->pool.release(slot); }      // finished, not collected yet
    if (e->pool.free_count() < pages_for(n + 1))
        return fail(MTTS_ENOMEM, "KV page pool: %d pages free, the prompt needs %d", e->pool.free_count(), pages_for(n + 1));
    const auto ship = ship_on(e, st);
    TRY(e->pool.grow(slot, pages_for(n), ship));
    TRY(e->pool.flush(ship));
    StagedRows sr;
    std::vector<uint32_t> bm((size_t)8 * e->bm_words, 0u);
    std::vector<int32_t> tf(7 * 8, 0);
    TRY(stage_rows({StageSeq{ids, n, slot, true, nullptr}}, e->V0, e->Vs, false, &sr));
    TRY(stage_tail(ids + (size_t)n * 8, e->V0, e->Vs, "", tf.data()));
    stage_bitmap(ids, n, e->bm_words, bm.data());
    std::vector<int32_t> hist;
    if (e->hist_on) TRY(upload_history(e, slot, ids, n, hist, false, st));
    TRY(upload_staged(e, sr, false, st));
    HIPCHK(hipMemcpy(e->d_bitmaps + (size_t)slot * 8 * e->bm_words, bm.data(), bm.size() * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(e->d_tf + (size_t)slot * 7 * 8, tf.data(), tf.size() * 4, hipMemcpyHostToDevice));
    TRY(set_seq_adapter(e, slot, adapter, st));
    TRY(prefill_staged(e, sr.Mpad, pages_for(n), 0, adapter >= 0, st));
    // logits of the dialogue's last prompt token only: heads on a one-row activation tile, copied into its slot
    // (the other slots' logits belong to dialogues that are mid-flight)
    if (e->f32) {            // fp32 engine: the GEMV writes the slot's logits rows directly
        const float* xin = e->hlast_f + (size_t)slot * e->H;
        launch_f32_linear(e->embf[0], xin, (float*)e->logits0 + (size_t)slot * e->V0_pad, 1, e->V0, e->H, e->V0_pad, e->h16, true, st);
        for (int c = 1; c < 8; ++c)
            launch_f32_linear(e->embf[c], xin, (float*)e->logits17 + (size_t)slot * 7 * e->Vs_pad + (size_t)(c - 1) * e->Vs_pad, 1, e->Vs,
                              e->H, 7 * e->Vs_pad, e->h16, true, st);
    } else {
    HIPCHK(hipMemsetAsync(e->xh, 0, (size_t)MTTS_MAXR * e->H * 2, st));
    launch_pack_rows((const uint16_t*)e->hlast + (size_t)slot * e->H, e->xh, 1, e->H, 1, st);
    launch_gemm(EPI_BF16, 1, e->p_h0, e->head0, e->xh, e->H, e->V0_pad, e->V0, nullptr, (uint16_t*)e->join_logits0, st);
    launch_gemm(EPI_BF16, 1, e->p_h17, e->heads17, e->xh, e->H, 7 * e->Vs_pad, 7 * e->Vs_pad, nullptr, (uint16_t*)e->join_logits17, st);
    HIPCHK(hipMemcpyAsync((uint16_t*)e->logits0 + (size_t)slot * e->V0_pad, e->join_logits0, (size_t)e->V0 * 2, hipMemcpyDeviceToDevice, st));
    HIPCHK(hipMemcpyAsync((uint16_t*)e->logits17 + (size_t)slot * 7 * e->Vs_pad, e->join_logits17, (size_t)7 * e->Vs_pad * 2, hipMemcpyDeviceToDevice, st));
    }
    SeqState ns{-1, 1, n, 0, base, max_length, row_id, 1, seed};
    HIPCHK(hipMemcpyAsync(e->d_seqs + slot, &ns, sizeof(ns), hipMemcpyHostToDevice, st));
    int32_t zero = 0;
    HIPCHK(hipMemcpyAsync(&e->d_ls->done, &zero, 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipStreamSynchronize(st));
    e->n_real[slot] = n - e->steps_issued;          // so that n_real + steps_issued is this dialogue's current length
    e->join_step[slot] = e->steps_issued;
    e->slot_live[slot] = 1;
    return MTTS_OK;
}

// Take of a just-submitted dialogue: dst starts where src starts (same prompt, KV, logits, history, teacher-forcing tail)
// and draws from (seed; step, row_id, channel).  src's complete prompt pages are shared (KvPool::share), its partially filled
// last page is copied into one fresh page; everything rides `stream` (one fork_kernel launch, one state upload).
int32_t mtts_slot_fork(MttsEngine* e, int32_t src, int32_t dst, uint64_t seed, int32_t row_id, void* stream) {
    if (!e || !e->began || !e->continuous) return fail(MTTS_ESTATE, "mtts_sched_open has not run");
    if (src < 0 || src >= e->B || dst < 0 || dst >= e->B || src == dst) return fail(MTTS_EINVAL, "fork: slots %d -> %d out of range", src, dst);
    HIPCHK(hipSetDevice(e->device));
    hipStream_t st = S(stream);
    // src must have been submitted since the last mtts_step: its last prompt page has not been written past the prompt
    if (!e->slot_live[src] || e->join_step[src] != e->steps_issued)
        return fail(MTTS_ESTATE, "fork: slot %d holds no dialogue submitted since the last step", src);
    HIPCHK(hipMemcpyAsync(e->h_seqs, e->d_seqs, (size_t)e->B * sizeof(SeqState), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (!e->h_seqs[src].active || e->h_seqs[src].step) return fail(MTTS_ESTATE, "fork: slot %d has stepped", src);
    if (e->h_seqs[dst].active) return fail(MTTS_ESTATE, "fork: slot %d is occupied", dst);
    if (e->slot_live[dst]) { e->slot_live[dst] = 0; e->pool.release(dst); }      // finished, not collected yet
    const int len = e->n_real[src] + e->steps_issued, full = len / MTTS_PAGE, tail = len % MTTS_PAGE != 0;
    if (e->pool.free_count() < tail)
        return fail(MTTS_ENOMEM, "KV page pool: no free page for the take's copy of the last prompt page");
    const auto ship = ship_on(e, st);
    ForkJob job;
    job.np = 0; job.nr = 1;
    job.rsrc[0] = src; job.rdst[0] = dst;
    int rc = e->pool.share(src, dst, full, ship);
    if (!rc && tail) {
        rc = e->pool.grow(dst, full + 1, ship);
        job.psrc[0] = e->pool.entry(src, full);
        job.pdst[0] = e->pool.entry(dst, full);
        job.np = 1;
    }
    if (!rc) rc = e->pool.flush(ship);
    if (!rc) rc = launch_fork_job(e, job, true, st);
    if (!rc && e->hist_on) {                        // the take's own copy of the prompt history (n-gram ban, rules); its generated part starts empty
        const size_t row = (size_t)e->bufs.hist_cap * 8;
        if (hipMemcpyAsync(e->bufs.d_hist + (size_t)dst * row, e->bufs.d_hist + (size_t)src * row, (size_t)e->h_seqs[src].base_length * 8 * 4,
                           hipMemcpyDeviceToDevice, st) != hipSuccess) rc = fail(MTTS_EHIP, "fork: copying the prompt history failed");
    }
    if (rc) { e->pool.release(dst); return rc; }    // the share is undone with the slot (counts, unshipped edits)
    SeqState ns = e->h_seqs[src];
    ns.row_id = row_id; ns.seed = seed;
    e->h_seqs[dst] = ns;                            // pinned staging of the upload
    TRY(set_seq_adapter(e, dst, e->seq_adapter[src], st));       // the shared pages hold K/V computed with src's adapter
    HIPCHK(hipMemcpyAsync(e->d_seqs + dst, e->h_seqs + dst, sizeof(SeqState), hipMemcpyHostToDevice, st));
    HIPCHK(hipStreamSynchronize(st));
    e->n_real[dst] = e->n_real[src];
    e->join_step[dst] = e->steps_issued;
    e->slot_live[dst] = 1;
    return MTTS_OK;
}

// host_state int32 [B][4] = (active, unfinished, steps generated, tokens in cache)
int32_t mtts_slot_states(MttsEngine* e, int32_t* host_state, void* stream) {
    if (!e || !e->began || !host_state) return fail(MTTS_ESTATE, "engine not started");
    HIPCHK(hipSetDevice(e->device));
    std::vector<SeqState> ss(MTTS_RCAP);
    HIPCHK(hipMemcpyAsync(ss.data(), e->d_seqs, ss.size() * sizeof(SeqState), hipMemcpyDeviceToHost, S(stream)));
    HIPCHK(hipStreamSynchronize(S(stream)));
    for (int b = 0; b < e->B; ++b) {
        host_state[b * 4 + 0] = ss[b].active; host_state[b * 4 + 1] = ss[b].unfinished;
        host_state[b * 4 + 2] = ss[b].step; host_state[b * 4 + 3] = ss[b].kv_len;
        // a dialogue that has left the batch (scheduler mode) gives its pages back: the stream is idle, nothing
        // in flight reads them
        if (e->continuous && e->slot_live[b] && !ss[b].active) { e->slot_live[b] = 0; e->pool.release(b); e->seq_adapter[b] = -1; }
    }
    return MTTS_OK;
}

int32_t mtts_slot_evict(MttsEngine* e, int32_t slot, void* stream) {
    if (!e || !e->began || !e->continuous) return fail(MTTS_ESTATE, "mtts_sched_open has not run");
    if (slot < 0 || slot >= e->B) return fail(MTTS_EINVAL, "slot %d out of range", slot);
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipStreamSynchronize(S(stream)));
    SeqState cur;
    HIPCHK(hipMemcpy(&cur, e->d_seqs + slot, sizeof(cur), hipMemcpyDeviceToHost));
    cur.active = 0; cur.unfinished = 0;
    HIPCHK(hipMemcpy(e->d_seqs + slot, &cur, sizeof(cur), hipMemcpyHostToDevice));
    RowMeta idle{-1, 0, 0, 0};
    HIPCHK(hipMemcpy(e->d_meta + slot, &idle, sizeof(idle), hipMemcpyHostToDevice));
    if (e->slot_live[slot]) { e->slot_live[slot] = 0; e->pool.release(slot); }
    e->seq_adapter[slot] = -1;                      // (the host's copy picks the step's launches; the device's is rewritten by the next submit)
    return MTTS_OK;
}

int32_t mtts_kv_pool_state(MttsEngine* e, int32_t* total_pages, int32_t* n_free, int32_t* max_pages_per_seq) {
    if (!e) return fail(MTTS_EINVAL, "null engine");
    if (total_pages) *total_pages = e->total_pages;
    if (n_free) *n_free = e->pool.free_count();
    if (max_pages_per_seq) *max_pages_per_seq = e->max_pages;
    return MTTS_OK;
}

int32_t mtts_read_page_table(MttsEngine* e, int32_t* host_table, int32_t* host_counts) {
    if (!e || !host_table || !host_counts) return fail(MTTS_EINVAL, "null argument");
    memcpy(host_table, e->pool.table().data(), e->pool.table().size() * 4);
    memcpy(host_counts, e->pool.counts().data(), e->pool.counts().size() * 4);
    return MTTS_OK;
}

// verification hook: the page table as the DEVICE holds it (after everything queued on `stream`)
int32_t mtts_debug_read_device_page_table(MttsEngine* e, int32_t* host_table, void* stream) {
    if (!e || !host_table) return fail(MTTS_EINVAL, "null argument");
    HIPCHK(hipSetDevice(e->device));
    TRY(e->pool.flush(ship_on(e, S(stream))));
    HIPCHK(hipMemcpyAsync(host_table, e->d_page_table, e->pool.table().size() * 4, hipMemcpyDeviceToHost, S(stream)));
    HIPCHK(hipStreamSynchronize(S(stream)));
    return MTTS_OK;
}

int32_t mtts_set_forced_mode(MttsEngine* e, int32_t as_draw) {
    if (!e) return fail(MTTS_EINVAL, "null engine");
    if (as_draw < 0 || as_draw > 2) return fail(MTTS_EINVAL, "forced mode must be 0, 1 or 2");
    e->forced_draw = as_draw;
    return MTTS_OK;
}

// generated rows of one slot: host_rows int64 [steps][8]
int32_t mtts_slot_read(MttsEngine* e, int32_t slot, int64_t* host_rows, int32_t capacity_steps, int32_t* n_steps) {
    if (!e || !e->began || !host_rows || slot < 0 || slot >= e->B) return fail(MTTS_EINVAL, "bad argument");
    return slot_read(e, e->bufs.d_gen, slot, host_rows, capacity_steps, n_steps);
}

// log-probabilities of one slot's generated rows: host_rows float [steps][8]
int32_t mtts_slot_read_scores(MttsEngine* e, int32_t slot, float* host_rows, int32_t capacity_steps, int32_t* n_steps) {
    if (!e || !e->began || !host_rows || slot < 0 || slot >= e->B) return fail(MTTS_EINVAL, "bad argument");
    if (!e->scores_on) return fail(MTTS_ESTATE, "the run was started with output_scores off (mtts_set_output_scores)");
    return slot_read(e, e->bufs.d_lp, slot, host_rows, capacity_steps, n_steps);
}

// the same of one slot's generated rows: host_logp float [steps][8], host_top_ids int32 / host_top_logp float [steps][8][k]
int32_t mtts_slot_read_top_logprobs(MttsEngine* e, int32_t slot, float* host_logp, int32_t* host_top_ids, float* host_top_logp,
                                    int32_t capacity_steps, int32_t* n_steps) {
    if (!e || !e->began || !host_logp || !host_top_ids || !host_top_logp || slot < 0 || slot >= e->B) return fail(MTTS_EINVAL, "bad argument");
    if (!e->topk_on) return fail(MTTS_ESTATE, "the run was started with top_logprobs off (mtts_set_top_logprobs)");
    TRY(slot_read(e, e->bufs.d_gt_logp, slot, host_logp, capacity_steps, n_steps));
    TRY(slot_read(e, e->bufs.d_gt_ids, slot, host_top_ids, capacity_steps, n_steps, 8 * e->topk_on));
    return slot_read(e, e->bufs.d_gt_tlp, slot, host_top_logp, capacity_steps, n_steps, 8 * e->topk_on);
}

// Frames first..first+n-1 of every sequence as codec codes int64 [8][B][n] on the device (delay pattern undone,
// channel-0 offset removed): lets the codec decode windows while the decode loop is still running.  The caller
// orders `stream` after the steps that produced frame first+n+6 (event / same stream).
int32_t mtts_export_codes(MttsEngine* e, int32_t first, int32_t n, int64_t* dev_codes, void* stream) {
    if (!e || !e->began || !dev_codes) return fail(MTTS_ESTATE, "nothing generated");
    if (first < 0 || n < 1 || first + n + 7 > e->steps_issued) return fail(MTTS_EINVAL, "frames %d..%d need %d issued steps, have %d", first, first + n - 1, first + n + 7, e->steps_issued);
    HIPCHK(hipSetDevice(e->device));
    launch_export_codes(e->bufs.d_gen, dev_codes, e->B, first, n, e->cfg.speech_range_lo, e->cfg.speech_vocab_size - 2, e->bufs.gen_cap, S(stream));
    HIPCHK(hipGetLastError());
    return MTTS_OK;
}

int32_t mtts_profile_enable(MttsEngine* e, int32_t on) {
    if (!e) return fail(MTTS_EINVAL, "null engine");
    e->prof = on != 0;
    for (int w = 0; w < PROF_N; ++w) {
        for (auto& pr : e->ev[w]) { hipEventDestroy(pr.first); hipEventDestroy(pr.second); }
        e->ev[w].clear();
        e->prof_bytes[w] = 0;
    }
    return MTTS_OK;
}

int32_t mtts_profile_read(MttsEngine* e, int32_t which, double* total_ms, int64_t* launches, int64_t* bytes) {
    if (!e || which < 0 || which >= PROF_N) return fail(MTTS_EINVAL, "bad profile slot");
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipDeviceSynchronize());
    double tot = 0;
    for (auto& pr : e->ev[which]) {
        float ms = 0;
        HIPCHK(hipEventElapsedTime(&ms, pr.first, pr.second));
        tot += ms;
    }
    if (total_ms) *total_ms = tot;
    if (launches) *launches = (int64_t)e->ev[which].size();
    if (bytes) *bytes = e->prof_bytes[which];
    return MTTS_OK;
}

