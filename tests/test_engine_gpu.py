"""HIP engine (through the C ABI) vs the oracle and the reference-generated fixtures.  -m gpu."""
import ctypes as C
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from mtts import capi, synth  # noqa: E402
from oracle import asteroid_oracle as ao  # noqa: E402

CASES = ["ar_text_ragged", "ar_flush0", "ar_audio_tail", "ar_gqa4", "ar_rep_penalty", "ar_flush_past_max", "ar_wide"]
# relative top-2 gap from which a decision must be identical: 2 bf16 ulps (one ulp is 2^-8..2^-7 of the value).  Below it
# the count of agreeing decisions is pinned instead (test_parity_scale_gpu.py::test_parity_decision_counts).
MARGIN_OK = 0.008
# Runs whose expected ids come from the numpy ORACLE (not from a reference fixture): oracle and engine each sum their dot
# products in an order of their own, so a logit may sit one bf16 ulp off the reference's in either of them, in opposite
# directions, and a two-ulp gap can flip; there the gate stays at ~5 ulps.
MARGIN_ORACLE = 0.02


def _bf16_t(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(torch.bfloat16).cuda()


def test_gemm_kernel_matches_fp32_reference():
    rng = np.random.default_rng(0)
    lib = capi.lib()
    for (M, N, K, ks) in [(32, 1024, 256, 0), (5, 4096, 2048, 0), (32, 2048, 6144, 4), (17, 1025, 512, 1), (32, 96, 64, 1),
                          (100, 1024, 512, 0), (128, 2048, 2048, 2), (64, 4096, 256, 1),
                          # > 128 rows: the tiled prefill kernel (128 x 128 blocks), ragged rows / columns, split-K
                          (512, 2048, 2048, 0), (384, 4096, 512, 1), (200, 1025, 512, 2), (160, 96, 64, 1), (512, 256, 6144, 4)]:
        w = ao.round_bf16(rng.standard_normal((N, K)).astype(np.float32) * 0.05)
        x = ao.round_bf16(rng.standard_normal((M, K)).astype(np.float32))
        wt, xt = _bf16_t(w), _bf16_t(x)
        y = torch.zeros(M, N, dtype=torch.bfloat16, device="cuda")
        capi.check(lib.mtts_k_gemm_bf16(wt.data_ptr(), xt.data_ptr(), y.data_ptr(), M, N, K, ks, None))
        torch.cuda.synchronize()
        ref = x.astype(np.float64) @ w.T.astype(np.float64)
        got = y.float().cpu().numpy()
        # bf16 output: half an ulp of rounding + fp32 accumulation noise
        np.testing.assert_allclose(got, ref, rtol=2 ** -8, atol=2e-3 * np.abs(ref).max())
        exact = (got == ao.round_bf16(ref.astype(np.float32))).mean()
        assert exact > 0.98, (M, N, K, exact)


def test_rmsnorm_kernel_bit_exact_vs_oracle():
    """mtts_k_rmsnorm launches rmsnorm_rows_kernel, a test-only entry point that the engine never launches.  The
    RMSNorms the engine runs (embed_norm_kernel, resid_norm_kernel, the norm prologue of gemv_small_kernel) are covered by
    test_layer_kernels_gpu.py: test_embed_norm_kernel, test_resid_norm_kernel, test_gemv_small_norm_prologue_identity."""
    rng = np.random.default_rng(1)
    lib = capi.lib()
    for rows, n in [(3, 256), (32, 2048), (7, 128)]:
        x = ao.round_bf16(rng.standard_normal((rows, n)).astype(np.float32) * 3)
        w = ao.round_bf16(1 + 0.1 * rng.standard_normal(n).astype(np.float32))
        xt, wt = _bf16_t(x), _bf16_t(w)
        y = torch.zeros(rows, n, dtype=torch.bfloat16, device="cuda")
        capi.check(lib.mtts_k_rmsnorm(xt.data_ptr(), wt.data_ptr(), y.data_ptr(), rows, n, 1e-6, None))
        torch.cuda.synchronize()
        orc = ao.AsteroidOracle(synth.tiny(), {}, "bf16")
        want = orc.rmsnorm(x, w)
        got = y.float().cpu().numpy()
        assert (got == want).mean() > 0.999
        np.testing.assert_allclose(got, want, rtol=2 ** -7)


def _sample_gpu(logits, hist, lc, do_sample, mask_id, seed, step, channel):
    from mtts.engine import sampler_cfgs
    lib = capi.lib()
    rows, V = logits.shape
    lt = _bf16_t(logits)
    words = (V + 31) // 32
    bm = np.zeros((rows, words), dtype=np.uint32)
    if hist is not None:
        for b in range(rows):
            for t in hist[b]:
                bm[b, t >> 5] |= np.uint32(1 << (t & 31))
    bmt = torch.from_numpy(bm.view(np.int32)).cuda()
    cfg = sampler_cfgs([lc] * 8, [do_sample] * 8)[0]
    out = torch.zeros(rows, dtype=torch.int32, device="cuda")
    capi.check(lib.mtts_k_sample(lt.data_ptr(), rows, V, bmt.data_ptr(), C.byref(cfg), mask_id, C.c_uint64(seed),
                                 step, channel, out.data_ptr(), None))
    torch.cuda.synchronize()
    return out.cpu().numpy().astype(np.int64)


def test_sampler_kernel_vs_oracle():
    rng = np.random.default_rng(2)
    for V in (1025, 152697):
        rows = 6
        logits = ao.round_bf16(rng.standard_normal((rows, V)).astype(np.float32) * 2.5)
        hist = rng.integers(0, V, (rows, 50))
        # greedy with repetition penalty + mask
        lc = dict(repetition_penalty=1.3)
        want = np.argmax(ao.apply_processors(hist, np.where(np.arange(V)[None] == 1024, -np.inf, logits), lc), -1)
        got = _sample_gpu(logits, hist, lc, False, 1024, 0, 0, 1)
        assert np.array_equal(got, want)
        # sampling: same kept set rule + same Philox draw as the oracle, many draws
        lc = dict(repetition_penalty=1.1, temperature=0.9, top_k=50, top_p=0.9)
        sc = ao.apply_processors(hist, logits, lc)
        mism = 0
        for step in range(40):
            want = ao.sample_from_scores(sc, 1234, step, 3)
            got = _sample_gpu(logits, hist, lc, True, -1, 1234, step, 3)
            assert all(np.isfinite(sc[b, got[b]]) for b in range(rows))      # always inside the kept set
            mism += int((want != got).sum())
        assert mism <= 1, mism      # fp32-vs-fp64 cumsum can move a boundary draw (p ~ 1e-6 each)
        # no top_k (nucleus only), plain multinomial, and a top_k beyond the candidate buffer: on the big vocabulary
        # these take the full-vocabulary kernel (global-memory sort), on 1025 tokens the in-block path
        for lc in (dict(top_p=0.9), dict(temperature=1.3), dict(top_k=6000, top_p=0.97, repetition_penalty=1.2)):
            sc = ao.apply_processors(hist, logits, lc)
            mism = 0
            for step in range(12):
                want = ao.sample_from_scores(sc, 99, step, 0)
                got = _sample_gpu(logits, hist, lc, True, -1, 99, step, 0)
                mism += int((want != got).sum())
                # A nucleus over ~150 k tokens has members of 1e-6 probability: which of them sit on the top-p
                # boundary is decided by fp32 noise in the reference's own cumsum, and that moves `total` by ~1e-5.
                # So require the engine's pick to be the token whose CDF interval contains u within 1e-4 of mass.
                for b in range(rows):
                    kept = np.nonzero(np.isfinite(sc[b]))[0]
                    kept = kept[np.lexsort((kept, sc[b][kept]))[::-1]]
                    e = np.exp((sc[b][kept] - sc[b][kept].max()).astype(np.float32)).astype(np.float64)
                    cum = np.cumsum(e) / e.sum()
                    u = float(ao.philox_uniform(99, step, b, 0))
                    j = int(np.nonzero(kept == got[b])[0][0])        # raises if the pick is outside the kept set
                    lo = cum[j - 1] if j else 0.0
                    assert lo - 1e-4 <= u <= cum[j] + 1e-4, (lc, V, b, step, lo, u, cum[j])
            assert mism <= (2 if V < 5000 else 12), (lc, V, mism)


def _load_case(golden_dir, name):
    z = np.load(os.path.join(golden_dir, name + ".npz"))
    cfg = json.loads(str(z["cfg"]))
    w = synth.synth_weights(cfg, int(z["seed"]), **json.loads(str(z["wkw"])))
    return z, cfg, w


@pytest.fixture(scope="module")
def engines():
    cache = {}
    yield cache
    for e in cache.values():
        e.close()


def _engine_for(engines, cfg, w, key):
    from mtts.engine import Engine
    if key not in engines:
        e = Engine(cfg, max_batch=4, max_seq_len=256)
        e.bind_state_dict(w)
        engines[key] = e
    return engines[key]


@pytest.mark.parametrize("name", CASES)
def test_engine_replay_matches_reference_fixture(golden_dir, engines, name):
    """Teacher-forced replay of the reference's own greedy run: every decision whose
    top-2 margin in the reference is not degenerate must be identical; state-machine
    outputs (teacher forcing, EOS flush, finished padding) must be identical always."""
    z, cfg, w = _load_case(golden_dir, name)
    eng = _engine_for(engines, cfg, w, name)
    gold = z["out_ids"]
    layers = json.loads(str(z["layers"])) or None
    T = z["input_ids"].shape[1]
    out, dec = eng.generate(z["input_ids"], z["attention_mask"], int(z["max_length"]), layers=layers, forced=gold)
    assert np.array_equal(out, gold)                      # forced rows were appended
    want = gold[:, T - 7:].transpose(1, 0, 2)
    margins = z["margins"]
    assert dec.shape == want.shape
    safe = margins >= MARGIN_OK
    bad = np.argwhere(safe & (dec != want))
    assert len(bad) == 0, bad[:10]
    forced_slots = margins >= 9.0
    assert np.array_equal(dec[forced_slots], want[forced_slots])
    # low-margin decisions: agreement is expected most of the time too
    low = (~safe) & (~forced_slots)
    if low.sum():
        assert (dec[low] == want[low]).mean() > 0.5


@pytest.mark.parametrize("name", ["ar_text_ragged", "ar_audio_tail"])
def test_engine_logits_close_to_oracle(golden_dir, engines, name):
    """Step API: prefill logits and the first decode steps against the oracle, bit level."""
    z, cfg, w = _load_case(golden_dir, name)
    eng = _engine_for(engines, cfg, w, name)
    orc = ao.AsteroidOracle(cfg, w, "bf16")
    gold = z["out_ids"]
    ids, dec, logs = orc.generate(z["input_ids"], z["attention_mask"], int(z["max_length"]), forced=gold,
                                  return_logits=True, max_steps=6)
    eng.begin(z["input_ids"], z["attention_mask"], int(z["max_length"]))
    exact, total = 0, 0
    for s in range(5):
        l0, l17 = eng.read_logits()
        # oracle logs carry the -inf masks; compare the raw logits elsewhere
        for c in range(8):
            got = l0 if c == 0 else l17[c - 1]
            ref = logs[s][c]
            fin = np.isfinite(ref)
            tol = (2.0 ** -6) * np.abs(np.where(fin, ref, 0)).max(axis=-1, keepdims=True)
            assert (np.abs(np.where(fin, got - np.where(fin, ref, 0), 0)) <= tol).all(), (s, c)
            exact += int((got[fin] == ref[fin]).sum())
            total += int(fin.sum())
        eng.step(1)
        st, done = eng.sync_state()
        gen = eng.read_generated(st)
        # free-running engine vs free-running oracle may part ways on a near tie; stop comparing then
        T = z["input_ids"].shape[1]
        if not np.array_equal(gen[-1], gold[:, T - 7 + s]):
            break
    assert total > 0 and exact >= 0.3 * total, (exact, total)


def test_engine_free_run_matches_oracle(golden_dir, engines):
    """mtts_generate end to end (no forcing) equals the oracle's free run up to the first
    low-margin decision, and has the same length bookkeeping."""
    compared = 0
    for name in CASES:
        z, cfg, w = _load_case(golden_dir, name)
        eng = _engine_for(engines, cfg, w, name)
        layers = json.loads(str(z["layers"])) or None
        out = eng.generate(z["input_ids"], z["attention_mask"], int(z["max_length"]), layers=layers)
        gold = z["out_ids"]
        T = z["input_ids"].shape[1]
        low = np.nonzero((z["margins"] < MARGIN_OK).any(axis=(1, 2)))[0]
        upto = (T - 7) + (int(low[0]) if len(low) else gold.shape[1])
        n = min(upto, out.shape[1], gold.shape[1])
        assert np.array_equal(out[:, :n], gold[:, :n]), name
        assert np.array_equal(out[:, :T - 7], z["input_ids"][:, :T - 7])
        compared += n - (T - 7)
    assert compared >= 5


def test_engine_rejects_bad_inputs(golden_dir, engines):
    z, cfg, w = _load_case(golden_dir, "ar_flush0")
    eng = _engine_for(engines, cfg, w, "ar_flush0")
    ids, mask = z["input_ids"].copy(), z["attention_mask"].copy()
    mask2 = mask.copy()
    mask2[0, 5] = 0      # hole in the mask: not the left-padded form
    mask2[0, 0] = 1
    with pytest.raises(capi.MttsError):
        eng.generate(ids, mask2, int(z["max_length"]))
    with pytest.raises(capi.MttsError):
        eng.generate(ids, mask, ids.shape[1] - 7)          # no room to generate
    ids[0, -1, 1] = 5000                                   # out-of-range speech token
    with pytest.raises(capi.MttsError):
        eng.generate(ids, mask, int(z["max_length"]))


def test_engine_long_run_crosses_kv_pages_vs_oracle(engines):
    """150 steps on a tiny model: positions cross the 64-token page boundaries twice.  The oracle's own greedy run
    is replayed through the engine; every decision with a safe margin must be identical."""
    cfg = synth.tiny()
    w = synth.synth_weights(cfg, 77, emb_row_sigma=0.6, speech_boost=6.0, eos_boost=1.0)
    eng = _engine_for(engines, cfg, w, "long_run")
    ids, mask = synth.synth_prompts(cfg, 78, 2, 30, 0.4, True)
    max_length = ids.shape[1] + 150
    orc = ao.AsteroidOracle(cfg, w, "bf16")
    gold = orc.generate(ids, mask, max_length)
    margins = np.stack(orc.last_margins)                      # [steps,B,C]
    T = ids.shape[1]
    assert gold.shape[1] - (T - 7) >= 150                      # nobody flushed early
    out, dec = eng.generate(ids, mask, max_length, forced=gold)
    want = gold[:, T - 7:].transpose(1, 0, 2)
    assert dec.shape == want.shape
    free = np.ones_like(margins, dtype=bool)
    for s in range(7):
        free[s, :, s + 1:] = False                             # teacher-forced slots
    safe = free & (margins >= MARGIN_ORACLE)
    assert safe.sum() > 0.8 * free.sum()
    bad = np.argwhere(safe & (dec != want))
    assert len(bad) == 0, bad[:10]
    assert np.array_equal(dec[~free], want[~free])


@pytest.mark.parametrize("mfma_from_pages", ["0", "1000"])
def test_long_ragged_prefill_vs_oracle(monkeypatch, mfma_from_pages):
    """Prompts of 350..517 tokens, ragged, through both prefill attention paths: "0" = every prompt takes the
    tile-sharing matrix-core kernels (several 32-row tiles per dialogue, 9 pages, 5 pass-B chunks, dialogue
    boundaries inside a pass; this is the engine's default, pf_mfma_pages = 0: every prompt goes there), "1000" =
    row-by-row kernels.
    The logits after the prefill and the decisions of the following steps must match the oracle."""
    from mtts.engine import Engine
    monkeypatch.setenv("MTTS_PREFILL_MFMA_PAGES", mfma_from_pages)
    cfg = synth.tiny()
    w = synth.synth_weights(cfg, 41, emb_row_sigma=0.6, speech_boost=6.0, eos_boost=1.0)
    eng = Engine(cfg, max_batch=4, max_seq_len=1024)
    eng.bind_state_dict(w)
    ids, mask = synth.synth_prompts(cfg, 42, 3, 640, 0.4, True)
    assert mask.sum(axis=1).min() >= 300 and mask.sum(axis=1).max() > 512      # > 8 pages: two pass-B chunks
    T = ids.shape[1]
    max_length = T + 12
    orc = ao.AsteroidOracle(cfg, w, "bf16")
    gold = orc.generate(ids, mask, max_length)
    margins = np.stack(orc.last_margins)
    _, _, logs = orc.generate(ids, mask, max_length, forced=gold, return_logits=True, max_steps=2)
    eng.begin(ids, mask, max_length)
    l0, l17 = eng.read_logits()
    exact = total = 0
    for c in range(8):
        got = l0 if c == 0 else l17[c - 1]
        ref = logs[0][c]
        fin = np.isfinite(ref)
        tol = (2.0 ** -6) * np.abs(np.where(fin, ref, 0)).max(axis=-1, keepdims=True)
        assert (np.abs(np.where(fin, got - np.where(fin, ref, 0), 0)) <= tol).all(), c
        exact += int((got[fin] == ref[fin]).sum())
        total += int(fin.sum())
    assert exact >= 0.3 * total, (exact, total)
    out, dec = eng.generate(ids, mask, max_length, forced=gold)
    want = gold[:, T - 7:].transpose(1, 0, 2)
    assert dec.shape == want.shape
    safe = margins >= MARGIN_ORACLE
    bad = np.argwhere(safe & (dec != want))
    assert len(bad) == 0, bad[:10]
    eng.close()


@pytest.mark.parametrize("small", ["4", "0"])
@pytest.mark.parametrize("nq,nkv", [(2, 2), (4, 1)])
def test_gqa_group_sizes_vs_oracle(monkeypatch, nq, nkv, small):
    """GQA groups 1 (multi-head) and 4: the attention kernels (decode fused / unfused, prefill tiles) are templated on
    the group size; the reference fixtures cover 2 and 4.  Oracle's greedy run replayed, 90 steps (one page boundary),
    prompts of 70..140 tokens (three prefill tiles).  `small`: decode through the small-batch kernels (prologue-fused
    GEMMs, the default for <= 4 dialogues) or through the general ones (MTTS_SMALL_ROWS=0)."""
    from mtts.engine import Engine
    monkeypatch.setenv("MTTS_SMALL_ROWS", small)
    cfg = synth.tiny(num_attention_heads=nq, num_key_value_heads=nkv)
    w = synth.synth_weights(cfg, 81, emb_row_sigma=0.6, speech_boost=6.0, eos_boost=1.0)
    ids, mask = synth.synth_prompts(cfg, 82, 3, 140, 0.4, True)
    max_length = ids.shape[1] + 90
    orc = ao.AsteroidOracle(cfg, w, "bf16")
    gold = orc.generate(ids, mask, max_length)
    margins = np.stack(orc.last_margins)
    T = ids.shape[1]
    eng = Engine(cfg, max_batch=4, max_seq_len=320)
    eng.bind_state_dict(w)
    out, dec = eng.generate(ids, mask, max_length, forced=gold)
    eng.close()
    want = gold[:, T - 7:].transpose(1, 0, 2)
    assert dec.shape == want.shape
    safe = margins >= MARGIN_ORACLE
    assert safe.mean() > 0.8
    bad = np.argwhere(safe & (dec != want))
    assert len(bad) == 0, bad[:10]


def _rand_weights_on_gpu(cfg, seed):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    lo, hi = cfg["speech_token_range"]
    for name, shape, kind in synth.weight_shapes(cfg):
        if kind == "norm":
            t = (1.0 + 0.1 * torch.randn(shape, device="cuda", generator=g)).to(torch.bfloat16)
        else:
            t = (0.02 * torch.randn(shape, device="cuda", generator=g)).to(torch.bfloat16)
            if name.endswith("embedding_list.0.weight"):
                t[lo:hi] *= 8.0
        yield name, t


def test_full_size_batch_and_padding_invariance():
    """BASELINE dims (ASSUMED 1.7B, 28 layers), batch 32, ragged prompts: size-independent properties.
    (1) a dialogue's tokens do not depend on which other dialogues share the batch or on its row index;
    (2) extra left padding changes nothing; (3) the first 7 steps reproduce the delayed prompt tail."""
    from mtts.engine import Engine
    cfg = synth.assumed_1p7b()
    eng = Engine(cfg, max_batch=32, max_seq_len=512)
    for name, t in _rand_weights_on_gpu(cfg, 5):
        eng.bind(name, t)
    ids, mask = synth.synth_prompts(cfg, 9, 32, 72, 0.5, True)
    T = ids.shape[1]
    max_length = T + 10
    full = eng.generate(ids, mask, max_length)                 # greedy
    assert full.shape == (32, T - 7 + 17, 8)
    rows = [0, 7, 19, 31]
    sub = eng.generate(ids[rows], mask[rows], max_length)
    assert np.array_equal(sub, full[rows])
    # padding invariance: re-pad the same rows 9 slots further left
    pad_ids = np.concatenate([np.tile(ids[rows][:, :1] * 0 + np.array([cfg["pad_token_id"]] + [1024] * 7), (1, 9, 1)), ids[rows]], axis=1)
    pad_mask = np.concatenate([np.zeros((len(rows), 9)), mask[rows]], axis=1)
    padded = eng.generate(pad_ids, pad_mask, max_length + 9)
    assert np.array_equal(padded[:, 9:], full[rows])
    # delayed tail: step s (< 7) copies channels s+1.. from the prompt's last 7 slots
    for s in range(7):
        assert np.array_equal(full[:, T - 7 + s, s + 1:], ids[:, T - 7 + s, s + 1:])
    # sampling: same seed -> same tokens; different seed -> different tokens
    layers = [dict(top_k=50, top_p=0.95, temperature=1.0)] * 8
    a = eng.generate(ids, mask, max_length, layers=layers, do_samples=[True] * 8, seed=3)
    b = eng.generate(ids, mask, max_length, layers=layers, do_samples=[True] * 8, seed=3)
    c = eng.generate(ids, mask, max_length, layers=layers, do_samples=[True] * 8, seed=4)
    assert np.array_equal(a, b) and not np.array_equal(a, c)
    eng.close()


def test_decode_fused_and_unfused_qkv_epilogue_agree(monkeypatch):
    """Decode steps run the q/k/v epilogue inside the attention kernels while rows x KV pages is small and as a
    launch of its own above that (MTTS_FUSE_QKV_MAX): same arithmetic, so tokens must be identical, greedy and sampled,
    across page boundaries (140 steps) and with a ragged batch."""
    from mtts.engine import Engine
    cfg = synth.tiny()
    w = synth.synth_weights(cfg, 61, emb_row_sigma=0.6, speech_boost=6.0, eos_boost=1.0)
    ids, mask = synth.synth_prompts(cfg, 62, 4, 40, 0.4, True)
    max_length = ids.shape[1] + 140
    layers = [dict(top_k=40, top_p=0.9, temperature=1.1, repetition_penalty=1.05)] * 8
    outs = []
    for limit in ("1000000", "0"):
        monkeypatch.setenv("MTTS_FUSE_QKV_MAX", limit)
        eng = Engine(cfg, max_batch=4, max_seq_len=256)
        eng.bind_state_dict(w)
        outs.append((eng.generate(ids, mask, max_length),
                     eng.generate(ids, mask, max_length, layers=layers, do_samples=[True] * 8, seed=9)))
        eng.close()
    assert np.array_equal(outs[0][0], outs[1][0])
    assert np.array_equal(outs[0][1], outs[1][1])
    assert outs[0][0].shape[1] - (ids.shape[1] - 7) > 100       # the run did cross page boundaries


def test_graph_replay_equals_stream_launches(monkeypatch):
    """mtts_step replays one captured hipGraph per decode step (re-captured when the KV page bound grows); with
    MTTS_GRAPHS=0 the same launches go straight onto the stream.  Same tokens either way, across a page-bound change."""
    from mtts.engine import Engine
    cfg = synth.tiny()
    w = synth.synth_weights(cfg, 71, emb_row_sigma=0.6, speech_boost=6.0, eos_boost=1.0)
    ids, mask = synth.synth_prompts(cfg, 72, 3, 50, 0.4, True)
    max_length = ids.shape[1] + 600                          # 50 -> 650 tokens: the 8-page bound is crossed
    layers = [dict(top_k=30, top_p=0.9, temperature=1.0)] * 8
    outs = []
    for flag in ("1", "0"):
        monkeypatch.setenv("MTTS_GRAPHS", flag)
        eng = Engine(cfg, max_batch=4, max_seq_len=768)
        eng.bind_state_dict(w)
        outs.append(eng.generate(ids, mask, max_length, layers=layers, do_samples=[True] * 8, seed=3))
        eng.close()
    assert outs[0].shape[1] - (ids.shape[1] - 7) > 520
    assert np.array_equal(outs[0], outs[1])


def test_engine_multi_tile_batch_equals_single_tile(engines):
    """40 dialogues in ONE pass (two 32-row activation tiles share each weight stream) == the same
    dialogues served 32 + 8: per-row results do not depend on the tiling."""
    from mtts.engine import Engine
    cfg = synth.tiny()
    w = synth.synth_weights(cfg, 91, emb_row_sigma=0.6, speech_boost=5.0, eos_boost=5.0)
    big = Engine(cfg, max_batch=64, max_seq_len=256)
    big.bind_state_dict(w)
    ids, mask = synth.synth_prompts(cfg, 92, 40, 26, 0.4, True)
    max_length = ids.shape[1] + 20
    one = big.generate(ids, mask, max_length)
    small = _engine_for(engines, cfg, w, "multi_tile_small")
    parts = [small.generate(ids[s:s + 4], mask[s:s + 4], max_length) for s in range(0, 40, 4)]
    for s, p in zip(range(0, 40, 4), parts):
        n = p.shape[1]
        assert np.array_equal(one[s:s + 4, :n], p), s
        assert (one[s:s + 4, n:, 0] == cfg["eos_token_id"]).all()        # finished-row padding beyond their own end
    layers = [dict(top_k=30, top_p=0.9, temperature=0.9, repetition_penalty=1.1)] * 8
    a = big.generate(ids, mask, max_length, layers=layers, do_samples=[True] * 8, seed=5)
    b = big.generate(ids, mask, max_length, layers=layers, do_samples=[True] * 8, seed=5)
    assert np.array_equal(a, b)
    big.close()


def test_continuous_batching_equals_standalone(engines):
    """11 dialogues of different prompt / output lengths through 4 slots: a finished dialogue leaves at once and
    the next is prefilled into its slot while the others are mid-flight.  Every dialogue's tokens equal what it
    gets alone (batch 1, same seed), greedy and sampled."""
    from mtts.engine import Engine
    from mtts.scheduler import ContinuousBatcher
    cfg = synth.tiny()
    w = synth.synth_weights(cfg, 61, emb_row_sigma=0.6, speech_boost=5.0, eos_boost=5.0)
    eng = Engine(cfg, max_batch=4, max_seq_len=256)
    eng.bind_state_dict(w)
    solo = _engine_for(engines, cfg, w, "cb_solo")
    rng = np.random.default_rng(3)
    prompts, mnts = [], []
    for i in range(11):
        n = int(rng.integers(6, 30))
        raw = np.full((n, 8), 1024, dtype=np.int64)
        raw[:, 0] = rng.integers(0, 151643, n)
        k = int(rng.integers(0, n // 2 + 1))
        if k:
            raw[n - k:, 0] = 151665 + rng.integers(0, 1024, k)
            raw[n - k:, 1:] = rng.integers(0, 1024, (k, 7))
        prompts.append(synth.shifting_inputs(raw, cfg["pad_token_id"]))
        mnts.append(int(rng.integers(3, 40)))
    for layers, ds in ((None, None), ([dict(top_k=20, top_p=0.9, temperature=1.1, repetition_penalty=1.2)] * 8, [True] * 8)):
        cb = ContinuousBatcher(eng, slots=4, gen_cap=64, layers=layers, do_samples=ds, steps_per_poll=5)
        seeds = list(range(100, 111))
        got = cb.run(prompts, mnts, seeds=seeds)
        for i, p in enumerate(prompts):
            alone = solo.generate(p[None], np.ones((1, p.shape[0])), p.shape[0] + mnts[i], layers=layers, do_samples=ds,
                                  seed=seeds[i])[0]
            assert got[i].shape == alone.shape, (i, got[i].shape, alone.shape)
            assert np.array_equal(got[i], alone), i
        # far fewer engine steps than serving the 11 dialogues as static batches of 4 would need
        static = sum(max(mnts[j:j + 4]) + 7 for j in range(0, 11, 4))
        assert cb.engine_steps <= static + 3 * 5 * 3
    eng.close()


def test_sampled_run_replay_against_reference_support(golden_dir):
    """ar_sampled.npz: a SAMPLED run of the reference's real `_sample` with the processed scores (kept set) of every
    step.  Replayed through the engine with the forced row taking the place of each raw draw (so the device state
    machine follows the reference's history): the run must reproduce the reference's ids (state machine), and the
    engine's own draws -- Philox, same rule as the oracle -- must fall inside the reference's kept set (a bf16 tie on a
    top-k / top-p boundary may move one: <= 3 %).  Against the oracle's draws for the same key the bar is lower: the
    tiny model's speech channels are nearly flat, a draw walks ~28 kept tokens in score order, and a one-ulp logit
    difference swaps neighbours in that order (tests with IDENTICAL logits: test_sampler_kernel_vs_oracle)."""
    z = np.load(os.path.join(golden_dir, "ar_sampled.npz"))
    cfg = json.loads(str(z["cfg"]))
    w = synth.synth_weights(cfg, int(z["seed"]), **json.loads(str(z["wkw"])))
    from mtts.engine import Engine
    eng = Engine(cfg, max_batch=2, max_seq_len=256)
    eng.bind_state_dict(w)
    layers = json.loads(str(z["layers"]))
    gold = z["out_ids"]
    T = z["input_ids"].shape[1]
    out, dec = eng.generate(z["input_ids"], z["attention_mask"], int(z["max_length"]), layers=layers,
                            do_samples=[True] * 8, seed=77, forced=gold, forced_as_draw=True)
    eng.close()
    assert np.array_equal(out, gold)
    orc = ao.AsteroidOracle(cfg, w, "bf16")
    _, odec, _ = orc.generate(z["input_ids"], z["attention_mask"], int(z["max_length"]), layers=layers,
                              do_samples=[True] * 8, seed=77, forced=gold, forced_as_draw=True)
    assert dec.shape == odec.shape
    kept = z["kept_idx"]
    n = inside = same = 0
    for s in range(dec.shape[0]):
        for b in range(dec.shape[1]):
            if s > 0 and gold[b, T - 7 + s - 1, 0] == cfg["eos_token_id"]:
                continue                                   # finished row: no draw
            for c in range(8):
                if s < 7 and c >= s + 1:
                    continue                               # teacher-forced slot
                n += 1
                inside += int(dec[s, b, c] in kept[s, b, c])
                same += int(dec[s, b, c] == odec[s, b, c])
    assert n > 200 and inside >= 0.97 * n and same >= 0.8 * n, (n, inside, same)


@pytest.mark.parametrize("dims", ["tiny", "full"])
def test_small_batch_path_equals_general_path(monkeypatch, dims):
    """Decode batches of <= 4 dialogues take the small-batch kernels (gemm.hip: gemv_small_kernel -- the residual +
    RMSNorm, the P.V chunk sum and the SwiGLU hand-over run as GEMM prologues, six launches per layer instead of
    nine); MTTS_SMALL_ROWS=0 sends them through the general kernels.  The prologues repeat the replaced kernels'
    arithmetic in the same order, so the tokens must be IDENTICAL: 1, 3 and 4 ragged dialogues, greedy and sampled,
    150 steps across page boundaries (tiny dims) / 24 steps at the ASSUMED 1.7B dims."""
    from mtts.engine import Engine
    if dims == "tiny":
        cfg = synth.tiny()
        w = synth.synth_weights(cfg, 171, emb_row_sigma=0.6, speech_boost=6.0, eos_boost=1.0)
        steps, plen = 150, 90
    else:
        cfg = synth.assumed_1p7b()
        steps, plen = 24, 100
    layers = [dict(top_k=40, top_p=0.9, temperature=1.1, repetition_penalty=1.05)] * 8
    outs = {}
    for small in ("4", "0"):
        monkeypatch.setenv("MTTS_SMALL_ROWS", small)
        eng = Engine(cfg, max_batch=4, max_seq_len=384)
        if dims == "tiny":
            eng.bind_state_dict(w)
        else:
            for name, t in _rand_weights_on_gpu(cfg, 5):
                eng.bind(name, t)
        res = []
        for B in (1, 3, 4):
            ids, mask = synth.synth_prompts(cfg, 172 + B, B, plen, 0.4, True)
            ml = ids.shape[1] + steps
            res.append(eng.generate(ids, mask, ml))
            res.append(eng.generate(ids, mask, ml, layers=layers, do_samples=[True] * 8, seed=11))
        outs[small] = res
        eng.close()
    for a, b in zip(outs["4"], outs["0"]):
        assert a.shape == b.shape and np.array_equal(a, b)
    assert outs["4"][0].shape[1] >= steps


def test_fp32_engine_strict_parity_with_reference_fixture(golden_dir):
    """`--dtype fp32` (reference inference.py:27-40): fp32 weights / arithmetic / KV / logits on the HIP path.  With no
    bf16 rounding points the only difference from the reference's CPU run is fp32 summation order, so this is the
    STRICT gate: against tests/golden/ar_text_ragged_fp32.npz (the reference's own fp32 run, real `_sample`):
    every decision of the teacher-forced replay is identical -- no margin gate --, the free run reproduces the
    reference's ids token for token, and the logits agree with the fp32 oracle to 1e-4 of the row maximum."""
    from mtts.engine import Engine
    z = np.load(os.path.join(golden_dir, "ar_text_ragged_fp32.npz"))
    cfg = json.loads(str(z["cfg"]))
    w = synth.synth_weights(cfg, int(z["seed"]), bf16=False, **json.loads(str(z["wkw"])))
    gold = z["out_ids"]
    T = z["input_ids"].shape[1]
    eng = Engine(cfg, max_batch=4, max_seq_len=256, dtype="fp32")
    eng.bind_state_dict(w)
    out, dec = eng.generate(z["input_ids"], z["attention_mask"], int(z["max_length"]), forced=gold)
    assert np.array_equal(out, gold)
    want = gold[:, T - 7:].transpose(1, 0, 2)
    assert dec.shape == want.shape and np.array_equal(dec, want)          # 100 % of the decisions, low-margin ones included
    free = eng.generate(z["input_ids"], z["attention_mask"], int(z["max_length"]))
    assert free.shape == gold.shape and np.array_equal(free, gold)
    # logits vs the fp32 oracle, prompt pass + 4 decode steps
    orc = ao.AsteroidOracle(cfg, w, "fp32")
    _, _, logs = orc.generate(z["input_ids"], z["attention_mask"], int(z["max_length"]), forced=gold, return_logits=True, max_steps=5)
    eng.begin(z["input_ids"], z["attention_mask"], int(z["max_length"]))
    worst = 0.0
    for s in range(5):
        l0, l17 = eng.read_logits()
        for c in range(8):
            got = l0 if c == 0 else l17[c - 1]
            ref = logs[s][c]
            fin = np.isfinite(ref)
            scale_ = np.abs(np.where(fin, ref, 0)).max(axis=-1, keepdims=True)
            worst = max(worst, float((np.abs(np.where(fin, got - np.where(fin, ref, 0), 0)) / scale_).max()))
        eng.step(1)
        eng.sync_state()
        if not np.array_equal(eng.read_generated(s + 1)[-1], gold[:, T - 7 + s]):
            break
    assert worst <= 1e-4, worst
    eng.close()


def test_fp32_engine_long_run_equals_fp32_oracle():
    """fp32 engine vs fp32 oracle, free-running greedy, ragged prompts of 150..300 tokens (prefill in 256-row passes,
    exact-f32 MFMA GEMM) and 120 decode steps across page boundaries (GEMV path), GQA group 2: identical ids; the
    same with a B=11 batch (decode rows through the MFMA GEMM)."""
    from mtts.engine import Engine
    cfg = synth.tiny()
    w = synth.synth_weights(cfg, 181, bf16=False, emb_row_sigma=0.6, speech_boost=6.0, eos_boost=1.0)
    orc = ao.AsteroidOracle(cfg, w, "fp32")
    for B, plen, steps in ((3, 300, 120), (11, 60, 40)):
        ids, mask = synth.synth_prompts(cfg, 182 + B, B, plen, 0.4, True)
        max_length = ids.shape[1] + steps
        gold = orc.generate(ids, mask, max_length)
        margins = np.stack(orc.last_margins)
        eng = Engine(cfg, max_batch=16, max_seq_len=512, dtype="fp32")
        eng.bind_state_dict(w)
        out = eng.generate(ids, mask, max_length)
        eng.close()
        # fp32 ties are not impossible (argmax over 152 697 random logits): compare up to the first decision whose
        # relative margin is below 1e-5, if there is one
        tight = np.nonzero((margins < 1e-5).any(axis=(1, 2)))[0]
        upto = (ids.shape[1] - 7) + (int(tight[0]) if len(tight) else gold.shape[1])
        n = min(upto, gold.shape[1], out.shape[1])
        assert n >= ids.shape[1] - 7 + steps // 2
        assert np.array_equal(out[:, :n], gold[:, :n]), B


def test_rope_kvwrite_kernel_bit_exact_vs_oracle():
    """mtts_k_rope_kvwrite = the q/k/v epilogue of a decode / prefill row on its own (qkv_post_kernel): per-head q/k
    RMSNorm, RoPE in bf16 with its three roundings (modeling_qwen3.py:148-170,251-252), K and V written into their
    cache pages (and read back from them).  Against the oracle's rmsnorm / apply_rope: every bit."""
    from mtts.engine import rope_tables
    lib = capi.lib()
    rng = np.random.default_rng(5)
    cfg = synth.tiny()
    orc = ao.AsteroidOracle(cfg, {}, "bf16")
    for R, nq, nkv in ((7, 4, 2), (32, 16, 8), (3, 2, 2)):
        N = (nq + 2 * nkv) * 128
        qkv = ao.round_bf16(rng.standard_normal((R, N)).astype(np.float32) * 2)
        pos = rng.integers(0, 700, R).astype(np.int32)
        qn = ao.round_bf16(1 + 0.2 * rng.standard_normal(128).astype(np.float32))
        kn = ao.round_bf16(1 + 0.2 * rng.standard_normal(128).astype(np.float32))
        cos, sin = rope_tables(128, float(cfg["rope_theta"]), 704, "cuda")
        q = torch.zeros(R, nq, 128, dtype=torch.bfloat16, device="cuda")
        k = torch.zeros(R, nkv, 128, dtype=torch.bfloat16, device="cuda")
        v = torch.zeros(R, nkv, 128, dtype=torch.bfloat16, device="cuda")
        qt, qnt, knt = _bf16_t(qkv), _bf16_t(qn), _bf16_t(kn)
        capi.check(lib.mtts_k_rope_kvwrite(qt.data_ptr(), pos.ctypes.data, qnt.data_ptr(), knt.data_ptr(), cos.data_ptr(),
                                           sin.data_ptr(), R, nq, nkv, C.c_float(1e-6), q.data_ptr(), k.data_ptr(), v.data_ptr(), None))
        torch.cuda.synchronize()
        oc, os_ = orc.rope(pos[:, None].astype(np.int64))                  # [R,1,128]
        qh = qkv[:, :nq * 128].reshape(R, 1, nq, 128)
        kh = qkv[:, nq * 128:(nq + nkv) * 128].reshape(R, 1, nkv, 128)
        want_q = orc.apply_rope(orc.rmsnorm(qh, qn).transpose(0, 2, 1, 3), oc, os_)[:, :, 0]
        want_k = orc.apply_rope(orc.rmsnorm(kh, kn).transpose(0, 2, 1, 3), oc, os_)[:, :, 0]
        want_v = qkv[:, (nq + nkv) * 128:].reshape(R, nkv, 128)
        assert np.array_equal(q.float().cpu().numpy(), want_q)
        assert np.array_equal(k.float().cpu().numpy(), want_k)
        assert np.array_equal(v.float().cpu().numpy(), want_v)


@pytest.mark.parametrize("nq,nkv", [(4, 2), (4, 4), (8, 2)])
def test_paged_attn_decode_kernel_vs_oracle(nq, nkv):
    """mtts_k_paged_attn_decode = the three attention launches of a decode step on their own (scores, P.V, combine)
    over a paged cache with a SHUFFLED page table, ragged lengths 1..1500 (24 pages, 3 pass-B chunks).  Against the
    eager formula with the reference's rounding points (s = bf16(bf16(q.k) * scale), p = bf16(softmax_fp32(s)),
    o = bf16(p.V), modeling_qwen3.py:185-208): fp32 summation order is the only freedom, so nearly every bf16 output is
    bit-identical and the rest is one ulp away."""
    lib = capi.lib()
    rng = np.random.default_rng(11 + nq + nkv)
    R, Lmax = 6, 1500
    lens = np.array([1500, 1, 64, 65, 777, 1023], dtype=np.int32)
    q = ao.round_bf16(rng.standard_normal((R, nq, 128)).astype(np.float32))
    K = ao.round_bf16(rng.standard_normal((R, Lmax, nkv, 128)).astype(np.float32))
    V = ao.round_bf16(rng.standard_normal((R, Lmax, nkv, 128)).astype(np.float32))
    pages = (Lmax + 63) // 64
    table = rng.permutation(R * pages).astype(np.int32).reshape(R, pages)
    out = torch.zeros(R, nq * 128, dtype=torch.bfloat16, device="cuda")
    qt, kt, vt = _bf16_t(q), _bf16_t(K), _bf16_t(V)
    capi.check(lib.mtts_k_paged_attn_decode(qt.data_ptr(), kt.data_ptr(), vt.data_ptr(), lens.ctypes.data, table.ctypes.data,
                                            R, Lmax, nq, nkv, out.data_ptr(), None))
    torch.cuda.synchronize()
    got = out.float().cpu().numpy().reshape(R, nq, 128)
    g = nq // nkv
    scale = np.float32(128 ** -0.5)
    exact = total = 0
    for r in range(R):
        n = int(lens[r])
        Kr = np.repeat(K[r, :n].transpose(1, 0, 2), g, axis=0)            # [nq, n, 128]
        Vr = np.repeat(V[r, :n].transpose(1, 0, 2), g, axis=0)
        s = ao.round_bf16(np.einsum("hd,hnd->hn", q[r], Kr).astype(np.float32))
        s = ao.round_bf16(s * scale)
        p = ao.round_bf16(ao.softmax_f32(s))
        o = ao.round_bf16(np.einsum("hn,hnd->hd", p, Vr).astype(np.float32))
        tol = 2.0 ** -7 * np.abs(o).max()
        assert np.abs(got[r] - o).max() <= tol, (r, float(np.abs(got[r] - o).max()), float(tol))
        exact += int((got[r] == o).sum())
        total += o.size
    assert exact >= 0.9 * total, (exact, total)
    # the same through consecutive pages: identical bits (the table only redirects)
    out2 = torch.zeros_like(out)
    capi.check(lib.mtts_k_paged_attn_decode(qt.data_ptr(), kt.data_ptr(), vt.data_ptr(), lens.ctypes.data, None,
                                            R, Lmax, nq, nkv, out2.data_ptr(), None))
    torch.cuda.synchronize()
    assert torch.equal(out, out2)


def test_fp32_continuous_batching_equals_standalone():
    """The fp32 engine under the continuous batcher: 6 dialogues through 2 slots, every dialogue's tokens equal its
    batch-1 run (greedy and sampled with per-dialogue Philox keys)."""
    from mtts.engine import Engine
    from mtts.scheduler import ContinuousBatcher
    cfg = synth.tiny()
    w = synth.synth_weights(cfg, 191, bf16=False, emb_row_sigma=0.6, speech_boost=5.0, eos_boost=5.0)
    eng = Engine(cfg, max_batch=2, max_seq_len=256, dtype="fp32")
    eng.bind_state_dict(w)
    solo = Engine(cfg, max_batch=1, max_seq_len=256, dtype="fp32")
    solo.bind_state_dict(w)
    rng = np.random.default_rng(7)
    prompts, mnts = [], []
    for i in range(6):
        n = int(rng.integers(6, 40))
        raw = np.full((n, 8), 1024, dtype=np.int64)
        raw[:, 0] = rng.integers(0, 151643, n)
        prompts.append(synth.shifting_inputs(raw, cfg["pad_token_id"]))
        mnts.append(int(rng.integers(5, 30)))
    for layers, ds in ((None, None), ([dict(top_k=20, top_p=0.9, temperature=1.1)] * 8, [True] * 8)):
        cb = ContinuousBatcher(eng, slots=2, gen_cap=64, layers=layers, do_samples=ds, steps_per_poll=4)
        got = cb.run(prompts, mnts, base_seed=40)
        for i, p in enumerate(prompts):
            alone = solo.generate(p[None], np.ones((1, p.shape[0])), p.shape[0] + mnts[i], layers=layers, do_samples=ds, seed=40 + i)[0]
            assert got[i].shape == alone.shape and np.array_equal(got[i], alone), i
    eng.close()
    solo.close()



def test_fp16_engine_parity_with_reference_fixture(golden_dir):
    """`--dtype fp16` (reference inference.py:27-40; modeling through `from_pretrained(torch_dtype=torch.float16)`): the
    fp32 kernels with an fp16 rounding point wherever the reference's fp16 CPU run materialises a tensor.  Against
    tests/golden/ar_text_ragged_fp16.npz (the reference's own fp16 run, real `_sample`): the teacher-forced replay gives
    the reference's decision wherever its top-2 margin is at least 4 fp16 ulps (2^-9 relative), the state-machine outputs
    always, >= 99 % of ALL free decisions; the free run reproduces the ids up to the first such near-tie; the logits
    agree with the fp16 oracle within 4 fp16 ulps of the row maximum and mostly bit for bit."""
    from mtts.engine import Engine
    z = np.load(os.path.join(golden_dir, "ar_text_ragged_fp16.npz"))
    cfg = json.loads(str(z["cfg"]))
    w = synth.synth_weights(cfg, int(z["seed"]), bf16=False, **json.loads(str(z["wkw"])))
    gold = z["out_ids"]
    T = z["input_ids"].shape[1]
    eng = Engine(cfg, max_batch=4, max_seq_len=256, dtype="fp16")
    eng.bind_state_dict(w)
    out, dec = eng.generate(z["input_ids"], z["attention_mask"], int(z["max_length"]), forced=gold)
    assert np.array_equal(out, gold)
    want = gold[:, T - 7:].transpose(1, 0, 2)
    m = z["margins"]
    gate = 2.0 ** -9
    used = m < 9.0
    safe = used & (m >= gate)
    assert dec.shape == want.shape and np.array_equal(dec[safe], want[safe])
    assert np.array_equal(dec[~used], want[~used])
    assert (dec[used] == want[used]).mean() >= 0.99, float((dec[used] == want[used]).mean())
    free = eng.generate(z["input_ids"], z["attention_mask"], int(z["max_length"]))
    low = np.nonzero((m < gate).any(axis=(1, 2)))[0]
    upto = (T - 7) + (int(low[0]) if len(low) else gold.shape[1])
    n = min(upto, free.shape[1], gold.shape[1])
    assert n > T - 7 + 5 and np.array_equal(free[:, :n], gold[:, :n])
    orc = ao.AsteroidOracle(cfg, w, "fp16")
    _, _, logs = orc.generate(z["input_ids"], z["attention_mask"], int(z["max_length"]), forced=gold, return_logits=True, max_steps=5)
    eng.begin(z["input_ids"], z["attention_mask"], int(z["max_length"]))
    exact = total = 0
    for s in range(5):
        l0, l17 = eng.read_logits()
        for c in range(8):
            got = l0 if c == 0 else l17[c - 1]
            ref = logs[s][c]
            fin = np.isfinite(ref)
            scale_ = np.abs(np.where(fin, ref, 0)).max(axis=-1, keepdims=True)
            assert (np.abs(np.where(fin, got - np.where(fin, ref, 0), 0)) <= 2.0 ** -9 * scale_).all(), (s, c)
            exact += int((got[fin] == ref[fin]).sum())
            total += int(fin.sum())
        eng.step(1)
        eng.sync_state()
        if not np.array_equal(eng.read_generated(s + 1)[-1], gold[:, T - 7 + s]):
            break
    eng.close()
    assert exact >= 0.3 * total, (exact, total)


@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
def test_fp32_family_engines_are_batch_invariant(dtype):
    """The fp32 / fp16 engines take the GEMV kernel for decode rows (8 rows per launch, whatever the batch) and the MFMA
    GEMM for prefill passes (whatever their row count), so a dialogue's fp32 summation order -- and with it every
    low-margin pick -- does not depend on how many dialogues share its batch: 12 ragged dialogues in one static batch
    equal their batch-1 runs, greedy and sampled (per-row Philox streams)."""
    from mtts.engine import Engine
    cfg = synth.tiny()
    w = synth.synth_weights(cfg, 271, bf16=False, emb_row_sigma=0.6, speech_boost=6.0, eos_boost=1.0)
    ids, mask = synth.synth_prompts(cfg, 272, 12, 40, 0.4, True)
    T = ids.shape[1]
    max_length = T + 30
    layers = [dict(top_k=20, top_p=0.9, temperature=1.1)] * 8
    eng = Engine(cfg, max_batch=16, max_seq_len=256, dtype=dtype)
    eng.bind_state_dict(w)
    full = eng.generate(ids, mask, max_length)
    samp = eng.generate(ids, mask, max_length, layers=layers, do_samples=[True] * 8, seed=13)
    for b in (0, 5, 11):
        pad = int(np.argmax(mask[b] > 0))
        p = ids[b, pad:][None]
        one = eng.generate(p, np.ones((1, p.shape[1])), p.shape[1] + 30)
        assert np.array_equal(one[0, p.shape[1] - 7:], full[b, T - 7:T - 7 + one.shape[1] - (p.shape[1] - 7)]), b
        one_s = eng.generate(p, np.ones((1, p.shape[1])), p.shape[1] + 30, layers=layers, do_samples=[True] * 8, seed=13, row_ids=[b])
        assert np.array_equal(one_s[0, p.shape[1] - 7:], samp[b, T - 7:T - 7 + one_s.shape[1] - (p.shape[1] - 7)]), b
    eng.close()
