"""output_scores: per-token log-probabilities from the device sampler.  -m gpu.

lp[g, r, c] = log_softmax(S)[d]: S the channel's processed score row (hard-coded masks, repetition penalty, temperature,
top-k, top-p; filtered tokens at -inf), d the sampler's own decision; NaN where the appended token is not a model
decision (include/mtts.h: mtts_set_output_scores).

Two kinds of check.  The kernel and the engine against float64 numpy ON THE SAME LOGITS hold the arithmetic: tolerance
2e-5, derived below.  The replays of reference fixtures hold the whole path to the reference: their tolerance is bf16
logit noise, measured for the numpy oracle when the fixtures were made (profiles/scores_parity.json).  The rest are exact
properties: switching scores on changes no token, and lp is a function of (prompt, seed, row id) alone.

The 2e-5 budget (absolute, on lp = (s_d - smax) - log(sum exp(s - smax))): |s - smax| < 64 in fp32 rounds once, <= 3.8e-6;
expf at 2 ulp per term and the fp32 sum of at most 19 terms per thread (the greedy slice pass; everything after it, and
every sampled-path sum, is fp64 or exact integers) give <= 3e-6 relative on a sum >= 1; the log of a value <= 12 adds
<= 1e-6.  2 x the total, rounded up.
"""
import ctypes as C
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from mtts import capi, synth  # noqa: E402
from oracle import asteroid_oracle as ao  # noqa: E402

import scores_parity_cpu as spc  # noqa: E402
import scores_ref as sr  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = sr.KERNEL_TOL
GREEDY = ([dict(repetition_penalty=1.3, temperature=0.8)] * 8, [False] * 8)
SAMPLED = sr.SCENARIO_SAMPLED
MIXED = ([dict(repetition_penalty=1.2)] + [dict(top_k=30, top_p=0.85, temperature=1.0, repetition_penalty=1.1)] * 7,
         [False] + [True] * 7)


def _eq(a, b):
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def _bf16_t(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(torch.bfloat16).cuda()


def _weights(cfg, seed=sr.SCENARIO["weight_seed"], bf16=True):
    return synth.synth_weights(cfg, seed, bf16=bf16, **sr.SCENARIO["wkw"])


def _engine(cfg, w, **kw):
    from mtts.engine import Engine
    kw.setdefault("max_batch", 8)
    kw.setdefault("max_seq_len", 256)
    eng = Engine(cfg, **kw)
    eng.bind_state_dict(w)
    return eng


# ---- 1. kernel against fp64 numpy on the same logits ------------------------------------------------------------------
def _k_sample_scores(logits, hist, lc, do_sample, mask_id, seed, step, channel):
    from mtts.engine import sampler_cfgs
    lib = capi.lib()
    rows, V = logits.shape
    lt = _bf16_t(logits)
    bm = np.zeros((rows, (V + 31) // 32), dtype=np.uint32)
    for b in range(rows):
        for t in hist[b]:
            bm[b, t >> 5] |= np.uint32(1 << (t & 31))
    bmt = torch.from_numpy(bm.view(np.int32)).cuda()
    cfg = sampler_cfgs([lc] * 8, [do_sample] * 8)[0]
    tok = torch.zeros(rows, dtype=torch.int32, device="cuda")
    lp = torch.zeros(rows, dtype=torch.float32, device="cuda")
    capi.check(lib.mtts_k_sample_scores(lt.data_ptr(), rows, V, bmt.data_ptr(), C.byref(cfg), mask_id, C.c_uint64(seed),
                                        step, channel, tok.data_ptr(), lp.data_ptr(), None))
    plain = torch.zeros(rows, dtype=torch.int32, device="cuda")
    capi.check(lib.mtts_k_sample(lt.data_ptr(), rows, V, bmt.data_ptr(), C.byref(cfg), mask_id, C.c_uint64(seed),
                                 step, channel, plain.data_ptr(), None))
    torch.cuda.synchronize()
    assert torch.equal(tok, plain)                                 # emitting lp changes no token
    return tok.cpu().numpy().astype(np.int64), lp.cpu().numpy()


KERNEL_MODES = {
    # name -> (layer config, do_sample)
    "greedy": (dict(repetition_penalty=1.3, temperature=0.8), False),
    "top_k": (dict(repetition_penalty=1.1, temperature=0.9, top_k=50), True),
    "top_p": (dict(repetition_penalty=1.1, temperature=0.9, top_p=0.9), True),
    "top_k_top_p": (dict(repetition_penalty=1.1, temperature=0.9, top_k=50, top_p=0.9), True),
    "no_top_k": (dict(repetition_penalty=1.2, temperature=1.3), True),
    "top_k_6000": (dict(repetition_penalty=1.2, temperature=0.9, top_k=6000, top_p=0.97), True),
}


@pytest.mark.parametrize("mode", list(KERNEL_MODES))
@pytest.mark.parametrize("V", [1025, 152697])
def test_kernel_lp_vs_fp64(V, mode):
    """mtts_k_sample_scores on random bf16 logits with a history bitmap, repetition penalty and temperature: lp against
    the float64 log-softmax of oracle.apply_processors' scores at the token the kernel returned.
    A kept set that differs by a boundary token legitimately moves lp by (its mass) / (kept mass).  Where the cuts act on
    few, heavy tokens (every mode on 1025 tokens, top_k <= 50 on the big vocabulary: the in-block path) the inputs are
    built so that this cannot happen (scores_ref.boundary_safe: rows are regenerated) and the tolerance is 2e-5.  A
    nucleus over the whole big vocabulary (no top_k, top_k = 6000: the full-vocabulary kernel) has ~1e-6 of mass per
    boundary token and which of them sit on the boundary is fp32 noise in HF's own cumsum:
    test_engine_gpu.py::test_sampler_kernel_vs_oracle grants 1e-4 of mass for exactly this, which is 1e-4 / top_p on lp
    (d log(tot) = delta / tot, tot >= top_p)."""
    lc, do_sample = KERNEL_MODES[mode]
    rng = np.random.default_rng(1000 + V % 97 + len(mode))
    rows = 6
    mask_id = 1024 if V == 1025 else 152694
    full_path = do_sample and V > 4096 and not (lc.get("top_k") and lc["top_k"] <= 4096)
    pre = {k: v for k, v in lc.items() if k in ("repetition_penalty", "temperature")}
    logits = np.zeros((rows, V), dtype=np.float32)
    hist = np.zeros((rows, 50), dtype=np.int64)
    for b in range(rows):
        for _ in range(200):
            logits[b] = ao.round_bf16(rng.standard_normal(V).astype(np.float32) * 2.5)
            hist[b] = rng.integers(0, V, 50)
            lm = logits[b].copy()
            lm[mask_id] = -np.inf
            if not do_sample or full_path or sr.boundary_safe(ao.apply_processors(hist[b][None], lm[None], pre)[0], lc):
                break
        else:
            raise AssertionError("no boundary-safe row found")
    lm = logits.copy()
    lm[:, mask_id] = -np.inf
    want_scores = ao.apply_processors(hist, lm, lc if do_sample else pre)      # (a greedy channel applies no top-k / top-p)
    tol = TOL + (1e-4 / lc["top_p"] if full_path and lc.get("top_p") else 0.0)
    worst = 0.0
    first = None
    for step in range(6 if do_sample else 1):
        tok, lp = _k_sample_scores(logits, hist, lc, do_sample, mask_id, 4321, step, 0 if V > 4096 else 3)
        tok2, lp2 = _k_sample_scores(logits, hist, lc, do_sample, mask_id, 4321, step, 0 if V > 4096 else 3)
        assert np.array_equal(tok, tok2) and np.array_equal(lp.view(np.uint32), lp2.view(np.uint32))     # bit-identical
        first = tok if first is None else first
        for b in range(rows):
            assert np.isfinite(want_scores[b, tok[b]]), (mode, V, b, step)       # the pick is inside the kept set
            want = sr.log_softmax64(want_scores[b], tok[b])
            worst = max(worst, abs(float(lp[b]) - want))
            assert abs(float(lp[b]) - want) <= tol, (mode, V, step, b, float(lp[b]), want, tol)
        if not do_sample:
            assert np.array_equal(tok, np.argmax(want_scores, -1))
    print(f"kernel lp {mode} V={V}: max |lp - fp64| = {worst:.3e} (tolerance {tol:.3e})")


# ---- 2. engine against its own logits ----------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["greedy", "sampled"])
@pytest.mark.parametrize("dtype", ["bf16", "fp32", "fp16"])
def test_engine_lp_vs_its_own_logits(dtype, mode):
    """All three engine dtypes (they share the sampler through LogitsPtr).  begin, then per step read_logits() -> step(1)
    (mtts_step samples from the last forward's logits, then runs the forward): lp recomputed on the host from those logits and the known history (prompt + generated tokens per channel, as
    HF's repetition penalty sees them) at the token the engine appended.  Ragged B=3, 51 steps, one row runs an EOS flush
    and finishes early.  Tolerance 2e-5; in the sampled run (top-k 20 / 30 with top-p) a boundary token that moves may
    put at most 1 slot in 240 outside it, the allowance test_sampler_kernel_vs_oracle uses for its 240 draws (that the host
    side alone moves none on these inputs is checked in test_scores_cpu.py on the oracle's logits of the same runs).  The NaN
    pattern must be exactly the complement of the host state machine's used mask."""
    sc = sr.SCENARIO
    cfg = synth.tiny()
    w = _weights(cfg, bf16=(dtype == "bf16"))
    ids, mask = synth.synth_prompts(cfg, sc["prompt_seed"], sc["batch"], sc["prompt_len"], sc["audio_frac"], True)
    new = sc["new"]
    ml = ids.shape[1] + new
    base = ids.shape[1] - 7
    layers, ds = GREEDY if mode == "greedy" else SAMPLED
    eng = _engine(cfg, w, max_batch=4, dtype=dtype)
    eng.begin(ids, mask, ml, layers=layers, do_samples=ds, seed=sc["seed"], output_scores=True)
    logs = []
    for _ in range(new + 8):
        logs.append(eng.read_logits())
        eng.step(1)
        _, done = eng.sync_state()
        if done:
            break
    gen = eng.read_generated(new + 16)
    lp = eng.read_scores(new + 16)
    eng.close()
    G = gen.shape[0]
    assert lp.shape == gen.shape and lp.dtype == np.float32
    assert G >= 40
    used = sr.used_mask(gen, base, ml, cfg)
    assert np.array_equal(np.isnan(lp), ~used)
    per_row = used.sum((0, 2))
    assert per_row.min() < per_row.max() and (gen[:, :, 0] == cfg["eos_token_id"]).any()      # a row flushed and left early
    worst, over, n = 0.0, 0, 0
    for g in range(G):
        l0, l17 = logs[g]
        for r in range(3):
            for c in range(8):
                if not used[g, r, c]:
                    continue
                row = l0[r] if c == 0 else l17[c - 1, r]
                history = np.concatenate([ids[r, :base, c], gen[:g, r, c]])
                want, s = sr.expected_lp(row, history, layers[c], g, c, int(gen[g, r, c]))
                assert np.isfinite(s[gen[g, r, c]]), (g, r, c)
                dev = abs(float(lp[g, r, c]) - want)
                n += 1
                if dev > TOL:
                    over += 1
                else:
                    worst = max(worst, dev)
    print(f"engine lp {dtype} {mode}: {n} slots, max deviation within tolerance {worst:.3e}, {over} over")
    assert n > 400
    assert over <= (n // 240 if mode == "sampled" else 0), (over, n)


# ---- 3. pinned by the reference ------------------------------------------------------------------------------------------
def _parity():
    with open(os.path.join(ROOT, "profiles", "scores_parity.json")) as f:
        return json.load(f)["cases"]


@pytest.mark.parametrize("name", ["ar_scores_bf16", "ar_scores_fp32"])
def test_replay_lp_matches_reference_scores(golden_dir, name):
    """Teacher-forced replay of the reference's real `_sample` run with output_scores: at every used slot where the
    engine's decision equals the reference's, lp within 2 x D_oracle + 2e-5 of the float64 log-softmax of the reference's
    own `scores`.  D_oracle: what the numpy oracle deviates by on this fixture (bf16: one-ulp logit differences); engine
    and oracle each sum dot products in an order of their own, so a logit may sit one ulp off the reference's in each and
    the two deviations can add; 2e-5 is the kernel budget.  Slots left out because decisions differ: at most 1 %."""
    z, cfg, w, dtype = spc.load(golden_dir, name)
    rec = _parity()[name]
    layers = json.loads(str(z["layers"]))
    eng = _engine(cfg, w, max_batch=4, dtype=dtype)
    out, dec, lp = eng.generate(z["input_ids"], z["attention_mask"], int(z["max_length"]), layers=layers,
                                forced=z["out_ids"], output_scores=True)
    eng.close()
    assert np.array_equal(out, z["out_ids"])
    used, ref_dec, ref_lp = z["used"], z["ref_dec"], z["ref_lp"]
    lp = lp.transpose(1, 0, 2)                                     # [steps, B, 8] like the fixture
    assert np.array_equal(np.isnan(lp), ~used)
    same = used & (dec == ref_dec)
    tol = 2 * rec["D_oracle"] + TOL
    dev = np.abs(lp[same].astype(np.float64) - ref_lp[same])
    print(f"{name}: used {int(used.sum())}, compared {int(same.sum())}, max deviation {dev.max():.3e} (tolerance {tol:.3e})")
    assert used.sum() - same.sum() <= 0.01 * used.sum()
    assert dev.max() <= tol


def test_sampled_replay_lp_matches_reference_kept_sets(golden_dir):
    """ar_sampled.npz replayed with forced_as_draw: lp is taken at the engine's own draw d; where d lies in the
    reference's kept set (stored whole) the reference value is kept_val[d] - logsumexp(kept_val).  At least 97 % of the used
    slots must be compared and within 2 x D_sampled + 2e-5 (the allowance test_sampled_run_replay_against_reference_support
    grants for draws outside the reference's kept set)."""
    z, cfg, w, _ = spc.load(golden_dir, "ar_sampled")
    rec = _parity()["ar_sampled"]
    layers = json.loads(str(z["layers"]))
    eng = _engine(cfg, w, max_batch=2)
    out, dec, lp = eng.generate(z["input_ids"], z["attention_mask"], int(z["max_length"]), layers=layers,
                                do_samples=[True] * 8, seed=rec["seed"], forced=z["out_ids"], forced_as_draw=True,
                                output_scores=True)
    eng.close()
    assert np.array_equal(out, z["out_ids"])
    lp = lp.transpose(1, 0, 2)
    used = spc.sampled_used(z, cfg)
    assert np.array_equal(np.isnan(lp), ~used)
    tol = 2 * rec["D_sampled"] + TOL
    ok, worst = 0, 0.0
    for s, b, c in zip(*np.nonzero(used)):
        ref = spc.sampled_reference_lp(z, s, b, c, int(dec[s, b, c]))
        if ref is not None:
            worst = max(worst, abs(float(lp[s, b, c]) - ref))
            ok += int(abs(float(lp[s, b, c]) - ref) <= tol)
    print(f"ar_sampled: used {int(used.sum())}, within tolerance {ok}, max deviation {worst:.3e} (tolerance {tol:.3e})")
    assert used.sum() > 200 and ok >= 0.97 * used.sum()


# ---- 4. properties (exact) -------------------------------------------------------------------------------------------------
def test_scores_change_no_token_and_do_not_depend_on_the_batch():
    """Static batch, greedy / sampled / greedy channel 0 + sampled speech channels: tokens with scores on == tokens with
    scores off; lp is run-to-run bit-identical; a dialogue alone (same seed and row id) has the lp it has inside a batch
    of 8; the take rows equal the repeat-interleaved batch."""
    cfg = synth.tiny()
    eng = _engine(cfg, _weights(cfg), max_batch=24)
    ids, mask = synth.synth_prompts(cfg, 104, 8, 24, 0.3, False)       # (no left padding: a row alone sees the same history)
    ml = ids.shape[1] + 44
    base = ids.shape[1] - 7
    for layers, ds in (GREEDY, SAMPLED, MIXED):
        off = eng.generate(ids, mask, ml, layers=layers, do_samples=ds, seed=5)
        on, lp = eng.generate(ids, mask, ml, layers=layers, do_samples=ds, seed=5, output_scores=True)
        assert _eq(on, off)
        assert lp.shape == (8, on.shape[1] - base, 8) and lp.dtype == np.float32
        assert np.isfinite(lp).any() and (lp[np.isfinite(lp)] <= 0).all()
        on2, lp2 = eng.generate(ids, mask, ml, layers=layers, do_samples=ds, seed=5, output_scores=True)
        assert _eq(on2, on) and np.array_equal(lp.view(np.uint32), lp2.view(np.uint32))
        for r in (0, 5):
            a_ids, a_lp = eng.generate(ids[r:r + 1], mask[r:r + 1], ml, layers=layers, do_samples=ds, seed=5, row_ids=[r],
                                       output_scores=True)
            g = a_ids.shape[1] - base
            assert _eq(a_ids[0], on[r, :base + g])
            assert _eq(a_lp[0], lp[r, :g])
    eng.generate(ids, mask, ml)
    with pytest.raises(capi.MttsError) as ei:                        # the last run had scores off
        eng.read_scores(64)
    assert ei.value.code == capi.ESTATE
    n = 3
    layers, ds = SAMPLED
    got, got_lp = eng.generate(ids[:4], mask[:4], ml, layers=layers, do_samples=ds, seed=9, takes=n, output_scores=True)
    want, want_lp = eng.generate(np.repeat(ids[:4], n, 0), np.repeat(mask[:4], n, 0), ml, layers=layers, do_samples=ds,
                                 seed=9, output_scores=True)
    assert _eq(got, want) and _eq(got_lp, want_lp)
    assert _eq(got, eng.generate(ids[:4], mask[:4], ml, layers=layers, do_samples=ds, seed=9, takes=n))
    eng.close()


def test_switch_is_refused_while_a_run_is_open():
    cfg = synth.tiny()
    eng = _engine(cfg, _weights(cfg), max_batch=4)
    ids, mask = synth.synth_prompts(cfg, 104, 3, 24, 0.3, True)
    eng.begin(ids, mask, ids.shape[1] + 44)
    eng.step(3)
    with pytest.raises(capi.MttsError) as ei:
        eng.set_output_scores(True)
    assert ei.value.code == capi.ESTATE
    eng.set_output_scores(False)                                       # no change: fine
    with pytest.raises(capi.MttsError) as ei:
        eng.read_scores(16)                                            # the open run was started with scores off
    assert ei.value.code == capi.ESTATE
    eng.close()


@pytest.mark.parametrize("knob", ["MTTS_GRAPHS", "MTTS_SMALL_ROWS"])
def test_lp_equal_across_launch_paths(monkeypatch, knob):
    """Graph replay vs MTTS_GRAPHS=0 (stream launches), and the small-batch path (<= 4 rows) vs MTTS_SMALL_ROWS=0 (the
    general kernels): same tokens, same lp bits, greedy and sampled, 3 ragged rows."""
    cfg = synth.tiny()
    w = _weights(cfg)
    ids, mask = synth.synth_prompts(cfg, 104, 3, 24, 0.3, True)
    ml = ids.shape[1] + 90
    res = []
    for val in ("1" if knob == "MTTS_GRAPHS" else "4", "0"):
        monkeypatch.setenv(knob, val)
        eng = _engine(cfg, w, max_batch=4)
        res.append([eng.generate(ids, mask, ml, layers=layers, do_samples=ds, seed=5, output_scores=True)
                    for layers, ds in (GREEDY, SAMPLED)])
        eng.close()
    for (a_ids, a_lp), (b_ids, b_lp) in zip(*res):
        assert _eq(a_ids, b_ids) and _eq(a_lp, b_lp)
        assert np.isfinite(a_lp).sum() > 400


def _plain_prompt(rng, n):
    raw = np.full((n, 8), 1024, dtype=np.int64)
    raw[:, 0] = rng.integers(0, 151643, n)
    raw[n - 6:, 0] = 151665 + rng.integers(0, 1024, 6)
    raw[n - 6:, 1:] = rng.integers(0, 1024, (6, 7))
    return synth.shifting_inputs(raw, 151643)


def test_scheduler_lp_survives_eviction_and_forks():
    """Continuous batcher, 5 prompts x 3 takes through 4 slots: on a pool of 13 pages takes are forked, the pool runs dry
    and dialogues are evicted and re-run; an unconstrained pool evicts nothing.  Same tokens and the same lp either way,
    equal to the batcher on the expanded prompt list (queued takes), and tokens equal to a run with scores off."""
    from mtts.scheduler import ContinuousBatcher
    cfg = synth.tiny()
    w = synth.synth_weights(cfg, 305, emb_row_sigma=0.6, speech_boost=6.0, eos_boost=1.0)
    layers, ds = ([dict(top_k=40, top_p=0.9, temperature=1.1, repetition_penalty=1.2)] * 8, [True] * 8)
    rng = np.random.default_rng(12)
    prompts = [_plain_prompt(rng, int(rng.integers(70, 120))) for _ in range(5)]
    mnts = [int(rng.integers(200, 240)) for _ in range(5)]
    seeds, rows, n = list(range(700, 705)), [3, 1, 4, 1, 5], 3
    runs = []
    for pool in (13, 0):
        eng = _engine(cfg, w, max_batch=4, max_seq_len=384, kv_pool_pages=pool)
        cb = ContinuousBatcher(eng, slots=4, gen_cap=260, layers=layers, do_samples=ds, steps_per_poll=8)
        off = cb.run(prompts, mnts, seeds=seeds, row_ids=rows, takes=n)
        on, sc = cb.run(prompts, mnts, seeds=seeds, row_ids=rows, takes=n, output_scores=True)
        assert (cb.evictions > 0) == (pool == 13) and cb.forks > 0
        for k in range(5 * n):
            assert _eq(on[k], off[k]), k
            assert sc[k].shape == (on[k].shape[0] - (prompts[k // n].shape[0] - 7), 8) and sc[k].dtype == np.float32
        runs.append((on, sc))
        if pool == 0:
            ex, ex_sc = cb.run([p for p in prompts for _ in range(n)], [m for m in mnts for _ in range(n)],
                               seeds=[s for s in seeds for _ in range(n)], row_ids=[r * n + j for r in rows for j in range(n)],
                               output_scores=True)
            for k in range(5 * n):
                assert _eq(ex[k], on[k]) and _eq(ex_sc[k], sc[k]), k
        eng.close()
    for k in range(5 * n):
        assert _eq(runs[0][0][k], runs[1][0][k]) and _eq(runs[0][1][k], runs[1][1][k]), k
        assert np.isfinite(runs[0][1][k]).sum() > 100


# ---- 5. drop-in surface ----------------------------------------------------------------------------------------------------
def test_dropin_return_dict_in_generate():
    from modeling_asteroid import AsteroidTTSInstruct, GenerateOutput, GenerationConfig
    cfg = synth.tiny()
    w = {k: torch.from_numpy(v) for k, v in _weights(cfg, 307).items()}
    gc = GenerationConfig(do_sample=True, top_k=30, top_p=0.9, temperature=1.0, repetition_penalty=1.1,
                          eos_token_id=cfg["eos_token_id"])
    m = AsteroidTTSInstruct.from_state_dict(cfg, w, gc).to("cuda")
    ids, mask = synth.synth_prompts(cfg, 41, 3, 40, 0.4, True)
    ids, mask = torch.from_numpy(ids), torch.from_numpy(mask)
    n = 2
    plain = m.generate(ids, mask, max_new_tokens=32, num_return_sequences=n, seed=5)
    out = m.generate(ids, mask, max_new_tokens=32, num_return_sequences=n, seed=5, return_dict_in_generate=True,
                     output_scores=True)
    assert isinstance(out, GenerateOutput) and out.scores is None
    assert torch.equal(out.sequences, plain)
    G = plain.shape[1] - (ids.shape[1] - 7)
    assert out.transition_scores.shape == (3 * n, G, 8) and out.transition_scores.dtype == torch.float32
    assert out.transition_scores.device == ids.device
    assert out.sequences_scores.shape == (3 * n,)
    assert torch.equal(out.sequences_scores, torch.nansum(out.transition_scores, dim=(1, 2)))
    assert (out.sequences_scores < 0).all()
    bare = m.generate(ids, mask, max_new_tokens=32, num_return_sequences=n, seed=5, return_dict_in_generate=True)
    assert torch.equal(bare.sequences, plain) and bare.transition_scores is None and bare.sequences_scores is None
    assert torch.equal(m.generate(ids, mask, max_new_tokens=32, num_return_sequences=n, seed=5, output_scores=True), plain)
    with pytest.raises(ValueError, match="output_logits"):
        m.generate(ids, mask, max_new_tokens=8, return_dict_in_generate=True, output_logits=True)
    # more rows than one engine pass: the scheduled path pads lp with NaN behind each dialogue's own end
    big_ids, big_mask = synth.synth_prompts(cfg, 42, 44, 40, 0.4, True)
    big_ids, big_mask = torch.from_numpy(big_ids), torch.from_numpy(big_mask)
    plain = m.generate(big_ids, big_mask, max_new_tokens=24, num_return_sequences=3, seed=9)
    out = m.generate(big_ids, big_mask, max_new_tokens=24, num_return_sequences=3, seed=9, return_dict_in_generate=True,
                     output_scores=True)
    assert plain.shape[0] == 132 and torch.equal(out.sequences, plain)
    G = plain.shape[1] - (big_ids.shape[1] - 7)
    assert out.transition_scores.shape == (132, G, 8)
    assert torch.equal(out.sequences_scores, torch.nansum(out.transition_scores, dim=(1, 2)))
    # rows 0..11 as one static batch with the same seed and row ids: the same lp wherever the tokens agree
    few = m.generate(big_ids[:4], big_mask[:4], max_new_tokens=24, num_return_sequences=3, seed=9,
                     return_dict_in_generate=True, output_scores=True)
    g = min(G, few.transition_scores.shape[1])
    for r in range(12):
        if torch.equal(few.sequences[r, :big_ids.shape[1] - 7 + g], plain[r, :big_ids.shape[1] - 7 + g]):
            a, b = few.transition_scores[r, :g].cpu().numpy(), out.transition_scores[r, :g].cpu().numpy()
            both = np.isfinite(a) & np.isfinite(b)
            assert both.any() and np.array_equal(a[both], b[both]), r
