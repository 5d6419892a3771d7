"""generate(top_logprobs=k): the model's own distribution at every decode decision.  -m gpu.

For step g, row r, channel c: L = the step's logits row in fp32 with the two hard-coded masks and no processor,
d = the sampler's decision; logprobs = log_softmax(L)[d], top_ids / top_logprobs = the first k tokens of L under
(descending logit, ascending id, -0 = +0) with their log_softmax(L) (include/mtts.h: mtts_set_top_logprobs;
mtts/topk_spec.py: gen_logprobs_spec states it in float64).

ids are compared exactly.  Values: scores_ref.KERNEL_TOL = 2e-5, the budget derived at the top of test_scores_gpu.py for
"a per-thread fp32 partial of at most 19 terms with fp64 above it".  csrc/gen_topk.hip sums that way: a thread adds the
expf(l - M) of its columns in fp32 -- ceil(ceil(152 697 / 32) / 256) = 19 terms in a slice of channel 0, at most 16 in a
row one block scans (<= 4096 columns), 1 in the 130-column slices of V = 4 133 -- the 256 thread sums and the 32 slice
sums are added in fp64, and l - (M + log S) is formed in fp64 and rounded once.  So the terms of that budget bound this
kernel too (the one rounding of |l - M| < 64 <= 3.8e-6, expf and the fp32 partial <= 3e-6 relative on a sum >= 1, the
log <= 1e-6, doubled).  Every test prints its measured maximum.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from mtts import capi, synth, topk_spec  # noqa: E402
from oracle import asteroid_oracle as ao  # noqa: E402

import scores_ref as sr  # noqa: E402

TOL = sr.KERNEL_TOL
KS = (1, 5, 16)
GREEDY = ([dict(repetition_penalty=1.3, temperature=0.8)] * 8, [False] * 8)
SAMPLED = sr.SCENARIO_SAMPLED


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else a.dtype)


def _eq(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b))


def _eq3(a, b):
    return all(_eq(x, y) for x, y in zip(a, b))


def _weights(cfg, seed=sr.SCENARIO["weight_seed"], bf16=True):
    return synth.synth_weights(cfg, seed, bf16=bf16, **sr.SCENARIO["wkw"])


def _engine(cfg, w, **kw):
    from mtts.engine import Engine
    kw.setdefault("max_batch", 8)
    kw.setdefault("max_seq_len", 256)
    eng = Engine(cfg, **kw)
    eng.bind_state_dict(w)
    return eng


# ---- 1. the kernels against gen_logprobs_spec on the same logits --------------------------------------------------------
def _mask_id(V):
    return {1025: 1024, 152697: 152694}.get(V, V - 33)         # V = 4 133: id 4 100, in the ragged last slice


def _planted(V, rows, f32, seed):
    """Random logits (bf16 values, or unrounded fp32) and decisions; the first rows carry the planted cases."""
    rng = np.random.default_rng(seed)
    lg = rng.standard_normal((rows, V)).astype(np.float32) * 2.5
    mask = _mask_id(V)
    dec = rng.integers(0, V, rows)
    far = [5, V // 2, V - 5]                                     # first, a middle and the last slice
    lg[0, far] = 12.0                                            # equal maxima in different slices: ascending id across the merge
    dec[0] = V - 5                                               # ... and the decision in the last slice, among the k best
    if rows > 1:
        lg[1] = 1.25                                             # all equal: ids 0..k-1, every value -log(V - 1)
        dec[1] = V - 1
    if rows > 2:
        lg[2, mask] = 15.0                                       # the masked id holds the largest raw logit
        lg[2, mask - 1] = 14.0
        dec[2] = mask - 1
    if rows > 3:
        lg[3] = -np.abs(lg[3]) - 1.0
        lg[3, [7, 2, V - 2]] = [0.0, -0.0, 0.0]                  # -0 and +0 are one value: ids 2, 7, V - 2
        dec[3] = 2                                               # the decision reads -0 where the list holds +0
    if rows > 4:
        dec[4] = V - 1                                           # the very last column
    dec[dec == mask] = 0
    if not f32:
        lg = ao.round_bf16(lg)                                   # (the planted values are bf16 numbers)
    return lg, dec.astype(np.int32), mask


def _hook(lt, f32, mask, dec_t, k):
    rows, V = lt.shape
    lp = torch.full((rows,), 7.0, dtype=torch.float32, device="cuda")
    ids = torch.full((rows, k), -7, dtype=torch.int32, device="cuda")
    tlp = torch.full((rows, k), 7.0, dtype=torch.float32, device="cuda")
    capi.check(capi.lib().mtts_k_gen_topk(lt.data_ptr(), 1 if f32 else 0, rows, V, mask, dec_t.data_ptr(), k, lp.data_ptr(),
                                          ids.data_ptr(), tlp.data_ptr(), None))
    torch.cuda.synchronize()
    return lp.cpu().numpy(), ids.cpu().numpy(), tlp.cpu().numpy()


def _check_hook(V, rows, f32):
    lg, dec, mask = _planted(V, rows, f32, 100 + V % 89 + rows)
    lt = torch.from_numpy(lg).cuda() if f32 else torch.from_numpy(lg).to(torch.bfloat16).cuda()
    dt = torch.from_numpy(dec).cuda()
    want_lp, want_ids, want_tlp = topk_spec.gen_logprobs_spec(lg, mask, dec, 16)
    worst, got = 0.0, {}
    for k in KS:
        lp, ids, tlp = got[k] = _hook(lt, f32, mask, dt, k)
        assert _eq3(got[k], _hook(lt, f32, mask, dt, k))                        # two calls: the same bits
        assert np.array_equal(ids.astype(np.int64), want_ids[:, :k])            # the order, exactly
        worst = max(worst, np.abs(lp - want_lp).max(), np.abs(tlp - want_tlp[:, :k]).max())
        hit = ids == dec[:, None]                                               # the decision among the k best: one number
        assert np.array_equal(_bits(tlp)[hit], _bits(np.broadcast_to(lp[:, None], tlp.shape).copy())[hit])
        assert not (ids == mask).any()
    for k in KS[:-1]:                                                           # the first k' entries do not depend on k
        assert _eq(got[k][0], got[16][0]) and _eq(got[k][1], got[16][1][:, :k].copy()) and _eq(got[k][2], got[16][2][:, :k].copy())
    lp, ids, tlp = got[16]
    assert ids[0, :3].tolist() == [5, V // 2, V - 5] and (ids[0] == dec[0]).any()
    if rows > 1:
        assert ids[1].tolist() == list(range(16)) and np.abs(tlp[1] + np.log(V - 1)).max() <= TOL
        assert abs(lp[1] + np.log(V - 1)) <= TOL
    if rows > 3:
        assert ids[3, :3].tolist() == [2, 7, V - 2] and _bits(tlp[3, :1])[0] == _bits(lp[3:4])[0]
    print(f"gen_topk kernel V={V} rows={rows} {'fp32' if f32 else 'bf16'}: max |value - fp64| = {worst:.3e} (tolerance {TOL:.1e})")
    assert worst <= TOL


@pytest.mark.parametrize("f32", [False, True], ids=["bf16", "fp32"])
@pytest.mark.parametrize("rows", [1, 6, 33])
@pytest.mark.parametrize("V", [1025, 4133])
def test_kernel_vs_spec(V, rows, f32):
    """V = 1025: one block scans the row.  V = 4 133 > SAMP_CAND: the slice path, 130 columns per slice, 103 in the last."""
    _check_hook(V, rows, f32)


@pytest.mark.parametrize("f32", [False, True], ids=["bf16", "fp32"])
def test_kernel_vs_spec_full_vocabulary(f32):
    _check_hook(152697, 6, f32)


def test_hook_refuses_bad_arguments():
    lt = torch.zeros((2, 64), dtype=torch.bfloat16, device="cuda")
    dt = torch.zeros(2, dtype=torch.int32, device="cuda")
    out = torch.zeros(2 * 16, dtype=torch.float32, device="cuda")
    oi = torch.zeros(2 * 16, dtype=torch.int32, device="cuda")
    for rows, V, k in ((2, 64, 0), (2, 64, 17), (2, 8, 9), (129, 64, 1)):
        rc = capi.lib().mtts_k_gen_topk(lt.data_ptr(), 0, rows, V, -1, dt.data_ptr(), k, out.data_ptr(), oi.data_ptr(), out.data_ptr(), None)
        assert rc == capi.EINVAL


# ---- 2. the engine against its own logits ---------------------------------------------------------------------------------
def _step_mask_id(g, c):
    if c != 0 and g >= c:
        return 1024
    if c == 0 and g <= 6:
        return 152694
    return -1


@pytest.mark.parametrize("mode", ["greedy", "sampled"])
@pytest.mark.parametrize("dtype", ["bf16", "fp32", "fp16"])
def test_engine_vs_its_own_logits(dtype, mode):
    """begin, then per step read_logits() -> step(1) (a step samples from the last forward's logits, then runs the forward):
    every non-NaN slot against gen_logprobs_spec of that step's row at the token the engine appended (where a slot is the
    model's decision, the appended token is the sampler's raw decision).  The NaN / -1 pattern is that of the run's own
    transition scores and of the host state machine: the first 7 steps, an EOS flush, a row that finished early."""
    sc = sr.SCENARIO
    k = 5
    cfg = synth.tiny()
    w = _weights(cfg, bf16=(dtype == "bf16"))
    ids, mask = synth.synth_prompts(cfg, sc["prompt_seed"], sc["batch"], sc["prompt_len"], sc["audio_frac"], True)
    new = sc["new"]
    ml = ids.shape[1] + new
    base = ids.shape[1] - 7
    layers, ds = GREEDY if mode == "greedy" else SAMPLED
    eng = _engine(cfg, w, max_batch=4, dtype=dtype)
    eng.begin(ids, mask, ml, layers=layers, do_samples=ds, seed=sc["seed"], output_scores=True, top_logprobs=k)
    logs = []
    for _ in range(new + 8):
        logs.append(eng.read_logits())
        eng.step(1)
        _, done = eng.sync_state()
        if done:
            break
    gen = eng.read_generated(new + 16)
    lp = eng.read_scores(new + 16)
    rlp, tid, tlp = eng.read_top_logprobs(new + 16)
    eng.close()
    G = gen.shape[0]
    assert rlp.shape == gen.shape and rlp.dtype == np.float32
    assert tid.shape == gen.shape + (k,) and tid.dtype == np.int32 and tlp.shape == tid.shape and tlp.dtype == np.float32
    used = sr.used_mask(gen, base, ml, cfg)
    assert np.array_equal(np.isnan(rlp), np.isnan(lp)) and np.array_equal(np.isnan(rlp), ~used)
    assert np.array_equal(np.isnan(tlp), np.broadcast_to(~used[..., None], tlp.shape))
    assert np.array_equal(tid == -1, np.broadcast_to(~used[..., None], tid.shape))
    per_row = used.sum((0, 2))
    assert per_row.min() < per_row.max() and (gen[:, :, 0] == cfg["eos_token_id"]).any()      # a row flushed and left early
    assert not used[0, :, 1:].any() and used[0, :, 0].all()                                   # teacher forcing of the first steps
    worst, n = 0.0, 0
    for g in range(G):
        l0, l17 = logs[g]
        for c in range(8):
            rows = np.flatnonzero(used[g, :, c])
            if not rows.size:
                continue
            lg = (l0 if c == 0 else l17[c - 1])[rows]
            want_lp, want_ids, want_tlp = topk_spec.gen_logprobs_spec(lg, _step_mask_id(g, c), gen[g, rows, c], k)
            assert np.array_equal(tid[g, rows, c].astype(np.int64), want_ids), (g, c)
            worst = max(worst, np.abs(rlp[g, rows, c] - want_lp).max(), np.abs(tlp[g, rows, c] - want_tlp).max())
            hit = tid[g, rows, c] == gen[g, rows, c][:, None]
            assert np.array_equal(_bits(tlp[g, rows, c])[hit], _bits(np.repeat(rlp[g, rows, c][:, None], k, 1))[hit])
            n += rows.size
    print(f"engine top_logprobs {dtype} {mode}: {n} slots, max |value - fp64| = {worst:.3e} (tolerance {TOL:.1e})")
    assert n > 400 and worst <= TOL
    if mode == "greedy":
        # a greedy decision on the processed scores is not always the raw argmax (repetition penalty), but its raw
        # log-probability can never exceed the best one's
        assert (rlp[used] <= tlp[..., 0][used]).all()


# ---- 3. exact properties -------------------------------------------------------------------------------------------------
def test_on_changes_nothing_and_does_not_depend_on_the_batch():
    """Tokens and transition scores with top_logprobs on == off; values are run-to-run bit-identical; a row alone (same
    seed and row id) has the values it has inside a batch of 8; k = 16 then k = 4 then k = 16 on one engine: the buffers
    are re-allocated, the step graphs follow, and the first 4 entries do not depend on k."""
    cfg = synth.tiny()
    eng = _engine(cfg, _weights(cfg), max_batch=8)
    ids, mask = synth.synth_prompts(cfg, 104, 8, 24, 0.3, False)       # (no left padding: a row alone sees the same history)
    ml = ids.shape[1] + 44
    base = ids.shape[1] - 7
    for layers, ds in (GREEDY, SAMPLED):
        kw = dict(layers=layers, do_samples=ds, seed=5)
        off = eng.generate(ids, mask, ml, **kw)
        off_s, off_lp = eng.generate(ids, mask, ml, output_scores=True, **kw)
        on, top = eng.generate(ids, mask, ml, top_logprobs=16, **kw)
        on_s, on_lp, top_s = eng.generate(ids, mask, ml, output_scores=True, top_logprobs=16, **kw)
        assert _eq(on, off) and _eq(on_s, off) and _eq(off_s, off) and _eq(on_lp, off_lp) and _eq3(top, top_s)
        G = on.shape[1] - base
        assert top[0].shape == (8, G, 8) and top[1].shape == (8, G, 8, 16) and top[2].shape == (8, G, 8, 16)
        assert np.array_equal(np.isnan(top[0]), np.isnan(on_lp)) and np.isfinite(top[0]).sum() > 400
        assert (top[0][np.isfinite(top[0])] <= 0).all()
        assert (np.diff(top[2][np.isfinite(top[0])], axis=-1) <= 0).all()                # descending
        few = eng.generate(ids, mask, ml, top_logprobs=4, **kw)[1]
        assert _eq(few[0], top[0]) and _eq(few[1], top[1][..., :4].copy()) and _eq(few[2], top[2][..., :4].copy())
        assert _eq3(eng.generate(ids, mask, ml, top_logprobs=16, **kw)[1], top)
        for r in (0, 5):
            a_ids, a_top = eng.generate(ids[r:r + 1], mask[r:r + 1], ml, row_ids=[r], top_logprobs=16, **kw)
            g = a_ids.shape[1] - base
            assert _eq(a_ids[0], on[r, :base + g].copy())
            assert all(_eq(x[0], y[r, :g].copy()) for x, y in zip(a_top, top))
    eng.generate(ids, mask, ml)
    with pytest.raises(capi.MttsError) as ei:                        # the last run had k = 0
        eng.read_top_logprobs(64)
    assert ei.value.code == capi.ESTATE
    eng.close()


def test_switch_is_refused_while_a_run_is_open():
    cfg = synth.tiny()
    eng = _engine(cfg, _weights(cfg), max_batch=4)
    ids, mask = synth.synth_prompts(cfg, 104, 3, 24, 0.3, True)
    for k in (-1, 17):
        with pytest.raises(capi.MttsError) as ei:
            eng.set_top_logprobs(k)
        assert ei.value.code == capi.EINVAL
    eng.begin(ids, mask, ids.shape[1] + 44, output_scores=True)
    eng.step(3)
    with pytest.raises(capi.MttsError) as ei:
        eng.set_top_logprobs(4)
    assert ei.value.code == capi.ESTATE
    eng.set_top_logprobs(0)                                            # no change: fine
    eng.set_output_scores(True)
    with pytest.raises(capi.MttsError) as ei:
        eng.read_top_logprobs(16)                                      # the open run was started with k = 0
    assert ei.value.code == capi.ESTATE
    assert eng.read_scores(16).shape[0] == 3                           # the other switch is its own
    eng.close()


@pytest.mark.parametrize("knob", ["MTTS_GRAPHS", "MTTS_SMALL_ROWS"])
def test_equal_across_launch_paths(monkeypatch, knob):
    """Graph replay vs MTTS_GRAPHS=0 (stream launches), and the small-batch path (<= 4 rows) vs MTTS_SMALL_ROWS=0 (the
    general kernels): same tokens, same bits, greedy and sampled, 3 ragged rows."""
    cfg = synth.tiny()
    w = _weights(cfg)
    ids, mask = synth.synth_prompts(cfg, 104, 3, 24, 0.3, True)
    ml = ids.shape[1] + 90
    res = []
    for val in ("1" if knob == "MTTS_GRAPHS" else "4", "0"):
        monkeypatch.setenv(knob, val)
        eng = _engine(cfg, w, max_batch=4)
        res.append([eng.generate(ids, mask, ml, layers=layers, do_samples=ds, seed=5, top_logprobs=8)
                    for layers, ds in (GREEDY, SAMPLED)])
        eng.close()
    for (a_ids, a_top), (b_ids, b_top) in zip(*res):
        assert _eq(a_ids, b_ids) and _eq3(a_top, b_top)
        assert np.isfinite(a_top[0]).sum() > 400


# ---- 4. scheduler ----------------------------------------------------------------------------------------------------------
def _plain_prompt(rng, n):
    raw = np.full((n, 8), 1024, dtype=np.int64)
    raw[:, 0] = rng.integers(0, 151643, n)
    raw[n - 6:, 0] = 151665 + rng.integers(0, 1024, 6)
    raw[n - 6:, 1:] = rng.integers(0, 1024, (6, 7))
    return synth.shifting_inputs(raw, 151643)


def test_scheduler_values_survive_eviction_and_forks():
    """The scenario of test_scores_gpu.py::test_scheduler_lp_survives_eviction_and_forks: 5 prompts x 3 takes through 4
    slots on a pool of 13 pages -- takes are forked, the pool runs dry, dialogues are evicted and re-run.  Every job's three
    arrays equal, as bits, those of its own run as a static batch of one row with the same seed and row id."""
    from mtts.scheduler import ContinuousBatcher
    cfg = synth.tiny()
    w = synth.synth_weights(cfg, 305, emb_row_sigma=0.6, speech_boost=6.0, eos_boost=1.0)
    layers, ds = ([dict(top_k=40, top_p=0.9, temperature=1.1, repetition_penalty=1.2)] * 8, [True] * 8)
    rng = np.random.default_rng(12)
    prompts = [_plain_prompt(rng, int(rng.integers(70, 120))) for _ in range(5)]
    mnts = [int(rng.integers(200, 240)) for _ in range(5)]
    seeds, rows, n, k = list(range(700, 705)), [3, 1, 4, 1, 5], 3, 6
    eng = _engine(cfg, w, max_batch=4, max_seq_len=384, kv_pool_pages=13)
    cb = ContinuousBatcher(eng, slots=4, gen_cap=260, layers=layers, do_samples=ds, steps_per_poll=8)
    off = cb.run(prompts, mnts, seeds=seeds, row_ids=rows, takes=n)
    on, sc, tops = cb.run(prompts, mnts, seeds=seeds, row_ids=rows, takes=n, top_logprobs=k)
    assert sc is None and cb.evictions > 0 and cb.forks > 0
    on2, sc2, tops2 = cb.run(prompts, mnts, seeds=seeds, row_ids=rows, takes=n, top_logprobs=k, output_scores=True)
    eng.close()
    eng = _engine(cfg, w, max_batch=4, max_seq_len=384)
    for j in range(5 * n):
        p = prompts[j // n]
        T = p.shape[0]
        assert _eq(on[j], off[j]) and _eq(on2[j], off[j]), j
        G = on[j].shape[0] - (T - 7)
        assert tops[0][j].shape == (G, 8) and tops[1][j].shape == (G, 8, k) and tops[2][j].shape == (G, 8, k)
        assert np.array_equal(np.isnan(tops[0][j]), np.isnan(sc2[j])) and all(_eq(tops[i][j], tops2[i][j]) for i in range(3))
        a_ids, a_top = eng.generate(p[None], np.ones((1, T)), T + mnts[j // n], layers=layers, do_samples=ds, seed=seeds[j // n],
                                    row_ids=[rows[j // n] * n + j % n], top_logprobs=k)
        assert _eq(a_ids[0, :T - 7 + G].copy(), on[j]), j
        assert all(_eq(np.ascontiguousarray(a_top[i][0, :G]), tops[i][j]) for i in range(3)), j
        assert np.isfinite(tops[0][j]).sum() > 100
    eng.close()


# ---- 5. drop-in surface ----------------------------------------------------------------------------------------------------
def test_dropin_generate_top_logprobs():
    from modeling_asteroid import AsteroidTTSInstruct, GenerateOutput, GenerationConfig
    cfg = synth.tiny()
    w = {k: torch.from_numpy(v) for k, v in _weights(cfg, 307).items()}
    gc = GenerationConfig(do_sample=True, top_k=30, top_p=0.9, temperature=1.0, repetition_penalty=1.1,
                          eos_token_id=cfg["eos_token_id"])
    m = AsteroidTTSInstruct.from_state_dict(cfg, w, gc).to("cuda")
    ids, mask = synth.synth_prompts(cfg, 41, 3, 40, 0.4, True)
    ids, mask = torch.from_numpy(ids), torch.from_numpy(mask)
    n, k = 3, 5
    kw = dict(max_new_tokens=32, num_return_sequences=n, seed=5)
    plain = m.generate(ids, mask, **kw)
    G = plain.shape[1] - (ids.shape[1] - 7)
    out = m.generate(ids, mask, return_dict_in_generate=True, top_logprobs=k, **kw)
    both = m.generate(ids, mask, return_dict_in_generate=True, top_logprobs=k, output_scores=True, **kw)
    scores = m.generate(ids, mask, return_dict_in_generate=True, output_scores=True, **kw)
    assert scores.logprobs is None and scores.top_ids is None and scores.top_logprobs is None
    for o in (out, both):
        assert isinstance(o, GenerateOutput) and o.scores is None and o.logits is None
        assert torch.equal(o.sequences, plain)
        assert o.logprobs.shape == (3 * n, G, 8) and o.logprobs.dtype == torch.float32
        assert o.top_ids.shape == (3 * n, G, 8, k) and o.top_ids.dtype == torch.int64
        assert o.top_logprobs.shape == (3 * n, G, 8, k) and o.top_logprobs.dtype == torch.float32
        assert o.logprobs.device == ids.device and o.top_ids.device == ids.device and o.top_logprobs.device == ids.device
    assert out.transition_scores is None and out.sequences_scores is None
    assert np.array_equal(both.transition_scores.numpy(), scores.transition_scores.numpy(), equal_nan=True)
    assert np.array_equal(torch.isnan(both.logprobs).numpy(), torch.isnan(both.transition_scores).numpy())
    assert np.array_equal(out.logprobs.numpy(), both.logprobs.numpy(), equal_nan=True) and torch.equal(out.top_ids, both.top_ids)
    assert ((out.top_ids == -1) == torch.isnan(out.top_logprobs)).all()
    with pytest.raises(ValueError, match="output_logits"):
        m.generate(ids, mask, max_new_tokens=8, return_dict_in_generate=True, output_logits=True, top_logprobs=k)
    # more rows than one engine pass: 44 prompts x 3 takes through the batcher, padded with NaN / -1 behind each dialogue's end
    big_ids, big_mask = synth.synth_prompts(cfg, 42, 44, 40, 0.4, True)
    big_ids, big_mask = torch.from_numpy(big_ids), torch.from_numpy(big_mask)
    kw = dict(max_new_tokens=24, num_return_sequences=3, seed=9)
    plain = m.generate(big_ids, big_mask, **kw)
    out = m.generate(big_ids, big_mask, return_dict_in_generate=True, top_logprobs=k, output_scores=True, **kw)
    assert plain.shape[0] == 132 and torch.equal(out.sequences, plain)
    G = plain.shape[1] - (big_ids.shape[1] - 7)
    assert out.logprobs.shape == (132, G, 8) and out.top_ids.shape == (132, G, 8, k) and out.top_logprobs.shape == (132, G, 8, k)
    assert out.top_ids.dtype == torch.int64 and out.transition_scores.shape == (132, G, 8)
    assert np.array_equal(torch.isnan(out.logprobs).numpy(), torch.isnan(out.transition_scores).numpy())
    assert ((out.top_ids == -1) == torch.isnan(out.top_logprobs)).all() and torch.isfinite(out.logprobs).sum() > 132 * 20
    # rows 0..11 as one static batch with the same seed and row ids: the same values wherever the tokens agree
    few = m.generate(big_ids[:4], big_mask[:4], return_dict_in_generate=True, top_logprobs=k, **kw)
    g = min(G, few.logprobs.shape[1])
    for r in range(12):
        if torch.equal(few.sequences[r, :big_ids.shape[1] - 7 + g], plain[r, :big_ids.shape[1] - 7 + g]):
            a, b = few.top_logprobs[r, :g].numpy(), out.top_logprobs[r, :g].numpy()
            ok = np.isfinite(a) & np.isfinite(b)
            assert ok.any() and np.array_equal(a[ok], b[ok]) and np.array_equal(few.top_ids[r, :g].numpy()[ok], out.top_ids[r, :g].numpy()[ok]), r
