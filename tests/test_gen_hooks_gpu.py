"""generate(logits_processor=, stopping_criteria=, streamer=) on the device: the split decode step.  -m gpu.

The toy model of the sampler tests (2 layers, H 256, synthetic weights), B = 3 ragged left-padded prompts of at most 20
slots, at most 24 new tokens.  The references: tests/hooks_ref.py for the materialised score row (held against HF's own
processors by test_gen_hooks_cpu.py), the plain generate() call for everything a hook must not change, the installed
transformers' processors for what a custom processor must do, and scores_ref.used_mask for where the state machine lets a
channel choose.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import modeling_asteroid as ma  # noqa: E402
from mtts import capi, synth  # noqa: E402
from mtts.engine import Engine, sampler_cfgs  # noqa: E402

import hooks_ref as hr  # noqa: E402
import scores_ref as sr  # noqa: E402

NEW = 24
SAMPLED = dict(do_sample=True, top_k=20, top_p=0.9, temperature=0.9, repetition_penalty=1.1)
GREEDY = dict(repetition_penalty=1.1)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a) if a.is_floating_point() else a, _bits(b) if b.is_floating_point() else b)


@pytest.fixture(scope="module")
def toy():
    sc = sr.SCENARIO
    cfg = synth.tiny()
    ids, mask = synth.synth_prompts(cfg, sc["prompt_seed"], 3, 20, sc["audio_frac"], True)
    assert ids.shape[1] <= 20 and (mask[:, :ids.shape[1] - 7] == 0).any()         # ragged: a left-padded row
    weights = {dt: synth.synth_weights(cfg, sc["weight_seed"], bf16=(dt == "bf16"), **sc["wkw"]) for dt in ("bf16", "fp32")}
    return cfg, weights, torch.from_numpy(ids), torch.from_numpy(mask)


def _new_model(toy, dtype):
    cfg, weights, _, _ = toy
    return ma.AsteroidTTSInstruct.from_state_dict(cfg, weights[dtype], ma.GenerationConfig(eos_token_id=cfg["eos_token_id"]), dtype=dtype).to("cuda")


@pytest.fixture(scope="module")
def models(toy):
    """One resident model per dtype for the whole module; a test sets its generation_config."""
    made = {}

    def get(dtype, **gen):
        if dtype not in made:
            made[dtype] = _new_model(toy, dtype)
        made[dtype].generation_config = ma.GenerationConfig(eos_token_id=toy[0]["eos_token_id"], **gen)
        return made[dtype]

    yield get
    for m in made.values():
        if m._engine is not None:
            m._engine.close()


def _gen(m, toy, **kw):
    _, _, ids, mask = toy
    kw.setdefault("seed", 5)
    return m.generate(ids, mask, max_new_tokens=NEW, **kw)


def _steps(seq, toy):
    """[B, base + G, 8] sequences -> (generated part as numpy [G, B, 8], base)."""
    base = toy[2].shape[1] - 7
    return np.ascontiguousarray(seq[:, base:].cpu().numpy().transpose(1, 0, 2)), base


def _padding(cfg):
    return np.array([cfg["eos_token_id"]] + [cfg["speech_pad_token"]] * 7)


# ---- 1. the kernel ---------------------------------------------------------------------------------------------------------
def _tables(tabs):
    raw = np.zeros((len(tabs), C.sizeof(capi.MttsBiasTable) // 4), dtype=np.int32)
    for r, (ids, terms) in enumerate(tabs):
        raw[r, 0] = len(ids)
        raw[r, 1:1 + len(ids)] = ids
        raw[r, 65:65 + len(ids)] = np.asarray(terms, dtype=np.float32).view(np.int32)
    return raw


@pytest.mark.parametrize("rows,V", [(4, 1025), (2, 152697)])
def test_scores_materialize_kernel_is_hooks_ref_bit_for_bit(rows, V):
    """One [4, 1025] and one [2, 152697] matrix whose rows carry a masked id, banned bits (one in the last, partial word), terms
    (one on a penalised token whose sign it flips), a penalised negative and a penalised positive logit.  The kernel's rows
    equal hooks_ref.materialized on the bits although the channel's config has a temperature (it is not applied), the pad
    columns up to the next multiple of 32 hold -inf, and without ban words, terms and bitmap the row is the masked logits."""
    lib = capi.lib()
    logits, hist, banned, tabs = hr.case(rows, V)
    want = hr.materialized(logits, hist, banned, tabs, hr.PENALTY, hr.MASKED[V])
    lt = torch.from_numpy(np.array(logits)).to(torch.bfloat16).cuda()
    assert np.array_equal(lt.float().cpu().numpy(), logits)                      # the case is made of bf16 values
    bm = torch.from_numpy(hr.bitmap(hist, V).view(np.int32)).cuda()
    ban = torch.from_numpy(hr.words(banned).view(np.int32)).cuda()
    bits = np.zeros((rows, V), dtype=bool)
    for r, (ids, _) in enumerate(tabs):
        bits[r, ids] = True
    bw = torch.from_numpy(hr.words(bits).view(np.int32)).cuda()
    tab = torch.from_numpy(_tables(tabs)).cuda()
    cfg = sampler_cfgs([dict(repetition_penalty=hr.PENALTY, temperature=0.7, top_k=5)] * 8, [True] * 8)[0]
    Vp = (V + 31) // 32 * 32
    channel = 0 if V > 2000 else 1
    out = torch.full((rows, Vp), float("nan"), dtype=torch.float32, device="cuda")
    capi.check(lib.mtts_k_scores_materialize(lt.data_ptr(), rows, V, bm.data_ptr(), C.byref(cfg), hr.MASKED[V], 3, channel, ban.data_ptr(),
                                             bw.data_ptr(), tab.data_ptr(), out.data_ptr(), None))
    got = out.cpu().numpy()
    assert np.array_equal(got[:, :V].view(np.uint32), want.view(np.uint32)), np.argwhere(got[:, :V].view(np.uint32) != want.view(np.uint32))[:5]
    assert np.isneginf(got[:, V:]).all() and Vp > V
    pen = np.float32(hr.PENALTY)
    assert np.isneginf(got[:, [hr.MASKED[V], hr.BANNED, hr.BANNED_PAIR, V - 1]]).all()
    assert (got[:, hr.NEG_HIST] == np.float32(-1.25) * pen).all() and (got[:, hr.POS_HIST] == np.float32(2.5) / pen).all()
    assert (got[:, hr.TERM_FLIP] == np.float32(0.5) / pen).all()
    # nothing but the mask
    out.fill_(float("nan"))
    capi.check(lib.mtts_k_scores_materialize(lt.data_ptr(), rows, V, None, C.byref(cfg), hr.MASKED[V], 3, channel, None, None, None,
                                             out.data_ptr(), None))
    bare = hr.materialized(logits, hist, np.zeros_like(banned), [(np.zeros(0, np.int32), np.zeros(0, np.float32))] * rows, 0.0, hr.MASKED[V])
    assert np.array_equal(out.cpu().numpy()[:, :V].view(np.uint32), bare.view(np.uint32))
    # refusals of the hook
    assert lib.mtts_k_scores_materialize(lt.data_ptr(), rows, V, None, C.byref(cfg), hr.MASKED[V], 3, channel, None, bw.data_ptr(), None,
                                         out.data_ptr(), None) == capi.EINVAL
    assert lib.mtts_k_scores_materialize(lt.data_ptr(), rows, V, None, C.byref(cfg), hr.MASKED[V], 3, channel, None, None, None,
                                         out.data_ptr() + 4, None) == capi.EINVAL


# ---- 2. transparency -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,gen,n", [("bf16", GREEDY, 1), ("bf16", SAMPLED, 2), ("fp32", GREEDY, 1), ("fp32", SAMPLED, 2)])
def test_identity_hooks_change_nothing(toy, models, dtype, gen, n):
    """An identity processor (it returns a copy, so the rows travel to the host framework and back), a criterion that is never
    true and a recording streamer, all at once: sequences, transition_scores, logprobs, top_ids and top_logprobs are those of
    the plain call on the bits -- the split step runs the same fp32 operations in the same order."""
    m = models(dtype, **gen)
    kw = dict(return_dict_in_generate=True, output_scores=True, top_logprobs=3)
    if n > 1:
        kw["num_return_sequences"] = n
    plain = _gen(m, toy, **kw)
    ident, never, rec = hr.Identity(), hr.Never(), hr.Recorder()
    got = _gen(m, toy, logits_processor=[ident], stopping_criteria=[never], streamer=rec, **kw)
    G = plain.sequences.shape[1] - (toy[2].shape[1] - 7)
    assert plain.sequences.shape[0] == 3 * n and G >= 8
    assert torch.equal(got.sequences, plain.sequences)
    for name in ("transition_scores", "logprobs", "top_ids", "top_logprobs"):
        assert _same(getattr(got, name), getattr(plain, name)), (dtype, n, name)
    assert torch.isfinite(plain.transition_scores).sum() > 20
    base = toy[2].shape[1] - 7
    assert ident.calls == 8 * G and never.lens == [base + 1 + t for t in range(G)]
    assert len(rec.events) == G + 2


# ---- 3. the streamer ---------------------------------------------------------------------------------------------------------
def test_streamer_gets_the_prompt_then_every_step_then_end(toy, models):
    """This fails on the parent commit, where nothing is ever put."""
    m = models("bf16", **SAMPLED)
    rec = hr.Recorder()
    seq = _gen(m, toy, streamer=rec)
    base = toy[2].shape[1] - 7
    G = seq.shape[1] - base
    kinds = [e[0] for e in rec.events]
    assert kinds == ["put"] * (G + 1) + ["end"], kinds
    first = rec.events[0][1]
    assert first.device.type == "cpu" and torch.equal(first, toy[2])
    for t in range(G):
        v = rec.events[1 + t][1]
        assert v.device.type == "cpu" and v.dtype == torch.int64 and tuple(v.shape) == (3,)
        assert torch.equal(v, seq[:, base + t, 0].cpu()), t
    assert torch.equal(seq, _gen(m, toy))                                       # and the tokens are the plain call's


# ---- 4. custom processors equal the built-in ones ------------------------------------------------------------------------------
@pytest.mark.parametrize("gen", [GREEDY, SAMPLED], ids=["greedy", "sampled"])
def test_hf_processors_as_custom_equal_the_device_keywords(toy, models, gen):
    """transformers' SuppressTokens, NoRepeatNGram(2) and MinNewTokensLength processors passed as logits_processor= give the
    tokens (and transition scores) of the device keywords suppress_tokens, no_repeat_ngram_size=2 and min_new_tokens: a -inf
    is a -inf on either side of the penalty.  The settings bite: the run differs from the plain one.  This fails on the
    parent commit, where the custom list is dropped."""
    lp = pytest.importorskip("transformers.generation.logits_process")
    cfg = toy[0]
    m = models("bf16", **gen)
    kw = dict(return_dict_in_generate=True, output_scores=True)
    plain = _gen(m, toy, **kw)
    free, base = _steps(plain.sequences, toy)
    T = toy[2].shape[1]
    suppress = sorted({int(t) for t in free[8:10].reshape(-1)} - {cfg["eos_token_id"], cfg["speech_pad_token"]})
    assert len(suppress) >= 4 and min(suppress) < 1025 < max(suppress)            # ids of the speech channels and of channel 0
    want = _gen(m, toy, suppress_tokens=suppress, no_repeat_ngram_size=2, min_new_tokens=6, **kw)
    procs = [lp.NoRepeatNGramLogitsProcessor(2), lp.MinNewTokensLengthLogitsProcessor(T, 6, cfg["eos_token_id"], device="cuda"),
             lp.SuppressTokensLogitsProcessor(suppress, device="cuda")]
    got = _gen(m, toy, logits_processor=lp.LogitsProcessorList(procs), **kw)
    assert not torch.equal(want.sequences[:, :plain.sequences.shape[1]], plain.sequences[:, :want.sequences.shape[1]])
    assert torch.equal(got.sequences, want.sequences)
    assert _same(got.transition_scores, want.transition_scores)
    # half of them on each side
    mixed = _gen(m, toy, logits_processor=procs[2:], no_repeat_ngram_size=2, min_new_tokens=6, **kw)
    assert torch.equal(mixed.sequences, want.sequences) and _same(mixed.transition_scores, want.transition_scores)


# ---- 5. forcing ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gen", [GREEDY, SAMPLED], ids=["greedy", "sampled"])
def test_a_processor_that_leaves_one_token_forces_it(toy, models, gen):
    """One finite token per channel, alternating with the parity of the history's length: wherever the state machine lets the
    channel choose, that token is emitted and its transition score is 0 (the log-softmax over a kept set of one)."""
    cfg = toy[0]
    lo = cfg["speech_token_range"][0]
    m = models("bf16", **gen)
    force = hr.Force(token=(lo + 3, 5), alt=(lo + 9, 6))
    out = _gen(m, toy, logits_processor=[force], return_dict_in_generate=True, output_scores=True)
    gen_t, base = _steps(out.sequences, toy)
    used = sr.used_mask(gen_t, base, toy[2].shape[1] + NEW, cfg)
    ts = out.transition_scores.cpu().numpy().transpose(1, 0, 2)
    assert gen_t.shape[0] == NEW + 7 and used.sum() > 300                         # speech tokens only: every row runs to max_length
    for g in range(gen_t.shape[0]):
        pair = force.token if (base + g) % 2 == 0 else force.alt
        for c in range(8):
            u = used[g, :, c]
            assert (gen_t[g, u, c] == pair[0 if c == 0 else 1]).all(), (g, c, gen_t[g, :, c])
            assert (ts[g, u, c] == 0).all() and np.isnan(ts[g, ~u, c]).all(), (g, c, ts[g, :, c])


# ---- 6. stopping criteria ------------------------------------------------------------------------------------------------------
def _first_padding(rows_gbc, r, pad):
    """The step from which row r emits nothing but finished-row padding (G if it never does)."""
    G = rows_gbc.shape[0]
    f = G
    while f > 0 and (rows_gbc[f - 1, r] == pad).all():
        f -= 1
    return f


def test_a_criterion_stops_one_row_and_leaves_the_others(toy, models):
    """True for row 1 after step 5 only.  Row 1 is the plain run's through step 5 and emits the reference's padding at step 6
    (:155-158); like a row that max_length finished it is still evaluated (:140-141), so all that can follow is EOS on
    channel 0 -- padding, or the flush of a resurrection.  Rows 0 and 2 are the plain run's on the bits, tokens and scores,
    and the call ends when the last row does."""
    cfg = toy[0]
    pad = _padding(cfg)
    m = models("bf16", **SAMPLED)
    kw = dict(return_dict_in_generate=True, output_scores=True)
    plain = _gen(m, toy, **kw)
    p, base = _steps(plain.sequences, toy)
    used = sr.used_mask(p, base, toy[2].shape[1] + NEW, cfg)
    assert used[5, 1, 0] and used[6, 1, 0], "the scenario's row 1 is past its own end at step 5"
    got = _gen(m, toy, stopping_criteria=[hr.StopAt([1], base + 6)], **kw)
    g, _ = _steps(got.sequences, toy)
    G = g.shape[0]
    assert np.array_equal(g[:6, 1], p[:6, 1]) and (g[6, 1] == pad).all() and (g[6:, 1, 0] == cfg["eos_token_id"]).all()
    n = min(G, p.shape[0])
    ts_p, ts_g = plain.transition_scores.cpu().numpy(), got.transition_scores.cpu().numpy()
    for r in (0, 2):
        assert np.array_equal(g[:n, r], p[:n, r]) and (g[n:, r] == pad).all() and (p[n:, r] == pad).all(), r
        assert np.array_equal(ts_g[r, :n].view(np.uint32), ts_p[r, :n].view(np.uint32)), r
    assert not np.array_equal(g[6, 1], p[6, 1])
    ends = [_first_padding(g, r, pad) for r in range(3)]
    assert G == max(ends) and G <= p.shape[0], (G, ends, p.shape[0])
    if ends[1] == 6:                                                             # no resurrection: rows 0 and 2 alone decide
        assert G == max(_first_padding(p, 0, pad), _first_padding(p, 2, pad), 6)
    # a criterion for every row ends the call at once: step 2 is the last
    short = _gen(m, toy, stopping_criteria=[hr.StopAt([0, 1, 2], base + 3)])
    assert short.shape[1] == base + 3 and torch.equal(short, plain.sequences[:, :base + 3])


def test_a_row_stopped_inside_its_flush_finishes_the_flush(toy, models):
    """A processor forces a text token on channel 0 at step 3: every row starts its 7-step EOS flush there.  A criterion that
    is true for every row from step 4 on, inside the flush, changes nothing: the run is that of the processor alone, flush
    complete.  The same criterion from step 1 on, in front of the flush, ends the run after step 1."""
    cfg = toy[0]
    lo = cfg["speech_token_range"][0]
    m = models("bf16", **GREEDY)
    base = toy[2].shape[1] - 7

    class FlushAt3(hr.Force):
        def __call__(self, input_ids, scores):
            if scores.shape[-1] > 2000 and input_ids.shape[1] == base + 3:
                out = torch.full_like(scores, float("-inf"))
                out[:, 7] = 0.0
                return out
            return super().__call__(input_ids, scores)

    force = FlushAt3(token=(lo + 3, 5), alt=(lo + 9, 6))
    alone = _gen(m, toy, logits_processor=[force])
    a, _ = _steps(alone, toy)
    assert a.shape[0] == 10 and (a[3, :, 0] == 7).all() and (a[4:, :, 0] == cfg["eos_token_id"]).all()     # steps 3..9: the pick, then six EOS
    assert (a[9, :, 7] != cfg["speech_pad_token"]).all() and (a[9, :, 1:7] == cfg["speech_pad_token"]).all()
    inside = _gen(m, toy, logits_processor=[force], stopping_criteria=[hr.StopAt([0, 1, 2], base + 5, onward=True)])
    assert torch.equal(inside, alone)
    before = _gen(m, toy, logits_processor=[force], stopping_criteria=[hr.StopAt([0, 1, 2], base + 2, onward=True)])
    assert before.shape[1] == base + 2 and torch.equal(before, alone[:, :base + 2])


# ---- 7. a row of -inf ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gen", [GREEDY, SAMPLED], ids=["greedy", "sampled"])
def test_a_row_of_minus_infinity_gives_token_0_and_nan(toy, models, gen):
    """Row 2 is set to -inf on every channel at step 9, in place in the engine's own rows: token 0 with a NaN score wherever
    the step's token is the model's decision, as for a row whose every token is banned; no fault, and rows 0 and 1 are the
    plain run's on the bits."""
    cfg = toy[0]
    m = models("bf16", **gen)
    kw = dict(return_dict_in_generate=True, output_scores=True)
    plain = _gen(m, toy, **kw)
    p, base = _steps(plain.sequences, toy)
    used_p = sr.used_mask(p, base, toy[2].shape[1] + NEW, cfg)
    assert used_p[9, 2].all(), "the scenario's row 2 is not free on every channel at step 9"
    got = _gen(m, toy, logits_processor=[hr.AllInfRow(2, base + 9)], **kw)
    g, _ = _steps(got.sequences, toy)
    ts = got.transition_scores.cpu().numpy()
    assert np.array_equal(g[:9, 2], p[:9, 2]) and (g[9, 2] == 0).all() and np.isnan(ts[2, 9]).all()
    assert np.array_equal(ts[2, :9].view(np.uint32), plain.transition_scores.cpu().numpy()[2, :9].view(np.uint32))
    n = min(g.shape[0], p.shape[0])
    for r in (0, 1):
        assert np.array_equal(g[:n, r], p[:n, r]), r
        assert np.array_equal(ts[r, :n].view(np.uint32), plain.transition_scores.cpu().numpy()[r, :n].view(np.uint32)), r


# ---- 8. the plans are kept apart -------------------------------------------------------------------------------------------------
def test_a_plain_call_after_a_hooked_one_is_a_fresh_engines(toy, models):
    m = models("bf16", **SAMPLED)
    kw = dict(return_dict_in_generate=True, output_scores=True)
    _gen(m, toy, logits_processor=[hr.Force(token=(toy[0]["speech_token_range"][0], 5), alt=(toy[0]["speech_token_range"][0] + 1, 6))],
         streamer=hr.Recorder(), **kw)
    after = _gen(m, toy, **kw)
    fresh_model = _new_model(toy, "bf16")
    fresh_model.generation_config = m.generation_config
    fresh = _gen(fresh_model, toy, **kw)
    fresh_model._engine.close()
    assert torch.equal(after.sequences, fresh.sequences) and _same(after.transition_scores, fresh.transition_scores)


# ---- the engine's own surface -----------------------------------------------------------------------------------------------------
def test_engine_split_step_protocol(toy):
    """step_begin / step_finish alone (the two-call form), mixed with step(): the tokens of step() throughout.  The rows
    step_begin reports, the order the calls are held to, and the scheduler's refusal."""
    cfg, weights, ids, mask = toy
    ids, mask = ids.numpy(), mask.numpy()
    ml = ids.shape[1] + 10
    layers, ds = [dict(repetition_penalty=1.1, temperature=0.9, top_k=20)] * 8, [True] * 8
    eng = Engine(cfg, max_batch=4, max_seq_len=256)
    eng.bind_state_dict(weights["bf16"])
    want = eng.generate(ids, mask, ml, layers=layers, do_samples=ds, seed=3)
    eng.begin(ids, mask, ml, layers=layers, do_samples=ds, seed=3)
    lib = eng.lib
    assert lib.mtts_step_sample(eng._h, None, None) == capi.ESTATE and lib.mtts_step_finish(eng._h, None, None) == capi.ESTATE
    done, t = False, 0
    while not done:
        if t % 3 == 2:
            eng.step(1)
        else:
            s0, s17, rows = eng.step_begin()
            assert s0.shape == (3, cfg["vocab_size"]) and s17.shape == (3, 7, cfg["speech_vocab_size"]) and rows.dtype == bool
            if t == 0:
                assert rows.all() and torch.isfinite(s0).sum() > 3 * 150000 and torch.isneginf(s0[:, 152694]).all()
                assert lib.mtts_step(eng._h, 1, None) == capi.ESTATE and b"split step" in lib.mtts_last_error()
                assert lib.mtts_step_begin(eng._h, s0.data_ptr(), s17.data_ptr(), None) == capi.ESTATE
            if t % 3 == 0:
                eng.step_finish()
            else:
                toks = eng.step_sample()
                assert lib.mtts_step_sample(eng._h, toks.data_ptr(), None) == capi.ESTATE
                eng.step_finish(np.zeros(3, dtype=bool))
        t += 1
        steps, done = eng.sync_state()
    gen = eng.read_generated(steps)
    base = ids.shape[1] - 7
    assert np.array_equal(gen.transpose(1, 0, 2), want[:, base:])
    eng.sched_open(2, 16)
    s = torch.zeros(4, dtype=torch.float32, device="cuda")
    assert lib.mtts_step_begin(eng._h, s.data_ptr(), s.data_ptr(), None) == capi.ESTATE and b"scheduler" in lib.mtts_last_error()
    eng.close()
