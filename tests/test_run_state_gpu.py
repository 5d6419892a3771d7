"""The two rules of csrc/runstate.h through the engine.  A captured decode step is found by its plan, its KV page bound and
the addresses it holds (StepBufs): a run that reallocated one of them captures its step again, an unchanged run replays,
and nothing computes differently from the engine that launches every step on the stream.  And the one-shot options of
the next run are consumed by the call that starts it, failures included.  tests/test_run_state_cpu.py pins the same
types on the host.  -m gpu."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from mtts import capi, synth  # noqa: E402
from mtts.engine import rope_tables, sampler_cfgs  # noqa: E402
from test_step_plan_gpu import CONFIGS, SWITCHES, _counters, _prompts, _rand_weights  # noqa: E402

SAMPLED = ([dict(top_k=40, top_p=0.9, temperature=1.1, repetition_penalty=1.2)] * 8, [True] * 8)
B, T, STEPS = 2, 20, 8


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype.itemsize == 4 else np.uint64)


def _run(eng, ids, mask, seed, max_new=STEPS + 20, scores=False, topk=0, row_adapters=None):
    """One short sampled run of STEPS steps, then abandoned and ended -> (what it produced, as bit patterns; whether a
    counted kernel was launched while its steps were issued -- with graphs that is a capture, a launch counts once)."""
    eng.begin(ids, mask, T + max_new, layers=SAMPLED[0], do_samples=SAMPLED[1], seed=seed, output_scores=scores, top_logprobs=topk,
              row_adapters=row_adapters)
    c0 = _counters()
    eng.step(STEPS)
    steps, _ = eng.sync_state()
    c1 = _counters()
    assert steps == STEPS
    out = [_bits(eng.read_generated(STEPS))]
    if scores:
        out.append(_bits(eng.read_scores(STEPS)))
    if topk:
        out += [_bits(a) for a in eng.read_top_logprobs(STEPS)]
    eng.sched_open(B, 8, output_scores=scores, top_logprobs=topk)          # ends the abandoned run; 8 steps of storage grow nothing
    return out, c1 != c0


def test_reallocated_buffers_are_never_replayed(monkeypatch):
    """One engine with MTTS_GRAPHS=1 and one with MTTS_GRAPHS=0 get the same sequence of short sampled runs at B = 2, each
    of which changes one thing a captured step holds: the output_scores buffer and its scratch appear; the top_logprobs
    buffers appear at k = 2 and change their stride (and grow their scratch) at k = 5; a longer max_length reallocates
    every per-slot store at the SAME plan as the run before it; mtts_bind_rope replaces the tables under an unchanged plain
    run; the first mtts_adapter_load widens the split-K slabs and brings the bank.  Tokens, scores and top-logprob
    arrays are bitwise equal between the engines, run by run.  The launch counters of test_step_plan_gpu (a launch inside
    a capture counts once) move over the steps of every run that reallocated something or has a new plan, and do not
    move over a run repeated unchanged -- a plain one and one with an adapter.
    The tiny config launches none of the counted kernels, and neither does the small-batch path that two dialogues take:
    the two-layer bench-width config of test_step_plan_gpu with MTTS_SMALL_ROWS=0 (o_proj, gate/up, down_proj and the
    heads are then counted launches of every step)."""
    from mtts.engine import Engine
    cfg = CONFIGS["bench_width"][0]()
    H, D = cfg["hidden_size"], cfg["head_dim"]
    ids, mask = _prompts(cfg, B, T, 3)
    rng = np.random.default_rng(8)
    name = "model.language_model.layers.1.self_attn.q_proj.weight"
    adapter = {name: ((rng.standard_normal((4, H)) * 0.3).astype(np.float32),
                      (rng.standard_normal((cfg["num_attention_heads"] * D, 4)) * 0.3).astype(np.float32))}
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("MTTS_SMALL_ROWS", "0")
    res = {}
    for graphs in ("1", "0"):
        monkeypatch.setenv("MTTS_GRAPHS", graphs)
        eng = Engine(cfg, max_batch=B, max_seq_len=512)
        for n, t in _rand_weights(cfg, 5):
            eng.bind(n, t)
        capi.check(eng.lib.mtts_weights_ready(eng._h))
        runs = {}
        runs["plain"] = _run(eng, ids, mask, 1)
        runs["scores"] = _run(eng, ids, mask, 2, scores=True)
        runs["top2"] = _run(eng, ids, mask, 3, topk=2)
        runs["top5"] = _run(eng, ids, mask, 4, topk=5)
        runs["top5_longer"] = _run(eng, ids, mask, 4, topk=5, max_new=STEPS + 300)        # the plan of top5; every store moves
        runs["plain_again"] = _run(eng, ids, mask, 1)
        cos, sin = rope_tables(D, float(cfg["rope_theta"]), 512 + 24 + 64, eng.device)      # 64 rows more, the same values below
        capi.check(eng.lib.mtts_bind_rope(eng._h, cos.data_ptr(), sin.data_ptr(), cos.shape[0], None))
        torch.cuda.synchronize()
        runs["plain_new_rope"] = _run(eng, ids, mask, 1)                                    # the plan of plain_again
        runs["plain_repeat"] = _run(eng, ids, mask, 1)
        eng.load_bank_adapter(0, adapter, 1.5)
        runs["adapter"] = _run(eng, ids, mask, 1, row_adapters=[0, -1])
        runs["plain_with_bank"] = _run(eng, ids, mask, 1)                                   # the plan of plain_repeat; wider slabs
        runs["adapter_repeat"] = _run(eng, ids, mask, 1, row_adapters=[0, -1])
        assert eng.close() == 0
        res[graphs] = runs
    for name, (out, _) in res["1"].items():
        ref = res["0"][name][0]
        assert len(out) == len(ref) and all(np.array_equal(a, b) for a, b in zip(out, ref)), name
    moved = {name: m for name, (_, m) in res["1"].items()}
    print(moved)
    assert all(m for _, m in res["0"].values())            # on the stream every step launches them
    assert moved == dict(plain=True, scores=True, top2=True, top5=True, top5_longer=True, plain_again=True, plain_new_rope=True,
                         plain_repeat=False, adapter=True, plain_with_bank=True, adapter_repeat=False)
    # the same run gives the same tokens whatever was reallocated under it, and the runs are not trivially equal
    g = {name: out[0] for name, (out, _) in res["1"].items()}
    assert np.array_equal(g["plain"], g["plain_again"]) and np.array_equal(g["plain"], g["plain_new_rope"])
    assert np.array_equal(g["plain"], g["plain_repeat"]) and np.array_equal(g["plain"], g["plain_with_bank"])
    assert np.array_equal(g["top5"], g["top5_longer"]) and np.array_equal(g["adapter"], g["adapter_repeat"])
    assert not np.array_equal(g["plain"], g["scores"]) and not np.array_equal(g["top2"], g["top5"])
    assert not np.array_equal(g["adapter"][:, 0], g["plain"][:, 0])          # (the plain run's seed: row 0 has the adapter)


def test_row_ids_are_consumed_by_a_failed_begin():
    """include/mtts.h: the ids of mtts_set_row_ids are consumed by the next mtts_begin.  A begin that fails (T = 4 < 8,
    MTTS_EINVAL) has consumed them: the valid sampled run that follows without ids draws what a fresh engine draws with the
    default ids, not what a run given those ids draws."""
    from mtts.engine import Engine
    cfg = synth.tiny()
    w = synth.synth_weights(cfg, 31, emb_row_sigma=0.6, speech_boost=5.0)
    ids, mask = _prompts(cfg, B, T, 6)
    other = np.array([5, 9], dtype=np.int32)

    def sampled(eng, row_ids):
        eng.begin(ids, mask, T + STEPS + 20, layers=SAMPLED[0], do_samples=SAMPLED[1], seed=11, row_ids=row_ids)
        eng.step(STEPS)
        assert eng.sync_state()[0] == STEPS
        return eng.read_generated(STEPS)

    eng = Engine(cfg, max_batch=B, max_seq_len=128)
    eng.bind_state_dict(w)
    capi.check(eng.lib.mtts_set_row_ids(eng._h, other.ctypes.data, B))
    short = np.ascontiguousarray(ids[:, :4])
    m4 = np.ones((B, 4), dtype=np.uint8)
    rc = eng.lib.mtts_begin(eng._h, short.ctypes.data, m4.ctypes.data, B, 4, 40, sampler_cfgs(*SAMPLED), C.c_uint64(11), None)
    assert rc == capi.EINVAL and b"T must be >= 8" in eng.lib.mtts_last_error()
    after_failure = sampled(eng, None)
    eng.close()
    fresh = Engine(cfg, max_batch=B, max_seq_len=128)
    fresh.bind_state_dict(w)
    default = sampled(fresh, None)
    fresh.sched_open(B, 8)                                  # ends the abandoned run
    with_ids = sampled(fresh, other)
    fresh.close()
    assert not np.array_equal(default, with_ids)
    assert np.array_equal(after_failure, default)
