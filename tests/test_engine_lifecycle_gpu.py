"""Lifetime of the engine's device memory (csrc/engine.h: DevBufs).  -m gpu.

One engine per dtype walks every path that reallocates a buffer -- RoPE tables, generated-token storage, the scores
buffer and its scratch, prefill staging -- and is then destroyed.  mtts_engine_destroy reports a free that failed, so a
double or stale free in the owner shows up here as an error code.  Nothing is provoked: only legitimate calls."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from mtts import capi, synth  # noqa: E402

SAMPLED = ([dict(top_k=40, top_p=0.9, temperature=1.1, repetition_penalty=1.2)] * 8, [True] * 8)


@pytest.fixture(scope="module")
def model():
    cfg = synth.tiny()
    return cfg, synth.synth_weights(cfg, 311, emb_row_sigma=0.6, speech_boost=6.0, eos_boost=1.0)


def _prompt(cfg, n, seed):
    """One delay-shifted prompt of n real tokens (half text, half audio), int64 [n + 7, 8]."""
    rng = np.random.default_rng(seed)
    raw = np.full((n, 8), 1024, dtype=np.int64)
    na = n // 2
    raw[:n - na, 0] = rng.integers(0, 151643, n - na)
    raw[n - na:, 0] = 151665 + rng.integers(0, 1024, na)
    raw[n - na:, 1:] = rng.integers(0, 1024, (na, 7))
    return synth.shifting_inputs(raw, cfg["pad_token_id"])


def _engine(cfg, w, dtype):
    from mtts.engine import Engine
    eng = Engine(cfg, max_batch=4, max_seq_len=512, dtype=dtype)
    eng.bind_state_dict(w)
    return eng


def _first_generate(eng, ids, mask):
    return eng.generate(ids, mask, ids.shape[1] + 6, *SAMPLED, seed=5, takes=2, output_scores=True)


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_reallocating_paths_then_destroy(model, dtype):
    from mtts.engine import rope_tables
    cfg, w = model
    ids, mask = synth.left_pad([_prompt(cfg, 40, 1), _prompt(cfg, 70, 2)], cfg["pad_token_id"])
    T = ids.shape[1]
    eng = _engine(cfg, w, dtype)                       # (its constructor bound a RoPE table of 536 rows)
    for rows in (300, 600):                            # RoPE tables: a smaller pair, then a larger one
        cos, sin = (t.to(eng.tdtype) for t in rope_tables(cfg["head_dim"], float(cfg["rope_theta"]), rows, eng.device, eng.model_dtype))
        torch.cuda.synchronize(eng.device)
        capi.check(eng.lib.mtts_bind_rope(eng._h, cos.data_ptr(), sin.data_ptr(), rows, None))
        torch.cuda.synchronize(eng.device)
    # scores buffer and scratch appear with the first run that asks for them; 2 takes per prompt
    out1, lp1 = _first_generate(eng, ids, mask)
    assert out1.shape[0] == 4 and lp1.shape[:2] == (4, out1.shape[1] - (T - 7))
    # a longer run: generated-token storage and the scores buffer regrow
    out2, lp2 = eng.generate(ids, mask, T + 60, *SAMPLED, seed=5, takes=2, output_scores=True)
    assert out2.shape[1] >= out1.shape[1] and lp2.shape[1] == out2.shape[1] - (T - 7)
    # scheduler run; one prompt longer than the static runs' prefill staging (2 prompts -> 256 rows)
    eng.sched_open(2, 64, *SAMPLED, output_scores=True)
    long_prompt = _prompt(cfg, 300, 3)
    eng.submit(0, long_prompt, long_prompt.shape[0] + 24, seed=7)
    eng.step(4)
    assert eng.slot_states()[0, 2] == 4
    assert eng.slot_read(0, 64).shape == (4, 8) and eng.slot_read_scores(0, 64).shape == (4, 8)
    assert eng.close() == 0, capi.lib().mtts_last_error().decode()             # MTTS_OK: every free succeeded
    # a second engine in the same process; the walked engine's first run equals the same call on this fresh one
    fresh = _engine(cfg, w, dtype)
    out_f, lp_f = _first_generate(fresh, ids, mask)
    assert np.array_equal(out1, out_f)
    assert np.array_equal(lp1, lp_f, equal_nan=True)
    assert fresh.close() == 0, capi.lib().mtts_last_error().decode()
