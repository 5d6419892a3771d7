"""generate(logits_processor=, stopping_criteria=, streamer=) without a GPU: the numpy statement of the materialised score row
against the installed transformers' processors, every refusal before an engine exists, the order of the calls the host loop
makes against a stub engine, and the plan's `split` key."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import modeling_asteroid as ma  # noqa: E402
from mtts import capi, synth  # noqa: E402

import bias_ref as bf  # noqa: E402
import hooks_ref as hr  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the materialised row -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,V", [(4, 1025), (2, 152697)])
def test_materialized_row_is_hf_on_the_bits(rows, V):
    """hooks_ref.materialized equals HF's SequenceBias -> RepetitionPenalty -> NoBadWords -> SuppressTokens on the masked
    logits bit for bit, and the case carries what the kernel test needs: a masked id, banned bits (one in the row's last
    word), a term, a penalised negative and a penalised positive logit, a term that flips a penalised token's sign."""
    pytest.importorskip("transformers")
    logits, hist, banned, tabs = hr.case(rows, V)
    got = hr.materialized(logits, hist, banned, tabs, hr.PENALTY, hr.MASKED[V])
    want = bf.hf_scores(logits, hist, hr.layer(V), hr.MASKED[V])
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), np.asarray(want, dtype=np.float32).view(np.uint32))
    pen = np.float32(hr.PENALTY)
    for r in range(rows):
        assert np.isinf(got[r, [hr.MASKED[V], hr.BANNED, hr.BANNED_PAIR, V - 1]]).all()
        assert got[r, hr.NEG_HIST] == np.float32(-1.25) * pen and got[r, hr.POS_HIST] == np.float32(2.5) / pen
        assert got[r, hr.TERM_FLIP] == np.float32(0.5) / pen                       # (-0.5 + 1.0) / penalty, not -0.5 * penalty + 1.0
        assert got[r, hr.TERM_UP] == np.float32(np.float32(logits[r, hr.TERM_UP] + np.float32(1.75)) + np.float32(0.125))
        free = np.ones(V, dtype=bool)
        free[hist[r]] = False
        free[tabs[r][0]] = False
        free[[hr.MASKED[V]]] = False
        free &= ~banned[r]
        assert np.array_equal(got[r, free], logits[r, free])                        # everything else is the raw logit
    # no penalty, no term, no ban: the mask alone
    bare = hr.materialized(logits, hist, np.zeros_like(banned), [(np.zeros(0, np.int32), np.zeros(0, np.float32))] * rows, 0.0, hr.MASKED[V])
    keep = np.arange(V) != hr.MASKED[V]
    assert np.array_equal(bare[:, keep], logits[:, keep]) and np.isinf(bare[:, hr.MASKED[V]]).all()


# ---- refusals, before an engine exists ----------------------------------------------------------------------------------------
class _NoEngine(ma.AsteroidTTSInstruct):
    def _get_engine(self, *a, **kw):
        raise AssertionError("the engine was asked for")


def _model(cls=_NoEngine, **gen):
    cfg = synth.tiny()
    return cls.from_state_dict(cfg, None, ma.GenerationConfig(eos_token_id=cfg["eos_token_id"], **gen))


def _ids(B=2, T=12):
    return torch.zeros(B, T, 8, dtype=torch.long)


def test_every_refusal_comes_before_the_engine():
    m = _model()
    with pytest.raises(ValueError, match=r"logits_processor\[1\].*not callable"):
        m.generate(_ids(), max_new_tokens=4, logits_processor=[hr.Identity(), "top_h"])
    with pytest.raises(ValueError, match=r"stopping_criteria\[0\].*not callable"):
        m.generate(_ids(), max_new_tokens=4, stopping_criteria=[3.5])
    with pytest.raises(ValueError, match="put.*end"):
        m.generate(_ids(), max_new_tokens=4, streamer=object())

    class HalfStreamer:
        def put(self, v):
            pass

    with pytest.raises(ValueError, match="put.*end"):
        m.generate(_ids(), max_new_tokens=4, streamer=HalfStreamer())
    with pytest.raises(ValueError, match="MAX_ENGINE_BATCH|static batch"):
        m.generate(_ids(B=129), max_new_tokens=4, streamer=hr.Recorder())
    with pytest.raises(ValueError, match="static batch"):
        _model(do_sample=True).generate(_ids(B=65), max_new_tokens=4, num_return_sequences=2, stopping_criteria=[hr.Never()])
    per_channel = _model(do_samples=[True] * 8, layers=[{}] * 8)
    with pytest.raises(ValueError, match="do_samples"):
        per_channel.generate(_ids(), max_new_tokens=4, logits_processor=[hr.Identity()])
    # ... which refuses the processors only: the per-channel branch takes the other two hooks, and so reaches the engine
    with pytest.raises(AssertionError, match="engine was asked for"):
        per_channel.generate(_ids(), max_new_tokens=4, streamer=hr.Recorder())
    # no hook (None or an empty list) is the call it always was
    with pytest.raises(AssertionError, match="engine was asked for"):
        m.generate(_ids(), max_new_tokens=4, logits_processor=[], stopping_criteria=None)


# ---- the host loop against a stub engine --------------------------------------------------------------------------------------
class _StubEngine:
    """Records the calls; its sampler takes the argmax of what the score rows hold, its run ends after `steps` steps."""
    V0, Vs = 40, 10

    def __init__(self, steps, log):
        self.steps, self.log, self.t = steps, log, 0

    def begin(self, ids, mask, max_length, **kw):
        self.B = ids.shape[0] * kw["takes"]
        self.log.append(("begin", kw["takes"], kw["output_scores"], kw["top_logprobs"]))
        self.gen = []

    def step_begin(self, want_rows=True):
        self.log.append(("step_begin", self.t))
        self.s0 = torch.arange(self.V0, dtype=torch.float32).repeat(self.B, 1) + self.t
        self.s17 = torch.arange(self.Vs, dtype=torch.float32).repeat(self.B, 7, 1)
        return self.s0, self.s17, None

    def step_sample(self):
        self.log.append(("step_sample", self.t))
        toks = torch.cat([self.s0.argmax(-1)[:, None], self.s17.argmax(-1)], dim=1)
        self.gen.append(toks.numpy().copy())
        return toks

    def step_finish(self, stop=None):
        self.log.append(("step_finish", self.t, None if stop is None else [bool(v) for v in stop]))
        self.t += 1

    def sync_state(self):
        return self.t, self.t >= self.steps

    def read_generated(self, n):
        return np.stack(self.gen[:n])

    def sched_open(self, *a, **kw):
        self.log.append(("abandon",))


class _Stubbed(ma.AsteroidTTSInstruct):
    def _get_engine(self, *a, **kw):
        return self._stub


class _LoggingProcessor:
    def __init__(self, log):
        self.log = log

    def __call__(self, input_ids, scores):
        self.log.append(("processor", tuple(input_ids.shape), tuple(scores.shape)))
        out = scores.clone()
        out[:, 3] = 1e9                 # a new tensor: the loop copies it back, and the stub's argmax shows that it did
        return out


class _LoggingCriterion:
    def __init__(self, log):
        self.log = log

    def __call__(self, input_ids, scores):
        self.log.append(("criterion", tuple(input_ids.shape), scores))
        return torch.tensor([False, input_ids.shape[1] == 7])


class _LoggingStreamer:
    def __init__(self, log):
        self.log = log

    def put(self, v):
        self.log.append(("put", tuple(v.shape), v.device.type))

    def end(self):
        self.log.append(("end",))


def test_call_order_of_the_host_loop():
    """begin; put(prompt); then per step: step_begin, the processors on channels 0..7 with the [B, cur_len] history of the
    channel, step_sample, put([B]) BEFORE the criteria (reference :161-168), the criteria with scores None, step_finish with
    the OR of the criteria; end() once and last.  The processor's returned tensor reaches the sampler."""
    log = []
    m = _model(_Stubbed)
    m._stub = _StubEngine(3, log)
    B, T = 2, 12
    base = T - 7
    out = m.generate(_ids(B, T), max_new_tokens=8, logits_processor=[_LoggingProcessor(log)], stopping_criteria=[_LoggingCriterion(log)],
                     streamer=_LoggingStreamer(log))
    want = [("begin", 1, False, 0), ("put", (B, T, 8), "cpu")]
    for t in range(3):
        want.append(("step_begin", t))
        want += [("processor", (B, base + t), (B, _StubEngine.V0 if c == 0 else _StubEngine.Vs)) for c in range(8)]
        want += [("step_sample", t), ("put", (B,), "cpu"), ("criterion", (B, base + t + 1), None),
                 ("step_finish", t, [False, base + t + 1 == 7])]
    want.append(("end",))
    assert log == want
    assert tuple(out.shape) == (B, base + 3, 8) and (out[:, base:] == 3).all()
    # a streamer alone: no processor, no criterion, no stop mask
    log.clear()
    m._stub = _StubEngine(2, log)
    m.generate(_ids(B, T), max_new_tokens=8, streamer=_LoggingStreamer(log))
    assert [e[0] for e in log] == ["begin", "put", "step_begin", "step_sample", "put", "step_finish", "step_begin", "step_sample", "put",
                                   "step_finish", "end"]
    assert log[5] == ("step_finish", 0, None)


def test_a_failing_hook_ends_the_run():
    log = []
    m = _model(_Stubbed)
    m._stub = _StubEngine(3, log)

    def bad_shape(input_ids, scores):
        return scores[:, :5]

    with pytest.raises(ValueError, match="logits_processor returned"):
        m.generate(_ids(), max_new_tokens=8, logits_processor=[bad_shape])
    assert log[-1] == ("abandon",) and not any(e[0] == "end" for e in log)


# ---- the C surface and the plan -------------------------------------------------------------------------------------------------
def test_split_step_abi():
    text = open(os.path.join(ROOT, "include", "mtts.h")).read()
    for name in ("mtts_step_begin", "mtts_step_sample", "mtts_step_finish", "mtts_k_scores_materialize"):
        assert re.search(r"int32_t\s+%s\(" % name, text) and name in capi.exported_symbols()


@pytest.mark.skipif(shutil.which("c++") is None, reason="c++ is not on the path")
def test_split_is_a_key_of_the_step_plan(tmp_path):
    """tests/host/split_plan_main.cpp, built with the host compiler under AddressSanitizer and UBSan and run as a child
    process: `split` is part of the plan's equality (so of the key a captured step is found by) and of its text."""
    out = str(tmp_path / "split_plan_main")
    cmd = ["c++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           os.path.join(ROOT, "tests", "host", "split_plan_main.cpp"), "-o", out]
    subprocess.run(cmd, check=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    r = subprocess.run([out, "key"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    assert r.returncode == 0 and r.stdout.splitlines()[-1] == "ok key", r.stdout + r.stderr
