"""output_scores (per-token log-probabilities) without a GPU.

* The fixtures tests/golden/ar_scores_{bf16,fp32}.npz hold the log-probabilities of the REFERENCE's own `_sample`
  (return_dict_in_generate / output_scores) on two greedy runs; ar_sampled.npz holds the reference's kept sets of a
  sampled run.  The numpy oracle must reproduce them; how closely it does on the machine that made the fixtures is
  recorded in profiles/scores_parity.json (D_oracle, D_sampled), and the GPU tests take their parity tolerance from
  that file (test_scores_gpu.py).
* The drop-in's argument handling happens before anything touches the device.
"""
import json
import os

import numpy as np
import pytest
import torch

from mtts import capi, synth

import scores_parity_cpu as spc
import scores_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _parity():
    with open(os.path.join(ROOT, "profiles", "scores_parity.json")) as f:
        return json.load(f)["cases"]


@pytest.mark.parametrize("name", ["ar_scores_bf16", "ar_scores_fp32"])
def test_fixture_used_mask_is_the_state_machines_rule(golden_dir, name):
    """`used` in the fixture = the structural rule restated in scores_ref.used_mask, and at every used slot the token the
    reference appended is its own pick (the argmax of the scores it returned)."""
    z = np.load(os.path.join(golden_dir, name + ".npz"))
    cfg = json.loads(str(z["cfg"]))
    base = z["input_ids"].shape[1] - 7
    gen = z["out_ids"][:, base:].transpose(1, 0, 2)
    used = sr.used_mask(gen, base, int(z["max_length"]), cfg)
    assert np.array_equal(used, z["used"])
    assert np.array_equal(gen[used], z["ref_dec"][used])
    assert not used[0, :, 1:].any() and used[0, :, 0].all()          # step 0: channels 1..7 are teacher-forced
    assert np.isfinite(z["ref_lp"][used]).all() and (z["ref_lp"][used] <= 0).all()


@pytest.mark.parametrize("name", ["ar_scores_bf16", "ar_scores_fp32"])
def test_oracle_reproduces_reference_log_probabilities(golden_dir, name):
    """Teacher-forced on the reference's ids, the oracle's lp at every used slot where its decision equals the
    reference's.  D_oracle (recorded when the fixture was made) is what one implementation with a summation order of
    its own deviates by; a second machine's BLAS is another such implementation, so the re-measured figure must stay
    within 2 x D_oracle + the 2e-5 arithmetic budget -- the bound the engine is held to."""
    rec = _parity()[name]
    got = spc.oracle_vs_reference(golden_dir, name)
    print(name, "recorded", rec, "measured", got)
    assert got["used"] == rec["used"] > 200
    assert got["used"] - got["compared"] <= 0.01 * got["used"]
    assert got["D_oracle"] <= 2 * rec["D_oracle"] + sr.KERNEL_TOL
    if name.endswith("fp32"):
        assert rec["D_oracle"] < 1e-4                                 # fp32: the structure is right, not merely close


def test_oracle_reproduces_reference_sampled_log_probabilities(golden_dir):
    rec = _parity()["ar_sampled"]
    got = spc.oracle_vs_reference_sampled(golden_dir, seed=rec["seed"])
    print("ar_sampled recorded", rec, "measured", got)
    assert got["used"] == rec["used"] > 200
    assert got["compared"] >= 0.97 * got["used"]
    assert got["D_sampled"] <= 2 * rec["D_sampled"] + sr.KERNEL_TOL


@pytest.mark.parametrize("dtype", ["bf16", "fp32", "fp16"])
def test_sampled_scenario_moves_no_boundary_on_the_host(dtype):
    """The sampled engine run of test_scores_gpu.py::test_engine_lp_vs_its_own_logits grants 1 slot in 240 for a top-k /
    top-p boundary token that moves.  Its inputs (weights, prompts, Philox seed: scores_ref.SCENARIO) are chosen so that
    the host side alone moves none: on the numpy oracle's logits of the same run, at every used slot, the kept set that
    apply_processors forms with fp32 sums equals the one formed with float64 sums.  (Scores that tie with the k-th are
    kept by HF's rule on every side: bf16 logits tie often, and a tie moves nothing.  The engine's logits are not the
    oracle's to the last bit; what can be checked without a GPU is checked.)"""
    from oracle import asteroid_oracle as ao
    sc = sr.SCENARIO
    cfg = synth.tiny()
    w = synth.synth_weights(cfg, sc["weight_seed"], bf16=(dtype == "bf16"), **sc["wkw"])
    ids, mask = synth.synth_prompts(cfg, sc["prompt_seed"], sc["batch"], sc["prompt_len"], sc["audio_frac"], True)
    layers, ds = sr.SCENARIO_SAMPLED
    ml = ids.shape[1] + sc["new"]
    base = ids.shape[1] - 7
    out, logs = ao.AsteroidOracle(cfg, w, dtype).generate(ids, mask, ml, layers=layers, do_samples=ds, seed=sc["seed"],
                                                         return_logits=True)
    gen = out[:, base:].transpose(1, 0, 2)
    used = sr.used_mask(gen, base, ml, cfg)
    assert gen.shape[0] >= 40 and used.sum() > 400
    n = 0
    for g, r, c in zip(*np.nonzero(used)):
        lc = layers[c]
        pre = {k: v for k, v in lc.items() if k in ("repetition_penalty", "temperature")}
        hist = out[r, :base + g, c][None]
        row = logs[g][c][r][None]                                    # (the oracle's logits carry the step's masks already)
        s = ao.apply_processors(hist, row, pre)[0]
        kept32 = np.nonzero(np.isfinite(ao.apply_processors(hist, row, lc)[0]))[0]
        assert np.array_equal(kept32, sr.kept_set_f64(s, lc)), (g, r, c)
        n += 1
    assert n == used.sum()


def test_boundary_safe_detects_knife_edges():
    s = np.log(np.array([0.05, 0.05, 0.2, 0.7], dtype=np.float64)).astype(np.float32)
    assert not sr.boundary_safe(s, dict(top_p=0.9))                   # cumulative 0.1 == 1 - top_p
    assert sr.boundary_safe(s, dict(top_p=0.8))
    assert not sr.boundary_safe(np.array([1.0, 2.0, 2.0, 3.0], dtype=np.float32), dict(top_k=2))
    assert sr.boundary_safe(np.array([1.0, 2.0, 2.5, 3.0], dtype=np.float32), dict(top_k=2))


def test_log_softmax64_ignores_filtered_tokens():
    s = np.array([0.0, -np.inf, np.log(3.0)], dtype=np.float32)
    assert abs(sr.log_softmax64(s, 2) - np.log(0.75)) < 1e-7
    assert abs(sr.log_softmax64(s, 0) - np.log(0.25)) < 1e-7


# ---- drop-in surface ------------------------------------------------------------------------------------------------
def _model(**gen):
    from modeling_asteroid import AsteroidTTSInstruct, GenerationConfig
    cfg = synth.tiny()
    return AsteroidTTSInstruct.from_state_dict(cfg, {}, GenerationConfig(eos_token_id=cfg["eos_token_id"], **gen))


def _inputs():
    ids, mask = synth.synth_prompts(synth.tiny(), 1, 2, 24, 0.3, False)
    return torch.from_numpy(ids), torch.from_numpy(mask)


@pytest.mark.parametrize("kw", ["output_logits", "output_attentions", "output_hidden_states"])
def test_unsupported_outputs_raise_instead_of_being_dropped(kw):
    ids, mask = _inputs()
    with pytest.raises(ValueError, match=kw):
        _model().generate(ids, mask, max_new_tokens=8, return_dict_in_generate=True, **{kw: True})


def test_scores_keywords_pass_the_checks():
    """return_dict_in_generate / output_scores are accepted and the call goes on to the device (absent here)."""
    ids, mask = _inputs()
    with pytest.raises(RuntimeError, match="cuda"):
        _model().generate(ids, mask, max_new_tokens=8, return_dict_in_generate=True, output_scores=True)


def test_generate_output_object():
    from modeling_asteroid import GenerateOutput
    seq = torch.zeros(2, 5, 8, dtype=torch.long)
    lp = torch.full((2, 3, 8), float("nan"))
    lp[0, 0, 0], lp[0, 1, 1], lp[1, 2, 7] = -0.5, -1.25, -2.0
    out = GenerateOutput(seq, lp)
    assert out.sequences is seq and out.scores is None and out["sequences"] is seq
    assert out.transition_scores.dtype == torch.float32
    assert torch.equal(out.sequences_scores, torch.tensor([-1.75, -2.0]))
    bare = GenerateOutput(seq)
    assert bare.transition_scores is None and bare.sequences_scores is None and bare.scores is None


def test_scores_entry_points_exported_and_bound():
    lib = capi.lib()
    for name in ("mtts_set_output_scores", "mtts_read_scores", "mtts_slot_read_scores", "mtts_k_sample_scores"):
        assert name in capi.exported_symbols()
        assert getattr(lib, name).argtypes is not None
    assert lib.mtts_version() >= 202
    assert lib.mtts_set_output_scores(None, 1) == -1             # null engine: MTTS_EINVAL, no device touched
    assert lib.mtts_read_scores(None, None, 0, None) == capi.ESTATE
    assert lib.mtts_slot_read_scores(None, 0, None, 0, None) == -1


def test_scheduler_scores_switch_comes_after_argument_checks():
    from mtts.scheduler import ContinuousBatcher
    cb = ContinuousBatcher.__new__(ContinuousBatcher)
    with pytest.raises(ValueError):
        cb.run([np.zeros((9, 8), dtype=np.int64)], 4, takes=0, output_scores=True)
