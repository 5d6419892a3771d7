"""typical_p (HF's TypicalLogitsWarper): the rule, its marshalling and its surface.  No GPU.

mtts/warp_spec.py states the rule once; here it is held against the installed transformers' own warper on the rows the GPU
test runs the kernels on (tests/typical_ref.py), and the way a setting travels -- generation_config.json or a generate()
keyword -> channel_settings -> sampler_typical -> float[8] -> the pending one-shot of csrc/runstate.h -- is checked.
"""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from mtts import capi, synth, warp_spec  # noqa: E402
from mtts.engine import sampler_floors, sampler_typical  # noqa: E402
from oracle import asteroid_oracle as ao  # noqa: E402

import floors_ref as fr  # noqa: E402
import typical_ref as tr  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(V, mode) for V in tr.VOCABS for mode in tr.MODES]


# ---- 1. the rule against HF ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V,mode", CASES)
def test_every_case_builds_within_the_draws(V, mode):
    """Each row of each (vocabulary, mode) case is found within typical_ref.DRAWS draws: doubt mass zero at V = 1 025, at
    most DOUBT_CAP at V = 152 697."""
    _, _, want, doubt, draws = tr.case(V, mode)
    assert draws.max() <= tr.DRAWS and want.shape == (tr.ROWS, V)
    assert (doubt == 0.0).all() if V <= fr.SAMP_CAND else (doubt <= tr.DOUBT_CAP).all()
    print(f"{mode} V={V}: draws {draws.tolist()}, doubt {doubt.tolist()}")


@pytest.mark.parametrize("V,mode", CASES)
def test_warp_spec_keeps_what_hf_keeps(V, mode):
    """On boundary-safe rows the float64 restatement and HF's fp32 warpers keep the same tokens, one for one, behind HF's
    own top-k / top-p; the kept tokens keep their scores.  The stage acts: every row loses tokens to typical_p."""
    lc = tr.MODES[mode]
    logits, hist, want, _, _ = tr.case(V, mode)
    hf4 = fr.hf_scores(logits, hist, fr.four(lc), tr.VOCABS[V]["mask_id"])
    got = warp_spec.apply_floors(hf4, lc)
    assert np.array_equal(np.isfinite(got), np.isfinite(want)), (mode, V, int((np.isfinite(got) != np.isfinite(want)).sum()))
    assert np.array_equal(got[np.isfinite(got)], want[np.isfinite(want)])
    if not (fr.full_path(V, lc) and lc.get("top_p")):           # (the oracle's own top-p on the big vocabulary: floors_cpu's note)
        lm = logits.copy()
        lm[:, tr.VOCABS[V]["mask_id"]] = -np.inf
        got = warp_spec.apply_floors(ao.apply_processors(hist, lm, fr.four(lc)), lc)
        assert np.array_equal(np.isfinite(got), np.isfinite(want))
    pre = np.isfinite(tr.hf_scores(logits, hist, lc, tr.VOCABS[V]["mask_id"], upto_typical=True)).sum(-1)
    only = np.isfinite(warp_spec.apply_floors(hf4, {k: v for k, v in lc.items() if k not in ("epsilon_cutoff", "eta_cutoff")})).sum(-1)
    kept = np.isfinite(want).sum(-1)
    assert kept.min() >= 1 and (only < pre).all(), (only, pre)
    print(f"{mode} V={V}: the typical stage keeps {only.tolist()} of {pre.tolist()}, the chain {kept.tolist()}")


@pytest.mark.parametrize("V", list(tr.VOCABS))
def test_window_and_delta_are_ten_times_the_measurement(V):
    """typical_ref.WINDOW / DELTA against HF's fp32 error on the rows in use: at least ten times it, and not a decade more."""
    ds = dc = 0.0
    for mode in tr.MODES:
        a, b = tr.measure(V, mode)
        ds, dc = max(ds, a), max(dc, b)
    print(f"V={V}: max |shift32 - shift64| = {ds:.3e}, max |cum32 - cum64| / typical_p = {dc:.3e}")
    assert 10 * ds <= tr.WINDOW[V] <= 100 * ds and 10 * dc <= tr.DELTA[V] <= 100 * dc


def test_the_mode_can_leave_and_ties_stay_together():
    row = np.array([[np.log(3.9), 0.0, 0.0, 0.0, 0.0, -np.inf]], dtype=np.float32)        # p(mode) just below 0.5
    out = warp_spec.apply_floors(row, dict(typical_p=0.3))
    assert np.array_equal(np.isfinite(out[0]), [False, True, True, True, True, False])
    row = np.array([[np.log(4.1), 0.0, 0.0, 0.0, 0.0, -np.inf]], dtype=np.float32)        # just above: the mode is the typical one
    out = warp_spec.apply_floors(row, dict(typical_p=0.3))
    assert np.array_equal(np.isfinite(out[0]), [True, False, False, False, False, False])
    uni = np.zeros((1, 7), dtype=np.float32)
    assert np.array_equal(warp_spec.apply_floors(uni, dict(typical_p=0.01)), uni)
    # the cutoffs that follow keep the maximum of the surviving interval, not of the row
    row = np.array([[np.log(3.9), 0.0, 0.0, 0.0, 0.0, -np.inf]], dtype=np.float32)
    out = warp_spec.apply_floors(row, dict(typical_p=0.3, epsilon_cutoff=0.9))
    assert np.array_equal(np.isfinite(out[0]), [False, True, True, True, True, False])
    # all banned: nothing to do, nothing raised
    none = np.full((1, 5), -np.inf, dtype=np.float32)
    assert np.array_equal(warp_spec.apply_floors(none, dict(typical_p=0.5)), none)


def test_a_layer_without_typical_p_gives_the_old_output():
    """apply_floors / floor_margin / floors_of for a layer without typical_p (or with 1.0 / None): bit for bit what the
    floors alone give -- restated here as the three stages of the module's docstring."""
    def old(scores, lc):
        mp, eps, eta, rt = warp_spec.floors_of(lc)
        out = np.array(scores, dtype=np.float32)
        for row in out:
            for which, v in enumerate((mp, eps, eta)):
                if v <= 0.0:
                    continue
                kept = np.flatnonzero(np.isfinite(row))
                s = row[kept].astype(np.float64)
                e = np.exp(s - s.max())
                p = e / e.sum()
                H = -(p[p > 0] * np.log(p[p > 0])).sum()
                floor = (v / e.sum(), v, min(v, rt * np.exp(-H)))[which]
                row[kept[(p < floor) & (s < s.max())]] = -np.inf
        return out
    rng = np.random.default_rng(5)
    s = ao.round_bf16(rng.standard_normal((4, 1025)).astype(np.float32) * 2.5)
    s[:, 1024] = -np.inf
    assert warp_spec.FLOOR_KEYS == ("min_p", "epsilon_cutoff", "eta_cutoff")
    for lc in fr.MODES.values():
        want = old(s, lc)
        for extra in ({}, dict(typical_p=1.0), dict(typical_p=None)):
            got = warp_spec.apply_floors(s, dict(lc, **extra))
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
            assert len(warp_spec.floors_of(dict(lc, **extra))) == 4
            assert warp_spec.floor_margin(s[0], dict(lc, **extra)) == warp_spec.floor_margin(s[0], lc)
            assert warp_spec.typical_margin(s[0], dict(lc, **extra), 1e-3, 1e-3) == 0.0
        assert not np.array_equal(warp_spec.apply_floors(s, dict(lc, typical_p=0.5)), want)


def test_typical_of_values_and_ranges():
    assert warp_spec.typical_of({}) == 0.0 and warp_spec.typical_of(None) == 0.0
    assert warp_spec.typical_of(dict(typical_p=None)) == 0.0 and warp_spec.typical_of(dict(typical_p=1.0)) == 0.0
    assert warp_spec.typical_of(dict(typical_p=1)) == 0.0
    assert warp_spec.typical_of(dict(typical_p=0.2, top_k=5)) == float(np.float32(0.2))
    for bad in (0, 0.0, 1.5, -0.1, float("nan"), float("inf"), "0.5", True, False, [0.5]):
        with pytest.raises(ValueError, match="typical_p"):
            warp_spec.typical_of(dict(typical_p=bad), "layers[3]: ")
        with pytest.raises(ValueError, match=r"layers\[3\]"):
            warp_spec.check_typical(bad, "layers[3]: ")


# ---- 2. marshalling -------------------------------------------------------------------------------------------------------
def test_sampler_typical_marshalling():
    assert sampler_typical(None, None) is None
    layers = [dict(top_k=20, typical_p=0.2), dict(typical_p=0.9), dict(typical_p=1.0), dict(top_p=0.9), {}, None,
              dict(typical_p=None), dict(typical_p=0.5)]
    assert sampler_typical(layers, None) is None                        # greedy channels apply none
    assert sampler_typical(layers, [False] * 8) is None
    assert sampler_typical(layers, [False] * 2 + [True] * 5 + [False]) is None
    arr = sampler_typical(layers, [True] * 7 + [False])
    assert isinstance(arr, C.c_float * 8)
    f32 = lambda v: float(np.float32(v))
    assert list(arr) == [f32(0.2), f32(0.9), 0.0, 0.0, 0.0, 0.0, 0.0, 0.0]       # the last one is set, but the channel is greedy
    assert sampler_typical(layers[:2], [True] * 8)[1] == f32(0.9)       # a short list: the rest absent
    with pytest.raises(ValueError, match=r"layers\[2\].*typical_p"):
        sampler_typical([{}, {}, dict(typical_p=1.2)], [True] * 8)
    with pytest.raises(ValueError, match=r"layers\[0\].*typical_p"):
        sampler_typical([dict(typical_p=0)], [False] * 8)               # a bad value is refused on a greedy channel too
    # the floors' table does not know the key, and keeps its layout
    assert sampler_floors(layers, [True] * 8) is None and C.sizeof(capi.MttsSamplerFloors) == 16


def test_generation_config_channel_settings():
    from modeling_asteroid import GenerationConfig
    four = dict(repetition_penalty=1.1, temperature=0.9, top_k=30, top_p=0.9)
    assert GenerationConfig().typical_p == 1.0                          # HF's default
    # typical_p = 1.0 (or None, or absent): the dicts as before
    before = GenerationConfig(do_sample=True, min_p=0.05, **four).channel_settings(8)
    for kw in ({}, dict(typical_p=1.0), dict(typical_p=None)):
        assert GenerationConfig(do_sample=True, min_p=0.05, **four, **kw).channel_settings(8) == before
    assert "typical_p" not in before[0][0] and sampler_typical(*before) is None
    gc = GenerationConfig(do_sample=True, typical_p=0.4, **four)
    layers, ds = gc.channel_settings(8)
    assert ds == [True] * 8 and layers[0] == dict(four, typical_p=0.4) and all(lc == layers[0] for lc in layers)
    assert list(sampler_typical(layers, ds)) == [float(np.float32(0.4))] * 8
    # one call's override, both ways
    assert gc.channel_settings(8, typical_p=0.7)[0][3]["typical_p"] == 0.7
    assert gc.channel_settings(8, typical_p=1.0)[0][3] == four
    assert GenerationConfig(do_sample=True, **four).channel_settings(8, typical_p=0.7)[0][0]["typical_p"] == 0.7
    # greedy: HF builds no warper
    greedy = GenerationConfig(do_sample=False, typical_p=0.4, repetition_penalty=1.2)
    assert greedy.channel_settings(8) == ([dict(repetition_penalty=1.2)] * 8, [False] * 8)
    # the per-channel branch reads layers[i] and ignores the top-level field
    per = GenerationConfig(do_samples=[True] * 4 + [False] * 4, layers=[dict(top_k=5, typical_p=0.3), dict(typical_p=0.6)], typical_p=0.9)
    layers, ds = per.channel_settings(8)
    assert layers[0] == dict(top_k=5, typical_p=0.3) and layers[1] == dict(typical_p=0.6) and layers[2:] == [{}] * 6
    assert list(sampler_typical(layers, ds))[:3] == [float(np.float32(0.3)), float(np.float32(0.6)), 0.0]
    import json
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        with open(os.path.join(d, "generation_config.json"), "w") as f:
            json.dump(dict(do_sample=True, typical_p=0.25), f)
        assert GenerationConfig.from_pretrained(d).channel_settings(8)[0][7] == dict(
            repetition_penalty=None, temperature=None, top_k=None, top_p=None, typical_p=0.25)


# ---- 3. refused, not dropped ------------------------------------------------------------------------------------------------
def test_generate_refuses_before_the_device_is_touched():
    """model.generate on a model that was never moved to a GPU: every ValueError below comes before an engine exists (the
    engine itself would raise RuntimeError here)."""
    from modeling_asteroid import AsteroidTTSInstruct, GenerationConfig
    cfg = synth.tiny()
    ids = torch.zeros(1, 12, 8, dtype=torch.long)
    m = AsteroidTTSInstruct.from_state_dict(cfg, {}, GenerationConfig(do_sample=True, temperature=0.9))
    for bad in (1.5, -0.5, 0, float("nan"), "x", True):
        with pytest.raises(ValueError, match="typical_p"):
            m.generate(ids, max_new_tokens=4, typical_p=bad)
    with pytest.raises(RuntimeError, match="cuda"):                     # a good value gets as far as the engine
        m.generate(ids, max_new_tokens=4, typical_p=0.5)
    m = AsteroidTTSInstruct.from_state_dict(cfg, {}, GenerationConfig(do_sample=True, typical_p=3.0))
    with pytest.raises(ValueError, match="typical_p"):
        m.generate(ids, max_new_tokens=4)
    per = GenerationConfig(do_samples=[True] * 8, layers=[dict(top_k=5)] * 8)
    m = AsteroidTTSInstruct.from_state_dict(cfg, {}, per)
    with pytest.raises(ValueError, match=r"typical_p.*layers\[i\]"):    # the floors' message
        m.generate(ids, max_new_tokens=4, typical_p=0.5)
    per = GenerationConfig(do_samples=[True] * 8, layers=[dict(top_k=5)] * 7 + [dict(typical_p=1.2)])
    m = AsteroidTTSInstruct.from_state_dict(cfg, {}, per)
    with pytest.raises(ValueError, match="channel 7.*typical_p"):
        m.generate(ids, max_new_tokens=4)


# ---- 4. the ABI and the pending state -----------------------------------------------------------------------------------
def test_new_symbols_in_header_library_and_capi():
    hdr = open(os.path.join(ROOT, "include", "mtts.h")).read()
    lib = capi.lib()
    for name in ("mtts_set_sampler_typical", "mtts_k_sample_typical"):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in capi.exported_symbols() and hasattr(lib, name)
    m = re.search(r"typedef struct MttsSamplerFloors \{(.*?)\} MttsSamplerFloors;", hdr, re.S)
    assert re.findall(r"float\s+(\w+);", m.group(1)) == ["min_p", "epsilon_cutoff", "eta_cutoff", "sqrt_eta_cutoff"]
    # the setter validates before it looks at the engine's device: a null engine is refused, not dereferenced
    assert lib.mtts_set_sampler_typical(None, None) == capi.EINVAL


def test_plan_says_typical_only_when_set():
    """csrc/stepplan.h: typical_on keys the plan, and describe() adds the word to the sample: line only when it is on."""
    src = open(os.path.join(ROOT, "moss-ttsd_amd", "csrc", "stepplan.h")).read()
    assert "typical_on == o.typical_on" in src and 'p.typical_on ? " typical" : ""' in src


@pytest.mark.skipif(shutil.which("c++") is None, reason="c++ is not on the path")
def test_pending_typical_is_a_one_shot_on_the_host(tmp_path):
    """tests/host/typical_state_main.cpp runs PendingRun::set_typical / take / take_typical of csrc/runstate.h under
    AddressSanitizer and UBSan as a child process: consumed by one take, failures included; a refused table names the
    channel and leaves nothing pending."""
    out = str(tmp_path / "typical_state_main")
    src = os.path.join(ROOT, "tests", "host", "typical_state_main.cpp")
    subprocess.run(["c++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", src, "-o", out],
                   check=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    r = subprocess.run([out], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    assert r.returncode == 0 and r.stdout.splitlines()[-1:] == ["ok"] and not r.stderr, r.stdout + r.stderr
