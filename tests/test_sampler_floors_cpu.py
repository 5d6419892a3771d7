"""Probability floors (min_p, epsilon_cutoff, eta_cutoff): the rule, its marshalling and its surface.  No GPU.

mtts/warp_spec.py states the rule once; here it is held against the installed transformers' own warpers on the rows the
GPU test runs the kernels on (tests/floors_ref.py), and the way a setting travels -- generation_config.json or a
generate() keyword -> channel_settings -> sampler_floors -> MttsSamplerFloors[8] -- is checked field by field.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from mtts import capi, synth, warp_spec  # noqa: E402
from mtts.engine import sampler_cfgs, sampler_floors  # noqa: E402
from oracle import asteroid_oracle as ao  # noqa: E402

import floors_ref as fr  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. the rule against HF ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", list(fr.MODES))
@pytest.mark.parametrize("V", list(fr.VOCABS))
def test_warp_spec_keeps_what_hf_keeps(V, mode):
    """On boundary-safe rows the float64 restatement and HF's fp32 warpers keep the same tokens, one for one; the kept
    tokens keep their scores.  (The top-k / top-p stage in front is the oracle's on both sides of the floors.)"""
    lc = fr.MODES[mode]
    logits, hist, want = fr.case(V, mode)
    lm = logits.copy()
    lm[:, fr.VOCABS[V]["mask_id"]] = -np.inf
    s4 = ao.apply_processors(hist, lm, fr.four(lc))
    got = warp_spec.apply_floors(s4, lc)
    if not (fr.full_path(V, lc) and lc.get("top_p")):
        # (a nucleus over the whole big vocabulary: its boundary tokens of 1e-6 mass are fp32 noise between torch's cumsum
        # and numpy's, test_sampler_kernel_vs_oracle; the floors are compared behind HF's own top-p below)
        assert np.array_equal(np.isfinite(got), np.isfinite(want)), (mode, V, int((np.isfinite(got) != np.isfinite(want)).sum()))
        assert np.array_equal(got[np.isfinite(got)], want[np.isfinite(want)])
    hf4 = fr.hf_scores(logits, hist, fr.four(lc), fr.VOCABS[V]["mask_id"])
    got = warp_spec.apply_floors(hf4, lc)
    assert np.array_equal(np.isfinite(got), np.isfinite(want))
    kept = np.isfinite(want).sum(-1)
    assert kept.min() >= 1 and (kept < np.isfinite(hf4).sum(-1)).any(), kept      # the floors act: some row loses tokens to one
    print(f"{mode} V={V}: kept {kept.tolist()}")


def test_floors_of_values_and_ranges():
    assert warp_spec.floors_of({}) == (0.0, 0.0, 0.0, 0.0) and warp_spec.floors_of(None) == (0.0, 0.0, 0.0, 0.0)
    mp, eps, eta, rt = warp_spec.floors_of(dict(min_p=0.05, epsilon_cutoff=3e-4, eta_cutoff=2e-3, top_k=5))
    assert (mp, eps, eta) == tuple(float(np.float32(v)) for v in (0.05, 3e-4, 2e-3))
    assert rt == float(torch.sqrt(torch.tensor(2e-3)))                  # HF: torch.sqrt of the fp32 scalar
    assert warp_spec.floors_of(dict(min_p=1, epsilon_cutoff=None, eta_cutoff=0))[:3] == (1.0, 0.0, 0.0)
    for bad in (dict(min_p=1.5), dict(min_p=-0.1), dict(epsilon_cutoff=1.0), dict(eta_cutoff=1), dict(eta_cutoff=-1e-3),
                dict(min_p=float("nan")), dict(min_p="0.1"), dict(epsilon_cutoff=True)):
        with pytest.raises(ValueError, match=list(bad)[0]):
            warp_spec.floors_of(bad, "layers[3]: ")


def test_a_token_at_the_maximum_never_leaves():
    row = np.array([[0.0, 0.0, -1.0, -30.0, -np.inf]], dtype=np.float32)
    out = warp_spec.apply_floors(row, dict(min_p=1.0))
    assert np.array_equal(np.isfinite(out[0]), [True, True, False, False, False])
    out = warp_spec.apply_floors(row, dict(epsilon_cutoff=0.9))         # every p is below 0.9: the two maxima stay
    assert np.array_equal(np.isfinite(out[0]), [True, True, False, False, False])
    assert np.array_equal(warp_spec.apply_floors(row, {}), row)


# ---- 2. marshalling -------------------------------------------------------------------------------------------------------
def test_sampler_floors_marshalling():
    assert sampler_floors(None, None) is None
    layers = [dict(top_k=20, min_p=0.05), dict(epsilon_cutoff=3e-4), dict(eta_cutoff=2e-3), dict(top_p=0.9), {}, None,
              dict(min_p=0.0), dict(min_p=0.3, eta_cutoff=0.01)]
    assert sampler_floors(layers, None) is None                         # greedy channels apply no floor
    assert sampler_floors(layers, [False] * 8) is None
    assert sampler_floors([dict(top_k=5)] * 8, [True] * 8) is None      # no sampled channel sets one
    assert sampler_floors(layers, [False] * 3 + [True] * 4 + [False]) is None
    arr = sampler_floors(layers, [True] * 7 + [False])
    assert isinstance(arr, capi.MttsSamplerFloors * 8) and C.sizeof(capi.MttsSamplerFloors) == 16
    f32 = lambda v: float(np.float32(v))
    got = [(a.min_p, a.epsilon_cutoff, a.eta_cutoff, a.sqrt_eta_cutoff) for a in arr]
    assert got[0] == (f32(0.05), 0.0, 0.0, 0.0)
    assert got[1] == (0.0, f32(3e-4), 0.0, 0.0)
    assert got[2] == (0.0, 0.0, f32(2e-3), float(np.sqrt(np.float32(2e-3))))
    assert got[3] == got[4] == got[5] == got[6] == (0.0, 0.0, 0.0, 0.0)
    assert got[7] == (0.0, 0.0, 0.0, 0.0)                               # set, but the channel is greedy
    assert sampler_floors(layers[:2], [True] * 8)[1].epsilon_cutoff == f32(3e-4)      # a short list: the rest absent
    with pytest.raises(ValueError, match=r"layers\[2\].*eta_cutoff"):
        sampler_floors([{}, {}, dict(eta_cutoff=1.0)], [True] * 8)
    with pytest.raises(ValueError, match=r"layers\[0\].*min_p"):
        sampler_floors([dict(min_p=2)], [False] * 8)                    # a bad value is refused on a greedy channel too
    # the four fields of MttsSamplerCfg do not move
    cfg = sampler_cfgs(layers, [True] * 8)
    assert cfg[0].top_k == 20 and C.sizeof(capi.MttsSamplerCfg) == 24


def test_generation_config_channel_settings():
    from modeling_asteroid import GenerationConfig
    gc = GenerationConfig(do_sample=True, temperature=0.9, top_k=30, top_p=0.9, repetition_penalty=1.1, min_p=0.05,
                          epsilon_cutoff=3e-4, eta_cutoff=2e-3)
    layers, ds = gc.channel_settings(8)
    assert ds == [True] * 8 and len(layers) == 8
    assert layers[0] == dict(repetition_penalty=1.1, temperature=0.9, top_k=30, top_p=0.9, min_p=0.05, epsilon_cutoff=3e-4,
                             eta_cutoff=2e-3)
    assert all(lc == layers[0] for lc in layers)
    assert sampler_floors(layers, ds)[5].min_p == float(np.float32(0.05))
    # HF's activation conditions (GenerationMixin._get_logits_processor): min_p is not None; 0 < cutoff < 1
    plain = GenerationConfig(do_sample=True, temperature=0.9)
    assert (plain.min_p, plain.epsilon_cutoff, plain.eta_cutoff) == (None, 0.0, 0.0)
    assert not set(plain.channel_settings(8)[0][0]) & set(warp_spec.FLOOR_KEYS)
    assert sampler_floors(*plain.channel_settings(8)) is None
    edge = GenerationConfig(do_sample=True, min_p=0.0, epsilon_cutoff=1.0, eta_cutoff=0.0)
    assert {k: v for k, v in edge.channel_settings(8)[0][0].items() if k in warp_spec.FLOOR_KEYS} == dict(min_p=0.0)
    assert sampler_floors(*edge.channel_settings(8)) is None            # min_p = 0 removes nothing
    # one call's overrides
    layers, _ = gc.channel_settings(8, min_p=0.2, eta_cutoff=None)
    assert layers[3]["min_p"] == 0.2 and layers[3]["eta_cutoff"] == 2e-3
    assert GenerationConfig(do_sample=True).channel_settings(8, epsilon_cutoff=0.01)[0][0]["epsilon_cutoff"] == 0.01
    # greedy: HF builds no warper
    greedy = GenerationConfig(do_sample=False, min_p=0.05, repetition_penalty=1.2)
    assert greedy.channel_settings(8) == ([dict(repetition_penalty=1.2)] * 8, [False] * 8)
    # the per-channel branch reads layers[i] and ignores the top-level fields, as the reference's ignores every top-level warper
    per = GenerationConfig(do_samples=[True] * 4 + [False] * 4, layers=[dict(top_k=5, min_p=0.1), dict(eta_cutoff=0.02)],
                           min_p=0.7, epsilon_cutoff=0.5)
    layers, ds = per.channel_settings(8)
    assert layers[0] == dict(top_k=5, min_p=0.1) and layers[1] == dict(eta_cutoff=0.02) and layers[2:] == [{}] * 6
    arr = sampler_floors(layers, ds)
    assert arr[0].min_p == float(np.float32(0.1)) and arr[0].epsilon_cutoff == 0.0 and arr[2].min_p == 0.0
    import json
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        with open(os.path.join(d, "generation_config.json"), "w") as f:
            json.dump(dict(do_sample=True, min_p=0.08, eta_cutoff=0.003), f)
        assert GenerationConfig.from_pretrained(d).channel_settings(8)[0][7] == dict(
            repetition_penalty=None, temperature=None, top_k=None, top_p=None, min_p=0.08, eta_cutoff=0.003)


# ---- 3. refused, not dropped ------------------------------------------------------------------------------------------------
def test_generate_refuses_before_the_device_is_touched():
    """model.generate on a model that was never moved to a GPU: every ValueError below comes before an engine exists (the
    engine itself would raise RuntimeError here)."""
    from modeling_asteroid import AsteroidTTSInstruct, GenerationConfig
    cfg = synth.tiny()
    ids = torch.zeros(1, 12, 8, dtype=torch.long)
    m = AsteroidTTSInstruct.from_state_dict(cfg, {}, GenerationConfig(do_sample=True, temperature=0.9))
    for kw, word in ((dict(min_p=1.5), "min_p"), (dict(min_p=-0.5), "min_p"), (dict(epsilon_cutoff=1.0), "epsilon_cutoff"),
                     (dict(eta_cutoff=7), "eta_cutoff"), (dict(eta_cutoff="x"), "eta_cutoff")):
        with pytest.raises(ValueError, match=word):
            m.generate(ids, max_new_tokens=4, **kw)
    with pytest.raises(RuntimeError, match="cuda"):                     # a good value gets as far as the engine
        m.generate(ids, max_new_tokens=4, min_p=0.1)
    m = AsteroidTTSInstruct.from_state_dict(cfg, {}, GenerationConfig(do_sample=True, min_p=3.0))
    with pytest.raises(ValueError, match="min_p"):                      # HF's MinPLogitsWarper refuses it too
        m.generate(ids, max_new_tokens=4)
    per = GenerationConfig(do_samples=[True] * 8, layers=[dict(top_k=5)] * 8)
    m = AsteroidTTSInstruct.from_state_dict(cfg, {}, per)
    with pytest.raises(ValueError, match=r"layers\[i\]"):
        m.generate(ids, max_new_tokens=4, min_p=0.1)
    per = GenerationConfig(do_samples=[True] * 8, layers=[dict(top_k=5)] * 7 + [dict(epsilon_cutoff=1.2)])
    m = AsteroidTTSInstruct.from_state_dict(cfg, {}, per)
    with pytest.raises(ValueError, match="channel 7.*epsilon_cutoff"):
        m.generate(ids, max_new_tokens=4)


# ---- 4. the ABI ---------------------------------------------------------------------------------------------------------------
def test_new_symbols_in_header_library_and_capi():
    hdr = open(os.path.join(ROOT, "include", "mtts.h")).read()
    lib = capi.lib()
    for name in ("mtts_set_sampler_floors", "mtts_k_sample_floors"):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in capi.exported_symbols() and hasattr(lib, name)
    m = re.search(r"typedef struct MttsSamplerFloors \{(.*?)\} MttsSamplerFloors;", hdr, re.S)
    fields = re.findall(r"float\s+(\w+);", m.group(1))
    assert fields == [f for f, _ in capi.MttsSamplerFloors._fields_] == ["min_p", "epsilon_cutoff", "eta_cutoff", "sqrt_eta_cutoff"]
    # the setter validates before it looks at the engine's device: a null engine is refused, not dereferenced
    assert lib.mtts_set_sampler_floors(None, None) == capi.EINVAL
