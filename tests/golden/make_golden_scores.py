"""Fixtures that pin output_scores (per-token log-probabilities) to the REFERENCE's own `_sample`.

Run in the build container only (needs the reference checkout that make_golden.py imports), after make_golden.py:
    python tests/golden/make_golden_scores.py

The reference's real `CustomMixin._sample` runs with return_dict_in_generate / output_scores
(modeling_asteroid.py:69-80,171-195) through make_golden.real_sample(want_scores=True) on two greedy cases, both with
repetition_penalty 1.3 and temperature 0.8 on all 8 channels:
  ar_scores_bf16  the inputs of ar_rep_penalty      (weights `hi`, seed 404, B=2, prompt 24, audio 0.3, 24 new tokens)
  ar_scores_fp32  the inputs of ar_text_ragged_fp32 (weights `lo`, seed 103, B=3, prompt 24, text only, 40 new tokens)
Stored (data only): out_ids, ref_dec [steps,B,8] (argmax of the reference's processed scores), ref_lp [steps,B,8]
(float64 log-softmax of those scores at ref_dec), the `used` mask and (cfg, wkw, seed, layers).

It then measures, on this CPU, how far the numpy oracle's log-probabilities sit from the reference's on these fixtures
(D_oracle) and on the sampled fixture ar_sampled.npz (D_sampled), and writes them to profiles/scores_parity.json: the
tests take their parity tolerances from that file.
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import make_golden as mg  # noqa: E402  (puts moss-ttsd_amd and the reference on sys.path)
from mtts import synth  # noqa: E402
import scores_ref as sr  # noqa: E402

LAYERS = [dict(repetition_penalty=1.3, temperature=0.8)] * 8
LO = dict(emb_row_sigma=0.6, speech_boost=3.2, eos_boost=3.2)
HI = dict(emb_row_sigma=0.6, speech_boost=4.0, eos_boost=11.0)
CASES = {
    # name -> (weight kwargs, seed, batch, prompt_len, audio_frac, max_new, torch dtype)
    "ar_scores_bf16": (HI, 404, 2, 24, 0.3, 24, torch.bfloat16),
    "ar_scores_fp32": (LO, 103, 3, 24, 0.0, 40, torch.float32),
}


def make_case(name, wkw, seed, batch, prompt_len, audio_frac, max_new, dtype):
    cfg = synth.tiny()
    w = synth.synth_weights(cfg, seed, bf16=(dtype == torch.bfloat16), **wkw)
    model = mg.build_reference(cfg, w, dtype)
    ids, mask = synth.synth_prompts(cfg, seed + 1, batch, prompt_len, audio_frac, True)
    ml = ids.shape[1] + max_new
    out, scores = mg.real_sample(model, torch.from_numpy(ids), torch.from_numpy(mask), ml, LAYERS, None, want_scores=True)
    base = ids.shape[1] - 7
    steps = out.shape[1] - base
    assert len(scores) == steps
    ref_dec = np.zeros((steps, batch, 8), dtype=np.int32)
    ref_lp = np.zeros((steps, batch, 8), dtype=np.float64)
    for s in range(steps):
        for c in range(8):
            sc = scores[s][c].float().numpy()
            for b in range(batch):
                d = int(np.argmax(sc[b]))
                ref_dec[s, b, c] = d
                ref_lp[s, b, c] = sr.log_softmax64(sc[b], d)
    gen = out[:, base:].transpose(1, 0, 2)
    used = sr.used_mask(gen, base, ml, cfg)
    assert np.array_equal(gen[used], ref_dec[used]), "a used slot does not carry the reference's own pick"
    np.savez_compressed(os.path.join(HERE, name + ".npz"), cfg=json.dumps(cfg), wkw=json.dumps(wkw), seed=seed,
                        layers=json.dumps(LAYERS), dtype="bf16" if dtype == torch.bfloat16 else "fp32",
                        input_ids=ids, attention_mask=mask, max_length=ml, out_ids=out, ref_dec=ref_dec, ref_lp=ref_lp,
                        used=used, transformers_version=__import__("transformers").__version__)
    print(f"{name}: steps={steps} used={int(used.sum())} lp range {ref_lp[used].min():.3f} .. {ref_lp[used].max():.3f}")


if __name__ == "__main__":
    torch.manual_seed(0)
    torch.set_num_threads(8)
    for name, args in CASES.items():
        make_case(name, *args)
    import scores_parity_cpu as spc  # noqa: E402
    rec = {"transformers_version": __import__("transformers").__version__, "cases": {}}
    for name in CASES:
        rec["cases"][name] = spc.oracle_vs_reference(HERE, name)
    rec["cases"]["ar_sampled"] = spc.oracle_vs_reference_sampled(HERE)
    path = os.path.join(ROOT, "profiles", "scores_parity.json")
    if os.path.exists(path):                                   # keep the engine's measured maxima (tools/scores_parity.py)
        old = json.load(open(path))
        for k, v in old.get("cases", {}).items():
            if k in rec["cases"] and "engine" in v:
                rec["cases"][k]["engine"] = v["engine"]
    with open(path, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(rec, indent=1))
