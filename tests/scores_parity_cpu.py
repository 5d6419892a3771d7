"""How far the numpy oracle's per-token log-probabilities sit from the reference's, on the output_scores fixtures.
Used by golden/make_golden_scores.py (which records the figures in profiles/scores_parity.json) and by
test_scores_cpu.py (which re-measures them).  numpy only; no reference import."""
import json
import os

import numpy as np

from mtts import synth
from oracle import asteroid_oracle as ao

import scores_ref as sr


def load(golden_dir, name):
    z = np.load(os.path.join(golden_dir, name + ".npz"))
    cfg = json.loads(str(z["cfg"]))
    dtype = str(z["dtype"]) if "dtype" in z.files else "bf16"
    w = synth.synth_weights(cfg, int(z["seed"]), bf16=(dtype == "bf16"), **json.loads(str(z["wkw"])))
    return z, cfg, w, dtype


def oracle_vs_reference(golden_dir, name):
    """Greedy fixture: the oracle, teacher-forced on the reference's out_ids, against ref_lp at every used slot where its
    decision (argmax of its own processed scores) equals the reference's."""
    z, cfg, w, dtype = load(golden_dir, name)
    layers = json.loads(str(z["layers"]))
    orc = ao.AsteroidOracle(cfg, w, dtype)
    orc.keep_scores = True
    orc.generate(z["input_ids"], z["attention_mask"], int(z["max_length"]), layers=layers, forced=z["out_ids"])
    used, ref_dec, ref_lp = z["used"], z["ref_dec"], z["ref_lp"]
    steps, B, _ = used.shape
    assert len(orc.last_scores) == steps
    dev, n_used, n_cmp = 0.0, 0, 0
    for s in range(steps):
        for c in range(8):
            sc = orc.last_scores[s][c]
            for b in range(B):
                if not used[s, b, c]:
                    continue
                n_used += 1
                d = int(np.argmax(sc[b]))
                if d != ref_dec[s, b, c]:
                    continue
                n_cmp += 1
                dev = max(dev, abs(sr.log_softmax64(sc[b], d) - float(ref_lp[s, b, c])))
    return {"D_oracle": dev, "used": n_used, "compared": n_cmp,
            "lp_min": float(ref_lp[used].min()), "lp_max": float(ref_lp[used].max())}


def sampled_reference_lp(z, s, b, c, d):
    """ar_sampled.npz stores the reference's full kept set (<= 32 entries) of every slot: the reference's
    log-probability of token d, or None when d is outside its kept set."""
    idx = z["kept_idx"][s, b, c]
    hit = np.nonzero(idx == d)[0]
    if hit.size == 0:
        return None
    val = z["kept_val"][s, b, c][idx >= 0].astype(np.float64)
    m = val.max()
    return float(z["kept_val"][s, b, c][hit[0]]) - m - float(np.log(np.exp(val - m).sum()))


def sampled_used(z, cfg):
    gold = z["out_ids"]
    base = z["input_ids"].shape[1] - 7
    return sr.used_mask(gold[:, base:].transpose(1, 0, 2), base, int(z["max_length"]), cfg)


def oracle_vs_reference_sampled(golden_dir, seed=77):
    """ar_sampled.npz replayed through the oracle with forced_as_draw (the state follows the reference's history, the
    draws are the oracle's own Philox draws): where a draw lies in the reference's kept set, the oracle's lp against
    kept_val[d] - logsumexp(kept_val)."""
    z, cfg, w, _ = load(golden_dir, "ar_sampled")
    layers = json.loads(str(z["layers"]))
    orc = ao.AsteroidOracle(cfg, w, "bf16")
    orc.keep_scores = True
    _, odec, _ = orc.generate(z["input_ids"], z["attention_mask"], int(z["max_length"]), layers=layers,
                              do_samples=[True] * 8, seed=seed, forced=z["out_ids"], forced_as_draw=True)
    used = sampled_used(z, cfg)
    devs, n_used = [], 0
    for s in range(odec.shape[0]):
        for b in range(odec.shape[1]):
            for c in range(8):
                if not used[s, b, c]:
                    continue
                n_used += 1
                d = int(odec[s, b, c])
                ref = sampled_reference_lp(z, s, b, c, d)
                if ref is None:
                    continue
                devs.append(abs(sr.log_softmax64(orc.last_scores[s][c][b], d) - ref))
    return {"D_sampled": float(max(devs)), "median": float(np.median(devs)), "used": n_used, "compared": len(devs), "seed": seed}
