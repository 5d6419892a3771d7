"""Measure, on the GPU, how far the engine's output_scores sit from the reference's on the three fixtures
(tests/golden/ar_scores_bf16.npz, ar_scores_fp32.npz, ar_sampled.npz) and add the figures as `engine` entries to a copy
of profiles/scores_parity.json.  Run once per change of the sampler and commit the result as
profiles/scores_parity.json; the tests read only D_oracle / D_sampled from that file (measured on the CPU by
tests/golden/make_golden_scores.py), the engine's own maxima are a record.

    python tools/scores_parity.py --out out/scores_parity.json
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "moss-ttsd_amd"), ROOT):
    sys.path.insert(0, p)
os.environ.setdefault("MTTS_KV_PACK_MIN", "0")          # sealed KV reads on, as in the test suite


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    import scores_parity_cpu as spc
    from mtts.engine import Engine
    golden = os.path.join(ROOT, "tests", "golden")
    with open(os.path.join(ROOT, "profiles", "scores_parity.json")) as f:
        rec = json.load(f)
    for name in ("ar_scores_bf16", "ar_scores_fp32"):
        z, cfg, w, dtype = spc.load(golden, name)
        eng = Engine(cfg, max_batch=4, max_seq_len=256, dtype=dtype)
        eng.bind_state_dict(w)
        _, dec, lp = eng.generate(z["input_ids"], z["attention_mask"], int(z["max_length"]),
                                  layers=json.loads(str(z["layers"])), forced=z["out_ids"], output_scores=True)
        eng.close()
        lp = lp.transpose(1, 0, 2)
        same = z["used"] & (dec == z["ref_dec"])
        dev = np.abs(lp[same].astype(np.float64) - z["ref_lp"][same])
        rec["cases"][name]["engine"] = {"max_deviation": float(dev.max()), "median_deviation": float(np.median(dev)),
                                        "used": int(z["used"].sum()), "compared": int(same.sum()),
                                        "nan_pattern_equals_rule": bool(np.array_equal(np.isnan(lp), ~z["used"]))}
    z, cfg, w, _ = spc.load(golden, "ar_sampled")
    seed = rec["cases"]["ar_sampled"]["seed"]
    eng = Engine(cfg, max_batch=2, max_seq_len=256)
    eng.bind_state_dict(w)
    _, dec, lp = eng.generate(z["input_ids"], z["attention_mask"], int(z["max_length"]), layers=json.loads(str(z["layers"])),
                              do_samples=[True] * 8, seed=seed, forced=z["out_ids"], forced_as_draw=True, output_scores=True)
    eng.close()
    lp = lp.transpose(1, 0, 2)
    used = spc.sampled_used(z, cfg)
    devs = []
    for s, b, c in zip(*np.nonzero(used)):
        ref = spc.sampled_reference_lp(z, s, b, c, int(dec[s, b, c]))
        if ref is not None:
            devs.append(abs(float(lp[s, b, c]) - ref))
    rec["cases"]["ar_sampled"]["engine"] = {"max_deviation": float(max(devs)), "median_deviation": float(np.median(devs)),
                                            "used": int(used.sum()), "compared": len(devs),
                                            "nan_pattern_equals_rule": bool(np.array_equal(np.isnan(lp), ~used))}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(rec, indent=1))


if __name__ == "__main__":
    main()
