"""Unmerged adapter row against the merged adapter, the figures behind tests/test_multi_adapter_gpu.py::
test_unmerged_row_against_the_merged_adapter: 48 greedy steps with the adapter merged, replayed through the unmerged row.
Prints one JSON document (kept as profiles/multi_adapter_parity.json): decisions, how many the gate leaves out, every miss
with its margin, and the largest absolute logit difference of each step under the replay."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "moss-ttsd_amd"), ROOT):
    sys.path.insert(0, p)
os.environ.setdefault("MTTS_KV_PACK_MIN", "0")           # as tests/conftest.py


def main():
    import multi_adapter_case as case
    r = case.merged_vs_unmerged()
    free = case.free_decisions(case.PARITY_STEPS)
    differ = free & (r["dec"] != r["gen"])
    safe = free & (r["margins"] >= case.PARITY_GATE)
    d = max(r["logit_diff"])
    safe_abs = free & (r["gaps"] >= 2 * d)
    print(json.dumps(dict(
        what="tiny model, adapter 1 (rank 8 on all seven projections of both layers, rsLoRA scaling 5.657): 48 greedy steps of one "
             "dialogue with the adapter merged (Engine.bind_lora), replayed through the unmerged row (forced=)",
        decisions=int(free.sum()), differing=int(differ.sum()), max_miss_gap=float(r["gaps"][differ].max(initial=0)),
        gate=case.PARITY_GATE, below_gate=int((free & ~safe).sum()),
        misses_above_gate=int((differ & safe).sum()), misses_below_gate=int((differ & ~safe).sum()),
        max_abs_logit_diff=d, gate_abs=2 * d, below_gate_abs=int((free & ~safe_abs).sum()),
        misses_above_gate_abs=int((differ & safe_abs).sum()), misses_below_gate_abs=int((differ & ~safe_abs).sum()),
        misses=[dict(step=int(s), channel=int(c), merged=int(r["gen"][s, b, c]), unmerged=int(r["dec"][s, b, c]),
                     margin=float(r["margins"][s, b, c]), gap=float(r["gaps"][s, b, c])) for s, b, c in np.argwhere(differ)],
        max_abs_logit_diff_per_step=r["logit_diff"],
        smallest_margin=float(r["margins"][free].min()), median_gap=float(np.median(r["gaps"][free]))), indent=1))


if __name__ == "__main__":
    main()
