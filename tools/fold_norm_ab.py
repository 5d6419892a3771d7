"""A/B of the seam o_proj -> post-attention RMSNorm -> gate/up at the bench's dims (csrc/gemm_fold.hip): launch trains over
rotating copies of both weight arrays (12 copies of 8.4 + 50.3 MB, more than 600 MB, so every launch reads its weights from
HBM), the three launches of today against producer + consumer, alternating, 8 legs each, in one process (tuning aid, GPU box only).  Prints one JSON object: per leg kind the times of
one pass through the seam in us, their mean and max - min."""
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "moss-ttsd_amd"))
from mtts import capi  # noqa: E402

N_GU, COPIES = 12288, 12
MODES = [("three_launches", 0), ("pair", 1), ("o_proj", 10), ("resid_norm", 11), ("gate_up", 12), ("producer", 13), ("consumer", 14)]


def main():
    legs = int(sys.argv[sys.argv.index("--legs") + 1]) if "--legs" in sys.argv else 8
    os.environ["MTTS_GEMM_DEPTH"] = "1"
    lib = capi.lib()
    out = {name: {"us": []} for name, _ in MODES}
    for leg in range(legs):
        for name, mode in MODES:
            us = C.c_float()
            capi.check(lib.mtts_k_fold_bench(N_GU, COPIES, COPIES * 8, mode, C.byref(us)))
            out[name]["us"].append(round(us.value, 3))
        print(leg, {n: out[n]["us"][-1] for n, _ in MODES}, file=sys.stderr, flush=True)
    for name, _ in MODES:
        t = out[name]["us"]
        out[name]["mean"] = round(sum(t) / len(t), 3)
        out[name]["spread"] = round(max(t) - min(t), 3)
    out["copies"], out["weights_MB"] = COPIES, round(COPIES * (2048 * 2048 + N_GU * 2048) * 2 / 1e6, 1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
