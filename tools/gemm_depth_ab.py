"""Per-kernel A/B of the depth-specialised decode GEMMs (csrc/gemm.hip) against gemm_skinny_kernel: trains of launches of
the four projections of a layer at the bench's dims over rotating weight copies (>= 16, and more than 600 MB of them, so
that every launch reads its weights from HBM), MTTS_GEMM_DEPTH = 0 / 1 / 0 / 1 ... in one process (tuning aid, GPU box
only).  Prints one JSON object; `--legs N` sets the number of off/on pairs."""
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "moss-ttsd_amd"))
from mtts import capi  # noqa: E402

SHAPES = [("qkv", 4096, 2048, 0, 2), ("o_proj", 2048, 2048, 0, 4), ("down_proj", 2048, 6144, 0, 4), ("gate_up", 12288, 2048, 2, 1)]


def main():
    legs = int(sys.argv[sys.argv.index("--legs") + 1]) if "--legs" in sys.argv else 3
    lib = capi.lib()
    out = {}
    for name, N, K, epi, ks in SHAPES:
        mb = N * K * 2 / 1e6
        copies = max(16, int(600 / mb) + 1)
        res = {"MB": round(mb, 1), "copies": copies, "off_us": [], "on_us": []}
        for leg in range(legs):
            for sw in ("0", "1"):
                os.environ["MTTS_GEMM_DEPTH"] = sw
                us = C.c_float()
                capi.check(lib.mtts_k_gemm_bench(N, K, epi, ks, 8, copies, copies * 4, C.byref(us)))
                res["on_us" if sw == "1" else "off_us"].append(round(us.value, 3))
        res["off_mean"] = round(sum(res["off_us"]) / legs, 3)
        res["on_mean"] = round(sum(res["on_us"]) / legs, 3)
        res["off_spread"] = round(max(res["off_us"]) - min(res["off_us"]), 3)
        res["on_spread"] = round(max(res["on_us"]) - min(res["on_us"]), 3)
        out[name] = res
        print(name, res, file=sys.stderr, flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
