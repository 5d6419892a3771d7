"""Per-kernel A/B of the sealed weight streams (csrc/gemm_sealed.hip) against the bf16 kernels they shadow: trains of
launches of gate/up, down_proj, head 0 and heads 1-7 at the bench's dims over rotating weight copies (more than 600 MB
of them, so that every launch reads its weights from HBM), bf16 / sealed / bf16 / sealed ... in one process (tuning aid,
GPU box only).  Weights: N(0, 0.02^2) as the bench draws them ("gaussian": whatever share of its groups does not seal);
the same with every magnitude raised to at least 2^-12 ("clean": every group seals); and clean weights in which every
8th group / every group was given a lane of 9 binade pairs ("eighth", "all"; `--variants` also takes "f64", "f512": every
64th / 512th group): the cost of the not-sealed path, and the point where the sealed train stops beating the bf16 one.
The heads also run in their two sealed forms (persistent / one tile per block).  Results: profiles/wseal_ab.json.  Prints one JSON object; `--legs N` sets the number of off/on pairs, `--only a,b` the shapes."""
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "moss-ttsd_amd"))
from mtts import capi  # noqa: E402

# name, N, K, epi, split-K, k-tiles per wave
SHAPES = [("gate_up", 12288, 2048, 2, 1, 16), ("down_proj", 2048, 6144, 0, 4, 12), ("head0", 152697, 2048, 1, 1, 16),
          ("heads17", 7 * 1056, 2048, 1, 1, 16)]
NINE = [(0x3f - j) << 8 for j in range(9)]


def weights(N, K, ktw, variant, seed):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    w = 0.02 * torch.randn(N, K, device="cuda", generator=g)
    if variant != "gaussian":
        w = torch.where(w < 0, -1.0, 1.0) * w.abs().clamp(min=2.0 ** -12)
    w = w.to(torch.bfloat16).contiguous()
    every = {"gaussian": 0, "clean": 0, "f512": 512, "f64": 64, "eighth": 8, "all": 1}[variant]
    if every:
        bits = w.view(torch.int16)
        span, G = 16 * ktw, K // (16 * ktw)
        nine = torch.tensor(NINE, dtype=torch.int16, device="cuda")
        for nt in range((N + 31) // 32):
            for c in range(G):
                if (nt * G + c) % every == 0 and nt * 32 < N:
                    bits[nt * 32, c * span:c * span + 9 * 16:16] = nine
    return w


def train(lib, w, N, K, epi, ks, copies, sealed, form):
    us, st = C.c_float(), np.zeros(2, dtype=np.int64)
    capi.check(lib.mtts_k_gemm_sealed_bench(w.data_ptr(), N, K, epi, ks, copies, copies * 4, sealed, form, C.byref(us), st.ctypes.data))
    return round(us.value, 3), int(st[0]), int(st[1])


def summary(v):
    return {"us": v, "mean": round(sum(v) / len(v), 3), "spread": round(max(v) - min(v), 3)}


def main():
    legs = int(sys.argv[sys.argv.index("--legs") + 1]) if "--legs" in sys.argv else 8
    only = sys.argv[sys.argv.index("--only") + 1].split(",") if "--only" in sys.argv else None
    variants = sys.argv[sys.argv.index("--variants") + 1].split(",") if "--variants" in sys.argv else ("gaussian", "clean", "eighth", "all")
    lib = capi.lib()
    out = {}
    for name, N, K, epi, ks, ktw in SHAPES:
        if only and name not in only:
            continue
        mb = N * K * 2 / 1e6
        copies = int(600 / mb) + 2
        forms = (1, 0) if epi == 1 else (0,)
        res = {"MB": round(mb, 1), "sealed_MB": round(mb * (ktw // 2 + ktw // 4 + 1) / ktw, 1), "copies": copies}
        for variant in variants:
            w = weights(N, K, ktw, variant, 17)
            legs_v = legs if variant == "gaussian" else max(2, legs // 2)
            off, on = [], {f: [] for f in forms}
            for _ in range(legs_v):
                off.append(train(lib, w, N, K, epi, ks, copies, 0, 0)[0])
                for f in forms:
                    us, groups, bad = train(lib, w, N, K, epi, ks, copies, 1, f)
                    on[f].append(us)
            r = {"groups": groups, "not_sealed": bad, "bf16": summary(off)}
            for f in forms:
                r["sealed" if epi != 1 else ("sealed_persistent" if f else "sealed_tile_per_block")] = summary(on[f])
            res[variant] = r
            print(name, variant, r, file=sys.stderr, flush=True)
            del w
        out[name] = res
    print(json.dumps(out))


if __name__ == "__main__":
    main()
