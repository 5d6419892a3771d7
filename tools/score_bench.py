"""What teacher-forced scoring costs, at the assumed 1.7B dims: Engine.score on B x T tokens (default 8 x 2048).

Records
  * scored tokens/s of the whole call (host clock around Engine.score, which is synchronous; the median of --reps calls
    after one warm-up call that also pays the first-use allocations);
  * the share of the call spent in head_ce_kernel + ce_finish_kernel (hipEvents around the two launches of every prefill
    pass, from a separate profiled call: mtts_profile_read slot 4);
  * for comparison, what merely MATERIALISING the logits costs: gemm_tile_kernel with the bf16 store epilogue at the same
    M, N, K (mtts_k_gemm_bench, waves < 0), head 0 and the seven speech heads -- without any log-softmax pass over the
    625 MB it writes.

    python tools/score_bench.py --out out/score_bench.json

Results: profiles/score_bench.json.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--tokens", type=int, default=2048)
    ap.add_argument("--layers", type=int, default=0, help="0: the config's 28")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--gemm-iters", type=int, default=5)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    import bench                                   # (puts the package on sys.path)
    from mtts import capi, synth
    from mtts.engine import Engine

    device = torch.device("cuda:0")
    torch.cuda.set_device(device)
    cfg = synth.assumed_1p7b()
    if args.layers:
        cfg["num_hidden_layers"] = args.layers
    B, T = args.batch, args.tokens
    eng = Engine(cfg, max_batch=B, max_seq_len=T, device=str(device))
    for name, t in bench.make_weights_on_device(cfg, 1234, device, 0, 1):
        eng.bind(name, t)
        del t
    capi.check(eng.lib.mtts_weights_ready(eng._h))
    rng = np.random.default_rng(5)
    ids = np.full((B, T, 8), 1024, dtype=np.int64)
    ids[:, :, 0] = synth.SPEECH_OFFSET + rng.integers(0, 1024, (B, T))
    ids[:, :, 1:] = rng.integers(0, 1024, (B, T, 7))
    mask = np.ones((B, T), dtype=np.uint8)
    labels = ids.copy()
    first = eng.score(ids, mask, labels)           # warm-up: first-use allocations, code objects
    assert np.isfinite(first[:, 1:]).all()
    calls = []
    for _ in range(args.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        lp = eng.score(ids, mask, labels)
        calls.append(time.perf_counter() - t0)
        assert np.array_equal(lp.view(np.uint32), first.view(np.uint32))
    eng.profile(True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    eng.score(ids, mask, labels)
    profiled_call = time.perf_counter() - t0
    ce_ms, ce_passes, _ = eng.profile_read(4)
    eng.profile(False)
    eng.close()
    # the parent's way to the same logits: the tiled prefill GEMM with the bf16 store, one pass of 2048 rows
    lib = capi.lib()
    H, V0p, Vsp = cfg["hidden_size"], (cfg["vocab_size"] + 31) // 32 * 32, (cfg["speech_vocab_size"] + 31) // 32 * 32
    rows = min(2048, B * T)
    us = C.c_float(0)
    gemm = {}
    for key, N in (("head0", V0p), ("heads17", 7 * Vsp)):
        capi.check(lib.mtts_k_gemm_bench(N, H, 1, 1, -rows, 1, args.gemm_iters, C.byref(us)))
        gemm[key + "_us"] = us.value
    passes = (B * T + 2047) // 2048
    call = statistics.median(calls)
    out = {
        "config": {k: cfg[k] for k in ("hidden_size", "intermediate_size", "num_hidden_layers", "num_attention_heads",
                                       "num_key_value_heads", "vocab_size", "speech_vocab_size")},
        "batch": B, "tokens_per_sequence": T, "prefill_passes": passes,
        "score_call_s": calls, "score_call_median_s": call, "scored_tokens_per_s": B * T / call,
        "profiled_call_s": profiled_call, "head_ce_plus_finish_ms_per_call": ce_ms, "profiled_passes": ce_passes,
        "head_ce_plus_finish_ms_per_pass": ce_ms / max(ce_passes, 1),
        "head_ce_share_of_call": ce_ms * 1e-3 / call,
        "gemm_tile_bf16_store_same_shape": dict(gemm, rows=rows, ms_per_pass=(gemm["head0_us"] + gemm["heads17_us"]) * 1e-3,
                                                logits_bytes_per_pass=rows * (V0p + 7 * Vsp) * 2),
    }
    out["fused_over_materialising_gemm"] = out["head_ce_plus_finish_ms_per_pass"] / out["gemm_tile_bf16_store_same_shape"]["ms_per_pass"]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
