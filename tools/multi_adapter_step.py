"""Decode step with per-dialogue adapters at the bench shape (B = 32, 4 k context, 28 layers, r = 16 on all seven
projections): the step with an empty bank, with a loaded bank and no adapter row, and with 1, 4 and 8 distinct adapters
spread over the rows.  One JSON document on stdout (kept as profiles/multi_adapter_step.json).

    python tools/multi_adapter_step.py                          # the table: ms per step, host clock around steps + sync
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/multi_adapter_step.py --only 8 --steps 32
                                                                # per-kernel times of one configuration (tools/rocpd_stats.py)

The context is set with mtts_debug_set_kv_len, as in bench.py --fake-context: the step's kernels run at 4 k positions
without a 3.5 k-step ramp per configuration."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "moss-ttsd_amd"))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--context", type=int, default=4096)
    ap.add_argument("--rank", type=int, default=16)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--only", type=int, default=None, help="one configuration: that many distinct adapters (rocprofv3 runs)")
    args = ap.parse_args()
    import torch
    import bench
    from mtts import adapters, capi, synth
    from mtts.engine import Engine
    device = torch.device("cuda:0")
    cfg = synth.assumed_1p7b()
    B, L, T = args.batch, args.context, 512
    eng = Engine(cfg, max_batch=B, max_seq_len=L + 64, device=str(device))
    for name, t in bench.make_weights_on_device(cfg, 1234, device, 0, 1):
        eng.bind(name, t)
        del t
    capi.check(eng.lib.mtts_weights_ready(eng._h))
    ids, mask = synth.synth_prompts(cfg, 77, B, T, audio_frac=0.5, ragged=False)
    layers = [dict(top_k=50, top_p=0.95, temperature=1.0, repetition_penalty=1.0)] * 8
    per_rep = args.steps + args.warmup
    kv0 = L - per_rep * args.repeats - 8

    def adapter(seed):
        g = torch.Generator(device=device)
        g.manual_seed(seed)
        out = {}
        for n in range(cfg["num_hidden_layers"]):
            for p in adapters.PROJECTIONS:
                o, i = adapters.projection_shape(cfg, p)
                out[f"model.language_model.layers.{n}.{p}.weight"] = (torch.randn(args.rank, i, device=device, generator=g) * 0.01,
                                                                      torch.randn(o, args.rank, device=device, generator=g) * 0.01)
        return out

    def measure(row_adapters):
        eng.begin(ids, mask, T + (L - (T - 7)) + 8, layers=layers, do_samples=[True] * 8, seed=42, row_adapters=row_adapters)
        eng.sync_state()
        eng.debug_set_kv_len(kv0)
        ms = []
        for _ in range(args.repeats):
            eng.step(args.warmup)
            eng.sync_state()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            eng.step(args.steps)
            _, fin = eng.sync_state()
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3 / args.steps)
            assert not fin, "a dialogue finished inside the timed steps"
        eng.sched_open(B, 64)              # ends the run
        return dict(ms_per_step=float(np.median(ms)), ms_per_step_runs=[float(x) for x in ms])

    out = dict(what=f"decode step, B = {B}, KV length {kv0}..{L} (mtts_debug_set_kv_len), {cfg['num_hidden_layers']} layers, rank {args.rank} on "
                    f"all seven projections; median of {args.repeats} x {args.steps} steps after {args.warmup} warm-up steps each, host clock "
                    "around mtts_step + mtts_sync_state", configs={})
    todo = [0, 1, 4, 8] if args.only is None else [args.only]
    if args.only is None:
        out["configs"]["empty_bank"] = measure(None)
    for i in range(max(todo)):
        eng.load_bank_adapter(i, adapter(100 + i), 2.0)
    if args.only is None:
        out["configs"]["bank_loaded_no_adapter_row"] = measure([-1] * B)
    for n in todo:
        if n:
            out["configs"][f"{n}_adapters"] = measure([b % n for b in range(B)])
    if "empty_bank" in out["configs"]:
        base = out["configs"]["empty_bank"]["ms_per_step"]
        for k, v in out["configs"].items():
            v["delta_ms_vs_empty_bank"] = v["ms_per_step"] - base
    print(json.dumps(out, indent=1))
    eng.close()


if __name__ == "__main__":
    main()
