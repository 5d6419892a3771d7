"""What generate(top_logprobs=k) costs per decode step, at the benchmark's operating point.

B=32 dialogues at ~4 k tokens of context, the assumed 1.7B dims, top-k 50 / top-p 0.95 sampling on all 8 channels
(bench.py's flagship setting).  One engine; legs off / k=1 / k=8 / k=16, the whole cycle repeated --cycles times, each leg =
begin, a real ramp to the target context, a warm-up, then REPS timed trains of STEPS decode steps (host clock around
step + sync_state).  Train i of every leg sits at the same KV lengths, and the step time depends on them (tools/scores_cost.py),
so a train is only ever compared with the train of the same index of the off leg of its cycle.  The switch is read when a
run begins, so every leg is a run of its own.

    python tools/gen_topk_cost.py --out profiles/gen_topk_cost.json
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/gen_topk_cost.py --cycles 1 --reps 1 --ks 1,8,16 --out <dir>/traced.json
    python tools/gen_topk_cost.py --from-json profiles/gen_topk_cost.json --kernel-stats <dir>/.../*_kernel_stats.csv --out profiles/gen_topk_cost.json

The second form is a run of its own under the profiler (its step times are not used); the third merges the average
duration of gen_topk_slice_kernel / gen_topk_finish_kernel / update_kernel per instantiation into the result.
"""
import argparse
import csv
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ("gen_topk_slice_kernel", "gen_topk_finish_kernel", "update_kernel")


def kernel_stats(paths):
    """rocprofv3 --stats kernel CSVs -> {kernel name: {calls, avg_us}} for the kernels of the feature."""
    out = {}
    for p in paths:
        with open(p) as f:
            for row in csv.DictReader(f):
                name = row.get("Name") or row.get("KernelName") or ""
                if any(k in name for k in KERNELS):
                    calls = int(row.get("Calls") or row.get("Count") or 0)
                    avg_ns = float(row.get("AverageNs") or row.get("Average") or 0.0)
                    out[name.split("(")[0]] = {"calls": calls, "avg_us": avg_ns / 1e3}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--from-json", help="an earlier result of this tool: merge --kernel-stats into it instead of measuring")
    ap.add_argument("--kernel-stats", nargs="+", help="kernel stats CSVs of a rocprofv3 --kernel-trace --stats run of this tool")
    ap.add_argument("--ks", default="1,8,16")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--context", type=int, default=4096)
    ap.add_argument("--prompt", type=int, default=512)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cycles", type=int, default=2, help="times the legs off, k... are repeated")
    args = ap.parse_args()
    if args.from_json:
        with open(args.from_json) as f:
            out = json.load(f)
    else:
        out = measure(args)
    if args.kernel_stats:
        out["kernel_trace_avg"] = kernel_stats(args.kernel_stats)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({k: v for k, v in out.items() if k != "legs"}, indent=1))


def measure(args):
    sys.path.insert(0, ROOT)
    import torch
    import bench                                   # (puts the package on sys.path)
    from mtts import capi, synth
    from mtts.engine import Engine

    device = torch.device("cuda:0")
    torch.cuda.set_device(device)
    cfg = synth.assumed_1p7b()
    B, L, T, K, W = args.batch, args.context, args.prompt, args.steps, 8
    n_real = T - 7
    ramp = L - n_real - W - K * args.reps
    eng = Engine(cfg, max_batch=B, max_seq_len=L + 64, device=str(device))
    for name, t in bench.make_weights_on_device(cfg, 1234, device, 0, 1):
        eng.bind(name, t)
        del t
    capi.check(eng.lib.mtts_weights_ready(eng._h))
    ids, mask = synth.synth_prompts(cfg, 77, B, T, audio_frac=0.5, ragged=False)
    max_length = T + (L - n_real) + 8
    layers, ds = [dict(top_k=50, top_p=0.95, temperature=1.0, repetition_penalty=1.0)] * 8, [True] * 8
    ks = [0] + [int(k) for k in args.ks.split(",")]
    legs = []
    for cycle in range(args.cycles):
        for k in ks:
            eng.begin(ids, mask, max_length, layers=layers, do_samples=ds, seed=42, top_logprobs=k)
            done = 0
            while done < ramp:
                n = min(256, ramp - done)
                eng.step(n)
                done += n
                _, fin = eng.sync_state()
                assert not fin
            eng.step(W)
            eng.sync_state()
            trains = []
            for _ in range(args.reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                eng.step(K)
                _, fin = eng.sync_state()
                trains.append((time.perf_counter() - t0) / K * 1e3)
                assert not fin
            if k:
                lp, tid, tlp = eng.read_top_logprobs(ramp + W + K * args.reps + 8)
                assert lp.shape[0] == ramp + W + K * args.reps and tid.shape[-1] == k
            legs.append({"cycle": cycle, "k": k, "ms_per_step_trains": trains, "median_ms": statistics.median(trains)})
            print("cycle", cycle, "k", k, "ms/step", [round(t, 4) for t in trains], flush=True)
            # the switch cannot change while rows are unfinished: an empty scheduler run (same setting) replaces the
            # abandoned one, and the next leg's begin may then change it
            eng.sched_open(B, 16, top_logprobs=k)
    eng.close()
    out = {"what": "decode step with generate(top_logprobs=k), B=%d at %d tokens of context, sampled; per-step times of "
                   "trains of %d steps, compared with the same train of the off leg of the same cycle" % (B, L, K),
           "batch": B, "context": L, "steps_per_train": K, "trains_per_leg": args.reps, "cycles": args.cycles, "legs": legs}
    off = {l["cycle"]: l for l in legs if l["k"] == 0}
    out["off_ms"] = statistics.median(l["median_ms"] for l in off.values())
    # the off legs of two cycles at equal train index: what process-internal repetition alone moves a train by
    if args.cycles > 1:
        out["off_leg_to_leg_spread_us"] = max(abs(off[0]["ms_per_step_trains"][i] - off[c]["ms_per_step_trains"][i]) * 1e3
                                              for c in range(1, args.cycles) for i in range(args.reps))
    out["on_minus_off_us"] = {}
    for k in ks[1:]:
        d = [(l["ms_per_step_trains"][i] - off[l["cycle"]]["ms_per_step_trains"][i]) * 1e3
             for l in legs if l["k"] == k for i in range(args.reps)]
        out["on_minus_off_us"][str(k)] = {"mean": statistics.mean(d), "min": min(d), "max": max(d), "trains": len(d)}
    return out


if __name__ == "__main__":
    main()
