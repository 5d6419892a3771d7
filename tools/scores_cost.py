"""What output_scores costs per decode step, at the benchmark's operating point.

B=32 dialogues at ~4 k tokens of context, the assumed 1.7B dims, (a) top-k 50 / top-p 0.95 sampling on all 8 channels
(bench.py's flagship setting) and (b) all channels greedy.  One engine; legs off / on / off / on, each leg = begin, a real
ramp to the target context, a warm-up, then REPS timed trains of STEPS decode steps (host clock around step + sync_state).
Train i of every leg sits at the same KV lengths, and the step time depends on them (a leg's trains differ by ~90 us in a
fixed pattern), so figures are only ever compared train by train.  The switch is read when a run begins, so every leg
is a run of its own.

    python tools/scores_cost.py --out out/scores_cost.json
    python tools/scores_cost.py --pkg <a checkout of the commit before the feature>/moss-ttsd_amd --label <its hash> --out before.json
    python tools/scores_cost.py --before-json before.json [more.json ...] --out out/scores_cost.json
    python tools/scores_cost.py --from-json out/scores_cost.json --before-json ... --out ...      (evaluate only)

A build without the switch runs the off legs only.  With --before-json those runs (one process each) are embedded and
the acceptance is evaluated per (leg, train) index: a scores-off train lies inside the earlier build's run-to-run spread
when it is within the range its processes span at that index; trains above and below it are counted separately.  The
scores-on trains are compared the same way and reported, not gated.
MTTS_PAGE_SHUFFLE (engine test hook: shuffled KV page placement) is recorded when set.  Results: profiles/scores_cost*.json.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pkg", default=os.path.join(ROOT, "moss-ttsd_amd"), help="package directory to measure")
    ap.add_argument("--label", default="output_scores")
    ap.add_argument("--out", required=True)
    ap.add_argument("--before-json", nargs="+", help="results of this tool for the build before the feature")
    ap.add_argument("--modes", default="sampled,greedy")
    ap.add_argument("--from-json", help="evaluate an earlier result of this tool against --before-json instead of measuring")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--context", type=int, default=4096)
    ap.add_argument("--prompt", type=int, default=512)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--legs", type=int, default=4, help="legs per mode (off, on alternating where the build has the switch)")
    args = ap.parse_args()
    if args.from_json:
        with open(args.from_json) as f:
            out = json.load(f)
        args.reps = out["trains_per_leg"]
        return finish(out, args)
    sys.path.insert(0, ROOT)
    import torch
    import bench                                   # (puts this checkout's package on sys.path: --pkg must come after it)
    sys.path.insert(0, os.path.abspath(args.pkg))
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
    has_switch = hasattr(eng, "set_output_scores")
    ids, mask = synth.synth_prompts(cfg, 77, B, T, audio_frac=0.5, ragged=False)
    max_length = T + (L - n_real) + 8
    modes = {"sampled": ([dict(top_k=50, top_p=0.95, temperature=1.0, repetition_penalty=1.0)] * 8, [True] * 8),
             "greedy": (None, [False] * 8)}
    modes = {k: v for k, v in modes.items() if k in args.modes.split(",")}
    out = {"label": args.label, "page_shuffle": os.environ.get("MTTS_PAGE_SHUFFLE"), "batch": B, "context": L, "steps_per_train": K, "trains_per_leg": args.reps,
           "has_switch": has_switch, "modes": {}}
    for mode, (layers, ds) in modes.items():
        legs = []
        for leg in range(args.legs):
            on = bool(has_switch and leg % 2)
            kw = dict(output_scores=on) if has_switch else {}
            eng.begin(ids, mask, max_length, layers=layers, do_samples=ds, seed=42, **kw)
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
            if on:
                lp = eng.read_scores(ramp + W + K * args.reps + 8)
                assert lp.shape[0] == ramp + W + K * args.reps
            legs.append({"scores": on, "ms_per_step_trains": trains, "median_ms": statistics.median(trains),
                         "min_ms": min(trains), "max_ms": max(trains)})
            print(mode, "leg", leg, "scores", on, "ms/step", [round(t, 4) for t in trains], flush=True)
            if has_switch:
                # the switch cannot change while rows are unfinished: an empty scheduler run (same setting) replaces the
                # abandoned one, and the next leg's begin may then flip it
                eng.sched_open(B, 16, output_scores=on)
        off = [l for l in legs if not l["scores"]]
        onl = [l for l in legs if l["scores"]]
        R = range(args.reps)
        m = {"legs": legs, "off_ms": statistics.median(l["median_ms"] for l in off),
             "off_by_train_ms": [[l["ms_per_step_trains"][i] for l in off] for i in R]}
        if onl:
            m["on_ms"] = statistics.median(l["median_ms"] for l in onl)
            m["on_by_train_ms"] = [[l["ms_per_step_trains"][i] for l in onl] for i in R]
            # on minus off at equal KV length: mean over legs, per train index
            m["on_minus_off_by_train_us"] = [(statistics.mean(m["on_by_train_ms"][i]) - statistics.mean(m["off_by_train_ms"][i])) * 1e3
                                             for i in R]
        out["modes"][mode] = m
    eng.close()
    finish(out, args)


def finish(out, args):
    if args.before_json:
        runs = [json.load(open(p)) for p in args.before_json]
        out["before"] = runs
        for mode, m in out["modes"].items():
            # leg j, train i of this build against leg j, train i of every process of the earlier build: the step time
            # depends on both indices (KV length; and the legs of a process alternate by ~25 us in either build)
            rows = []
            for j, leg in enumerate(m["legs"]):
                for i, t in enumerate(leg["ms_per_step_trains"]):
                    ref = [r["modes"][mode]["legs"][j]["ms_per_step_trains"][i] for r in runs]
                    rows.append({"leg": j, "train": i, "scores": leg["scores"], "ms": t, "before_range_ms": [min(ref), max(ref)],
                                 "inside": bool(min(ref) <= t <= max(ref)), "above": bool(t > max(ref)),
                                 "minus_before_mean_us": (t - statistics.mean(ref)) * 1e3})
            m["vs_before_by_leg_and_train"] = rows
            for key, flag in (("off", False), ("on", True)):
                sel = [r for r in rows if r["scores"] == flag]
                if sel:
                    m[key + "_vs_before"] = {"trains": len(sel), "inside": sum(r["inside"] for r in sel),
                                             "above": sum(r["above"] for r in sel),
                                             "below": sum(not r["inside"] and not r["above"] for r in sel),
                                             "mean_minus_before_us": statistics.mean(r["minus_before_mean_us"] for r in sel),
                                             "max_minus_before_max_us": max((r["ms"] - r["before_range_ms"][1]) * 1e3 for r in sel)}
            m["off_inside_before_spread"] = bool(all(r["inside"] for r in rows if not r["scores"]))
            m["off_not_above_before_spread"] = bool(not any(r["above"] for r in rows if not r["scores"]))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({k: {kk: vv for kk, vv in v.items() if kk not in ("legs", "off_by_train_ms", "on_by_train_ms", "vs_before_by_leg_and_train")}
                      for k, v in out["modes"].items()}, indent=1))


if __name__ == "__main__":
    main()
