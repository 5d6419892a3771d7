"""What generate(logits_processor= / stopping_criteria= / streamer=) costs per decode step, at the benchmark's operating point.

B=32 dialogues at ~4 k tokens of context, the assumed 1.7B dims, top-k 50 / top-p 0.95 sampling on all 8 channels
(bench.py's flagship setting).  One engine, one process; the legs, the whole cycle repeated --cycles times:

    plain      Engine.step(1) + sync_state per step: the unsplit step, replayed from its captured graph, with the host
               round trip per step that every hooked run has (so the legs below differ from it by the split alone)
    run_ahead  Engine.step(K) + one sync_state: the unsplit step as generate() without hooks issues it
    split      step_begin / step_sample / step_finish + sync_state per step, no hook: the launches on the stream, the score
               rows written and read back by the sampler
    identity   the same with an identity processor as generate() runs it: per channel a clone of the [B, V] rows and the
               copy back, and the step's tokens appended to a device history
    stream     identity plus a streamer's tokens[:, 0].cpu() and an all-false stop mask per step

Each leg = begin, a real ramp to the target context (unsplit steps), a warm-up, then REPS timed trains of STEPS decode
steps (host clock).  Train i of every leg sits at the same KV lengths, so a train is only compared with the train of the same
index of the plain leg of its cycle.

    python tools/gen_hooks_cost.py --out profiles/gen_hooks_cost.json
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEGS = ("plain", "run_ahead", "split", "identity", "stream")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--context", type=int, default=4096)
    ap.add_argument("--prompt", type=int, default=512)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cycles", type=int, default=2)
    args = ap.parse_args()
    out = measure(args)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({k: v for k, v in out.items() if k != "legs"}, indent=1))


def measure(args):
    sys.path.insert(0, ROOT)
    import numpy as np
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
    hist = torch.zeros((B, L + 64, 8), dtype=torch.int64, device=device)
    no_stop = np.zeros(B, dtype=bool)

    def one_step(leg, cur):
        if leg == "plain":
            eng.step(1)
            return
        s0, s17, _ = eng.step_begin(want_rows=False)
        if leg in ("identity", "stream"):
            for c in range(8):
                view = s0 if c == 0 else s17[:, c - 1]
                view.copy_(view.clone())
        toks = eng.step_sample()
        if leg in ("identity", "stream"):
            hist[:, cur] = toks
        if leg == "stream":
            toks[:, 0].cpu()
            eng.step_finish(no_stop)
        else:
            eng.step_finish()

    legs = []
    for cycle in range(args.cycles):
        for leg in LEGS:
            eng.begin(ids, mask, max_length, layers=layers, do_samples=ds, seed=42)
            done = 0
            while done < ramp:
                n = min(256, ramp - done)
                eng.step(n)
                done += n
                _, fin = eng.sync_state()
                assert not fin
            cur = n_real + ramp
            for _ in range(W):
                one_step("plain" if leg == "run_ahead" else leg, cur)
                eng.sync_state()
                cur += 1
            trains = []
            for _ in range(args.reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                if leg == "run_ahead":
                    eng.step(K)
                    _, fin = eng.sync_state()
                    cur += K
                else:
                    for _ in range(K):
                        one_step(leg, cur)
                        _, fin = eng.sync_state()
                        cur += 1
                trains.append((time.perf_counter() - t0) / K * 1e3)
                assert not fin
            legs.append({"cycle": cycle, "leg": leg, "ms_per_step_trains": trains, "median_ms": statistics.median(trains)})
            print("cycle", cycle, leg, "ms/step", [round(t, 4) for t in trains], flush=True)
            eng.sched_open(B, 16)           # ends the abandoned run
    eng.close()
    out = {"what": "decode step under generate()'s hooks, B=%d at %d tokens of context, sampled; per-step times (host clock) of "
                   "trains of %d steps, compared with the same train of the plain leg of the same cycle" % (B, L, K),
           "legs_mean": {"plain": "unsplit step from its graph, one host round trip per step", "run_ahead": "unsplit steps issued %d at a time" % K,
                         "split": "split step, no hook", "identity": "split step, identity processor on 8 channels, history appended",
                         "stream": "identity + tokens[:, 0].cpu() + an all-false stop mask"},
           "batch": B, "context": L, "steps_per_train": K, "trains_per_leg": args.reps, "cycles": args.cycles, "legs": legs}
    plain = {l["cycle"]: l for l in legs if l["leg"] == "plain"}
    out["median_ms"] = {leg: statistics.median(l["median_ms"] for l in legs if l["leg"] == leg) for leg in LEGS}
    if args.cycles > 1:
        out["plain_leg_to_leg_spread_us"] = max(abs(plain[0]["ms_per_step_trains"][i] - plain[c]["ms_per_step_trains"][i]) * 1e3
                                                for c in range(1, args.cycles) for i in range(args.reps))
    out["minus_plain_us"] = {}
    for leg in LEGS[1:]:
        d = [(l["ms_per_step_trains"][i] - plain[l["cycle"]]["ms_per_step_trains"][i]) * 1e3
             for l in legs if l["leg"] == leg for i in range(args.reps)]
        out["minus_plain_us"][leg] = {"mean": statistics.mean(d), "min": min(d), "max": max(d), "trains": len(d)}
    return out


if __name__ == "__main__":
    main()
