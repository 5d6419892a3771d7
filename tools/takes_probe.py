"""Takes on shared KV pages against the repeat-interleaved batch, at the assumed 1.7B dims (synthetic weights).

8 prompts of 2 000 real tokens, 4 takes each = 32 rows, on ONE engine, alternating forked (begin(takes=4)) and expanded
(begin of the repeat-interleaved batch) runs A/B/A/B.  Per run: begin() wall time (synchronised), pages in use after
begin, decode ms/step over 64 steps at a KV length of ~2.1 k and ~4 k (sealed reads as in bench.py: no
MTTS_KV_PACK_MIN override).  The forked and expanded runs must generate the same tokens (checked on the first pair).

    python tools/takes_probe.py --out profiles/takes_probe.json
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/takes_probe.py --fork-only      (fork kernel time, own run)
    python tools/takes_probe.py --out profiles/takes_probe.json --merge-stats DIR/..._results.db
"""
import argparse
import json
import os
import sqlite3
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "moss-ttsd_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

PROMPTS, REAL, TAKES = 8, 2000, 4
KV_POINTS = (2064, 4008)          # KV length at the start of each timed window of 64 steps
TIMED = 64


def merge_stats(out, db_path):
    """fork_kernel's dispatches from a rocprofv3 rocpd database (sqlite, as tools/rocpd_stats.py reads it)."""
    db = sqlite3.connect(db_path)
    tabs = [r[0] for r in db.execute("select name from sqlite_master where type='table'")]
    kd = [x for x in tabs if x.startswith("rocpd_kernel_dispatch")][0]
    ks = [x for x in tabs if x.startswith("rocpd_info_kernel_symbol")][0]
    cols = [r[1] for r in db.execute(f"pragma table_info({ks})")]
    name = "display_name" if "display_name" in cols else "kernel_name"
    durs = [r[0] for r in db.execute(f"select d.end - d.start from {kd} d join {ks} s on d.kernel_id = s.id "
                                     f"where s.{name} like 'fork_kernel%'")]
    res = json.load(open(out)) if os.path.exists(out) else {}
    moved = res.get("fork_bytes_each_way", 0)
    avg_us = sum(durs) / len(durs) / 1e3
    res["fork_kernel_rocprofv3"] = dict(
        how="rocprofv3 --kernel-trace --stats, a run of its own (tools/takes_probe.py --fork-only: three forked begins)",
        calls=len(durs), avg_us=avg_us, min_us=min(durs) / 1e3, max_us=max(durs) / 1e3,
        GBps_read_plus_write=round(2 * moved / (avg_us * 1e-6) / 1e9, 1) if moved else None)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res["fork_kernel_rocprofv3"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/takes_probe.json")
    ap.add_argument("--fork-only", action="store_true", help="three forked begins and nothing else (kernel trace run)")
    ap.add_argument("--merge-stats", default=None, help="rocprofv3 database of a --fork-only run: add the fork kernel's time")
    ap.add_argument("--reps", type=int, default=2, help="A/B pairs")
    args = ap.parse_args()
    if args.merge_stats:
        return merge_stats(args.out, args.merge_stats)

    import numpy as np
    import torch
    from bench import make_weights_on_device
    from mtts import capi, synth
    from mtts.engine import Engine

    cfg = synth.assumed_1p7b()
    device = torch.device("cuda:0")
    torch.cuda.set_device(device)
    R = PROMPTS * TAKES
    eng = Engine(cfg, max_batch=R, max_seq_len=4288, device="cuda:0")
    for name, t in make_weights_on_device(cfg, 1234, device, 0, 1):
        eng.bind(name, t)
        del t
    capi.check(eng.lib.mtts_weights_ready(eng._h))
    ids, mask = synth.synth_prompts(cfg, 77, PROMPTS, REAL + 7, audio_frac=0.5, ragged=False)
    ex_ids, ex_mask = np.repeat(ids, TAKES, 0), np.repeat(mask, TAKES, 0)
    base = ids.shape[1] - 7
    max_length = base + 2200
    layers = [dict(top_k=50, top_p=0.95, temperature=1.0, repetition_penalty=1.0)] * 8
    total = eng.kv_pool_state()[0]

    def begin(forked):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if forked:
            eng.begin(ids, mask, max_length, layers=layers, do_samples=[True] * 8, seed=42, takes=TAKES)
        else:
            eng.begin(ex_ids, ex_mask, max_length, layers=layers, do_samples=[True] * 8, seed=42)
        eng.sync_state()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    if args.fork_only:
        for _ in range(3):
            begin(True)
        print("fork-only: 3 forked begins")
        return

    runs = []
    first_tokens = {}
    for rep in range(args.reps):
        for forked in (True, False):
            r = dict(variant="forked" if forked else "expanded", rep=rep)
            r["begin_s"] = begin(forked)
            r["pages_in_use"] = total - eng.kv_pool_state()[1]
            steps = 0
            for kv in KV_POINTS:
                while base + steps < kv:
                    n = min(256, kv - base - steps)
                    eng.step(n)
                    steps += n
                    _, fin = eng.sync_state()
                    assert not fin
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                eng.step(TIMED)
                st, fin = eng.sync_state()
                torch.cuda.synchronize()
                r[f"ms_per_step_kv{kv}"] = (time.perf_counter() - t0) * 1e3 / TIMED
                steps += TIMED
                assert st == steps and not fin, (st, steps, fin)
            if rep == 0:
                first_tokens[forked] = eng.read_generated(steps + 8)
            runs.append(r)
            print(json.dumps(r), flush=True)
    same = bool(np.array_equal(first_tokens[True], first_tokens[False]))

    def stat(variant, key):
        v = [r[key] for r in runs if r["variant"] == variant]
        return dict(mean=float(np.mean(v)), min=float(np.min(v)), max=float(np.max(v)), runs=v)

    blk = 64 * cfg["head_dim"] * 2                      # one (layer, kv head) page block, bf16
    tails = PROMPTS * (TAKES - 1) if REAL % 64 else 0
    res = dict(
        what="forked begin(takes=4) vs the repeat-interleaved batch on one engine, alternated A/B/A/B",
        dims="assumed 1.7B (synth.assumed_1p7b), synthetic weights (bench.make_weights_on_device)",
        prompts=PROMPTS, real_tokens=REAL, takes=TAKES, rows=R, kv_pool_pages=total,
        pages_expected=dict(forked=PROMPTS * -(-REAL // 64) + tails, expanded=R * -(-REAL // 64)),
        tokens_identical=same,
        fork_tail_pages=tails,
        fork_bytes_each_way=tails * cfg["num_hidden_layers"] * cfg["num_key_value_heads"] * 2 * blk,
        runs=runs,
        summary={k: dict(forked=stat("forked", k), expanded=stat("expanded", k))
                 for k in ["begin_s", "pages_in_use"] + [f"ms_per_step_kv{kv}" for kv in KV_POINTS]},
        device=torch.cuda.get_device_name(0),
    )
    b = res["summary"]["begin_s"]
    res["begin_ratio_forked_over_expanded"] = b["forked"]["mean"] / b["expanded"]["mean"]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(dict(begin_ratio=res["begin_ratio_forked_over_expanded"], tokens_identical=same,
                          pages={k: res["summary"]["pages_in_use"][k]["mean"] for k in ("forked", "expanded")})))
    eng.close()


if __name__ == "__main__":
    main()
