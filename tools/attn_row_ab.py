"""A/B of the whole-row decode attention kernel (csrc/attn.hip: attn_row_kernel, one launch per layer) against the launches
it replaces (attn_scores + attn_pv + attn_combine), as trains of back-to-back launches through mtts_k_attn_bench
(phase 0 = the three launches in a row, phase 4 = the row kernel) at the bench's width, alternating A/B/A/B in one process
(tuning aid, GPU box only).  Both trains run the fused q/k/v epilogue and read sealed pages.

Cells: batch x context with every row at the same length (the context is reached with mtts_debug_set_kv_len: random
page contents, all sealed), and one ragged cell (32 real prompts of 1 k .. 4 k tokens, prefilled).  The engine has
`--layers` layers (default 12) so that a train cycles over more K/V bytes than the Infinity Cache holds in every cell.

  python tools/attn_row_ab.py --out profiles/attn_row_ab.json [--legs 4] [--cells 32:4096,16:1024] [--lib other/libmtts.so]

`--lib` times another build of the library (a ROW_WAVES variant built with MTTS_BUILD_FLAGS=-DROW_WAVES=N)."""
import argparse
import json
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "moss-ttsd_amd"))

SWEEP = [(b, c) for c in (1024, 4096) for b in (16, 24, 32, 48, 64)]


def weights(synth, cfg, seed, torch):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    for name, shape, kind in synth.weight_shapes(cfg):
        if kind == "norm":
            yield name, (1.0 + 0.1 * torch.randn(shape, device="cuda", generator=g)).to(torch.bfloat16)
        else:
            yield name, (0.02 * torch.randn(shape, device="cuda", generator=g)).to(torch.bfloat16)


def trains(eng, legs, iters):
    two, row, parts = [], [], {}
    for ph, nm in ((1, "scores"), (2, "pv"), (3, "combine")):
        parts[nm + "_us"] = round(eng.attn_bench(ph, iters)[0] * 1e3, 2)
    by = 0
    for _ in range(legs):
        ms, by = eng.attn_bench(0, iters)
        two.append(round(ms * 1e3, 2))
        ms, by = eng.attn_bench(4, iters)
        row.append(round(ms * 1e3, 2))
    mean = lambda v: sum(v) / len(v)
    res = dict(parts, two_pass_us=two, row_us=row, two_pass_mean=round(mean(two), 2), row_mean=round(mean(row), 2),
               two_pass_spread=round(max(two) - min(two), 2), row_spread=round(max(row) - min(row), 2), kv_bytes=by,
               row_gbs=round(by / mean(row) / 1e3, 1), two_pass_gbs=round(by / mean(two) / 1e3, 1))
    # the project's criterion: every B run below every A run, means apart by twice A's spread
    res["row_wins"] = bool(max(row) < min(two) and mean(two) - mean(row) >= 2 * (max(two) - min(two)))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--legs", type=int, default=4)
    ap.add_argument("--layers", type=int, default=12)
    ap.add_argument("--cells", default=None, help="B:context,... (default: the sweep + the ragged cell)")
    ap.add_argument("--no-ragged", action="store_true")
    ap.add_argument("--lib", default=None)
    args = ap.parse_args()
    from mtts import capi
    if args.lib:
        capi.LIB_PATH = os.path.abspath(args.lib)
    import numpy as np
    import torch
    from mtts import synth
    from mtts.engine import Engine
    cells = [tuple(int(x) for x in c.split(":")) for c in args.cells.split(",")] if args.cells else SWEEP
    cfg = synth.assumed_1p7b()
    cfg["num_hidden_layers"] = args.layers
    iters = 8 * args.layers
    maxb = max([b for b, _ in cells] + [32])
    eng = Engine(cfg, max_batch=maxb, max_seq_len=max([c for _, c in cells] + [4096]) + 128)
    for name, t in weights(synth, cfg, 5, torch):
        eng.bind(name, t)
    layers = [dict(top_k=50, top_p=0.95, temperature=1.0, repetition_penalty=1.0)] * 8
    out = {"lib": args.lib or "default", "layers": args.layers, "iters_per_train": iters, "legs": args.legs, "cells": {}}
    for B, ctx in cells:
        ids, mask = synth.synth_prompts(cfg, 77, B, 40, audio_frac=0.5, ragged=False)
        eng.begin(ids, mask, ids.shape[1] + ctx + 64, layers=layers, do_samples=[True] * 8, seed=42)
        eng.sync_state()
        eng.debug_set_kv_len(ctx - 2)
        eng.step(1)                      # the rows' metadata of a decode step at this length
        eng.sync_state()
        res = trains(eng, args.legs, iters)
        out["cells"]["B%d_ctx%d" % (B, ctx)] = res
        print(B, ctx, res, file=sys.stderr, flush=True)
    if not args.no_ragged:
        lens = [int(x) for x in np.linspace(1024, 4000, 32)]
        seqs = [synth.synth_prompts(cfg, 300 + i, 1, n, 0.4, False)[0][0] for i, n in enumerate(lens)]
        ids, mask = synth.left_pad(seqs, cfg["pad_token_id"])
        eng.begin(ids, mask, ids.shape[1] + 72, layers=layers, do_samples=[True] * 8, seed=42)
        eng.step(1)
        eng.sync_state()
        res = trains(eng, args.legs, iters)
        out["cells"]["B32_ragged_1k_4k"] = res
        print("ragged", res, file=sys.stderr, flush=True)
    eng.close()
    s = json.dumps(out, indent=1)
    if args.out:
        with open(args.out, "w") as f:
            f.write(s + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
