"""What forward(top_logprobs=k) adds to teacher-forced scoring, at the assumed 1.7B dims: Engine.score on B x T tokens
(default 8 x 256: one prefill pass of 2048 rows) with top_k in {0, 1, 8, 16}.

Records
  * the wall time of the whole call (host clock around Engine.score, which is synchronous; a sample is --inner calls) and
    the time of the scoring kernels alone (profile slot 4: hipEvents around the head launches of every pass), the
    variants INTERLEAVED round by round, after one warm-up call each that also pays the first-use allocations; the
    ratio of every top_k to top_k = 0, and slot 4's share of the call;
  * with --parent-lib (a libmtts.so built from the parent commit, loaded next to this tree's into the same process, an
    engine of its own with the same weights): top_k = 0 against the parent's score in alternating pairs, the spread of
    the parent against itself from one round to the next, and whether the two return the same bits.

    python tools/score_topk_bench.py --out out/score_topk.json [--parent-lib /path/to/parent/libmtts.so]

Results: profiles/score_topk.json.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KS = (0, 1, 8, 16)


def _load_lib(path, sigs):
    """Another build of the library, with the prototypes of the symbols it has (dlopen'ed RTLD_LOCAL: its own globals)."""
    L = C.CDLL(path)
    for name, (res, args) in sigs.items():
        fn = getattr(L, name, None)
        if fn is not None:
            fn.restype, fn.argtypes = res, args
    return L


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--tokens", type=int, default=256)
    ap.add_argument("--layers", type=int, default=0, help="0: the config's 28")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--inner", type=int, default=4, help="calls per timed sample")
    ap.add_argument("--parent-lib", default=None)
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

    def engine(lib=None):
        saved = capi.lib()
        if lib is not None:
            capi._lib = lib                        # Engine keeps the library it was created with
        try:
            eng = Engine(cfg, max_batch=B, max_seq_len=T, device=str(device))
        finally:
            if lib is not None:
                capi._lib = saved
        for name, t in bench.make_weights_on_device(cfg, 1234, device, 0, 1):
            eng.bind(name, t)
            del t
        assert eng.lib.mtts_weights_ready(eng._h) == 0
        return eng

    eng = engine()
    parent = engine(_load_lib(args.parent_lib, capi._SIGS)) if args.parent_lib else None
    rng = np.random.default_rng(5)
    ids = np.full((B, T, 8), 1024, dtype=np.int64)
    ids[:, :, 0] = synth.SPEECH_OFFSET + rng.integers(0, 1024, (B, T))
    ids[:, :, 1:] = rng.integers(0, 1024, (B, T, 7))
    mask = np.ones((B, T), dtype=np.uint8)
    labels = ids.copy()

    def call(e, k):
        return e.score(ids, mask, labels, top_k=k) if k else e.score(ids, mask, labels)

    def sample(e, k):
        """-> (wall seconds per call, slot-4 ms per call) over --inner calls; the events are on in both, for every variant"""
        ms0 = e.profile_read(4)[0]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.inner):
            call(e, k)
        wall = (time.perf_counter() - t0) / args.inner
        return wall, (e.profile_read(4)[0] - ms0) / args.inner

    # warm-up, and what must not change: the labels' log-probabilities are the same bits in every variant
    first = {k: call(eng, k) for k in KS}
    lp0 = first[0]
    assert np.isfinite(lp0[:, 1:]).all()
    for k in KS[1:]:
        assert np.array_equal(first[k][0].view(np.uint32), lp0.view(np.uint32))
        assert np.array_equal(first[k][1], first[16][1][..., :k]) and (first[k][1][:, 1:] >= 0).all()
    same_as_parent = None
    if parent is not None:
        same_as_parent = bool(np.array_equal(call(parent, 0).view(np.uint32), lp0.view(np.uint32)))
        parent.profile(True)
    eng.profile(True)
    variants = [("k%d" % k, eng, k) for k in KS] + ([("parent", parent, 0)] if parent is not None else [])
    wall = {n: [] for n, _, _ in variants}
    slot4 = {n: [] for n, _, _ in variants}
    for r in range(args.rounds):
        order = variants[r % len(variants):] + variants[:r % len(variants)]       # no variant always follows the same one
        for n, e, k in order:
            w, s = sample(e, k)
            wall[n].append(w)
            slot4[n].append(s)
    eng.close()
    if parent is not None:
        parent.close()

    med = statistics.median
    out = {
        "config": {k: cfg[k] for k in ("hidden_size", "intermediate_size", "num_hidden_layers", "num_attention_heads",
                                       "num_key_value_heads", "vocab_size", "speech_vocab_size")},
        "batch": B, "tokens_per_sequence": T, "rounds": args.rounds, "calls_per_sample": args.inner,
        "wall_s_per_call": wall, "slot4_ms_per_call": slot4,
        "median": {n: {"wall_s": med(wall[n]), "slot4_ms": med(slot4[n]), "slot4_share_of_call": med(slot4[n]) * 1e-3 / med(wall[n])}
                   for n in wall},
        "ratio_to_top_k_0": {"k%d" % k: {"wall": med(wall["k%d" % k]) / med(wall["k0"]), "slot4": med(slot4["k%d" % k]) / med(slot4["k0"])}
                             for k in KS[1:]},
    }
    if parent is not None:
        def spread(key):
            pairs = [a / b for a, b in zip(key["k0"], key["parent"])]                          # this tree over the parent, round by round
            own = [a / b for a, b in zip(key["parent"][1:], key["parent"][:-1])]               # the parent over itself, next round
            own += [1 / x for x in own]
            return {"k0_over_parent_per_round": pairs, "k0_over_parent_median": med(pairs),
                    "parent_over_parent_next_round": own, "parent_spread": [min(own), max(own)],
                    "inside_parent_spread": bool(min(own) <= med(pairs) <= max(own))}
        out["top_k_0_against_parent"] = {"same_bits": same_as_parent, "wall": spread(wall), "slot4": spread(slot4)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v for k, v in out.items() if k not in ("wall_s_per_call", "slot4_ms_per_call")}, indent=1))


if __name__ == "__main__":
    main()
