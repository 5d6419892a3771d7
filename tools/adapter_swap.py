"""What swapping a LoRA adapter on a resident engine costs, at the assumed 1.7B dims (28 layers, 196 projection matrices,
1.41 G weights: 2.8 GB read and 2.8 GB written per swap).

Records, for a synthetic adapter on all seven modules of every layer at each --ranks value (device-resident fp32 tensors)
  * wall time of model.load_adapter and model.unload_adapter, synchronised (host clock; --reps repeats after one warm-up);
  * beside them the parent's way of changing the 196 matrices of a resident engine: mtts_bind_weight over already-merged
    device tensors (the base tensors stand in: same bytes), once as Engine.bind issues it (a synchronise per matrix; this
    is also what unload_adapter does) and once as a bare train of calls with one synchronise at the end;
  * lora_pack_kernel alone on gate_proj (6144 x 2048) against pack_weight_kernel alone on the same matrix: device events
    around a train of --iters mtts_bind_weight_lora / mtts_bind_weight calls on one stream.

    python tools/adapter_swap.py --out out/adapter_swap.json

Results: profiles/adapter_swap.json.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _stats(v):
    return {"min_s": min(v), "mean_s": sum(v) / len(v), "max_s": max(v), "all_s": v}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--ranks", type=int, nargs="+", default=[16, 64])
    ap.add_argument("--layers", type=int, default=0, help="0: the config's 28")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    import bench                                   # (puts the package on sys.path)
    import modeling_asteroid as ma
    from mtts import adapters, capi, synth

    device = torch.device("cuda:0")
    torch.cuda.set_device(device)
    cfg = synth.assumed_1p7b()
    if args.layers:
        cfg["num_hidden_layers"] = args.layers
    sd = dict(bench.make_weights_on_device(cfg, 1234, device, 0, 1))
    model = ma.AsteroidTTSInstruct.from_state_dict(cfg, sd).eval().to(device)
    eng = model._get_engine(1, 256)
    proj = [f"model.language_model.layers.{n}.{p}.weight" for n in range(cfg["num_hidden_layers"]) for p in adapters.PROJECTIONS]
    weights = sum(sd[k].numel() for k in proj)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    out = {"config": {k: cfg[k] for k in ("hidden_size", "intermediate_size", "num_hidden_layers", "num_attention_heads", "num_key_value_heads")},
           "matrices": len(proj), "projection_weights": weights, "bytes_read_plus_written_per_swap": 4 * weights, "reps": args.reps,
           "swap": {}}
    g = torch.Generator(device=device)
    g.manual_seed(7)
    for r in args.ranks:
        ad = {k: (0.02 * torch.randn((r, sd[k].shape[1]), device=device, generator=g),
                  0.02 * torch.randn((sd[k].shape[0], r), device=device, generator=g)) for k in proj}
        scaling = float(np.float32(32 / np.sqrt(r)))
        timed(lambda: model.load_adapter(ad, scaling=scaling))          # warm-up: code objects
        timed(model.unload_adapter)
        loads, unloads = [], []
        for _ in range(args.reps):
            loads.append(timed(lambda: model.load_adapter(ad, scaling=scaling)))
            unloads.append(timed(model.unload_adapter))
        out["swap"][f"r{r}"] = {"adapter_parameters": sum(a.numel() + b.numel() for a, b in ad.values()),
                                "load_adapter": _stats(loads), "unload_adapter": _stats(unloads),
                                "load_adapter_GBps": 4 * weights / min(loads) / 1e9}
        del ad

    # the parent's way: mtts_bind_weight over already-merged device tensors
    lib = capi.lib()

    def bind_train():
        for k in proj:
            capi.check(lib.mtts_bind_weight(eng._h, k.encode(), sd[k].data_ptr(), sd[k].shape[0], sd[k].shape[1], None))

    def bind_each():
        for k in proj:
            eng.bind(k, sd[k])

    timed(bind_train)
    out["parent_rebind_merged"] = {"engine_bind_sync_per_matrix": _stats([timed(bind_each) for _ in range(args.reps)]),
                                   "bare_calls_one_sync": _stats([timed(bind_train) for _ in range(args.reps)])}

    # the two kernels alone on gate_proj
    k = "model.language_model.layers.0.mlp.gate_proj.weight"
    w = sd[k]
    kern = {"matrix": list(w.shape), "iters": args.iters}

    def train(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        fn()
        torch.cuda.synchronize()
        e0.record()
        for _ in range(args.iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / args.iters

    kern["pack_weight_kernel_ms"] = train(lambda: capi.check(lib.mtts_bind_weight(eng._h, k.encode(), w.data_ptr(), w.shape[0], w.shape[1], None)))
    for r in args.ranks:
        a = 0.02 * torch.randn((r, w.shape[1]), device=device, generator=g)
        b = 0.02 * torch.randn((w.shape[0], r), device=device, generator=g)
        kern[f"lora_pack_kernel_r{r}_ms"] = train(lambda: capi.check(lib.mtts_bind_weight_lora(
            eng._h, k.encode(), w.data_ptr(), w.shape[0], w.shape[1], a.data_ptr(), b.data_ptr(), r, C.c_float(2.0), None)))
        kern[f"lora_pack_kernel_r{r}_GBps"] = 4 * w.numel() / kern[f"lora_pack_kernel_r{r}_ms"] / 1e6
    kern["pack_weight_kernel_GBps"] = 4 * w.numel() / kern["pack_weight_kernel_ms"] / 1e6
    out["gate_proj_kernels"] = kern
    eng.bind(k, w)
    eng.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
