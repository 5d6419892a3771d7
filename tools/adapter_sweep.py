"""Which LoRA checkpoint is best?  A fine-tune run (reference finetune/finetune.py with --lora) leaves `checkpoint-N/`
directories that hold an adapter each and no validation loss (the reference trains with eval_dataset=None).  This scores
every one of them on a held-out set, on ONE resident engine: the base model is loaded once, and each checkpoint is a
load_adapter() -- a merge-and-pack pass over the projection weights -- followed by forward(labels=...).

    python tools/adapter_sweep.py --base /models/MOSS-TTSD-v0.5 --data out/val --checkpoints out/run/checkpoint-*

--data: an output directory of moss-ttsd_amd/finetune/data_preprocess.py (every <name>.pkl with its <name>_metas.npy).
Rows are delay-shifted with mtts.synth.shifting_inputs, labels the same way with -100 as the fill (what the fine-tune
dataset does), and right-padded per batch as forward(labels) expects.  Prints one JSON line per checkpoint (and "base"
first): loss, loss_all[8] over the whole set (sums and counts are combined across batches), seconds the swap took.
"""
import argparse
import glob
import json
import os
import pickle
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "moss-ttsd_amd"))


def load_rows(data_dir, pad_token_id, max_tokens):
    """-> list of (ids [T, 8], labels [T, 8]) int64, delay-shifted, cut to max_tokens."""
    from mtts import synth
    rows = []
    for pkl in sorted(glob.glob(os.path.join(data_dir, "*.pkl"))):
        offsets = np.load(pkl[:-len(".pkl")] + "_metas.npy")[0]
        with open(pkl, "rb") as f:
            for off in offsets:
                f.seek(int(off))
                e = pickle.load(f)
                ids, lab = (np.asarray(e[k], dtype=np.int64)[:, :synth.CHANNELS] for k in ("input_ids", "labels"))
                rows.append((synth.shifting_inputs(ids, pad_token_id)[:max_tokens],
                             synth.shifting_inputs(lab, -100, pad_token=-100)[:max_tokens]))
    if not rows:
        raise FileNotFoundError(f"no <name>.pkl with <name>_metas.npy under {data_dir}")
    return rows


def batches(rows, batch, pad_token_id):
    """Right-padded batches, longest rows first (less padding): ids [B, T, 8], mask [B, T], labels [B, T, 8]."""
    from mtts import synth
    order = sorted(range(len(rows)), key=lambda i: -rows[i][0].shape[0])
    for b0 in range(0, len(order), batch):
        part = [rows[i] for i in order[b0:b0 + batch]]
        T = max(r[0].shape[0] for r in part)
        ids = np.full((len(part), T, synth.CHANNELS), synth.SPEECH_PAD, dtype=np.int64)
        ids[:, :, 0] = pad_token_id
        lab = np.full(ids.shape, -100, dtype=np.int64)
        mask = np.zeros((len(part), T), dtype=np.uint8)
        for j, (i, l) in enumerate(part):
            ids[j, :i.shape[0]], lab[j, :i.shape[0]], mask[j, :i.shape[0]] = i, l, 1
        yield ids, mask, lab


def evaluate(model, rows, batch, pad_token_id):
    import torch
    sums, counts = np.zeros(8), np.zeros(8, dtype=np.int64)
    for ids, mask, lab in batches(rows, batch, pad_token_id):
        lp = model(input_ids=torch.from_numpy(ids), attention_mask=torch.from_numpy(mask), labels=torch.from_numpy(lab)).token_logprobs.numpy()
        ok = ~np.isnan(lp)
        sums += np.where(ok, lp, 0).astype(np.float64).sum(axis=(0, 1))
        counts += ok.sum(axis=(0, 1))
    with np.errstate(invalid="ignore", divide="ignore"):
        loss_all = -(sums / counts)
    w = np.asarray(model.weights, dtype=np.float64)
    return float((loss_all * w / w.sum()).sum()), [float(x) for x in loss_all]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--base", required=True, help="base model directory (config.json + *.safetensors)")
    ap.add_argument("--data", required=True, help="data_preprocess.py output directory")
    ap.add_argument("--checkpoints", nargs="+", required=True, help="PEFT checkpoint directories")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--max-tokens", type=int, default=16000, help="rows are cut here, as the fine-tune collator cuts them")
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp16", "fp32"])
    args = ap.parse_args()
    import torch
    import modeling_asteroid as ma
    model = ma.AsteroidTTSInstruct.from_pretrained(args.base, torch_dtype={"bf16": torch.bfloat16, "fp16": torch.float16,
                                                                           "fp32": torch.float32}[args.dtype]).eval().to("cuda")
    pad = model.config.pad_token_id
    rows = load_rows(args.data, pad, args.max_tokens)
    loss, loss_all = evaluate(model, rows, args.batch, pad)
    print(json.dumps({"checkpoint": "base", "loss": loss, "loss_all": loss_all, "rows": len(rows)}), flush=True)
    best = None
    for ck in args.checkpoints:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        model.load_adapter(ck)
        torch.cuda.synchronize()
        swap = time.perf_counter() - t0               # reading the file included
        loss, loss_all = evaluate(model, rows, args.batch, pad)
        print(json.dumps({"checkpoint": ck, "loss": loss, "loss_all": loss_all, "swap_s": swap}), flush=True)
        if best is None or loss < best[0]:
            best = (loss, ck)
    print(json.dumps({"best": best[1], "loss": best[0]}))


if __name__ == "__main__":
    main()
