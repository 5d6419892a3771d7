"""Generate the teacher-forced loss fixtures by running the REFERENCE's own forward(labels=...) (CPU, eager).

Run in the build container only (needs the reference checkout, like make_golden.py):
    python tests/golden/make_golden_loss.py [case ...]

What comes from the reference: `AsteroidTTSInstruct.forward(input_ids, attention_mask, labels=..., skip_logits=False)`
(modeling_asteroid.py:337-426): `loss`, `loss_all` and `logits_all`.  `logp_ref[b, t, c]` is taken from the reference's
own logits, `log_softmax(logits_all[c][b, t - 1].float())[labels[b, t, c]]` (the shift and the upcast of transformers'
ForCausalLMLoss), NaN at t = 0 and where the label is -100.  The numpy oracle runs on the same inputs and its two
distances from the reference are stored with the case: `D_oracle` = max |oracle logp - reference logp| and
`D_oracle_loss` = max over channels of the loss difference.  They are the tolerance of the GPU replay
(tests/test_loss_gpu.py): whatever this script measures is what it stores.

Only data is written: inputs, labels, expected values and the (config, seed) that regenerate the weights with mtts.synth.
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
import make_golden as mg  # noqa: E402  (shims + build_reference; puts moss-ttsd_amd on the path)
from mtts import synth  # noqa: E402
from oracle import asteroid_oracle as ao  # noqa: E402

IGNORE = -100
WIDE = dict(hidden_size=2048, intermediate_size=6144, num_attention_heads=16, num_key_value_heads=8)
TORCH_DTYPE = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}

# name -> (cfg overrides, weight kwargs, dtype, seed, T, lengths)
CASES = {
    "loss_ragged_fp32": ({}, {}, "fp32", 811, 200, (200, 130, 9)),
    "loss_ragged_bf16": ({}, {}, "bf16", 811, 200, (200, 130, 9)),
    "loss_ragged_fp16": ({}, {}, "fp16", 811, 200, (200, 130, 9)),
    # peaked logits (up to about 60): one bf16 ulp of a logit is then 0.25
    "loss_peaked_bf16": ({}, dict(emb_row_sigma=1.0), "bf16", 811, 200, (200, 130, 9)),
    # production width: the `ar_wide` layer shape with the full 152 697-row channel-0 table
    "loss_wide_bf16": (WIDE, {}, "bf16", 813, 80, (80, 41)),
}


def synth_batch(cfg, seed, T, lengths):
    """Right-padded (input_ids, attention_mask, labels): per row a text part (channel 0 labelled, channels 1-7 ignored),
    then a speech part, delay-shifted with synth.shifting_inputs; one label in ten is ignored at random."""
    rng = np.random.default_rng(seed)
    B = len(lengths)
    ids = np.full((B, T, 8), synth.SPEECH_PAD, dtype=np.int64)
    ids[:, :, 0] = cfg["pad_token_id"]
    mask = np.zeros((B, T), dtype=np.int64)
    labels = np.full((B, T, 8), IGNORE, dtype=np.int64)
    for b, n in enumerate(lengths):
        m = n - 7
        n_text = max(1, m // 3)
        raw = np.full((m, 8), synth.SPEECH_PAD, dtype=np.int64)
        raw[:n_text, 0] = rng.integers(0, 151643, n_text)
        raw[n_text:, 0] = synth.SPEECH_OFFSET + rng.integers(0, 1024, m - n_text)
        raw[n_text:, 1:] = rng.integers(0, 1024, (m - n_text, 7))
        seq = synth.shifting_inputs(raw, cfg["pad_token_id"])
        lab = seq.copy()
        lab[:n_text, 1:] = IGNORE
        lab[rng.random(lab.shape) < 0.1] = IGNORE
        ids[b, :n] = seq
        labels[b, :n] = lab
        mask[b, :n] = 1
    return ids, mask, labels


def logp_from_logits(logits_all, labels):
    """8 x [B,T,V_c] float -> [B,T,8] float32: log_softmax of position t - 1 at labels[t]; NaN at t = 0 / ignored."""
    B, T, _ = labels.shape
    out = np.full((B, T, 8), np.nan, dtype=np.float32)
    lab = torch.from_numpy(labels)
    for c, lg in enumerate(logits_all):
        lsm = torch.log_softmax(torch.as_tensor(lg).float()[:, :-1], dim=-1)          # [B,T-1,V]
        tgt = lab[:, 1:, c]
        got = lsm.gather(-1, tgt.clamp_min(0)[..., None])[..., 0].numpy()
        keep = (tgt != IGNORE).numpy()
        out[:, 1:, c][keep] = got[keep]
    return out


def losses_from_logp(logp):
    """[B,T,8] -> float64 [8]: -(mean over the non-NaN slots) per channel (NaN for a channel without a label)."""
    with np.errstate(invalid="ignore"), __import__("warnings").catch_warnings():
        __import__("warnings").simplefilter("ignore")
        return -np.nanmean(logp.astype(np.float64).reshape(-1, 8), axis=0)


def make_case(name):
    co, wkw, dtype, seed, T, lengths = CASES[name]
    cfg = synth.tiny(**co)
    w = synth.synth_weights(cfg, seed, bf16=(dtype == "bf16"), **wkw)
    model = mg.build_reference(cfg, w, TORCH_DTYPE[dtype])
    ids, mask, labels = synth_batch(cfg, seed + 1, T, lengths)
    with torch.no_grad():
        out = model(input_ids=torch.from_numpy(ids), attention_mask=torch.from_numpy(mask), labels=torch.from_numpy(labels),
                    skip_logits=False, return_dict=True)
    loss_all = out.loss_all.float().numpy()
    logp_ref = logp_from_logits(out.logits_all, labels)
    orc = ao.AsteroidOracle(cfg, w, dtype)
    pos = np.broadcast_to(np.arange(T), (len(lengths), T))
    logp_orc = logp_from_logits(orc.forward(ids, pos, mask, all_positions=True), labels)
    assert np.array_equal(np.isnan(logp_orc), np.isnan(logp_ref))
    d_oracle = float(np.nanmax(np.abs(logp_orc.astype(np.float64) - logp_ref.astype(np.float64))))
    d_loss = float(np.max(np.abs(losses_from_logp(logp_orc) - loss_all.astype(np.float64))))
    d = dict(cfg=json.dumps(cfg), wkw=json.dumps(wkw), seed=seed, dtype=dtype, input_ids=ids, attention_mask=mask, labels=labels,
             loss=np.float32(float(out.loss)), loss_all=loss_all, logp_ref=logp_ref, D_oracle=d_oracle, D_oracle_loss=d_loss,
             transformers_version=__import__("transformers").__version__)
    np.savez_compressed(os.path.join(HERE, name + ".npz"), **d)
    coh = float(np.max(np.abs(losses_from_logp(logp_ref) - loss_all.astype(np.float64))))
    print(f"{name}: loss={float(out.loss):.6f} slots={int(np.isfinite(logp_ref).sum())} max|logit|="
          f"{max(float(torch.as_tensor(l).float().abs().max()) for l in out.logits_all):.1f} D_oracle={d_oracle:.3g} "
          f"D_oracle_loss={d_loss:.3g} |loss_all + nanmean(logp_ref)|={coh:.2g}")


if __name__ == "__main__":
    torch.manual_seed(0)
    torch.set_num_threads(8)
    for name in (sys.argv[1:] or list(CASES)):
        make_case(name)
