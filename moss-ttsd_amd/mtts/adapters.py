"""PEFT LoRA adapter checkpoints for the HIP engine: the reader, and the merge as numpy states it.

The reference's documented fine-tune is LoRA on the seven projections of every layer (finetune/lora_config.yaml,
finetune/finetune.py:146-176), saved every few steps as `checkpoint-N/{adapter_config.json, adapter_model.bin |
adapter_model.safetensors}`; its end state is `model.merge_and_unload()` (finetune.py:237).  The engine does that merge
on the device, per matrix, on the way into its weight layout (csrc/adapter.hip, mtts_bind_weight_lora).  This module
holds what is host work: reading such a directory (`read_peft_dir`), and `merge_spec`, the definition of the merged
matrix in numpy float32 -- the tests compare the device against it bit for bit; nothing on the product path calls it.

What is PEFT's and what is this project's: `(B @ A) * scaling` in fp32 added to the base weight with ONE rounding of the
fp32 sum to the model dtype is PEFT's merge for fp32 adapter weights on a half-precision base (its default,
autocast_adapter_dtype; torch's in-place `bf16 += fp32` rounds once).  The order of the r-term sum -- ascending j, a
multiply and an add per term, no fma -- is this project's choice: a BLAS matmul fixes no order.
"""
from __future__ import annotations

import json
import math
import os
import re

import numpy as np

from . import synth

PROJECTIONS = ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.o_proj",
               "mlp.gate_proj", "mlp.up_proj", "mlp.down_proj")
MAX_RANK = 256
_KEY = re.compile(r"^base_model\.model\.(?P<mod>.+)\.lora_(?P<ab>[AB])(?:\.default)?\.weight$")
_MOD = re.compile(r"^model\.language_model\.layers\.(?P<layer>\d+)\.(?P<proj>.+)$")


def _cfg_get(cfg, k):
    return cfg[k] if isinstance(cfg, dict) else getattr(cfg, k)


def projection_shape(model_cfg, proj):
    """[out, in] of a layer's projection weight."""
    H, I = _cfg_get(model_cfg, "hidden_size"), _cfg_get(model_cfg, "intermediate_size")
    D = _cfg_get(model_cfg, "head_dim")
    q, kv = _cfg_get(model_cfg, "num_attention_heads") * D, _cfg_get(model_cfg, "num_key_value_heads") * D
    return {"self_attn.q_proj": (q, H), "self_attn.k_proj": (kv, H), "self_attn.v_proj": (kv, H), "self_attn.o_proj": (H, q),
            "mlp.gate_proj": (I, H), "mlp.up_proj": (I, H), "mlp.down_proj": (H, I)}[proj]


def scaling_of(config):
    """lora_alpha / sqrt(r) with use_rslora, else lora_alpha / r (peft LoraLayer.update_layer), as one fp32 value."""
    r, alpha = int(config["r"]), float(config["lora_alpha"])
    return float(np.float32(alpha / math.sqrt(r) if config.get("use_rslora") else alpha / r))


def check_tensors(tensors, model_cfg=None, rank=None):
    """{engine weight name: (A [r, in], B [out, r])} as the engine takes it: projection weights of existing layers, the
    weight's shape (with `model_cfg`), one rank 1..256 per matrix (`rank`: the one every matrix must have).  ValueError
    names what is wrong."""
    for name, (A, B) in tensors.items():
        mod = name[:-len(".weight")] if name.endswith(".weight") else None
        m = _MOD.match(mod) if mod else None
        if not m or m.group("proj") not in PROJECTIONS:
            raise ValueError(f"adapter target {name!r} is not one of the seven projection weights of a layer "
                             f"({', '.join(p.split('.')[1] for p in PROJECTIONS)})")
        if A.ndim != 2 or B.ndim != 2 or A.shape[0] != B.shape[1]:
            raise ValueError(f"{name}: lora_A {tuple(A.shape)} and lora_B {tuple(B.shape)} are not [r, in] and [out, r]")
        r = int(A.shape[0])
        if not 1 <= r <= MAX_RANK:
            raise ValueError(f"{name}: rank {r} is outside 1..{MAX_RANK}")
        if rank is not None and r != rank:
            raise ValueError(f"{name}: the tensors have rank {r} but adapter_config.json says r = {rank}")
        if model_cfg is not None:
            if int(m.group("layer")) >= _cfg_get(model_cfg, "num_hidden_layers"):
                raise ValueError(f"{name}: layer index {m.group('layer')} is past the model's "
                                 f"{_cfg_get(model_cfg, 'num_hidden_layers')} layers")
            out, inn = projection_shape(model_cfg, m.group("proj"))
            if (int(B.shape[0]), int(A.shape[1])) != (out, inn):
                raise ValueError(f"{name}: adapter is for a [{int(B.shape[0])}, {int(A.shape[1])}] weight, the model's is [{out}, {inn}]")


def _refuse(config):
    if config.get("peft_type") != "LORA":
        raise ValueError(f"adapter_config.json: peft_type = {config.get('peft_type')!r}: only LORA adapters can be merged")
    if config.get("use_dora"):
        raise ValueError("adapter_config.json: use_dora is set: DoRA's magnitude vectors are not a low-rank update")
    if config.get("bias", "none") != "none":
        raise ValueError(f"adapter_config.json: bias = {config['bias']!r}: the engine's projections have no bias to train")
    if config.get("fan_in_fan_out"):
        raise ValueError("adapter_config.json: fan_in_fan_out is set: the weights would be stored transposed")
    for k in ("modules_to_save", "rank_pattern", "alpha_pattern"):
        if config.get(k):
            raise ValueError(f"adapter_config.json: {k} = {config[k]!r} is not supported (one rank and alpha, adapters only)")
    for k in ("r", "lora_alpha"):
        if config.get(k) is None:
            raise ValueError(f"adapter_config.json: {k} is missing")


def _load_tensors(path):
    st, pt = os.path.join(path, "adapter_model.safetensors"), os.path.join(path, "adapter_model.bin")
    if os.path.exists(st):
        from safetensors.torch import load_file
        return load_file(st)
    if os.path.exists(pt):
        import torch
        return torch.load(pt, map_location="cpu", weights_only=True)
    raise FileNotFoundError(f"{path}: neither adapter_model.safetensors nor adapter_model.bin")


def read_peft_dir(path, model_cfg=None):
    """A PEFT checkpoint directory -> (tensors {engine weight name: (A, B)}, scaling, config): A = lora_A.weight [r, in]
    and B = lora_B.weight [out, r] as contiguous numpy float32 (stored bf16 / fp16 tensors widened), scaling one fp32
    value, config the parsed adapter_config.json.  Goes by the tensors in the file (target_modules may be a regex or a
    superset); keys `base_model.model.<module>.lora_A.weight` or `....lora_A.default.weight`.  `model_cfg`
    (AsteroidTTSConfig or dict): layer count and shapes are checked against it.  ValueError, naming the field or the key,
    for everything that could not be merged faithfully; nothing is dropped silently."""
    import torch
    with open(os.path.join(path, "adapter_config.json")) as f:
        config = json.load(f)
    _refuse(config)
    halves = {}
    for key, t in _load_tensors(path).items():
        m = _KEY.match(key)
        if not m:
            raise ValueError(f"{path}: tensor {key!r} is not a lora_A / lora_B weight of a module (base_model.model.<module>.lora_A[.default].weight)")
        a = t.detach().to(torch.float32).contiguous().numpy()
        halves.setdefault(m.group("mod") + ".weight", {})[m.group("ab")] = a
    if not halves:
        raise ValueError(f"{path}: the adapter file holds no tensors")
    tensors = {}
    for name in sorted(halves):
        h = halves[name]
        if "A" not in h or "B" not in h:
            raise ValueError(f"{path}: {name} has lora_{'A' if 'A' in h else 'B'} without lora_{'B' if 'A' in h else 'A'}")
        tensors[name] = (h["A"], h["B"])
    check_tensors(tensors, model_cfg, rank=int(config["r"]))
    return tensors, scaling_of(config), config


def is_adapter_dir(path):
    return os.path.isfile(os.path.join(path, "adapter_config.json")) and not os.path.exists(os.path.join(path, "config.json"))


BASE_ADAPTER = "__base__"          # generate(adapter_names=[...]): this row runs without an adapter (PEFT's name for it)
MAX_BANK_RANK = 64                 # include/mtts.h: MTTS_LORA_MAX_RANK (resident, unmerged adapters)
MAX_BANK_ADAPTERS = 16             # include/mtts.h: MTTS_MAX_ADAPTERS


def delta_spec(x, A, B, scaling):
    """The unmerged low-rank path of one projection by definition, numpy float32 (every + and * one IEEE operation):

        t[j] = sum over k of A[j, k] * x[k]:  64 partial sums, number l taking k = 256 i + 4 l + c in the order i ascending,
               then c = 0..3 (acc = acc + A[j, k] * x[k], from 0; k >= in: no term), reduced by the xor tree
               v = v + v[l ^ m] for m = 32, 16, 8, 4, 2, 1
        y[n] = (sum over j ascending of B[n, j] * t[j], from 0) * scaling

    x [rows, in] (float32 holding the activation's bf16 values), A [r, in], B [out, r] -> float32 [rows, out].  A function
    of one row of x and of (A, B, scaling) alone; csrc/multilora.hip computes it with one partial sum per lane and the
    kernels' wave sum, and the tests compare bit for bit."""
    x, A, B = (np.ascontiguousarray(v, dtype=np.float32) for v in (x, A, B))
    one = x.ndim == 1
    x = x.reshape(-1, x.shape[-1])
    assert A.shape[0] == B.shape[1] and A.shape[1] == x.shape[1]
    R, K = x.shape
    r = A.shape[0]
    Kp = -(-K // 256) * 256
    xp = np.zeros((R, Kp), np.float32)
    xp[:, :K] = x
    Ap = np.zeros((r, Kp), np.float32)
    Ap[:, :K] = A
    xp, Ap = xp.reshape(R, 1, Kp // 256, 64, 4), Ap.reshape(1, r, Kp // 256, 64, 4)
    v = np.zeros((R, r, 64), np.float32)
    for i in range(Kp // 256):
        for c in range(4):
            # (a padded term adds +0.0 or -0.0 to a sum that is never -0.0: the same as no term)
            v = v + Ap[:, :, i, :, c] * xp[:, :, i, :, c]
    lanes = np.arange(64)
    for m in (32, 16, 8, 4, 2, 1):
        v = v + v[:, :, lanes ^ m]
    t = v[:, :, 0]                                                       # [R, r]
    acc = np.zeros((R, B.shape[0]), np.float32)
    for j in range(r):
        acc = acc + B[None, :, j] * t[:, j:j + 1]
    y = acc * np.float32(scaling)
    assert y.dtype == np.float32
    return y[0] if one else y


def merge_spec(W, A, B, scaling, dtype="bf16"):
    """The merged matrix by definition, numpy float32 (every + and * one IEEE operation):

        acc = 0;  for j ascending: acc = acc + B[:, j] * A[j, :];  merged = round(W + acc * scaling)

    W [out, in] float32 holding values of the model dtype; dtype "bf16" / "fp16": round to nearest even, "fp32": none.
    -> float32 [out, in]."""
    W, A, B = (np.ascontiguousarray(x, dtype=np.float32) for x in (W, A, B))
    assert A.shape[0] == B.shape[1] and W.shape == (B.shape[0], A.shape[1])
    acc = np.zeros(W.shape, dtype=np.float32)
    for j in range(A.shape[0]):
        acc = acc + B[:, j:j + 1] * A[j:j + 1, :]
    s = W + acc * np.float32(scaling)
    assert s.dtype == np.float32
    if dtype == "bf16":
        return synth.round_bf16(s)
    if dtype == "fp16":
        with np.errstate(over="ignore"):
            return s.astype(np.float16).astype(np.float32)
    if dtype == "fp32":
        return s
    raise ValueError(f"dtype {dtype!r} (bf16, fp16, fp32)")
