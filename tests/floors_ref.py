"""Host-side expectations for the probability-floor tests (test_sampler_floors_cpu.py, test_sampler_floors_gpu.py).

The reference is HF itself: the installed transformers' TemperatureLogitsWarper, TopKLogitsWarper, TopPLogitsWarper,
MinPLogitsWarper, EpsilonLogitsWarper and EtaLogitsWarper on CPU torch, in the order GenerationMixin._get_logits_processor
gives them, behind the oracle's repetition penalty (oracle.asteroid_oracle.proc_repetition_penalty).
"""
import functools

import numpy as np
import torch

from mtts import warp_spec
from oracle import asteroid_oracle as ao

import scores_ref as sr

# name -> layer config of a sampled channel (every mode runs behind a repetition penalty over a 50-token history)
MODES = {
    "min_p": dict(temperature=0.9, min_p=0.05),
    "top_k_min_p": dict(temperature=0.9, top_k=50, min_p=0.1),
    "top_p_min_p": dict(temperature=0.9, top_p=0.9, min_p=0.05),
    "epsilon": dict(temperature=1.1, epsilon_cutoff=3e-4),
    "eta": dict(temperature=1.1, eta_cutoff=2e-3),
    "all": dict(temperature=0.9, top_k=6000, top_p=0.97, min_p=0.02, epsilon_cutoff=3e-4, eta_cutoff=2e-3),
}
MODES = {k: dict(v, repetition_penalty=1.1) for k, v in MODES.items()}
VOCABS = {1025: dict(mask_id=1024, channel=3), 152697: dict(mask_id=152694, channel=0)}
ROWS, STEPS, SEED = 6, 6, 4321
FLOOR_REL = 1e-3          # no token within this (relative, float64) of a floor: one on it carries up to min_p * p_max of mass
SAMP_CAND = 4096          # csrc: candidates the in-block path holds; beyond it (or without top_k) channel 0 takes the full path

FOUR = ("repetition_penalty", "temperature", "top_k", "top_p")


def four(lc):
    """The reference's four keys of a layer config (what oracle.apply_processors reads)."""
    return {k: v for k, v in lc.items() if k in FOUR}


def full_path(V, lc):
    return V > SAMP_CAND and not (lc.get("top_k") and lc["top_k"] <= SAMP_CAND)


def hf_process(scores, lc):
    """scores fp32 [R, V] after the hard-coded mask and the repetition penalty -> fp32 [R, V] after HF's warpers for `lc`,
    filtered tokens at -inf."""
    from transformers.generation.logits_process import (EpsilonLogitsWarper, EtaLogitsWarper, MinPLogitsWarper,
                                                        TemperatureLogitsWarper, TopKLogitsWarper, TopPLogitsWarper)
    s = torch.from_numpy(np.ascontiguousarray(scores, dtype=np.float32))
    procs = []
    if lc.get("temperature") is not None:
        procs.append(TemperatureLogitsWarper(float(lc["temperature"])))
    if lc.get("top_k"):
        procs.append(TopKLogitsWarper(top_k=int(lc["top_k"])))
    if lc.get("top_p") is not None:
        procs.append(TopPLogitsWarper(top_p=float(lc["top_p"])))
    if lc.get("min_p") is not None:
        procs.append(MinPLogitsWarper(min_p=float(lc["min_p"])))
    if lc.get("epsilon_cutoff"):
        procs.append(EpsilonLogitsWarper(epsilon=float(lc["epsilon_cutoff"])))
    if lc.get("eta_cutoff"):
        procs.append(EtaLogitsWarper(epsilon=float(lc["eta_cutoff"])))
    for p in procs:
        s = p(None, s)
    return s.numpy()


def hf_scores(logits, hist, lc, mask_id):
    """Raw logits fp32 [R, V], history int64 [R, n] -> HF's processed rows, behind the mask and the oracle's penalty."""
    lm = np.array(logits, dtype=np.float32)
    if mask_id is not None and mask_id >= 0:
        lm[:, mask_id] = -np.inf
    if lc.get("repetition_penalty") is not None:
        lm = ao.proc_repetition_penalty(np.asarray(hist), lm, lc["repetition_penalty"])
    return hf_process(lm, lc)


def safe_row(rng, V, lc, mask_id, tie_free=False):
    """One boundary-safe row: bf16-rounded N(0, 2.5^2) logits and a 50-token history, drawn again (200 times at most) while
    a top-k / top-p cut sits on a knife edge (scores_ref.boundary_safe, where test_kernel_lp_vs_fp64 applies it: not on
    the full-vocabulary path) or a token lies within FLOOR_REL of a floor; tie_free: or the maximum is shared."""
    pre = {k: v for k, v in lc.items() if k in ("repetition_penalty", "temperature")}
    for _ in range(200):
        logits = ao.round_bf16(rng.standard_normal(V).astype(np.float32) * 2.5)
        hist = rng.integers(0, V, 50)
        lm = logits.copy()
        lm[mask_id] = -np.inf
        if not full_path(V, lc) and not sr.boundary_safe(ao.apply_processors(hist[None], lm[None], pre)[0], lc):
            continue
        s4 = ao.apply_processors(hist[None], lm[None], four(lc))[0]
        if tie_free and (s4 == s4.max()).sum() != 1:
            continue
        if warp_spec.floor_margin(s4, lc) > FLOOR_REL:
            return logits, hist
    raise AssertionError("no boundary-safe row found")


@functools.lru_cache(maxsize=None)
def case(V, mode):
    """-> (logits fp32 [ROWS, V], hist int64 [ROWS, 50], HF's processed rows fp32 [ROWS, V]); built once per session and
    shared: treat as read-only."""
    lc = MODES[mode]
    rng = np.random.default_rng(2000 + V % 97 + len(mode))
    rows = [safe_row(rng, V, lc, VOCABS[V]["mask_id"]) for _ in range(ROWS)]
    logits, hist = np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows])
    want = hf_scores(logits, hist, lc, VOCABS[V]["mask_id"])
    for a in (logits, hist, want):
        a.setflags(write=False)
    return logits, hist, want


def expected_lp(logits_row, history, layer, do_sample, step, channel, token):
    """scores_ref.expected_lp with HF's warpers as the reference: raw logits fp32 [V] of a generation step -> (float64 lp at
    `token`, the processed row).  A greedy channel applies the repetition penalty and the temperature only."""
    lc = layer if do_sample else {k: v for k, v in layer.items() if k in ("repetition_penalty", "temperature")}
    lm = sr.masked(logits_row, step, channel)[None]
    if lc.get("repetition_penalty") is not None:
        lm = ao.proc_repetition_penalty(np.asarray(history)[None], lm, lc["repetition_penalty"])
    s = hf_process(lm, lc)[0]
    return sr.log_softmax64(s, token), s
