"""Host-side expectations for the hard-ban tests (test_sampler_bans_cpu.py, test_sampler_bans_gpu.py).

The reference is HF itself: the installed transformers' NoRepeatNGramLogitsProcessor, SuppressTokensLogitsProcessor and
MinNewTokensLengthLogitsProcessor on CPU torch, in GenerationMixin._get_logits_processor's order behind the oracle's
repetition penalty and in front of the warpers of floors_ref.hf_process.
"""
import functools

import numpy as np
import torch

from mtts import ban_spec, warp_spec
from oracle import asteroid_oracle as ao

import floors_ref as fr
import scores_ref as sr

VOCABS = fr.VOCABS
ROWS, STEPS, SEED = fr.ROWS, fr.STEPS, fr.SEED
SUPPRESS = [3, 17, 1000, 1024, 1030, 5000, 152000]          # one list, ids on both sides of 1025


def hf_ban_row(history, vocab, layer, step=0, eos_token_id=None, base=None):
    """bool [vocab]: the tokens HF's three processors put at -inf on a row of zeros.  history: 1-D ints, len = base + step."""
    from transformers.generation.logits_process import (MinNewTokensLengthLogitsProcessor, NoRepeatNGramLogitsProcessor,
                                                        SuppressTokensLogitsProcessor)
    ids = torch.from_numpy(np.asarray(history, dtype=np.int64).reshape(1, -1))
    s = torch.zeros(1, int(vocab), dtype=torch.float32)
    n, m, sup = ban_spec.bans_of(layer)
    if n > 0:
        s = NoRepeatNGramLogitsProcessor(n)(ids, s)
    if m > 0 and eos_token_id is not None:
        # HF: prompt_length_to_skip = the full prompt width T = base + 7; the processor sees base + step columns
        T = (ids.shape[1] - step if base is None else base) + ban_spec.DELAY_TAIL
        s = MinNewTokensLengthLogitsProcessor(T, m, eos_token_id, device="cpu")(ids, s)
    if layer.get("suppress_tokens") is not None:
        s = SuppressTokensLogitsProcessor(sup, device="cpu")(ids, s)
    return np.isinf(s.numpy()[0])


def hf_scores(logits, hist, lc, mask_id):
    """Raw logits fp32 [R, V], history int64 [R, n] -> HF's processed rows: mask, the oracle's repetition penalty,
    NoRepeatNGram, SuppressTokens, then floors_ref.hf_process (Temperature, TopK, TopP, the floors)."""
    from transformers.generation.logits_process import NoRepeatNGramLogitsProcessor, SuppressTokensLogitsProcessor
    lm = np.array(logits, dtype=np.float32)
    if mask_id is not None and mask_id >= 0:
        lm[:, mask_id] = -np.inf
    if lc.get("repetition_penalty") is not None:
        lm = ao.proc_repetition_penalty(np.asarray(hist), lm, lc["repetition_penalty"])
    s = torch.from_numpy(np.ascontiguousarray(lm))
    ids = torch.from_numpy(np.asarray(hist, dtype=np.int64))
    if lc.get("no_repeat_ngram_size"):
        s = NoRepeatNGramLogitsProcessor(int(lc["no_repeat_ngram_size"]))(ids, s)
    if lc.get("suppress_tokens") is not None:
        s = SuppressTokensLogitsProcessor(list(lc["suppress_tokens"]), device="cpu")(ids, s)
    return fr.hf_process(s.numpy(), lc)


# name -> (layer config, do_sample): in-block path, full-vocabulary path (on 152 697 tokens), a greedy channel, floors behind bans
MODES = {
    "top_k_top_p": (dict(temperature=0.9, top_k=50, top_p=0.9), True),
    "top_p": (dict(temperature=0.9, top_p=0.9), True),
    "greedy": (dict(temperature=0.9), False),
    "top_k_min_p": (dict(temperature=0.9, top_k=50, min_p=0.1), True),
}
MODES = {k: (dict(v, repetition_penalty=1.1, no_repeat_ngram_size=2, suppress_tokens=SUPPRESS), ds) for k, (v, ds) in MODES.items()}


def safe_row(rng, V, lc, mask_id):
    """floors_ref.safe_row with bans that bite: the 50-token history is drawn from the row's 12 most probable tokens, so
    no_repeat_ngram_size = 2 bans several of them; drawn again while a top-k / top-p cut of the BANNED row sits on a knife
    edge (not on the full-vocabulary path, as there) or a token lies within FLOOR_REL of a floor."""
    pre = {k: v for k, v in lc.items() if k in ("repetition_penalty", "temperature")}
    for _ in range(200):
        logits = ao.round_bf16(rng.standard_normal(V).astype(np.float32) * 2.5)
        top = np.argsort(-logits)[:12]
        hist = rng.choice(top, 50)
        hist[-1] = hist[0]                      # the last token occurred before: its follower hist[1] is banned
        lm = logits.copy()
        lm[mask_id] = -np.inf
        lm[ban_spec.banned_mask(hist, 0, V, lc)] = -np.inf
        if not fr.full_path(V, lc) and not sr.boundary_safe(ao.apply_processors(hist[None], lm[None], pre)[0], lc):
            continue
        s4 = ao.apply_processors(hist[None], lm[None], fr.four(lc))[0]
        if warp_spec.floor_margin(s4, lc) > fr.FLOOR_REL:
            return logits, hist
    raise AssertionError("no boundary-safe row found")


@functools.lru_cache(maxsize=None)
def case(V, mode):
    """-> (logits fp32 [ROWS, V], hist int64 [ROWS, 50], ban words uint32 [ROWS, ceil(V/32)] by ban_spec, HF's processed
    rows fp32 [ROWS, V]); built once per session and shared: read-only."""
    lc, _ = MODES[mode]
    rng = np.random.default_rng(3000 + V % 97 + len(mode))
    rows = [safe_row(rng, V, lc, VOCABS[V]["mask_id"]) for _ in range(ROWS)]
    logits, hist = np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows])
    words = np.stack([ban_spec.ban_words(ban_spec.banned_mask(h, 0, V, lc)) for h in hist])
    want = hf_scores(logits, hist, lc, VOCABS[V]["mask_id"])
    for a in (logits, hist, words, want):
        a.setflags(write=False)
    return logits, hist, words, want


def hf_step_row(logits_row, history, layer, step, channel, eos_token_id, base):
    """A greedy engine step on its own logits: raw logits fp32 [V] of decode step `step` -> the row after the hard-coded
    masks and HF's three ban processors (greedy channels of these tests set no penalty and no temperature)."""
    s = sr.masked(logits_row, step, channel)
    s[hf_ban_row(history, s.shape[0], layer, step, eos_token_id, base)] = -np.inf
    return s
