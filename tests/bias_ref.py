"""Host-side expectations for the sequence-rule tests (test_sampler_bias_cpu.py, test_sampler_bias_gpu.py).

The reference is HF itself: the installed transformers' SequenceBiasLogitsProcessor, NoBadWordsLogitsProcessor,
MinLengthLogitsProcessor and SuppressTokensAtBeginLogitsProcessor on CPU torch, in GenerationMixin._get_logits_processor's
order -- SequenceBias, the oracle's repetition penalty, NoRepeatNGram, NoBadWords, MinLength, SuppressTokens,
SuppressTokensAtBegin -- in front of the warpers of floors_ref.hf_process.  HF refuses a rule with an id outside the
vocabulary where the engine ignores it on that channel, so such rules are taken out before HF sees them.
"""
import functools

import numpy as np
import torch

from mtts import ban_spec, bias_spec, warp_spec
from oracle import asteroid_oracle as ao

import bans_ref as br
import floors_ref as fr
import scores_ref as sr

VOCABS = fr.VOCABS
ROWS, STEPS, SEED = fr.ROWS, fr.STEPS, fr.SEED


def _inside(rules, vocab):
    return [(ids, b) for ids, b in rules if all(t < vocab for t in ids)]


def hf_bias(history, scores, layer, step=0, eos_token_id=None, base=None):
    """scores fp32 [R, V] (the hard-coded masks applied), history int64 [R, n] (n = base + step) -> HF's four processors on
    them, in _get_logits_processor's order, without the penalty between them (hf_scores puts it there)."""
    from transformers.generation.logits_process import SequenceBiasLogitsProcessor
    ids = torch.from_numpy(np.asarray(history, dtype=np.int64).reshape(len(scores), -1))
    s = torch.from_numpy(np.ascontiguousarray(scores, dtype=np.float32))
    V = s.shape[-1]
    seq = _inside(bias_spec.check_bias("sequence_bias", layer.get("sequence_bias")), V)
    if seq:
        s = SequenceBiasLogitsProcessor(sequence_bias=dict(seq))(ids, s)
    return _hf_bans(ids, s, layer, step, eos_token_id, base)


def _hf_bans(ids, s, layer, step, eos_token_id, base):
    from transformers.generation.logits_process import (MinLengthLogitsProcessor, NoBadWordsLogitsProcessor,
                                                        SuppressTokensAtBeginLogitsProcessor)
    V = s.shape[-1]
    bad = [list(w) for w in bias_spec.check_bias("bad_words_ids", layer.get("bad_words_ids")) if all(t < V for t in w)]
    if bad:
        proc = NoBadWordsLogitsProcessor(bad, eos_token_id)        # (HF's own EOS filter; it refuses an empty result)
        s = proc(ids, s)
    m = bias_spec.check_bias("min_length", layer.get("min_length"))
    if m > 0 and eos_token_id is not None:
        s = MinLengthLogitsProcessor(m, eos_token_id, device="cpu")(ids, s)
    if layer.get("begin_suppress_tokens") is not None:
        # HF: begin_index = input_ids_seq_length = the full prompt width T = base + 7; the processor sees base + step columns
        T = (ids.shape[1] - step if base is None else base) + ban_spec.DELAY_TAIL
        s = SuppressTokensAtBeginLogitsProcessor(list(layer["begin_suppress_tokens"]), T, device="cpu")(ids, s)
    return s.numpy()


def hf_scores(logits, hist, lc, mask_id):
    """Raw logits fp32 [R, V], history int64 [R, n] -> HF's processed rows: mask, SequenceBias, the oracle's repetition
    penalty, NoRepeatNGram, NoBadWords, SuppressTokens, then floors_ref.hf_process (Temperature, TopK, TopP, the floors)."""
    from transformers.generation.logits_process import SequenceBiasLogitsProcessor
    lm = np.array(logits, dtype=np.float32)
    V = lm.shape[-1]
    if mask_id is not None and mask_id >= 0:
        lm[:, mask_id] = -np.inf
    ids = torch.from_numpy(np.asarray(hist, dtype=np.int64))
    seq = _inside(bias_spec.check_bias("sequence_bias", lc.get("sequence_bias")), V)
    if seq:
        lm = SequenceBiasLogitsProcessor(sequence_bias=dict(seq))(ids, torch.from_numpy(lm)).numpy()
    rest = {k: lc[k] for k in ("repetition_penalty", "no_repeat_ngram_size", "suppress_tokens") if k in lc}
    s = br.hf_scores(lm, hist, rest, None)          # the penalty, NoRepeatNGram, SuppressTokens (no warper among the keys)
    s = _hf_bans(ids, torch.from_numpy(np.ascontiguousarray(s)), lc, 0, None, None)
    return fr.hf_process(s, lc)


# ---- the sampler cases ------------------------------------------------------------------------------------------------------
# The tokens the rules name (all below 1024: one list serves both vocabularies), and what each is for
UP, DOWN, FLIP, GONE, PRE, NEXT, NEXT_BAD = 11, 12, 13, 14, 15, 16, 18
SEQUENCE_BIAS = {
    (UP,): 1.7,                 # a positive term that makes a non-maximal token the argmax (with the 0.1 below: a chain of two)
    (DOWN,): -6.0,              # a negative term on the raw maximum
    (FLIP,): 1.0,               # raw -0.5 with the history bit: +0.5 is divided by the penalty, not multiplied
    (1024,): 50.0,              # the masked id of the 1025-token channels stays -inf (an ordinary token on channel 0)
    (152694,): 50.0,            # ... of channel 0 (ignored on the others)
    (PRE, UP): 0.1,             # fires: every history ends in PRE
    (PRE, NEXT): 2.5,           # fires, on a token without a single-token rule
    (NEXT, UP): 9.0,            # does not fire
    (PRE, PRE, NEXT): 7.0,      # does not fire (the history's last two are not PRE, PRE)
    (GONE, 5000): 1.0,          # ignored on the 1025-token channels, no match on channel 0
}
BAD_WORDS = [[GONE], [PRE, NEXT_BAD], [NEXT, DOWN]]        # a single-token ban, a 2-token ban that fires, one that does not
MODES = {k: (dict(v, sequence_bias=SEQUENCE_BIAS, bad_words_ids=BAD_WORDS), ds) for k, (v, ds) in br.MODES.items()}
_SPECIAL = (UP, DOWN, FLIP, GONE, PRE, NEXT, NEXT_BAD)


def spec_inputs(hist, V, lc):
    """ban_spec and bias_spec on one row's history -> (banned bool [V], term row fp32 [V])."""
    rules, _, _ = bias_spec.bias_of(lc)
    banned = ban_spec.banned_mask(hist, 0, V, lc) | bias_spec.banned_mask(hist, 0, V, lc)
    return banned, bias_spec.bias_row(hist, V, rules)


def safe_row(rng, V, lc, mask_id):
    """floors_ref.safe_row with rules that bite: DOWN is the raw maximum, UP lies 1.0 below it, FLIP is at -0.5 and in the
    history, GONE and NEXT_BAD lie between the two, and the history ends in PRE.  Drawn again while a top-k / top-p cut of the
    biased, banned row sits on a knife edge (not on the full-vocabulary path, as there) or a token lies within FLOOR_REL of
    a floor."""
    pre = {k: v for k, v in lc.items() if k in ("repetition_penalty", "temperature")}
    free = np.setdiff1d(np.arange(V), list(_SPECIAL) + [mask_id, 1024])
    for _ in range(200):
        logits = ao.round_bf16(rng.standard_normal(V).astype(np.float32) * 2.5)
        top = float(np.sort(logits)[-1])
        logits[DOWN], logits[UP], logits[FLIP] = top + 1.0, top - 1.0, -0.5
        logits[GONE], logits[NEXT_BAD], logits[NEXT] = top + 0.5, top + 0.25, top - 3.0
        logits = ao.round_bf16(logits)
        hist = rng.choice(free, 50)
        hist[7], hist[-1] = FLIP, PRE
        banned, term = spec_inputs(hist, V, lc)
        lm = logits.copy()
        lm[mask_id] = -np.inf
        lm = bias_spec.apply_bias(lm, term)
        lm[banned] = -np.inf
        if not fr.full_path(V, lc) and not sr.boundary_safe(ao.apply_processors(hist[None], lm[None], pre)[0], lc):
            continue
        s4 = ao.apply_processors(hist[None], lm[None], fr.four(lc))[0]
        if (s4 == s4.max()).sum() == 1 and warp_spec.floor_margin(s4, lc) > fr.FLOOR_REL:
            return logits, hist
    raise AssertionError("no boundary-safe row found")


@functools.lru_cache(maxsize=None)
def case(V, mode):
    """-> (logits fp32 [ROWS, V], hist int64 [ROWS, 50], ban words uint32 [ROWS, ceil(V/32)], bias words the same shape,
    tables [(ids int32, terms fp32)] per row, HF's processed rows fp32 [ROWS, V]); built once per session: read-only."""
    lc, _ = MODES[mode]
    rng = np.random.default_rng(4000 + V % 97 + len(mode))
    rows = [safe_row(rng, V, lc, VOCABS[V]["mask_id"]) for _ in range(ROWS)]
    logits, hist = np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows])
    rules, _, _ = bias_spec.bias_of(lc)
    ban = np.stack([ban_spec.ban_words(spec_inputs(h, V, lc)[0]) for h in hist])
    tabs = [bias_spec.bias_terms(h, V, rules) for h in hist]
    bits = np.zeros((ROWS, V), dtype=bool)
    for r, (ids, _) in enumerate(tabs):
        bits[r, ids] = True
    words = np.stack([ban_spec.ban_words(b) for b in bits])
    want = hf_scores(logits, hist, lc, VOCABS[V]["mask_id"])
    for a in (logits, hist, ban, words, want):
        a.setflags(write=False)
    return logits, hist, ban, words, tabs, want


def hf_step_row(logits_row, history, layer, step, channel, eos_token_id, base):
    """A greedy engine step on its own logits: raw logits fp32 [V] of decode step `step` -> the row after the hard-coded
    masks and HF's four processors (greedy channels of these tests set no penalty and no temperature)."""
    s = sr.masked(logits_row, step, channel)
    return hf_bias(np.asarray(history)[None], s[None], layer, step, eos_token_id, base)[0]
