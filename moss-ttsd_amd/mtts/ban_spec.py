"""The hard bans of the sampler -- HF's NoRepeatNGramLogitsProcessor, SuppressTokensLogitsProcessor and
MinNewTokensLengthLogitsProcessor -- as numpy states them (csrc/sampler.hip: ban_kernel, proc_score; include/mtts.h:
MttsSamplerBans).  numpy only.  The counterpart of warp_spec.py: value checks plus the rule.

All three only put tokens at -inf, and -inf survives repetition penalty and temperature, so HF's order among the
processors reduces to: a banned token has processed score -inf, everything else is as without bans.  They are processors,
not warpers: a greedy channel applies them too.  For one channel of a row at decode step g (0-based), h is the channel's
history as the reference's input_ids[..., c] holds it, len(h) = base + g: every left-padded slot of the prompt and every
token the step appended since (teacher-forced, flush, padding and forced-replay tokens included) -- the stream that sets
bits in the repetition-penalty bitmap.  The banned set is the union of

    no_repeat_ngram_size n (1..16)   if len(h) >= n: every h[j+n-1] with h[j : j+n-1] == h[len(h)-n+1 :],
                                     0 <= j <= len(h)-n.  With n = 1 that is every token of h.
    suppress_tokens                  every listed id inside [0, V); ids outside the channel's vocabulary are ignored (HF's
                                     isin(arange(V), ids); one list meets eight vocabularies).  Negative ids are refused.
    min_new_tokens m (> 0)           eos_token_id, where the vocabulary holds it, while g < m + 7: HF sets
                                     prompt_length_to_skip = T, the full prompt width including the 7-slot delay tail,
                                     and the processor sees T - 7 + g columns.  It keeps EOS out and nothing else: a
                                     dialogue still ends on any non-speech pick on channel 0, as in the reference.

A value that is absent, None or 0 (an empty list) means "processor absent".
"""
import numpy as np

BAN_KEYS = ("no_repeat_ngram_size", "suppress_tokens", "min_new_tokens")
NGRAM_MAX = 16          # include/mtts.h: MTTS_NGRAM_MAX
DELAY_TAIL = 7          # prompt slots behind base that HF's prompt_length_to_skip counts


def is_int(v):
    return isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_))


def check_ban(name, value, where=""):
    """-> int (0 for None), or for suppress_tokens a list of ints ([] for None); ValueError, `where` in front, for an
    n-gram size outside [0, 16], a negative min_new_tokens or id, a bool or something that is no integer."""
    if name == "suppress_tokens":
        if value is None:
            return []
        if isinstance(value, (str, bytes)) or not hasattr(value, "__iter__"):
            raise ValueError(f"{where}suppress_tokens must be a list of token ids, got {value!r}")
        ids = list(value)
        for t in ids:
            if not is_int(t) or int(t) < 0 or int(t) > 2 ** 31 - 1:
                raise ValueError(f"{where}suppress_tokens must hold token ids >= 0, got {t!r}")
        return [int(t) for t in ids]
    if value is None:
        return 0
    if not is_int(value):
        raise ValueError(f"{where}{name} must be an integer, got {value!r}")
    v = int(value)
    if name == "no_repeat_ngram_size" and not 0 <= v <= NGRAM_MAX:
        raise ValueError(f"{where}no_repeat_ngram_size must be in [0, {NGRAM_MAX}], got {v}")
    if name == "min_new_tokens" and not 0 <= v <= 2 ** 31 - 1 - DELAY_TAIL:
        raise ValueError(f"{where}min_new_tokens must be >= 0, got {v}")
    return v


def bans_of(layer, where=""):
    """One channel's dict (generation_config.layers[i]) -> (no_repeat_ngram_size, min_new_tokens, suppress list) as the
    engine takes them, 0 / [] = absent."""
    lc = layer or {}
    return (check_ban("no_repeat_ngram_size", lc.get("no_repeat_ngram_size"), where),
            check_ban("min_new_tokens", lc.get("min_new_tokens"), where),
            check_ban("suppress_tokens", lc.get("suppress_tokens"), where))


def ngram_banned(history, n):
    """The ids no_repeat_ngram_size = n bans after `history` (1-D ints) -> sorted unique int64 array."""
    h = np.asarray(history, dtype=np.int64).reshape(-1)
    L = h.shape[0]
    if n <= 0 or L < n:
        return np.zeros(0, dtype=np.int64)
    if n == 1:
        return np.unique(h)
    suffix = h[L - n + 1:]
    starts = np.arange(0, L - n + 1)
    ok = np.ones(starts.shape[0], dtype=bool)
    for k in range(n - 1):
        ok &= h[starts + k] == suffix[k]
    return np.unique(h[starts[ok] + n - 1])


def banned_mask(history, step, vocab, layer, eos_token_id=None):
    """bool [vocab]: the tokens at -inf for a channel of `vocab` tokens with history `history` (len = base + step) at decode
    step `step` under the bans of `layer`."""
    n, m, sup = bans_of(layer)
    mask = np.zeros(int(vocab), dtype=bool)
    ids = ngram_banned(history, n)
    mask[ids[(ids >= 0) & (ids < vocab)]] = True
    for t in sup:
        if t < vocab:
            mask[t] = True
    if m > 0 and eos_token_id is not None and 0 <= int(eos_token_id) < vocab and step < m + DELAY_TAIL:
        mask[int(eos_token_id)] = True
    return mask


def ban_words(mask):
    """bool [V] -> uint32 [ceil(V / 32)], bit i of word i // 32 = mask[i] (the layout of the device's ban words)."""
    m = np.asarray(mask, dtype=bool)
    pad = np.zeros((m.shape[0] + 31) // 32 * 32, dtype=bool)
    pad[:m.shape[0]] = m
    return np.packbits(pad.reshape(-1, 32), axis=1, bitorder="little").view("<u4").reshape(-1).astype(np.uint32)


def apply_bans(scores, mask):
    """scores [..., V] -> a float32 copy with the banned tokens at -inf."""
    out = np.array(scores, dtype=np.float32)
    out[..., np.asarray(mask, dtype=bool)] = -np.inf
    return out
