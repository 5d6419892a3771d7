"""The sequence rules and step-conditioned bans of the sampler -- HF's SequenceBiasLogitsProcessor, NoBadWordsLogitsProcessor,
MinLengthLogitsProcessor and SuppressTokensAtBeginLogitsProcessor -- as numpy states them (csrc/sampler.hip: bias_kernel,
ban_kernel, proc_score; include/mtts.h: MttsSamplerBias).  numpy only.  The counterpart of ban_spec.py: value checks plus
the rule.

For one channel of a row at decode step g (0-based), h is the channel's history exactly as ban_spec.py defines it,
len(h) = base + g, and V the channel's vocabulary size.

    sequence_bias        HF's two forms, {(ids...): float} and [[[ids...], float], ...]; the list form becomes the dict the
                         way HF makes it (a repeated id tuple keeps its first place and its last value).  A rule
                         (t_1..t_L, beta) with L = 1 always gives t_1 the term beta; with L > 1 it gives t_L the term beta
                         at a step where len(h) >= L and h[-(L-1):] == t_1..t_{L-1} (HF skips a rule "longer than the
                         context": one that needs L-1 tokens waits until the history holds L).  A token's term is an fp32 chain:
                         its single-token value (0 without one), then the beta of every matching longer rule in the
                         dict's order, each beta rounded to fp32 first (torch.tensor(float)), each addition in fp32.  The
                         processed score is penalty(raw + term) / temperature: one fp32 addition on the fp32 value of the
                         raw logit, behind the two hard-coded masks (-inf + term = -inf) and in front of the repetition
                         penalty, HF's order.  A token at raw -0.5 with term +1.0 and a history bit is therefore divided
                         by the penalty, not multiplied.  beta = -inf is a ban; +inf and NaN are refused.
    bad_words_ids        sequence_bias with beta = -inf for every list, after HF dropped the lists equal to [eos_token_id].
                         A matching rule puts t_L among the step's banned tokens; from there on everything ban_spec.py
                         says about a banned token holds, the all-banned row (token 0, NaN) included.
    min_length m (> 0)   eos_token_id, where the vocabulary holds it, is banned while len(h) < m.
    begin_suppress_tokens   the listed ids inside [0, V) are banned at the one step with len(h) == base + 7: HF's
                         begin_index is input_ids_seq_length, the full prompt width T = base + 7 including the delay
                         tail (ban_spec.DELAY_TAIL), and the processor fires where input_ids.shape[-1] == begin_index.

At most RULES_MAX rules per channel, sequence_bias and bad_words_ids together after the EOS filter, of at most
RULE_LEN_MAX tokens each; more is refused by name.  A rule with any id outside a channel's [0, V) is ignored on that
channel: it can never match or land there, and one list meets eight vocabularies.  Negative ids, bools, non-integers and
empty rules are refused.  A value that is absent, None, 0 or empty means "processor absent".
"""
import numpy as np

from .ban_spec import DELAY_TAIL, is_int

BIAS_KEYS = ("sequence_bias", "bad_words_ids", "min_length", "begin_suppress_tokens")
RULES_MAX = 64          # include/mtts.h: MTTS_BIAS_RULES_MAX
RULE_LEN_MAX = 16       # include/mtts.h: MTTS_BIAS_RULE_LEN_MAX
_ID_MAX = 2 ** 31 - 1


def _ids(name, seq, where):
    if isinstance(seq, (str, bytes)) or not hasattr(seq, "__iter__"):
        raise ValueError(f"{where}{name}: a rule must be a sequence of token ids, got {seq!r}")
    ids = list(seq)
    if not ids:
        raise ValueError(f"{where}{name} holds an empty rule")
    if len(ids) > RULE_LEN_MAX:
        raise ValueError(f"{where}{name}: a rule has at most {RULE_LEN_MAX} tokens, got {len(ids)}")
    for t in ids:
        if not is_int(t) or int(t) < 0 or int(t) > _ID_MAX:
            raise ValueError(f"{where}{name} must hold token ids >= 0, got {t!r}")
    return tuple(int(t) for t in ids)


def check_bias(name, value, where=""):
    """-> sequence_bias: [(ids tuple, float)] in the dict's order; bad_words_ids: [ids tuple]; begin_suppress_tokens: [int];
    min_length: int.  None gives [] / 0.  ValueError, `where` in front, for anything the module docstring refuses."""
    if name == "min_length":
        if value is None:
            return 0
        if not is_int(value) or not 0 <= int(value) <= _ID_MAX:
            raise ValueError(f"{where}min_length must be an integer >= 0, got {value!r}")
        return int(value)
    if value is None:
        return []
    if name == "begin_suppress_tokens":
        if isinstance(value, (str, bytes)) or not hasattr(value, "__iter__"):
            raise ValueError(f"{where}begin_suppress_tokens must be a list of token ids, got {value!r}")
        out = list(value)
        for t in out:
            if not is_int(t) or int(t) < 0 or int(t) > _ID_MAX:
                raise ValueError(f"{where}begin_suppress_tokens must hold token ids >= 0, got {t!r}")
        return [int(t) for t in out]
    if name == "bad_words_ids":
        if isinstance(value, (str, bytes, dict)) or not hasattr(value, "__iter__"):
            raise ValueError(f"{where}bad_words_ids must be a list of lists of token ids, got {value!r}")
        return [_ids(name, seq, where) for seq in value]
    if name != "sequence_bias":
        raise KeyError(name)
    if isinstance(value, dict):
        pairs = list(value.items())
    elif isinstance(value, (str, bytes)) or not hasattr(value, "__iter__"):
        raise ValueError(f"{where}sequence_bias must be a dict {{(ids...): float}} or a list [[[ids...], float], ...], got {value!r}")
    else:
        pairs = []
        for item in value:
            if isinstance(item, (str, bytes)) or not hasattr(item, "__len__") or len(item) != 2:
                raise ValueError(f"{where}sequence_bias: every entry is [[ids...], float], got {item!r}")
            pairs.append((item[0], item[1]))
    rules = {}
    for seq, beta in pairs:
        if isinstance(beta, (bool, np.bool_)) or not isinstance(beta, (int, float, np.integer, np.floating)):
            raise ValueError(f"{where}sequence_bias: a bias must be a number, got {beta!r}")
        beta = float(beta)
        if np.isnan(beta) or beta == np.inf:
            raise ValueError(f"{where}sequence_bias: a bias of {beta!r} is refused (finite, or -inf for a ban)")
        rules[_ids(name, seq, where)] = beta          # HF's dict: the first place, the last value
    return list(rules.items())


def bias_of(layer, where="", eos_token_id=None):
    """One channel's dict (generation_config.layers[i]) -> (rules, min_length, begin list) as the engine takes them.  rules:
    [(ids tuple, beta)], the sequence_bias rules in their order, then the bad words with beta = -inf (those equal to
    (eos_token_id,) dropped, as HF drops them); at most RULES_MAX."""
    lc = layer or {}
    rules = check_bias("sequence_bias", lc.get("sequence_bias"), where)
    bad = check_bias("bad_words_ids", lc.get("bad_words_ids"), where)
    if eos_token_id is not None:
        bad = [seq for seq in bad if seq != (int(eos_token_id),)]
    rules = rules + [(seq, -np.inf) for seq in dict.fromkeys(bad)]
    if len(rules) > RULES_MAX:
        raise ValueError(f"{where}sequence_bias and bad_words_ids hold {len(rules)} rules together, at most {RULES_MAX}")
    return (rules, check_bias("min_length", lc.get("min_length"), where),
            check_bias("begin_suppress_tokens", lc.get("begin_suppress_tokens"), where))


def rule_hits(history, vocab, rules):
    """The rules that fire after `history` (1-D ints) on a channel of `vocab` tokens -> [(last token, beta)] in the chain's
    order: the single-token rules, then the matching longer ones in the list's order.  Rules with an id outside [0, vocab)
    are ignored."""
    h = np.asarray(history, dtype=np.int64).reshape(-1)
    live = [(ids, b) for ids, b in rules if all(0 <= t < vocab for t in ids)]
    hits = [(ids[0], b) for ids, b in live if len(ids) == 1]
    for ids, b in live:
        n = len(ids) - 1
        if n >= 1 and h.shape[0] >= n + 1 and np.array_equal(h[h.shape[0] - n:], np.asarray(ids[:-1], dtype=np.int64)):
            hits.append((ids[-1], b))
    return hits


def bias_terms(history, vocab, rules):
    """-> (ids int32 ascending, terms float32): the tokens that carry a finite term after `history`, each with its fp32
    chain -- the device's bias table."""
    chain = {}
    for t, b in rule_hits(history, vocab, rules):
        if b > -np.inf:
            chain[t] = np.float32(chain.get(t, np.float32(0.0)) + np.float32(b))
    ids = np.array(sorted(chain), dtype=np.int32)
    return ids, np.array([chain[int(t)] for t in ids], dtype=np.float32)


def bias_row(history, vocab, rules):
    """float32 [vocab]: the term of every token (0 where none; -inf where a -inf rule fires)."""
    row = np.zeros(int(vocab), dtype=np.float32)
    ids, terms = bias_terms(history, vocab, rules)
    row[ids] = terms
    row[[t for t, b in rule_hits(history, vocab, rules) if b == -np.inf]] = -np.inf
    return row


def banned_mask(history, step, vocab, layer, eos_token_id=None, base=None):
    """bool [vocab]: the tokens these four processors put at -inf for a channel of `vocab` tokens with history `history`
    (len = base + step) at decode step `step`: the -inf rules that fire, eos under min_length, the begin list at its step."""
    rules, m, begin = bias_of(layer, eos_token_id=eos_token_id)
    h = np.asarray(history, dtype=np.int64).reshape(-1)
    base = h.shape[0] - step if base is None else base
    mask = np.zeros(int(vocab), dtype=bool)
    mask[[t for t, b in rule_hits(h, vocab, rules) if b == -np.inf]] = True
    if m > 0 and eos_token_id is not None and 0 <= int(eos_token_id) < vocab and h.shape[0] < m:
        mask[int(eos_token_id)] = True
    if h.shape[0] == base + DELAY_TAIL:
        mask[[t for t in begin if t < vocab]] = True
    return mask


def apply_bias(scores, term_row):
    """Raw scores [..., V] (the masks applied) + the term row, one fp32 addition each."""
    return (np.asarray(scores, dtype=np.float32) + np.asarray(term_row, dtype=np.float32)).astype(np.float32)
