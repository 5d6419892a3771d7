"""Host-side expectations for the generate() hook tests (test_gen_hooks_cpu.py, test_gen_hooks_gpu.py).

materialized() restates in numpy what scores_materialize_kernel (csrc/sampler.hip) writes for one (row, channel): the
processed scores in front of the warpers -- the masked id and the banned tokens at -inf, the additive term of a sequence
rule on the fp32 value of the raw logit, then HF's repetition penalty on the sign of that sum; no temperature.  One fp32
operation per stage, in HF's order, so the row is HF's on the bits (test_gen_hooks_cpu.py holds it against the installed
transformers' processors).

The rest are the hooks the tests pass to generate(): plain Python objects with HF's call signatures.
"""
import functools

import numpy as np

from mtts import ban_spec, bias_spec
from oracle import asteroid_oracle as ao

import bias_ref as bf

PENALTY = 1.3
# the tokens the case names (below 1024: one list serves both vocabularies)
MASKED = {1025: 1024, 152697: 152694}
BANNED, BANNED_PAIR = 14, 18          # a suppressed id; the last token of a 2-token bad word whose first ends every history
TERM_UP, TERM_FLIP, PRE = 11, 13, 15  # a term on a token outside the history; one that flips the sign of a penalised token
NEG_HIST, POS_HIST = 21, 22           # penalised tokens with a negative and a positive logit


def layer(V):
    """The settings whose processed row the case holds: every stage of the row on at least one token, the last token of the
    vocabulary (in the tail word of a 152 697-token row) among the banned ones."""
    return dict(repetition_penalty=PENALTY,
                sequence_bias={(TERM_UP,): 1.75, (TERM_FLIP,): 1.0, (PRE, TERM_UP): 0.125, (BANNED,): 3.0, (MASKED[V],): 50.0},
                bad_words_ids=[[PRE, BANNED_PAIR]], suppress_tokens=[BANNED, V - 1])


@functools.lru_cache(maxsize=None)
def case(rows, V):
    """-> (logits fp32 [rows, V] of bf16 values, hist int64 [rows, 40], banned bool [rows, V], tables [(ids, terms)] per row);
    built once per session: read-only."""
    rng = np.random.default_rng(900 + rows + V % 89)
    lc = layer(V)
    rules, _, _ = bias_spec.bias_of(lc)
    free = np.setdiff1d(np.arange(V), [MASKED[V], 1024, BANNED, BANNED_PAIR, TERM_UP, TERM_FLIP, PRE, NEG_HIST, POS_HIST, V - 1])
    logits = ao.round_bf16(rng.standard_normal((rows, V)).astype(np.float32) * 2.5)
    logits[:, TERM_FLIP], logits[:, NEG_HIST], logits[:, POS_HIST] = -0.5, -1.25, 2.5
    hist = rng.choice(free, (rows, 40))
    hist[:, 3], hist[:, 5], hist[:, 9], hist[:, -1] = TERM_FLIP, NEG_HIST, POS_HIST, PRE
    banned = np.stack([bf.spec_inputs(h, V, lc)[0] for h in hist])
    tabs = [bias_spec.bias_terms(h, V, rules) for h in hist]
    for a in (logits, hist, banned):
        a.setflags(write=False)
    return logits, hist, banned, tabs


def materialized(logits, hist, banned, tabs, penalty, mask_id):
    """The rows scores_materialize_kernel writes: logits fp32 [R, V], hist int64 [R, n] (the tokens whose history bit is set),
    banned bool [R, V], tabs [(ids, terms fp32)] per row, penalty 0 = none -> fp32 [R, V]."""
    out = np.array(logits, dtype=np.float32)
    pen = np.float32(penalty)
    for r in range(out.shape[0]):
        s = out[r]
        ids, terms = tabs[r]
        if len(ids):
            s[ids] = s[ids] + np.asarray(terms, dtype=np.float32)               # one fp32 addition on the raw value
        if penalty > 0:
            seen = np.zeros(s.shape[0], dtype=bool)
            seen[np.asarray(hist[r])] = True
            s[seen] = np.where(s[seen] < 0, s[seen] * pen, s[seen] / pen)       # HF: on the sign of raw + term
        if mask_id is not None and mask_id >= 0:
            s[mask_id] = -np.inf
        s[banned[r]] = -np.inf
    return out


def bitmap(hist, V):
    """History bitmap of one channel, uint32 [R, ceil(V / 32)]."""
    bm = np.zeros((len(hist), (V + 31) // 32), dtype=np.uint32)
    for r, h in enumerate(hist):
        for t in h:
            bm[r, int(t) >> 5] |= np.uint32(1 << (int(t) & 31))
    return bm


def words(bits):
    return np.stack([ban_spec.ban_words(b) for b in bits])


# ---- hooks with HF's call signatures ------------------------------------------------------------------------------------------
class Identity:
    """A LogitsProcessor that changes nothing; it returns a new tensor, so the copy back into the engine's rows runs."""

    def __init__(self):
        self.calls = 0

    def __call__(self, input_ids, scores):
        self.calls += 1
        return scores.clone()


class Never:
    """A StoppingCriteria that is never true; it records the lengths it was shown."""

    def __init__(self):
        self.lens = []

    def __call__(self, input_ids, scores, **kw):
        import torch
        assert scores is None
        self.lens.append(int(input_ids.shape[1]))
        return torch.zeros(input_ids.shape[0], dtype=torch.bool, device=input_ids.device)


class StopAt:
    """True for `rows` at the call whose history has `length` slots (every call from there on with `onward`), else false."""

    def __init__(self, rows, length, onward=False):
        self.rows, self.length, self.onward = list(rows), int(length), onward

    def __call__(self, input_ids, scores, **kw):
        import torch
        out = torch.zeros(input_ids.shape[0], dtype=torch.bool, device=input_ids.device)
        n = int(input_ids.shape[1])
        if n == self.length or (self.onward and n > self.length):
            out[self.rows] = True
        return out


class Recorder:
    """A streamer that records its calls in order: ("put", tensor) ... ("end",)."""

    def __init__(self):
        self.events = []

    def put(self, value):
        self.events.append(("put", value.clone()))

    def end(self):
        self.events.append(("end",))


class Force:
    """Leaves one token finite per channel: token[c] where the history has an even number of slots, alt[c] where odd."""

    def __init__(self, token, alt):
        self.token, self.alt = token, alt

    def __call__(self, input_ids, scores):
        import torch
        c = 0 if scores.shape[-1] > 2000 else 1         # (channel 0 has the large vocabulary; 1..7 share one pair)
        t = (self.token if input_ids.shape[1] % 2 == 0 else self.alt)[c]
        out = torch.full_like(scores, float("-inf"))
        out[:, t] = scores[:, t]
        return out


class AllInfRow:
    """Sets every score of `row` to -inf on every channel at the call whose history has `length` slots."""

    def __init__(self, row, length):
        self.row, self.length = row, int(length)

    def __call__(self, input_ids, scores):
        if int(input_ids.shape[1]) == self.length:
            scores[self.row] = float("-inf")             # in place: the engine's own rows
        return scores
