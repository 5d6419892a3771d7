"""The order of forward(top_logprobs=k) / Engine.score(top_k=k) as numpy states it (csrc/score.hip: head_topk_kernel,
topk_finish_kernel, topk_rows_f32_kernel).  numpy only.

The k best tokens of a row of logits are its first k under the total order (descending logit, ascending id among equal
logits).  bf16 logits tie often, so the second key is part of the contract; -0.0 and +0.0 are equal logits.
"""
import numpy as np

MAX_TOPK = 16          # include/mtts.h: MTTS_SCORE_MAX_TOPK


def check_k(k):
    """-> int k in 1..MAX_TOPK; ValueError for anything else (a bool and a float are not counts)."""
    if isinstance(k, (bool, np.bool_)) or not isinstance(k, (int, np.integer)):
        raise ValueError(f"top_logprobs must be an integer in 1..{MAX_TOPK}, got {k!r}")
    if not 1 <= int(k) <= MAX_TOPK:
        raise ValueError(f"top_logprobs must be in 1..{MAX_TOPK}, got {int(k)}")
    return int(k)


def topk_order(logits, k):
    """logits [..., V] -> int64 [..., k]: the ids of the k largest logits of every row, descending logit, ties by
    ascending id: the first k entries of lexsort((id, -logit)) -- lexsort's last key is the primary one, and -logit + 0.0
    turns -0.0 into +0.0.  Only the ids whose logit reaches the row's k-th largest value can be among them, so only
    those are sorted."""
    lg = np.asarray(logits)
    V = lg.shape[-1]
    assert 1 <= k <= V and not np.isnan(lg).any()
    flat = lg.reshape(-1, V)
    out = np.empty((flat.shape[0], k), dtype=np.int64)
    for r, row in enumerate(flat):
        kth = np.partition(row, V - k)[V - k]
        ids = np.flatnonzero(row >= kth)
        out[r] = ids[np.lexsort((ids, -row[ids].astype(np.float64) + 0.0))[:k]]
    return out.reshape(lg.shape[:-1] + (k,))


def gen_logprobs_spec(logits, mask_id, decisions, k):
    """generate(top_logprobs=k) on one step's logits (csrc/gen_topk.hip), in float64.  logits [R, V] (the fp32 view of the
    rows the forward wrote), mask_id the one id the reference's hard-coded masks put at -inf (None or < 0: none),
    decisions int [R] -> (logp float64 [R] = log_softmax(L)[decision], top_ids int64 [R, k] = the first k tokens of L
    under topk_order, top_logp float64 [R, k] = their log_softmax(L)).  No repetition penalty, temperature, top-k or
    top-p: L is what output_logits would return."""
    L = np.array(logits, dtype=np.float64)
    assert L.ndim == 2
    if mask_id is not None and int(mask_id) >= 0:
        L[:, int(mask_id)] = -np.inf
    m = L.max(-1, keepdims=True)
    with np.errstate(divide="ignore"):
        logp = L - (m + np.log(np.exp(L - m).sum(-1, keepdims=True)))
    ids = topk_order(L, k)
    d = np.asarray(decisions, dtype=np.int64).reshape(-1, 1)
    return np.take_along_axis(logp, d, -1)[:, 0], ids, np.take_along_axis(logp, ids, -1)


def topk_of_logprobs(logp, k):
    """A full row of log-probabilities [..., V] (float32) -> (ids int64 [..., k], their values [..., k]) under the same
    order: what a sweep of the label over the whole vocabulary must agree with."""
    ids = topk_order(logp, k)
    return ids, np.take_along_axis(np.asarray(logp), ids, -1)
