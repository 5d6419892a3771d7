"""Host-side expectations for the output_scores tests (test_scores_cpu.py, test_scores_gpu.py,
golden/make_golden_scores.py).  numpy only.

lp = log_softmax(S)[d]: S the processed score row (oracle.asteroid_oracle.apply_processors, fp32, filtered tokens at
-inf), the log-softmax in float64 over its finite entries, d the decision.
"""
import numpy as np

from oracle import asteroid_oracle as ao

# Kernel budget (derived, see test_scores_gpu.py::test_kernel_lp_vs_fp64): 2 x (3.8e-6 + 3e-6 + 1e-6) rounded up.
KERNEL_TOL = 2e-5


def log_softmax64(scores_row, token):
    """float64 log-softmax of one processed score row (fp32, -inf = filtered) at `token`."""
    s = np.asarray(scores_row, dtype=np.float64)
    fin = np.isfinite(s)
    m = s[fin].max()
    return float(s[token] - m - np.log(np.exp(s[fin] - m).sum()))


def masked(logits_row, step, channel):
    """The reference's hard-coded masks (modeling_asteroid.py:124-128) on one row of raw logits of generation step `step`."""
    out = np.array(logits_row, dtype=np.float32)
    if channel != 0 and step >= channel:
        out[1024] = -np.inf
    if channel == 0 and step <= 6:
        out[152694] = -np.inf
    return out


def used_mask(gen, base_length, max_length, cfg):
    """The state machine's rule (csrc/sampler.hip update_kernel; reference modeling_asteroid.py:139-169) restated on the
    appended tokens: gen int64 [G, R, 8] -> bool [G, R, 8], True where the appended token is the model's own decision
    (not teacher-forced, not replaced by the EOS flush, not finished-row padding).  Channel 0 of an unfinished row outside a
    flush always carries the raw pick, so the appended tokens alone drive the machine.  The one raw pick that is not in the
    output is that of a row which max_length has cut off and which the reference keeps evaluating (:140-141): a
    non-speech pick resurrects it for a flush.  That step still emits padding, but the next one carries decisions on
    channels 2..7, and a decision there can never be the pad id (1024 is masked once step >= channel): a cut-off row whose
    NEXT appended row is not padding was resurrected at this step.
    """
    G, R, C = gen.shape
    lo, hi = cfg["speech_token_range"]
    eos = cfg["eos_token_id"]
    used = np.zeros((G, R, C), dtype=bool)
    unfinished = np.ones(R, dtype=bool)
    nas = -np.ones(R, dtype=np.int64)
    for g in range(G):
        for r in range(R):
            t0 = int(gen[g, r, 0])
            if unfinished[r] and nas[r] < 0 and not (lo <= t0 < hi):
                nas[r] = C - 1
            if not unfinished[r] and nas[r] < 0 and g + 1 < G and gen[g + 1, r, C - 1] != cfg["speech_pad_token"]:
                nas[r] = C - 1                              # cut-off row, resurrected by this step's (unseen) pick
            flush = 0 < nas[r] < C - 1
            for c in range(C):
                tf = g < C - 1 and c >= g + 1
                fl = flush and (c == 0 or nas[r] < C - c)
                used[g, r, c] = unfinished[r] and not tf and not fl
            if nas[r] > 0:
                nas[r] -= 1
            stopping = (base_length + g + 1 >= max_length) or t0 == eos or nas[r] == 0
            unfinished[r] = (unfinished[r] and not stopping) or nas[r] > 0
    return used


def expected_lp(logits_rows, history, layer, step, channel, token):
    """logits_rows fp32 [V] (raw logits of the step), history int64 [n] (the channel as HF's repetition penalty sees it:
    prompt slots incl. padding + generated tokens) -> float64 lp at `token`."""
    s = ao.apply_processors(np.asarray(history)[None], masked(logits_rows, step, channel)[None], layer)[0]
    return log_softmax64(s, token), s


def boundary_safe(scores_row, layer, rel=1e-4):
    """Row of scores after repetition penalty / temperature (before top-k / top-p): True when neither cut sits on a knife
    edge: the k-th and (k+1)-th scores differ, and no float64 cumulative mass of the ascending softmax over the top-k
    survivors lies within `rel` (relative) of 1 - top_p."""
    s = np.sort(np.asarray(scores_row, dtype=np.float64)[np.isfinite(scores_row)])
    k = layer.get("top_k")
    if k is not None and k < s.size:
        if s[-k] == s[-k - 1]:
            return False
        s = s[-k:]
    p = layer.get("top_p")
    if p is not None:
        e = np.exp(s - s.max())
        cum = np.cumsum(e / e.sum())
        thr = 1.0 - p
        if np.any(np.abs(cum - thr) <= rel * thr):
            return False
    return True


# The engine-against-its-own-logits runs of test_scores_gpu.py (tiny dims, ragged B=3, 44 new tokens); test_scores_cpu.py
# checks on the numpy oracle's logits of the same runs that the host side alone moves no top-k / top-p boundary.
SCENARIO = dict(weight_seed=103, wkw=dict(emb_row_sigma=0.6, speech_boost=3.6, eos_boost=2.4), prompt_seed=104, batch=3,
                prompt_len=24, audio_frac=0.3, new=44, seed=5)
SCENARIO_SAMPLED = ([dict(repetition_penalty=1.1, temperature=0.9, top_k=20, top_p=0.9)]
                    + [dict(repetition_penalty=1.05, temperature=1.1, top_k=30, top_p=0.95)] * 7, [True] * 8)


def kept_set_f64(scores_row, layer):
    """HF's top-k then top-p rules on one row of scores (after repetition penalty / temperature) with the softmax and its
    ascending cumulative sum in float64 -> sorted ids of the kept tokens.  apply_processors does the same in fp32."""
    s = np.asarray(scores_row, dtype=np.float64)
    keep = np.isfinite(s)
    k = layer.get("top_k")
    if k is not None:
        kth = np.sort(s)[-min(int(k), s.size)]
        keep &= s >= kth
    p = layer.get("top_p")
    if p is not None:
        ids = np.nonzero(keep)[0]
        order = ids[np.argsort(s[ids], kind="stable")]
        e = np.exp(s[order] - s[order].max())
        cum = np.cumsum(e / e.sum())
        remove = cum <= float(np.float32(1.0 - p))
        remove[-1] = False
        keep[order[remove]] = False
    return np.nonzero(keep)[0]
