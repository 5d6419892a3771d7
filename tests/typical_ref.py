"""Host-side expectations for the typical_p tests (test_sampler_typical_cpu.py, test_sampler_typical_gpu.py).

The reference is HF itself, as in floors_ref.py: the installed transformers' warpers on CPU torch in the order
GenerationMixin._get_logits_processor gives them -- temperature, top-k, top-p, min_p, TypicalLogitsWarper, epsilon_cutoff,
eta_cutoff -- behind the oracle's repetition penalty.

Boundary-safe rows.  HF computes the shifts |-ln p - H| and the cumulative sums in fp32; which token a knife edge falls on
is its own rounding noise.  warp_spec.typical_margin gives the doubt mass of a row: the share of the kept mass held by
tokens whose membership a perturbation of WINDOW in the shifts, or of DELTA (relative) in the cumulative sums, could flip.
Both are ten times what measure() finds on the rows of this file's cases (all modes, HF's fp32 against float64 on the row
HF's typical warper sees; run `python tests/typical_ref.py` to repeat it):

    V = 1 025     max |shift32 - shift64| = 2.47e-6    max |cum32 - cum64| / typical_p = 9.68e-7
    V = 152 697   max |shift32 - shift64| = 3.28e-5    max |cum32 - cum64| / typical_p = 4.54e-5

    WINDOW[1025] = 5e-5, DELTA[1025] = 2e-5; WINDOW[152697] = 1e-3, DELTA[152697] = 1e-3

(times ten, then rounded up generously: torch's fp32 reductions may run in another order on another host, and a wider window
only makes the choice of rows stricter)

(The large vocabulary's errors are larger because HF's fp32 log-softmax and cumsum run over 152 697 terms.  The rows are
bf16-rounded logits, so a row holds only ~2 900 distinct scores and as many distinct shifts: sparse against these windows.
test_sampler_typical_cpu.py holds the constants to ten times the measurement on the rows in use.)

At V = 1 025 a safe row has doubt mass zero and every check is exact / scores_ref.KERNEL_TOL.  At V = 152 697 a row is drawn
again, 200 times at most, until its doubt mass is zero; failing that the first row drawn with a doubt mass of at most
DOUBT_CAP = 1e-5 is taken.  The full-vocabulary path gets the allowances test_kernel_vs_hf_warpers grants it and nothing
wider.  With these rows every case finds zero-doubt rows within a few draws.
"""
import functools

import numpy as np
import torch

from mtts import warp_spec
from oracle import asteroid_oracle as ao

import floors_ref as fr
import scores_ref as sr

MODES = {
    "typ02": dict(temperature=0.9, typical_p=0.2),                  # the mode leaves on most rows
    "typ09": dict(temperature=0.9, typical_p=0.9),
    "top_k_typ": dict(temperature=0.9, top_k=50, typical_p=0.5),
    "top_p_min_p_typ": dict(temperature=0.9, top_p=0.9, min_p=0.05, typical_p=0.6),
    "typ_eps_eta": dict(temperature=1.1, typical_p=0.9, epsilon_cutoff=3e-4, eta_cutoff=2e-3),      # floors on an interval
    "all": dict(temperature=0.9, top_k=6000, top_p=0.97, min_p=0.02, typical_p=0.9, epsilon_cutoff=3e-4, eta_cutoff=2e-3),
}
MODES = {k: dict(v, repetition_penalty=1.1) for k, v in MODES.items()}
VOCABS = fr.VOCABS
ROWS, STEPS, SEED = 6, 6, 4321
WINDOW = {1025: 5e-5, 152697: 1e-3}        # per vocabulary: ten times the measurement in the docstring, rounded up
DELTA = {1025: 2e-5, 152697: 1e-3}
DOUBT_CAP = 1e-5
DRAWS = 200


def plain(lc):
    """The layer without its typical_p."""
    return {k: v for k, v in lc.items() if k != "typical_p"}


def _procs(lc, upto_typical=False):
    from transformers.generation.logits_process import (EpsilonLogitsWarper, EtaLogitsWarper, MinPLogitsWarper,
                                                        TemperatureLogitsWarper, TopKLogitsWarper, TopPLogitsWarper,
                                                        TypicalLogitsWarper)
    procs = []
    if lc.get("temperature") is not None:
        procs.append(TemperatureLogitsWarper(float(lc["temperature"])))
    if lc.get("top_k"):
        procs.append(TopKLogitsWarper(top_k=int(lc["top_k"])))
    if lc.get("top_p") is not None:
        procs.append(TopPLogitsWarper(top_p=float(lc["top_p"])))
    if lc.get("min_p") is not None:
        procs.append(MinPLogitsWarper(min_p=float(lc["min_p"])))
    if upto_typical:
        return procs
    if lc.get("typical_p") is not None and lc["typical_p"] < 1.0:
        procs.append(TypicalLogitsWarper(mass=float(lc["typical_p"])))
    if lc.get("epsilon_cutoff"):
        procs.append(EpsilonLogitsWarper(epsilon=float(lc["epsilon_cutoff"])))
    if lc.get("eta_cutoff"):
        procs.append(EtaLogitsWarper(epsilon=float(lc["eta_cutoff"])))
    return procs


def hf_process(scores, lc, upto_typical=False):
    """scores fp32 [R, V] after the hard-coded mask and the repetition penalty -> fp32 [R, V] after HF's warpers for `lc`,
    filtered tokens at -inf.  upto_typical: the row HF's typical warper sees (the chain stops in front of it)."""
    s = torch.from_numpy(np.ascontiguousarray(scores, dtype=np.float32))
    for p in _procs(lc, upto_typical):
        s = p(None, s)
    return s.numpy()


def hf_scores(logits, hist, lc, mask_id, upto_typical=False):
    """Raw logits fp32 [R, V], history int64 [R, n] -> HF's processed rows, behind the mask and the oracle's penalty."""
    lm = np.array(logits, dtype=np.float32)
    if mask_id is not None and mask_id >= 0:
        lm[:, mask_id] = -np.inf
    if lc.get("repetition_penalty") is not None:
        lm = ao.proc_repetition_penalty(np.asarray(hist), lm, lc["repetition_penalty"])
    return hf_process(lm, lc, upto_typical)


def draw_row(rng, V, lc, mask_id):
    """One candidate row -> (logits, hist, doubt mass), or None when a top-k / top-p cut or a floor sits on a knife edge
    (floors_ref.safe_row's conditions, the floors measured behind the typical stage)."""
    pre = {k: v for k, v in lc.items() if k in ("repetition_penalty", "temperature")}
    logits = ao.round_bf16(rng.standard_normal(V).astype(np.float32) * 2.5)
    hist = rng.integers(0, V, 50)
    lm = logits.copy()
    lm[mask_id] = -np.inf
    if not fr.full_path(V, lc) and not sr.boundary_safe(ao.apply_processors(hist[None], lm[None], pre)[0], lc):
        return None
    s4 = ao.apply_processors(hist[None], lm[None], fr.four(lc))[0]
    if not warp_spec.floor_margin(s4, lc) > fr.FLOOR_REL:
        return None
    return logits, hist, warp_spec.typical_margin(s4, lc, WINDOW[V], DELTA[V])


def safe_row(rng, V, lc, mask_id):
    """-> (logits, hist, doubt mass, draws used): the first row with doubt mass zero; where DRAWS draws give none and V is
    the large vocabulary, the first one drawn with at most DOUBT_CAP."""
    spare = None
    for n in range(1, DRAWS + 1):
        r = draw_row(rng, V, lc, mask_id)
        if r is None:
            continue
        if r[2] == 0.0:
            return r + (n,)
        if spare is None and V > fr.SAMP_CAND and r[2] <= DOUBT_CAP:
            spare = r + (n,)
    if spare is not None:
        return spare[:3] + (DRAWS,)
    raise AssertionError(f"no boundary-safe row within {DRAWS} draws (V={V}, {lc})")


@functools.lru_cache(maxsize=None)
def case(V, mode):
    """-> (logits fp32 [ROWS, V], hist int64 [ROWS, 50], HF's processed rows fp32 [ROWS, V], doubt mass [ROWS], draws
    [ROWS]); built once per session and shared: treat as read-only."""
    lc = MODES[mode]
    rng = np.random.default_rng(3000 + V % 97 + len(mode))
    rows = [safe_row(rng, V, lc, VOCABS[V]["mask_id"]) for _ in range(ROWS)]
    logits, hist = np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows])
    doubt, draws = np.array([r[2] for r in rows]), np.array([r[3] for r in rows])
    want = hf_scores(logits, hist, lc, VOCABS[V]["mask_id"])
    for a in (logits, hist, want, doubt, draws):
        a.setflags(write=False)
    return logits, hist, want, doubt, draws


def lp_extra(V, lc):
    """What lp gets beyond scores_ref.KERNEL_TOL: nothing on the in-block path; on the full-vocabulary path 1e-4 over the
    kept mass, which is at least top_p * typical_p of the row (test_kernel_vs_hf_warpers: 1e-4 / top_p)."""
    if not fr.full_path(V, lc):
        return 0.0
    return 1e-4 / ((lc.get("top_p") or 1.0) * (lc.get("typical_p") or 1.0))


def expected_lp(logits_row, history, layer, do_sample, step, channel, token):
    """floors_ref.expected_lp with this file's chain (TypicalLogitsWarper included)."""
    lc = layer if do_sample else {k: v for k, v in layer.items() if k in ("repetition_penalty", "temperature")}
    lm = sr.masked(logits_row, step, channel)[None]
    if lc.get("repetition_penalty") is not None:
        lm = ao.proc_repetition_penalty(np.asarray(history)[None], lm, lc["repetition_penalty"])
    s = hf_process(lm, lc)[0]
    return sr.log_softmax64(s, token), s


def measure(V, mode):
    """-> (max |shift32 - shift64|, max |cum32 - cum64| / typical_p) over the case's rows: HF's fp32 arithmetic
    (TypicalLogitsWarper.__call__, restated) against float64 on the row its typical warper sees, in HF's own order."""
    lc = MODES[mode]
    logits, hist = case(V, mode)[:2]
    pre = hf_scores(logits, hist, lc, VOCABS[V]["mask_id"], upto_typical=True)
    ds, dc = 0.0, 0.0
    for row in pre:
        t = torch.from_numpy(row[None].copy())
        normalized = torch.nn.functional.log_softmax(t, dim=-1)
        ent = -(normalized * torch.exp(normalized)).nansum(-1, keepdim=True)
        shifted = torch.abs((-normalized) - ent)
        sorted_scores, idx = torch.sort(shifted, descending=False)
        cum32 = t.gather(-1, idx).softmax(dim=-1).cumsum(dim=-1)[0].numpy().astype(np.float64)
        kept = np.isfinite(row)
        s = row.astype(np.float64)
        d = s[kept] - s[kept].max()
        lnp = d - np.log(np.exp(d).sum())
        H = -(np.exp(lnp) * lnp).sum()
        shift64 = np.abs(-lnp - H)
        ds = max(ds, float(np.abs(shifted[0].numpy().astype(np.float64)[kept] - shift64).max()))
        p64 = np.zeros(row.shape[0])
        p64[kept] = np.exp(lnp)
        cum64 = np.cumsum(p64[idx[0].numpy()])
        dc = max(dc, float(np.abs(cum32 - cum64).max()) / lc["typical_p"])
    return ds, dc


if __name__ == "__main__":
    for V in VOCABS:
        worst = [0.0, 0.0]
        for mode in MODES:
            ds, dc = measure(V, mode)
            _, _, want, doubt, draws = case(V, mode)
            print(f"V={V} {mode}: shift {ds:.2e} cum {dc:.2e}; kept {np.isfinite(want).sum(-1).tolist()} doubt {doubt.tolist()} draws {draws.tolist()}")
            worst = [max(worst[0], ds), max(worst[1], dc)]
        print(f"V={V}: max |shift32 - shift64| = {worst[0]:.2e}, max |cum32 - cum64| / typical_p = {worst[1]:.2e}")
