"""The probability floors of the sampler -- HF's MinPLogitsWarper, EpsilonLogitsWarper and EtaLogitsWarper -- as numpy
states them (csrc/sampler.hip: finish_sample, sample_full_kernel; include/mtts.h: MttsSamplerFloors).  numpy only.

Repetition penalty, temperature, top-k and top-p run first and leave a kept set K.  The active floors then run in HF's
order, min_p, epsilon_cutoff, eta_cutoff, each on the survivors of the one before it.  With e_i = exp(s_i - smax),
tot = sum over K of e_i and p_i = e_i / tot:

    min_p            floor = min_p * p_max, p_max = 1 / tot
    epsilon_cutoff   floor = epsilon
    eta_cutoff       floor = min(eta, sqrt(eta) * exp(-H)), H = -sum over K of p_i ln p_i; sqrt(eta) in fp32

Token i leaves iff p_i < floor and s_i < smax (HF's min_tokens_to_keep = 1: a token at the maximum never leaves).  A value
that is absent, None or 0 means "warper absent"; a greedy channel applies none.

typical_p (HF's TypicalLogitsWarper, locally typical sampling) runs between min_p and epsilon_cutoff, HF's place for it.
Over the set K kept so far, with p_i the softmax over K:

    H       = -sum p_i ln p_i
    shift_i = |(-ln p_i) - H|
    M(t)    = sum of p_i over shift_i <= t
    t*      = the smallest shift value with M(t*) >= typical_p, or the largest shift value when none reaches it

Token i stays iff shift_i <= t*.  Tokens of equal score have equal shift and stay or leave together; the least-shifted
token always stays.  In score order the kept set is an interval, not a suffix: the most probable token can leave.  The
cutoffs that follow run on the survivors, so their "a token at the maximum never leaves" means the maximum of that
interval.  None or 1.0 means "warper absent" (HF adds it for typical_p < 1).
"""
import numpy as np

FLOOR_KEYS = ("min_p", "epsilon_cutoff", "eta_cutoff")
# the closed / half-open ranges HF's constructors accept, 0 ("absent") added to the two cutoffs'
_RANGES = {"min_p": (True, "[0, 1]"), "epsilon_cutoff": (False, "[0, 1)"), "eta_cutoff": (False, "[0, 1)")}


def check_floor(name, value, where=""):
    """-> float (0.0 for None); ValueError for a value outside the warper's range, a bool or something that is no number."""
    if value is None:
        return 0.0
    if isinstance(value, (bool, np.bool_)) or not isinstance(value, (int, float, np.integer, np.floating)):
        raise ValueError(f"{where}{name} must be a number in {_RANGES[name][1]}, got {value!r}")
    v = float(value)
    closed, text = _RANGES[name]
    if not (0.0 <= v <= 1.0) or (v == 1.0 and not closed):
        raise ValueError(f"{where}{name} must be in {text}, got {v!r}")
    return v


TYPICAL_KEY = "typical_p"


def check_typical(value, where=""):
    """-> float, 0.0 ("absent") for None and 1.0; otherwise a number strictly inside (0, 1), as HF's constructor demands.
    ValueError for anything else: a bool, NaN, 0, a value outside the range or something that is no number."""
    if value is None:
        return 0.0
    if isinstance(value, (bool, np.bool_)) or not isinstance(value, (int, float, np.integer, np.floating)):
        raise ValueError(f"{where}typical_p must be a number in (0, 1), or 1.0 / None for none, got {value!r}")
    v = float(value)
    if v == 1.0:
        return 0.0
    if not (0.0 < v < 1.0):
        raise ValueError(f"{where}typical_p must be in (0, 1), or 1.0 / None for none, got {v!r}")
    return v


def typical_of(layer, where=""):
    """One channel's dict -> typical_p as the engine takes it: the fp32 value, 0 = absent."""
    return float(np.float32(check_typical((layer or {}).get(TYPICAL_KEY), where)))


def _typical_row(row, tp, probe=None):
    """typical_p on one fp32 row, in place (leavers at -inf), float64 throughout.  probe = (window, delta): -> the doubt
    mass of the row as a share of the kept mass -- the tokens a small perturbation could flip: those of another score
    than the crossing token whose shift lies within `window` of t*, and those between the first positions at which the
    cumulative mass reaches typical_p * (1 - delta) and typical_p * (1 + delta)."""
    kept = np.flatnonzero(np.isfinite(row))
    if kept.size == 0:
        return 0.0
    s = row[kept].astype(np.float64)
    d = s - s.max()
    lnp = d - np.log(np.exp(d).sum())
    p = np.exp(lnp)
    H = -(p * lnp).sum()
    shift = np.abs(-lnp - H)
    order = np.argsort(shift, kind="stable")
    cum = np.cumsum(p[order])
    at = min(int(np.searchsorted(cum, tp, side="left")), kept.size - 1)       # the first position with cum >= typical_p
    tstar = shift[order[at]]
    stay = shift <= tstar
    doubt = 0.0
    if probe is not None:
        window, delta = probe
        other = s != s[order[at]]
        flip = other & (np.abs(shift - tstar) <= window)
        lo = min(int(np.searchsorted(cum, tp * (1.0 - delta), side="left")), kept.size - 1)
        hi = min(int(np.searchsorted(cum, tp * (1.0 + delta), side="left")), kept.size - 1)
        between = np.zeros(kept.size, dtype=bool)
        between[order[lo + 1:hi + 1]] = True
        flip |= other & between
        doubt = float(p[flip].sum() / p[stay].sum())
    row[kept[~stay]] = -np.inf
    return doubt


def floors_of(layer, where=""):
    """One channel's dict (generation_config.layers[i]) -> (min_p, epsilon_cutoff, eta_cutoff, sqrt_eta_cutoff) as the
    engine takes them: fp32 values, 0 = absent, the square root taken in fp32 as torch.sqrt of HF's fp32 scalar gives it."""
    lc = layer or {}
    mp, eps, eta = (np.float32(check_floor(k, lc.get(k), where)) for k in FLOOR_KEYS)
    return float(mp), float(eps), float(eta), float(np.sqrt(eta, dtype=np.float32))


def _cut_row(row, floors, typical=0.0, probe=None):
    """The active floors on one fp32 row, in place (leavers at -inf) -> min over the stages and the tokens below the
    maximum of |p_i / floor - 1| (inf when nothing was compared).  typical > 0: typical_p runs between min_p and
    epsilon_cutoff; probe = [window, delta]: its doubt mass (_typical_row) is appended to the list."""
    mp, eps, eta, sqrt_eta = floors
    margin = np.inf
    for which, v in enumerate((mp, eps, eta)):
        if which == 1 and typical > 0.0:
            doubt = _typical_row(row, typical, None if probe is None else (probe[0], probe[1]))
            if probe is not None:
                probe.append(doubt)
        if v <= 0.0:
            continue
        kept = np.flatnonzero(np.isfinite(row))
        s = row[kept].astype(np.float64)
        smax = s.max()
        e = np.exp(s - smax)
        tot = e.sum()
        p = e / tot
        if which == 0:
            floor = v / tot
        elif which == 1:
            floor = v
        else:
            H = -(p[p > 0] * np.log(p[p > 0])).sum()
            floor = min(v, sqrt_eta * np.exp(-H))
        below = s < smax
        if below.any():
            margin = min(margin, float(np.abs(p[below] / floor - 1.0).min()))
        row[kept[(p < floor) & below]] = -np.inf
    return margin


def apply_floors(scores, layer):
    """scores [..., V] after repetition penalty, temperature, top-k and top-p (filtered tokens at -inf) -> a float32 copy
    with the tokens the active floors of `layer`, and its typical_p, remove at -inf as well.  Sums in float64."""
    floors, typical = floors_of(layer), typical_of(layer)
    out = np.array(scores, dtype=np.float32)
    for row in out.reshape(-1, out.shape[-1]):
        _cut_row(row, floors, typical)
    return out


def floor_margin(scores_row, layer):
    """How close any token sits to an active floor of `layer`: the least |p_i / floor - 1| in float64 over the stages (inf
    without an active floor).  A token on a floor carries real mass, up to min_p * p_max, so the tests draw their rows
    again while this is small."""
    row = np.array(scores_row, dtype=np.float32)
    assert row.ndim == 1
    return _cut_row(row, floors_of(layer), typical_of(layer))


def typical_margin(scores_row, layer, window, delta):
    """The doubt mass of a row under `layer`'s typical_p, as a share of the mass typical_p keeps (0.0 without one): the mass
    of the tokens whose membership a perturbation of `window` in the shifts or of `delta` (relative) in the cumulative sums
    could flip.  scores_row as for floor_margin: after repetition penalty, temperature, top-k and top-p."""
    row = np.array(scores_row, dtype=np.float32)
    assert row.ndim == 1
    probe = [window, delta]
    _cut_row(row, floors_of(layer), typical_of(layer), probe)
    return probe[2] if len(probe) > 2 else 0.0
