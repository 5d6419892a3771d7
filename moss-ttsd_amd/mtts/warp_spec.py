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


def floors_of(layer, where=""):
    """One channel's dict (generation_config.layers[i]) -> (min_p, epsilon_cutoff, eta_cutoff, sqrt_eta_cutoff) as the
    engine takes them: fp32 values, 0 = absent, the square root taken in fp32 as torch.sqrt of HF's fp32 scalar gives it."""
    lc = layer or {}
    mp, eps, eta = (np.float32(check_floor(k, lc.get(k), where)) for k in FLOOR_KEYS)
    return float(mp), float(eps), float(eta), float(np.sqrt(eta, dtype=np.float32))


def _cut_row(row, floors):
    """The active floors on one fp32 row, in place (leavers at -inf) -> min over the stages and the tokens below the
    maximum of |p_i / floor - 1| (inf when nothing was compared)."""
    mp, eps, eta, sqrt_eta = floors
    margin = np.inf
    for which, v in enumerate((mp, eps, eta)):
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
    with the tokens the active floors of `layer` remove at -inf as well.  Sums in float64."""
    floors = floors_of(layer)
    out = np.array(scores, dtype=np.float32)
    for row in out.reshape(-1, out.shape[-1]):
        _cut_row(row, floors)
    return out


def floor_margin(scores_row, layer):
    """How close any token sits to an active floor of `layer`: the least |p_i / floor - 1| in float64 over the stages (inf
    without an active floor).  A token on a floor carries real mass, up to min_p * p_max, so the tests draw their rows
    again while this is small."""
    row = np.array(scores_row, dtype=np.float32)
    assert row.ndim == 1
    return _cut_row(row, floors_of(layer))
