"""generate(top_logprobs=k), the parts that need no GPU: the numpy statement the GPU tests compare with
(mtts/topk_spec.py: gen_logprobs_spec) against a brute-force log-softmax and lexsort, the argument checks of
AsteroidTTSInstruct.generate, the batcher's return shapes, and the ctypes prototypes against include/mtts.h."""
import ctypes as C
import os
import re

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from mtts import capi, synth, topk_spec  # noqa: E402

import modeling_asteroid as ma  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the statement ---------------------------------------------------------------------------------------------------------
def _brute(logits, mask_id, decisions, k):
    """Row by row: float64 log-softmax by the textbook formula, the order by one lexsort over the whole row."""
    R, V = logits.shape
    lp, ids, tlp = np.empty(R), np.empty((R, k), dtype=np.int64), np.empty((R, k))
    for r in range(R):
        L = logits[r].astype(np.float64)
        if mask_id is not None and mask_id >= 0:
            L[mask_id] = -np.inf
        with np.errstate(divide="ignore"):
            row = L - L.max() - np.log(np.sum(np.exp(L - L.max())))
        order = np.lexsort((np.arange(V), -L + 0.0))             # last key first: descending logit, then ascending id
        lp[r], ids[r], tlp[r] = row[decisions[r]], order[:k], row[order[:k]]
    return lp, ids, tlp


def _planted_rows(V, mask_id, seed):
    """bf16-like rows (many ties) with the planted cases: equal maxima far apart, +0 / -0 as the largest values, an
    all-equal row, the masked id holding the largest raw logit."""
    rng = np.random.default_rng(seed)
    rows = (rng.integers(-40, 24, (6, V)) / 8).astype(np.float32)
    rows[0, [3, V // 2, V - 2]] = 5.0                              # equal maxima: ascending id
    rows[1] = -np.abs(rows[1]) - 1.0
    rows[1, [7, 2, V - 2]] = [0.0, -0.0, 0.0]                      # +0 and -0 are one value: ids 2, 7, V - 2
    rows[2] = 1.25                                                 # all equal: ids 0..k-1, value -log V (or V - 1)
    rows[3, mask_id] = 9.0                                         # the masked id would win
    rows[4, mask_id] = 3.0
    rows[4, 5] = 3.0
    return rows


@pytest.mark.parametrize("V,mask_id", [(1025, 1024), (4133, 17), (4133, -1)])
def test_gen_logprobs_spec_against_brute_force(V, mask_id):
    rows = _planted_rows(V, max(mask_id, 0), 3)
    rng = np.random.default_rng(4)
    dec = rng.integers(0, V - 1, rows.shape[0])
    dec[0], dec[2] = V - 2, 0
    if mask_id >= 0:
        dec[dec == mask_id] = 0
    for k in (1, 5, 16):
        lp, ids, tlp = topk_spec.gen_logprobs_spec(rows, mask_id, dec, k)
        wlp, wids, wtlp = _brute(rows, mask_id, dec, k)
        assert lp.dtype == np.float64 and ids.dtype == np.int64 and ids.shape == (6, k) and tlp.shape == (6, k)
        assert np.array_equal(ids, wids)
        assert np.allclose(lp, wlp, rtol=0, atol=1e-12) and np.allclose(tlp, wtlp, rtol=0, atol=1e-12)
        assert ids[0, :min(k, 3)].tolist() == [3, V // 2, V - 2][:k]
        assert ids[1, :min(k, 3)].tolist() == [2, 7, V - 2][:k]
        assert ids[2].tolist() == list(range(k)) or (mask_id >= 0 and mask_id < k)
        n = V - (1 if mask_id >= 0 else 0)
        assert np.allclose(tlp[2], -np.log(n), atol=1e-12)
        if mask_id >= 0:
            assert not (ids == mask_id).any()                      # at -inf it is last in the order
            full = topk_spec.gen_logprobs_spec(rows[3:4], mask_id, [mask_id], 1)
            assert full[0][0] == -np.inf                           # ... and has probability 0
        # where the decision is among the k best, the two values are the same number
        for r in range(6):
            for j in np.flatnonzero(ids[r] == dec[r]):
                assert lp[r] == tlp[r, j]
    # the first k' entries do not depend on k
    a, b = topk_spec.gen_logprobs_spec(rows, mask_id, dec, 16), topk_spec.gen_logprobs_spec(rows, mask_id, dec, 4)
    assert np.array_equal(a[1][:, :4], b[1]) and np.array_equal(a[2][:, :4], b[2]) and np.array_equal(a[0], b[0])


def test_gen_logprobs_spec_applies_no_processor():
    """The values are those of the raw row: probabilities sum to one over the unmasked ids."""
    rng = np.random.default_rng(8)
    rows = rng.standard_normal((2, 300)).astype(np.float32) * 3
    _, ids, tlp = topk_spec.gen_logprobs_spec(rows, 11, [0, 1], 16)
    lp_all = np.stack([topk_spec.gen_logprobs_spec(rows, 11, [t, t], 1)[0] for t in range(300)], -1)
    assert np.allclose(np.exp(lp_all).sum(-1), 1.0, atol=1e-12) and np.all(lp_all[:, 11] == -np.inf)
    assert np.array_equal(np.take_along_axis(lp_all, ids, -1), tlp)


# ---- generate's arguments --------------------------------------------------------------------------------------------------
def _model():
    return ma.AsteroidTTSInstruct.from_state_dict(synth.tiny(), None)


def test_generate_top_logprobs_argument_checks_need_no_engine():
    m = _model()                                           # device cpu: creating an engine would raise
    ids = torch.zeros((2, 12, 8), dtype=torch.int64)
    mask = torch.ones((2, 12), dtype=torch.int64)
    for k in (0, 17, -3, 2.5, "4", True, False):
        with pytest.raises(ValueError, match="top_logprobs must be"):
            m.generate(ids, mask, max_new_tokens=4, return_dict_in_generate=True, top_logprobs=k)
        with pytest.raises(ValueError, match="top_logprobs must be"):
            m.generate(ids, mask, max_new_tokens=4, top_logprobs=k)
    with pytest.raises(ValueError, match="return_dict_in_generate"):
        m.generate(ids, mask, max_new_tokens=4, top_logprobs=5)
    with pytest.raises(ValueError, match="return_dict_in_generate"):
        m.generate(ids, mask, max_new_tokens=4, top_logprobs=5, output_scores=True)
    with pytest.raises(ValueError, match="output_logits"):   # full logits rows stay refused, with or without the new keyword
        m.generate(ids, mask, max_new_tokens=4, return_dict_in_generate=True, output_logits=True, top_logprobs=5)


def test_generate_output_fields():
    seq = torch.zeros((2, 9, 8), dtype=torch.int64)
    plain = ma.GenerateOutput(seq)
    assert plain.logprobs is None and plain.top_ids is None and plain.top_logprobs is None and plain.logits is None
    lp = torch.zeros((2, 4, 8))
    full = ma.GenerateOutput(seq, None, lp, torch.zeros((2, 4, 8, 3), dtype=torch.int64), torch.zeros((2, 4, 8, 3)))
    assert full["logprobs"] is lp and full.top_ids.shape == (2, 4, 8, 3) and full.transition_scores is None


class _StubEngine:
    """The engine calls ContinuousBatcher makes, for one poll: every dialogue finishes in its first poll with `steps` rows."""

    def __init__(self, steps):
        self.steps, self.opened, self.live = steps, [], {}

    def sched_open(self, slots, gen_cap, layers=None, do_samples=None, output_scores=False, top_logprobs=0):
        self.opened.append((bool(output_scores), int(top_logprobs)))
        self.k = int(top_logprobs)

    def kv_pool_state(self):
        return 64, 64, 8

    def submit(self, slot, ids, max_length, seed=0, row_id=0, adapter=None):
        self.live[slot] = seed

    def step(self, n):
        pass

    def slot_states(self):
        return np.zeros((4, 4), dtype=np.int32)

    def slot_read(self, slot, cap):
        return np.full((self.steps, 8), self.live[slot], dtype=np.int64)

    def slot_read_scores(self, slot, cap):
        return np.full((self.steps, 8), -float(self.live[slot]), dtype=np.float32)

    def slot_read_top_logprobs(self, slot, cap):
        s = self.live[slot]
        return (np.full((self.steps, 8), -s, np.float32), np.full((self.steps, 8, self.k), s, np.int32),
                np.full((self.steps, 8, self.k), -s, np.float32))


def test_batcher_return_value_with_and_without_the_argument():
    from mtts.scheduler import ContinuousBatcher
    eng = _StubEngine(steps=5)
    cb = ContinuousBatcher(eng, slots=4, gen_cap=32)
    prompts = [np.zeros((10, 8), dtype=np.int64)] * 3
    res = cb.run(prompts, 8, seeds=[1, 2, 3])
    assert isinstance(res, list) and len(res) == 3                 # exactly what it returned before
    res, sc = cb.run(prompts, 8, seeds=[1, 2, 3], output_scores=True)
    assert len(sc) == 3 and sc[1][0, 0] == -2.0
    res, sc, (lp, tid, tlp) = cb.run(prompts, 8, seeds=[1, 2, 3], top_logprobs=4)
    assert sc is None and [len(x) for x in (lp, tid, tlp)] == [3, 3, 3]
    assert lp[2].shape == (5, 8) and tid[2].shape == (5, 8, 4) and tlp[2].shape == (5, 8, 4) and tid[2][0, 0, 0] == 3
    res, sc, tops = cb.run(prompts, 8, seeds=[1, 2, 3], top_logprobs=4, output_scores=True)
    assert sc[0].shape == (5, 8) and tops[1][0].dtype == np.int32
    # the switches are read when the scheduler opens: one re-open per change, none without
    assert eng.opened == [(False, 0), (True, 0), (False, 4), (True, 4)]
    cb.run(prompts, 8, seeds=[1, 2, 3], top_logprobs=4, output_scores=True)
    assert len(eng.opened) == 4


# ---- the C interface -------------------------------------------------------------------------------------------------------
_CTYPE = {"int32_t": C.c_int32, "int64_t": C.c_int64, "float": C.c_float}
NEW = {"mtts_set_top_logprobs": 2, "mtts_read_top_logprobs": 6, "mtts_slot_read_top_logprobs": 7, "mtts_k_gen_topk": 11}


def _header_prototype(name):
    hdr = open(os.path.join(ROOT, "include", "mtts.h")).read()
    m = re.search(r"^(\w+)\s+%s\(([^)]*)\);" % name, hdr, re.M)
    assert m, name
    args = [" ".join(a.split()) for a in m.group(2).split(",")]
    return m.group(1), ["ptr" if "*" in a else _CTYPE[a.split()[-2]] for a in args]


@pytest.mark.parametrize("name", list(NEW))
def test_ctypes_prototypes_match_the_header(name):
    res, args = _header_prototype(name)
    got_res, got_args = capi._SIGS[name]
    kind = lambda t: "ptr" if (t is C.c_void_p or issubclass(t, C._Pointer)) else t
    assert got_res is _CTYPE[res] and [kind(t) for t in got_args] == args and len(args) == NEW[name]
    assert hasattr(capi.lib(), name)


def test_the_switch_shares_the_limit_of_the_scoring_top_k():
    hdr = open(os.path.join(ROOT, "include", "mtts.h")).read()
    assert int(re.search(r"#define MTTS_SCORE_MAX_TOPK (\d+)", hdr).group(1)) == topk_spec.MAX_TOPK == 16
