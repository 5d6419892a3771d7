"""forward(top_logprobs=k), the parts that need no GPU: the order as numpy states it (mtts/topk_spec.py), the argument
checks of AsteroidTTSInstruct.forward, its slicing of large batches, and the ctypes prototypes against include/mtts.h."""
import ctypes as C
import os
import re

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from mtts import capi, synth, topk_spec  # noqa: E402

import modeling_asteroid as ma  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the order -------------------------------------------------------------------------------------------------------------
def test_order_on_hand_made_ties():
    #                 0    1    2     3    4    5     6    7
    row = np.array([1.0, 3.0, 3.0, -2.0, 3.0, 0.5, -0.0, 0.0], dtype=np.float32)
    assert topk_spec.topk_order(row, 1).tolist() == [1]
    assert topk_spec.topk_order(row, 3).tolist() == [1, 2, 4]              # equal logits: ascending id
    assert topk_spec.topk_order(row, 8).tolist() == [1, 2, 4, 0, 5, 6, 7, 3]      # -0.0 and +0.0 are equal
    assert topk_spec.topk_order(row[::-1].copy(), 4).tolist() == [3, 5, 6, 7]
    # the first k' of the top k; rows are independent; -inf is a value like any other
    two = np.stack([row, np.array([-np.inf, 7, -np.inf, 7, 7, 7, -np.inf, 9], dtype=np.float32)])
    full = topk_spec.topk_order(two, 8)
    assert full[1].tolist() == [7, 1, 3, 4, 5, 0, 2, 6]
    for k in range(1, 9):
        assert np.array_equal(topk_spec.topk_order(two, k), full[:, :k])
    # against a plain sort on random bf16-like rows with many ties
    rng = np.random.default_rng(0)
    rows = (rng.integers(-6, 7, (5, 3, 300)) / 4).astype(np.float32)
    got = topk_spec.topk_order(rows, 16)
    for idx in np.ndindex(5, 3):
        want = sorted(range(300), key=lambda i: (-rows[idx][i], i))[:16]
        assert got[idx].tolist() == want
    ids, vals = topk_spec.topk_of_logprobs(rows, 4)
    assert np.array_equal(ids, got[..., :4]) and np.array_equal(vals, np.take_along_axis(rows, ids, -1))


def test_check_k():
    for k in (1, 5, 16, np.int64(3)):
        assert topk_spec.check_k(k) == int(k)
    for k in (0, 17, -1, 2.0, "4", True, None, [3]):
        with pytest.raises(ValueError, match="top_logprobs"):
            topk_spec.check_k(k)
    assert topk_spec.MAX_TOPK == 16


# ---- forward's arguments ---------------------------------------------------------------------------------------------------
def _model():
    return ma.AsteroidTTSInstruct.from_state_dict(synth.tiny(), None)


def _batch(B=2, T=12, lens=None, seed=0):
    rng = np.random.default_rng(seed)
    ids = np.full((B, T, 8), 1024, dtype=np.int64)
    ids[:, :, 0] = rng.integers(0, 151643, (B, T))
    ids[:, :, 1:] = rng.integers(0, 1024, (B, T, 7))
    mask = np.zeros((B, T), dtype=np.int64)
    for b in range(B):
        mask[b, :(lens[b] if lens else T)] = 1
    labels = np.where(mask[..., None] > 0, ids, -100)
    return torch.from_numpy(ids), torch.from_numpy(mask), torch.from_numpy(labels)


def test_forward_top_logprobs_argument_checks_need_no_engine():
    m = _model()                                           # device cpu: creating an engine would raise RuntimeError
    ids, mask, labels = _batch(lens=[12, 7])
    with pytest.raises(ValueError, match="keeps no logits.*generate"):    # neither labels nor top_logprobs: the old message
        m(input_ids=ids, attention_mask=mask)
    for k in (0, 17, -3, 2.5, "4", True):
        with pytest.raises(ValueError, match="top_logprobs must be"):
            m(input_ids=ids, attention_mask=mask, labels=labels, top_logprobs=k)
        with pytest.raises(ValueError, match="top_logprobs must be"):
            m(input_ids=ids, attention_mask=mask, top_logprobs=k)
    # the label-free call goes through the same checks of ids and mask
    with pytest.raises(ValueError, match="batch, seq, channels"):
        m(input_ids=ids[0], attention_mask=mask, top_logprobs=4)
    with pytest.raises(ValueError, match="left-padded"):
        m(input_ids=ids, attention_mask=torch.flip(mask, dims=[1]), top_logprobs=4)
    with pytest.raises(ValueError, match="does not take output_hidden_states"):
        m(input_ids=ids, attention_mask=mask, top_logprobs=4, output_hidden_states=True)
    # well-formed arguments get past the checks and reach the engine, which a CPU model does not have
    for kw in (dict(labels=labels), {}):
        with pytest.raises(RuntimeError, match="cuda"):
            m(input_ids=ids, attention_mask=mask, top_logprobs=16, **kw)


class _StubEngine:
    """score() fills every slot from tables keyed by the row's first channel-0 token."""

    def __init__(self, ids, lp, tid, tlp):
        self.rows = {int(ids[b, 0, 0]): b for b in range(ids.shape[0])}
        self.lp, self.tid, self.tlp = lp, tid, tlp
        self.calls = []

    def score(self, ids, mask, labels, top_k=0):
        rows = [self.rows[int(ids[b, 0, 0])] for b in range(ids.shape[0])]
        self.calls.append((ids.shape[0], labels is not None, top_k))
        lp = None if labels is None else self.lp[rows]
        return (lp, self.tid[rows][..., :top_k].astype(np.int32), self.tlp[rows][..., :top_k]) if top_k else lp


def test_forward_top_logprobs_fields_and_slices():
    m = _model()
    m.MAX_ENGINE_BATCH = 2
    ids, mask, labels = _batch(B=5, T=12, lens=[12, 2, 9, 12, 4], seed=5)
    rng = np.random.default_rng(6)
    lp = -rng.random(labels.shape).astype(np.float32) * 9
    lp[np.asarray(labels) == -100] = np.nan
    lp[:, 0] = np.nan
    tid = rng.integers(0, 1025, labels.shape + (16,))
    tlp = -np.sort(rng.random(labels.shape + (16,)).astype(np.float32), -1)
    tid[:, 0], tlp[:, 0] = -1, np.nan
    stub = _StubEngine(ids.numpy(), lp, tid, tlp)
    m._get_engine = lambda batch, need_len: stub
    plain = m(input_ids=ids, attention_mask=mask, labels=labels)
    assert plain.top_ids is None and plain.top_logprobs is None and stub.calls == [(2, True, 0), (2, True, 0), (1, True, 0)]
    stub.calls.clear()
    out = m(input_ids=ids, attention_mask=mask, labels=labels, top_logprobs=3)
    assert stub.calls == [(2, True, 3), (2, True, 3), (1, True, 3)]
    assert torch.equal(out.loss_all, plain.loss_all) and np.array_equal(out.token_logprobs.numpy(), lp, equal_nan=True)
    assert out.top_ids.dtype == torch.int64 and out.top_logprobs.dtype == torch.float32
    assert np.array_equal(out.top_ids.numpy(), tid[..., :3]) and np.array_equal(out.top_logprobs.numpy(), tlp[..., :3], equal_nan=True)
    stub.calls.clear()
    free = m(input_ids=ids, attention_mask=mask, top_logprobs=16)
    assert stub.calls == [(2, False, 16), (2, False, 16), (1, False, 16)]
    assert free.loss is None and free.loss_all is None and free.token_logprobs is None and free.logits is None
    assert np.array_equal(free.top_ids.numpy(), tid) and np.array_equal(free.top_logprobs.numpy(), tlp, equal_nan=True)
    loss, loss_all, none = m.forward(input_ids=ids, attention_mask=mask, labels=labels, top_logprobs=3, return_dict=False)
    assert none is None and torch.equal(loss_all, plain.loss_all)


# ---- the C interface -------------------------------------------------------------------------------------------------------
_CTYPE = {"int32_t": C.c_int32, "int64_t": C.c_int64, "float": C.c_float}


def _header_prototype(name):
    hdr = open(os.path.join(ROOT, "include", "mtts.h")).read()
    m = re.search(r"^(\w+)\s+%s\(([^)]*)\);" % name, hdr, re.M)
    assert m, name
    args = [" ".join(a.split()) for a in m.group(2).split(",")]
    return m.group(1), [C.c_void_p if "*" in a else _CTYPE[a.split()[-2]] for a in args]


@pytest.mark.parametrize("name", ["mtts_score_topk", "mtts_k_head_topk", "mtts_score"])
def test_ctypes_prototypes_match_the_header(name):
    res, args = _header_prototype(name)
    got_res, got_args = capi._SIGS[name]
    assert got_res is _CTYPE[res] and list(got_args) == args
    assert hasattr(capi.lib(), name)


def test_header_limits():
    hdr = open(os.path.join(ROOT, "include", "mtts.h")).read()
    assert int(re.search(r"#define MTTS_SCORE_MAX_TOPK (\d+)", hdr).group(1)) == topk_spec.MAX_TOPK
    assert len(_header_prototype("mtts_score_topk")[1]) == 11 and len(_header_prototype("mtts_k_head_topk")[1]) == 11
