"""Teacher-forced loss, the parts that need no GPU: the fixtures are coherent, the numpy oracle reproduces them, and
AsteroidTTSInstruct.forward checks its arguments and reduces per-token log-probabilities the way the reference's
forward(labels=...) does (modeling_asteroid.py:382-410)."""
import json
import os
import warnings

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from mtts import synth  # noqa: E402
from oracle import asteroid_oracle as ao  # noqa: E402

import modeling_asteroid as ma  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = ["loss_ragged_fp32", "loss_ragged_bf16", "loss_ragged_fp16", "loss_peaked_bf16", "loss_wide_bf16"]
TINY = CASES[:4]


def neg_nanmean(logp):
    """[..., 8] -> float64 [8]: -(mean of the non-NaN entries) per channel."""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return -np.nanmean(np.asarray(logp, dtype=np.float64).reshape(-1, 8), axis=0)


def logp_of(logits_all, labels):
    """8 x [B,T,V_c] fp32 logits -> [B,T,8]: float64 log-softmax of position t - 1 at labels[t]; NaN at t = 0 / -100."""
    B, T, _ = labels.shape
    out = np.full((B, T, 8), np.nan)
    for c, lg in enumerate(logits_all):
        lg = lg[:, :-1].astype(np.float64)
        m = lg.max(-1, keepdims=True)
        lse = (m + np.log(np.exp(lg - m).sum(-1, keepdims=True)))[..., 0]
        tgt = labels[:, 1:, c]
        keep = tgt != -100
        pick = np.take_along_axis(lg, np.maximum(tgt, 0)[..., None], -1)[..., 0]
        out[:, 1:, c][keep] = (pick - lse)[keep]
    return out


@pytest.mark.parametrize("name", CASES)
def test_fixture_is_coherent(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    ids, mask, labels, logp = z["input_ids"], z["attention_mask"], z["labels"], z["logp_ref"]
    assert ids.shape == labels.shape == logp.shape and mask.shape == ids.shape[:2]
    lens = mask.sum(1)
    for b in range(ids.shape[0]):                          # right-padded
        assert mask[b, :lens[b]].all() and not mask[b, lens[b]:].any()
        assert (labels[b, lens[b]:] == -100).all()
    want_nan = labels == -100
    want_nan[:, 0] = True
    assert np.array_equal(np.isnan(logp), want_nan)
    assert np.abs(neg_nanmean(logp) - z["loss_all"].astype(np.float64)).max() <= 5e-6
    assert abs(float(z["loss_all"].astype(np.float64).mean()) - float(z["loss"])) <= 5e-6      # weights [1] * 8


@pytest.mark.parametrize("name", TINY)
def test_oracle_reproduces_reference_logp(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    cfg = json.loads(str(z["cfg"]))
    dtype = str(z["dtype"])
    w = synth.synth_weights(cfg, int(z["seed"]), bf16=(dtype == "bf16"), **json.loads(str(z["wkw"])))
    ids, mask, labels = z["input_ids"], z["attention_mask"], z["labels"]
    B, T, _ = ids.shape
    orc = ao.AsteroidOracle(cfg, w, dtype)
    got = logp_of(orc.forward(ids, np.broadcast_to(np.arange(T), (B, T)), mask, all_positions=True), labels)
    ref = z["logp_ref"].astype(np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(ref))
    d = float(np.nanmax(np.abs(got - ref)))
    print(f"{name}: max |oracle - reference| = {d:.3g} (stored D_oracle {float(z['D_oracle']):.3g})")
    assert d <= float(z["D_oracle"]) + 1e-6                 # (the fixture's logp_ref is stored as float32)


# ---- AsteroidTTSInstruct.forward ---------------------------------------------------------------------------------------
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


def test_forward_argument_checks_need_no_engine():
    m = _model()                                           # device cpu: creating an engine would raise RuntimeError
    ids, mask, labels = _batch(lens=[12, 7])
    with pytest.raises(ValueError, match="keeps no logits.*generate"):
        m(input_ids=ids, attention_mask=mask)
    with pytest.raises(ValueError, match="batch, seq, channels"):
        m(input_ids=ids[0], attention_mask=mask, labels=labels[0])
    with pytest.raises(ValueError, match="Expected 8 channels"):
        m(input_ids=ids[..., :7], attention_mask=mask, labels=labels[..., :7])
    with pytest.raises(ValueError, match="shaped like input_ids"):
        m(input_ids=ids, attention_mask=mask, labels=labels[:, :-1])
    with pytest.raises(ValueError, match="attention_mask must be"):
        m(input_ids=ids, attention_mask=mask[:, :-1], labels=labels)
    with pytest.raises(ValueError, match="left-padded"):
        m(input_ids=ids, attention_mask=torch.flip(mask, dims=[1]), labels=torch.flip(labels, dims=[1]))
    holes = mask.clone()
    holes[0, 3] = 0
    lab2 = labels.clone()
    lab2[0, 3] = -100
    with pytest.raises(ValueError, match="ones followed by zeros"):
        m(input_ids=ids, attention_mask=holes, labels=lab2)
    bad = labels.clone()
    bad[1, 9, 2] = 5                                       # a label where the mask is 0
    with pytest.raises(ValueError, match="-100 wherever attention_mask is 0"):
        m(input_ids=ids, attention_mask=mask, labels=bad)
    bad = labels.clone()
    bad[0, 2, 3] = 1025                                    # outside the speech vocabulary
    with pytest.raises(ValueError, match="vocabulary"):
        m(input_ids=ids, attention_mask=mask, labels=bad)
    for kw in (dict(position_ids=torch.arange(12)[None].expand(2, 12)), dict(inputs_embeds=torch.zeros(2, 12, 4)),
               dict(skip_logits=False), dict(output_hidden_states=True)):
        with pytest.raises(ValueError, match="does not take " + next(iter(kw))):
            m(input_ids=ids, attention_mask=mask, labels=labels, **kw)
    # well-formed arguments get past the checks and reach the engine, which a CPU model does not have
    with pytest.raises(RuntimeError, match="cuda"):
        m(input_ids=ids, attention_mask=mask, labels=labels)


class _StubEngine:
    """score() looks every row up in a table of per-token log-probabilities, keyed by the row's first channel-0 token."""

    def __init__(self, ids, table):
        self.rows = {int(ids[b, 0, 0]): table[b] for b in range(ids.shape[0])}
        self.calls = []

    def score(self, ids, mask, labels):
        self.calls.append(ids.shape[0])
        out = np.stack([self.rows[int(ids[b, 0, 0])] for b in range(ids.shape[0])]).astype(np.float32)
        assert np.array_equal(np.isnan(out[:, 1:]), np.asarray(labels)[:, 1:] == -100)
        return out


def _table(labels, seed):
    rng = np.random.default_rng(seed)
    lp = -rng.random(labels.shape).astype(np.float32) * 9
    lp[np.asarray(labels) == -100] = np.nan
    lp[:, 0] = np.nan
    return lp


def test_forward_losses_and_set_weights():
    m = _model()
    ids, mask, labels = _batch(B=3, T=12, lens=[12, 7, 3], seed=1)
    labels[:, :, 5] = -100                                 # a channel without a label: NaN, as cross_entropy's mean
    lp = _table(labels, 2)
    stub = _StubEngine(ids.numpy(), lp)
    m._get_engine = lambda batch, need_len: stub
    out = m(input_ids=ids, attention_mask=mask, labels=labels)
    want = neg_nanmean(lp).astype(np.float32)
    assert isinstance(out, ma.AsteroidTTSOutputWithPast)
    assert out.loss_all.dtype == torch.float32 and tuple(out.loss_all.shape) == (8,)
    assert np.array_equal(out.loss_all.numpy(), want, equal_nan=True) and np.isnan(want[5])
    assert torch.isnan(out.loss)                           # the reference's weighted sum carries the NaN
    assert out.logits is None and out.logits_all is None and out.past_key_values is None
    assert out.hidden_states is None and out.attentions is None
    assert np.array_equal(out.token_logprobs.numpy(), lp, equal_nan=True)
    # with every channel labelled: loss = sum w_c / sum(w) * loss_all[c]
    ids, mask, labels = _batch(B=3, T=12, lens=[12, 7, 3], seed=3)
    lp = _table(labels, 4)
    stub = _StubEngine(ids.numpy(), lp)
    want = torch.from_numpy(neg_nanmean(lp).astype(np.float32))
    out = m(input_ids=ids, attention_mask=mask, labels=labels)
    assert m.weights == [1] * 8
    assert abs(float(out.loss) - float(want.double().mean())) <= 1e-6
    m.set_weights([4, 1, 1, 1, 0.5, 0.5, 0, 0])
    loss, loss_all, none = m.forward(input_ids=ids, attention_mask=mask, labels=labels, return_dict=False)
    assert none is None and torch.equal(loss_all, want)
    ref = 0
    for w, l in zip([w / 8.0 for w in m.weights], want):   # modeling_asteroid.py:405-410
        ref = ref + w * l
    assert float(loss) == float(ref)
    assert abs(float(loss) - float((torch.tensor(m.weights).double() / 8 * want.double()).sum())) <= 1e-6


def test_forward_slices_large_batches_and_combines_sums_and_counts():
    m = _model()
    m.MAX_ENGINE_BATCH = 2
    ids, mask, labels = _batch(B=5, T=12, lens=[12, 2, 9, 12, 4], seed=5)
    lp = _table(labels, 6)
    stub = _StubEngine(ids.numpy(), lp)
    m._get_engine = lambda batch, need_len: stub
    out = m(input_ids=ids, attention_mask=mask, labels=labels)
    assert stub.calls == [2, 2, 1]
    whole = neg_nanmean(lp)
    of_means = np.mean([neg_nanmean(lp[i:i + 2]) for i in (0, 2, 4)], axis=0)
    assert np.abs(whole - of_means).max() > 1e-2           # the slices hold different numbers of labels
    assert np.array_equal(out.loss_all.numpy(), whole.astype(np.float32))
    assert np.array_equal(out.token_logprobs.numpy(), lp, equal_nan=True)
