"""tests/layer_ref.py against the numpy oracle, on the seeded inputs that test_layer_kernels_gpu.py feeds the kernels: the
expectations the GPU tests compare with are the oracle's operations, the RMSNorm window holds the oracle's own fp32
result for every row, and the inputs make the summation orders observable.  No GPU."""
import numpy as np
import pytest

import layer_ref as lr
from mtts import synth
from oracle import asteroid_oracle as ao

F32 = np.float32


def _oracle(H, weights=None):
    cfg = synth.tiny(hidden_size=H)
    cfg["rms_norm_eps"] = lr.EPS
    return ao.AsteroidOracle(cfg, weights or {}, "bf16")


def _window_holds(x, w, H, what):
    """Every row of the oracle's fp32 rmsnorm is reproduced, whole, by one candidate of the window."""
    want = lr.bits(_oracle(H).rmsnorm(x, w))
    offs = lr.assert_rmsnorm_rows(want, x, w, what=what)
    return max(abs(o) for o in offs)


@pytest.mark.parametrize("H,R", lr.EMBED_CASES)
def test_embed_sum_is_the_oracles_and_its_order_shows(H, R):
    d = lr.embed_inputs(H, R)
    x = lr.embed_sum(d["tables"], d["tokens"], d["seq"])
    act = d["seq"] >= 0
    orc = _oracle(H, {f"model.embedding_list.{c}.weight": d["tables"][c] for c in range(8)})
    want = orc.embed_sum(np.where(act[:, None], d["tokens"], 0)[None])[0]
    assert np.array_equal(lr.bits(x[act]), lr.bits(want[act]))
    assert not x[~act].any()
    # the inputs: vocabulary edges, zeros, and an order of the adds that gives other bits
    assert all((d["tokens"][act][:, c] == V - 1).any() for c, V in enumerate(lr.VOCAB))
    other = lr.embed_sum(d["tables"], d["tokens"], d["seq"], order=lr.swapped(8))
    assert (lr.bits(other[0]) != lr.bits(x[0])).mean() > 0.5
    if R > 1:
        assert (d["tokens"][act] == 0).any() and not x[1].any() and (~act).any()
        assert np.abs(x[2]).max() > 2.0 ** 18
    _window_holds(x, d["w"], H, ("embed", H, R))


@pytest.mark.parametrize("H,ks,R", lr.RESID_CASES + lr.SMALL_NORM_CASES)
def test_resid_is_the_oracles_and_the_window_holds(H, ks, R):
    d = lr.resid_inputs(H, ks, R)
    x1 = lr.resid(d["slabs"], d["x"])
    if ks == 0:
        assert np.array_equal(x1, d["x"])
    else:
        # x = r(x + linear(...)): the Linear's bf16 output is the rounded slab sum
        y = lr.rbf(lr.slab_sum(d["slabs"], H))
        assert np.array_equal(lr.bits(x1), lr.bits(ao.round_bf16(d["x"] + y)))
        assert np.isnan(d["slabs"][:, :, H:]).all() and np.isfinite(x1).all()
    if ks >= 3:                                    # another slab order gives other bits in the cancellation row
        other = lr.resid(d["slabs"], d["x"], order=lr.swapped(ks))
        assert (lr.bits(other[0]) != lr.bits(x1[0])).mean() > 0.5
    assert not (d["seq"] == np.arange(R)).any() and d["seq"].max() < d["nseq"]
    live = d["seq"][d["seq"] >= 0]
    assert len(set(live.tolist())) == live.size
    if R > 1:
        assert not x1[1].any() and (x1[:, 5] == 0).all()
    if R > 2:
        assert np.abs(x1[2]).max() > 2.0 ** 18
    if R >= 5:
        assert (d["seq"] < 0).any() and d["last"][d["seq"] < 0].any()
    _window_holds(x1, d["w"], H, ("resid", H, ks, R))


def test_resid_of_one_slab_is_the_oracles_residual_linear():
    """One slab = the fp32 product: resid is `x = r(x + linear(o, W))` of forward_hidden."""
    rng = np.random.default_rng(5)
    H, K, R = 256, 512, 7
    orc = _oracle(H)
    w, o = lr.gemm_inputs(R, H, K, 5)
    x = ao.round_bf16(rng.standard_normal((R, H)).astype(F32))
    slab = np.matmul(o.astype(F32), w.T.astype(F32))[None]
    assert np.array_equal(lr.bits(lr.resid(slab, x)), lr.bits(orc.r(x + orc.linear(o, w))))


def test_window_rejects_wrong_rounding_eps_width_and_weight():
    """The candidate rule has teeth: a dropped inner rounding, a missing eps on a small row, a mean over the wrong width
    and one wrong weight element each leave no candidate that reproduces the row."""
    H = 2048
    d = lr.resid_inputs(H, 2, 5)
    x, w = lr.resid(d["slabs"], d["x"]), d["w"]
    good = lr.bits(_oracle(H).rmsnorm(x, w))
    assert all(isinstance(v, int) for v in lr.rmsnorm_match(good, x, w))
    inv = F32(1) / np.sqrt(np.mean(x.astype(np.float64) ** 2, axis=-1, keepdims=True) + lr.EPS).astype(F32)
    no_inner = lr.bits(lr.rbf(w * (x * inv)))
    assert not isinstance(lr.rmsnorm_match(no_inner, x, w)[0], int)
    inv_w = F32(1) / np.sqrt(np.sum(x.astype(np.float64) ** 2, axis=-1, keepdims=True) / (H + 16) + lr.EPS).astype(F32)
    assert not isinstance(lr.rmsnorm_match(lr.bits(lr.rmsnorm_with_inv(x, w, inv_w)), x, w)[0], int)
    w2 = w.copy()
    w2[17] = w[18]
    assert not isinstance(lr.rmsnorm_match(lr.bits(lr.rmsnorm_with_inv(x, w2, inv)), x, w)[0], int)
    tiny = lr.rbf((x[:1] * F32(2.0 ** -12)))                      # mean(x^2) ~ 6e-8: eps is most of the denominator
    inv_ne = F32(1) / np.sqrt(np.mean(tiny.astype(np.float64) ** 2, axis=-1, keepdims=True)).astype(F32)
    assert not isinstance(lr.rmsnorm_match(lr.bits(lr.rmsnorm_with_inv(tiny, w, inv_ne)), tiny, w)[0], int)


@pytest.mark.parametrize("nq", [2, 4])
@pytest.mark.parametrize("which", [0, 1])
def test_combine_inputs_and_order(nq, which):
    d = lr.combine_inputs(nq, which)
    out = lr.combine(d["opart"], d["nch"])
    assert np.isfinite(out).all()
    for r in range(4):
        assert np.isnan(d["opart"][r, :, d["nch"][r]:]).all()
        if d["nch"][r] == 0:
            assert not out[r].any()
        elif d["nch"][r] == 1:
            assert np.array_equal(lr.bits(out[r]), lr.bits(lr.rbf(d["opart"][r, :, 0]).reshape(-1)))
        if d["nch"][r] >= 3:                       # the chunk order shows
            o = lr.swapped(int(d["nch"][r]))
            other = lr.combine(d["opart"][r:r + 1][:, :, o + list(range(len(o), lr.NCHUNKS_MAX))], d["nch"][r:r + 1])
            assert (lr.bits(other[0]) != lr.bits(out[r])).mean() > 0.2
    # one chunk too many reads a NaN slot
    live = d["nch"] > 0
    more = np.where(live & (d["nch"] < lr.NCHUNKS_MAX), d["nch"] + 1, d["nch"])
    assert np.isnan(lr.combine(d["opart"], more)).any()


def test_combine_cases_cover_the_chunk_counts():
    got = set()
    for which in (0, 1):
        got |= set(lr.nch_of(lr.COMBINE_ROWS[which]["seq"], lr.COMBINE_ROWS[which]["pos"]).tolist())
    assert got == {0, 1, 8, 9, 17}


def test_swiglu_is_the_mlp_of_forward_hidden():
    """layer_ref.swiglu on the interleaved gate/up product = the MLP lines of AsteroidOracle.forward_hidden."""
    H, inter, R = 256, 160, 9
    orc = _oracle(H)
    d = lr.resid_inputs(H, 2, R)
    hn = orc.rmsnorm(lr.resid(d["slabs"], d["x"]), d["w"])
    wg, _ = lr.gemm_inputs(R, inter, H, 21)
    wu, _ = lr.gemm_inputs(R, inter, H, 22)
    gt, up = orc.linear(hn, wg), orc.linear(hn, wu)
    with np.errstate(over="ignore"):
        act = orc.r(gt / (F32(1) + np.exp(-gt, dtype=F32)))
    want = orc.r(act * up)
    wgu = np.empty((2 * inter, H), dtype=F32)
    wgu[0::2], wgu[1::2] = wg, wu
    got = lr.swiglu(np.matmul(hn.astype(F32), wgu.T.astype(F32)))
    assert np.array_equal(lr.bits(got), lr.bits(want))
