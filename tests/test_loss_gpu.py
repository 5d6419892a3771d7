"""Teacher-forced scoring on the GPU: mtts_k_head_ce / mtts_score / AsteroidTTSInstruct.forward(labels=...).  -m gpu.

Three kinds of check.  The kernels against float64 numpy on inputs whose logits are EXACT (X and W entries are multiples
of 1/8 in [-1, 1], K = 256: every partial sum is a multiple of 1/64 below 2^9, exact in fp32 in any order, so the bf16
rounding of a logit is unambiguous and the only difference left is fp32 exp / log): tolerance TOL = 2e-5, the budget
test_scores_gpu.py derives for the same arithmetic (one fp32 rounding of a difference below 256, expf at 2 ulp, an fp32
sum, the log).  The replays of the reference fixtures (tests/golden/make_golden_loss.py): |logp - logp_ref| <=
2 * D_oracle + TOL at every labelled slot, D_oracle being the numpy oracle's distance from the reference stored with the
fixture -- bf16 logit noise; the same form test_scores_gpu.py uses for its reference replays.  The rest are exact
properties: a sequence's numbers do not depend on its batch, and a scoring call leaves the engine as it found it."""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from mtts import capi, synth  # noqa: E402
from oracle import asteroid_oracle as ao  # noqa: E402

import scores_ref as sr  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
TOL = sr.KERNEL_TOL
CASES = ["loss_ragged_fp32", "loss_ragged_bf16", "loss_ragged_fp16", "loss_peaked_bf16", "loss_wide_bf16"]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def neg_nanmean(logp):
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return -np.nanmean(np.asarray(logp, dtype=np.float64).reshape(-1, 8), axis=0)


# ---- 1. the kernels on exact inputs -------------------------------------------------------------------------------------
K = 256
GARBAGE = 7          # single head: rows of W beyond n_valid that hold weights the kernel must drop


@functools.lru_cache(maxsize=None)
def _head(n_valid, segments):
    """W [N, K] fp32, multiples of 1/8 in [-1, 1].  Columns 0..15 are structured so that the activation row
    (1 x 16, 0 ...) has every valid logit in [-12, -8]: W[:, :8] = -1, W[:, 8:16] in [-1/2, 0]; the padding rows of a
    single head get +1 there (logit +16), and the zero rows the packing adds give logit 0: either would move that row's
    log-sum-exp by more than 4 if it were not dropped.  One row per head is all ones beyond column 16 (a logit of ~110
    against the all-ones activation: exp overflows without the max subtraction)."""
    rng = np.random.default_rng(7000 + n_valid + segments)
    N = n_valid * segments + (GARBAGE if segments == 1 else 0)
    W = rng.integers(-8, 9, (N, K)).astype(np.float32) / 8
    W[:, :8] = -1.0
    W[:, 8:16] = rng.integers(-4, 1, (N, 8)).astype(np.float32) / 8
    if segments == 1:
        W[n_valid:, :16] = 1.0
    hot = [(s * n_valid + (n_valid * 2) // 3) for s in range(segments)]
    for h in hot:
        W[h, 16:136] = 1.0
    return W, hot


def _activations(M):
    rng = np.random.default_rng(9000 + M)
    X = rng.integers(-8, 9, (M, K)).astype(np.float32) / 8
    X[M - 1] = 0.0
    X[M - 1, :16] = 1.0                                    # every valid logit below -4
    if M >= 2:
        X[M - 2] = 0.0
        X[M - 2, :136] = 1.0                               # the hot row of W gives -8 + [-4, 0] + 120
    return X


def _labels(M, n_valid, segments):
    """Per (row, head), in turn: column 0, the last valid column, a column of the last partial 128-block, -100, random."""
    rng = np.random.default_rng(M + n_valid)
    last_block = (n_valid - 1) // 128 * 128
    lab = np.zeros((M, segments), dtype=np.int32)
    for r in range(M):
        for s in range(segments):
            lab[r, s] = [0, n_valid - 1, last_block + (n_valid - 1 - last_block) // 2, -100, int(rng.integers(0, n_valid))][(r + s) % 5]
    if M >= 2:
        lab[M - 2, 0] = (n_valid * 2) // 3                 # the hot column itself: logp close to 0
    return lab


def _k_head_ce(W, X, lab, n_valid, segments):
    wt = torch.from_numpy(W).to(torch.bfloat16).cuda()
    xt = torch.from_numpy(X).to(torch.bfloat16).cuda()
    M = X.shape[0]
    out = torch.full((M * segments,), 7.0, dtype=torch.float32, device="cuda")
    lab = np.ascontiguousarray(lab, dtype=np.int32)
    capi.check(capi.lib().mtts_k_head_ce(wt.data_ptr(), xt.data_ptr(), lab.ctypes.data, M, W.shape[0], X.shape[1], n_valid, segments,
                                          out.data_ptr(), None))
    torch.cuda.synchronize()
    return out.cpu().numpy().reshape(M, segments)


@pytest.mark.parametrize("M", [1, 31, 33, 130])
@pytest.mark.parametrize("head", ["1025", "5000", "152697", "7x1025"])
def test_head_ce_kernel_vs_fp64(head, M):
    segments, n_valid = (7, 1025) if head == "7x1025" else (1, int(head))
    W, hot = _head(n_valid, segments)
    X = _activations(M)
    lab = _labels(M, n_valid, segments)
    got = _k_head_ce(W, X, lab, n_valid, segments)
    logits = X.astype(np.float64) @ W.astype(np.float64).T                 # exact
    assert np.array_equal(logits, logits.astype(np.float32))
    worst = 0.0
    for s in range(segments):
        lg = ao.round_bf16(logits[:, s * n_valid:(s + 1) * n_valid].astype(np.float32)).astype(np.float64)
        if s == 0:
            assert lg[M - 1].max() < -4 and (M < 2 or lg[M - 2].max() > 100)
        m = lg.max(-1, keepdims=True)
        lse = (m + np.log(np.exp(lg - m).sum(-1, keepdims=True)))[:, 0]
        for r in range(M):
            if lab[r, s] < 0:
                assert np.isnan(got[r, s]), (head, M, r, s)
                continue
            want = lg[r, lab[r, s]] - lse[r]
            assert np.isfinite(got[r, s]), (head, M, r, s)
            worst = max(worst, abs(float(got[r, s]) - want))
            assert abs(float(got[r, s]) - want) <= TOL, (head, M, r, s, float(got[r, s]), want)
    print(f"head_ce {head} M={M}: max |logp - fp64| = {worst:.3g}")
    # a row's result does not depend on the rows that share its launch
    if M == 130:
        for r0, n in ((0, 1), (32, 33), (97, 33)):
            alone = _k_head_ce(W, X[r0:r0 + n], lab[r0:r0 + n], n_valid, segments)
            assert np.array_equal(_bits(alone), _bits(got[r0:r0 + n]))


def test_head_ce_kernel_k_tail():
    """K = 272 is 17 k-tiles: two unrolled groups of 8 and one through the main loop's remainder path (K = 256 and the
    engines' hidden sizes are whole groups).  272 products of multiples of 1/64 still sum exactly in fp32."""
    rng = np.random.default_rng(272)
    Kt, M, n_valid = 272, 33, 1025
    W = rng.integers(-8, 9, (n_valid, Kt)).astype(np.float32) / 8
    X = rng.integers(-8, 9, (M, Kt)).astype(np.float32) / 8
    lab = _labels(M, n_valid, 1)
    got = _k_head_ce(W, X, lab, n_valid, 1)
    lg = ao.round_bf16((X.astype(np.float64) @ W.astype(np.float64).T).astype(np.float32)).astype(np.float64)
    m = lg.max(-1, keepdims=True)
    want = np.take_along_axis(lg, np.maximum(lab, 0), -1)[:, 0] - (m + np.log(np.exp(lg - m).sum(-1, keepdims=True)))[:, 0]
    keep = lab[:, 0] >= 0
    assert np.isnan(got[~keep, 0]).all() and np.abs(got[keep, 0] - want[keep]).max() <= TOL


# ---- 2. the reference's forward(labels=...) ------------------------------------------------------------------------------
def _load(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    cfg = json.loads(str(z["cfg"]))
    dtype = str(z["dtype"])
    w = synth.synth_weights(cfg, int(z["seed"]), bf16=(dtype == "bf16"), **json.loads(str(z["wkw"])))
    return z, cfg, dtype, w


def _engine(cfg, w, dtype="bf16", **kw):
    from mtts.engine import Engine
    kw.setdefault("max_batch", 4)
    kw.setdefault("max_seq_len", 256)
    eng = Engine(cfg, dtype=dtype, **kw)
    eng.bind_state_dict(w)
    return eng


@functools.lru_cache(maxsize=None)
def _scored(name):
    """One scoring call per fixture, shared by the tests below -> (fixture, logp [B,T,8])."""
    z, cfg, dtype, w = _load(name)
    eng = _engine(cfg, w, dtype)
    try:
        return z, eng.score(z["input_ids"], z["attention_mask"], z["labels"])
    finally:
        eng.close()


def _record(name, **figures):
    path = os.path.join(ROOT, "profiles", "score_parity.json")
    rec = json.load(open(path)) if os.path.exists(path) else {}
    rec.setdefault(name, {}).update(figures)
    with open(path, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")


@pytest.mark.parametrize("name", CASES)
def test_score_vs_reference(name):
    z, logp = _scored(name)
    ref = z["logp_ref"]
    D, Dl = float(z["D_oracle"]), float(z["D_oracle_loss"])
    assert logp.shape == ref.shape and logp.dtype == np.float32
    assert np.array_equal(np.isnan(logp), np.isnan(ref))                  # NaN exactly where the fixture has NaN
    d = np.abs(logp.astype(np.float64) - ref.astype(np.float64))
    dmax = float(np.nanmax(d))
    loss_all = neg_nanmean(logp)
    dloss = float(np.abs(loss_all - z["loss_all"].astype(np.float64)).max())
    print(f"{name}: max |logp - ref| = {dmax:.3g} (2 D + TOL = {2 * D + TOL:.3g}), max |loss_all - ref| = {dloss:.3g} "
          f"(2 D_loss + TOL = {2 * Dl + TOL:.3g}), {int(np.isfinite(ref).sum())} slots")
    _record(name, max_abs_logp_diff=dmax, max_abs_loss_all_diff=dloss, D_oracle=D, D_oracle_loss=Dl,
            slots=int(np.isfinite(ref).sum()), tol_logp=2 * D + TOL, tol_loss=2 * Dl + TOL)
    assert dmax <= 2 * D + TOL                                            # every labelled slot
    assert dloss <= 2 * Dl + TOL


# ---- 3. exact properties ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["loss_ragged_bf16", "loss_ragged_fp32"])
def test_score_does_not_depend_on_the_batch(name):
    z, cfg, dtype, w = _load(name)
    ids, mask, labels = z["input_ids"], z["attention_mask"], z["labels"]
    eng = _engine(cfg, w, dtype)
    try:
        full = eng.score(ids, mask, labels)
        again = eng.score(ids, mask, labels)
        assert np.array_equal(_bits(full), _bits(again))                  # two calls in a row
        assert np.array_equal(_bits(full), _bits(_scored(name)[1]))       # and another engine
        for b in range(ids.shape[0]):                                     # alone and unpadded
            n = int(mask[b].sum())
            alone = eng.score(ids[b:b + 1, :n], mask[b:b + 1, :n], labels[b:b + 1, :n])
            assert np.array_equal(_bits(alone[0]), _bits(full[b, :n])), b
        rev = eng.score(ids[::-1], mask[::-1], labels[::-1])              # batch order
        assert np.array_equal(_bits(rev[::-1]), _bits(full))
    finally:
        eng.close()


def test_score_across_prefill_passes():
    """3 x 800 tokens are 2400 staged rows: more than one 2048-row prefill pass, the second sequence's pages written by
    both.  Each sequence equals itself scored alone (one pass)."""
    z, cfg, dtype, w = _load("loss_ragged_bf16")
    rng = np.random.default_rng(77)
    B, T = 3, 800
    ids = np.full((B, T, 8), 1024, dtype=np.int64)
    ids[:, :, 0] = rng.integers(0, 151643, (B, T))
    ids[:, :, 1:] = rng.integers(0, 1024, (B, T, 7))
    mask = np.ones((B, T), dtype=np.uint8)
    labels = ids.copy()
    labels[rng.random(labels.shape) < 0.1] = -100
    eng = _engine(cfg, w, dtype, max_batch=4, max_seq_len=832)
    try:
        full = eng.score(ids, mask, labels)
        assert np.array_equal(np.isnan(full[:, 1:]), labels[:, 1:] == -100) and np.isnan(full[:, 0]).all()
        for b in range(B):
            alone = eng.score(ids[b:b + 1], mask[b:b + 1], labels[b:b + 1])
            assert np.array_equal(_bits(alone[0]), _bits(full[b])), b
    finally:
        eng.close()


# ---- 4. the engine is left as it was found ---------------------------------------------------------------------------------
def test_score_leaves_the_engine_untouched():
    z, cfg, dtype, w = _load("loss_ragged_bf16")
    g = np.load(os.path.join(GOLDEN, "ar_text_ragged.npz"))
    gw = synth.synth_weights(json.loads(str(g["cfg"])), int(g["seed"]), **json.loads(str(g["wkw"])))
    assert json.loads(str(g["cfg"])) == cfg
    eng = _engine(cfg, gw, "bf16")
    try:
        free0 = eng.kv_pool_state()[1]
        before = eng.generate(g["input_ids"], g["attention_mask"], int(g["max_length"]))
        assert np.array_equal(before, g["out_ids"])
        free1 = eng.kv_pool_state()[1]
        lp = eng.score(z["input_ids"], z["attention_mask"], z["labels"])
        assert np.isfinite(lp).sum() == np.isfinite(z["logp_ref"]).sum()
        assert eng.kv_pool_state()[1] == free1
        after = eng.generate(g["input_ids"], g["attention_mask"], int(g["max_length"]))
        assert np.array_equal(after, before)
        assert eng.kv_pool_state()[1] == free1 and free1 <= free0
        # a run is open: begin without its steps
        eng.begin(g["input_ids"], g["attention_mask"], int(g["max_length"]))
        with pytest.raises(capi.MttsError) as ei:
            eng.score(z["input_ids"], z["attention_mask"], z["labels"])
        assert ei.value.code == capi.ESTATE
        eng.step(3)
        eng.sched_open(4, 64)                              # ends the abandoned run (include/mtts.h: mtts_set_output_scores)
        assert np.array_equal(_bits(eng.score(z["input_ids"], z["attention_mask"], z["labels"])), _bits(lp))
        assert np.array_equal(eng.generate(g["input_ids"], g["attention_mask"], int(g["max_length"])), before)
    finally:
        eng.close()


def test_score_argument_errors():
    z, cfg, dtype, w = _load("loss_ragged_bf16")
    ids, mask, labels = z["input_ids"], z["attention_mask"].astype(np.uint8), z["labels"]
    eng = _engine(cfg, w, dtype, max_batch=3, max_seq_len=200)
    try:
        free = eng.kv_pool_state()[1]

        def einval(i, m, l, match):
            with pytest.raises(capi.MttsError, match=match) as ei:
                eng.score(i, m, l)
            assert ei.value.code == capi.EINVAL
            assert eng.kv_pool_state()[1] == free

        einval(ids[:, ::-1], mask[:, ::-1], labels[:, ::-1], "left-padded")
        holes = mask.copy()
        holes[0, 50] = 0
        l2 = labels.copy()
        l2[0, 50] = -100
        einval(ids, holes, l2, "ones followed by zeros")
        bad = labels.copy()
        bad[2, 100, 3] = 17
        einval(ids, mask, bad, "masked position")
        bad = labels.copy()
        bad[0, 10, 1] = 1025
        einval(ids, mask, bad, r"outside \[0, 1025\)")
        bad = labels.copy()
        bad[0, 10, 0] = -5
        einval(ids, mask, bad, "outside")
        four = lambda a: np.concatenate([a, a[:1]])
        einval(four(ids), four(mask), four(labels), "max_batch")
        wide = lambda a, v: np.concatenate([a, np.full_like(a[:, :1], v)], axis=1)
        einval(wide(ids, 0), wide(mask, 0), wide(labels, -100), "max_seq_len")
        assert np.isfinite(eng.score(ids, mask, labels)).sum() == np.isfinite(z["logp_ref"]).sum()
    finally:
        eng.close()
    small = _engine(cfg, w, dtype, max_batch=3, max_seq_len=200, kv_pool_pages=5)      # the batch needs 4 + 3 + 1 pages
    try:
        with pytest.raises(capi.MttsError, match="KV pages") as ei:
            small.score(ids, mask, labels)
        assert ei.value.code == capi.ENOMEM and small.kv_pool_state()[1] == 5
        one = small.score(ids[:1], mask[:1], labels[:1])
        assert np.array_equal(_bits(one[0]), _bits(_scored("loss_ragged_bf16")[1][0]))
    finally:
        small.close()


# ---- 5. the product surface ------------------------------------------------------------------------------------------------
def test_model_forward_returns_the_reference_losses():
    import modeling_asteroid as ma
    z, cfg, dtype, w = _load("loss_ragged_bf16")
    model = ma.AsteroidTTSInstruct.from_state_dict(cfg, w).eval().to("cuda")
    ids, mask, labels = (torch.from_numpy(z[k]) for k in ("input_ids", "attention_mask", "labels"))
    out = model(input_ids=ids, attention_mask=mask, labels=labels)
    Dl = float(z["D_oracle_loss"])
    assert out.loss_all.dtype == torch.float32 and out.loss_all.device.type == "cuda" and tuple(out.loss_all.shape) == (8,)
    assert np.abs(out.loss_all.cpu().numpy().astype(np.float64) - z["loss_all"]).max() <= 2 * Dl + TOL
    assert abs(float(out.loss) - float(z["loss"])) <= 2 * Dl + TOL
    assert np.array_equal(np.isnan(out.token_logprobs.numpy()), np.isnan(z["logp_ref"]))
    assert np.array_equal(_bits(out.token_logprobs.numpy()), _bits(_scored("loss_ragged_bf16")[1]))
    assert out.logits is None and out.logits_all is None and out.past_key_values is None
    loss, loss_all, none = model.forward(input_ids=ids, attention_mask=mask, labels=labels, return_dict=False)
    assert none is None and torch.equal(loss_all, out.loss_all) and float(loss) == float(out.loss)
    model._engine.close()
