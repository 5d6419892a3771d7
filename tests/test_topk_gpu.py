"""Top-k log-probabilities from teacher-forced scoring: mtts_k_head_topk / mtts_score_topk / Engine.score(top_k=) /
AsteroidTTSInstruct.forward(top_logprobs=).  -m gpu.

The kernels run on test_loss_gpu.py's exact inputs (X and W multiples of 1/8, K = 256: every logit is exact in fp32 in any
order of summation, so its bf16 rounding is unambiguous and ties are abundant): the returned ids must EQUAL numpy's top k
under (descending logit, ascending id) -- mtts/topk_spec.py -- and the log-probabilities lie within scores_ref.KERNEL_TOL
of float64, the budget of the same fp32 exp / sum / log the scoring kernels are held to.  Everything else is bitwise: a
returned log-probability is the number mtts_k_head_ce / Engine.score gives for that id as the label, and a row's result
does not depend on the launch, the batch, the prefill pass or k."""
import functools
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from mtts import capi, synth, topk_spec  # noqa: E402
from oracle import asteroid_oracle as ao  # noqa: E402

import scores_ref as sr  # noqa: E402
import test_loss_gpu as tl  # noqa: E402  (the exact-input construction and the fixture helpers)

TOL = sr.KERNEL_TOL
GOLDEN = tl.GOLDEN
_bits = tl._bits
KMAX = topk_spec.MAX_TOPK
K_EXACT = tl.K
HEADS = ["1025", "5000", "152697", "7x1025"]


def _shape(head):
    return (7, 1025) if head == "7x1025" else (1, int(head))


# ---- 1. the kernels on exact inputs -------------------------------------------------------------------------------------
def _k_head_topk(W, X, n_valid, segments, k):
    """-> ids int32 [M, segments, k], logp float32 [M, segments, k]; W, X numpy fp32 or cuda bf16 tensors."""
    wt = W if torch.is_tensor(W) else torch.from_numpy(W).to(torch.bfloat16).cuda()
    xt = X if torch.is_tensor(X) else torch.from_numpy(X).to(torch.bfloat16).cuda()
    M = xt.shape[0]
    ids = torch.full((M * segments * k,), -7, dtype=torch.int32, device="cuda")
    lp = torch.full((M * segments * k,), 7.0, dtype=torch.float32, device="cuda")
    capi.check(capi.lib().mtts_k_head_topk(wt.data_ptr(), xt.data_ptr(), M, wt.shape[0], xt.shape[1], n_valid, segments, k,
                                           ids.data_ptr(), lp.data_ptr(), None))
    torch.cuda.synchronize()
    return ids.cpu().numpy().reshape(M, segments, k), lp.cpu().numpy().reshape(M, segments, k)


def _expect(W, X, n_valid, segments):
    """The exact bf16 logits [M, segments, n_valid] (float32), their float64 log-sum-exp [M, segments] and the ids of the
    KMAX best [M, segments, KMAX].  A float32 matmul is exact here whatever its order (see the module docstring)."""
    logits = X @ W[:segments * n_valid].T if segments > 1 else X @ W[:n_valid].T
    lg = ao.round_bf16(logits.astype(np.float32)).reshape(X.shape[0], segments, n_valid)
    l64 = lg.astype(np.float64)
    m = l64.max(-1, keepdims=True)
    lse = (m + np.log(np.exp(l64 - m).sum(-1, keepdims=True)))[..., 0]
    return lg, lse, topk_spec.topk_order(lg, KMAX)


@functools.lru_cache(maxsize=4)
def _case(head, M):
    segments, n_valid = _shape(head)
    W, hot = tl._head(n_valid, segments)
    X = tl._activations(M)
    assert np.array_equal((X[:2].astype(np.float64) @ W[:64].astype(np.float64).T).astype(np.float32), X[:2] @ W[:64].T)
    return W, hot, X, _expect(W, X, n_valid, segments)


@functools.lru_cache(maxsize=2)
def _dev(head):
    segments, n_valid = _shape(head)
    return torch.from_numpy(tl._head(n_valid, segments)[0]).to(torch.bfloat16).cuda()


def _check(ids, lp, lg, lse, want_ids, k, where):
    """ids equal, every id a valid column, log-probabilities within TOL of float64."""
    assert ids.dtype == np.int32 and lp.dtype == np.float32
    assert np.array_equal(ids, want_ids[..., :k]), where
    want = np.take_along_axis(lg.astype(np.float64), want_ids[..., :k], -1) - lse[..., None]
    worst = float(np.abs(lp.astype(np.float64) - want).max())
    print(f"head_topk {where}: max |logp - fp64| = {worst:.3g}")
    assert np.isfinite(lp).all() and worst <= TOL, (where, worst)


@pytest.mark.parametrize("k", [1, 5, 16])
@pytest.mark.parametrize("M", [1, 33, 130])
@pytest.mark.parametrize("head", HEADS)
def test_head_topk_kernel_vs_fp64(head, M, k):
    segments, n_valid = _shape(head)
    W, hot, X, (lg, lse, want_ids) = _case(head, M)
    xt = torch.from_numpy(X).to(torch.bfloat16).cuda()
    ids, lp = _k_head_topk(_dev(head), xt, n_valid, segments, k)
    # the garbage rows of W beyond n_valid (logit +16 on the last row) and the packing's zero rows (logit 0) never appear:
    # every valid logit of the last row is below -4
    assert ids.min() >= 0 and ids.max() < n_valid and lg[M - 1].max() < -4
    _check(ids, lp, lg, lse, want_ids, k, (head, M, k))
    if M >= 2:                                             # the hot column wins the hot row, in every head
        assert lg[M - 2].max() > 100
        assert np.array_equal(ids[M - 2, :, 0], np.array(hot) - np.arange(segments) * n_valid)
    if M == 130:                                           # a row's result does not depend on the rows that share its launch
        for r0, n in ((0, 1), (32, 33), (97, 33)):
            ai, al = _k_head_topk(_dev(head), xt[r0:r0 + n].contiguous(), n_valid, segments, k)
            assert np.array_equal(ai, ids[r0:r0 + n]) and np.array_equal(_bits(al), _bits(lp[r0:r0 + n])), (r0, n)
    if k == 5:                                             # nor on k: the first five of the top 16
        i16, l16 = _k_head_topk(_dev(head), xt, n_valid, segments, 16)
        assert np.array_equal(i16[..., :5], ids) and np.array_equal(_bits(l16[..., :5]), _bits(lp))


def test_head_topk_k_tail():
    """K = 272: the main loop's remainder path (test_loss_gpu.py: test_head_ce_kernel_k_tail)."""
    rng = np.random.default_rng(272)
    Kt, M, n_valid = 272, 33, 1025
    W = rng.integers(-8, 9, (n_valid, Kt)).astype(np.float32) / 8
    X = rng.integers(-8, 9, (M, Kt)).astype(np.float32) / 8
    lg, lse, want_ids = _expect(W, X, n_valid, 1)
    ids, lp = _k_head_topk(W, X, n_valid, 1, 16)
    _check(ids, lp, lg, lse, want_ids, 16, "K=272")


# Columns whose W rows are copies of column 0's: equal logits on every row.  Inside a block a lane holds the columns
# {0..3, 8..11, 16..19, 24..27} (+4 for lane ^ 32) of each 32-column tile, a wave 64 columns, a block 128; the finishing
# wave's lane j merges the blocks j, j + 64, ...
TIE_COLS = {
    1: "the same lane's registers", 33: "the same lane, its second tile", 4: "lane ^ 32", 64: "the other wave of the block",
    131: "the next block (another lane of the finish)", 8192: "block 64: the same lane of the finish as block 0",
    8999: "the last, partial block",
}


def test_head_topk_ties_everywhere():
    """A 9000-column head (71 blocks) in which the columns of TIE_COLS duplicate column 0, and column 0 is the hot one: on
    the hot row the eight tie for rank 0 and must come out in ascending id; on every other row they tie wherever they
    rank.  On the last-but-two row 16 columns of block 3 alone are raised above everything else."""
    n_valid, M = 9000, 34
    W, hot = tl._head(n_valid, 1)
    W = W.copy()
    W[hot[0]] = W[hot[0] - 1]                              # no other hot column
    W[0, 16:136] = 1.0
    for c in TIE_COLS:
        W[c] = W[0]
    X = tl._activations(M).copy()
    X[M - 3] = 0.0
    X[M - 3, 136:256] = 1.0                                # the row that looks at columns 136..255 of W only
    W[:, 136:256] = np.minimum(W[:, 136:256], 0.5)
    for j in range(16):                                    # 16 distinct values of 75..105, far above 120 x 1/2
        W[384 + 5 * j, 136:256] = 0.5
        W[384 + 5 * j, 136:136 + 30 + 4 * j] = 1.0
    lg, lse, want_ids = _expect(W, X, n_valid, 1)
    tied = sorted([0] + list(TIE_COLS))
    assert want_ids[M - 2, 0, :8].tolist() == tied and len(set(lg[M - 2, 0, tied].tolist())) == 1
    assert sorted(want_ids[M - 3, 0].tolist()) == [384 + 5 * j for j in range(16)]      # all of one block
    for k in (1, 5, 16):
        ids, lp = _k_head_topk(W, X, n_valid, 1, k)
        _check(ids, lp, lg, lse, want_ids, k, ("ties", k))


def test_head_topk_best_in_the_one_column_block():
    """n_valid = 1025: the ninth block of a head holds column 1024 alone, and fills the rest of its list with nothing."""
    for segments in (1, 7):
        W, hot = tl._head(1025, segments)
        W = W.copy()
        for s, h in enumerate(hot):
            W[h] = W[h - 1]
            W[s * 1025 + 1024, 16:136] = 1.0
        X = tl._activations(33)
        lg, lse, want_ids = _expect(W, X, 1025, segments)
        assert (want_ids[31, :, 0] == 1024).all()
        for k in (1, 16):
            ids, lp = _k_head_topk(W, X, 1025, segments, k)
            _check(ids, lp, lg, lse, want_ids, k, ("last block", segments, k))


def test_head_topk_argument_errors():
    W, _ = tl._head(1025, 1)
    X = tl._activations(2)
    for k in (0, 17):
        with pytest.raises(capi.MttsError) as ei:
            _k_head_topk(W, X, 1025, 1, k)
        assert ei.value.code == capi.EINVAL
    with pytest.raises(capi.MttsError) as ei:                             # fewer columns than k
        _k_head_topk(W, X, 3, 1, 4)
    assert ei.value.code == capi.EINVAL


# ---- 2. the exactness contract at kernel level ---------------------------------------------------------------------------
@pytest.mark.parametrize("head", HEADS)
def test_head_topk_logp_is_head_ce_of_the_id(head):
    segments, n_valid = _shape(head)
    M, k = 33, 16
    W, hot, X, _ = _case(head, M)
    wt, xt = _dev(head), torch.from_numpy(X).to(torch.bfloat16).cuda()
    ids, lp = _k_head_topk(wt, xt, n_valid, segments, k)
    out = torch.empty(M * segments, dtype=torch.float32, device="cuda")
    for j in range(k):
        lab = np.ascontiguousarray(ids[:, :, j], dtype=np.int32)
        capi.check(capi.lib().mtts_k_head_ce(wt.data_ptr(), xt.data_ptr(), lab.ctypes.data, M, wt.shape[0], K_EXACT, n_valid, segments,
                                             out.data_ptr(), None))
        assert np.array_equal(_bits(out.cpu().numpy().reshape(M, segments)), _bits(lp[:, :, j])), (head, j)


# ---- 3. the engine: the speech channels exhaustively ---------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _top16(name):
    """One top_k = 16 call with labels per fixture, shared by the tests below -> (fixture, logp, top_ids, top_logp)."""
    z, cfg, dtype, w = tl._load(name)
    eng = tl._engine(cfg, w, dtype)
    try:
        return (z,) + tuple(eng.score(z["input_ids"], z["attention_mask"], z["labels"], top_k=KMAX))
    finally:
        eng.close()


@pytest.mark.parametrize("name", ["loss_ragged_bf16", "loss_ragged_fp32"])
def test_engine_topk_is_the_top_of_the_swept_rows(name):
    z, cfg, dtype, w = tl._load(name)
    T, Vs = 6, int(cfg["speech_vocab_size"])
    assert z["attention_mask"][0, :T].all()
    ids, mask = z["input_ids"][:1, :T], np.ones((1, T), dtype=np.uint8)
    eng = tl._engine(cfg, w, dtype, max_batch=32, max_seq_len=64)
    try:
        rows = np.empty((T, 7, Vs), dtype=np.float32)                     # log_softmax of every speech head at every position
        for v0 in range(0, Vs, 32):
            vals = np.arange(v0, min(v0 + 32, Vs))
            lab = np.full((len(vals), T, 8), -100, dtype=np.int64)
            lab[:, :, 1:] = vals[:, None, None]
            lp = eng.score(np.repeat(ids, len(vals), 0), np.repeat(mask, len(vals), 0), lab)
            rows[:, :, vals] = lp[:, :, 1:].transpose(1, 2, 0)
        none, tid, tlp = eng.score(ids, mask, None, top_k=KMAX)
    finally:
        eng.close()
    assert none is None and tid.shape == (1, T, 8, KMAX) and tid.dtype == np.int32 and tlp.dtype == np.float32
    assert (tid[0, 0] == -1).all() and np.isnan(tlp[0, 0]).all() and np.isfinite(rows[1:]).all()
    want_ids, want_lp = topk_spec.topk_of_logprobs(rows[1:], KMAX)
    assert np.array_equal(tid[0, 1:, 1:], want_ids)
    assert np.array_equal(_bits(tlp[0, 1:, 1:]), _bits(want_lp))


# ---- 4. the engine: channel 0 (and every other), through the label ------------------------------------------------------------
@pytest.mark.parametrize("name", ["loss_ragged_bf16", "loss_ragged_fp32", "loss_ragged_fp16"])
def test_engine_topk_against_scored_labels(name):
    z, logp, tid, tlp = _top16(name)
    ids, mask, labels = z["input_ids"], z["attention_mask"], z["labels"]
    lens = mask.sum(1)
    assert np.array_equal(_bits(logp), _bits(tl._scored(name)[1]))        # logp is what score() alone returns
    live = np.zeros(mask.shape, dtype=bool)
    for b, n in enumerate(lens):
        live[b, 1:n] = True
    cfg, dtype, w = tl._load(name)[1:]
    vocab = np.array([cfg["vocab_size"]] + [cfg["speech_vocab_size"]] * 7)[None, None, :, None]
    assert ((tid >= 0) & (tid < vocab))[live].all() and np.isfinite(tlp[live]).all()
    assert (tid[~live] == -1).all() and np.isnan(tlp[~live]).all()        # t = 0, padding; a -100 label blanks nothing
    assert (labels[live] == -100).any()
    # entries are non-increasing, ids ascending within equal values
    a, b_ = tlp[live][..., :-1], tlp[live][..., 1:]
    assert (a >= b_).all() and (tid[live][..., :-1] < tid[live][..., 1:])[a == b_].all()
    # every labelled slot: the label is in the list with its token_logprobs bits, or it lies below the last entry
    lab_live = live[:, :, None] & (labels != -100)
    hit = (tid == labels[..., None]) & lab_live[..., None]
    assert np.array_equal(_bits(tlp[hit]), _bits(np.broadcast_to(logp[..., None], tlp.shape)[hit]))
    miss = lab_live & ~hit.any(-1)
    assert hit.any() and miss.any()
    last_lp, last_id = tlp[..., -1][miss], tid[..., -1][miss]
    assert ((logp[miss] < last_lp) | ((logp[miss] == last_lp) & (labels[miss] > last_id))).all()
    # every returned id, scored as the label of its slot, gives the same bits
    eng = tl._engine(cfg, w, dtype)
    try:
        for j in range(KMAX):
            lab_j = np.where(live[:, :, None], tid[..., j], -100).astype(np.int64)
            assert np.array_equal(_bits(eng.score(ids, mask, lab_j)), _bits(tlp[..., j])), j
    finally:
        eng.close()


# ---- 5. invariance ---------------------------------------------------------------------------------------------------------------
def _same(a, b):
    return np.array_equal(a[-2], b[-2]) and np.array_equal(_bits(a[-1]), _bits(b[-1]))


@pytest.mark.parametrize("name", ["loss_ragged_bf16", "loss_ragged_fp32"])
def test_engine_topk_does_not_depend_on_the_batch(name):
    z, cfg, dtype, w = tl._load(name)
    ids, mask, labels = z["input_ids"], z["attention_mask"], z["labels"]
    full = _top16(name)[1:]
    eng = tl._engine(cfg, w, dtype)
    try:
        once = eng.score(ids, mask, None, top_k=KMAX)                     # without labels, on another engine
        again = eng.score(ids, mask, None, top_k=KMAX)                    # two calls in a row
        assert _same(once, full) and _same(again, full)
        five = eng.score(ids, mask, labels, top_k=5)                      # k
        assert np.array_equal(five[1], full[1][..., :5]) and np.array_equal(_bits(five[2]), _bits(full[2][..., :5]))
        assert np.array_equal(_bits(five[0]), _bits(full[0]))
        for b in range(ids.shape[0]):                                     # alone and unpadded
            n = int(mask[b].sum())
            alone = eng.score(ids[b:b + 1, :n], mask[b:b + 1, :n], None, top_k=KMAX)
            assert np.array_equal(alone[1][0], full[1][b, :n]) and np.array_equal(_bits(alone[2][0]), _bits(full[2][b, :n])), b
        rev = eng.score(ids[::-1], mask[::-1], None, top_k=KMAX)          # batch order
        assert np.array_equal(rev[1][::-1], full[1]) and np.array_equal(_bits(rev[2][::-1]), _bits(full[2]))
    finally:
        eng.close()


def test_engine_topk_across_prefill_passes():
    """test_loss_gpu.py's 3 x 800 tokens: 2400 staged rows are two prefill passes, and five head launches of 512 rows."""
    z, cfg, dtype, w = tl._load("loss_ragged_bf16")
    rng = np.random.default_rng(77)
    B, T = 3, 800
    ids = np.full((B, T, 8), 1024, dtype=np.int64)
    ids[:, :, 0] = rng.integers(0, 151643, (B, T))
    ids[:, :, 1:] = rng.integers(0, 1024, (B, T, 7))
    mask = np.ones((B, T), dtype=np.uint8)
    eng = tl._engine(cfg, w, dtype, max_batch=4, max_seq_len=832)
    try:
        full = eng.score(ids, mask, None, top_k=KMAX)
        assert (full[1][:, 1:] >= 0).all() and (full[1][:, 0] == -1).all()
        for b in range(B):
            alone = eng.score(ids[b:b + 1], mask[b:b + 1], None, top_k=KMAX)
            assert np.array_equal(alone[1][0], full[1][b]) and np.array_equal(_bits(alone[2][0]), _bits(full[2][b])), b
    finally:
        eng.close()


# ---- 6. the engine is left as it was found -----------------------------------------------------------------------------------------
def test_topk_leaves_the_engine_untouched():
    z, cfg, dtype, w = tl._load("loss_ragged_bf16")
    g = np.load(os.path.join(GOLDEN, "ar_text_ragged.npz"))
    gw = synth.synth_weights(json.loads(str(g["cfg"])), int(g["seed"]), **json.loads(str(g["wkw"])))
    ids, mask, labels = z["input_ids"], z["attention_mask"], z["labels"]
    fresh = tl._engine(cfg, gw, "bf16")
    try:
        want_lp = fresh.score(ids, mask, labels)
    finally:
        fresh.close()
    eng = tl._engine(cfg, gw, "bf16")
    try:
        before = eng.generate(g["input_ids"], g["attention_mask"], int(g["max_length"]))
        assert np.array_equal(before, g["out_ids"])
        free = eng.kv_pool_state()[1]
        top = eng.score(ids, mask, labels, top_k=4)
        assert eng.kv_pool_state()[1] == free                             # the pool's pages are back
        assert np.array_equal(_bits(top[0]), _bits(want_lp))
        assert np.array_equal(_bits(eng.score(ids, mask, labels)), _bits(want_lp))     # score() as on a fresh engine
        assert np.array_equal(eng.generate(g["input_ids"], g["attention_mask"], int(g["max_length"])), before)
        assert eng.kv_pool_state()[1] == free
        # a run is open: begin without its steps
        eng.begin(g["input_ids"], g["attention_mask"], int(g["max_length"]))
        with pytest.raises(capi.MttsError) as ei:
            eng.score(ids, mask, None, top_k=4)
        assert ei.value.code == capi.ESTATE
        eng.step(3)
        eng.sched_open(4, 64)                              # ends the abandoned run
        # an adapter list is pending: refused, and the list stays
        three = np.full(3, -1, dtype=np.int32)
        capi.check(eng.lib.mtts_set_row_adapters(eng._h, three.ctypes.data, 3))
        with pytest.raises(capi.MttsError) as ei:
            eng.score(ids, mask, None, top_k=4)
        assert ei.value.code == capi.ESTATE
        capi.check(eng.lib.mtts_set_row_adapters(eng._h, None, 0))
        assert _same(eng.score(ids, mask, None, top_k=4), top)
        assert np.array_equal(eng.generate(g["input_ids"], g["attention_mask"], int(g["max_length"])), before)
    finally:
        eng.close()


def test_topk_argument_errors():
    z, cfg, dtype, w = tl._load("loss_ragged_bf16")
    ids, mask, labels = z["input_ids"], z["attention_mask"].astype(np.uint8), z["labels"]
    eng = tl._engine(cfg, w, dtype, max_batch=3, max_seq_len=200)
    try:
        free = eng.kv_pool_state()[1]

        def einval(i, m, l, match, k=3):
            with pytest.raises(capi.MttsError, match=match) as ei:
                eng.score(i, m, l, top_k=k)
            assert ei.value.code == capi.EINVAL
            assert eng.kv_pool_state()[1] == free

        # k through the C call
        B, T, _ = ids.shape
        lp = np.empty((B, T, 8), dtype=np.float32)
        ti, tp = np.empty((B, T, 8, 17), dtype=np.int32), np.empty((B, T, 8, 17), dtype=np.float32)
        i64, l64 = np.ascontiguousarray(ids, dtype=np.int64), np.ascontiguousarray(labels, dtype=np.int64)
        for k in (0, 17, -1):
            rc = eng.lib.mtts_score_topk(eng._h, i64.ctypes.data, mask.ctypes.data, l64.ctypes.data, B, T, lp.ctypes.data, k,
                                         ti.ctypes.data, tp.ctypes.data, None)
            assert rc == capi.EINVAL and "1..16" in eng.lib.mtts_last_error().decode() and eng.kv_pool_state()[1] == free
        for args in ((l64.ctypes.data, None, ti.ctypes.data, tp.ctypes.data), (None, lp.ctypes.data, ti.ctypes.data, tp.ctypes.data),
                     (None, None, None, tp.ctypes.data), (None, None, ti.ctypes.data, None)):
            rc = eng.lib.mtts_score_topk(eng._h, i64.ctypes.data, mask.ctypes.data, args[0], B, T, args[1], 4, args[2], args[3], None)
            assert rc == capi.EINVAL and eng.kv_pool_state()[1] == free
        einval(ids, mask, None, "1..16", k=17)
        # what mtts_score reports, with and without labels
        einval(ids[:, ::-1], mask[:, ::-1], labels[:, ::-1], "left-padded")
        einval(ids[:, ::-1], mask[:, ::-1], None, "left-padded")
        holes = mask.copy()
        holes[0, 50] = 0
        l2 = labels.copy()
        l2[0, 50] = -100
        einval(ids, holes, l2, "ones followed by zeros")
        einval(ids, holes, None, "ones followed by zeros")
        bad = labels.copy()
        bad[2, 100, 3] = 17
        einval(ids, mask, bad, "masked position")
        bad = labels.copy()
        bad[0, 10, 1] = 1025
        einval(ids, mask, bad, r"outside \[0, 1025\)")
        bad = labels.copy()
        bad[0, 10, 0] = -5
        einval(ids, mask, bad, "outside")
        bad = ids.copy()
        bad[0, 10, 1] = 1025
        einval(bad, mask, None, "out of range")
        four = lambda a: np.concatenate([a, a[:1]])
        einval(four(ids), four(mask), four(labels), "max_batch")
        wide = lambda a, v: np.concatenate([a, np.full_like(a[:, :1], v)], axis=1)
        einval(wide(ids, 0), wide(mask, 0), None, "max_seq_len")
        assert _same(eng.score(ids, mask, labels, top_k=KMAX), _top16("loss_ragged_bf16")[1:])
    finally:
        eng.close()
    small = tl._engine(cfg, w, dtype, max_batch=3, max_seq_len=200, kv_pool_pages=5)   # the batch needs 4 + 3 + 1 pages
    try:
        with pytest.raises(capi.MttsError, match="KV pages") as ei:
            small.score(ids, mask, None, top_k=2)
        assert ei.value.code == capi.ENOMEM and small.kv_pool_state()[1] == 5
    finally:
        small.close()


# ---- 7. the product surface --------------------------------------------------------------------------------------------------------
def test_model_forward_top_logprobs():
    import modeling_asteroid as ma
    z, cfg, dtype, w = tl._load("loss_ragged_bf16")
    model = ma.AsteroidTTSInstruct.from_state_dict(cfg, w).eval().to("cuda")
    ids, mask, labels = (torch.from_numpy(z[k]) for k in ("input_ids", "attention_mask", "labels"))
    try:
        plain = model(input_ids=ids, attention_mask=mask, labels=labels)
        assert plain.top_logprobs is None and plain.top_ids is None
        out = model(input_ids=ids, attention_mask=mask, labels=labels, top_logprobs=4)
        assert np.array_equal(_bits(out.token_logprobs.numpy()), _bits(plain.token_logprobs.numpy()))
        assert np.array_equal(_bits(out.loss_all.cpu().numpy()), _bits(plain.loss_all.cpu().numpy()))
        assert np.array_equal(_bits(np.float32(float(out.loss))), _bits(np.float32(float(plain.loss))))
        ref = _top16("loss_ragged_bf16")
        assert out.top_ids.dtype == torch.int64 and out.top_logprobs.dtype == torch.float32
        assert tuple(out.top_ids.shape) == tuple(ids.shape) + (4,) == tuple(out.top_logprobs.shape)
        assert np.array_equal(out.top_ids.numpy(), ref[2][..., :4]) and np.array_equal(_bits(out.top_logprobs.numpy()), _bits(ref[3][..., :4]))
        free = model(input_ids=ids, attention_mask=mask, top_logprobs=4)  # the label-free forward
        assert free.loss is None and free.loss_all is None and free.token_logprobs is None and free.logits is None
        assert torch.equal(free.top_ids, out.top_ids) and np.array_equal(_bits(free.top_logprobs.numpy()), _bits(out.top_logprobs.numpy()))
        loss, loss_all, none = model.forward(input_ids=ids, attention_mask=mask, labels=labels, top_logprobs=4, return_dict=False)
        assert none is None and torch.equal(loss_all, plain.loss_all) and float(loss) == float(plain.loss)
    finally:
        model._engine.close()
