"""tests/attn_ref.py on the CPU: the staging, the page layouts, the case generator and the reference that
test_attn_prefill_gpu.py compares the prefill attention kernels with.  No GPU."""
import time

import numpy as np
import pytest

import attn_ref as ar
from oracle import asteroid_oracle as ao


def _staging_by_hand(lens, cached):
    """The engine's own loop (mtts_begin: a row counter rounded up to the next tile after every dialogue)."""
    seq, pos, row0, r = [], [], [], 0
    for b, (n, c) in enumerate(zip(lens, cached)):
        row0.append(r)
        for i in range(c, n):
            seq.append(b)
            pos.append(i)
            r += 1
        while r % 32:
            seq.append(-1)
            pos.append(0)
            r += 1
    return r, np.array(seq), np.array(pos), np.array(row0)


@pytest.mark.parametrize("lens,cached", [(ar.RAGGED_LENS, (0,) * 7), (ar.LATER["lens"], ar.LATER["cached"]), ((31, 1, 96), (0, 0, 64))])
def test_staging_against_the_engines_loop(lens, cached):
    M, seq, pos, row0 = ar.stage(lens, cached)
    M2, seq2, pos2, row02 = _staging_by_hand(lens, cached)
    assert M == M2 == sum(ar.round_up(n - c, 32) for n, c in zip(lens, cached))
    assert np.array_equal(seq, seq2) and np.array_equal(pos, pos2) and np.array_equal(row0, row02)
    assert (row0 % 32 == 0).all()
    for t in range(M // 32):                         # a tile holds consecutive positions of one dialogue, live rows first
        s, p = seq[32 * t:32 * t + 32], pos[32 * t:32 * t + 32]
        live = int((s >= 0).sum())
        assert live >= 1 and (s[:live] == s[0]).all() and (s[live:] == -1).all()
        assert np.array_equal(p[:live], p[0] + np.arange(live)) and p[0] % 32 == 0


def test_ragged_case_is_the_one_the_issue_describes():
    c = ar.ragged_case(4, 2)
    assert c["M"] == 1120 and c["pages"] == 10 and c["ksplit"] == 3
    assert max(-(-int(n) // 64) for n in c["lens"]) == 9                 # pages_bound, below max_pages
    assert sorted(c["table"].ravel()) == list(range(70)) and not np.array_equal(c["table"].ravel(), np.arange(70))
    assert np.isnan(c["slabs"][:, c["seq"] < 0]).all() and np.isfinite(c["slabs"][:, c["seq"] >= 0]).all()
    for b, n in enumerate(c["lens"]):
        assert not c["K"][b, n:].any() and not c["V"][b, n:].any()
    j = ar.ragged_case(4, 2, stale="junk")
    for k in ("slabs", "qnw", "knw", "table"):
        assert np.array_equal(c[k], j[k], equal_nan=True)
    for b, n in enumerate(c["lens"]):
        assert np.array_equal(c["K"][b, :n], j["K"][b, :n]) and np.array_equal(c["V"][b, :n], j["V"][b, :n])
        junk = np.abs(ar.from_bits(np.concatenate([j["K"][b, n:], j["V"][b, n:]])).astype(np.float64))
        assert np.isfinite(junk).all() and junk.min() >= 2.0 ** 97 and junk.max() < 2.0 ** 105
    signs = ar.from_bits(j["V"][0, 1:]) > 0
    assert 0.4 < signs.mean() < 0.6
    assert np.array_equal(ar.ragged_case(4, 2, shuffled=False)["table"].ravel(), np.arange(70))


def test_page_layouts_and_pool_packing():
    rng = np.random.default_rng(3)
    B, Lmax, nkv = 2, 130, 2
    pages = 3
    K = rng.integers(0, 1 << 16, (B, Lmax, nkv, 128)).astype(np.uint16)
    V = rng.integers(0, 1 << 16, (B, Lmax, nkv, 128)).astype(np.uint16)
    table = rng.permutation(B * pages).reshape(B, pages)
    kc, vc = ar.pack_pools(K, V, table)
    for b, tok, h, d in ((0, 0, 0, 0), (1, 129, 1, 127), (0, 64, 1, 9), (1, 63, 0, 64), (0, 65, 0, 7)):
        pg, t = table[b][tok // 64], tok % 64
        assert kc[h, pg, ((d // 8) * 64 + t) * 8 + d % 8] == K[b, tok, h, d]
        assert vc[h, pg, ((t >> 1) * 128 + d) * 2 + (t & 1)] == V[b, tok, h, d]
    # each layout is a bijection of (token, dim) onto the page
    tok, d = np.meshgrid(np.arange(64), np.arange(128), indexing="ij")
    for f in (ar.k_index, ar.v_index):
        assert sorted(f(tok, d).ravel()) == list(range(64 * 128))
    for b in range(B):
        assert np.array_equal(ar.pool_tokens(kc, table, b, np.arange(Lmax), ar.k_index), K[b])
        assert np.array_equal(ar.pool_tokens(vc, table, b, np.arange(Lmax), ar.v_index), V[b])


def test_q_and_k_are_the_oracles_and_the_window_holds():
    """norm_rope is oracle.rmsnorm + oracle.apply_rope at the row's position; rmsnorm_rope_match accepts the oracle's own
    rows and a row computed with the float64 mean, and rejects a wrong position, weight element and rounding point."""
    c = ar.ragged_case(4, 2)
    ref = ar.ragged_reference(4, 2)
    live = np.nonzero(c["seq"] >= 0)[0]
    x, pos = ref["x"][live], c["pos"][live]
    orc = ao.AsteroidOracle(dict(head_dim=128, rope_theta=ar.THETA, num_hidden_layers=1, rms_norm_eps=ar.EPS), {}, "bf16")
    oc, os_ = orc.rope(pos[:, None].astype(np.int64))
    want = orc.apply_rope(orc.rmsnorm(x[:, None, :4], c["qnw"]).transpose(0, 2, 1, 3), oc, os_)[:, :, 0]
    assert np.array_equal(want, ref["q"][live])
    assert np.isnan(ref["q"][c["seq"] < 0]).all()
    got = ar.bits(want)
    assert ar.rmsnorm_rope_match(got, x[:, :4], c["qnw"], pos, c["cos"], c["sin"]) == (got.shape[0] * 4, [])
    # the float64 mean: a different but equally valid inv
    xq = x[:64, :4]
    inv = (1.0 / np.sqrt(np.mean(xq.astype(np.float64) ** 2, -1, keepdims=True) + ar.EPS)).astype(np.float32)
    alt = ar.rope_row(ar.rbf(c["qnw"] * ar.rbf(xq * inv)), pos[:64], c["cos"], c["sin"])
    assert ar.rmsnorm_rope_match(ar.bits(alt), xq, c["qnw"], pos[:64], c["cos"], c["sin"])[1] == []
    # what it must reject
    shifted = ar.norm_rope(xq, c["qnw"], pos[:64] + 1, c["cos"], c["sin"])
    w2 = c["qnw"].copy()
    w2[5:6] = ar.rbf(w2[5:6] * np.float32(1.02))
    once = ar.rope_row(ar.rbf(c["qnw"] * (xq * inv)), pos[:64], c["cos"], c["sin"])          # inner rounding left out
    for wrong in (shifted, ar.norm_rope(xq, w2, pos[:64], c["cos"], c["sin"]), once):
        n_same, bad = ar.rmsnorm_rope_match(ar.bits(wrong), xq, c["qnw"], pos[:64], c["cos"], c["sin"])
        assert len(bad) >= 32, (n_same, len(bad))


def test_reference_is_finite_causal_and_the_decode_formula_row_by_row():
    t0 = time.perf_counter()
    c, ref = ar.ragged_case(4, 2), ar.reference(ar.ragged_case(4, 2))
    took = time.perf_counter() - t0
    assert took < 3.0, took
    live = c["seq"] >= 0
    assert np.isfinite(ref["out"]).all() and np.isfinite(ref["q"][live]).all()
    assert not ref["out"][~live].any() and np.abs(ref["out"][live]).max(-1).min() > 0
    for b in range(c["B"]):
        assert ref["Kfull"][b].shape == (c["lens"][b], 2, 128) and np.isfinite(ref["Kfull"][b]).all() and np.isfinite(ref["Vfull"][b]).all()
    # row t = the decode-style formula on the dialogue's first t + 1 tokens
    for r in np.nonzero(live)[0]:
        b, t = int(c["seq"][r]), int(c["pos"][r])
        o = ar.attend_row(ref["q"][r], ref["Kfull"][b][:t + 1], ref["Vfull"][b][:t + 1])
        assert np.array_equal(ar.bits(o).ravel(), ar.bits(ref["out"][r])), (r, b, t)
    # token 0 attends to itself alone: its output is its own V row, for every head of the group
    for b in range(c["B"]):
        r0 = int(c["row0"][b])
        assert np.array_equal(ref["out"][r0].reshape(4, 128), np.repeat(ref["Vfull"][b][0], 2, axis=0))


def test_later_pass_reference_uses_the_cached_prefix():
    c, ref = ar.later_case(), ar.later_reference()
    assert c["M"] == 104 + 24 + 65 + 31 and list(c["row0"]) == [0, 128]
    assert np.isfinite(ref["out"]).all()
    for b in range(2):
        n0 = int(c["cached"][b])
        assert np.array_equal(ar.bits(ref["Kfull"][b][:n0]), c["K"][b, :n0])
    r = int(c["row0"][1])                              # first row of the second dialogue: position 512, 513 tokens
    assert c["pos"][r] == 512
    o = ar.attend_row(ref["q"][r], ref["Kfull"][1][:513], ref["Vfull"][1][:513])
    assert np.array_equal(ar.bits(o).ravel(), ar.bits(ref["out"][r]))
    kc, vc = ar.expected_pools(c, ref)
    for b in range(2):
        n0, n = int(c["cached"][b]), int(c["lens"][b])
        assert np.array_equal(ar.pool_tokens(kc, c["table"], b, np.arange(n0), ar.k_index), c["K"][b, :n0])
        assert np.array_equal(ar.pool_tokens(vc, c["table"], b, np.arange(n0, n), ar.v_index), ar.bits(ref["Vfull"][b][n0:]))
        assert not ar.pool_tokens(kc, c["table"], b, np.arange(n, c["Lmax"]), ar.k_index).any()


def test_reference_on_given_q_and_k():
    """reference(given=...) on the oracle's own q / K rows is the reference; with one K element moved by a bf16 ulp only rows
    at or behind that token, of that dialogue and kv head, can change."""
    c, ref = ar.ragged_case(4, 2), ar.ragged_reference(4, 2)
    ks = [ref["Kfull"][b][int(c["cached"][b]):].copy() for b in range(c["B"])]
    same = ar.reference(c, given=dict(q=ref["q"], k=ks))
    assert np.array_equal(same["out"], ref["out"]) and np.array_equal(same["q"], ref["q"], equal_nan=True)
    ks[5][100, 1, 24:25] = ar.from_bits(ar.bits(ks[5][100, 1, 24:25]) + 1)
    moved = ar.reference(c, given=dict(q=ref["q"], k=ks))
    assert ar.bits(moved["Kfull"][5][100, 1, 24]) == ar.bits(ref["Kfull"][5][100, 1, 24]) + 1
    diff = (moved["out"] != ref["out"]).reshape(c["M"], 4, 128).any(-1)
    r0 = int(c["row0"][5])
    assert not diff[:r0 + 100].any() and not diff[r0 + 257:].any() and not diff[:, :2].any()
    assert np.abs(moved["out"] - ref["out"]).max() <= 2.0 ** -7 * np.abs(ref["out"]).max()


def test_decode_sample_rows():
    c = ar.ragged_case(4, 2)
    rows = ar.decode_sample_rows(c)
    assert len(rows) == len(set(rows)) == 32 and (c["seq"][rows] >= 0).all()
    for b in range(c["B"]):
        assert int(c["row0"][b]) in rows and int(c["row0"][b]) + int(c["lens"][b]) - 1 in rows
    assert (c["seq"][rows] == 6).sum() >= 19 and c["pos"][rows][c["seq"][rows] == 6].max() == 512
