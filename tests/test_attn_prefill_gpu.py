"""The prefill attention kernels, one pass at a time, against tests/attn_ref.py.  -m gpu.

qkv_post_kernel over many rows of one dialogue, attn_prefill_scores_kernel and attn_prefill_pv_kernel (csrc/attn.hip:
32-row tiles of one dialogue on the matrix cores) and attn_combine_kernel with the prefill chunking (ATT_PF = 2 pages),
through mtts_k_attn_prefill, which launches them as the engine's prefill does.  Every prompt goes through these kernels
(pf_mfma_pages = 0).  q and the K / V rows in the pools are compared bit for bit (a q / K head-row with the oracle's
rmsnorm + RoPE row; the few rows -- one K row in 20 000 head-rows on the MI355X -- where the kernel's sum of the 128
squares gives another fp32 inv than numpy's sum must be reproduced whole, bit for bit, by ONE inv inside the window
attn_ref derives), everything in the pools that the pass must not write has to keep what the test put there, the attention rows keep the decode test's bound against the eager
formula with its three bf16 rounding points, and causality / isolation are shown by perturbation, bit for bit.  The
hook starts q, scores, statistics and chunk partials as NaN: a slot a kernel loads but must not use shows in the output.
test_attn_ref_cpu.py checks the reference, the staging and the inputs on the CPU.

Shapes.  lens = 1, 32, 33, 64, 65, 257, 513 in one pass of 1120 rows: one live row in a tile; a full tile; a tile with
one live row (33; 65: alone on a new page); a full page; 5 pages = a second scores block with one live wave; 9 pages =
5 chunks = a second P.V block, and pages_bound (9) far above the short dialogues' own pages; Lmax = 640: max_pages (10)
above pages_bound.  (nq, nkv) = (2,2), (4,2), (4,1): G = 1, 2, 4; only G = 4 makes two GP sweeps.
"""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import attn_ref as ar  # noqa: E402
import layer_ref as lr  # noqa: E402
from mtts import capi  # noqa: E402

F32 = np.float32

# SHARES.  Measured on an MI355X: share of attention outputs equal to attn_ref.reference bit for bit.
#   prefill: every live output of the ragged pass (mtts_k_attn_prefill);  prefill-32 / decode-32: the 32 sample rows
#   (attn_ref.decode_sample_rows), prefill kernels / decode kernels (mtts_k_paged_attn_decode on the same q and the row's
#   own first pos + 1 tokens)
#     (nq, nkv)     prefill     prefill-32   decode-32
#     (2, 2)        0.9999      1.0000       1.0000
#     (4, 2)        0.9997      0.9999       1.0000
#     (4, 1)        0.9997      1.0000       0.9999
#   the later pass of a long prompt (test_later_pass_of_a_long_prompt, (4, 2)): prefill 0.9996
# A build whose scores kernel scales ONE page's sum of exponentials by 1.01 stays inside the 2^-7 bound on nearly every row
# and drops these shares to 0.86: the share is what notices a wrong (max, sum) pair.
# test_exact_share_against_decode_kernels pins the prefill share to at least the decode share minus 0.5 percentage
# points (summation order is the only freedom of either; expf differs by an ulp between orders) and prints all three.


def _dev_bits(b):
    return torch.from_numpy(np.ascontiguousarray(b, dtype=np.uint16).view(np.int16)).cuda()


def _dev_bf16(a):
    return _dev_bits(ar.bits(a))


def _poisoned(*shape):
    return _dev_bits(np.full(shape, lr.SENTINEL, dtype=np.uint16))


def _host(t):
    return t.cpu().numpy().view(np.uint16)


def _call(nq, nkv, lens, cached, Lmax, ksplit, slabs, qnw, knw, cos, sin, K, V, table, rows):
    """One mtts_k_attn_prefill call on outputs prefilled with the sentinel -> (rc, out, q, kcache, vcache) as uint16 bits."""
    B, pages = len(lens), (Lmax + 63) // 64
    out, q = _poisoned(rows, nq * 128), _poisoned(rows, nq, 128)
    kc, vc = _poisoned(nkv, B * pages, 64 * 128), _poisoned(nkv, B * pages, 64 * 128)
    ins = [torch.from_numpy(np.ascontiguousarray(slabs, dtype=F32)).cuda(), _dev_bf16(qnw), _dev_bf16(knw), _dev_bf16(cos), _dev_bf16(sin),
           _dev_bits(K), _dev_bits(V)]
    hl, hc = np.ascontiguousarray(lens, dtype=np.int32), np.ascontiguousarray(cached, dtype=np.int32)
    ht = None if table is None else np.ascontiguousarray(table, dtype=np.int32)
    torch.cuda.synchronize()
    rc = capi.lib().mtts_k_attn_prefill(
        ins[0].data_ptr(), ksplit, ins[1].data_ptr(), ins[2].data_ptr(), ins[3].data_ptr(), ins[4].data_ptr(), C.c_float(ar.EPS),
        ins[5].data_ptr(), ins[6].data_ptr(), hl.ctypes.data, hc.ctypes.data, None if ht is None else ht.ctypes.data, B, Lmax, nq, nkv,
        out.data_ptr(), q.data_ptr(), kc.data_ptr(), vc.data_ptr(), None)
    torch.cuda.synchronize()
    return rc, _host(out), _host(q), _host(kc), _host(vc)


def _run(case, table="case"):
    rc, out, q, kc, vc = _call(case["nq"], case["nkv"], case["lens"], case["cached"], case["Lmax"], case["ksplit"], case["slabs"],
                               case["qnw"], case["knw"], case["cos"], case["sin"], case["K"], case["V"],
                               case["table"] if isinstance(table, str) else table, case["M"])
    capi.check(rc)
    return dict(out=out, q=q, kc=kc, vc=vc)


@functools.lru_cache(maxsize=None)
def _ragged_run(nq, nkv):
    """The ragged pass on the GPU, once per group size; the tests share it and leave it unchanged."""
    return _run(ar.ragged_case(nq, nkv))


def _first(mask):
    return np.argwhere(mask)[:5].tolist()


def _validate_qk(case, ref, got, what):
    """q and the pass's K / V rows in the pools, bit for bit: V is the rounded slab sum; a q / K head-row is the oracle's
    rmsnorm + RoPE row, or -- where the kernel's fp32 sum of the 128 squares and numpy's land on different fp32 values
    of inv -- the row some inv inside attn_ref's window reproduces whole (attn_ref docstring; every element of the row has
    to come from that ONE inv).  Returns the reference the attention rows are held against: `ref`, or, when a row took
    the second leg, the same formula on the q and K the kernels actually read."""
    nq, nkv, live = case["nq"], case["nkv"], case["seq"] >= 0
    rows, pos = np.nonzero(live)[0], case["pos"][live]
    n_q, bad_q = ar.rmsnorm_rope_match(got["q"][rows], ref["x"][rows, :nq], case["qnw"], pos, case["cos"], case["sin"])
    assert not bad_q, (what, "q rows no inv reproduces (live row index, head)", bad_q[:5])
    assert (got["q"][~live] == ar.NAN_BITS).all(), (what, "q written for an idle row", _first(got["q"][~live] != ar.NAN_BITS))
    n_k = tot_k = 0
    gks = []
    for b in range(case["B"]):
        c, n = int(case["cached"][b]), int(case["lens"][b])
        toks = np.arange(c, n)
        r0 = int(case["row0"][b])
        gk = ar.pool_tokens(got["kc"], case["table"], b, toks, ar.k_index)
        gv = ar.pool_tokens(got["vc"], case["table"], b, toks, ar.v_index)
        same, bad_k = ar.rmsnorm_rope_match(gk, ref["x"][r0:r0 + n - c, nq:nq + nkv], case["knw"], toks, case["cos"], case["sin"])
        assert not bad_k, (what, "K rows no inv reproduces (dialogue, token - cached, head)", b, bad_k[:5])
        assert np.array_equal(gv, ar.bits(ref["Vfull"][b][c:])), (what, "V rows of dialogue", b, _first(gv != ar.bits(ref["Vfull"][b][c:])))
        n_k, tot_k = n_k + same, tot_k + (n - c) * nkv
        gks.append(ar.from_bits(gk))
    print("%s: head-rows equal to the oracle's own rmsnorm: q %d of %d, K %d of %d (the rest: another inv inside the window)"
          % (what, n_q, len(rows) * nq, n_k, tot_k))
    if n_q == len(rows) * nq and n_k == tot_k:
        return ref
    return ar.reference(case, given=dict(q=ar.from_bits(got["q"]), k=gks))


def _check(case, ref, got, what):
    """The assertions of a pass: q and the pass's K / V rows bit for bit, the rest of the pools untouched, idle rows, the bound.
    -> (share of live outputs equal to the reference bit for bit, the reference used)."""
    live = case["seq"] >= 0
    rows, pos = np.nonzero(live)[0], case["pos"][live]
    ref = _validate_qk(case, ref, got, what)
    # everything else in the pools -- the cached prefix, the slots at and behind every dialogue's end -- is what the test put there
    kc, vc = ar.expected_pools(case, ref)
    assert np.array_equal(got["kc"], kc), (what, "K pool (kv head, page, element)", _first(got["kc"] != kc))
    assert np.array_equal(got["vc"], vc), (what, "V pool (kv head, page, element)", _first(got["vc"] != vc))
    # attention rows
    assert not got["out"][~live].any(), (what, "idle rows of the output are not zero", _first(got["out"][~live] != 0))
    o, g = ref["out"][live].astype(np.float64), ar.from_bits(got["out"][live]).astype(np.float64)
    assert np.isfinite(g).all(), (what, "non-finite outputs: a NaN scratch slot reached a result", _first(~np.isfinite(g)))
    err, tol = np.abs(g - o).max(-1), 2.0 ** -7 * np.abs(o).max(-1)
    worst = int(np.argmax(err / tol))
    print("%s: worst row %d (dialogue %d, position %d): error %.3g of bound %.3g" % (what, rows[worst], case["seq"][rows[worst]], pos[worst], err[worst], tol[worst]))
    assert (err <= tol).all(), (what, "live rows beyond 2^-7 of the row maximum", rows[err > tol][:5].tolist(), float(err[worst]), float(tol[worst]))
    return float((got["out"][live] == ar.bits(ref["out"][live])).mean()), ref


@functools.lru_cache(maxsize=None)
def _ragged_checked(nq, nkv):
    """_check of the ragged pass, once per group size -> (exact share, the reference its attention rows were held against)."""
    return _check(ar.ragged_case(nq, nkv), ar.ragged_reference(nq, nkv), _ragged_run(nq, nkv), "ragged (%d, %d)" % (nq, nkv))


@pytest.mark.parametrize("nq,nkv", ar.GROUPS)
def test_ragged_batch(nq, nkv):
    """lens 1, 32, 33, 64, 65, 257, 513 in one pass, cached 0, shuffled page table, ksplit 3 (shapes: module docstring)."""
    share, _ = _ragged_checked(nq, nkv)
    print("ragged (%d, %d): exact share of live outputs %.4f" % (nq, nkv, share))


def _decode_rows(case, ref, q_bits, rows):
    """mtts_k_paged_attn_decode (the decode kernels: attn_scores + attn_pv + attn_combine) on rows `rows` of the pass, each as
    a sequence of its own holding the dialogue's first pos + 1 tokens -> bf16 bits [len(rows)][nq * 128]."""
    nq, nkv, R, Lmax = case["nq"], case["nkv"], len(rows), case["Lmax"]
    K, V = np.zeros((R, Lmax, nkv, 128), dtype=F32), np.zeros((R, Lmax, nkv, 128), dtype=F32)
    lens = np.zeros(R, dtype=np.int32)
    for i, r in enumerate(rows):
        b, n = int(case["seq"][r]), int(case["pos"][r]) + 1
        K[i, :n], V[i, :n], lens[i] = ref["Kfull"][b][:n], ref["Vfull"][b][:n], n
    qt, kt, vt, out = _dev_bits(q_bits[rows]), _dev_bf16(K), _dev_bf16(V), _poisoned(R, nq * 128)
    capi.check(capi.lib().mtts_k_paged_attn_decode(qt.data_ptr(), kt.data_ptr(), vt.data_ptr(), lens.ctypes.data, None, R, Lmax, nq, nkv,
                                                   out.data_ptr(), None))
    torch.cuda.synchronize()
    return _host(out)


@pytest.mark.parametrize("nq,nkv", ar.GROUPS)
def test_exact_share_against_decode_kernels(nq, nkv):
    """Share of live outputs equal to the reference bit for bit: at least what the already tested decode kernels reach on 32
    of those rows (same q, each row's own first pos + 1 tokens) minus 0.5 percentage points.  Measured: SHARES above."""
    case, got = ar.ragged_case(nq, nkv), _ragged_run(nq, nkv)
    share, ref = _ragged_checked(nq, nkv)
    want = ar.bits(ref["out"])
    rows = ar.decode_sample_rows(case)
    dec = _decode_rows(case, ref, got["q"], rows)
    share32, decode32 = float((got["out"][rows] == want[rows]).mean()), float((dec == want[rows]).mean())
    print("attention exact share (%d, %d): prefill %.4f, prefill on the 32 rows %.4f, decode kernels on the 32 rows %.4f" % (nq, nkv, share, share32, decode32))
    o = ar.from_bits(want[rows]).astype(np.float64)
    assert (np.abs(ar.from_bits(dec) - o).max(-1) <= 2.0 ** -7 * np.abs(o).max(-1)).all()      # the decode kernels on their own bound
    assert share >= decode32 - 0.005, (share, share32, decode32)


def test_later_pass_of_a_long_prompt():
    """cached = (96, 512), lens = (200, 577): the pass starts in the middle of a page the prefix half filled, and on a page
    boundary nine pages in.  The cached tokens' pool elements stay untouched, bit for bit (the pool comparison of _check)."""
    case, ref = ar.later_case(), ar.later_reference()
    got = _run(case)
    share, _ = _check(case, ref, got, "later pass")
    for b in range(case["B"]):
        toks = np.arange(int(case["cached"][b]))
        assert np.array_equal(ar.pool_tokens(got["kc"], case["table"], b, toks, ar.k_index), case["K"][b, toks]), b
        assert np.array_equal(ar.pool_tokens(got["vc"], case["table"], b, toks, ar.v_index), case["V"][b, toks]), b
    print("later pass: exact share of live outputs %.4f" % share)


def test_perturbed_token_reaches_only_later_rows_of_its_dialogue():
    """(a) The slab rows of token 40 of the 65-token dialogue change: its rows 0..39 and every other dialogue are
    bit-identical, rows 40..64 differ."""
    base, case = _ragged_run(4, 2), dict(ar.ragged_case(4, 2))
    r0 = int(case["row0"][ar.PERTURB_DIALOGUE])
    assert case["lens"][ar.PERTURB_DIALOGUE] == 65
    case["slabs"] = case["slabs"].copy()
    case["slabs"][:, r0 + ar.PERTURB_TOKEN] = np.random.default_rng(5).standard_normal(case["slabs"][:, 0].shape).astype(F32)
    got = _run(case)
    later = np.zeros(case["M"], dtype=bool)
    later[r0 + ar.PERTURB_TOKEN:r0 + 65] = True
    assert np.array_equal(got["out"][~later], base["out"][~later]), _first(got["out"][~later] != base["out"][~later])
    changed = (got["out"][later] != base["out"][later]).reshape(25, 4, 128).any(-1)
    assert changed.all(), ("rows 40..64 x heads that did not change", _first(~changed))
    only = np.zeros(case["M"], dtype=bool)
    only[r0 + ar.PERTURB_TOKEN] = True
    assert np.array_equal(got["q"][~only], base["q"][~only]) and (got["q"][only] != base["q"][only]).any()


def test_stale_pages_behind_a_dialogues_end_reach_nothing():
    """(b) Large finite junk (around 2^100, both signs) instead of zeros behind every dialogue's end: the output is
    bit-identical and the junk is still there.  Finite, not NaN: P.V multiplies masked tokens by an exact 0 on the matrix
    cores, and the engine's pool is zeroed at creation and only ever holds kernel-written values."""
    base, case = _ragged_run(4, 2), ar.ragged_case(4, 2, stale="junk")
    got = _run(case)
    assert np.array_equal(got["out"], base["out"]), _first(got["out"] != base["out"])
    assert np.array_equal(got["q"], base["q"])
    kc, vc = ar.expected_pools(case, _ragged_checked(4, 2)[1])
    assert np.array_equal(got["kc"], kc), _first(got["kc"] != kc)
    assert np.array_equal(got["vc"], vc), _first(got["vc"] != vc)


def test_page_table_only_redirects():
    """(c) NULL (consecutive) page table against the shuffled one: bit-identical output, the same K / V rows in other pages."""
    base, case = _ragged_run(4, 2), ar.ragged_case(4, 2)
    got = _run(case, table=None)
    assert np.array_equal(got["out"], base["out"]), _first(got["out"] != base["out"])
    ident = ar.ragged_case(4, 2, shuffled=False)["table"]
    for b in range(case["B"]):
        toks = np.arange(case["Lmax"])
        for pool, layout in (("kc", ar.k_index), ("vc", ar.v_index)):
            assert np.array_equal(ar.pool_tokens(got[pool], ident, b, toks, layout), ar.pool_tokens(base[pool], case["table"], b, toks, layout)), (b, pool)


@pytest.mark.parametrize("name,kw", [
    ("cached not a multiple of 32", dict(cached=(16, 0))),
    ("cached >= lens", dict(cached=(64, 0), lens=(64, 40))),
    ("lens > Lmax", dict(lens=(129, 40))),
    ("nq % nkv != 0", dict(nq=3)),
    ("M > 2048", dict(lens=(640,) * 5, cached=(0,) * 5, Lmax=640)),
    ("page table not a permutation", dict(dup=True)),
])
def test_refusals(name, kw):
    """Each returns MTTS_EINVAL and leaves the output buffers (prefilled with layer_ref.SENTINEL) untouched."""
    nq, nkv, Lmax = kw.get("nq", 2), 2, kw.get("Lmax", 128)
    lens, cached = kw.get("lens", (100, 40)), kw.get("cached", (32, 0))
    B, pages = len(lens), (Lmax + 63) // 64
    rows = B * ar.round_up(Lmax + 1, 32)                                  # more than any staging of these lengths needs
    rng = np.random.default_rng(9)
    slabs = rng.standard_normal((1, rows, (nq + 2 * nkv) * 128)).astype(F32)
    w = np.ones(128, dtype=F32)
    cos, sin = ar.rope_tables(Lmax + 64)
    K = np.zeros((B, Lmax + 64, nkv, 128), dtype=np.uint16)
    table = np.arange(B * pages, dtype=np.int32).reshape(B, pages)
    if kw.get("dup"):
        table[1, 0] = table[0, 0]
    rc, out, q, kc, vc = _call(nq, nkv, lens, cached, Lmax, 1, slabs, w, w, cos, sin, K, K, table, rows)
    assert rc == capi.EINVAL, (name, rc)
    for buf, what in ((out, "out"), (q, "q"), (kc, "K pool"), (vc, "V pool")):
        assert (buf == lr.SENTINEL).all(), (name, what, "written by a refused call")
