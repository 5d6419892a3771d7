"""Host-side expectations for the prefill attention tests (test_attn_ref_cpu.py, test_attn_prefill_gpu.py).  numpy only.

The kernels under test (csrc/layer.hip: qkv_post_kernel over many rows of one dialogue; csrc/attn.hip:
attn_prefill_scores_kernel, attn_prefill_pv_kernel, attn_combine_kernel with the prefill chunking), reached through
mtts_k_attn_prefill, compute for every token t of a dialogue

    x    = bf16(slab 0 + slab 1 + slab 2 + ...)                       fp32, in that order
    q, k = apply_rope(rmsnorm(x_q / x_k, weight)), v = x_v            oracle/asteroid_oracle.py: rmsnorm, apply_rope
    s    = bf16(bf16(q . k) * scale)   over the tokens <= t            modeling_qwen3.py:185-208, the rounding points that
    p    = bf16(softmax_fp32(s))                                       test_paged_attn_decode_kernel_vs_oracle states
    o    = bf16(p . V)

The two dot products are float64 sums here (their order is not part of the contract), everything else is fp32 with the
roundings above.  The softmax of row t is taken over its first t + 1 scores only, never over a masked row: numpy's sum
then sees exactly what the decode-style formula sees.

How a q / K row is compared (rmsnorm_rope_match): like layer_ref.rmsnorm_match.  The row is bf16(w * bf16(x * inv))
through RoPE, and only the fp32 VALUE of inv = 1 / sqrt(mean(x^2) + eps) depends on the order in which the 128 squares
are summed.  The oracle's order (numpy's pairwise sum) is one choice, the kernel's (a * a + b * b per lane, six
butterfly levels) another; both are right.  So a row passes when it equals the oracle's row bit for bit, or when some
fp32 inv within NORM_WINDOW ulps of the float64 value reproduces all of its 128 elements bit for bit.  Window, as in
layer_ref: 2 squares and 6 tree levels give a relative error of the sum of at most (2 + 1 + 6) u, u = 2^-24; the
division by 128 is exact, adding eps rounds once (+ u); the square root halves that and adds an ulp (2 u) of its own, as
does the reciprocal: (10 / 2 + 4) u = 9 ulps at most, one more for centring on the rounded float64 value and one for the
second-order terms: 11.
"""
import functools
import math

import numpy as np

from oracle import asteroid_oracle as ao

F32 = np.float32
rbf = ao.round_bf16
PAGE, TILE, HD, PASS_ROWS, PASS_CAP = 64, 32, 128, 128, 2048
EPS = 1e-6
THETA = 1.0e6
SCALE = F32(HD ** -0.5)
NORM_WINDOW = 11
NAN_BITS = 0xFFFF                       # what the hook fills q rows with before the launches
_ORC = ao.AsteroidOracle(dict(head_dim=HD, rope_theta=THETA, num_hidden_layers=1, rms_norm_eps=EPS), {}, "bf16")


def bits(a):
    a = np.ascontiguousarray(a, dtype=F32)
    return (a.view(np.uint32) >> 16).astype(np.uint16)


def from_bits(b):
    return (np.ascontiguousarray(b, dtype=np.uint16).astype(np.uint32) << 16).view(F32)


def round_up(a, b):
    return (a + b - 1) // b * b


# ---- page layouts (csrc/layer.hip: qkv_post_kernel) -------------------------------------------------------------------------
def k_index(tok, d):
    """Element (token tok of the page, dim d) of a K page [d/8][token][8]."""
    return ((d // 8) * PAGE + tok) * 8 + d % 8


def v_index(tok, d):
    """Element (tok, d) of a V page [token pair][d][2]."""
    return ((tok >> 1) * HD + d) * 2 + (tok & 1)


def pack_pools(K, V, table):
    """K, V uint16 bits [B][Lmax][nkv][128], table int [B][pages] -> pools [nkv][B * pages][64 * 128] as
    launch_pack_kv_pages fills them with every one of the Lmax tokens."""
    B, Lmax, nkv, _ = K.shape
    pages = table.shape[1]
    kc = np.zeros((nkv, B * pages, PAGE * HD), dtype=np.uint16)
    vc = np.zeros_like(kc)
    tok, d = np.meshgrid(np.arange(Lmax), np.arange(HD), indexing="ij")
    ki, vi = k_index(tok % PAGE, d), v_index(tok % PAGE, d)
    for b in range(B):
        pg = table[b][tok // PAGE]
        for h in range(nkv):
            kc[h, pg, ki] = K[b, :, h, :]
            vc[h, pg, vi] = V[b, :, h, :]
    return kc, vc


def pool_tokens(pool, table, b, toks, layout):
    """The rows of tokens `toks` of dialogue b out of a pool -> [len(toks)][nkv][128]."""
    toks = np.asarray(toks)
    d = np.arange(HD)[None, :]
    idx = layout(toks[:, None] % PAGE, d)
    return pool[:, table[b][toks // PAGE][:, None], idx].transpose(1, 0, 2)


# ---- staging of a pass's rows into 32-row tiles --------------------------------------------------------------------------
def stage(lens, cached):
    """-> (M, seq int32 [M], pos int32 [M], row0 [B]): dialogue b's tokens cached[b] .. lens[b] - 1 on rows row0[b] ..., every
    dialogue on a tile boundary, filler rows seq -1."""
    n = np.asarray(lens) - np.asarray(cached)
    row0 = np.concatenate([[0], np.cumsum(round_up(n, TILE))])
    M = int(row0[-1])
    seq, pos = np.full(M, -1, dtype=np.int32), np.zeros(M, dtype=np.int32)
    for b in range(len(lens)):
        seq[row0[b]:row0[b] + n[b]] = b
        pos[row0[b]:row0[b] + n[b]] = np.arange(cached[b], lens[b])
    return M, seq, pos, row0[:-1].astype(np.int64)


# ---- the case generator --------------------------------------------------------------------------------------------------
def rope_tables(Lmax):
    c, s = _ORC.rope(np.arange(Lmax, dtype=np.int64)[None])            # [1][Lmax][128], both halves alike
    return c[0, :, :HD // 2].copy(), s[0, :, :HD // 2].copy()


def junk_bits(rng, shape):
    """Finite bf16 junk around 2^100, both signs."""
    e = rng.integers(127 + 97, 127 + 104, shape).astype(np.uint16)
    return (rng.integers(0, 2, shape).astype(np.uint16) << 15) | (e << 7) | rng.integers(0, 128, shape).astype(np.uint16)


def make_case(nq, nkv, lens, cached, Lmax, ksplit, seed, stale="zeros", shuffled=True):
    """Inputs of one mtts_k_attn_prefill call.  Slab rows of idle rows are NaN (the engine's are whatever its GEMM made of
    an idle activation row: nothing may depend on them).  K / V: the cached prefix is random, the slots of the tokens the
    pass writes hold junk that must be overwritten, the slots behind a dialogue's end hold zeros or (`stale` = "junk") large
    finite junk that must survive untouched and reach no result."""
    rng = np.random.default_rng(seed)
    lens, cached = np.asarray(lens, dtype=np.int32), np.asarray(cached, dtype=np.int32)
    B, pages = len(lens), (Lmax + PAGE - 1) // PAGE
    M, seq, pos, row0 = stage(lens, cached)
    Npad = (nq + 2 * nkv) * HD
    slabs = (rng.standard_normal((ksplit, M, Npad)) * (2.0 / math.sqrt(ksplit))).astype(F32)
    slabs[:, seq < 0] = np.nan
    qnw = rbf((1 + 0.1 * rng.standard_normal(HD)).astype(F32))
    knw = rbf((1 + 0.1 * rng.standard_normal(HD)).astype(F32))
    cos, sin = rope_tables(Lmax)
    K = bits(rbf(rng.standard_normal((B, Lmax, nkv, HD)).astype(F32)))
    V = bits(rbf(rng.standard_normal((B, Lmax, nkv, HD)).astype(F32)))
    jk, jv = junk_bits(rng, K.shape), junk_bits(rng, V.shape)           # drawn always: `stale` does not move the other draws
    for b in range(B):
        K[b, cached[b]:lens[b]], V[b, cached[b]:lens[b]] = jk[b, cached[b]:lens[b]], jv[b, cached[b]:lens[b]]
        if stale == "junk":
            K[b, lens[b]:], V[b, lens[b]:] = jk[b, lens[b]:], jv[b, lens[b]:]
        else:
            K[b, lens[b]:], V[b, lens[b]:] = 0, 0
    table = rng.permutation(B * pages).astype(np.int32).reshape(B, pages)
    if not shuffled:
        table = np.arange(B * pages, dtype=np.int32).reshape(B, pages)
    return dict(nq=nq, nkv=nkv, lens=lens, cached=cached, Lmax=Lmax, ksplit=ksplit, B=B, pages=pages, M=M, seq=seq, pos=pos,
                row0=row0, slabs=slabs, qnw=qnw, knw=knw, cos=cos, sin=sin, K=K, V=V, table=table)


# ---- the operations ------------------------------------------------------------------------------------------------------
def slab_sum(slabs):
    """bf16(slab 0 + slab 1 + ...): fp32, in that order."""
    acc = slabs[0].astype(F32)
    for k in range(1, slabs.shape[0]):
        acc = (acc + slabs[k]).astype(F32)
    return rbf(acc)


def rope_row(y, pos, cos, sin):
    """The oracle's apply_rope on rows [rows][..., 128] at positions pos [rows]."""
    c = np.concatenate([cos[pos], cos[pos]], -1)[:, None]
    s = np.concatenate([sin[pos], sin[pos]], -1)[:, None]
    return _ORC.apply_rope(y.reshape(len(pos), -1, 1, HD), c, s).reshape(y.shape)


def norm_rope(x, w, pos, cos, sin):
    """x [rows][heads][128] -> the oracle's rmsnorm, then its RoPE."""
    return rope_row(_ORC.rmsnorm(x, w), pos, cos, sin)


def rmsnorm_rope_match(got_bits, x, w, pos, cos, sin):
    """got_bits uint16 [rows][heads][128] against x: -> (number of head-rows equal to the oracle's, list of (row, head)
    that no inv in the window reproduces).  See the module docstring."""
    want = bits(norm_rope(x, w, pos, cos, sin))
    same = (got_bits == want).all(-1)
    bad = []
    for r, h in np.argwhere(~same):
        xr = x[r, h].astype(F32)
        inv64 = 1.0 / math.sqrt(float(np.mean(xr.astype(np.float64) ** 2)) + EPS)
        c = np.array([F32(inv64)] * (2 * NORM_WINDOW + 1), dtype=F32)
        cand = (c.view(np.int32) + np.arange(-NORM_WINDOW, NORM_WINDOW + 1, dtype=np.int32)).view(F32)
        rows = rope_row(rbf(w[None] * rbf(xr[None] * cand[:, None])), np.full(len(cand), pos[r]), cos, sin)
        if not (bits(rows) == got_bits[r, h][None]).all(-1).any():
            bad.append((int(r), int(h)))
    return int(same.sum()), bad


def attend_row(q, K, V):
    """The decode-style formula for one query: q [nq][128], K / V [n][nkv][128] (its first pos + 1 tokens) -> o [nq][128]."""
    g = q.shape[0] // K.shape[1]
    Kr = np.repeat(K.transpose(1, 0, 2), g, axis=0).astype(np.float64)
    Vr = np.repeat(V.transpose(1, 0, 2), g, axis=0).astype(np.float64)
    s = rbf(np.einsum("hd,hnd->hn", q.astype(np.float64), Kr).astype(F32))
    s = rbf(s * SCALE)
    p = rbf(ao.softmax_f32(s))
    return rbf(np.einsum("hn,hnd->hd", p.astype(np.float64), Vr).astype(F32))


def reference(case, given=None):
    """-> dict: q [M][nq][128] fp32 of bf16 values (idle rows NaN), out [M][nq * 128] (idle rows 0), and for every dialogue
    its full K / V after the pass, Kfull[b] / Vfull[b] [lens[b]][nkv][128].
    `given` = dict(q=fp32 [M][nq][128], k=[per dialogue fp32 [lens - cached][nkv][128]]): q and K rows that
    rmsnorm_rope_match has accepted (a row may differ from the oracle's by its inv: module docstring) take the place of the
    oracle's, so that the attention rows are held against the formula on the very q and K the kernels were given."""
    nq, nkv, M = case["nq"], case["nkv"], case["M"]
    g = nq // nkv
    x = slab_sum(case["slabs"]).reshape(M, nq + 2 * nkv, HD)
    q = np.full((M, nq, HD), np.nan, dtype=F32)
    out = np.zeros((M, nq, HD), dtype=F32)
    Kfull, Vfull = [], []
    for b in range(case["B"]):
        c, n = int(case["cached"][b]), int(case["lens"][b])
        rows = slice(int(case["row0"][b]), int(case["row0"][b]) + n - c)
        pos = np.arange(c, n)
        qb = norm_rope(x[rows, :nq], case["qnw"], pos, case["cos"], case["sin"])
        kb = norm_rope(x[rows, nq:nq + nkv], case["knw"], pos, case["cos"], case["sin"])
        if given is not None:
            qb, kb = np.asarray(given["q"][rows], dtype=F32), np.asarray(given["k"][b], dtype=F32)
        Kb = np.concatenate([from_bits(case["K"][b, :c]), kb], 0)
        Vb = np.concatenate([from_bits(case["V"][b, :c]), x[rows, nq + nkv:]], 0)
        q[rows] = qb
        Kfull.append(Kb)
        Vfull.append(Vb)
        for h in range(nq):
            S = rbf((qb[:, h].astype(np.float64) @ Kb[:, h // g].astype(np.float64).T).astype(F32))
            S = rbf(S * SCALE)
            P = np.zeros_like(S)
            for i, t in enumerate(pos):
                P[i, :t + 1] = rbf(ao.softmax_f32(S[i, :t + 1]))
            out[rows, h] = rbf((P.astype(np.float64) @ Vb[:, h // g].astype(np.float64)).astype(F32))
    return dict(q=q, out=out.reshape(M, nq * HD), Kfull=Kfull, Vfull=Vfull, x=x)


def expected_pools(case, ref):
    """The pools after the pass: what the test put there, with the pass's tokens replaced by the reference's K / V rows."""
    K, V = case["K"].copy(), case["V"].copy()
    for b in range(case["B"]):
        c, n = int(case["cached"][b]), int(case["lens"][b])
        K[b, c:n], V[b, c:n] = bits(ref["Kfull"][b][c:]), bits(ref["Vfull"][b][c:])
    return pack_pools(K, V, case["table"])


# ---- the cases of test_attn_prefill_gpu.py -----------------------------------------------------------------------------------
RAGGED_LENS = (1, 32, 33, 64, 65, 257, 513)
RAGGED_LMAX = 640
GROUPS = ((2, 2), (4, 2), (4, 1))
LATER = dict(nq=4, nkv=2, lens=(200, 577), cached=(96, 512), Lmax=640, ksplit=3, seed=77)
PERTURB_DIALOGUE, PERTURB_TOKEN = 4, 40           # token 40 of the 65-token dialogue


@functools.lru_cache(maxsize=None)
def ragged_case(nq, nkv, stale="zeros", shuffled=True):
    return make_case(nq, nkv, RAGGED_LENS, (0,) * len(RAGGED_LENS), RAGGED_LMAX, 3, 100 + 10 * nq + nkv, stale, shuffled)


@functools.lru_cache(maxsize=None)
def ragged_reference(nq, nkv):
    """Shared by the tests and left unchanged by them (neither `stale` nor the page table enters it)."""
    return reference(ragged_case(nq, nkv))


@functools.lru_cache(maxsize=None)
def later_case():
    return make_case(**LATER)


@functools.lru_cache(maxsize=None)
def later_reference():
    return reference(later_case())


def decode_sample_rows(case):
    """The 32 rows the exact-share comparison runs through the decode kernels: the first and last live row of every
    dialogue, the rest spread over the longest one."""
    rows = []
    for b in range(case["B"]):
        n = int(case["lens"][b] - case["cached"][b])
        rows += [int(case["row0"][b]), int(case["row0"][b]) + n - 1]
    big = int(np.argmax(case["lens"] - case["cached"]))
    n = int(case["lens"][big] - case["cached"][big])
    rows = sorted(set(rows))
    rows += [int(case["row0"][big]) + int(t) for t in np.linspace(1, n - 2, 32 - len(rows)).astype(int)]
    assert len(set(rows)) == 32
    return sorted(rows)
