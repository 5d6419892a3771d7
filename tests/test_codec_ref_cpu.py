"""tests/codec_ref.py checked on the CPU: the references against the oracle's own code, the packed layout against the
offset formula of common.h, the split, the case tables against the entries' documented preconditions, and the exactness
the RVQ test rests on.  Nothing here runs a kernel."""
import numpy as np
import pytest

import codec_ref as cr
from oracle import codec_oracle as co

F64 = np.float64


@pytest.fixture
def oracle64(monkeypatch):
    """The oracle's code with its working precision switched from fp32 to fp64 (its formulas, no fp32 rounding)."""
    monkeypatch.setattr(co, "F32", np.float64)
    return co


def _bare_oracle(w, cfg=None):
    orc = co.CodecOracle.__new__(co.CodecOracle)
    orc.w, orc.c = w, cfg or {}
    return orc


@pytest.mark.parametrize("B,heads,T,lens", [(3, 2, 9, (9, 4, 0)), (2, 3, 33, (1, 28)), (1, 2, 1, (1,))])
def test_attention_ref_matches_oracle_layer(oracle64, B, heads, T, lens):
    """CodecOracle._layer with identity out_proj and a zero MLP returns x + attention(LN(x))."""
    d = 64 * heads
    rng = np.random.default_rng(5)
    x = rng.standard_normal((B, T, d))
    p = "L."
    one, zero = np.ones(d), np.zeros(d)
    w = {p + "self_attn_layer_norm.weight": one, p + "self_attn_layer_norm.bias": zero,
         p + "self_attn.q_proj.weight": rng.standard_normal((d, d)) / np.sqrt(d), p + "self_attn.q_proj.bias": rng.standard_normal(d),
         p + "self_attn.k_proj.weight": rng.standard_normal((d, d)) / np.sqrt(d),
         p + "self_attn.v_proj.weight": rng.standard_normal((d, d)) / np.sqrt(d), p + "self_attn.v_proj.bias": rng.standard_normal(d),
         p + "self_attn.out_proj.weight": np.eye(d), p + "self_attn.out_proj.bias": zero,
         p + "final_layer_norm.weight": one, p + "final_layer_norm.bias": zero,
         p + "fc1.weight": np.zeros((4, d)), p + "fc1.bias": np.zeros(4), p + "fc2.weight": np.zeros((d, 4)), p + "fc2.bias": zero}
    want = _bare_oracle(w)._layer(x, lens, p, heads) - x
    h = co.layer_norm(x, one, zero, 1e-5)
    qkv = np.concatenate([h @ w[p + "self_attn.q_proj.weight"].T + w[p + "self_attn.q_proj.bias"],
                          h @ w[p + "self_attn.k_proj.weight"].T,
                          h @ w[p + "self_attn.v_proj.weight"].T + w[p + "self_attn.v_proj.bias"]], axis=-1)
    got, c, spv = cr.attn_ref(qkv, lens, heads)
    assert np.abs(got - want).max() <= 1e-12
    # a padded query row is the mean of V over all T keys; a row that sees one key is V[0]
    v = qkv[..., 2 * d:]
    for b, n in enumerate(lens):
        assert np.abs(got[b, n:] - v[b].mean(0)).max(initial=0.0) <= 1e-12
        if n == 1:
            assert np.abs(got[b, 0] - v[b, 0]).max() <= 1e-15
            assert (c[b, :, 0] == cr.B3).all()
        assert (c[b, :, n:] == cr.B3).all()
    assert (c >= cr.B3).all() and (spv >= np.abs(got) - 1e-12).all()


def test_attention_ref_is_softmax_ref_times_v():
    B, heads, T, lens = 3, 2, 21, (21, 0, 6)
    qkv = cr.attn_inputs(B, heads, T, 0).astype(F64)
    d = 64 * heads
    q = qkv[..., :d].reshape(B, T, heads, 64).transpose(0, 2, 1, 3)
    k = qkv[..., d:2 * d].reshape(B, T, heads, 64).transpose(0, 2, 1, 3)
    v = qkv[..., 2 * d:].reshape(B, T, heads, 64).transpose(0, 2, 1, 3)
    S = np.zeros((B, heads, T, cr.ld16(T)))
    S[..., :T] = np.matmul(q, k.transpose(0, 1, 3, 2)) * cr.ATTN_SCALE
    P = cr.softmax_mask_ref(S, lens, T)
    assert not P[..., T:].any() and np.abs(P.sum(-1) - 1).max() <= 1e-14
    out = np.matmul(P[..., :T], v).transpose(0, 2, 1, 3).reshape(B, T, d)
    assert np.abs(out - cr.attn_ref(qkv, lens, heads)[0]).max() <= 1e-13


def test_layernorm_ref_matches_oracle(oracle64):
    x, w, b = (a.astype(F64) for a in cr.ln_inputs(5, 80))
    assert np.abs(cr.layernorm_ref(x, w, b, 1e-5) - co.layer_norm(x, w, b, 1e-5)).max() <= 1e-12
    y = cr.layernorm_ref(np.tile(x, (2, 1))[:8], w, b, 1e-5, lens=(3, 0), T=4)
    assert not y[3:].any() and y[:3].all()


def test_dwconv_ln_ref_matches_oracle_vocos_block(oracle64, monkeypatch):
    """CodecOracle.vocos on a one-block backbone: its second layer_norm call takes the depthwise conv of the first call's
    output and returns what dwconv_ln_ref must give."""
    C, mel, nfft, hop, B, T = 48, 6, 16, 4, 2, 9
    rng = np.random.default_rng(7)
    p, q = "enhanced_vocos.backbone.", "enhanced_vocos.backbone.convnext.0."
    w = {p + "embed.weight": rng.standard_normal((C, mel, 7)), p + "embed.bias": rng.standard_normal(C),
         p + "norm.weight": 1 + 0.3 * rng.standard_normal(C), p + "norm.bias": rng.standard_normal(C),
         q + "dwconv.weight": rng.standard_normal((C, 1, 7)), q + "dwconv.bias": rng.standard_normal(C),
         q + "norm.weight": 1 + 0.3 * rng.standard_normal(C), q + "norm.bias": rng.standard_normal(C),
         q + "pwconv1.weight": rng.standard_normal((8, C)) / 8, q + "pwconv1.bias": np.zeros(8),
         q + "pwconv2.weight": rng.standard_normal((C, 8)) / 8, q + "pwconv2.bias": np.zeros(C), q + "gamma": np.ones(C),
         p + "final_layer_norm.weight": np.ones(C), p + "final_layer_norm.bias": np.zeros(C),
         "enhanced_vocos.head.out.weight": rng.standard_normal((nfft + 2, C)) / 8, "enhanced_vocos.head.out.bias": np.zeros(nfft + 2)}
    orc = _bare_oracle(w, dict(voc_layers=1, n_fft=nfft, hop=hop))
    orc.window = np.hanning(nfft + 1)[:nfft]
    calls = []
    real = co.layer_norm

    def recording(x, lw, lb, eps):
        y = real(x, lw, lb, eps)
        calls.append((np.array(x), np.array(y)))
        return y

    monkeypatch.setattr(co, "layer_norm", recording)
    orc.vocos(rng.standard_normal((B, T, mel)))
    assert len(calls) == 3
    h, (conv, want) = calls[0][1], calls[1]
    dw = w[q + "dwconv.weight"][:, 0, :].T                       # the engine's [7][C]
    got_conv, mag = cr.dwconv_ref(h, dw, w[q + "dwconv.bias"])
    assert np.abs(got_conv - conv).max() <= 1e-12 and (mag >= np.abs(got_conv) - 1e-12).all()
    got, atol = cr.dwconv_ln_ref(h, dw, w[q + "dwconv.bias"], w[q + "norm.weight"], w[q + "norm.bias"], 1e-6)
    assert np.abs(got - want.reshape(B * T, C)).max() <= 1e-12
    assert atol.shape == (B * T, 1) and (atol >= cr.LN_TOL).all()


def test_dwconv_inputs_do_not_leak_between_windows():
    """The inputs make a leak visible: window 1's first rows would move by far more than any tolerance."""
    for T in cr.DW_T:
        h, dw, dwb, lw, lb = cr.dw_inputs(T, 80)
        y, atol = cr.dwconv_ln_ref(h, dw, dwb, lw, lb, 1e-6)
        flat = h.astype(F64).reshape(1, cr.DW_B * T, 80)          # what a kernel that ignores the window boundary would see
        leak = cr.dwconv_ln_ref(flat, dw, dwb, lw, lb, 1e-6)[0]
        assert np.abs(leak[T] - y[T]).max() > 1e3 * float(atol[T, 0])


def test_gelu_and_gemm_ref():
    from scipy.special import erf
    x = np.linspace(-6, 6, 101)
    assert np.abs(cr.gelu(x) - 0.5 * x * (1 + erf(x / np.sqrt(2)))).max() <= 1e-15
    a, w, bias, gamma, res = cr.gemm_inputs(5, 8, 64)
    y, pre, mag = cr.gemm_ref(a, w, bias, 1, gamma, res)
    want = cr.gelu(a.astype(F64) @ w.T.astype(F64) + bias) * gamma + res                 # bias -> GELU -> gamma -> + residual
    assert np.abs(y - want).max() <= 1e-15 and (mag >= np.abs(pre - bias) - 1e-12).all()
    e = cr.b3_bound(mag, 1, gamma, y, True)
    assert (e[:, gamma == 0] <= 2.0 ** -23 * np.abs(y[:, gamma == 0]) + 1e-30).all() and (e >= 0).all()
    assert (gamma == 0).any() and (gamma < 0).any()
    g = cr.vocos_weights()[4]
    assert (g == 0).any() and (g < 0).any() and (g > 0).any()


def test_pack_matches_offset_formula():
    """Element by element against common.h: xpack_off / wpack_off, which are the same map with KT = K / 16."""
    R, K = 45, 64
    m = (np.arange(R * K, dtype=np.uint32) % 65521 + 1).astype(np.uint16).reshape(R, K)
    plane = cr.pack(m, fill=0)
    assert plane.size == 64 * K
    seen = set()
    for r in range(R):
        for k in range(K):
            x = (r >> 5) * 32 * K + (((k >> 4) * 64) + (r & 31) + 32 * ((k >> 3) & 1)) * 8 + (k & 7)
            wp = ((((r >> 5) * (K // 16) + (k >> 4)) * 64) + (r & 31) + 32 * ((k >> 3) & 1)) * 8 + (k & 7)
            assert x == wp == int(cr.pack_off(r, k, K)) and plane[x] == m[r, k]
            seen.add(x)
    assert len(seen) == R * K and int((plane != 0).sum()) == R * K          # one to one; padding rows stay at the fill
    assert np.array_equal(cr.unpack(plane, R, K), m)
    hi, lo = cr.planes_of(np.concatenate([plane, plane[::-1]]), R, K)
    assert np.array_equal(hi, m) and np.array_equal(lo, cr.unpack(plane[::-1], R, K))


def test_split_reproduces_fp32():
    rng = np.random.default_rng(3)
    x = np.concatenate([rng.standard_normal(4000) * 10.0 ** rng.integers(-6, 6, 4000), [0.0, 1.0, -1.0, 1 + 2.0 ** -8, 1 + 2.0 ** -9]]).astype(np.float32)
    hi, lo = cr.split(x)
    assert (np.abs(cr.planes_value(hi, lo) - x.astype(F64)) <= 2.0 ** -16 * np.abs(x.astype(F64))).all()
    # round to nearest even: 1 + 2^-8 is a tie between two bf16 values and goes to the even one
    assert cr.bf16_bits(np.float32(1 + 2.0 ** -8)) == 0x3F80 and cr.bf16_bits(np.float32(1 + 3 * 2.0 ** -8)) == 0x3F82
    import torch
    t = torch.from_numpy(x)
    assert np.array_equal(t.bfloat16().view(torch.int16).numpy().view(np.uint16), hi)
    assert np.array_equal((t - t.bfloat16().float()).bfloat16().view(torch.int16).numpy().view(np.uint16), lo)


def test_case_tables_meet_the_entries_preconditions():
    for B, heads, T, lens, peak in cr.ATTN_CASES:
        assert len(lens) == B and all(0 <= n <= T for n in lens) and heads in (2, 3) and B in (1, 3)
    assert {c[2] for c in cr.ATTN_CASES} == {1, 31, 32, 33, 65, 97, 128, 129, 161}
    assert {c[0] * c[1] for c in cr.ATTN_CASES} >= {2, 6, 9}
    flat = [n for c in cr.ATTN_CASES for n in c[3]]
    assert 0 in flat and 1 in flat and 17 in flat and any(c[4] for c in cr.ATTN_CASES)
    for B, heads, T, lens, peak in cr.ATTN_CASES:
        if peak:
            qkv = cr.attn_inputs(B, heads, T, peak).astype(F64)
            d = 64 * heads
            s = np.einsum("bthd,buhd->bhtu", qkv[..., :d].reshape(B, T, heads, 64), qkv[..., d:2 * d].reshape(B, T, heads, 64)) / 8
            assert abs(np.abs(s).max() - peak) < 1e-3
    for M, N, K, flags, tile, row0, prow, extra in cr.GEMM_PLANES_CASES:
        assert K % 64 == 0 and N % 4 == 0 and row0 % 32 == 0 and extra % 4 == 0 and flags in (0, 4, 6, 9) and tile in cr.TILE_CODES
        assert (prow >= row0 + M) if prow else row0 == 0
        if flags & 8:
            assert N % 16 == 0 and extra == 0
    plain = [c for c in cr.GEMM_PLANES_CASES if not c[4]]
    assert {c[0] for c in plain} >= {1, 33, 130, 257} and {c[1] for c in plain} >= {4, 68, 132, 516}
    assert {c[2] for c in plain} == {64, 128, 512} and {c[3] for c in plain} == {0, 4, 6, 9}
    assert any(c[1] % 8 == 4 and c[3] == 6 for c in plain)                   # N = 4 (mod 8) with bias, gamma and residual
    assert {c[5] for c in plain} >= {32, 96} and all(c[6] > c[5] + c[0] for c in plain if c[5])
    assert {c[4] for c in cr.GEMM_PLANES_CASES} == set(cr.TILE_CODES)
    for name, M, N, K, b_kn in cr.GEMM_EX_CASES:
        assert M >= 1 and N >= 1 and K % 4 == 0
    for C, rows in cr.LN_CASES:
        assert C <= 1024 and C % 16 == 0
    for kernel, C in cr.DW_CASES:
        assert C % 16 == 0 and C <= 1024 and (kernel == 0 or C == 512)
    assert (cr.DW_B * max(cr.DW_T)) % 32 and all((cr.DW_B * T) % 16 for T in cr.DW_T)      # never a multiple of 4 R rows
    for B, heads, T, lens in cr.SOFTMAX_CASES:
        assert len(lens) == B and all(0 <= n <= T for n in lens) and (cr.ld16(T) > 2048) == (T == 2100)
    assert cr.ln_tol(cr.ln_inputs(5, 512)[0]) == cr.LN_TOL
    assert 40 * cr.LN_TOL < cr.ln_tol(cr.ln_inputs(5, 512, 50.0)[0]) < 60 * cr.LN_TOL


@pytest.mark.parametrize("K,D", cr.VQ_CASES)
def test_vq_inputs_are_exact_in_fp32(K, D):
    d = cr.vq_inputs(K, D)
    r, cb, dot, cc = d["r"], d["cb"], d["dot"], d["cc"]
    for a in (r, cb, dot, cc):
        assert np.array_equal(a.astype(np.float32).astype(F64), a)
    # every partial sum is a multiple of 2^-16 below 2^8: exact in fp32 whatever the order
    assert np.array_equal(np.round(r * 256), r * 256) and np.abs(r).max() <= 8 / 256 and np.abs(cb).max() <= 8 / 256
    assert D * (8 / 256) ** 2 <= 1.0
    rr = (r * r).sum(-1)
    comb = (rr[:, None] - 2 * dot) + cc[None, :]
    for a in (rr, rr[:, None] - 2 * dot, comb):
        assert np.array_equal(a.astype(np.float32).astype(F64), a) and np.abs(a).max() < 4
    f = np.float32
    assert np.array_equal(((rr.astype(f)[:, None] - f(2) * dot.astype(f)) + cc.astype(f)[None, :]).astype(F64), comb)
    codes, res = cr.vq_ref(dot, cb, cc, r, cr.VQ_LENS, cr.VQ_T)
    assert np.array_equal(res.astype(np.float32).astype(F64), res)
    # the planted ties: both copies at distance 0, the lower index wins
    for i, (lo, hi) in enumerate(d["dups"]):
        row = 2 * i
        if (row % cr.VQ_T) < cr.VQ_LENS[row // cr.VQ_T]:
            assert comb[row, lo] == comb[row, hi] == comb[row].min() and codes[row] == min(np.flatnonzero(comb[row] == comb[row].min()))
            assert codes[row] <= lo
    valid = (np.arange(r.shape[0]) % cr.VQ_T) < np.asarray(cr.VQ_LENS)[np.arange(r.shape[0]) // cr.VQ_T]
    assert (~valid).any() and np.array_equal(res[~valid], r[~valid]) and (codes[~valid] == cc.argmin()).all()
    if K > 64:
        assert len(d["dups"]) >= 2
