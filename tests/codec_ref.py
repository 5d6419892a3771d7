"""fp64 references, seeded inputs, case tables and error bounds for the codec's kernel tests (numpy only, no GPU).

test_codec_kernels_gpu.py launches each kernel of csrc/codec.hip / codec_fused.hip through its mtts_k_codec_* entry and
compares with the functions here; test_codec_ref_cpu.py checks these functions, the inputs and the case tables on the CPU.
Every bound is built from a tolerance the project already asserts (exact-f32 GEMM: rtol = atol = 2e-5; bf16x3 product:
3e-5 * sum |a||w| + 1e-6, both from test_codec_gpu.py::test_gemm_f32_kernel) or from a rounding count written next to it.
"""
import functools
import math

import numpy as np

F32, F64 = np.float32, np.float64
SENT32 = np.uint32(0xFFC12345)          # a NaN pattern no kernel produces: "never written"
SENT16 = np.uint16(0xFFC1)
B3 = 3e-5                                # the project's bf16x3 product bound, relative to sum |a||w|
B3_ATOL = 1e-6
F32_RTOL = F32_ATOL = 2e-5               # the project's exact-f32 GEMM tolerance
LN_TOL = 1e-5                            # 22 roundings of 2^-24 per sum (16 sequential adds per lane + 6 butterfly steps)
GELU_SLOPE = 1.13                        # max |d GELU / dx| = 1.1289
GELU_FAST_ERR = 7e-7                     # stated at gelu_fast / gelu_fast2 (Abramowitz-Stegun 7.1.26)
TILE_CODES = (0, 2222, 2312, 4221, 3311, 3411, 4311, 4411, 2122, 1222, 1122)

_erf = np.vectorize(math.erf, otypes=[F64])


def gelu(x):
    x = np.asarray(x, F64)
    return 0.5 * x * (1.0 + _erf(x / math.sqrt(2.0)))


def pad32(r):
    return (r + 31) // 32 * 32


# ---- hi / lo split and the fragment-packed layout (common.h: xpack_off = wpack_off with KT = K / 16) ---------------------
def bf16_bits(x):
    """fp32 -> bf16 bits, round to nearest even (finite inputs)."""
    u = np.ascontiguousarray(x, F32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def bf16_f32(b):
    return (np.asarray(b, np.uint16).astype(np.uint32) << 16).view(F32)


def split(x):
    """split2 of codec.hip: hi = bf16(x), lo = bf16(x - hi), both RNE; returns the bit patterns."""
    x = np.ascontiguousarray(x, F32)
    hi = bf16_bits(x)
    lo = bf16_bits(x - bf16_f32(hi))          # x - hi is exact in fp32
    return hi, lo


def pack_off(r, k, K):
    r, k = np.asarray(r, np.int64), np.asarray(k, np.int64)
    return (r >> 5) * 32 * K + (((k >> 4) * 64) + (r & 31) + 32 * ((k >> 3) & 1)) * 8 + (k & 7)


def _offsets(R, K):
    return pack_off(np.arange(R)[:, None], np.arange(K)[None, :], K)


def pack(m, fill=0):
    """[R][K] of uint16 -> one plane of pad32(R) * K elements; positions no element maps to hold `fill`."""
    R, K = m.shape
    out = np.full(pad32(R) * K, fill, np.uint16)
    out[_offsets(R, K)] = m
    return out


def unpack(plane, R, K):
    return np.asarray(plane)[_offsets(R, K)]


def planes_of(buf_u16, R, K, rows_alloc=None):
    """(hi, lo) bit matrices [R][K] out of a buffer holding the hi plane and, pad32(rows_alloc) * K further, the lo plane."""
    n = pad32(R if rows_alloc is None else rows_alloc) * K
    return unpack(buf_u16[:n], R, K), unpack(buf_u16[n:2 * n], R, K)


def planes_value(hi, lo):
    return bf16_f32(hi).astype(F64) + bf16_f32(lo).astype(F64)


# ---- attention -----------------------------------------------------------------------------------------------------------
#   (B, heads, T, lens, peak |score| the queries are scaled to, or 0)
ATTN_CASES = [
    (1, 2, 1, (1,), 0), (3, 3, 1, (1, 0, 1), 0),
    (1, 2, 31, (26,), 0), (3, 2, 31, (31, 17, 1), 0),
    (3, 3, 32, (32, 0, 27), 0), (1, 3, 33, (33,), 0), (3, 2, 33, (28, 1, 33), 0),
    (3, 3, 65, (65, 17, 0), 0), (1, 2, 65, (60,), 0),
    (3, 2, 97, (97, 92, 1), 0), (1, 3, 97, (17,), 0),
    (3, 3, 128, (128, 123, 0), 0), (1, 2, 128, (128,), 0),
    (3, 3, 129, (129, 1, 124), 0), (1, 2, 129, (17,), 0),
    (3, 2, 161, (161, 156, 0), 0), (3, 3, 161, (17, 161, 1), 0),
    (3, 3, 97, (97, 92, 17), 20.0), (1, 2, 161, (161,), 20.0),
]
ATTN_SCALE = 0.125                       # head dim 64


@functools.lru_cache(maxsize=None)
def attn_inputs(B, heads, T, peak):
    d = 64 * heads
    rng = np.random.default_rng(1000 + 97 * B + 13 * heads + T + int(peak))
    qkv = rng.standard_normal((B, T, 3 * d)).astype(F32)
    if peak:
        q = qkv[..., :d].astype(F64).reshape(B, T, heads, 64)
        k = qkv[..., d:2 * d].astype(F64).reshape(B, T, heads, 64)
        s = np.einsum("bthd,buhd->bhtu", q, k) * ATTN_SCALE
        qkv[..., :d] = (qkv[..., :d] * F32(peak / np.abs(s).max())).astype(F32)
    qkv.setflags(write=False)
    return qkv


def attn_ref(qkv, lens, heads):
    """VarLenAttention (modules.py:84-151, as oracle/codec_oracle.py: CodecOracle._layer): a valid query gets softmax
    over keys < len; a padded query the mean of V over ALL T keys.  Returns (out [B][T][d], c [B][heads][T],
    spv [B][T][d]) with spv = sum_j p_j |v_j| and c the relative error the bf16x3 kernels may make on it (attn_bound)."""
    qkv = np.asarray(qkv, F64)
    B, T, d3 = qkv.shape
    d = d3 // 3
    q = qkv[..., :d].reshape(B, T, heads, 64).transpose(0, 2, 1, 3)
    k = qkv[..., d:2 * d].reshape(B, T, heads, 64).transpose(0, 2, 1, 3)
    v = qkv[..., 2 * d:].reshape(B, T, heads, 64).transpose(0, 2, 1, 3)
    s = np.matmul(q, k.transpose(0, 1, 3, 2)) * ATTN_SCALE                        # [B][h][Tq][Tk]
    ds = B3 * ATTN_SCALE * np.matmul(np.abs(q), np.abs(k).transpose(0, 1, 3, 2))   # score error of the bf16x3 product
    valid = np.arange(T)[None, :] < np.asarray(lens)[:, None]                      # [B][T]
    m = (valid[:, :, None] & valid[:, None, :])[:, None]                           # query and key both valid
    qv = valid[:, None, :, None]
    s = np.where(qv, np.where(m, s, -np.inf), 0.0)                                 # padded query: all T keys, equal scores
    e = np.exp(s - s.max(-1, keepdims=True))
    p = e / e.sum(-1, keepdims=True)
    out = np.matmul(p, v).transpose(0, 2, 1, 3).reshape(B, T, d)
    spv = np.matmul(p, np.abs(v)).transpose(0, 2, 1, 3).reshape(B, T, d)
    nkeys = (p > 0).sum(-1)
    dmax = np.where(m, ds, 0.0).max(-1)                                            # largest score error among the keys seen
    dmax = np.where(valid[:, None, :] & (nkeys > 1), dmax, 0.0)                    # one key, or uniform: p is exact
    c = np.expm1(2.0 * dmax) + B3 + np.expm1(2.0 * dmax) * B3
    return out, c, spv


def attn_bound(c, spv, heads):
    """|got - ref| <= c * sum_j p_j |v_j| + 1e-6 for the bf16x3 attention kernels.

    A score is a 64-term bf16x3 product: |ds_ij| <= 3e-5 * scale * sum_d |q_id||k_jd|.  With every score of a row off by
    at most D = max_j ds_ij, p_j = e^{s_j} / sum e^{s} moves by a factor within e^{+-2D} (numerator e^{+-D}, denominator
    e^{-+D}): relative error expm1(2D).  The P.V product is bf16x3 again: another 3e-5 relative to sum p_j |v_j|.  Together
    (1 + expm1(2D)) (1 + 3e-5) - 1.  A row that sees one key has p = 1 exactly, a padded row p = 1/T whatever the scores:
    D = 0 there and the bound collapses to 3e-5 * |v| + 1e-6 -- what a dropped hi*lo term (2^-9 |v|) cannot meet."""
    B, h, T = c.shape
    cc = np.repeat(c.transpose(0, 2, 1), 64, axis=2)                               # [B][T][d]
    return cc * spv + B3_ATOL


# ---- LayerNorm -----------------------------------------------------------------------------------------------------------
LN_CASES = [(C, rows) for C in (80, 512, 768, 1024) for rows in (1, 5, 130)]
LN_WIDE_CASES = [(256, 3), (1000, 5), (3072, 2)]


@functools.lru_cache(maxsize=None)
def ln_inputs(rows, C, offset=0.0, seed=0):
    rng = np.random.default_rng(2000 + 7 * rows + C + seed)
    x = (rng.standard_normal((rows, C)) + offset).astype(F32)
    w = (1.0 + 0.5 * rng.standard_normal(C)).astype(F32)
    b = (0.5 * rng.standard_normal(C)).astype(F32)
    for a in (x, w, b):
        a.setflags(write=False)
    return x, w, b


def layernorm_ref(x, w, b, eps, lens=None, T=1):
    x = np.asarray(x, F64)
    mu = x.mean(-1, keepdims=True)
    var = ((x - mu) ** 2).mean(-1, keepdims=True)
    y = (x - mu) / np.sqrt(var + eps) * np.asarray(w, F64) + np.asarray(b, F64)
    if lens is not None:
        r = np.arange(x.shape[0])
        y[(r % T) >= np.asarray(lens)[r // T]] = 0.0
    return y


def ln_tol(x):
    """rtol = atol: a sum takes at most 22 roundings of 2^-24 (layernorm_kernel: 16 sequential adds per lane + 6 butterfly
    steps; layernorm_wide_kernel: <= 12 per thread at C <= 3072, + 6 butterfly steps + 3 adds over the waves = 21), so mean
    and variance are off by <= 1.3e-6 relative to mean |x| and the normalised value by a few of those: 1e-5 at unit
    scale.  An offset input loses mean|x| / sigma more in x - mu.  (A one-pass variance E[x^2] - mu^2 loses that factor
    SQUARED: at mean = 50 sigma it may still slip under this tolerance, at 1000 sigma it cannot, so both are run.)"""
    x = np.asarray(x, F64)
    return LN_TOL * max(1.0, float((np.abs(x).mean(-1) / x.std(-1)).max()))


# ---- depthwise conv (k = 7, pad 3, per window) + LayerNorm ----------------------------------------------------------------
#   (kernel, C): kernel 0 = dwconv_ln_kernel, 4 / 8 = dwconv_ln512_kernel<R>
DW_CASES = [(4, 512), (8, 512), (0, 512), (0, 80), (0, 768)]
DW_T = (1, 3, 7, 37)
DW_B = 2


@functools.lru_cache(maxsize=None)
def dw_inputs(T, C):
    """Two windows; window 0 ends in (up to) three rows of huge values that window 1 must not see."""
    rng = np.random.default_rng(3000 + 11 * T + C)
    h = rng.standard_normal((DW_B, T, C)).astype(F32)
    h[0, max(0, T - 3):] *= F32(1e4)
    dw = (rng.standard_normal((7, C)) * 0.4).astype(F32)
    dwb = (rng.standard_normal(C) * 0.2).astype(F32)
    lw = (1.0 + 0.5 * rng.standard_normal(C)).astype(F32)
    lb = (0.5 * rng.standard_normal(C)).astype(F32)
    for a in (h, dw, dwb, lw, lb):
        a.setflags(write=False)
    return h, dw, dwb, lw, lb


def dwconv_ref(h, dw, dwb):
    """[B][T][C]; y[b,t] = bias + sum_j h[b, t + j - 3] * dw[j], taps in order, zeros outside the window.  Also returns
    sum |h||dw| + |bias|, the scale of the conv's own roundings."""
    h, dw = np.asarray(h, F64), np.asarray(dw, F64)
    B, T, C = h.shape
    hp = np.pad(h, ((0, 0), (3, 3), (0, 0)))
    y = np.broadcast_to(np.asarray(dwb, F64), h.shape).copy()
    mag = np.abs(y)
    for j in range(7):
        y += hp[:, j:j + T] * dw[j]
        mag += np.abs(hp[:, j:j + T] * dw[j])
    return y, mag


def dwconv_ln_ref(h, dw, dwb, lw, lb, eps):
    """-> (y [B T][C], atol [B T][1]).  Tolerance as LayerNorm's, plus the conv's 7 products and 7 adds (14 roundings of
    2^-24 relative to sum |h||dw| + |bias|), which reach the output divided by the row's sigma and times |lw|, once
    directly and once through the mean / variance."""
    v, mag = dwconv_ref(h, dw, dwb)
    B, T, C = v.shape
    v, mag = v.reshape(B * T, C), mag.reshape(B * T, C)
    y = layernorm_ref(v, lw, lb, eps)
    sig = np.sqrt(v.var(-1, keepdims=True) + eps)
    conv = 2.0 * 14 * 2.0 ** -24 * mag.max(-1, keepdims=True) / sig * float(np.abs(lw).max())
    ln = LN_TOL * np.maximum(1.0, np.abs(v).mean(-1, keepdims=True) / sig)
    return y, ln + conv


# ---- masked softmax ------------------------------------------------------------------------------------------------------
#   (B, heads, T, lens)
SOFTMAX_CASES = [(3, 2, 5, (5, 1, 0)), (3, 1, 16, (16, 0, 1)), (3, 2, 100, (100, 1, 37)), (2, 1, 2047, (2047, 1)),
                 (1, 1, 2047, (0,)), (2, 1, 2100, (2100, 1)), (2, 1, 2100, (0, 1500))]


def ld16(T):
    return (T + 15) // 16 * 16


@functools.lru_cache(maxsize=2)
def softmax_inputs(B, heads, T):
    rng = np.random.default_rng(3500 + B + heads + T)
    S = (3.0 * rng.standard_normal((B, heads, T, ld16(T)))).astype(F32)
    S.setflags(write=False)
    return S


def softmax_mask_ref(S, lens, T):
    """S [B][heads][T][ldT] -> P: valid query: softmax over keys < len, exactly 0 elsewhere; padded query: 1/T on all T
    keys; columns [T, ldT) zero."""
    S = np.asarray(S, F64)
    B, H, Tq, ldT = S.shape
    assert Tq == T
    P = np.zeros_like(S)
    for b in range(B):
        n = int(lens[b])
        if n:
            s = S[b, :, :n, :n]
            e = np.exp(s - s.max(-1, keepdims=True))
            P[b, :, :n, :n] = e / e.sum(-1, keepdims=True)
        P[b, :, n:, :T] = 1.0 / T
    return P


# ---- one RVQ stage -------------------------------------------------------------------------------------------------------
VQ_CASES = [(K, D) for K in (7, 256, 1024) for D in (8, 512)]
VQ_B, VQ_T, VQ_LENS = 2, 9, (9, 4)


@functools.lru_cache(maxsize=None)
def vq_inputs(K, D):
    """Residual and codebook entries are integers in [-8, 8] times 2^-8: every product is a multiple of 2^-16 below 2^-10,
    every partial sum of |r|^2, r.c and |c|^2 over D <= 512 terms a multiple of 2^-16 below 1, and (rr - 2 dot) + cc one
    below 4: all exact in fp32 in any summation order (test_codec_ref_cpu.py asserts it).  Codebook rows are duplicated
    across the kernel's strides (j, j + 64: two waves; j, j + 256: two rounds of one thread) and some residual rows ARE
    such a row, so the minimum is an exact tie and the lowest index must win."""
    rng = np.random.default_rng(4000 + K + D)
    cb = rng.integers(-8, 9, (K, D)).astype(F64) / 256.0
    dups = [(j, j + o) for j, o in ((3, 64), (70, 256), (1, 4), (130, 64)) if j + o < K]
    for lo, hi in dups:
        cb[hi] = cb[lo]
    rows = VQ_B * VQ_T
    r = rng.integers(-8, 9, (rows, D)).astype(F64) / 256.0
    for i, (lo, hi) in enumerate(dups):
        r[2 * i] = cb[hi]                     # distance 0 to both copies
    dot = r @ cb.T
    cc = (cb * cb).sum(-1)
    out = dict(cb=cb, r=r, dot=dot, cc=cc, dups=dups)
    for a in (cb, r, dot, cc):
        a.setflags(write=False)
    return out


def vq_ref(dot, cb, cc, r, lens, T):
    """-> (codes, residual) in fp64; np.argmin returns the first index of the minimum."""
    rows = r.shape[0]
    valid = (np.arange(rows) % T) < np.asarray(lens)[np.arange(rows) // T]
    rr = np.where(valid, (r * r).sum(-1), 0.0)
    dist = (rr[:, None] - 2.0 * np.where(valid[:, None], dot, 0.0)) + cc[None, :]
    codes = dist.argmin(-1)
    out = np.where(valid[:, None], r - cb[codes], r)
    return codes.astype(np.int64), out


# ---- GEMMs ---------------------------------------------------------------------------------------------------------------
def gemm_ref(a, w, bias=None, act=0, gamma=None, res=None, scale=1.0):
    """((a w^T + bias) * scale) -> GELU -> * gamma -> + res, fp64.  Also returns the pre-activation and sum |a||w|."""
    a, w = np.asarray(a, F64), np.asarray(w, F64)
    pre = a @ w.T
    if bias is not None:
        pre = pre + np.asarray(bias, F64)
    pre = pre * scale
    y = gelu(pre) if act else pre
    if gamma is not None:
        y = y * np.asarray(gamma, F64)
    if res is not None:
        y = y + np.asarray(res, F64)
    return y, pre, np.abs(a) @ np.abs(w).T


def b3_bound(mag, act=0, gamma=None, out=None, res=False):
    """Error bound of the pre-split bf16x3 GEMM's output: 3e-5 * sum |a||w| + 1e-6 on the pre-activation, carried through
    the epilogue: * 1.13 (GELU's largest slope) + 7e-7 (the fast formula's own error), * |gamma|, + one fp32 ulp (2^-23
    relative) of the result for the residual add."""
    e = B3 * mag + B3_ATOL
    if act:
        e = GELU_SLOPE * e + GELU_FAST_ERR
    if gamma is not None:
        e = e * np.abs(np.asarray(gamma, F64))
    if res:
        e = e + 2.0 ** -23 * np.abs(out)
    return e


#   (M, N, K, flags, tile, row0, plane_rows, extra ldc): flags 1 GELU | 2 gamma | 4 residual | 8 plane output
GEMM_PLANES_CASES = [
    (1, 4, 64, 0, 0, 0, 0, 0), (33, 68, 128, 4, 0, 0, 0, 0), (130, 132, 512, 6, 0, 0, 0, 0), (257, 516, 64, 6, 0, 0, 0, 0),
    (33, 516, 128, 0, 0, 0, 0, 0), (257, 68, 512, 4, 0, 0, 0, 0), (130, 4, 128, 6, 0, 0, 0, 0), (1, 132, 64, 4, 0, 0, 0, 0),
    (33, 68, 128, 4, 0, 0, 0, 8), (130, 132, 64, 0, 0, 0, 0, 4),                      # ldc > N: the columns between keep the sentinel
    (130, 144, 128, 9, 0, 0, 0, 0), (33, 64, 64, 9, 0, 0, 0, 0), (257, 528, 64, 9, 0, 0, 0, 0), (1, 16, 512, 9, 0, 0, 0, 0),
    (33, 68, 64, 6, 0, 32, 100, 0), (40, 132, 128, 4, 0, 96, 160, 0), (33, 64, 64, 9, 0, 32, 96, 0), (31, 144, 128, 9, 0, 96, 130, 0),
    (130, 4, 64, 0, 0, 32, 200, 0),
] + [(130, 132, 128, 6, t, 0, 0, 0) for t in TILE_CODES[1:]] + [(130, 144, 64, 9, t, 0, 0, 0) for t in TILE_CODES[1:]]


@functools.lru_cache(maxsize=None)
def gemm_inputs(R, N, K, seed=0):
    rng = np.random.default_rng(5000 + 3 * R + 5 * N + K + seed)
    a = rng.standard_normal((R, K)).astype(F32)
    w = (rng.standard_normal((N, K)) / np.sqrt(K)).astype(F32)
    bias = rng.standard_normal(N).astype(F32)
    gamma = rng.standard_normal(N).astype(F32)
    gamma[::7] = 0.0
    res = rng.standard_normal((R, N)).astype(F32)
    for x in (a, w, bias, gamma, res):
        x.setflags(write=False)
    return a, w, bias, gamma, res


#   general gemm_f32: (name, M, N, K, b_kn)
GEMM_EX_CASES = [("kn_n5", 33, 5, 20, 1), ("kn_n64", 130, 64, 36, 1), ("kn_n130", 7, 130, 20, 1),
                 ("nk_k4", 33, 70, 4, 0), ("nk_k20", 130, 9, 20, 0)]
GEMM_EX_GRIDS = [(3, 5), (9, 1), (1, 9)]  # tiles of 128 along (M, N) with the XCD map on


# ---- fused Vocos pointwise pair ------------------------------------------------------------------------------------------
VOCOS_M = (1, 63, 64, 65, 129)
VD, VI = 512, 4096


@functools.lru_cache(maxsize=None)
def vocos_weights():
    rng = np.random.default_rng(6000)
    w1 = (rng.standard_normal((VI, VD)) / np.sqrt(VD)).astype(F32)
    b1 = (0.3 * rng.standard_normal(VI)).astype(F32)
    w2 = (rng.standard_normal((VD, VI)) / np.sqrt(VI)).astype(F32)
    b2 = (0.3 * rng.standard_normal(VD)).astype(F32)
    gamma = rng.standard_normal(VD).astype(F32)          # random sign; some exactly zero
    gamma[::9] = 0.0
    for x in (w1, b1, w2, b2, gamma):
        x.setflags(write=False)
    return w1, b1, w2, b2, gamma


@functools.lru_cache(maxsize=None)
def vocos_inputs(M):
    rng = np.random.default_rng(6100 + M)
    rows = (M + 63) // 64 * 64 + 32                       # rows past M: must stay as they are
    xn = rng.standard_normal((M, VD)).astype(F32)
    h = rng.standard_normal((rows, VD)).astype(F32)
    xn.setflags(write=False)
    h.setflags(write=False)
    return xn, h


@functools.lru_cache(maxsize=None)
def vocos_ref(M):
    """-> (h' [M][512], bound [M][512]).  Bound: the intermediate's 3e-5 * sum |x||w1| (+ 1e-6), through GELU (* 1.13 +
    7e-7), through |W2|, plus the second product's 3e-5 * sum |g||w2|, times |gamma|, plus 1e-6."""
    w1, b1, w2, b2, gamma = vocos_weights()
    xn, h = vocos_inputs(M)
    g, _, mag1 = gemm_ref(xn, w1, b1, act=1)
    y, _, mag2 = gemm_ref(g, w2, b2)
    e_g = GELU_SLOPE * (B3 * mag1 + B3_ATOL) + GELU_FAST_ERR
    e_y = e_g @ np.abs(w2.astype(F64)).T + B3 * mag2
    out = h[:M].astype(F64) + gamma.astype(F64) * y
    return out, np.abs(gamma.astype(F64)) * e_y + B3_ATOL
