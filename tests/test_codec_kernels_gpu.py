"""The codec's kernels (csrc/codec.hip, csrc/codec_fused.hip), one launch function of the engine each, against the fp64
references of tests/codec_ref.py.  -m gpu.

Every entry (mtts_k_codec_*, include/mtts.h) calls the launch function the engine itself calls.  Output buffers start as
a sentinel pattern and every element a kernel must not write has to keep it.  Bounds come from codec_ref.py: the
project's exact-f32 tolerance, its bf16x3 product bound carried through each epilogue, or a rounding count; each test
prints its worst error / bound ratio ("RATIO <group> <value>") before it asserts.  test_codec_ref_cpu.py checks the
references, the inputs and the case tables on the CPU.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import codec_ref as cr  # noqa: E402
from mtts import capi  # noqa: E402
from mtts.codec import _check  # noqa: E402

F32, F64 = np.float32, np.float64


def _lib():
    return capi.lib()


def _dev(a):
    return torch.from_numpy(np.array(a, dtype=F32, order="C")).cuda()         # a copy: the shared inputs are read-only


def _ptr(t, off=0):
    return None if t is None else t.data_ptr() + 4 * off


def _sent32(n):
    return torch.from_numpy(np.full(int(n), cr.SENT32, np.uint32).view(np.int32)).cuda()


def _sent16(n):
    return torch.from_numpy(np.full(int(n), cr.SENT16, np.uint16).view(np.int16)).cuda()


def _u32(t):
    torch.cuda.synchronize()
    return t.cpu().numpy().view(np.uint32)


def _u16(t):
    torch.cuda.synchronize()
    return t.cpu().numpy().view(np.uint16)


def _lens(lens):
    return np.ascontiguousarray(lens, dtype=np.int32)


def _ratio(group, err, bound):
    r = float(np.max(np.asarray(err, F64) / np.asarray(bound, F64)))
    print("RATIO %s %.4f" % (group, r))
    return r


def _check_bound(group, got, ref, bound, what):
    got = np.asarray(got, F64)
    assert np.isfinite(got).all(), (what, "not finite", np.argwhere(~np.isfinite(got))[:5].tolist())
    err = np.abs(got - ref)
    bound = np.broadcast_to(bound, err.shape)
    r = _ratio(group, err, bound)
    bad = np.argwhere(err > bound)
    assert bad.size == 0, (what, "error / bound", r, "first offenders", bad[:5].tolist(), len(bad))


def _check_close(group, got, ref, rtol, atol, what):
    _check_bound(group, got, ref, atol + rtol * np.abs(ref), what)


def _written(u, mask, sent, what):
    """Exactly the elements of `mask` were written: the others keep the sentinel, and none of those is a sentinel."""
    assert (u[~mask] == sent).all(), (what, "written where nothing may be written", np.argwhere(~mask & (u != sent))[:5].tolist())
    assert (u[mask] != sent).all(), (what, "left unwritten", np.argwhere(mask & (u == sent))[:5].tolist())


def _plane_mask(R, K, rows_alloc=None, row0=0, M=None):
    """Positions of rows row0 .. row0 + M - 1 in a (hi, lo) buffer laid out for rows_alloc rows of K."""
    n = cr.pad32(R if rows_alloc is None else rows_alloc) * K
    M = R - row0 if M is None else M
    off = cr.pack_off(np.arange(row0, row0 + M)[:, None], np.arange(K)[None, :], K).ravel()
    mask = np.zeros(2 * n, bool)
    mask[off] = True
    mask[n + off] = True
    return mask


def _assert_bits(got, want, what):
    bad = np.argwhere(got != want)
    assert bad.size == 0, (what, "first differing (row, column)", bad[:5].tolist(), len(bad))


# ---- attention -----------------------------------------------------------------------------------------------------------
def _attn(qkv, lens, B, T, heads, mode, planes):
    d, rows = 64 * heads, B * T
    if planes:
        out = _sent16(2 * cr.pad32(rows) * d)
    else:
        out = _sent32(rows * d + 64)
    _check(_lib().mtts_k_codec_attn(qkv.data_ptr(), _lens(lens).ctypes.data, out.data_ptr(), B, T, heads, mode, int(planes), None))
    if planes:
        u = _u16(out)
        _written(u, _plane_mask(rows, d), cr.SENT16, ("attn planes", mode, B, heads, T))
        return cr.planes_of(u, rows, d)
    u = _u32(out)
    assert (u[rows * d:] == cr.SENT32).all(), ("attn", mode, "wrote past the last row")
    assert (u[:rows * d] != cr.SENT32).all(), ("attn", mode, "left elements unwritten")
    return u[:rows * d].view(F32).reshape(B, T, d)


@pytest.mark.parametrize("B,heads,T,lens,peak", cr.ATTN_CASES)
def test_codec_attention(B, heads, T, lens, peak):
    """Three-launch form (exact f32) and both fused bf16x3 kernels against fp64; plane output = split of the fp32 output."""
    qkv_h = cr.attn_inputs(B, heads, T, peak)
    ref, c, spv = cr.attn_ref(qkv_h, lens, heads)
    bound = cr.attn_bound(c, spv, heads)
    qkv = _dev(qkv_h)
    tag = "peak" if peak else "unit"
    got0 = _attn(qkv, lens, B, T, heads, 0, False)
    _check_close("attn3_" + tag, got0, ref, cr.F32_RTOL, cr.F32_ATOL, ("attn mode 0", B, heads, T, lens))
    v = qkv_h[..., 128 * heads:].astype(F64)
    for mode in (1, 2):
        got = _attn(qkv, lens, B, T, heads, mode, False)
        _check_bound("attn_fused%d_%s" % (mode, tag), got, ref, bound, ("attn mode", mode, B, heads, T, lens))
        for b, n in enumerate(lens):
            if n == 1:            # one key: the row is V[0] to the product's own error -- a dropped hi*lo term is 2^-9 |v|
                _check_bound("attn_fused%d_len1" % mode, got[b, 0], v[b, 0], cr.B3 * np.abs(v[b, 0]) + cr.B3_ATOL, ("len 1", mode))
            if n < T:             # padded queries: the mean of V over all T keys
                mean = np.broadcast_to(v[b].mean(0), (T - n, v.shape[-1]))
                _check_bound("attn_fused%d_pad" % mode, got[b, n:], mean, cr.B3 * np.abs(v[b]).mean(0) + cr.B3_ATOL, ("padded rows", mode))
        hi, lo = _attn(qkv, lens, B, T, heads, mode, True)
        whi, wlo = cr.split(got.reshape(B * T, -1))
        _assert_bits(hi, whi, ("attn hi plane", mode, B, heads, T))
        _assert_bits(lo, wlo, ("attn lo plane", mode, B, heads, T))


def test_codec_attention_refuses_bad_arguments():
    qkv = _dev(cr.attn_inputs(1, 2, 31, 0))
    out = _sent32(31 * 128)
    L = _lib()
    assert L.mtts_k_codec_attn(qkv.data_ptr(), _lens([32]).ctypes.data, out.data_ptr(), 1, 31, 2, 1, 0, None) != 0      # len > T
    assert L.mtts_k_codec_attn(qkv.data_ptr(), _lens([3]).ctypes.data, out.data_ptr(), 1, 31, 2, 3, 0, None) != 0       # no mode 3
    assert L.mtts_k_codec_attn(qkv.data_ptr(), _lens([3]).ctypes.data, out.data_ptr(), 1, 31, 2, 0, 1, None) != 0       # mode 0 has no planes
    assert (_u32(out) == cr.SENT32).all()


# ---- pre-split bf16x3 GEMM -----------------------------------------------------------------------------------------------
def _gemm_planes(a, w, bias, gamma, res, M, N, K, ldc, flags, tile, row0, prow, nt_out):
    R = prow or M
    if flags & 8:
        out = _sent16(2 * cr.pad32(R) * N)
    else:
        out = _sent32(R * ldc)
    _check(_lib().mtts_k_codec_gemm_planes(a.data_ptr(), w.data_ptr(), _ptr(bias), _ptr(gamma), _ptr(res), out.data_ptr(), M, N, K, ldc,
                                           flags, tile, row0, prow, nt_out, None))
    return _u16(out) if flags & 8 else _u32(out).reshape(R, ldc)


@pytest.mark.parametrize("M,N,K,flags,tile,row0,prow,extra", cr.GEMM_PLANES_CASES)
def test_codec_gemm_planes(M, N, K, flags, tile, row0, prow, extra):
    R, ldc = prow or M, N + extra
    a_h, w_h, bias_h, gamma_h, res_h = cr.gemm_inputs(R, N, K)
    res_ld = np.full((R, ldc), 7.0, F32)
    res_ld[:, :N] = res_h
    gam = gamma_h if flags & 2 else None
    rs = res_h[row0:row0 + M] if flags & 4 else None
    ref, pre, mag = cr.gemm_ref(a_h[row0:row0 + M], w_h, bias_h, flags & 1, gam, rs)
    bound = cr.b3_bound(mag, flags & 1, gam, ref, bool(flags & 4))
    a, w, bias = _dev(a_h), _dev(w_h), _dev(bias_h)
    gamma = _dev(gamma_h) if flags & 2 else None
    res = _dev(res_ld) if flags & 4 else None
    what = ("gemm_planes", M, N, K, flags, tile, row0, prow, extra)
    group = "b3t_flags%d" % flags
    if flags & 8:
        u = [_gemm_planes(a, w, bias, gamma, res, M, N, K, ldc, flags, tile, row0, prow, nt) for nt in (0, 1)]
        assert np.array_equal(u[0], u[1]), (what, "nontemporal and plain stores differ")
        _written(u[0], _plane_mask(R, N, R, row0, M), cr.SENT16, what)
        hi, lo = cr.planes_of(u[0], R, N)
        val = cr.planes_value(hi[row0:row0 + M], lo[row0:row0 + M])
        # the planes hold split(v) of the fp32 result v: hi + lo is v to 2^-16 relative (test_codec_ref_cpu.py)
        _check_bound(group, val, ref, bound + 2.0 ** -16 * np.abs(ref), what)
        # lo is the remainder of rounding to hi: at most half a bf16 ulp of hi, 2^-8 |hi|
        hf, lf = (cr.bf16_f32(x[row0:row0 + M]).astype(F64) for x in (hi, lo))
        assert (np.abs(lf) <= 2.0 ** -8 * np.abs(hf)).all(), (what, "lo plane is not a rounding remainder of the hi plane")
        return
    u = _gemm_planes(a, w, bias, gamma, res, M, N, K, ldc, flags, tile, row0, prow, 1)
    mask = np.zeros((R, ldc), bool)
    mask[row0:row0 + M, :N] = True
    _written(u, mask, cr.SENT32, what)
    _check_bound(group, u.view(F32)[row0:row0 + M, :N], ref, bound, what)


def test_codec_gemm_planes_tile_codes_agree_bit_for_bit():
    M, N, K = 130, 132, 128
    a_h, w_h, bias_h, gamma_h, res_h = cr.gemm_inputs(M, N, K)
    a, w, bias, gamma, res = (_dev(x) for x in (a_h, w_h, bias_h, gamma_h, res_h))
    outs = [_gemm_planes(a, w, bias, gamma, res, M, N, K, N, 6, t, 0, 0, 1) for t in cr.TILE_CODES]
    for t, o in zip(cr.TILE_CODES, outs):
        assert np.array_equal(o, outs[0]), t


def test_codec_gemm_planes_refuses_bad_arguments():
    a_h, w_h, bias_h, gamma_h, res_h = cr.gemm_inputs(33, 68, 128)
    a, w, bias, gamma, res = (_dev(x) for x in (a_h, w_h, bias_h, gamma_h, res_h))
    out = _sent32(33 * 68)
    L = _lib()

    def call(M=33, N=68, K=128, ldc=68, flags=0, tile=0, row0=0, prow=0, g=None, r=None):
        return L.mtts_k_codec_gemm_planes(a.data_ptr(), w.data_ptr(), bias.data_ptr(), _ptr(g), _ptr(r), out.data_ptr(), M, N, K, ldc,
                                          flags, tile, row0, prow, 1, None)
    assert call(K=96) != 0 and call(N=66, ldc=66) != 0 and call(M=1, row0=16, prow=33) != 0 and call(M=2, row0=32, prow=33) != 0
    assert call(flags=2, g=gamma) != 0 and call(flags=1) != 0 and call(flags=6, g=gamma) != 0 and call(flags=9) != 0      # 68 % 16
    assert call(tile=1234) != 0 and call(ldc=64) != 0
    assert (_u32(out) == cr.SENT32).all()
    assert call() == 0


# ---- fused Vocos pointwise pair ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def vocos_dev():
    return [_dev(x) for x in cr.vocos_weights()]


@pytest.mark.parametrize("M", cr.VOCOS_M)
def test_codec_vocos_pw_fused(M, vocos_dev):
    w1, b1, w2, b2, gamma = vocos_dev
    xn_h, h_h = cr.vocos_inputs(M)
    ref, bound = cr.vocos_ref(M)
    xn, h = _dev(xn_h), _dev(h_h)
    _check(_lib().mtts_k_codec_vocos_pw(xn.data_ptr(), w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr(), gamma.data_ptr(),
                                        h.data_ptr(), M, None))
    got = _u32(h).reshape(h_h.shape)
    _assert_bits(got[M:], h_h[M:].view(np.uint32), ("vocos_pw rows past M", M))
    _check_bound("vocos_fused", got.view(F32)[:M], ref, bound, ("vocos_pw fused", M))
    g0 = cr.vocos_weights()[4] == 0
    _assert_bits(got[:M, g0], h_h[:M, g0].view(np.uint32), ("vocos_pw gamma = 0 columns", M))
    # the same operands through the two launches the engine uses for the rows the fused kernel leaves
    mid = _gemm_planes(xn, w1, b1, None, None, M, cr.VI, cr.VD, cr.VI, 9, 0, 0, 0, 1)
    g32 = cr.planes_value(*cr.planes_of(mid, M, cr.VI)).astype(F32)
    out = _gemm_planes(_dev(g32), w2, b2, gamma, _dev(h_h[:M]), M, cr.VD, cr.VI, cr.VD, 6, 0, 0, 0, 1)
    _check_bound("vocos_two_launch", out.view(F32), ref, bound, ("vocos_pw two launches", M))
    # Same splits and same products in both forms; only the fp32 summation order of the second GEMM's 4096 terms (and exp2
    # against exp in GELU) differs: a random walk of 64 roundings of 2^-24 on sums of size ~0.6, about 2e-6.  The project's
    # figure for this pair is 1e-5 RMS (test_parity_scale_gpu.py); a dropped hi*lo term moves the result by ~2e-4.
    dif = got.view(F32)[:M].astype(F64) - out.view(F32).astype(F64)
    rms = float(np.sqrt(np.mean(dif ** 2)))
    print("RATIO vocos_fused_vs_two_rms %.4f" % (rms / 1e-5))
    assert rms <= 1e-5, ("fused vs two launches", M, rms)


# ---- LayerNorm -----------------------------------------------------------------------------------------------------------
def _layernorm(x_h, w_h, b_h, eps, lens=None, T=1, extra=0, planes=False):
    rows, Cc = x_h.shape
    ldy = Cc + extra
    x, w, b = _dev(x_h), _dev(w_h), _dev(b_h)
    out = _sent16(2 * cr.pad32(rows) * Cc) if planes else _sent32(rows * ldy)
    lp = None if lens is None else _lens(lens).ctypes.data
    _check(_lib().mtts_k_codec_layernorm(x.data_ptr(), w.data_ptr(), b.data_ptr(), out.data_ptr(), rows, Cc, C.c_float(eps), lp, T, ldy,
                                         int(planes), None))
    if planes:
        u = _u16(out)
        _written(u, _plane_mask(rows, Cc), cr.SENT16, ("layernorm planes", rows, Cc))
        return cr.planes_of(u, rows, Cc)
    u = _u32(out).reshape(rows, ldy)
    mask = np.zeros((rows, ldy), bool)
    mask[:, :Cc] = True
    _written(u, mask, cr.SENT32, ("layernorm", rows, Cc, extra))
    return u.view(F32)[:, :Cc]


@pytest.mark.parametrize("Cc,rows", cr.LN_CASES)
def test_codec_layernorm(Cc, rows):
    x, w, b = cr.ln_inputs(rows, Cc)
    tol = cr.ln_tol(x)
    ref = cr.layernorm_ref(x, w, b, 1e-5)
    got = _layernorm(x, w, b, 1e-5)
    _check_close("layernorm", got, ref, tol, tol, ("layernorm", Cc, rows))
    assert np.array_equal(_layernorm(x, w, b, 1e-5, extra=8).view(np.uint32), got.view(np.uint32)), "ldy > C changes the values"
    hi, lo = _layernorm(x, w, b, 1e-5, planes=True)
    whi, wlo = cr.split(got)
    _assert_bits(hi, whi, ("layernorm hi plane", Cc, rows))
    _assert_bits(lo, wlo, ("layernorm lo plane", Cc, rows))


@pytest.mark.parametrize("Cc", [80, 512, 1024])
def test_codec_layernorm_offset_and_masking(Cc):
    """mean = 50 sigma and 1000 sigma (where a one-pass variance has lost everything), and rows past a window's length
    written as exact zeros."""
    for offset in (50.0, 1000.0):         # at 1000 sigma E[x^2] - mu^2 has no digit left in fp32; x - mu keeps the tolerance
        x, w, b = cr.ln_inputs(10, Cc, offset)
        tol = cr.ln_tol(x)
        assert 0.8 * offset * cr.LN_TOL < tol < 1.2 * offset * cr.LN_TOL
        _check_close("layernorm_offset", _layernorm(x, w, b, 1e-6), cr.layernorm_ref(x, w, b, 1e-6), tol, tol, ("layernorm offset", Cc, offset))
    x, w, b = cr.ln_inputs(10, Cc)
    for lens in ((3, 0), (0, 5), (5, 4)):
        got = _layernorm(x, w, b, 1e-5, lens=lens, T=5, extra=4)
        ref = cr.layernorm_ref(x, w, b, 1e-5, lens=lens, T=5)
        _check_close("layernorm", got, ref, cr.LN_TOL, cr.LN_TOL, ("layernorm masked", Cc, lens))
        dead = np.concatenate([np.arange(5) >= lens[0], np.arange(5) >= lens[1]])
        assert (got.view(np.uint32)[dead] == 0).all(), ("masked rows are not +0", lens)
        hi, lo = _layernorm(x, w, b, 1e-5, lens=lens, T=5, planes=True)
        whi, wlo = cr.split(got)
        _assert_bits(hi, whi, ("masked layernorm hi plane", Cc, lens))
        _assert_bits(lo, wlo, ("masked layernorm lo plane", Cc, lens))


@pytest.mark.parametrize("Cc,rows", cr.LN_WIDE_CASES)
def test_codec_layernorm_wide(Cc, rows):
    for offset in (0.0, 50.0, 1000.0):
        x_h, w_h, b_h = cr.ln_inputs(rows, Cc, offset, seed=1)
        tol = cr.ln_tol(x_h)
        x, w, b = _dev(x_h), _dev(w_h), _dev(b_h)
        out = _sent32((rows + 1) * Cc)
        _check(_lib().mtts_k_codec_layernorm_wide(x.data_ptr(), w.data_ptr(), b.data_ptr(), out.data_ptr(), rows, Cc, C.c_float(1e-5), None))
        u = _u32(out).reshape(rows + 1, Cc)
        mask = np.zeros((rows + 1, Cc), bool)
        mask[:rows] = True
        _written(u, mask, cr.SENT32, ("layernorm_wide", Cc, rows))
        _check_close("layernorm_wide" + ("_offset" if offset else ""), u.view(F32)[:rows], cr.layernorm_ref(x_h, w_h, b_h, 1e-5), tol, tol,
                     ("layernorm_wide", Cc, rows, offset))


# ---- depthwise conv + LayerNorm ------------------------------------------------------------------------------------------
def _dwconv_ln(T, Cc, kernel, planes):
    h_h, dw_h, dwb_h, lw_h, lb_h = cr.dw_inputs(T, Cc)
    rows = cr.DW_B * T
    h, dw, dwb, lw, lb = (_dev(x) for x in (h_h, dw_h, dwb_h, lw_h, lb_h))
    out = _sent16(2 * cr.pad32(rows) * Cc) if planes else _sent32((rows + 1) * Cc)
    _check(_lib().mtts_k_codec_dwconv_ln(h.data_ptr(), dw.data_ptr(), dwb.data_ptr(), lw.data_ptr(), lb.data_ptr(), out.data_ptr(),
                                         cr.DW_B, T, Cc, C.c_float(1e-6), kernel, int(planes), None))
    if planes:
        u = _u16(out)
        _written(u, _plane_mask(rows, Cc), cr.SENT16, ("dwconv_ln planes", kernel, T, Cc))
        return cr.planes_of(u, rows, Cc)
    u = _u32(out).reshape(rows + 1, Cc)
    mask = np.zeros((rows + 1, Cc), bool)
    mask[:rows] = True
    _written(u, mask, cr.SENT32, ("dwconv_ln", kernel, T, Cc))
    return u.view(F32)[:rows]


@pytest.mark.parametrize("T", cr.DW_T)
@pytest.mark.parametrize("kernel,Cc", cr.DW_CASES)
def test_codec_dwconv_ln(kernel, Cc, T):
    h, dw, dwb, lw, lb = cr.dw_inputs(T, Cc)
    ref, atol = cr.dwconv_ln_ref(h, dw, dwb, lw, lb, 1e-6)
    got = _dwconv_ln(T, Cc, kernel, False)
    _check_bound("dwconv_ln", got, ref, atol + cr.LN_TOL * np.abs(ref), ("dwconv_ln", kernel, Cc, T))
    hi, lo = _dwconv_ln(T, Cc, kernel, True)
    whi, wlo = cr.split(got)
    _assert_bits(hi, whi, ("dwconv_ln hi plane", kernel, Cc, T))
    _assert_bits(lo, wlo, ("dwconv_ln lo plane", kernel, Cc, T))


@pytest.mark.parametrize("T", cr.DW_T)
def test_codec_dwconv_ln512_rows_per_wave_agree_bit_for_bit(T):
    a, b = _dwconv_ln(T, 512, 4, False), _dwconv_ln(T, 512, 8, False)
    _assert_bits(a.view(np.uint32), b.view(np.uint32), ("dwconv_ln512 <4> vs <8>", T))


# ---- masked softmax ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,heads,T,lens", cr.SOFTMAX_CASES)
def test_codec_softmax_mask(B, heads, T, lens):
    S_h = cr.softmax_inputs(B, heads, T)
    ldT = S_h.shape[-1]
    S = _dev(S_h)
    guard = _sent32(64)
    _check(_lib().mtts_k_codec_softmax_mask(S.data_ptr(), _lens(lens).ctypes.data, B, heads, T, ldT, None))
    got = _u32(S).view(F32).reshape(S_h.shape)
    assert (_u32(guard) == cr.SENT32).all()
    ref = cr.softmax_mask_ref(S_h, lens, T)
    assert (got.view(np.uint32)[..., T:] == 0).all(), "pad columns are not +0"
    assert np.abs(got.astype(F64).sum(-1) - 1.0).max() <= 1e-6
    _ratio("softmax_rowsum", np.abs(got.astype(F64).sum(-1) - 1.0), 1e-6)
    for b, n in enumerate(lens):
        assert (got.view(np.uint32)[b, :, :n, n:] == 0).all(), ("a masked key has weight", b)
        pad = got[b, :, n:, :T]
        one_ulp = np.spacing(F32(1.0 / T))
        assert (np.abs(pad.astype(F64) - 1.0 / T) <= one_ulp).all(), ("padded row is not 1/T", b)
        if n == 1:
            assert (got[b, :, 0, 0] == 1.0).all()
    _check_close("softmax", got, ref, 1e-5, 1e-12, ("softmax_mask", B, heads, T, lens))


# ---- one RVQ stage -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,D", cr.VQ_CASES)
def test_codec_vq_argmin_update(K, D):
    """Inputs exact in fp32 (test_codec_ref_cpu.py): the codes equal the fp64 argmin on every row, first index on the planted
    ties, the residual update is exact and masked rows keep their residual."""
    d = cr.vq_inputs(K, D)
    rows = cr.VQ_B * cr.VQ_T
    codes_ref, res_ref = cr.vq_ref(d["dot"], d["cb"], d["cc"], d["r"], cr.VQ_LENS, cr.VQ_T)
    dot, cb, cc, r = (_dev(d[k]) for k in ("dot", "cb", "cc", "r"))
    codes = torch.full((rows + 2,), -7, dtype=torch.int64, device="cuda")
    _check(_lib().mtts_k_codec_vq_argmin_update(dot.data_ptr(), cb.data_ptr(), cc.data_ptr(), r.data_ptr(), codes.data_ptr(),
                                                _lens(cr.VQ_LENS).ctypes.data, cr.VQ_B, cr.VQ_T, K, D, None))
    torch.cuda.synchronize()
    got = codes.cpu().numpy()
    assert (got[rows:] == -7).all()
    assert np.array_equal(got[:rows], codes_ref), np.argwhere(got[:rows] != codes_ref)[:5].tolist()
    _assert_bits(r.cpu().numpy().view(np.uint32), res_ref.astype(F32).view(np.uint32), ("vq residual", K, D))


# ---- the exact-f32 GEMM in its general form ------------------------------------------------------------------------------
def _gemm_ex(a, w, c, bias, gamma, res, M, N, K, b_kn, lda, ldw, ldc, ldres=0, res_rows=0, act=0, scale=1.0, batch=1, inner=1,
             strides=(0,) * 6, offs=(0, 0, 0)):
    st = (C.c_int64 * 6)(*strides)
    _check(_lib().mtts_k_codec_gemm_f32_ex(_ptr(a, offs[0]), _ptr(w, offs[1]), _ptr(c, offs[2]), _ptr(bias), _ptr(gamma), _ptr(res), M, N, K,
                                           b_kn, lda, ldw, ldc, ldres, res_rows, act, C.c_float(scale), batch, inner, st, None))


@pytest.mark.parametrize("name,M,N,K,b_kn", cr.GEMM_EX_CASES)
def test_codec_gemm_f32_general(name, M, N, K, b_kn):
    """[K][N] and [N][K] weights with N and K tails, leading dimensions longer than the rows; then scale, GELU, gamma and a
    residual indexed m % res_rows on the same shape."""
    rng = np.random.default_rng(len(name) + M + N + K)
    ldn = (N + 3) // 4 * 4 + 4
    lda, ldc = K + 4, N + 3
    a_h = rng.standard_normal((M, lda)).astype(F32)
    w_nk = (rng.standard_normal((N, K)) / np.sqrt(K)).astype(F32)
    if b_kn:
        w_h = np.full((K, ldn), 1e30, F32)
        w_h[:, :N] = w_nk.T
        ldw = ldn
    else:
        w_h = np.full((N, K + 8), 1e30, F32)
        w_h[:, :K] = w_nk
        ldw = K + 8
    a_h[:, K:] = 1e30                     # past the row's K elements: must not be read into the product
    bias_h, gamma_h = rng.standard_normal(N).astype(F32), rng.standard_normal(N).astype(F32)
    RR = 8
    res_h = rng.standard_normal((RR, N + 1)).astype(F32)
    a, w, bias, gamma, res = (_dev(x) for x in (a_h, w_h, bias_h, gamma_h, res_h))
    mask = np.zeros((M + 1, ldc), bool)
    mask[:M, :N] = True
    for full in (False, True):
        c = _sent32((M + 1) * ldc)
        if full:
            _gemm_ex(a, w, c, bias, gamma, res, M, N, K, b_kn, lda, ldw, ldc, ldres=N + 1, res_rows=RR, act=1, scale=0.5)
            ref = cr.gemm_ref(a_h[:, :K], w_nk, bias_h, 1, gamma_h, res_h[np.arange(M) % RR, :N], scale=0.5)[0]
        else:
            _gemm_ex(a, w, c, bias, None, None, M, N, K, b_kn, lda, ldw, ldc)
            ref = cr.gemm_ref(a_h[:, :K], w_nk, bias_h)[0]
        u = _u32(c).reshape(M + 1, ldc)
        _written(u, mask, cr.SENT32, ("gemm_f32_ex", name, full))
        _check_close("gemm_f32_ex", u.view(F32)[:M, :N], ref, cr.F32_RTOL, cr.F32_ATOL, ("gemm_f32_ex", name, full))


def test_codec_gemm_f32_batched_as_attention():
    """The attention's two batched products with its stride pattern (batch_inner = heads): S = Q K^T * scale into rows of
    ldT > T, and P V reading such rows ([K][N] weights, K = T not a multiple of 4)."""
    B, heads, T = 3, 2, 33
    d, ldT = 64 * heads, cr.ld16(T)
    qkv_h = cr.attn_inputs(B, heads, T, 0)
    qkv = _dev(qkv_h)
    S = _sent32(B * heads * T * ldT)
    _gemm_ex(qkv, qkv, S, None, None, None, T, T, 64, 0, 3 * d, 3 * d, ldT, scale=0.125, batch=B * heads, inner=heads,
             strides=(T * 3 * d, 64, T * 3 * d, 64, heads * T * ldT, T * ldT), offs=(0, d, 0))
    u = _u32(S).reshape(B, heads, T, ldT)
    mask = np.zeros(u.shape, bool)
    mask[..., :T] = True
    _written(u, mask, cr.SENT32, "batched S")
    q = qkv_h[..., :d].astype(F64).reshape(B, T, heads, 64)
    k = qkv_h[..., d:2 * d].astype(F64).reshape(B, T, heads, 64)
    v = qkv_h[..., 2 * d:].astype(F64).reshape(B, T, heads, 64)
    _check_close("gemm_f32_ex", u.view(F32)[..., :T], np.einsum("bthd,buhd->bhtu", q, k) * 0.125, cr.F32_RTOL, cr.F32_ATOL, "batched S")
    rng = np.random.default_rng(9)
    P_h = np.full((B, heads, T, ldT), 1e30, F32)              # the pad columns must not be read
    P_h[..., :T] = rng.random((B, heads, T, T)) / T
    P = _dev(P_h)
    att = _sent32(B * T * d)
    _gemm_ex(P, qkv, att, None, None, None, T, 64, T, 1, ldT, 3 * d, d, batch=B * heads, inner=heads,
             strides=(heads * T * ldT, T * ldT, T * 3 * d, 64, T * d, 64), offs=(0, 2 * d, 0))
    got = _u32(att)
    assert (got != cr.SENT32).all()
    ref = np.einsum("bhtu,buhd->bthd", P_h[..., :T].astype(F64), v).reshape(B, T, d)
    _check_close("gemm_f32_ex", got.view(F32).reshape(B, T, d), ref, cr.F32_RTOL, cr.F32_ATOL, "batched P V")


@pytest.mark.parametrize("tm,tn", cr.GEMM_EX_GRIDS)
def test_codec_gemm_f32_xcd_map_covers_every_tile(tm, tn):
    """Grids of 3 x 5, 9 x 1 and 1 x 9 tiles through the XCD-aware block -> tile map: every element is written (the map is a
    bijection, so exactly once) and right."""
    M, N, K = 128 * tm - 5, 128 * tn - 3, 8
    rng = np.random.default_rng(tm * 10 + tn)
    a_h, w_h = rng.standard_normal((M, K)).astype(F32), rng.standard_normal((N, K)).astype(F32)
    c = _sent32(M * N + 64)
    _gemm_ex(_dev(a_h), _dev(w_h), c, None, None, None, M, N, K, 0, K, K, N)
    u = _u32(c)
    mask = np.arange(M * N + 64) < M * N
    _written(u, mask, cr.SENT32, ("xcd grid", tm, tn))
    _check_close("gemm_f32_ex", u[:M * N].view(F32).reshape(M, N), a_h.astype(F64) @ w_h.astype(F64).T, cr.F32_RTOL, cr.F32_ATOL, ("xcd grid", tm, tn))
