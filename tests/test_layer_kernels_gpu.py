"""The layer kernels the engine launches, one launch each, against tests/layer_ref.py.  -m gpu.

embed_norm_kernel and resid_norm_kernel (every layer of every pass), gemv_small_kernel with each prologue / epilogue pair
of the small-batch decode step, and gemm_tile_kernel on prefill passes of fewer than four row tiles and with its SwiGLU
epilogue, through mtts_k_embed_norm / mtts_k_resid_norm / mtts_k_gemv_small / mtts_k_gemm_tile.  Residual streams, chunk
sums and everything behind an identity weight are compared bit for bit; an RMSNorm row must be reproduced whole by one
fp32 inv inside the window layer_ref derives; GEMM outputs keep the project's bound for this MFMA path.  Outputs start as
a sentinel pattern and every element a kernel must not write has to keep it; slots a kernel may load but must not add
are NaN.  test_layer_ref_cpu.py checks the expectations and the inputs on the CPU.
"""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import layer_ref as lr  # noqa: E402
from mtts import capi  # noqa: E402

F32 = np.float32
EPI_PARTIAL, EPI_BF16, EPI_SILU, EPI_SILU_RM = 0, 1, 2, 3
PRO_NORM, PRO_COMBINE, PRO_ROWS = 1, 2, 3
SMALL_RP = 4
EPS = C.c_float(lr.EPS)


def _dev_bits(b):
    return torch.from_numpy(np.ascontiguousarray(b, dtype=np.uint16).view(np.int16)).cuda()


def _dev_bf16(a):
    return _dev_bits(lr.bits(a))


def _dev_f32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=F32)).cuda()


def _poisoned(*shape):
    return _dev_bits(np.full(shape, lr.SENTINEL, dtype=np.uint16))


def _host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy().view(np.uint16)


def _canon(b):
    """-0 -> +0: an MFMA accumulator that starts at +0 cannot return -0 through an identity weight."""
    return np.where((b & 0x7FFF) == 0, np.uint16(0), b)


def _assert_untouched(b, what):
    assert (b == lr.SENTINEL).all(), (what, "written where nothing may be written", np.argwhere(b != lr.SENTINEL)[:5])


def _assert_bits(got, want, what):
    bad = np.argwhere(got != want)
    assert bad.size == 0, (what, "first differing (row, column)", bad[:5].tolist(), len(bad))


# ---- embed_norm_kernel ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,R", lr.EMBED_CASES)
def test_embed_norm_kernel(H, R):
    """x = the eight bf16-rounded adds in channel order, every bit (idle rows zero); xn = RMSNorm(x) * w by the candidate rule."""
    d = lr.embed_inputs(H, R)
    tabs = [_dev_bf16(t) for t in d["tables"]]
    ptrs = (C.c_void_p * 8)(*[t.data_ptr() for t in tabs])
    vocab = np.array(lr.VOCAB, dtype=np.int32)
    w = _dev_bf16(d["w"])
    x, xn = _poisoned(R, H), _poisoned(R, H)
    capi.check(capi.lib().mtts_k_embed_norm(d["tokens"].ctypes.data, d["seq"].ctypes.data, ptrs, vocab.ctypes.data, w.data_ptr(),
                                            R, H, EPS, x.data_ptr(), xn.data_ptr(), None))
    want = lr.embed_sum(d["tables"], d["tokens"], d["seq"])
    _assert_bits(_host(x), lr.bits(want), ("embed_sum", H, R))
    got_xn = _host(xn)
    idle = d["seq"] < 0
    assert not lr.from_bits(got_xn[idle]).any() and not lr.from_bits(_host(x)[idle]).any()
    lr.assert_rmsnorm_rows(got_xn, want, d["w"], what=("embed_norm xn", H, R))


# ---- resid_norm_kernel ---------------------------------------------------------------------------------------------------
def _resid_norm(d, slabs=None):
    """mtts_k_resid_norm on a layer_ref.resid_inputs case -> bits of x', xn, hlast."""
    slabs = d["slabs"] if slabs is None else slabs
    R, H = d["R"], d["H"]
    x, w = _dev_bf16(d["x"]), _dev_bf16(d["w"])
    xn, hlast = _poisoned(R, H), _poisoned(d["nseq"], H)
    sl = _dev_f32(slabs)
    capi.check(capi.lib().mtts_k_resid_norm(sl.data_ptr(), slabs.shape[0], d["Npad"], x.data_ptr(), w.data_ptr(), d["seq"].ctypes.data,
                                            d["last"].ctypes.data, R, H, d["nseq"], EPS, xn.data_ptr(), hlast.data_ptr(), None))
    return _host(x), _host(xn), _host(hlast)


@pytest.mark.parametrize("H,ks,R", lr.RESID_CASES)
def test_resid_norm_kernel(H, ks, R):
    """x' = round(x + round(slabs summed k = 0, 1, 2, ...)), every bit; xn by the candidate rule; hlast[seq] = the xn row of
    the live `last` rows and nothing else."""
    d = lr.resid_inputs(H, ks, R)
    x1, xn, hlast = _resid_norm(d)
    want = lr.resid(d["slabs"], d["x"])
    _assert_bits(x1, lr.bits(want), ("resid x'", H, ks, R))
    lr.assert_rmsnorm_rows(xn, want, d["w"], what=("resid_norm xn", H, ks, R))
    written = np.zeros(d["nseq"], dtype=bool)
    for r in range(R):
        if d["seq"][r] >= 0 and d["last"][r]:
            _assert_bits(hlast[d["seq"][r]], xn[r], ("hlast of row", r))
            written[d["seq"][r]] = True
    assert written.any()
    _assert_untouched(hlast[~written], ("hlast", H, ks, R))


# ---- gemv_small_kernel ---------------------------------------------------------------------------------------------------
def _gemv_small(epi, pro, w, rows, N, K, want_ks, y, x_in=None, slabs=None, norm_w=None, x_out=None, opart=None, seq=None, pos=None,
                nq=0, nchunks_max=0, xrows=None, expect=0):
    keep = [_dev_bf16(t) if t is not None else None for t in (w, x_in, norm_w, xrows)]
    sl = _dev_f32(slabs) if slabs is not None else None
    op = _dev_f32(opart) if opart is not None else None
    ptr = lambda t: t.data_ptr() if t is not None else None
    plan = (C.c_int32 * 2)(0, 0)
    rc = capi.lib().mtts_k_gemv_small(epi, pro, ptr(keep[0]), rows, N, K, want_ks, ptr(keep[1]), ptr(sl), 0 if slabs is None else slabs.shape[0],
                                      ptr(keep[2]), EPS, ptr(x_out), ptr(op), seq.ctypes.data if seq is not None else None,
                                      pos.ctypes.data if pos is not None else None, nq, nchunks_max, ptr(keep[3]), y.data_ptr(), plan, None)
    if expect:
        assert rc == expect, rc
    else:
        capi.check(rc)
    torch.cuda.synchronize()
    return plan[0], plan[1]


@functools.lru_cache(maxsize=None)
def _identity(n):
    return np.eye(n, dtype=F32)


@pytest.mark.parametrize("H,ks", [(H, ks) for H in (256, 2048) for ks in (0, 1, 4, 5, 12)])
def test_gemv_small_norm_prologue_identity(H, ks):
    """Behind an identity weight (every product exact in fp32) the bf16 epilogue returns the prologue's xn: the same bits
    as resid_norm_kernel's xn on the same inputs, for every element, and x_out the same bits as its x'.  ks = 0 (first
    layer, no slabs): the plain RMSNorm of x_in, which is also resid_norm_kernel on one slab of zeros.  H = 256 plans 4
    waves per block, H = 2048 plans 8."""
    for rows in (1, 2, 3, 4):
        d = lr.resid_inputs(H, ks, rows)
        ref_slabs = d["slabs"] if ks else np.zeros((1, rows, d["Npad"]), dtype=F32)
        x1, xn, _ = _resid_norm(d, ref_slabs)
        y, x_out = _poisoned(SMALL_RP, H), _poisoned(SMALL_RP, H)
        waves, split = _gemv_small(EPI_BF16, PRO_NORM, _identity(H), rows, H, H, 1, y, x_in=d["x"], slabs=d["slabs"], norm_w=d["w"],
                                   x_out=x_out)
        assert (waves, split) == ((4, 1) if H == 256 else (8, 1))
        y, x_out = _host(y), _host(x_out)
        _assert_bits(x_out[:rows], x1, ("x_out against resid_norm's x'", H, ks, rows))
        _assert_bits(y[:rows], _canon(xn), ("xn against resid_norm's xn", H, ks, rows))
        _assert_untouched(y[lr.untouched_rows(rows)], ("y rows >= rows", H, ks, rows))
        _assert_untouched(x_out[lr.untouched_rows(rows)], ("x_out rows >= rows", H, ks, rows))
        want = lr.resid(d["slabs"], d["x"])
        _assert_bits(x_out[:rows], lr.bits(want), ("x_out", H, ks, rows))
        if ks == 0:
            res = lr.rmsnorm_match(xn, want, d["w"])         # the one inv of each row, then the -0 of the identity product
            for r in range(rows):
                assert isinstance(res[r], int), ("plain RMSNorm", H, rows, r, res[r])


@pytest.mark.parametrize("H", [256, 2048])
def test_gemv_small_norm_prologue_bf16_tail(H):
    """Random weight, bf16 epilogue, n_valid = 1025 of Npad = 1056 (the last tile's scalar tail store) against the float64
    product of resid_norm_kernel's (verified) xn; columns >= n_valid and rows >= rows keep the sentinel."""
    rows, N, ks = 3, 1025, 4
    d = lr.resid_inputs(H, ks, rows)
    _, xn, _ = _resid_norm(d)
    w, _ = lr.gemm_inputs(rows, N, H, 31)
    y = _poisoned(SMALL_RP, 1056)
    _gemv_small(EPI_BF16, PRO_NORM, w, rows, N, H, 1, y, x_in=d["x"], slabs=d["slabs"], norm_w=d["w"])
    y = _host(y)
    _assert_untouched(y[:, N:], "columns >= n_valid")
    _assert_untouched(y[lr.untouched_rows(rows)], "rows >= rows")
    ref = lr.from_bits(xn).astype(np.float64) @ w.T.astype(np.float64)
    lr.assert_gemm_close(lr.from_bits(y[:rows, :N]), ref, ("bf16 tail", H))


# SHARES.  Measured on an MI355X: share of SwiGLU outputs equal to layer_ref.swiglu (of the float64 product) bit for
# bit, kernel under test / general kernel (gemm_skinny_kernel through mtts_k_gemm_swiglu_bf16) on the same operands.
#   gemv_small_kernel, EPI_SILU_RM, 3 rows:   H 256, N 512: 1.0000 / 1.0000      H 2048, N 1024: 1.0000 / 1.0000
#   gemm_tile_kernel, EPI_SILU  (N, K) =      (256, 64)          (320, 528)         (2048, 2048)
#     M = 32                                  0.9998 / 0.9998    0.9998 / 0.9994    0.9997 / 0.9999
#     M = 64                                  0.9999 / 0.9999    0.9998 / 0.9996    0.9997 / 0.9999
#     M = 96                                  0.9999 / 0.9999    0.9999 / 0.9997    0.9997 / 0.9999
#     M = 160                                 1.0000 / 1.0000    0.9999 / 0.9998    0.9996 / 0.9998
# The tests pin each share to at least the general kernel's minus 0.5 percentage points and print both.
def _swiglu_general(w, x):
    """gemm_skinny_kernel's SwiGLU (mtts_k_gemm_swiglu_bf16: at most 128 rows a call) -> bf16 bits [M][N/2]."""
    M, (N, K) = x.shape[0], w.shape
    wt = _dev_bf16(w)
    out = []
    for a in range(0, M, 128):
        m = min(128, M - a)
        xt, y = _dev_bf16(x[a:a + m]), _poisoned(m, N // 2)
        capi.check(capi.lib().mtts_k_gemm_swiglu_bf16(wt.data_ptr(), xt.data_ptr(), y.data_ptr(), m, N, K, None))
        out.append(_host(y))
    return np.concatenate(out)


def _swiglu_shares(got_bits, w, x, what):
    """The bound of test_swiglu_epilogue_bitwise against layer_ref.swiglu of the float64 product, and the share of outputs
    that equal it bit for bit: at least the already tested general kernel's share on the same operands minus 0.5
    percentage points (expf differs by an ulp between summation orders)."""
    ref = lr.swiglu(x.astype(np.float64) @ w.T.astype(np.float64))
    lr.assert_swiglu_close(lr.from_bits(got_bits), ref, what)
    share = float((got_bits == lr.bits(ref)).mean())
    general = float((_swiglu_general(w, x) == lr.bits(ref)).mean())
    print("swiglu exact share %s: kernel under test %.4f, general kernel %.4f" % (what, share, general))
    assert share >= general - 0.005, (what, share, general)
    return share, general


@pytest.mark.parametrize("H,N,ks", [(256, 512, 1), (2048, 1024, 4)])
def test_gemv_small_swiglu_row_major(H, N, ks):
    """EPI_SILU_RM behind the norm prologue: [rows][N/2] row-major, row `rows` untouched.  Measured shares of outputs equal
    to layer_ref.swiglu bit for bit (small kernel / general kernel on the same xn and weights): see SHARES below."""
    rows = 3
    d = lr.resid_inputs(H, ks, rows)
    _, xn, _ = _resid_norm(d)
    w, _ = lr.gemm_inputs(rows, N, H, 32)
    y = _poisoned(SMALL_RP, N // 2)
    _gemv_small(EPI_SILU_RM, PRO_NORM, w, rows, N, H, 1, y, x_in=d["x"], slabs=d["slabs"], norm_w=d["w"])
    y = _host(y)
    _assert_untouched(y[lr.untouched_rows(rows)], "rows >= rows")
    _swiglu_shares(y[:rows], w, lr.from_bits(xn), ("gemv_small", H, N))


def test_gemv_small_refuses_what_it_does_not_take():
    """H = 4096 needs 32 KiB of LDS for the norm prologue, above the small path's budget; a pair the decode step does not
    use; a split-K under the bf16 epilogue.  Each is MTTS_EINVAL and nothing is launched."""
    d = lr.resid_inputs(256, 0, 1)
    big = np.zeros((1, 4096), dtype=F32)
    y = _poisoned(SMALL_RP, 32)
    _gemv_small(EPI_BF16, PRO_NORM, np.zeros((32, 4096), dtype=F32), 1, 32, 4096, 1, y, x_in=big, norm_w=big[0], expect=capi.EINVAL)
    assert b"LDS" in capi.lib().mtts_last_error()
    _gemv_small(EPI_BF16, PRO_ROWS, _identity(256), 1, 256, 256, 1, y, xrows=d["x"], expect=capi.EINVAL)
    _gemv_small(EPI_BF16, PRO_NORM, _identity(256), 1, 256, 256, 2, y, x_in=d["x"], norm_w=d["w"], expect=capi.EINVAL)
    _gemv_small(EPI_PARTIAL, PRO_ROWS, _identity(256), 5, 256, 256, 0, y, xrows=d["x"], expect=capi.EINVAL)
    _assert_untouched(_host(y), "refused calls")


@pytest.mark.parametrize("nq", [2, 4])
@pytest.mark.parametrize("which", [0, 1])
def test_gemv_small_combine_prologue(nq, which):
    """Identity weight, fp32 slabs with the planned split-K: the output is bf16(fp32 sum of the row's first nch chunk
    partials, ascending), every bit; chunks >= nch are NaN and must not be added; an idle row gives exact zeros."""
    d = lr.combine_inputs(nq, which)
    K = nq * 128
    want = lr.bits(lr.combine(d["opart"], d["nch"]))
    for rows in (4, 3):
        y = _poisoned(SMALL_RP, K)
        _gemv_small(EPI_PARTIAL, PRO_COMBINE, _identity(K), rows, K, K, 0, y, opart=d["opart"][:rows], seq=d["seq"][:rows], pos=d["pos"][:rows],
                    nq=nq, nchunks_max=lr.NCHUNKS_MAX)
        y = _host(y)
        _assert_bits(y[:rows], _canon(want[:rows]), ("combine", nq, which, rows))
        _assert_untouched(y[lr.untouched_rows(rows)], "rows >= rows")
        for r in range(rows):
            if d["nch"][r] == 0:
                assert not y[r].any()


@pytest.mark.parametrize("K,N,want_ks", [(256, 96, 0), (256, 2048, 0), (6144, 96, 0), (6144, 2048, 0), (6144, 96, 5)])
def test_gemv_small_rows_prologue(K, N, want_ks):
    """Row-major activations in front of an fp32-slab GEMM, planned split-K (and 5: waves with a short last range),
    against the float64 product."""
    for rows in (1, 4):
        w, x = lr.gemm_inputs(rows, N, K, 33)
        y = _poisoned(SMALL_RP, N)
        waves, split = _gemv_small(EPI_PARTIAL, PRO_ROWS, w, rows, N, K, want_ks, y, xrows=x)
        assert split > 1 or K == 256
        y = _host(y)
        _assert_untouched(y[lr.untouched_rows(rows)], "rows >= rows")
        lr.assert_gemm_close(lr.from_bits(y[:rows]), x.astype(np.float64) @ w.T.astype(np.float64), ("rows prologue", K, N, rows, waves, split))


# ---- gemm_tile_kernel ----------------------------------------------------------------------------------------------------
TILE_SHAPES = [(256, 64), (320, 528), (2048, 2048)]


@functools.lru_cache(maxsize=None)
def _tile_operands(N, K):
    w, x = lr.gemm_inputs(160, N, K, 34)
    return w, x, x.astype(np.float64) @ w.T.astype(np.float64)


def _gemm_tile(epi, w, x, ksplit):
    M, (N, K) = x.shape[0], w.shape
    wt, xt = _dev_bf16(w), _dev_bf16(x)
    y = _poisoned(M, N if epi == EPI_PARTIAL else N // 2)
    capi.check(capi.lib().mtts_k_gemm_tile(epi, wt.data_ptr(), xt.data_ptr(), y.data_ptr(), M, N, K, ksplit, None))
    return _host(y)


@pytest.mark.parametrize("N,K", TILE_SHAPES)
@pytest.mark.parametrize("M", [32, 64, 96, 160])
def test_gemm_tile_partial_small_passes(M, N, K):
    """The prefill GEMM on passes of 1, 2, 3 and 5 row tiles (N = 320: a partial last column block), split-K 1 and 2."""
    w, x, ref = _tile_operands(N, K)
    for ks in (1, 2):
        y = _gemm_tile(EPI_PARTIAL, w, x[:M], ks)
        lr.assert_gemm_close(lr.from_bits(y), ref[:M], ("gemm_tile", M, N, K, ks))


@pytest.mark.parametrize("N,K", TILE_SHAPES)
@pytest.mark.parametrize("M", [32, 64, 96, 160])
def test_gemm_tile_swiglu(M, N, K):
    """The prefill SwiGLU (EPI_SILU on the tile kernel) against layer_ref.swiglu; measured exact shares: see SHARES below."""
    w, x, _ = _tile_operands(N, K)
    y = _gemm_tile(EPI_SILU, w, x[:M], 1)
    _swiglu_shares(y, w, x[:M], ("gemm_tile", M, N, K))
