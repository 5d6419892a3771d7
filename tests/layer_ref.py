"""Host-side expectations for the layer-kernel tests (test_layer_ref_cpu.py, test_layer_kernels_gpu.py).  numpy only.

The kernels under test (csrc/layer.hip: embed_norm_kernel, resid_norm_kernel; csrc/gemm.hip: gemv_small_kernel's
prologues and its row-major SwiGLU, gemm_tile_kernel's SwiGLU) round to bf16 at the points the reference's CPU bf16
execution does (oracle/asteroid_oracle.py lists them).  Every function here reproduces those points with
oracle.asteroid_oracle.round_bf16; fp32 operations whose ORDER is part of the contract (the eight embedding adds, the
split-K slab sum, the chunk sum) are done in that order in fp32; every long reduction whose order is NOT part of the
contract (the mean of squares, a GEMM's dot products) is done in float64.

How an RMSNorm row is compared
------------------------------
xn[i] = rbf(w[i] * rbf(x[i] * inv)), inv = 1 / sqrt(mean(x^2) + eps), one fp32 number per row.  Only the fp32 VALUE of
inv depends on how the kernel sums the squares, so the check is: some fp32 number within a window of W ulps around the
float64 inv reproduces the whole row bit for bit.  A wrong rounding point, a wrong H in the mean, a missing eps or a
wrong weight element breaks that for every candidate; the shape of the reduction tree does not.

The window.  u = 2^-24 is the unit roundoff of fp32; one ulp of an fp32 number is between u and 2u of its value.
  * a thread sums n_t = 8 * ceil(H / 2048) squares one after another: n_t roundings of the running sum and one of each
    product (none when the compiler contracts to an FMA);
  * the 256 lanes are summed as a tree: 6 butterfly levels inside a wave, then 3 adds over the 4 waves;
  every term is >= 0, so the relative error of the total is at most (n_t + 1 + 6 + 3) u to first order;
  * tot / H and (...) + eps: one rounding each, +2u (eps > 0 only shrinks the relative error of the first);
  * the square root halves the relative error of its argument and adds at most one ulp (2u) of its own, as does the
    reciprocal.
  relative error of inv <= ((n_t + 12) / 2 + 4) u, that is at most that many ulps of inv; one more ulp because the
  window is centred on the float64 value rounded to fp32, and one for the second-order terms:
      W = ceil((n_t + 12) / 2) + 6          (16 ulps at H <= 2048, 28 at H = 8192).
test_layer_ref_cpu.py checks, for every row of every input the GPU tests use, that the oracle's own fp32 rmsnorm (numpy's
pairwise sum: a different tree again) is reproduced by a candidate inside this window.
"""
import math

import numpy as np

from oracle import asteroid_oracle as ao

F32 = np.float32
rbf = ao.round_bf16
EPS = 1e-6
SENTINEL = 0xABCD                      # bf16 bit pattern that outputs are prefilled with (-1.22e-12: no input produces it)


def bits(a):
    """fp32 array holding bf16 values -> their uint16 bit patterns."""
    a = np.ascontiguousarray(a, dtype=F32)
    return (a.view(np.uint32) >> 16).astype(np.uint16)


def from_bits(b):
    return (np.ascontiguousarray(b, dtype=np.uint16).astype(np.uint32) << 16).view(F32)


def round_up(a, b):
    return (a + b - 1) // b * b


# ---- the operations ------------------------------------------------------------------------------------------------------
def embed_sum(tables, tokens, seq, order=range(8)):
    """tables: 8 fp32 arrays [V_c][H] of bf16 values; tokens int [R][8]; seq int [R] (< 0: idle row -> zeros).
    Eight sequential bf16-rounded adds in channel order (`order`: the CPU test sums in another one to show that it matters)."""
    tokens = np.asarray(tokens)
    act = np.asarray(seq) >= 0
    acc = np.zeros((tokens.shape[0], tables[0].shape[1]), dtype=F32)
    for c in order:
        acc = rbf(acc + tables[c][np.where(act, tokens[:, c], 0)])
    acc[~act] = 0
    return acc


def slab_sum(slabs, H, order=None):
    """fp32 sum of the split-K slabs [ksplit][R][Npad] over k = 0, 1, 2, ... (columns < H)."""
    order = range(slabs.shape[0]) if order is None else order
    s = None
    for k in order:
        s = slabs[k][:, :H].astype(F32) if s is None else (s + slabs[k][:, :H]).astype(F32)
    return s


def resid(slabs, x, order=None):
    """x' = round(x + round(sum of the slabs)); slabs None: x' = x (first layer: x is the embedding sum)."""
    x = np.asarray(x, dtype=F32)
    if slabs is None or slabs.shape[0] == 0:
        return x.copy()
    return rbf(x + rbf(slab_sum(slabs, x.shape[1], order)))


def norm_window(H):
    n_t = 8 * math.ceil(H / 2048)
    return math.ceil((n_t + 12) / 2) + 6


def rmsnorm_with_inv(x, w, inv):
    """One row (or rows, inv broadcast) with a given fp32 inv: the two rounding points of Qwen3RMSNorm in bf16."""
    return rbf(np.asarray(w, dtype=F32) * rbf(np.asarray(x, dtype=F32) * F32(inv)))


def rmsnorm_candidates(xrow, eps=EPS):
    """The fp32 values inside the window around the float64 inv of one row, nearest first."""
    x64 = np.asarray(xrow, dtype=np.float64)
    H = x64.shape[-1]
    inv = F32(1.0 / math.sqrt(float(np.mean(x64 * x64)) + eps))
    centre = int(np.array(inv, dtype=F32).view(np.uint32))
    W = norm_window(H)
    offs = [0] + [s * d for d in range(1, W + 1) for s in (1, -1)]
    return [np.array(centre + o, dtype=np.uint32).view(F32)[()] for o in offs], offs


def rmsnorm_match(got_bits, x, w, eps=EPS):
    """got_bits uint16 [R][H] against rows x fp32 [R][H]: per row, the window offset (in ulps of inv) of the ONE candidate
    that reproduces the whole row, or a description of the best candidate's first mismatch."""
    out = []
    for r in range(x.shape[0]):
        cands, offs = rmsnorm_candidates(x[r], eps)
        best = None
        for inv, o in zip(cands, offs):
            bad = np.nonzero(bits(rmsnorm_with_inv(x[r], w, inv)) != got_bits[r])[0]
            if bad.size == 0:
                best = o
                break
            if best is None or bad.size < best[0]:
                best = (bad.size, int(bad[0]), o)
        out.append(best)
    return out


def assert_rmsnorm_rows(got_bits, x, w, eps=EPS, what=""):
    res = rmsnorm_match(got_bits, x, w, eps)
    bad = [(r, v) for r, v in enumerate(res) if not isinstance(v, int)]
    assert not bad, f"{what}: no inv within {norm_window(x.shape[1])} ulps reproduces row(s) (row, (mismatches, first column, offset)): {bad[:5]}"
    return res


def combine(opart, nch):
    """opart fp32 [rows][nq][nchunks_max][128], nch int [rows] -> bf16 of the fp32 sum of each row's first nch chunk
    partials in ascending order, [rows][nq*128]."""
    rows, nq = opart.shape[:2]
    out = np.zeros((rows, nq, opart.shape[3]), dtype=F32)
    for r in range(rows):
        for c in range(int(nch[r])):
            out[r] = (out[r] + opart[r, :, c]).astype(F32)
    return rbf(out).reshape(rows, -1)


def swiglu(z):
    """z [M][N]: the gate/up Linear before its bf16 rounding, gate and up columns interleaved (2i = gate i, 2i + 1 = up i).
    The rounding points of AsteroidOracle.forward_hidden: gate, up -> bf16; silu(gate) -> bf16; product -> bf16."""
    z = rbf(np.asarray(z, dtype=F32))
    g, u = z[:, 0::2], z[:, 1::2]
    with np.errstate(over="ignore", invalid="ignore"):
        a = rbf(g / (F32(1) + np.exp(-g, dtype=F32)))
        return rbf(a * u)


def untouched_rows(rows):
    """Rows of a SMALL_RP-row output buffer that a launch on `rows` rows must leave as they were."""
    return slice(rows, None)


def nch_of(seq, pos, pages_per_chunk=8):
    """Chunks a decode row sums: ceil(pages / pages_per_chunk) with pages = ceil((pos + 1) / 64); 0 for an idle row."""
    pages = np.where(np.asarray(seq) >= 0, np.asarray(pos) // 64 + 1, 0)
    return (pages + pages_per_chunk - 1) // pages_per_chunk


# ---- the seeded inputs both test files use -----------------------------------------------------------------------------------
H_SET = (256, 2048, 2064, 8192)
EMBED_CASES = [(H, R) for H in H_SET for R in (1, 5, 33)]
_KS, _RS = (1, 2, 8, 9, 12), (1, 5, 32, 130)
RESID_CASES = [(H, ks, _RS[(hi + ki) % 4]) for hi, H in enumerate(H_SET) for ki, ks in enumerate(_KS)]
SMALL_NORM_CASES = [(H, ks, rows) for H in (256, 2048) for ks in (0, 1, 4, 5, 12) for rows in (1, 2, 3, 4)]
VOCAB = (37, 11, 37, 11, 11, 37, 11, 11)
COMBINE_ROWS = [dict(seq=[-1, 0, 2, 1], pos=[700, 100, 64 * 60, 64 * 64]),          # nch 0 (idle), 1, 8, 9
                dict(seq=[3, 1, -1, 0], pos=[64 * 130, 64 * 64 + 5, 0, 511])]       # nch 17, 9, 0 (idle), 1
NCHUNKS_MAX = 17


def norm_weight(H, seed):
    rng = np.random.default_rng(seed)
    w = 1 + 0.1 * rng.standard_normal(H)
    w[3] = 0.0
    w[4::61] *= -1                                 # negative weights: the sign of a zero product is part of the bits
    return rbf(w.astype(F32))


def embed_inputs(H, R, seed=11):
    """Tables of two vocabulary sizes, tokens with 0 and V_c - 1, idle rows, exact zeros, a whole zero row (all tokens 0),
    a row of large magnitude, and a cancellation that makes the order of the eight adds observable: the last token of
    channels 0 / 1 / 2 holds big / small / -big, so channel order gives (big + small) - big = 0 where small is below half
    an ulp of big, and any order that meets -big before small keeps small."""
    rng = np.random.default_rng(seed * 1000 + H + R)
    tables = [rbf((0.5 * rng.standard_normal((V, H))).astype(F32)) for V in VOCAB]
    for t in tables:
        t[0] = 0                                   # token 0 of every channel: a whole zero row
    tables[3][:, ::7] = 0
    big = rbf((256 * (1 + rng.random(H))).astype(F32))
    tables[0][-1], tables[2][-1] = big, -big
    tables[1][-1] = rbf((0.25 + 0.5 * rng.random(H)).astype(F32))
    tables[4][1] = rbf((2.0 ** 20 * rng.standard_normal(H)).astype(F32))
    tokens = np.stack([rng.integers(0, V, R) for V in VOCAB], axis=1).astype(np.int32)
    seq = np.arange(R, dtype=np.int32)
    tokens[0] = [V - 1 for V in VOCAB]             # the cancellation row
    if R > 1:
        tokens[1] = 0                              # whole zero row
        tokens[2, 4] = 1                           # row of large magnitude
        idle = np.arange(R) % 4 == 3
        seq[idle] = -1
        tokens[idle] = -7                          # an idle row's tokens are never used
    return dict(tables=tables, tokens=tokens, seq=seq, w=norm_weight(H, seed), H=H, R=R)


def resid_inputs(H, ksplit, R, seed=12):
    """Slabs fp32 [ksplit][R][Npad] (NaN in the padding columns, which no row may read), x bf16 [R][H], seq = a permutation
    shifted by 2 (never the row index), idle rows, a few `last` rows (one of them idle: it must not reach hlast), exact
    zeros, a whole zero row, a row of large magnitude, and in row 0 a cancellation that makes the slab order observable:
    slab 0 = big, slab 1 = small, last slab = -big with small below half an ulp of big."""
    rng = np.random.default_rng(seed * 1000 + H + 7 * ksplit + R)
    Npad = round_up(H, 32)
    x = rbf(rng.standard_normal((R, H)).astype(F32))
    slabs = (0.3 * rng.standard_normal((ksplit, R, Npad))).astype(F32) if ksplit else None
    if ksplit:
        slabs[:, :, H:] = np.nan
    if ksplit >= 3:
        big = (2.0 ** 24 * (1 + rng.random(H))).astype(F32)
        slabs[0, 0, :H], slabs[ksplit - 1, 0, :H] = big, -big
        slabs[1, 0, :H] = (0.5 + rng.random(H)).astype(F32)
    if R > 1:
        x[1] = 0
        if ksplit:
            slabs[:, 1] = 0
            slabs[:, 1, H:] = np.nan
    if R > 2:
        x[2] = rbf(x[2] * F32(2.0 ** 18))
        if ksplit:
            slabs[:, 2, :H] *= F32(2.0 ** 18)
    x[:, 5] = 0
    if ksplit:
        slabs[:, :, 5] = 0
    nseq = R + 3
    seq = ((np.arange(R) * 7 + 3) % R + 2).astype(np.int32)
    last = np.zeros(R, dtype=np.int32)
    last[[0, R // 2, R - 1]] = 1
    if R >= 5:
        seq[np.arange(R) % 5 == 4] = -1
        last[4] = 1                                # idle and `last`: nothing may be written for it
    return dict(slabs=slabs, x=x, w=norm_weight(H, seed + 1), seq=seq, last=last, nseq=nseq, H=H, Npad=Npad, R=R, ksplit=ksplit)


def swapped(n):
    """The slab / chunk / channel order with elements 1 and n - 1 exchanged (an order that meets -big before small)."""
    o = list(range(n))
    o[1], o[n - 1] = o[n - 1], o[1]
    return o


def combine_inputs(nq, which, seed=13):
    """opart fp32 [4][nq][17][128]: every chunk a row must not add is NaN (an idle row: all of them); exact zeros; and
    in the rows with >= 3 chunks the big / small / -big cancellation over chunks 0, 1 and nch - 1."""
    rng = np.random.default_rng(seed * 1000 + nq + which)
    seq, pos = (np.array(COMBINE_ROWS[which][k], dtype=np.int32) for k in ("seq", "pos"))
    nch = nch_of(seq, pos)
    opart = rng.standard_normal((4, nq, NCHUNKS_MAX, 128)).astype(F32)
    opart[..., 9] = 0
    for r in range(4):
        if nch[r] >= 3:
            big = (2.0 ** 24 * (1 + rng.random((nq, 64)))).astype(F32)
            opart[r, :, 0, :64], opart[r, :, nch[r] - 1, :64] = big, -big
            opart[r, :, 1, :64] = (0.5 + rng.random((nq, 64))).astype(F32)
        opart[r, :, nch[r]:] = np.nan
    return dict(opart=opart, seq=seq, pos=pos, nch=nch, nq=nq)


def gemm_inputs(M, N, K, seed):
    """Weights and activations of test_gemm_kernel_matches_fp32_reference's kind, with exact zeros and a zero row."""
    rng = np.random.default_rng(seed * 100003 + M * 31 + N * 7 + K)
    w = rbf((0.05 * rng.standard_normal((N, K))).astype(F32))
    x = rbf(rng.standard_normal((M, K)).astype(F32))
    x[:, 3] = 0
    if M > 1:
        x[1] = 0
    return w, x


def assert_gemm_close(got, ref64, what=""):
    """The project's bound for a bf16 output of this MFMA path (test_gemm_kernel_matches_fp32_reference)."""
    np.testing.assert_allclose(got, ref64, rtol=2 ** -8, atol=2e-3 * np.abs(ref64).max(), err_msg=str(what))
    exact = (got == rbf(ref64.astype(F32))).mean()
    assert exact > 0.98, (what, exact)


def assert_swiglu_close(got, ref, what=""):
    """The bound of test_swiglu_epilogue_bitwise, as an upper bound."""
    fin = np.isfinite(ref) & np.isfinite(got)
    assert fin.mean() > 0.99, what
    rowmax = np.abs(np.where(fin, ref, 0)).max(axis=1, keepdims=True)
    tol = 2.0 ** -5 * np.abs(ref) + 2e-2 * rowmax
    with np.errstate(invalid="ignore"):
        ok = (np.abs(got - ref) <= tol) | ~fin
    assert ok.all(), (what, np.argwhere(~ok)[:5])
