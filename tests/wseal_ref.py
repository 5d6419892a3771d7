"""numpy side of the sealed weight streams (csrc/gemm_sealed.hip), shared by tests/test_wseal_cpu.py and
tests/test_wseal_gpu.py: the packed weight layout cut into groups, the 12-tile group's specification stated with
oracle/kv_seal_oracle.py alone, and the weights the tests use."""
import numpy as np

from oracle import kv_seal_oracle as ks

KEEP12 = [0, 1, 2, 3, 4, 5, 8, 9, 10, 12]          # units of the 16-unit form a 12-tile group keeps, in stored order


def bf16_bits(x):
    """fp32 -> bf16 bit patterns, round to nearest even (finite inputs)."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def groups_of(w_bits, ktw):
    """Row-major weight bits uint16 [N][K] (N % 32 == 0, K % (16 ktw) == 0) -> uint16 [N/32][K/16/ktw][64 lanes][8 ktw
    values]: the lanes of every group of ktw k-tiles of the packed array (common.h: wpack_off -- lane = n % 32 + 32 *
    ((k % 16) / 8), a lane's values in k order)."""
    N, K = w_bits.shape
    t = w_bits.reshape(N // 32, 32, K // (16 * ktw), ktw, 2, 8)        # [nt][row][c][tile][half][8]
    return np.ascontiguousarray(t.transpose(0, 2, 4, 1, 3, 5)).reshape(N // 32, K // (16 * ktw), 64, ktw * 8)


def packed_of(groups):
    """groups uint16 [..., 64 lanes, 8 ktw] -> the packed array's memory order [..., ktw units, 64 lanes, 8]."""
    ktw = groups.shape[-1] // 8
    g = groups.reshape(groups.shape[:-1] + (ktw, 8))
    return np.ascontiguousarray(np.swapaxes(g, -3, -2))


def seal_group(lanes):
    """One group uint16 [64 lanes][8 ktw values], ktw = 16 or 12 -> (sealed uint8 [13 or 10][64][16], fit bool [64]).
    The 12-tile form is the specification's: the lane's 96 values followed by 32 copies of its first value, sealed as a
    16-unit lane, units 0-5, 8-10 and 12 kept."""
    if lanes.shape[1] == 128:
        return ks.seal(lanes, as_k=0)
    assert lanes.shape[1] == 96
    padded = np.concatenate([lanes, np.repeat(lanes[:, :1], 32, axis=1)], axis=1)
    s, fit = ks.seal(padded, as_k=0)
    return s[KEEP12], fit


def unseal_group12(sealed10):
    """sealed uint8 [10][64][16] -> (uint16 [64][96], fit): the kept units put back where the 16-unit form has them."""
    full = np.zeros((13, 64, 16), dtype=np.uint8)
    full[KEEP12] = sealed10
    page, fit = ks.unseal(full, as_k=0)
    return page[:, :96], fit


def unsealed_share(w_bits, ktw):
    """Share of the groups of W [N][K] with a lane of more than 8 distinct high bytes (what the bind-time count reports)."""
    g = groups_of(w_bits, ktw)
    hb = (g >> 8) & 0x7f
    present = np.zeros(g.shape[:-1] + (128,), dtype=bool)
    np.put_along_axis(present, hb.astype(np.int64), True, axis=-1)
    bad = (present.sum(axis=-1) > 8).any(axis=-1)
    return float(bad.mean())
