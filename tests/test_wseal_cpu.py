"""Sealed weight streams (csrc/gemm_sealed.hip), the part that needs no GPU.

1. The kernels rest on their load order, like the bf16 kernels they shadow (tests/test_gemm_isa_cpu.py): gemm_sealed.hip is
   compiled for gfx950 to assembly and every dispatched instantiation is read.  The counts are the design's: a wave
   requests its X fragments (16, or 12 for down_proj), then the units of its sealed group(s) -- 13 for 16 k-tiles, 10 for
   12 -- all before its first product, the dictionary unit (whose flag decides the path) first among them:
     gateup48_sealed_kernel<8, 16>        16 + 13 (whole tile) + 13 (half tile) = 42
     depth_sealed_kernel<8, 12, partial>  12 + 10 = 22
     head_sealed_kernel<8, 16>            16 + 13 (first tile) + 13 (the next tile, requested before the first product) = 42
     depth_sealed_kernel<8, 16, bf16>     16 + 13 = 29 (a head tile per block: the form the persistent kernel is measured against)
   The bf16 tiles of a group that did not seal are requested behind the flag's branch, outside this straight-line head.
2. The 12-tile group is specified through the 16-unit oracle (oracle/kv_seal_oracle.py) without touching it.
3. The weights the GPU tests draw seal: the condition under which a green GPU comparison shows the sealed path ran."""
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import wseal_ref as wr
from mtts import synth
from oracle import kv_seal_oracle as ks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "moss-ttsd_amd", "csrc")

needs_hipcc = pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc is not on the path")

# mangled-name fragment of every instantiation launch_gemm_sealed dispatches -> 16-byte loads in front of the first product
DISPATCHED = {
    "gateup48_sealed_kernelILi8ELi16EE": 42,
    "depth_sealed_kernelILi8ELi12ELi0EE": 22,
    "head_sealed_kernelILi8ELi16EE": 42,
    "depth_sealed_kernelILi8ELi16ELi1EE": 29,
}
# share of not-sealed groups the GPU tests' weights may have (the oracle's Gaussian rate is about 0.98 sealed)
UNSEALED_CAP = 0.10


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("wseal_isa") / "gemm_sealed.s")
    cmd = ["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fno-gpu-rdc", "--offload-device-only", "-S",
           "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, os.path.join(CSRC, "gemm_sealed.hip"), "-o", out]
    subprocess.run(cmd, check=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    return open(out).read()


def _body(asm, frag):
    """Instructions of the one kernel whose mangled name contains `frag`, from its label to the first s_endpgm."""
    m = re.search(r"^(_Z\w*%s\w*):" % re.escape(frag), asm, re.M)
    assert m, "no kernel matching %s in the assembly" % frag
    end = asm.index("s_endpgm", m.end())
    lines = [ln.split(";")[0].strip() for ln in asm[m.end():end].splitlines()]
    return m.group(1), [ln for ln in lines if ln]


def _meta(asm, name, key):
    blocks = [b for b in asm.split("\n  - .") if re.search(r"^\s+\.name:\s+%s$" % re.escape(name), b, re.M)]
    assert len(blocks) == 1, "metadata entries for %s: %d" % (name, len(blocks))
    m = re.search(r"(?:^|\s)\.?%s:\s+(\d+)" % key, blocks[0])
    assert m, "no %s in the metadata of %s" % (key, name)
    return int(m.group(1))


@needs_hipcc
@pytest.mark.parametrize("frag", sorted(DISPATCHED))
def test_sealed_units_are_requested_before_the_first_product(asm, frag):
    name, ins = _body(asm, frag)
    first = next(i for i, s in enumerate(ins) if s.startswith("v_mfma"))
    head = ins[:first]
    loads = sum(1 for s in head if s.startswith("global_load_dwordx4"))
    assert loads == DISPATCHED[frag], "%s: %d loads of 16 bytes before the first v_mfma" % (name, loads)
    drains = [s for s in head if s.startswith("s_waitcnt") and re.search(r"vmcnt\(0\)", s)]
    assert not drains, "%s waits for all of its loads before the first v_mfma: %s" % (name, drains)


@needs_hipcc
@pytest.mark.parametrize("frag", sorted(DISPATCHED))
def test_no_scratch(asm, frag):
    name, _ = _body(asm, frag)
    whole = asm[asm.index(name + ":"):asm.index(".Lfunc_end", asm.index(name + ":"))]      # the not-sealed path included
    ins = [ln.split(";")[0].strip() for ln in whole.splitlines()]
    assert not [s for s in ins if s.startswith("scratch_") or s.startswith("buffer_")], name + " touches scratch"
    assert _meta(asm, name, "private_segment_fixed_size") == 0
    assert _meta(asm, name, "vgpr_spill_count") == 0
    assert _meta(asm, name, "sgpr_spill_count") == 0


def _adversarial_lanes(rng):
    """uint16 [64 lanes][96 values]: Gaussian lanes, then lanes built by hand."""
    v = wr.bf16_bits(0.02 * rng.standard_normal((64, 96), dtype=np.float32))
    e8 = np.array([0x3f, 0x3e, 0x3d, 0x3c, 0x3b, 0x20, 0x10, 0x00], dtype=np.uint16)
    v[0] = (e8[rng.integers(0, 8, 96)] << 8) | rng.integers(0, 256, 96) | (rng.integers(0, 2, 96) << 15)
    v[0, :8] = (e8 << 8) | 0x55                                   # exactly 8 distinct high bytes: fits
    v[1] = v[0]
    v[1, 95] = 0x2a11                                             # a ninth, in the last value: does not fit
    v[2] = v[0]
    v[2, 0] = 0x2a11                                              # a ninth, in the value the padding repeats
    v[3] = rng.integers(0, 0x80, 96)                              # denormals
    v[4] = np.where(rng.random(96) < 0.5, 0x7f80, 0xffc1)         # +inf and a negative NaN
    v[5] = np.where(rng.random(96) < 0.5, 0x0000, 0x8000)         # +0.0 and -0.0
    v[6] = rng.integers(0, 1 << 16, 96)                           # random bits: far more than 8
    v[7] = 0x3c3c                                                 # one value
    return v


@pytest.mark.parametrize("seed", [0, 1])
def test_twelve_tile_group_is_the_sixteen_unit_oracle_with_units_dropped(seed):
    rng = np.random.default_rng(seed)
    v = _adversarial_lanes(rng)
    sealed, fit = wr.seal_group(v)
    assert sealed.shape == (10, 64, 16)
    assert list(fit[:8]) == [True, False, False, True, True, True, False, True]
    assert fit[8:].mean() > 0.95
    # the padding adds no high byte: a lane fits exactly when its own 96 values hold at most 8
    own = np.array([len(np.unique((l >> 8) & 0x7f)) <= 8 for l in v])
    assert np.array_equal(fit, own)
    got, fit2 = wr.unseal_group12(sealed)
    assert np.array_equal(fit2, fit)
    assert np.array_equal(got[fit], v[fit])                       # bit for bit: zeros' signs, denormals, inf, NaN
    # what is dropped holds nothing of the 96 values: units 6, 7 (low bytes of the padding) and 11 (its nibbles)
    padded = np.concatenate([v, np.repeat(v[:, :1], 32, axis=1)], axis=1)
    full, _ = ks.seal(padded, as_k=0)
    changed = padded.copy()
    changed[fit, 96:] ^= 0x00ff                                   # other low bytes in the padding, same high bytes
    full2, _ = ks.seal(changed, as_k=0)
    assert np.array_equal(full[wr.KEEP12][:9], full2[wr.KEEP12][:9]) and np.array_equal(full[12], full2[12])


def test_groups_follow_the_packed_layout():
    """groups_of against common.h's wpack_off, element by element on a small matrix."""
    N, K, ktw = 64, 384, 12
    w = np.arange(N * K, dtype=np.uint32).reshape(N, K)
    g = wr.groups_of((w & 0xffff).astype(np.uint16), ktw)
    KT = K // 16
    flat = np.zeros(N * K, dtype=np.uint16)
    n, k = np.meshgrid(np.arange(N), np.arange(K), indexing="ij")
    off = ((((n >> 5) * KT + (k >> 4)) * 64) + (n & 31) + 32 * ((k >> 3) & 1)) * 8 + (k & 7)
    flat[off.ravel()] = (w & 0xffff).astype(np.uint16).ravel()
    packed = flat.reshape(N // 32, KT // ktw, ktw, 64, 8)          # [nt][group][unit][lane][8]
    assert np.array_equal(wr.packed_of(g), packed)


def test_the_gpu_tests_weights_seal():
    """N(0, 0.02^2) rounded to bf16 -- what mtts.synth draws for matrices and embedding tables at the bench's width, and what
    tests/test_wseal_gpu.py draws on the device -- in the three group shapes: gate/up (gate and up rows interleaved),
    down_proj, a head's tiles."""
    p = inspect.signature(synth.synth_weights).parameters
    assert p["emb_std"].default == 0.02 and "else 0.02" in inspect.getsource(synth.synth_weights)
    rng = np.random.default_rng(11)
    for name, (N, K), ktw in (("gate/up", (3072, 2048), 16), ("down_proj", (1024, 6144), 12), ("head", (2048, 2048), 16)):
        share = wr.unsealed_share(wr.bf16_bits(0.02 * rng.standard_normal((N, K), dtype=np.float32)), ktw)
        print("%s: %.4f of the groups do not seal" % (name, share))
        assert share <= UNSEALED_CAP, name
