"""The depth-specialised decode GEMMs (csrc/gemm.hip: gemm_depth_kernel, gemm_gateup48_kernel) rest on what the compiler
does with their load order: every load of a wave must be requested before its first product.  That is a fact about the
code, so it is checked here without a GPU: gemm.hip is compiled for gfx950 to assembly (device only, into a temporary
directory) and each dispatched instantiation is read.

The counts are the design's, not tuned thresholds: a wave of gemm_depth_kernel<8, KTW> requests KTW X fragments and KTW
weight tiles (2 * KTW loads of 16 bytes per lane); a wave of gemm_gateup48_kernel<8, 16> requests 16 X fragments, 16 whole
weight tiles and 16 half tiles (48)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "moss-ttsd_amd", "csrc")

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc is not on the path")

# mangled-name fragment of every specialised instantiation launch_gemm_depth dispatches -> loads in flight per wave
DISPATCHED = {
    "gemm_depth_kernelILi8ELi4ELi0EE": 8,        # o_proj: 2048 x 2048, split-K 4
    "gemm_depth_kernelILi8ELi12ELi0EE": 24,      # down_proj: 2048 x 6144, split-K 4
    "gemm_gateup48_kernelILi8ELi16EE": 48,       # gate/up: 12288 x 2048 on 256 blocks of 48 columns
}


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("gemm_isa") / "gemm.s")
    cmd = ["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fno-gpu-rdc", "--offload-device-only", "-S",
           "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, os.path.join(CSRC, "gemm.hip"), "-o", out]
    subprocess.run(cmd, check=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    return open(out).read()


def _body(asm, frag):
    """Instructions of the one kernel whose mangled name contains `frag`, from its label to s_endpgm."""
    m = re.search(r"^(_Z\w*%s\w*):" % re.escape(frag), asm, re.M)
    assert m, "no kernel matching %s in the assembly" % frag
    end = asm.index("s_endpgm", m.end())
    lines = [ln.split(";")[0].strip() for ln in asm[m.end():end].splitlines()]
    return m.group(1), [ln for ln in lines if ln]


def _meta(asm, name, key):
    """A number from the kernel's entry in amdhsa.kernels (one "  - .key: value" block per kernel, keys sorted)."""
    blocks = [b for b in asm.split("\n  - .") if re.search(r"^\s+\.name:\s+%s$" % re.escape(name), b, re.M)]
    assert len(blocks) == 1, "metadata entries for %s: %d" % (name, len(blocks))
    m = re.search(r"(?:^|\s)\.?%s:\s+(\d+)" % key, blocks[0])
    assert m, "no %s in the metadata of %s" % (key, name)
    return int(m.group(1))


@pytest.mark.parametrize("frag", sorted(DISPATCHED))
def test_all_loads_precede_the_first_product(asm, frag):
    name, ins = _body(asm, frag)
    first = next(i for i, s in enumerate(ins) if s.startswith("v_mfma"))
    head = ins[:first]
    loads = sum(1 for s in head if s.startswith("global_load_dwordx4"))
    assert loads == DISPATCHED[frag], "%s: %d loads of 16 bytes before the first v_mfma" % (name, loads)
    # nothing but these loads reads global memory in the kernel, before or after
    assert sum(1 for s in ins if s.startswith("global_load")) == DISPATCHED[frag]
    drains = [s for s in head if s.startswith("s_waitcnt") and re.search(r"vmcnt\(0\)", s)]
    assert not drains, "%s waits for all of its loads before the first v_mfma: %s" % (name, drains)
    # no branch in the load stream: the head is straight-line code
    assert not [s for s in head if s.startswith("s_cbranch") or s.startswith("s_branch")]


@pytest.mark.parametrize("frag", sorted(DISPATCHED))
def test_no_scratch(asm, frag):
    name, ins = _body(asm, frag)
    assert not [s for s in ins if s.startswith("scratch_") or s.startswith("buffer_")], name + " touches scratch"
    assert _meta(asm, name, "private_segment_fixed_size") == 0
    assert _meta(asm, name, "vgpr_spill_count") == 0
    assert _meta(asm, name, "sgpr_spill_count") == 0
