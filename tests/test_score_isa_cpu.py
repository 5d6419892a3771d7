"""head_ce_kernel (csrc/score.hip) keeps gemm_tile_kernel's 2 x 2 accumulators (64 registers) live through an epilogue
that reduces them in place.  That only works while everything stays in registers: a spill would put the accumulators in
scratch memory in the middle of the hot loop.  A fact about the code, checked without a GPU: score.hip is compiled for
gfx950 to assembly (device only, into a temporary directory) and the kernels' resource metadata is read -- register and
scratch counts only."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "moss-ttsd_amd", "csrc")
KERNELS = ["head_ce_kernel", "ce_finish_kernel", "ce_rows_f32_kernel"]


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("score_isa") / "score.s")
    cmd = ["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fno-gpu-rdc", "--offload-device-only", "-S",
           "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, os.path.join(CSRC, "score.hip"), "-o", out]
    subprocess.run(cmd, check=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    return open(out).read()


def _meta(asm, frag, key):
    """A number from the entry in amdhsa.kernels of the one kernel whose name contains `frag`."""
    blocks = [b for b in asm.split("\n  - .") if re.search(r"^\s+\.name:\s+_Z\w*%s\w*$" % re.escape(frag), b, re.M)]
    assert len(blocks) == 1, "metadata entries for %s: %d" % (frag, len(blocks))
    m = re.search(r"(?:^|\s)\.?%s:\s+(\d+)" % key, blocks[0])
    assert m, "no %s in the metadata of %s" % (key, frag)
    return int(m.group(1))


@pytest.mark.parametrize("frag", KERNELS)
def test_no_scratch_no_spills(asm, frag):
    assert _meta(asm, frag, "private_segment_fixed_size") == 0
    assert _meta(asm, frag, "vgpr_spill_count") == 0
    assert _meta(asm, frag, "sgpr_spill_count") == 0


def test_head_ce_register_budget(asm):
    """The main loop alone holds 64 accumulators + 4 x 8 operand fragments of 4 registers; the epilogue reduces the
    accumulators in place and must add next to nothing.  The kernel compiles to 176 registers per lane (112 + the 64
    accumulators); 192 leaves two allocation steps of 8 for the compiler's scheduling and no more."""
    assert _meta(asm, "head_ce_kernel", "agpr_count") == 64               # the four 32 x 32 accumulators
    assert _meta(asm, "head_ce_kernel", "vgpr_count") <= 192              # arch + acc registers of a wave
    assert _meta(asm, "head_ce_kernel", "group_segment_fixed_size") == 2048
