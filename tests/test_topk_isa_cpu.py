"""The top-k kernels of csrc/score.hip, in the manner of test_score_isa_cpu.py: score.hip is compiled for gfx950 to
assembly (device only, into a temporary directory) and the kernels' resource metadata is read -- register, LDS and
scratch counts only.  head_topk_kernel is head_ce_kernel's body with a selection after its reduction: it holds the same
64 accumulators through the main loop and must keep its 32 keys of a row tile, and the finish kernels their sorted lists,
in registers -- an array that the compiler indexes dynamically lands in scratch memory.  head_ce_kernel itself, which
shares the body, keeps the figures it had before the top-k kernels existed."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "moss-ttsd_amd", "csrc")
LISTS = [1, 4, 8, 16]                                      # list lengths the finish kernels are instantiated for
NEW = ["head_topk_kernel"] + ["topk_finish_kernelILi%dEE" % n for n in LISTS] + ["topk_rows_f32_kernelILi%dEE" % n for n in LISTS]


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    """-> {mangled name: its entry in amdhsa.kernels}"""
    out = str(tmp_path_factory.mktemp("topk_isa") / "score.s")
    cmd = ["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fno-gpu-rdc", "--offload-device-only", "-S",
           "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, os.path.join(CSRC, "score.hip"), "-o", out]
    subprocess.run(cmd, check=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    found = {}
    for b in open(out).read().split("\n  - ."):
        m = re.search(r"^\s+\.name:\s+(_Z\w+)$", b, re.M)
        if m:
            found[m.group(1)] = b
    return found


def _meta(kernels, frag, key):
    """A number from the metadata of the one kernel whose mangled name contains `frag`."""
    hits = [b for name, b in kernels.items() if frag in name]
    assert len(hits) == 1, "metadata entries for %s: %d" % (frag, len(hits))
    m = re.search(r"(?:^|\s)\.?%s:\s+(\d+)" % key, hits[0])
    assert m, "no %s in the metadata of %s" % (key, frag)
    return int(m.group(1))


def test_the_kernels_of_score_hip(kernels):
    assert len(kernels) == 3 + len(NEW)                    # head_ce, ce_finish, ce_rows_f32 and the new ones


@pytest.mark.parametrize("frag", NEW)
def test_no_scratch_no_spills(kernels, frag):
    assert _meta(kernels, frag, "private_segment_fixed_size") == 0
    assert _meta(kernels, frag, "vgpr_spill_count") == 0
    assert _meta(kernels, frag, "sgpr_spill_count") == 0


def test_head_topk_register_budget(kernels):
    """The four 32 x 32 accumulators stay in the accumulator registers through the main loop; the selection works on one
    row tile at a time (32 keys), after the main loop's operand fragments are dead, so the kernel fits the 192 registers
    head_ce_kernel is held to: two waves per SIMD either way.  LDS: the partials (2 KiB) and the waves' sorted lists,
    2 x 2 x 2 x 16 x 32 words."""
    assert _meta(kernels, "head_topk_kernel", "agpr_count") == 64
    assert _meta(kernels, "head_topk_kernel", "vgpr_count") <= 192
    assert _meta(kernels, "head_topk_kernel", "group_segment_fixed_size") == 2048 + 16384


def test_head_ce_kernel_is_as_it_was(kernels):
    """The figures of the kernel before the body was shared (176 registers, 96 scalar registers, 2 KiB of LDS)."""
    assert _meta(kernels, "head_ce_kernel", "agpr_count") == 64
    assert _meta(kernels, "head_ce_kernel", "vgpr_count") == 176
    assert _meta(kernels, "head_ce_kernel", "sgpr_count") == 96
    assert _meta(kernels, "head_ce_kernel", "group_segment_fixed_size") == 2048
    assert _meta(kernels, "head_ce_kernel", "private_segment_fixed_size") == 0
    for frag, vgpr, lds in (("16ce_finish_kernel", 11, 0), ("ce_rows_f32_kernel", 15, 16)):
        assert _meta(kernels, frag, "vgpr_count") == vgpr and _meta(kernels, frag, "group_segment_fixed_size") == lds


def test_finish_lists_stay_in_registers(kernels):
    """A list of n (value, column) pairs is 2 n registers; the kernels around it need a few dozen more, not hundreds."""
    for n in LISTS:
        assert _meta(kernels, "topk_finish_kernelILi%dEE" % n, "vgpr_count") <= 2 * n + 32
        assert _meta(kernels, "topk_rows_f32_kernelILi%dEE" % n, "vgpr_count") <= 2 * n + 32
