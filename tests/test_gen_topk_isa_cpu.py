"""The kernels of csrc/gen_topk.hip (generate(top_logprobs=k)), in the manner of test_topk_isa_cpu.py: the file is compiled
for gfx950 to assembly (device only, into a temporary directory) and the kernels' resource metadata is read -- register,
LDS and scratch counts only.  Both kernels keep a thread's sorted list of (value, id) pairs in registers (topk.h:
TopList); a list the compiler indexes dynamically would land in scratch memory.  The same for update_kernel's two
instantiations in sampler.hip, which commits the results."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "moss-ttsd_amd", "csrc")
LISTS = [1, 4, 8, 16]                                      # list lengths the kernels are instantiated for
NEW = ["gen_topk_slice_kernelILi%dEE" % n for n in LISTS] + ["gen_topk_finish_kernelILi%dEE" % n for n in LISTS]


def _kernels(tmp, src):
    """-> {mangled name: its entry in amdhsa.kernels}"""
    out = str(tmp / (src + ".s"))
    cmd = ["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fno-gpu-rdc", "--offload-device-only", "-S",
           "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, os.path.join(CSRC, src), "-o", out]
    subprocess.run(cmd, check=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    found = {}
    for b in open(out).read().split("\n  - ."):
        m = re.search(r"^\s+\.name:\s+(_Z\w+)$", b, re.M)
        if m:
            found[m.group(1)] = b
    return found


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    return _kernels(tmp_path_factory.mktemp("gen_topk_isa"), "gen_topk.hip")


@pytest.fixture(scope="module")
def sampler_kernels(tmp_path_factory):
    return _kernels(tmp_path_factory.mktemp("gen_topk_isa_sampler"), "sampler.hip")


def _meta(kernels, frag, key):
    """A number from the metadata of the one kernel whose mangled name contains `frag`."""
    hits = [b for name, b in kernels.items() if frag in name]
    assert len(hits) == 1, "metadata entries for %s: %d" % (frag, len(hits))
    m = re.search(r"(?:^|\s)\.?%s:\s+(\d+)" % key, hits[0])
    assert m, "no %s in the metadata of %s" % (key, frag)
    return int(m.group(1))


def test_the_kernels_of_gen_topk_hip(kernels):
    assert len(kernels) == len(NEW)                        # one slice and one finish kernel per list length, nothing else


@pytest.mark.parametrize("frag", NEW)
def test_no_scratch_no_spills(kernels, frag):
    assert _meta(kernels, frag, "private_segment_fixed_size") == 0
    assert _meta(kernels, frag, "vgpr_spill_count") == 0
    assert _meta(kernels, frag, "sgpr_spill_count") == 0


def test_lists_stay_in_registers(kernels):
    """A list of n (value, id) pairs is 2 n registers.  Around it: the pair being inserted and the one it displaces (4),
    the wave maximum's exchange (4), the row pointer, column index and bounds (8), the fp32 / fp64 sums and the log-sum-exp
    (8), addresses of the results (8), and room for the scheduler: 48, not hundreds.  LDS: four floats, four doubles and
    four pairs, padded to 80 bytes; the finish kernel also holds the 32 rescaled slice sums (256 bytes)."""
    for n in LISTS:
        for kern, lds in (("gen_topk_slice_kernelILi%dEE", 96), ("gen_topk_finish_kernelILi%dEE", 96 + 256)):
            assert _meta(kernels, kern % n, "vgpr_count") <= 2 * n + 48
            assert _meta(kernels, kern % n, "group_segment_fixed_size") <= lds


@pytest.mark.parametrize("frag", ["update_kernelILb0EE", "update_kernelILb1EE"])
def test_update_kernel_commits_from_registers(sampler_kernels, frag):
    """tok[8] and the rule's eight outcomes are indexed by unrolled loops in both instantiations."""
    assert _meta(sampler_kernels, frag, "private_segment_fixed_size") == 0
    assert _meta(sampler_kernels, frag, "vgpr_spill_count") == 0
    assert _meta(sampler_kernels, frag, "sgpr_spill_count") == 0
