"""The whole-row decode attention kernel (csrc/attn.hip: attn_row_kernel) runs ROW_WAVES waves per block, one block per
CU, so ROW_WAVES / 4 waves share a SIMD's 512 registers: what the compiler allocates per lane has to fit that share, and
nothing may spill (a spilled page unit is a round trip through memory in the middle of the stream).  Both are facts about
the code, so they are checked without a GPU: attn.hip is compiled for gfx950 to assembly (device only, into a temporary
directory) and the resource metadata of every dispatched instantiation is read."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "moss-ttsd_amd", "csrc")

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc is not on the path")

# launch_attn dispatches G = 1, 2, 4, each with bf16 pages only and with sealed pages
DISPATCHED = ["attn_row_kernelILi%dELb%dEE" % (g, pk) for g in (1, 2, 4) for pk in (0, 1)]


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("attn_isa") / "attn.s")
    cmd = ["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fno-gpu-rdc", "--offload-device-only", "-S",
           "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, os.path.join(CSRC, "attn.hip"), "-o", out]
    subprocess.run(cmd, check=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    return open(out).read()


def _row_waves():
    src = open(os.path.join(CSRC, "shapes.h")).read()          # (single-sourced with the step planner)
    return int(re.search(r"^#define ROW_WAVES (\d+)", src, re.M).group(1))


def _entry(asm, frag):
    """The amdhsa.kernels entry of the one kernel whose mangled name contains `frag`."""
    blocks = [b for b in asm.split("\n  - .") if re.search(r"^\s+\.name:\s+_Z\w*%s\w*$" % re.escape(frag), b, re.M)]
    assert len(blocks) == 1, "metadata entries for %s: %d" % (frag, len(blocks))
    return blocks[0]


def _meta(entry, key):
    m = re.search(r"(?:^|\s)\.?%s:\s+(\d+)" % key, entry)
    assert m, "no %s in the metadata" % key
    return int(m.group(1))


def _body(asm, frag):
    """Instructions of the one kernel whose mangled name contains `frag`, from its label to its .Lfunc_end label (the
    kernel has more than one s_endpgm: the idle row leaves early)."""
    m = re.search(r"^(_Z\w*%s\w*):" % re.escape(frag), asm, re.M)
    assert m, "no kernel matching %s in the assembly" % frag
    end = re.compile(r"^\.Lfunc_end\d+:", re.M).search(asm, m.end()).start()
    lines = [ln.split(";")[0].strip() for ln in asm[m.end():end].splitlines()]
    return [ln for ln in lines if ln]


@pytest.mark.parametrize("frag", DISPATCHED)
def test_no_scratch(asm, frag):
    e = _entry(asm, frag)
    assert _meta(e, "private_segment_fixed_size") == 0
    assert _meta(e, "vgpr_spill_count") == 0
    assert _meta(e, "sgpr_spill_count") == 0
    assert not [s for s in _body(asm, frag) if s.startswith("scratch_")], frag + " touches scratch"


@pytest.mark.parametrize("frag", DISPATCHED)
def test_registers_fit_the_waves_of_a_block(asm, frag):
    """A SIMD holds min(8, 512 / allocation) waves, the allocation being VGPRs + AGPRs rounded up to 8; a block puts
    ceil(ROW_WAVES / 4) on each."""
    e = _entry(asm, frag)
    waves_per_simd = (_row_waves() + 3) // 4
    alloc = (_meta(e, "vgpr_count") + _meta(e, "agpr_count") + 7) // 8 * 8
    assert alloc * waves_per_simd <= 512, "%s: %d registers per lane x %d waves per SIMD" % (frag, alloc, waves_per_simd)
    assert _meta(e, "max_flat_workgroup_size") == 64 * _row_waves()


def test_static_lds_is_none(asm):
    """Everything the block keeps in LDS is in the dynamic segment sized by attn_row_lds_bytes."""
    for frag in DISPATCHED:
        assert _meta(_entry(asm, frag), "group_segment_fixed_size") == 0
