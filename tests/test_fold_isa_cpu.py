"""The kernels of csrc/gemm_fold.hip rest, like the depth-specialised GEMMs (tests/test_gemm_isa_cpu.py), on what the
compiler does with their load order and their registers.  Checked without a GPU: the file is compiled for gfx950 to
assembly (device only, into a temporary directory) and each dispatched instantiation is read.

The counts are the design's: a wave of oproj_resid_kernel<8, 4, 4> requests 16 X fragments and 16 weight tiles (32 loads of
16 bytes per lane) and the 8 bytes of residual its lane adds; a wave of gemm_gateup48_norm_kernel<8, 16> requests its
share of the norm weights (1), 16 fragments of x' and 16 whole + 16 half weight tiles (49).  The norm prologue runs under
the weight loads, so it must wait for its own operands by count and never for everything."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "moss-ttsd_amd", "csrc")

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc is not on the path")

# mangled-name fragment of every instantiation the launchers dispatch -> (16-byte loads per wave, of which weight tiles)
DISPATCHED = {
    "oproj_resid_kernelILi8ELi4ELi4EE": (32, 16),              # o_proj on 256 blocks of 8 columns
    "gemm_gateup48_norm_kernelILi8ELi16EE": (49, 32),
}


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("fold_isa") / "gemm_fold.s")
    cmd = ["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fno-gpu-rdc", "--offload-device-only", "-S",
           "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, os.path.join(CSRC, "gemm_fold.hip"), "-o", out]
    subprocess.run(cmd, check=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    return open(out).read()


def _body(asm, frag):
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


@pytest.mark.parametrize("frag", sorted(DISPATCHED))
def test_all_loads_precede_the_first_product(asm, frag):
    name, ins = _body(asm, frag)
    loads, tiles = DISPATCHED[frag]
    first = next(i for i, s in enumerate(ins) if s.startswith("v_mfma"))
    head = ins[:first]
    x4 = [s for s in head if s.startswith("global_load_dwordx4")]
    assert len(x4) == loads, "%s: %d loads of 16 bytes before the first v_mfma" % (name, len(x4))
    # the weight tiles are the non-temporal ones; every one of them is requested before the first product
    assert sum(1 for s in x4 if s.endswith(" nt")) == tiles
    assert not [s for s in ins[first:] if s.startswith("global_load_dwordx4")]
    # no 16-byte load anywhere else, and nothing else but the producer's 8 bytes of residual
    other = [s for s in ins if s.startswith("global_load") and not s.startswith("global_load_dwordx4")]
    assert len(other) == (1 if "oproj" in frag else 0) and all(s.startswith("global_load_dwordx2") for s in other)
    drains = [s for s in head if s.startswith("s_waitcnt") and re.search(r"vmcnt\(0\)", s)]
    assert not drains, "%s waits for all of its loads before the first v_mfma: %s" % (name, drains)


def test_the_norm_prologue_waits_by_count(asm):
    """The first wait of the consumer leaves at least its 32 weight tiles in flight."""
    name, ins = _body(asm, "gemm_gateup48_norm_kernelILi8ELi16EE")
    first = next(i for i, s in enumerate(ins) if s.startswith("v_mfma"))
    waits = [int(m.group(1)) for s in ins[:first] for m in [re.search(r"vmcnt\((\d+)\)", s)] if m]
    assert waits and waits[0] >= 32, waits
    # and the prologue is there: its three barriers (sums of squares, row scales, the GEMM's reduction)
    assert sum(1 for s in ins if s.startswith("s_barrier")) == 3


@pytest.mark.parametrize("frag", sorted(DISPATCHED))
def test_no_scratch_no_spill(asm, frag):
    name, ins = _body(asm, frag)
    assert not [s for s in ins if s.startswith("scratch_") or s.startswith("buffer_")], name + " touches scratch"
    assert _meta(asm, name, "private_segment_fixed_size") == 0
    assert _meta(asm, name, "vgpr_spill_count") == 0
    assert _meta(asm, name, "sgpr_spill_count") == 0
