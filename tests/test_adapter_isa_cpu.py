"""The adapter-merge kernels (csrc/adapter.hip) keep a thread's 16 sums and its base groups in registers while the
adapter's rows and columns pass through LDS: a spill would put them in scratch memory inside the r loop.  And the
definition they implement (mtts/adapters.py: merge_spec) is one IEEE multiply and one IEEE add per term, which hipcc's
default contraction would turn into fused multiply-adds -- different bits.  Facts about the code, checked without a GPU:
adapter.hip is compiled for gfx950 to assembly (device only, into a temporary directory); the kernels' resource metadata
and the floating-point opcodes are read."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "moss-ttsd_amd", "csrc")
KERNELS = ["lora_pack_kernel", "lora_rows_f32_kernel"]


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("adapter_isa") / "adapter.s")
    cmd = ["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fno-gpu-rdc", "--offload-device-only", "-S",
           "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, os.path.join(CSRC, "adapter.hip"), "-o", out]
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
    assert _meta(asm, frag, "vgpr_count") <= 128                          # four waves per SIMD
    assert _meta(asm, frag, "group_segment_fixed_size") <= 32 * 1024      # A chunk 16 KiB + B chunk 4.1 KiB


def test_multiply_and_add_stay_apart(asm):
    """No fused or multiply-accumulate fp32 opcode anywhere in the file; the sums are v_(pk_)mul_f32 and v_(pk_)add_f32."""
    ops = set(re.findall(r"^\s+(v_[a-z0-9_]+)", asm, re.M))
    fused = sorted(o for o in ops if re.match(r"v_(pk_)?(fma|fmac|mac|mad|dot)\w*_(f32|f16|bf16)", o) or o.startswith("v_mfma"))
    assert not fused, fused
    assert ops & {"v_mul_f32_e32", "v_mul_f32_e64", "v_pk_mul_f32"} and ops & {"v_add_f32_e32", "v_add_f32_e64", "v_pk_add_f32"}
