"""resid_norm_kernel and the kernels of csrc/gemm_fold.hip round fp32 to bf16 with the hardware's v_cvt_pk_bf16_f32
(csrc/norm_ops.h: pack2_rn) where the rest of the engine uses the software f2bf (csrc/common.h).  Their bits are the
reference's only if the two are the same function, so a kernel compares them on every one of the 2^32 inputs.  -m gpu."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

pytest.importorskip("torch")

from mtts import capi  # noqa: E402


def test_hardware_rounding_is_f2bf_on_every_input():
    out = np.full(2, -1, dtype=np.int64)
    capi.check(capi.lib().mtts_k_bf16_round_check(out.ctypes.data, None))
    assert out.tolist() == [0, 0], "inputs on which pack2_rn != f2bf: %d that are not NaN, %d NaN" % tuple(out)
