"""Host logic of the weight-gradient dispatch (gemm_dw): which kernel takes a dense [N x K] product of a training backward, as
`aline_backward_dw_kernel_name` reports it -- the exact-fp32 block kernel, `gemm_tn_f16_kernel` (256 x 256 blocks) or the narrow-tile
instantiation `gemm_tn_f16_narrow_kernel<128, 128>` where a dimension is a multiple of 128 only.  No GPU."""
import ctypes

import pytest

from test_abi import _small_model, lib  # noqa: F401  (the module fixture that builds / loads the library)

F32, WIDE, NARROW = ("gemm_tn_block_kernel", 0), ("gemm_tn_f16_kernel", 1), ("gemm_tn_f16_narrow_kernel<128, 128>", 1)


@pytest.mark.parametrize("prec,N,K,flag,expect", [
    ("f16x3", 256, 256, None, WIDE),
    ("f16x3", 1024, 256, None, WIDE),
    ("f16x3", 128, 128, None, NARROW),
    ("f16x3", 384, 128, None, NARROW),
    ("f16x3", 256, 128, None, NARROW),
    ("f16x3", 512, 128, None, NARROW),
    ("f16x3", 128, 512, None, NARROW),
    ("f16x3", 192, 128, None, F32),
    ("f16x3", 128, 64, None, F32),
    ("f16x3", 128, 129, None, F32),                       # the time-token head's K = d + 1
    ("f32", 128, 128, None, F32),
    ("f32", 256, 256, None, F32),
    ("f16x3", 128, 128, "NO_BWD_DW_NARROW", F32),
    ("f16x3", 512, 128, "NO_BWD_DW_NARROW", F32),
    ("f16x3", 256, 256, "NO_BWD_DW_NARROW", WIDE),        # the switch leaves the 256 x 256 products alone
    ("f16x3", 128, 128, "BWD_GRAD_F32", F32),
    ("f16x3", 256, 256, "BWD_GRAD_F32", F32),
])
def test_which_kernel_takes_a_weight_gradient_product(lib, prec, N, K, flag, expect):
    from aline_amd import _lib
    m = _small_model()
    m.d, m.F, m.H, m.precision = 128, 512, 4, _lib.PREC[prec]
    buf = ctypes.create_string_buffer(64)
    with _lib.debug(*([flag] if flag else [])):
        rc = _lib.lib.aline_backward_dw_kernel_name(ctypes.byref(m), N, K, buf, 64)
    assert (buf.value.decode(), rc) == expect
    assert _lib.lib.aline_backward_dw_kernel_name(None, N, K, buf, 64) < 0
