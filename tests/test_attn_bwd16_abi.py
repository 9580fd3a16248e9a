"""Host logic of the attention-backward dispatch (launch_attention_bwd), as `aline_backward_attn_kernel_name` reports it: heads of 16
channels of an F16X3 model at d >= 64 take `abw16::attention_bwd16_kernel` (attn_bwd16.h) for 1 - 160 keys, whatever N its streamed row
side admits; every other shape keeps its kernel.  No GPU."""
import ctypes

import pytest

from test_abi import _small_model, lib  # noqa: F401  (the module fixture that builds / loads the library)

ABW16, VALU = "abw16::attention_bwd16_kernel", "attention_bwd_kernel"


@pytest.mark.parametrize("d,H,prec,keys,N,flag,expect", [
    (64, 4, "f16x3", 1, 203, None, ABW16),
    (64, 4, "f16x3", 48, 203, None, ABW16),
    (64, 4, "f16x3", 49, 203, None, ABW16),
    (64, 4, "f16x3", 160, 203, None, ABW16),
    (64, 4, "f16x3", 161, 203, None, VALU),
    (128, 8, "f16x3", 64, 203, None, ABW16),
    (256, 16, "f16x3", 64, 203, None, ABW16),
    (64, 4, "f16x3", 40, 1203, None, ABW16),                       # the VALU kernel's LDS: 132 * 40 + 144 * 1203 = 178 512 bytes
    (64, 4, "f16x3", 40, 1203, "NO_BWD_ATTN_MFMA", "unsupported"),
    (64, 4, "f32", 64, 203, None, VALU),
    (64, 4, "f16x3", 64, 203, "NO_BWD_ATTN_MFMA", VALU),
    (64, 4, "f16x3", 64, 203, "BWD_GRAD_F32", VALU),
    (32, 2, "f16x3", 64, 203, None, VALU),                         # d < 64: exact-fp32 gradient products
    (128, 4, "f16x3", 64, 203, None, "abwl::attention_bwd_long_kernel"),
    (128, 2, "f16x3", 64, 203, None, "abwl64::attention_bwd_long64_kernel"),
    (32, 4, "f16x3", 150, 203, None, "abw8::attention_bwd8_kernel"),
])
def test_which_kernel_takes_the_attention_backward(lib, d, H, prec, keys, N, flag, expect):
    from aline_amd import _lib
    m = _small_model()
    m.d, m.F, m.H, m.precision = d, 128, H, _lib.PREC[prec]
    buf = ctypes.create_string_buffer(64)
    with _lib.debug(*([flag] if flag else [])):
        rc = _lib.lib.aline_backward_attn_kernel_name(ctypes.byref(m), keys, N, buf, 64)
    assert rc >= 0 and buf.value.decode() == expect
    assert _lib.lib.aline_backward_attn_kernel_name(None, keys, N, buf, 64) < 0
