"""Dispatch rules of the x1 path (aline_amd/csrc/x1.h: d = 128, 4 heads of 32, f16x3, up to 64 visible keys) -- host logic only -- and
the workspace sizes of the rollouts that take another path, which the x1 buffers must not change."""
import ctypes

import pytest

from test_abi import _small_model

X1, GENERIC = 6, 0


def _rollout(B=1000, P=201, n_ctx0=1, n_td=0, T=30):
    from aline_amd import _lib
    r = _lib.AlineRollout()
    r.B, r.P, r.n_ctx0, r.n_target_data, r.T = B, P, n_ctx0, n_td, T
    return r


def _model(d, F, H, prec="f16x3"):
    from aline_amd import _lib
    m = _small_model()
    m.d, m.F, m.H, m.precision = d, F, H, _lib.PREC[prec]
    return m


def test_x1_dispatch():
    from aline_amd import _lib
    L, byref = _lib.lib, ctypes.byref
    m = _model(128, 512, 4)
    buf = ctypes.create_string_buffer(64)
    assert L.aline_rollout_path(byref(m), byref(_rollout())) == X1
    assert L.aline_rollout_kernel_name(byref(m), byref(_rollout()), buf, 64) == X1 and buf.value == b"x1::layer_kernel<true>"
    assert L.aline_rollout_path(byref(m), byref(_rollout(T=62))) == X1            # 1 + 61 + 2 = 64 keys
    assert L.aline_rollout_path(byref(m), byref(_rollout(T=63))) == GENERIC       # 65 keys
    assert L.aline_rollout_path(byref(_model(128, 512, 8)), byref(_rollout())) == GENERIC      # head_dim 16
    assert L.aline_rollout_path(byref(_model(128, 512, 4, "f32")), byref(_rollout())) != X1
    with _lib.debug("DISABLE_X1"):
        assert L.aline_rollout_path(byref(m), byref(_rollout())) == GENERIC
    with _lib.debug_env({"ALINE_DISABLE_X1": "1"}):
        assert L.aline_rollout_path(byref(m), byref(_rollout())) == GENERIC
    assert L.aline_rollout_path(byref(m), byref(_rollout())) == X1


@pytest.mark.parametrize("d,F,H,B,path,nbytes", [(32, 128, 4, 1000, 4, 498799872), (256, 1024, 8, 1000, 3, 4412366848),
                                                (512, 128, 8, 256, 5, 1653520128)])
def test_other_paths_keep_their_workspace(d, F, H, B, path, nbytes):
    """Literals: aline_rollout_workspace_bytes of the library before the x1 path existed."""
    from aline_amd import _lib
    m, r = _model(d, F, H), _rollout(B=B)
    assert _lib.lib.aline_rollout_path(ctypes.byref(m), ctypes.byref(r)) == path
    assert _lib.lib.aline_rollout_workspace_bytes(ctypes.byref(m), ctypes.byref(r)) == nbytes
