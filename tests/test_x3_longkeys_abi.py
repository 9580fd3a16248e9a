"""Host logic of the long-key x3 variants (x3_impl.h, KV_EP: d = 256 rollouts with 65 .. 160 visible keys): which rollouts take the
path, what the dominant kernel is called, and that a rollout inside the 64-key layout keeps its workspace size.  No GPU."""
import ctypes

from test_abi import _small_model, lib  # noqa: F401  (the module fixture that builds / loads the library)

GENERIC, X3 = 0, 3


def test_long_key_rollouts_take_the_x3_path(lib):
    from aline_amd import _lib
    L = _lib.lib
    byref = ctypes.byref

    def rollout(B=1000, P=201, n_ctx0=1, n_td=0, T=30):
        r = _lib.AlineRollout()
        r.B, r.P, r.n_ctx0, r.n_target_data, r.T = B, P, n_ctx0, n_td, T
        return r

    def name(m, r):
        buf = ctypes.create_string_buffer(64)
        L.aline_rollout_kernel_name(byref(m), byref(r), buf, 64)
        return buf.value

    w = _small_model()                                        # theta mode, n_theta = 2: n_ctx0 + T - 1 + 2 keys
    w.d, w.F, w.H = 256, 1024, 8
    w.precision = _lib.PREC["f16x3"]
    assert L.aline_rollout_path(byref(w), byref(rollout(T=62))) == X3 and name(w, rollout(T=62)) == b"x3::layer_kernel<true>"      # 64 keys
    assert L.aline_rollout_path(byref(w), byref(rollout(T=63))) == X3                                  # 65 keys
    assert name(w, rollout(T=63)) == b"x3::layer_long_kernel<true>"
    assert L.aline_rollout_path(byref(w), byref(rollout(T=158))) == X3                                 # 160 keys
    assert L.aline_rollout_path(byref(w), byref(rollout(T=159))) == GENERIC                            # 161 keys
    w.n_theta, w.embedding_type = 3, 2                                                                 # mix mode (cfg3): 1 + 49 + 103 keys
    assert L.aline_rollout_path(byref(w), byref(rollout(B=512, n_td=100, T=50))) == X3
    w.n_theta, w.embedding_type = 2, 1
    # a rollout inside the 64-key layout is sized as before (the literal: aline_rollout_workspace_bytes of the parent commit's build)
    assert L.aline_rollout_workspace_bytes(byref(w), byref(rollout(B=8, P=101, T=62))) == WS_BYTES_64_KEYS
    assert L.aline_rollout_workspace_bytes(byref(w), byref(rollout(B=8, P=101, T=63))) > WS_BYTES_64_KEYS
    w.d, w.F = 512, 128                                                                                # x5 keeps the 64-key limit
    assert L.aline_rollout_path(byref(w), byref(rollout(B=256, T=70))) == GENERIC                      # 72 keys


WS_BYTES_64_KEYS = 78845184      # d = 256 / F = 1024 / L = 3 / C = 10, B = 8, P = 101, T = 62: measured on the parent commit's library
