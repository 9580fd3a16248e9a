"""Host logic of the training backward's forward recompute on the long-key layout (x3_host.h: recompute, `x3::layer_save_long_kernel`):
which kernel recomputes a chunk, whether Q comes from it, and what the key buffers of the larger plan cost.  No GPU."""
import ctypes

import pytest

from test_abi import _small_model, lib  # noqa: F401  (the module fixture that builds / loads the library)


def _rollout(P=201, T=159):
    from aline_amd import _lib
    r = _lib.AlineRollout()
    r.B, r.P, r.n_ctx0, r.n_target_data, r.T = 4, P, 1, 0, T
    return r


def _wide(d=256, F=1024, prec="f16x3"):
    from aline_amd import _lib
    w = _small_model()                                        # theta mode, n_theta = 2: a chunk [t0, t0 + nt) shows t0 + nt + 2 keys
    w.d, w.F, w.H, w.precision = d, F, 8, _lib.PREC[prec]
    return w


def _name(m, r, t0, nt):
    from aline_amd import _lib
    buf = ctypes.create_string_buffer(64)
    rc = _lib.lib.aline_backward_recompute_name(ctypes.byref(m), ctypes.byref(r), t0, nt, buf, 64)
    return buf.value.decode(), rc


SHORT, LONG = "x3::layer_save_kernel", "x3::layer_save_long_kernel"


@pytest.mark.parametrize("model,t0,nt,flag,expect", [
    (dict(), 0, 46, None, (SHORT, 1)),                                 # 48 keys: abww <32, 3>
    (dict(), 0, 47, None, (SHORT, 1)),                                 # 49 keys: abwl reads key rows only -- Q from the layer kernel (was 0)
    (dict(), 40, 22, None, (SHORT, 1)),                                # 64 keys
    (dict(), 40, 23, None, (LONG, 1)),                                 # 65 keys
    (dict(), 100, 58, None, (LONG, 1)),                                # 160 keys
    (dict(), 100, 59, None, ("generic", 0)),                           # 161 keys
    (dict(d=512, F=128), 0, 62, None, ("x5::layer_save_kernel", 0)),   # d = 512 keeps the 64-key limit (and abww's 48 for Q)
    (dict(d=512, F=128), 0, 63, None, ("generic", 0)),
    (dict(prec="f32"), 40, 23, None, ("generic", 0)),
    (dict(), 40, 23, "NO_BWD_IMAGE_RECOMPUTE", ("generic", 0)),
    (dict(), 40, 23, "BWD_RECOMPUTE_F32", ("generic", 0)),
    (dict(), 40, 23, "NO_BWD_ATTN_MFMA", (LONG, 0)),                   # the VALU attention backward reads K | V of every row
])
def test_which_kernel_recomputes_a_chunk(lib, model, t0, nt, flag, expect):
    from aline_amd import _lib
    with _lib.debug(*([flag] if flag else [])):
        assert _name(_wide(**model), _rollout(), t0, nt) == expect
    assert _name(_wide(), _rollout(), 100, 60)[1] < 0 and _name(_wide(), _rollout(), 0, 0)[1] < 0      # past T, empty chunk


def test_backward_workspace_grows_only_where_a_chunk_exceeds_64_keys(lib):
    """The literals: aline_rollout_backward_workspace_bytes of the parent commit's library (B = 4, P = 101 / 201, L = 3, C = 10)."""
    from aline_amd import _lib

    def ws(w, P, T, tc):
        return _lib.lib.aline_rollout_backward_workspace_bytes(ctypes.byref(w), ctypes.byref(_rollout(P, T)), tc)
    w, w5 = _wide(), _wide(d=512, F=128)
    assert ws(w, 101, 62, 31) == 779947008           # 64 keys
    assert ws(w, 101, 63, 31) > 779947008            # 65 keys: same rows, two blocks of keys (parent: equal)
    assert ws(w, 101, 70, 35) > 875857664            # 72 keys
    assert ws(w5, 101, 70, 35) == 1129208064         # d = 512 at 72 keys: generic recompute, as before
    assert ws(w5, 101, 30, 15) == 497654272
    # a backward that ends beyond 160 keys still has chunks within them, on up to three blocks: no smaller than the same rows at 160 keys
    assert ws(w, 201, 159, 23) >= ws(w, 201, 158, 23) > ws(w, 201, 62, 23)
