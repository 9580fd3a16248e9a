"""Host logic of the training backward's forward recompute at d = 128 (x3_host.h: recompute in namespace x1, `x1::layer_save_kernel`):
which kernel recomputes a chunk and whether Q comes from it.  No GPU."""
import pytest

from test_abi import lib  # noqa: F401  (the module fixture that builds / loads the library)
from test_recompute_longkeys_abi import _name, _rollout, _wide

SAVE = "x1::layer_save_kernel"


def _x1(H=4, prec="f16x3"):      # theta mode, n_theta = 2: a chunk [t0, t0 + nt) shows t0 + nt + 2 keys
    w = _wide(d=128, F=512, prec=prec)
    w.H = H
    return w


@pytest.mark.parametrize("model,t0,nt,flag,expect", [
    (dict(), 0, 46, None, (SAVE, 1)),                            # 48 keys: abww <32, 3> reads key rows only
    (dict(), 0, 47, None, (SAVE, 1)),                            # 49 keys: abwl
    (dict(), 40, 22, None, (SAVE, 1)),                           # 64 keys: the last the x1 attention holds
    (dict(), 40, 23, None, ("generic", 0)),                      # 65 keys
    (dict(H=8), 0, 46, None, ("generic", 0)),                    # head_dim 16
    (dict(prec="f32"), 0, 46, None, ("generic", 0)),
    (dict(), 0, 46, "NO_BWD_IMAGE_RECOMPUTE", ("generic", 0)),
    (dict(), 0, 46, "BWD_RECOMPUTE_F32", ("generic", 0)),
    (dict(), 0, 46, "NO_BWD_ATTN_MFMA", (SAVE, 0)),              # the VALU attention backward reads K | V of every row
])
def test_which_kernel_recomputes_a_d128_chunk(lib, model, t0, nt, flag, expect):
    from aline_amd import _lib
    with _lib.debug(*([flag] if flag else [])):
        assert _name(_x1(**model), _rollout(), t0, nt) == expect
