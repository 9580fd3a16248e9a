"""GPU: the forward recompute of the training backward on the long-key layout -- `x3::layer_save_long_kernel` behind
`keys_long_kernel` / `kv_*_long_kernel` for chunks of 65 - 160 keys (x3_host.h: recompute), and Q from the layer kernel wherever a
matrix-pipe attention backward follows (49 - 160 keys: `abwl`)."""
import ctypes

import pytest
import torch

from test_attn_bwd_long_gpu import _model, _rollout_and_grads
from test_backward_gpu import _explain_with_gate_flips, _oracle_gradients_with_gate_flips
from test_s3_gpu import make_batch

pytestmark = pytest.mark.gpu


def _chunk_kernels(ro, T, tc):      # (kernel, Q from it) of every chunk of the backward, as the library reports them
    from aline_amd import _lib
    out, buf = [], ctypes.create_string_buffer(64)
    for t0 in range(0, T, tc or T):
        rc = _lib.lib.aline_backward_recompute_name(ctypes.byref(ro.m), ctypes.byref(ro.r), t0, min(tc or T, T - t0), buf, 64)
        out.append((buf.value.decode(), rc))
    return out


SHORT, LONG = ("x3::layer_save_kernel", 1), ("x3::layer_save_long_kernel", 1)


@pytest.mark.parametrize("emb,n_td,T,B,nq,hide,tc,kernels", [
    ("theta", 0, 70, 2, 90, False, 45, [SHORT, LONG]),     # 3 - 47 keys on the short kernel, then 48 - 72 on the long strides inside the larger plan: 1 - 5 tiles, the sixth empty
    ("data", 70, 5, 3, 20, False, None, [LONG]),           # 71 - 75 keys: 5 tiles, the second half of the last V^T k-step zero
    ("mix", 100, 6, 2, 30, False, None, [LONG]),           # 104 - 109 keys, 8 tiles (7 live); context / target rows see <= 6 keys
    ("mix", 100, 6, 2, 30, True, None, [LONG]),            # every second target hidden: key list not contiguous, K | V gathered / scattered by list
    ("mix", 141, 16, 2, 32, False, None, [LONG]),          # 145 - 160 keys: 10 tiles, three groups, the last admissible key
    ("theta", 0, 60, 2, 64, False, None, [SHORT]),         # 3 - 62 keys: Q from the short kernel at 49 - 64 keys, abwl <2, 2> behind it
    # 149 - 158 keys on three blocks inside a backward that ends at 168 keys (generic there).  (Not n_td = 141: at that seed the generic
    # REFERENCE is 9.6e-3 from the exact-fp32 recompute in one GMM head -- a knife-edge gate at B = 2 --, the new kernel 6e-5 from the exact one.)
    ("mix", 145, 20, 2, 32, False, 10, [LONG, ("generic", 0)]),
])
def test_long_key_recompute_matches_the_generic_recompute(emb, n_td, T, B, nq, hide, tc, kernels):
    """Every parameter gradient of one sampled rollout, by default and with the generic recompute (`ALINE_DBG_NO_BWD_IMAGE_RECOMPUTE`: four
    GEMMs, `attention_kernel<32>` and two LayerNorm kernels per layer, Q | K | V of every row).  The two recomputes round differently, so a
    knife-edge ReLU gate may flip: the bounds are those of test_image_recompute_and_key_row_products_match_the_generic_recompute (its
    docstring has the reasoning) -- nothing beyond 3e-3 of max |grad| (floor 1e-2 of the largest), four tensors in five within 2e-4."""
    from aline_amd import _lib
    model = _model(256, 256, 8, 2, emb)
    batch = make_batch(emb, B, nq, seed=T + n_td, n_td=n_td)
    if hide:
        batch["target_mask"] = (torch.arange(n_td + 3, device="cuda") % 2 == 0)
    ro, _, (new, ref) = _rollout_and_grads(model, batch, emb, T, ([], ["NO_BWD_IMAGE_RECOMPUTE"]), tc)
    assert _chunk_kernels(ro, T, tc) == kernels
    with _lib.debug("NO_BWD_IMAGE_RECOMPUTE"):
        assert _chunk_kernels(ro, T, tc) == [("generic", 0)] * len(kernels)
    floor = 1e-2 * max(float(g.abs().max()) for g in ref.values())
    assert all(torch.isfinite(v).all() for v in new.values())
    errs = {k: float((new[k] - ref[k]).abs().max()) / max(float(ref[k].abs().max()), floor) for k in ref}
    worst = max(errs.items(), key=lambda kv: kv[1])
    close = sum(e < 2e-4 for e in errs.values())
    print("worst", worst, "close", close, "of", len(errs))
    assert worst[1] < 3e-3, worst
    assert close >= 0.8 * len(errs), (close, len(errs), sorted(errs.items(), key=lambda kv: -kv[1])[:6])


def test_long_key_recompute_against_the_fp64_oracle():
    """d = 256 / F = 64 / L = 1, mix, 107 - 111 keys: gradients against fp64 autograd of the CPU oracle on the same designs and upstream
    gradients, with the knife-edge ReLU arbitration (at most 64 gates) and the 2e-4 bound of
    test_backward_of_a_shape_the_valu_kernel_cannot_hold_against_the_fp64_oracle."""
    n_td, nq, T, H, B = 103, 24, 5, 8, 2
    model = _model(256, 64, H, 1, "mix")
    batch = make_batch("mix", B, nq, seed=ORACLE_SEED, n_td=n_td, n_ctx=1)
    ro, terms, (g,) = _rollout_and_grads(model, batch, "mix", T, ([],))
    assert _chunk_kernels(ro, T, None) == [LONG] and 1 + (T - 1) + n_td + 3 == 111
    g = {k: v.cpu().double() for k, v in g.items()}
    sd = {k: v.detach().cpu().double().requires_grad_(True) for k, v in model.state_dict().items()}
    cpu = {k: (v.cpu().double() if v.is_floating_point() else v.cpu()) for k, v in batch.items() if torch.is_tensor(v)}
    cfg = dict(embedding_type="mix", n_head=H, num_layers=1, num_components=10, std_min=1e-4, n_target_theta=3)
    g0, deltas, ref, n_gates = _oracle_gradients_with_gate_flips(sd, cpu, cfg, T, ro.idx.cpu(), "all", terms["g_logp"].cpu().double(),
                                                              terms["g_ll"].cpu().double(), eps=5e-6)
    assert float((ro.target_ll.cpu().double() - torch.stack(ref["target_ll"]).detach()).abs().max()) < 1e-4
    assert len(deltas) <= 64, (len(deltas), n_gates)
    res, _flips = _explain_with_gate_flips(torch.cat([g[k].reshape(-1) for k in sd]) - g0, deltas)
    floor = 1e-2 * float(g0.abs().max())
    sizes = [v.numel() for v in sd.values()]
    errs = [float(e.abs().max()) / max(float(r.abs().max()), floor) for e, r in zip(res.split(sizes), g0.split(sizes))]
    worst = max(zip(sd, errs), key=lambda kv: kv[1])
    print("worst", worst, "gates", len(deltas))
    assert worst[1] < 2e-4, (worst, len(deltas))


# 2 * 5 * 131 rows: 84 k hidden units of the layer, 84 k of the acquisition head, 0.68 M of the ten GMM heads; a pre-activation of O(1) spread
# lies within 5e-6 of zero about once in 1e5 units, so the oracle arbitrates about 8 gates at any seed (8 at this one), far inside the cap
ORACLE_SEED = 4
