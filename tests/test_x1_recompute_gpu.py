"""GPU: the forward recompute of the training backward at d = 128 / 4 heads of 32 on `x1::layer_save_kernel` (x1_layer.h) -- the x1 layer
kernel, two token tiles per wave, over the (step, episode) instances of a chunk, with the fp32 rows the per-op backward reads."""
import pytest
import torch

from test_attn_bwd_long_gpu import _model, _rollout_and_grads
from test_backward_gpu import _explain_with_gate_flips, _oracle_gradients_with_gate_flips
from test_recompute_longkeys_gpu import _chunk_kernels
from test_s3_gpu import make_batch

pytestmark = pytest.mark.gpu

SAVE = ("x1::layer_save_kernel", 1)


def _cus():      # (read when the test runs, not at collection)
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.mark.parametrize("emb,F,L,n_td,T,B,nq,hide,tc", [
    ("theta", 256, 2, 0, 6, 3, 200, False, None),     # N = 203: 13 tiles per instance, the lone last tile, whose partner must store nothing
    ("theta", 256, 2, 0, 4, 5, 37, False, None),      # N = 40: partial last tile, 3 tiles per instance, odd tile total
    ("theta", 256, 2, 0, 3, 2, 16, False, None),      # 6 units: waves without a unit (not B = 1: rewards z-scored over the batch are NaN there)
    ("theta", 256, 2, 0, 62, 2, 90, False, 31),       # 3 - 64 keys over two chunks: 1, 2 and 4 key tiles, abwl behind Q at 49 - 64, the last admissible key
    ("mix", 256, 2, 40, 5, 2, 30, False, None),       # 44 - 48 keys for query rows, <= 5 for context / target rows
    ("mix", 256, 2, 40, 5, 2, 30, True, None),        # every second target hidden: key list not contiguous, K | V gathered / scattered by list
    ("data", 256, 2, 30, 5, 3, 20, False, None),      # data embedding mode: no theta tokens
    ("theta", 32, 2, 0, 4, 2, 20, False, None),       # one FFN chunk: Hid stored once per layer
    ("theta", 96, 1, 0, 4, 2, 20, False, None),       # odd number of hidden groups
    ("theta", 256, 1, 0, 8, lambda: _cus() + 3, 16, False, None),      # N = 19, one unit per instance: 8 x CUs (a full persistent round) + 24 (a tail)
])
def test_d128_recompute_matches_the_generic_recompute(emb, F, L, n_td, T, B, nq, hide, tc):
    """Every parameter gradient of one sampled rollout, by default and with the generic recompute (`ALINE_DBG_NO_BWD_IMAGE_RECOMPUTE`: four
    GEMMs, `attention_kernel<32>` and two LayerNorm kernels per layer, Q | K | V of every row).  The two recomputes round differently, so a
    knife-edge ReLU gate may flip: the bounds are those of test_long_key_recompute_matches_the_generic_recompute -- nothing beyond 3e-3 of
    max |grad| (floor 1e-2 of the largest), four tensors in five within 2e-4."""
    from aline_amd import _lib
    B = B() if callable(B) else B
    model = _model(128, F, 4, L, emb)
    batch = make_batch(emb, B, nq, seed=T + n_td, n_td=n_td)
    if hide:
        batch["target_mask"] = (torch.arange(n_td + 3, device="cuda") % 2 == 0)
    ro, _, (new, ref) = _rollout_and_grads(model, batch, emb, T, ([], ["NO_BWD_IMAGE_RECOMPUTE"]), tc)
    nchunks = len(range(0, T, tc or T))
    assert _chunk_kernels(ro, T, tc) == [SAVE] * nchunks
    with _lib.debug("NO_BWD_IMAGE_RECOMPUTE"):
        assert _chunk_kernels(ro, T, tc) == [("generic", 0)] * nchunks
    floor = 1e-2 * max(float(g.abs().max()) for g in ref.values())
    assert all(torch.isfinite(v).all() for v in new.values())
    errs = {k: float((new[k] - ref[k]).abs().max()) / max(float(ref[k].abs().max()), floor) for k in ref}
    worst = max(errs.items(), key=lambda kv: kv[1])
    close = sum(e < 2e-4 for e in errs.values())
    print("worst", worst, "close", close, "of", len(errs))
    assert worst[1] < 3e-3, worst
    assert close >= 0.8 * len(errs), (close, len(errs), sorted(errs.items(), key=lambda kv: -kv[1])[:6])


def test_d128_recompute_against_the_fp64_oracle():
    """d = 128 / F = 64 / L = 1, mix, 44 - 48 keys: gradients against fp64 autograd of the CPU oracle on the same designs and upstream
    gradients, with the knife-edge ReLU arbitration (at most 64 gates) and the 2e-4 bound of
    test_long_key_recompute_against_the_fp64_oracle."""
    n_td, nq, T, H, B = 40, 24, 5, 4, 2
    model = _model(128, 64, H, 1, "mix")
    batch = make_batch("mix", B, nq, seed=ORACLE_SEED, n_td=n_td, n_ctx=1)
    ro, terms, (g,) = _rollout_and_grads(model, batch, "mix", T, ([],))
    assert _chunk_kernels(ro, T, None) == [SAVE] and 1 + (T - 1) + n_td + 3 == 48
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


# 2 * 5 * 68 rows: 44 k hidden units of the layer, 44 k of the acquisition head, 0.28 M of the ten GMM heads; a pre-activation of O(1) spread
# lies within 5e-6 of zero about once in 1e5 units, so the oracle arbitrates a handful of gates at any seed (1 at this one), far inside the cap
ORACLE_SEED = 4
