"""GPU: weight-gradient products with a dimension that is a multiple of 128 only on `gemm_tn_f16_narrow_kernel<128, 128>` (backward.h) -- every
encoder product of a d = 128 model, the 128-wide ones of d = 512 / F = 128 -- and `kv_sparse` (the in-projection's K | V products over the
key rows) at d = 128."""
import pytest
import torch

from test_attn_bwd_long_gpu import _rollout_and_grads
from test_backward_gpu import _explain_with_gate_flips, _oracle_gradients_with_gate_flips
from test_s3_gpu import make_batch

pytestmark = pytest.mark.gpu


def _model(d, F, H, emb, seed, jitter=0.02):
    from aline_amd import Aline, Embedder, Encoder, OutputHead
    torch.manual_seed(seed)
    model = Aline(Embedder(2, 1, d, F, 3 if emb == "mix" else 2, emb), Encoder(d, F, H, 0.0, 2), OutputHead(2, 1, d, F)).cuda()
    model = model.set_precision("f16x3").train()
    with torch.no_grad():
        for p in model.parameters():
            p.add_(jitter * torch.randn_like(p))
    return model


def _worst(new, ref):
    floor = 1e-2 * max(float(g.abs().max()) for g in ref.values())
    assert all(torch.isfinite(v).all() for v in new.values())
    errs = {k: float((new[k] - ref[k]).abs().max()) / max(float(ref[k].abs().max()), floor) for k in ref}
    worst = max(errs.items(), key=lambda kv: kv[1])
    print("worst", worst)
    return worst


def test_d128_backward_on_narrow_tiles_against_the_fp64_oracle():
    """d = 128 / F = 256 / 4 heads / 2 layers, 3 - 7 keys: every encoder product is narrow (128 x 128, 256 x 128 dense and over the key
    list, 128 x 256) and kv_sparse is on.  Against fp64 autograd of the CPU oracle on the same designs and upstream gradients, with the
    knife-edge ReLU arbitration and the 2e-4 bound of test_per_op_backward_of_wider_models_against_the_fp64_oracle."""
    H, T = 4, 5
    model = _model(128, 256, H, "theta", 21, jitter=0.0)
    batch = make_batch("theta", 6, 30, seed=21)
    ro, terms, (g,) = _rollout_and_grads(model, batch, "theta", T, ([],))
    g = {k: v.cpu().double() for k, v in g.items()}
    sd = {k: v.detach().cpu().double().requires_grad_(True) for k, v in model.state_dict().items()}
    cpu = {k: (v.cpu().double() if v.is_floating_point() else v.cpu()) for k, v in batch.items() if torch.is_tensor(v)}
    cfg = dict(embedding_type="theta", n_head=H, num_layers=2, num_components=10, std_min=1e-4, n_target_theta=2)
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


@pytest.mark.parametrize("d,F,H,emb,B,T,tc", [
    (128, 512, 4, "theta", 48, 5, 2),      # M = B T 63 is no multiple of 32, several row chunks per block, 1 - 4 blocks along either operand
    (128, 128, 4, "theta", 7, 3, None),    # every product a single 128 x 128 block
    (512, 128, 8, "theta", 20, 3, None),   # cfg5's widths: the 256 x 256 kernel and the narrow ones in one backward
    (128, 256, 4, "mix", 5, 4, None),      # 20 data targets: the GMM heads' first layers read a row-mapped X (Rx != Gx)
])
def test_narrow_f16_gradient_products_match_the_exact_fp32_products(d, F, H, emb, B, T, tc):
    """Against the exact-fp32 products (`ALINE_DBG_BWD_GRAD_F32`) of the same rollout, structure and 2e-4 bound of
    test_scaled_f16_gradient_products_match_the_exact_fp32_products."""
    from aline_amd import _lib
    from aline_amd.rollout import Rollout
    from aline_amd.train import backward, reinforce_terms
    model = _model(d, F, H, emb, 3)
    batch = make_batch(emb, B, 60, seed=3, n_td=20)
    grads = []
    with torch.no_grad():
        ro = Rollout(model, batch, T, select="sample").run()
        terms = reinforce_terms(ro, emb, "all")
        for flags in ([], ["BWD_GRAD_F32"]):
            with _lib.debug(*flags):
                for p in model.parameters():
                    p.grad = None
                backward(model, ro, terms["g_logp"], terms["g_ll"], t_chunk=tc if flags == [] else None)
                torch.cuda.synchronize()
            grads.append({k: p.grad.clone() for k, p in model.named_parameters()})
    worst = _worst(*grads)
    assert worst[1] < 2e-4, worst


@pytest.mark.parametrize("flag", ["NO_BWD_KV_SPARSE", "NO_BWD_DW_NARROW"])
def test_narrow_products_and_key_row_products_agree_with_their_switches(flag):
    """d = 128 / F = 256, T = 50 in chunks of 16 steps: chunks of <= 48 keys split the in-projection's products over the key list, later
    ones are dense, in one backward.  Default against the all-rows products and against the fp32 block kernel with the old kv_sparse
    rule: both sides read the same recomputed activations, so every tensor is held to 2e-4 of its max |grad|."""
    model = _model(128, 256, 4, "theta", 128 + 50)
    batch = make_batch("theta", 4, 60, seed=50)
    _, _, (new, ref) = _rollout_and_grads(model, batch, "theta", 50, ([], [flag]), 16)
    worst = _worst(new, ref)
    assert worst[1] < 2e-4, worst
