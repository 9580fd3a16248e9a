"""GPU: `abwl::attention_bwd_long_kernel<TPW, G>` (attn_bwd_long.h) -- the attention backward of the head_dim-32 models (d = 128 / 4 heads,
d = 256 / 8 heads) with 49 - 160 keys on the f16 matrix pipe, a head's key tiles split over a group of waves."""
import pytest
import torch

from test_backward_gpu import _explain_with_gate_flips, _oracle_gradients_with_gate_flips
from test_s3_gpu import make_batch, n_theta_of

pytestmark = pytest.mark.gpu


def _model(d, F, H, L, emb):
    from aline_amd import Aline, Embedder, Encoder, OutputHead
    torch.manual_seed(d + H)
    model = Aline(Embedder(2, 1, d, F, n_theta_of(emb, 2), emb), Encoder(d, F, H, 0.0, L), OutputHead(2, 1, d, F)).cuda()
    return model.set_precision("f16x3").train()


def _rollout_and_grads(model, batch, emb, T, flag_sets, t_chunk=None):
    from aline_amd import _lib
    from aline_amd.rollout import Rollout
    from aline_amd.train import backward, reinforce_terms
    grads = []
    with torch.no_grad():
        ro = Rollout(model, batch, T, select="sample").run()
        terms = reinforce_terms(ro, emb, "all")
        for flags in flag_sets:
            with _lib.debug(*flags):
                for p in model.parameters():
                    p.grad = None
                backward(model, ro, terms["g_logp"], terms["g_ll"], t_chunk=t_chunk)
                torch.cuda.synchronize()
            grads.append({k: p.grad.clone() for k, p in model.named_parameters()})
    return ro, terms, grads


@pytest.mark.parametrize("d,F,H,emb,n_td,T,B,nq,hide,tc", [
    (256, 256, 8, "theta", 0, 60, 2, 64, False, None),     # 3 - 62 keys in one chunk: <2, 2>, last tile partial, instances of 1 - 4 tiles
    (256, 256, 8, "theta", 0, 60, 2, 64, False, 45),       # chunk of <= 47 keys on abww <32, 3>, chunk of 48 - 62 keys on the new kernel
    (128, 192, 4, "mix", 70, 5, 3, 20, False, None),       # 74 - 78 keys: <3, 2>, 5 tiles, the second wave's third tile empty
    (256, 256, 8, "mix", 100, 6, 2, 30, True, None),       # every second target hidden: key list not contiguous, queries see more keys
    (128, 192, 4, "mix", 120, 5, 2, 24, False, None),      # 124 - 128 keys: <2, 4>, exactly 8 full tiles
    (256, 256, 8, "mix", 141, 16, 2, 32, False, None),     # 145 - 160 keys: <3, 4>, 10 tiles over waves of 3 / 3 / 2 / 2, the last admissible key
    (128, 192, 4, "mix", 90, 4, 4, 21, False, None),       # N = 1 + 21 + 93 = 115 rows: ragged last row tile; 94 - 97 keys: <2, 4> with 7 of 8 tiles
])
def test_long_key_attention_backward_matches_the_valu_kernel(d, F, H, emb, n_td, T, B, nq, hide, tc):
    """Every parameter gradient of one rollout, by default and with the fp32 VALU `attention_bwd_kernel<32>` (`ALINE_DBG_NO_BWD_ATTN_MFMA`):
    both read the same recomputed activations, so no ReLU gate differs, and the scaled f16 split is held to the bound of
    test_scaled_f16_gradient_products_match_the_exact_fp32_products: 2e-4 of the reference tensor's max |grad| (floor 1e-2 of the largest)."""
    model = _model(d, F, H, 2, emb)
    batch = make_batch(emb, B, nq, seed=T + n_td, n_td=n_td)
    if hide:
        batch["target_mask"] = (torch.arange(n_td + 3, device="cuda") % 2 == 0)
    _, _, (new, ref) = _rollout_and_grads(model, batch, emb, T, ([], ["NO_BWD_ATTN_MFMA"]), tc)
    floor = 1e-2 * max(float(g.abs().max()) for g in ref.values())
    errs = {}
    for k in ref:
        assert torch.isfinite(new[k]).all(), k
        errs[k] = float((new[k] - ref[k]).abs().max()) / max(float(ref[k].abs().max()), floor)
    worst = max(errs.items(), key=lambda kv: kv[1])
    print("worst", worst)
    assert worst[1] < 2e-4, worst


@pytest.mark.parametrize("B", [2])
def test_backward_of_a_shape_the_valu_kernel_cannot_hold_against_the_fp64_oracle(B):
    """d = 128 / 4 heads, 160 keys, N = 324 rows: the VALU kernel's LDS would be 160 * 516 + 324 * 272 = 170 688 bytes > 162 816 (the
    backward of this shape used to end with "unsupported").  Gradients against fp64 autograd of the CPU oracle on the same designs and
    upstream gradients, with the knife-edge ReLU arbitration and the 2e-4 bound of test_per_op_backward_of_wider_models_against_the_fp64_oracle."""
    n_td, nq, T, H = 150, 170, 7, 4
    model = _model(128, 64, H, 1, "mix")
    batch = make_batch("mix", B, nq, seed=4, n_td=n_td, n_ctx=1)
    ro, terms, (g,) = _rollout_and_grads(model, batch, "mix", T, ([],))
    assert ro.P + ro.n_t == 324 and 1 + (T - 1) + n_td + 3 == 160
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
    worst, off = ("", 0.0), 0
    for k, v in sd.items():
        n = v.numel()
        err = float(res[off:off + n].abs().max()) / max(float(g0[off:off + n].abs().max()), floor)
        if err > worst[1]:
            worst = (k, err)
        off += n
    print("worst", worst, "gates", len(deltas))
    assert worst[1] < 2e-4, (worst, len(deltas))
