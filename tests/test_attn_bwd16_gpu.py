"""GPU: `abw16::attention_bwd16_kernel<NKT>` (attn_bwd16.h) -- the attention backward of the models with heads of 16 channels (d = 64 / 4
heads, 128 / 8, 192 / 12) with 1 - 160 keys on the f16 matrix pipe: two waves per head, heads in rounds of four, the row side streamed."""
import pytest
import torch

from test_attn_bwd_long_gpu import _model, _rollout_and_grads
from test_backward_gpu import _explain_with_gate_flips, _oracle_gradients_with_gate_flips
from test_s3_gpu import make_batch, n_theta_of

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("d,F,H,emb,n_td,T,B,nq,hide,tc", [
    (64, 64, 4, "theta", 0, 60, 2, 64, False, None),       # 3 - 62 keys in one chunk: <4>, instances of 1 - 4 tiles, last tile partial
    (64, 64, 4, "theta", 0, 60, 2, 64, False, 45),         # the same with a chunk boundary
    (64, 64, 4, "mix", 70, 5, 3, 20, False, None),         # 74 - 78 keys: <7> with 5 tiles
    (64, 64, 4, "mix", 70, 5, 3, 20, True, None),          # every second target hidden: key list not contiguous, queries see more keys
    (128, 64, 8, "mix", 70, 5, 2, 20, False, None),        # two rounds of heads
    (192, 64, 12, "mix", 70, 5, 2, 20, False, None),       # three rounds of heads
    (64, 64, 4, "mix", 90, 4, 3, 21, False, None),         # N = 115 rows: ragged last row tile, the first wave of a pair has one tile more
    (64, 64, 4, "mix", 150, 7, 2, 170, False, None),       # 160 keys: <10>, ten full tiles, the last admissible key; N = 324
])
def test_attention_backward_at_head_dim_16_matches_the_valu_kernel(d, F, H, emb, n_td, T, B, nq, hide, tc):
    """Every parameter gradient of one rollout, by default and with the fp32 VALU `attention_bwd_kernel<16>` (`ALINE_DBG_NO_BWD_ATTN_MFMA`),
    which launches at these shapes: same recomputed activations, so no ReLU gate differs; the scaled f16 split is held to 2e-4 of the
    reference tensor's max |grad| (floor 1e-2 of the largest), as at head_dim 32 / 64."""
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


@pytest.mark.parametrize("emb,nq,n_td,T,seed,keys,rows", [
    ("theta", 1200, 0, 3, 4, 5, 1203),       # 3 - 5 keys, N = 1203: the VALU kernel needs 144 * 1203 = 173 232 bytes for the rows alone
    ("mix", 900, 150, 7, 4, 160, 1054),      # 160 keys, N = 1054: 132 * 160 + 144 * 1054 = 172 896 bytes
])
def test_backward_at_head_dim_16_beyond_the_valu_kernel_against_the_fp64_oracle(emb, nq, n_td, T, seed, keys, rows):
    """d = 64 / 4 heads at shapes whose backward used to end with "unsupported".  Gradients against fp64 autograd of the CPU oracle on
    the same designs and upstream gradients, with the knife-edge ReLU arbitration and the 2e-4 bound of the head_dim-32 / 64 tests."""
    H, B = 4, 2
    model = _model(64, 64, H, 1, emb)
    batch = make_batch(emb, B, nq, seed=seed, n_td=n_td, n_ctx=1)
    ro, terms, (g,) = _rollout_and_grads(model, batch, emb, T, ([],))
    assert ro.P + ro.n_t == rows and 1 + (T - 1) + n_td + n_theta_of(emb, 2) == keys
    g = {k: v.cpu().double() for k, v in g.items()}
    sd = {k: v.detach().cpu().double().requires_grad_(True) for k, v in model.state_dict().items()}
    cpu = {k: (v.cpu().double() if v.is_floating_point() else v.cpu()) for k, v in batch.items() if torch.is_tensor(v)}
    cfg = dict(embedding_type=emb, n_head=H, num_layers=1, num_components=10, std_min=1e-4, n_target_theta=n_theta_of(emb, 2))
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
