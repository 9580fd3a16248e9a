"""GPU: `abwl64::attention_bwd_long64_kernel<TPW, G>` (attn_bwd_long64.h) -- the attention backward of the head_dim-64 models (d = 128 / 2
heads, d = 192 / 3, d = 512 / 8) with 49 - 160 keys on the f16 matrix pipe: at most two key tiles per wave, operands streamed from split
row images."""
import pytest
import torch

from test_attn_bwd_long_gpu import _model, _rollout_and_grads
from test_backward_gpu import _explain_with_gate_flips, _oracle_gradients_with_gate_flips
from test_s3_gpu import make_batch

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("d,F,H,emb,n_td,T,B,nq,hide,tc", [
    (128, 64, 2, "theta", 0, 60, 2, 64, False, None),      # 3 - 62 keys in one chunk: <1, 4>, last tile partial, instances of 1 - 4 tiles
    (128, 64, 2, "theta", 0, 60, 2, 64, False, 45),        # chunk of <= 47 keys on abww <64, 3>, chunk of 48 - 62 keys on the new kernel
    (128, 64, 2, "mix", 70, 5, 3, 20, False, None),        # 74 - 78 keys: <2, 4>, 5 tiles, only wave 0 of a group owns two
    (128, 64, 2, "mix", 70, 5, 3, 20, True, None),         # every second target hidden: key list not contiguous, queries see more keys
    (192, 64, 3, "mix", 70, 5, 2, 20, False, None),        # 3 heads, two per round: the second group idles in the last round
    (512, 128, 8, "theta", 0, 60, 2, 64, False, 45),       # x5 rollout, x5::layer_save_kernel recompute, Q / K / V of every row from the GEMM
    (128, 64, 2, "mix", 90, 4, 3, 21, False, None),        # N = 115 rows: ragged last row tile; 94 - 97 keys: <2, 4> with 7 of 8 tiles
])
def test_long_key_attention_backward_at_head_dim_64_matches_the_valu_kernel(d, F, H, emb, n_td, T, B, nq, hide, tc):
    """Every parameter gradient of one rollout, by default and with the fp32 VALU `attention_bwd_kernel<64>` (`ALINE_DBG_NO_BWD_ATTN_MFMA`),
    which still launches at these shapes (1028 * keys + 528 * N <= 162 816): same recomputed activations, so no ReLU gate differs; the
    scaled f16 split is held to 2e-4 of the reference tensor's max |grad| (floor 1e-2 of the largest), as at head_dim 32."""
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


@pytest.mark.parametrize("nq,n_td,T,keys,rows", [
    (24, 120, 5, 128, 148),       # 124 - 128 keys: <2, 4>, 8 full tiles (the VALU kernel: 128 * 1028 + 148 * 528 = 209 728 bytes)
    (170, 150, 7, 160, 324),      # 160 keys: <2, 8>, 10 tiles over waves of 2 / 2 / 1 .. 1, the last admissible key
])
def test_backward_at_head_dim_64_beyond_the_valu_kernel_against_the_fp64_oracle(nq, n_td, T, keys, rows):
    """d = 128 / 2 heads at shapes whose backward used to end with "unsupported".  Gradients against fp64 autograd of the CPU oracle on
    the same designs and upstream gradients, with the knife-edge ReLU arbitration and the 2e-4 bound of the head_dim-32 test."""
    H, B = 2, 2
    model = _model(128, 64, H, 1, "mix")
    batch = make_batch("mix", B, nq, seed=4, n_td=n_td, n_ctx=1)
    ro, terms, (g,) = _rollout_and_grads(model, batch, "mix", T, ([],))
    assert ro.P + ro.n_t == rows and 1 + (T - 1) + n_td + 3 == keys
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
