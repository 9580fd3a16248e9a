"""Long-key variants of the x3 path (x3_impl.h, KV_EP / attention_long: d = 256 rollouts that show an episode 65 .. 160 keys) against
the exact-fp32 pipeline of the same C ABI on the same weights and forced designs, at the reference-precision bounds of
test_x5_gpu.py::test_tile_image_paths_in_mix_and_data_mode."""
import pytest
import torch

from helpers import native_model
from test_s3_gpu import make_batch, n_theta_of
from test_x3_gpu import DIMS, LL_TOL, LP_TOL

pytestmark = pytest.mark.gpu

B = 3


def _dims(emb):
    return dict(DIMS, F=256, L=2, dim_x=2, n_theta=n_theta_of(emb, 2), embedding_type=emb)


def _forced(n_query, T, nb):
    g = torch.Generator(device="cpu").manual_seed(5)
    return torch.stack([torch.stack([torch.randint(0, n_query - t, (1,), generator=g)[0] for t in range(T)]) for _ in range(nb)]).to("cuda")


@pytest.mark.parametrize("emb,n_td,n_query,T,every_second,postq", [
    ("theta", 0, 90, 70, False, False),      # 3 .. 72 keys: crosses 64 inside the rollout, 1 .. 5 key tiles on the long strides, an empty sixth tile
    ("data", 70, 40, 5, False, False),       # 71 .. 75 keys: odd tile count, the second half of the last V^T k-step zero
    ("mix", 100, 40, 6, False, False),       # 104 .. 109 keys: 8 tiles, a partial one; context / target rows see <= 6 keys
    ("mix", 130, 60, 20, False, True),       # 134 .. 153 keys: 10 tiles, three groups (cfg3-like); posterior_out_query too
    ("mix", 100, 40, 6, True, False),        # every second target hidden: the key list is not contiguous in the row order
    ("mix", 141, 30, 16, False, False),      # 145 .. 160 keys: the last admissible key
])
def test_long_key_rollout_matches_fp32_pipeline(emb, n_td, n_query, T, every_second, postq):
    from aline_amd.rollout import Rollout
    out = {}
    for prec in ("f16x3", "f32"):
        model, _ = native_model(_dims(emb), 11, prec)
        batch = make_batch(emb, B, n_query, 5, n_td=n_td)
        if every_second:
            batch["target_mask"] = (torch.arange(n_td + n_theta_of(emb, 2), device="cuda") % 2 == 0)
        ro = Rollout(model, batch, T, select="forced", forced_idx=_forced(n_query, T, B), keep_query_posterior=postq)
        if prec == "f16x3":
            assert ro.path == "x3::layer_kernel" and ro.kernel_name == "x3::layer_long_kernel<true>", (ro.path, ro.kernel_name)
        ro.run()
        torch.cuda.synchronize()
        out[prec] = {k: getattr(ro, k).float().cpu().clone() for k in ("target_ll", "log_prob", "post_std")}
        if postq:
            role = ro.role.cpu()         # slot p is a candidate at step t unless it entered the context before it (role = order of entry)
            out[prec]["cand"] = torch.stack([~((role > 0) & (role <= ro.n_c0 + t)) for t in range(T)])
            out[prec].update({k: getattr(ro, k).float().cpu().clone() for k in ("postq_mean", "postq_std", "postq_weight")})
    x, f = out["f16x3"], out["f32"]
    assert torch.isfinite(x["target_ll"]).all() and torch.isfinite(x["log_prob"]).all()
    d_ll = (x["target_ll"] - f["target_ll"]).abs()
    well = f["post_std"].min(-1).values >= 1e-2      # (a sharper component amplifies 1e-6 of its mean beyond any fixed bound: NLL bound only)
    d_nll = (x["target_ll"].mean(-1) - f["target_ll"].mean(-1)).abs().max()
    d_lp = (x["log_prob"] - f["log_prob"]).abs().max()
    print(f"single-target ll {float((d_ll * well).max()):.2e}  episode mean ll {float(d_nll):.2e}  log_prob {float(d_lp):.2e}")
    assert (d_ll * well).max() < 3e-4, float((d_ll * well).max())
    assert d_nll < LL_TOL, float(d_nll)
    assert d_lp < LP_TOL, float(d_lp)
    if postq:
        cand = x["cand"]
        assert (cand == f["cand"]).all()
        m = cand[..., None].float()
        assert torch.isfinite(x["postq_mean"][cand]).all() and (x["postq_std"][cand] > 0).all()
        assert ((x["postq_mean"] - f["postq_mean"]).abs() * m).max() < 2e-4
        assert ((x["postq_weight"] - f["postq_weight"]).abs() * m).max() < 1e-4
        assert (((x["postq_std"] - f["postq_std"]).abs() / f["postq_std"]) * m).max() < 1e-3


def test_training_gradients_do_not_depend_on_the_rollout_path():
    """The per-op backward of a > 64-key rollout reads nothing the x3 rollout wrote, but shares its workspace plan: the gradients of a
    training step with the rollout on the long-key path against the same step with the rollout on the generic pipeline
    (ALINE_DISABLE_X3), at test_backward_gpu.py's bounds between two fp32-grade evaluations of one backward."""
    from aline_amd import _lib
    from aline_amd.train import train_step
    nb, T, n_query = 4, 4, 40
    grads = []
    for env, path in (({}, "x3::layer_kernel"), ({"ALINE_DISABLE_X3": "1"}, "generic pipeline")):
        with _lib.debug_env(env):
            model, _ = native_model(_dims("mix"), 11, "f16x3")
            batch = make_batch("mix", nb, n_query, 5, n_td=100)
            _, ro = train_step(model, batch, T, embedding_type="mix", forced_idx=_forced(n_query, T, nb), clip_grads=False)
            torch.cuda.synchronize()
            assert ro.path == path, ro.path
        grads.append({k: p.grad.clone() for k, p in model.named_parameters()})
    new, ref = grads
    floor = 1e-2 * max(float(g.abs().max()) for g in ref.values())
    errs = {k: float((new[k] - ref[k]).abs().max()) / max(float(ref[k].abs().max()), floor) for k in ref}
    assert all(torch.isfinite(g).all() for g in new.values())
    worst = max(errs.items(), key=lambda kv: kv[1])
    assert worst[1] < 3e-3, worst
    close = sum(e < 2e-4 for e in errs.values())
    assert close >= 0.8 * len(errs), (close, len(errs), sorted(errs.items(), key=lambda kv: -kv[1])[:6])
