"""x1 path (aline_amd/csrc/x1.h): d_model = 128, 4 heads of 32, every product a 3-term f16 split on the matrix pipe, two token tiles per
wave.  Against the exact-fp32 pipeline of the same C ABI (precision "f32") on the same weights and forced designs, at the
reference-precision bounds of test_x3_gpu.py / test_x3_longkeys_gpu.py; shapes: the smallest at which this kernel can go wrong."""
import pytest
import torch

import aline_oracle as orc
from helpers import maxdiff, native_model, to_dev
from test_s3_gpu import make_batch, n_theta_of
from test_x3_gpu import LL_TOL, LP_TOL

pytestmark = pytest.mark.gpu

X1 = "x1::layer_kernel"
# Weight seed: chosen on the REFERENCE side.  With seed 11 (test_x3_gpu.py's) the d = 128 theta-mode heads put a component below std 1e-2 at
# every target (nothing left for the single-target bound); with seed 1 every case keeps >= 0.99 of its targets and the two existing
# pipelines (f32, generic f16x3) agree within single 1.1e-4 / episode mean 3.4e-5 / log_prob 8.6e-6 on these inputs.
WSEED = 1


def _dims(emb="theta", **kw):
    return dict({"dim_x": 2, "dim_y": 1, "d": 128, "F": 256, "n_head": 4, "L": 2, "C": 10, "n_theta": n_theta_of(emb, 2),
                 "embedding_type": emb, "time_token": False}, **kw)


def _forced(n_query, T, nb):
    g = torch.Generator(device="cpu").manual_seed(5)
    return torch.stack([torch.stack([torch.randint(0, n_query - t, (1,), generator=g)[0] for t in range(T)]) for _ in range(nb)]).to("cuda")


def _rollout(prec, dims, B, n_query, T, n_td=0, mask=None, postq=False, path=X1):
    from aline_amd.rollout import Rollout
    emb = dims["embedding_type"]
    model, _ = native_model(dims, WSEED, prec)
    batch = make_batch(emb, B, n_query, 5, n_td=n_td)
    if mask == "every_second":
        batch["target_mask"] = (torch.arange(n_td + dims["n_theta"], device="cuda") % 2 == 0)
    elif mask is not None:
        batch["target_mask"] = torch.tensor(mask, dtype=torch.bool, device="cuda")
    ro = Rollout(model, batch, T, select="forced", forced_idx=_forced(n_query, T, B), keep_query_posterior=postq)
    if prec == "f16x3":
        assert ro.path == path, ro.path
    ro.run()
    torch.cuda.synchronize()
    assert ro.range_status() == 0
    return ro


def _persistent_B():
    """More tile pairs than one round of the grid: B ceil(19 / 16) > 16 CUs."""
    return 8 * torch.cuda.get_device_properties(0).multi_processor_count + 1


@pytest.mark.parametrize("emb,B,n_query,T,n_td,mask,over,postq", [
    ("theta", 3, 200, 6, 0, None, {}, False),             # 13 tiles per episode: an odd count, a wave holds the episode's lone last tile
    ("theta", 5, 37, 4, 0, None, {}, False),              # partial tile, an odd number of tiles overall
    ("theta", 1, 16, 3, 0, None, {}, False),              # two tiles in the whole launch: seven waves without work
    ("theta", 2, 90, 62, 0, None, {}, False),             # 3 .. 64 keys: every key-tile count, the last admissible key
    ("theta", None, 16, 2, 0, None, {"L": 1}, False),     # persistent loop: a full round of the grid and a tail (N = 19)
    ("mix", 3, 37, 5, 40, None, {}, False),               # mix, all targets visible
    ("mix", 3, 37, 5, 40, "every_second", {}, False),     # every second target hidden: the key list is not contiguous
    ("data", 3, 37, 5, 30, None, {}, False),              # data embedding mode
    ("theta", 3, 70, 5, 0, [True, False], {}, False),
    ("theta", 3, 70, 5, 0, [False, False], {}, False),
    ("theta", 3, 37, 4, 0, None, {"F": 32}, False),       # one FFN chunk per layer, half a head chunk
    ("theta", 2, 40, 3, 0, None, {"F": 96, "C": 16, "L": 1}, False),      # an odd number of hidden groups: the head image's half chunk
    ("theta", 3, 37, 4, 0, None, {"time_token": True}, False),
    ("theta", 3, 37, 4, 0, None, {}, True),               # posterior_out_query on the candidate slots
])
def test_x1_matches_fp32_pipeline(emb, B, n_query, T, n_td, mask, over, postq):
    B = B or _persistent_B()
    dims = _dims(emb, **over)
    out = {}
    for prec in ("f16x3", "f32"):
        ro = _rollout(prec, dims, B, n_query, T, n_td, mask, postq)
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
    print(f"single-target ll {float((d_ll * well).max()):.2e}  episode mean ll {float(d_nll):.2e}  log_prob {float(d_lp):.2e}  "
          f"well-conditioned targets {float(well.float().mean()):.2f}")
    assert well.float().mean() > 0.3
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


def test_x1_is_reproducible():
    a, b = (_rollout("f16x3", _dims(), 9, 200, 6) for _ in range(2))
    assert torch.equal(a.target_ll, b.target_ll) and torch.equal(a.log_prob, b.log_prob)


def test_x1_against_the_cpu_oracle():
    """Fresh seeded inputs through oracle/aline_oracle.py, as test_hip_parity.py::test_oracle_cross_check_random_inputs, at its bounds."""
    from aline_amd.rollout import Rollout
    dims = dict(dim_x=3, dim_y=1, d=128, F=96, n_head=4, L=2, C=7, n_theta=3, embedding_type="mix", time_token=False)
    model, sd = native_model(dims, 99, "f16x3")
    g = torch.Generator().manual_seed(5)
    B, n_c, n_q, n_td, T = 5, 3, 37, 11, 6
    batch = dict(context_x=torch.randn(B, n_c, 3, generator=g), context_y=torch.randn(B, n_c, 1, generator=g),
                 query_x=torch.randn(B, n_q, 3, generator=g), query_y=torch.randn(B, n_q, 1, generator=g),
                 target_x=torch.randn(B, n_td, 3, generator=g), target_all=torch.randn(B, n_td + 3, 1, generator=g),
                 target_mask=torch.rand(n_td + 3, generator=g) > 0.5)
    cfg = dict(embedding_type="mix", n_head=4, num_layers=2, num_components=7, std_min=1e-4, n_target_theta=3)
    forced = torch.stack([torch.randint(0, n_q - t, (B,), generator=g) for t in range(T)], 1)
    ref = orc.rollout(sd, batch, cfg, T, forced_idx=forced, mask_type="partial")
    ro = Rollout(model, to_dev(batch), T, select="forced", forced_idx=forced, keep_zt=True)
    assert ro.path == X1
    ro.run()
    assert maxdiff(ro.target_ll, torch.stack(ref["target_ll"])) < 1e-4
    assert maxdiff(ro.log_prob, torch.stack(ref["log_prob"], 1)) < 1e-4


def test_training_gradients_do_not_depend_on_the_rollout_path():
    """The backward stays per-op: a training step with the rollout on x1 against the same step with the rollout on the generic pipeline
    (ALINE_DISABLE_X1), at test_x3_longkeys_gpu.py's bounds between two fp32-grade evaluations of one backward."""
    from aline_amd import _lib
    from aline_amd.train import train_step
    nb, T, n_query = 4, 4, 40
    grads = []
    for env, path in (({}, X1), ({"ALINE_DISABLE_X1": "1"}, "generic pipeline")):
        with _lib.debug_env(env):
            model, _ = native_model(_dims("mix"), 11, "f16x3")
            batch = make_batch("mix", nb, n_query, 5, n_td=40)
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
