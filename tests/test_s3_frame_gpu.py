"""The launches around the s3 step loop (aline_amd/csrc/s3.h): setup_kernel (range flag, roles, selection arguments in one launch),
pack_kernel's embedder images, embed_kernel (Ex / Ey rows AND the X0 image of step 0 from the same registers) and the double-buffered
gmm_kernel<F, GT>.  Everything runs through the C ABI on the s3 path and is held against the CPU oracle with the bounds of
tests/test_hip_parity.py: target_ll 1e-4, log_prob 1e-4, zt / GMM parameters 5e-5 (d = 32).  The embedder has no output of its own
on this path: its rows are checked through step 0 (the X0 image it wrote) and steps 1, 2 (rows patched from its Ex + Ey)."""
import pytest
import torch

import aline_oracle as orc
from helpers import maxdiff, native_model, to_dev

pytestmark = pytest.mark.gpu

LL_TOL, LP_TOL, P_TOL = 1e-4, 1e-4, 5e-5


def _dims(emb, dx=2, F=128, C=10, L=2, n_theta=None, time_token=False):
    n_th = n_theta if n_theta is not None else {"theta": 2, "mix": dx + 1, "data": 0}[emb]
    return {"dim_x": dx, "dim_y": 1, "d": 32, "F": F, "n_head": 4, "L": L, "C": C, "n_theta": n_th, "embedding_type": emb,
            "time_token": time_token}


def _cfg(dims):
    return dict(embedding_type=dims["embedding_type"], n_head=4, num_layers=dims["L"], num_components=dims["C"], std_min=1e-4,
                n_target_theta=dims["n_theta"], time_token=dims["time_token"])


def _batch(dims, B, n_c, n_q, n_td=0, seed=0):
    g = torch.Generator().manual_seed(seed)
    dx = dims["dim_x"]
    b = dict(context_x=torch.rand(B, n_c, dx, generator=g), context_y=torch.randn(B, n_c, 1, generator=g),
             query_x=torch.rand(B, n_q, dx, generator=g), query_y=torch.randn(B, n_q, 1, generator=g),
             target_all=torch.rand(B, n_td + dims["n_theta"], 1, generator=g))
    if n_td:
        b["target_x"] = torch.rand(B, n_td, dx, generator=g)
    return b


def _forced(B, n_q, T, seed=1):
    g = torch.Generator().manual_seed(seed)
    return torch.stack([torch.randint(0, n_q - t, (B,), generator=g) for t in range(T)], 1)


def _against_oracle(dims, batch, T, wseed=3, **debug):
    """Teacher-forced rollout on the s3 path vs the oracle: log-likelihoods, log-probabilities, design distributions, GMM parameters."""
    from aline_amd import _lib
    from aline_amd.rollout import Rollout
    model, sd = native_model(dims, wseed, "f16x3")
    B, n_q = batch["query_x"].shape[:2]
    forced = _forced(B, n_q, T)
    ref = orc.rollout(sd, batch, _cfg(dims), T, forced_idx=forced)
    with _lib.debug(**debug):
        ro = Rollout(model, to_dev(batch), T, select="forced", forced_idx=forced.cuda(), keep_zt=True,
                     time_token_T=T if dims["time_token"] else 0)
        assert ro.path == "s3::step_kernel", ro.path
        ro.run()
        torch.cuda.synchronize()
    assert ro.range_status() == 0
    figs = {"target_ll": maxdiff(ro.target_ll, torch.stack(ref["target_ll"])),
            "log_prob": maxdiff(ro.log_prob, torch.stack(ref["log_prob"], 1)),
            "mean": maxdiff(ro.post_mean, torch.stack(ref["means"]).reshape(ro.post_mean.shape)),
            "std": maxdiff(ro.post_std, torch.stack(ref["stds"]).reshape(ro.post_std.shape)),
            "weight": maxdiff(ro.post_weight, torch.stack(ref["weights"]).reshape(ro.post_weight.shape)),
            "zt": max(maxdiff(ro.zt[t, :, :ref["zt"][t].shape[1]], ref["zt"][t]) for t in range(T))}
    print(figs)
    assert figs["target_ll"] < LL_TOL and figs["log_prob"] < LP_TOL, figs
    assert max(figs["mean"], figs["std"], figs["weight"], figs["zt"]) < P_TOL, figs
    return ro


@pytest.mark.parametrize("emb,n_c,n_q,n_td,F", [
    ("theta", 2, 15, 0, 128),      # P = 17: two point tiles, the second with one valid row; the context rows in the first only
    ("theta", 2, 15, 0, 32),
    ("theta", 2, 14, 0, 128),      # P = 16 exactly: the theta tokens open the second tile
    ("mix", 2, 15, 9, 128),        # target-data rows: the x-embedder covers P + n_td rows (tiles that straddle episodes), the y-embedder P
    ("data", 3, 18, 13, 32),       # no theta tokens: the kernel's tail writes zero rows only
])
def test_embedder_writes_rows_and_the_x0_image(emb, n_c, n_q, n_td, F):
    """Teacher-forced T = 3: step 0 reads the X0 image the embedder wrote (Ex, Ex + Ey on the initial context rows, theta tokens, zero
    padding); steps 1 and 2 read rows patched from its fp32 Ex / Ey rows."""
    dims = _dims(emb, F=F)
    _against_oracle(dims, _batch(dims, 3, n_c, n_q, n_td), 3)


@pytest.mark.parametrize("C", [1, 2, 10])
def test_gmm_component_counts(C):
    """C = 1: no prefetch at all; C = 2: one prefetch, both buffers; C = 10: the buffers alternate five times."""
    dims = _dims("theta", C=C)
    _against_oracle(dims, _batch(dims, 3, 1, 12), 2)


@pytest.mark.parametrize("gt", [1, 2])
@pytest.mark.parametrize("B", [1, 513])
def test_gmm_row_counts_in_both_instantiations(B, gt):
    """M = T * B * n_t target rows with T = 1 and one theta token: M = 1 (a single row of a single tile), and M = 513 = one past four
    workgroups of 128 rows (GT = 1) and one past two workgroups of 256 rows (GT = 2)."""
    dims = _dims("theta", n_theta=1, L=1)
    _against_oracle(dims, _batch(dims, B, 1, 5), 1, S3_GMM_GT=gt)


def test_flag_clear_precedes_every_raiser_on_a_reused_workspace():
    """A first rollout raises the f16 range flag (a weight beyond f16 after the 2^8 pre-scale: pack_kernel raises it); the second, clean
    rollout on the same workspace must report 0 -- the clear in setup_kernel is ordered before pack_kernel and everything behind it."""
    from aline_amd.rollout import Rollout
    dims = _dims("theta")
    model, _ = native_model(dims, 7, "f16x3")
    batch = _batch(dims, 4, 1, 20)
    ro = Rollout(model, to_dev(batch), 3, select="argmax")
    assert ro.path == "s3::step_kernel"
    w = dict(model.named_parameters())["encoder.encoder.layers.1.linear1.weight"]
    with torch.no_grad():
        w.mul_(512.0)          # (a power of two: undone exactly below)
    ro.run()
    assert ro.range_status() & 2
    with torch.no_grad():
        w.mul_(1.0 / 512.0)
    ro.run()
    assert ro.range_status() == 0
    with torch.no_grad():
        dict(model.named_parameters())["embedder.x_embedder.2.weight"].mul_(2.0 ** 19)      # layer-0 input rows beyond 65504: the embedder raises
    ro.run()
    assert ro.range_status() & 1
    with torch.no_grad():
        dict(model.named_parameters())["embedder.x_embedder.2.weight"].mul_(2.0 ** -19)
    ro.run()
    assert ro.range_status() == 0


def test_sampled_rollout_with_time_token_matches_the_oracle_on_the_same_uniforms():
    """select = "sample", T = 3, time token on: the roles and the selection arguments of setup_kernel take effect before step 0.  The
    oracle is teacher-forced with the sampled designs; the designs themselves are the inverse CDF of the oracle's distribution at the
    rollout's uniforms (compared where the uniform is not within 1e-4 of a CDF step), slots and roles follow from the designs."""
    from aline_amd.rollout import Rollout
    dims = _dims("theta", time_token=True)
    model, sd = native_model(dims, 5, "f16x3")
    model.train()
    B, n_c, n_q, T = 6, 2, 21, 3
    batch = _batch(dims, B, n_c, n_q, seed=4)
    uni = torch.rand(T, B, generator=torch.Generator().manual_seed(9))
    ro = Rollout(model, to_dev(batch), T, select="sample", uniform=uni.cuda(), keep_zt=True, time_token_T=T)
    assert ro.path == "s3::step_kernel"
    ro.run()
    torch.cuda.synchronize()
    assert ro.range_status() == 0
    idx = ro.idx.cpu()
    ref = orc.rollout(sd, batch, _cfg(dims), T, forced_idx=idx)
    assert maxdiff(ro.target_ll, torch.stack(ref["target_ll"])) < LL_TOL
    assert maxdiff(ro.log_prob, torch.stack(ref["log_prob"], 1)) < LP_TOL
    P = n_c + n_q
    role = torch.zeros(B, P, dtype=torch.int32)
    role[:, :n_c] = torch.arange(1, n_c + 1, dtype=torch.int32)
    for t in range(T):
        zt = ref["zt"][t].double()
        assert maxdiff(ro.zt[t, :, :zt.shape[1]], zt.float()) < P_TOL
        cdf = torch.cumsum(zt / zt.sum(1, keepdim=True), 1)
        u = uni[t].double()
        want = (cdf <= u[:, None]).sum(1).clamp(max=zt.shape[1] - 1)
        clear = ((cdf - u[:, None]).abs().min(1).values > 1e-4)
        assert clear.sum() >= B - 1
        assert (idx[:, t][clear] == want[clear]).all(), (t, idx[:, t], want)
        for b in range(B):
            slot = int(torch.where(role[b] == 0)[0][idx[b, t]])
            assert int(ro.slot[b, t]) == slot, (b, t)
            role[b, slot] = n_c + t + 1
    assert (ro.role.cpu() == role).all()
