"""Rollout throughput on the five BASELINE.json configs, one JSON object per config:
   python tools/config_bench.py [--configs 1,2,3,5] [--steps 3]
cfg1 al_mix dx=1 B=8 T=5 nq=32 | cfg2 location B=1000 T=30 nq=200 (d=32 and d=256/F=1024/H=8 bf16) |
cfg3 al_mix dx=2 B=512 (one GPU's share of 4096) T=50 nq=200, split mask | cfg5 psychometric d=512 H=8 predefined
mask T=30 nq=200 (F=128 literal config and F=2048).  cfg4 (CES EIG) is tools/eig_bench.py.
--configs 3w [--pairs N]: cfg3's geometry at d=256/F=1024/H=8 f16x3 (153 keys: the long-key variants of the x3 path), N alternating
pairs of the x3 path and the generic pipeline (ALINE_DISABLE_X3) in one process, one JSON line per pair.
--configs 1w [--pairs N]: the headline geometry (location_finding B=1000 T=30 nq=200) at d=128/F=512/H=4 f16x3, the same pairs for the
x1 path (ALINE_DISABLE_X1).
--configs 1wt [--pairs N]: the training leg of 1w -- `train_step` at that geometry, N alternating pairs of the default backward
(forward recompute on x1::layer_save_kernel) and ALINE_DBG_NO_BWD_IMAGE_RECOMPUTE (the generic recompute); --pairs 0: the default alone.
--configs 2h16t,3h16t --train-flag NO_BWD_ATTN_MFMA [--pairs N]: `train_step` of the models with heads of 16 channels (d=64/F=256/H=4) at the
headline geometry and at cfg3's, default (abw16::attention_bwd16_kernel) against the fp32 VALU attention backward.
Random-init weights, synthetic task data, sampled designs, HIP-graph replay; which kernel path ran is reported."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from aline_amd import Aline, Embedder, Encoder, OutputHead  # noqa: E402
from aline_amd.rollout import Rollout  # noqa: E402
from aline_amd.tasks import GPTask, HiddenLocation, PsychometricTask  # noqa: E402
from aline_amd.utils import create_target_mask  # noqa: E402
from bench import PEAK_BF16_DENSE_TFLOPS, PEAK_F32_MFMA_TFLOPS, HipEvents, algorithmic_flops_per_episode, x3_layer_flops  # noqa: E402

# MFMA passes a product costs on the f16/bf16 pipe, by arithmetic policy (f32 runs on the fp32 MFMA instead)
PASSES = {"bf16": 1, "bf16x3": 3, "f16x3": 3}


def build(dx, d, F, H, n_theta, emb, precision):
    m = Aline(Embedder(dx, 1, d, F, n_theta, emb), Encoder(d, F, H, 0.0, 3), OutputHead(dx, 1, d, F)).cuda()
    return m.set_precision(precision).train()


def path_of(d, F, H, emb, precision, keys):
    if precision == "f32" and (d, F, H) == (32, 128, 4) and emb == "theta":
        return "fused::rollout_f32_kernel"
    if precision == "f16x3" and d == 256 and H == 8 and keys <= 160:
        return "x3::layer_kernel"
    if precision == "f16x3" and d == 512 and H == 8 and keys <= 64:
        return "x5::layer_kernel"
    if precision == "f16x3" and d == 128 and H == 4 and keys <= 64:
        return "x1::layer_kernel"
    return "generic pipeline"


def roofline(geo, precision, B, dt):
    """Whole-rollout roofline on the FLOPs the kernels execute for the reference's algorithm (SURVEY 8-d formula,
    WITHOUT posterior_out_query: it is lazy and not computed).  `frac` prices the algorithmic FLOPs against the peak of
    the pipe the policy runs on; `frac_executed` counts the 3 passes of a split product (instruction-mix view)."""
    fl = algorithmic_flops_per_episode(with_query_gmm=False, **geo) * B
    peak = PEAK_F32_MFMA_TFLOPS if precision == "f32" else PEAK_BF16_DENSE_TFLOPS
    ach = fl / dt / 1e12
    r = {"bound": "mfma", "achieved": ach, "peak": peak, "unit": "TFLOP/s", "frac": ach / peak, "traffic": None,
         "algorithmic_flops_per_rollout": fl, "with_query_gmm": False, "scope": "whole rollout graph"}
    if precision in PASSES and PASSES[precision] > 1:
        r["frac_executed"] = ach * PASSES[precision] / peak
    return r


ONLY_PRECS = None


def run(name, model, batch, T, steps, meta):
    if ONLY_PRECS is not None and meta["precision"] not in ONLY_PRECS:
        return
    ro = Rollout(model, batch, T, select="sample", keep_zt=False, keep_posterior=True)
    ro.run()
    torch.cuda.synchronize()
    ro.capture()
    ro.refresh_uniform(); ro.replay()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        ro.refresh_uniform()
        ro.replay()
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / steps
    B, nq = ro.B, ro.n_q0
    out = {"config": name, "ms_per_rollout": dt * 1e3, "designs_per_s": B * T * nq / dt, "B": B, "T": T,
           "n_query_init": nq, "n_tokens": ro.P + ro.n_t, **{k: v for k, v in meta.items() if k != "geo"}, "path": ro.path}
    if "geo" in meta:
        out["roofline"] = roofline(dict(meta["geo"], T=T), meta["precision"], B, dt)
    print(json.dumps(out), flush=True)


def timed_replays(ro, steps):
    ro.refresh_uniform(); ro.replay()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        ro.refresh_uniform()
        ro.replay()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def run_pairs(name, model, batch, T, steps, pairs, geo, key="x3"):
    """Same-box alternating pairs: ms per graph-replayed rollout on the x3 (key = "x1": x1) path and on the generic pipeline (the same
    library with ALINE_DISABLE_X3 / _X1), then the path's layer-kernel launch (the C ABI's event pair: last layer of the last step) and its fraction
    of the f16 matrix pipe's peak on the SURVEY 8-d FLOPs of that launch."""
    from aline_amd import _lib
    ros, paths = {}, {}
    for k, env in ((key, {}), ("generic", {f"ALINE_DISABLE_{key.upper()}": "1"})):
        with _lib.debug_env(env):
            ros[k] = Rollout(model, batch, T, select="sample", keep_zt=False, keep_posterior=True)
            ros[k].run()
            torch.cuda.synchronize()
            paths[k] = ros[k].path
            ros[k].capture()              # (the graph holds this path's kernels: replays need no switch)
    for i in range(pairs):
        ms = {k: timed_replays(ros[k], steps) for k in (key, "generic")}
        print(json.dumps({"config": name, "pair": i, "B": ros[key].B, "T": T, f"{key}_ms_per_rollout": round(ms[key], 3),
                          "generic_ms_per_rollout": round(ms["generic"], 3), "ratio": round(ms["generic"] / ms[key], 3), "paths": paths,
                          "kernel": ros[key].kernel_name}), flush=True)
    ro, ev = ros[key], HipEvents()
    ro.r.ev_kernel_start, ro.r.ev_kernel_stop = ev.a, ev.b
    ks = []
    for _ in range(3):
        ro.refresh_uniform(); ro.run(); torch.cuda.synchronize()
        ks.append(ev.elapsed_ms())
    k = sum(ks) / len(ks)
    fl = x3_layer_flops(geo["d"], geo["F"], geo["n_c0"] + T - 1, geo["n_q0"] - (T - 1), geo["n_td"] + geo["n_th"], geo["n_s"]) * ro.B
    print(json.dumps({"config": name, "kernel": ro.kernel_name, "layer_kernel_us": round(k * 1e3, 1),
                      "frac_of_peak": round(fl / (k * 1e-3) / (PEAK_BF16_DENSE_TFLOPS * 1e12), 4),
                      "frac_executed": round(3 * fl / (k * 1e-3) / (PEAK_BF16_DENSE_TFLOPS * 1e12), 4),
                      "range": ro.range_status()}), flush=True)


def timed_train_steps(model, batch, T, opt, steps):
    from aline_amd.train import train_step
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        train_step(model, batch, T, optimizer=opt)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def run_train_pairs(name, model, batch, T, steps, pairs, flag="NO_BWD_IMAGE_RECOMPUTE"):
    """Same-box alternating pairs: ms per `train_step` (sampled rollout, REINFORCE terms, backward, optimiser) with the library's default
    backward and with the diagnostic switch `flag` set -- the generic forward recompute, which is what the library did for this shape before
    the layer kernel's SAVE variant.  One JSON line per pair; which kernel recomputes the chunks is reported by the library.
    (pairs = 0: timed steps of the default only -- the form a run on another build of the library takes, ALINE_HIP_LIB.)
    --train-flag NO_BWD_DW_NARROW: the other side is the weight-gradient dispatch before the narrow-tile f16 kernel (fp32 block kernel)."""
    import ctypes
    from aline_amd import _lib
    from aline_amd.train import train_step
    opt = torch.optim.Adam(model.parameters(), lr=1e-5)
    names = {}
    other = "generic_recompute" if flag == "NO_BWD_IMAGE_RECOMPUTE" else flag.lower()
    for k, flags in (("default", []), (other, [flag])):
        with _lib.debug(*flags):
            for _ in range(2):                              # warm-up of both sides: code objects, graph cache, workspace
                _, ro = train_step(model, batch, T, optimizer=opt)
            buf = ctypes.create_string_buffer(64)      # (the answer for the last step's key count: the most any chunk of the backward shows)
            rc = _lib.lib.aline_backward_recompute_name(ctypes.byref(ro.m), ctypes.byref(ro.r), T - 1, 1, buf, 64)
            names[k] = [buf.value.decode(), rc]
    if pairs == 0:
        for i in range(3):
            print(json.dumps({"config": name, "run": i, "lib": os.path.basename(_lib.LIB_PATH), "ms_per_train_step": round(timed_train_steps(model, batch, T, opt, steps), 2),
                              "recompute": names["default"]}), flush=True)
        return
    for i in range(pairs):
        ms = {}
        for k, flags in (("default", []), (other, [flag])):
            with _lib.debug(*flags):
                ms[k] = timed_train_steps(model, batch, T, opt, steps)
        print(json.dumps({"config": name, "pair": i, "B": int(ro.B), "T": T, "default_ms_per_train_step": round(ms["default"], 2),
                          f"{other}_ms_per_train_step": round(ms[other], 2),
                          "ratio": round(ms[other] / ms["default"], 4), "recompute": names}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="1,2,3,5")
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--precs", default="", help="comma list: only these precisions (default: all)")
    ap.add_argument("--pairs", type=int, default=5, help="3w / 1w: alternating pairs")
    ap.add_argument("--train-flag", default="NO_BWD_IMAGE_RECOMPUTE", help="1wt / 5t: the diagnostic switch of the other side of a pair")
    args = ap.parse_args()
    global ONLY_PRECS
    ONLY_PRECS = set(args.precs.split(",")) if args.precs else None
    want = set(args.configs.split(","))
    dev = torch.device("cuda")
    torch.manual_seed(123)
    if "1" in want:
        task = GPTask(dim_x=1, embedding_type="mix", n_context_init=1, n_query_init=32, n_target_theta=2,
                      n_target_data=100, device=dev)
        geo = dict(dx=1, dy=1, d=32, F=128, H=4, L=3, C=10, n_c0=1, n_q0=32, n_td=100, n_th=2, n_s=102, embedding_type="mix")
        b1 = task.sample_batch(8)
        for prec in ("f32", "f16x3"):
            run(f"cfg1 al_mix dx=1 B=8 T=5 {prec}", build(1, 32, 128, 4, 2, "mix", prec), b1, 5, args.steps,
                {"d": 32, "precision": prec, "path": "", "geo": geo})
    if "2" in want:
        task = HiddenLocation(n_query_init=200, device=dev)
        batch = task.sample_batch(1000)
        geo = dict(dx=2, dy=1, d=32, F=128, H=4, L=3, C=10, n_c0=1, n_q0=200, n_td=0, n_th=2, n_s=2)
        run("cfg2 location_finding B=1000 T=30 d=32", build(2, 32, 128, 4, 2, "theta", "f32"), batch, 30, args.steps,
            {"d": 32, "precision": "f32", "path": path_of(32, 128, 4, "theta", "f32", 32), "geo": geo})
        run("cfg2 location_finding B=1000 T=30 d=32 f16x3", build(2, 32, 128, 4, 2, "theta", "f16x3"), batch, 30, args.steps,
            {"d": 32, "precision": "f16x3", "path": "", "geo": geo})
        for prec in ("f16x3", "bf16"):
            run(f"cfg2 location_finding B=1000 T=30 d=256 F=1024 H=8 {prec}", build(2, 256, 1024, 8, 2, "theta", prec), batch, 30,
                args.steps, {"d": 256, "precision": prec, "path": path_of(256, 1024, 8, "theta", prec, 32),
                             "geo": dict(geo, d=256, F=1024, H=8)})
    if "3" in want:
        task = GPTask(dim_x=2, embedding_type="mix", n_context_init=1, n_query_init=200, n_target_theta=3,
                      n_target_data=100, device=dev)
        batch = task.sample_batch(512)
        batch["target_mask"] = create_target_mask("split", "mix", 100, 3, None, None, None, None, "data")
        geo = dict(dx=2, dy=1, d=32, F=128, H=4, L=3, C=10, n_c0=1, n_q0=200, n_td=100, n_th=3, n_s=100, embedding_type="mix")
        for prec in ("f32", "f16x3"):
            run(f"cfg3 al_mix dx=2 B=512 (of 4096 over 8 GPUs) T=50, split mask (data) {prec}", build(2, 32, 128, 4, 3, "mix", prec),
                batch, 50, args.steps, {"d": 32, "precision": prec, "path": path_of(32, 128, 4, "mix", prec, 999), "geo": geo})
    if "3w" in want:
        task = GPTask(dim_x=2, embedding_type="mix", n_context_init=1, n_query_init=200, n_target_theta=3,
                      n_target_data=100, device=dev)
        batch = task.sample_batch(512)
        batch["target_mask"] = create_target_mask("split", "mix", 100, 3, None, None, None, None, "data")
        geo = dict(dx=2, dy=1, d=256, F=1024, H=8, L=3, C=10, n_c0=1, n_q0=200, n_td=100, n_th=3, n_s=100, embedding_type="mix")
        run_pairs("cfg3 geometry at d=256 F=1024 H=8 f16x3: al_mix dx=2 B=512 T=50, split mask (data)", build(2, 256, 1024, 8, 3, "mix", "f16x3"),
                  batch, 50, args.steps, args.pairs, geo)
    if "1w" in want:
        batch = HiddenLocation(n_query_init=200, device=dev).sample_batch(1000)
        geo = dict(dx=2, dy=1, d=128, F=512, H=4, L=3, C=10, n_c0=1, n_q0=200, n_td=0, n_th=2, n_s=2)
        run_pairs("headline geometry at d=128 F=512 H=4 f16x3: location_finding B=1000 T=30", build(2, 128, 512, 4, 2, "theta", "f16x3"),
                  batch, 30, args.steps, args.pairs, geo, key="x1")
    if "1wt" in want:
        batch = HiddenLocation(n_query_init=200, device=dev).sample_batch(1000)
        run_train_pairs("headline geometry at d=128 F=512 H=4 f16x3: location_finding B=1000 T=30, train_step",
                        build(2, 128, 512, 4, 2, "theta", "f16x3"), batch, 30, args.steps, args.pairs, args.train_flag)
    if "2h16t" in want:   # heads of 16 channels: the headline geometry at d = 64 / F = 256 / H = 4, pairs against --train-flag NO_BWD_ATTN_MFMA
        batch = HiddenLocation(n_query_init=200, device=dev).sample_batch(1000)
        run_train_pairs("headline geometry at d=64 F=256 H=4 f16x3: location_finding B=1000 T=30, train_step",
                        build(2, 64, 256, 4, 2, "theta", "f16x3"), batch, 30, args.steps, args.pairs, args.train_flag)
    if "3h16t" in want:   # cfg3's geometry at d = 64 / F = 256 / H = 4 (up to 153 keys)
        batch = GPTask(dim_x=2, embedding_type="mix", n_context_init=1, n_query_init=200, n_target_theta=3,
                       n_target_data=100, device=dev).sample_batch(512)
        batch["target_mask"] = create_target_mask("split", "mix", 100, 3, None, None, None, None, "data")
        run_train_pairs("cfg3 geometry at d=64 F=256 H=4 f16x3: al_mix dx=2 B=512 T=50, split mask (data), train_step",
                        build(2, 64, 256, 4, 3, "mix", "f16x3"), batch, 50, args.steps, args.pairs, args.train_flag)
    if "5t" in want:      # the training leg of cfg5 at F = 128 (its 128-wide weight-gradient products), pairs against --train-flag
        batch = PsychometricTask(n_query_init=200, n_context_init=1, device=dev).sample_batch(256)
        batch["target_mask"] = torch.tensor([False, False, True, True])
        run_train_pairs("cfg5 psychometric B=256 T=30 d=512 F=128 H=8 f16x3, predefined mask, train_step",
                        build(1, 512, 128, 8, 4, "theta", "f16x3"), batch, 30, args.steps, args.pairs, args.train_flag)
    if "5" in want:
        task = PsychometricTask(n_query_init=200, n_context_init=1, device=dev)
        batch = task.sample_batch(256)
        batch["target_mask"] = torch.tensor([False, False, True, True])
        for F in (128, 2048):
            geo = dict(dx=1, dy=1, d=512, F=F, H=8, L=3, C=10, n_c0=1, n_q0=200, n_td=0, n_th=4, n_s=2)
            for prec in ("f16x3", "bf16"):
                run(f"cfg5 psychometric B=256 T=30 d=512 F={F} H=8, predefined mask {prec}", build(1, 512, F, 8, 4, "theta", prec),
                    batch, 30, args.steps, {"d": 512, "precision": prec, "path": path_of(512, F, 8, "theta", prec, 0), "geo": geo})


if __name__ == "__main__":
    main()
