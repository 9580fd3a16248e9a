"""Time the training step of the d = 256 / F = 1024 model (bench `d256.train_step` shape) under debug flags: python tools/d256_train_time.py [FLAGS ...]
--cfg3[=B]: cfg3's geometry at that width instead (al_mix dx = 2, 100 data targets + 3 theta tokens, split mask, T = 50, 104 - 153 keys: the
attention backward of attn_bwd_long.h), B = 512 episodes unless given; one JSON line (library variants: ALINE_HIP_LIB=... for alternating runs)."""
import json, os, sys, time, torch
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from aline_amd import Aline, Embedder, Encoder, OutputHead, _lib
from aline_amd.tasks import GPTask, HiddenLocation
from aline_amd.train import train_step
from aline_amd.utils import create_target_mask
torch.manual_seed(0)
dev = torch.device("cuda")
d, F = 256, 1024
flags = [a for a in sys.argv[1:] if not a.startswith("--")]
cfg3 = [a for a in sys.argv[1:] if a.startswith("--cfg3")]
if cfg3:
    B, T, kw = int(cfg3[0].partition("=")[2] or 512), 50, {"embedding_type": "mix", "mask_type": "split"}
    m = Aline(Embedder(2, 1, d, F, 3, "mix"), Encoder(d, F, 8, 0.0, 3), OutputHead(2, 1, d, F)).cuda().set_precision("f16x3").train()
    batch = GPTask(dim_x=2, embedding_type="mix", n_context_init=1, n_query_init=200, n_target_theta=3, n_target_data=100, device=dev).sample_batch(B)
    batch["target_mask"] = create_target_mask("split", "mix", 100, 3, None, None, None, None, "data")
else:
    B, T, kw = 1000, 30, {}
    m = Aline(Embedder(2, 1, d, F, 2, "theta"), Encoder(d, F, 8, 0.0, 3), OutputHead(2, 1, d, F)).cuda().set_precision("f16x3").train()
    batch = HiddenLocation(n_query_init=200, device=dev).sample_batch(B)
opt = torch.optim.AdamW(m.parameters(), lr=1e-3)
with _lib.debug(*flags):
    train_step(m, batch, T, optimizer=opt, **kw); torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(2):
        terms, _ = train_step(m, batch, T, optimizer=opt, **kw)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / 2 * 1e3
    if cfg3:
        print(json.dumps({"shape": "cfg3 geometry at d=256 F=1024 H=8 f16x3, train step", "B": B, "T": T, "flags": flags,
                          "lib": os.path.basename(os.environ.get("ALINE_HIP_LIB", "libaline_hip.so")), "train_step_ms": round(ms, 1), "loss": float(terms["loss"])}))
    else:
        print(flags, "d256 train step %.1f ms" % ms, "loss", float(terms["loss"]))
