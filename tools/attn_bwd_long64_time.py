"""Backward time of head_dim-64 models at 49 - 160 keys, the kernel of attn_bwd_long64.h against the fp32 VALU kernel (NO_BWD_ATTN_MFMA):
    python tools/attn_bwd_long64_time.py ab [pairs]     alternating pairs in one process where both launch, one JSON line per shape
    python tools/attn_bwd_long64_time.py new | parent   one side only, for a `rocprofv3 --kernel-trace --stats` run of its own
                                                        (new: also the 8- and 10-tile shapes, which the VALU kernel cannot hold)"""
import json, os, sys, torch
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from aline_amd import Aline, Embedder, Encoder, OutputHead, _lib
from aline_amd.rollout import Rollout
from aline_amd.tasks import GPTask, HiddenLocation
from aline_amd.train import backward, reinforce_terms

dev = torch.device("cuda")
# name, d, F, H, L, emb, n_query, n_td, T, t_chunk, B, the VALU kernel launches
SHAPES = [
    ("location d=512 H=8 N=203, last chunk 49-54 keys (4 tiles)", 512, 128, 8, 2, "theta", 200, 0, 52, 46, 256, True),
    ("mix d=128 H=2 N=94, 74-78 keys (5 tiles)", 128, 64, 2, 2, "mix", 20, 70, 5, None, 1024, True),
    ("mix d=128 H=2 N=148, 124-128 keys (8 tiles)", 128, 64, 2, 2, "mix", 24, 120, 5, None, 1024, False),
    ("mix d=128 H=2 N=324, 160 keys (10 tiles)", 128, 64, 2, 2, "mix", 170, 150, 7, None, 512, False),
]


def prepare(d, F, H, L, emb, nq, n_td, T, B):
    torch.manual_seed(d + T)
    n_theta = 2 if emb == "theta" else 3
    m = Aline(Embedder(2, 1, d, F, n_theta, emb), Encoder(d, F, H, 0.0, L), OutputHead(2, 1, d, F)).cuda().set_precision("f16x3").train()
    if emb == "theta":
        batch = HiddenLocation(n_query_init=nq, device=dev).sample_batch(B)
    else:
        batch = GPTask(dim_x=2, embedding_type=emb, n_context_init=1, n_query_init=nq, n_target_theta=3, n_target_data=n_td, device=dev).sample_batch(B)
    with torch.no_grad():
        ro = Rollout(m, batch, T, select="sample").run()
        terms = reinforce_terms(ro, emb, "all")
    return m, ro, terms


def timed(m, ro, terms, tc, flags, reps):
    """ms per backward over reps calls between two device events"""
    with torch.no_grad(), _lib.debug(*flags):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            for p in m.parameters():
                p.grad = None
            backward(m, ro, terms["g_logp"], terms["g_ll"], t_chunk=tc)
        e1.record()
        torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


mode = sys.argv[1]
pairs = int(sys.argv[2]) if len(sys.argv) > 2 else 6
for name, d, F, H, L, emb, nq, n_td, T, tc, B, valu in SHAPES:
    if not valu and mode != "new":
        continue
    m, ro, terms = prepare(d, F, H, L, emb, nq, n_td, T, B)
    if mode == "ab":
        reps = 4
        for flags in ([], ["NO_BWD_ATTN_MFMA"]):      # warm both sides
            timed(m, ro, terms, tc, flags, 1)
        new, old = [], []
        for _ in range(pairs):
            new.append(timed(m, ro, terms, tc, [], reps))
            old.append(timed(m, ro, terms, tc, ["NO_BWD_ATTN_MFMA"], reps))
        print(json.dumps({"shape": name, "B": B, "T": T, "t_chunk": tc, "backward_ms_new": [round(x, 2) for x in new],
                          "backward_ms_valu": [round(x, 2) for x in old], "ratio_valu_over_new_per_pair": [round(o / n, 3) for n, o in zip(new, old)]}), flush=True)
    else:
        flags = [] if mode == "new" else ["NO_BWD_ATTN_MFMA"]
        timed(m, ro, terms, tc, flags, 1)
        print(json.dumps({"shape": name, "side": mode, "B": B, "backward_ms": round(timed(m, ro, terms, tc, flags, 3), 2)}), flush=True)
