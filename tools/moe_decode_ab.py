"""The routed-only decode call (moe_forward on experts with a decode copy: gptq_moe_decode_forward, two launches) of ONE checkout, timed so that two
checkouts can be compared: run it once per tree, alternating, and read the lines side by side (profiles/moe_decode_shared_form_ab.log compares the
commit before the decode kernels got their shared form with the commit after).

Shapes (E, topk, H, I): Qwen1.5-MoE-A2.7B's experts (60, 4, 2048, 1408) and Mixtral-8x7B's (8, 2, 4096, 14336), 4-bit g128 fp16, T = 1..4.
ROTATING WEIGHTS: --sets expert sets with weights and routing of their own run back to back in one captured graph, so that a replay streams more than the
Infinity Cache holds (A2.7B at T = 1: 17 MB per layer, 16 sets; Mixtral: 176 MB per layer, 3 sets); times are per layer (graph time / sets).  Per sample
one pair of device events around 10 replays; median [p10 .. p90] of 30 samples after 5 warm-up samples, and a checksum of the outputs (equal checksums:
the two checkouts compute the same values on the same seeded inputs).

    python tools/moe_decode_ab.py --tree /path/to/checkout --label parent [--out profiles/moe_decode_shared_form_ab.log]
"""
import argparse
import os
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--label", default="this tree")
ap.add_argument("--out", default=None)
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.tree))

import torch  # noqa: E402

import autogptq_amd  # noqa: E402
from autogptq_amd.moe import QuantMoEExperts, moe_forward  # noqa: E402

assert os.path.abspath(autogptq_amd.__file__).startswith(os.path.abspath(args.tree)), autogptq_amd.__file__
assert torch.cuda.is_available(), "moe_decode_ab.py needs the GPU"
DEV = "cuda:0"
SHAPES = {"a2.7b": (60, 4, 2048, 1408, 16), "mixtral": (8, 2, 4096, 14336, 3)}


def fill(lin, gen):
    lin.qweight = torch.randint(-2 ** 31, 2 ** 31 - 1, lin.qweight.shape, generator=gen, dtype=torch.int64).to(torch.int32)
    lin.qzeros = torch.randint(-2 ** 31, 2 ** 31 - 1, lin.qzeros.shape, generator=gen, dtype=torch.int64).to(torch.int32)
    lin.scales = (torch.rand(lin.scales.shape, generator=gen) * 0.004 + 0.001).to(lin.scales.dtype)
    lin.g_idx = torch.arange(lin.infeatures, dtype=torch.int32) // lin.group_size


def experts(E, H, I, topk, seed):
    gen = torch.Generator().manual_seed(seed)
    q = QuantMoEExperts(E, H, I, 4, 128, top_k=topk, weight_dtype=torch.float16)
    for e in range(E):
        for l in q[e].layers():
            fill(l, gen)
    return q.to(DEV).post_init(decode_copy=True)


lines = []
for name, (E, topk, H, I, nsets) in SHAPES.items():
    sets = [experts(E, H, I, topk, 10 + i) for i in range(nsets)]
    for T in (1, 2, 3, 4):
        x = (torch.rand((T, H), generator=torch.Generator().manual_seed(T)) - 0.5).half().to(DEV)
        g0 = torch.Generator().manual_seed(T)
        routes = []
        for _ in sets:
            idx = torch.stack([torch.randperm(E, generator=g0)[:topk] for _ in range(T)]).to(DEV)
            routes.append((idx, torch.full((T, topk), 1.0 / topk, device=DEV)))

        def run():
            return [moe_forward(q, x, i, w) for q, (i, w) in zip(sets, routes)]

        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.no_grad(), torch.cuda.stream(side):
            for _ in range(3):
                run()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.no_grad(), torch.cuda.graph(g):
            out = run()
        assert sets[0].last_plan["path"] == "decode"
        ts = []
        for s in range(35):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(10):
                g.replay()
            b.record()
            b.synchronize()
            if s >= 5:
                ts.append(a.elapsed_time(b) * 1e3 / 10 / len(sets))
        ts.sort()
        chk = float(sum(o.float().abs().sum() for o in out))
        lines.append(f"{args.label:>10} {name:>8} T={T}: {ts[15]:7.2f} us per layer [{ts[3]:7.2f} .. {ts[27]:7.2f}]  checksum {chk:.6e}")
        print(lines[-1], flush=True)
        del g, out
    del sets
    torch.cuda.empty_cache()
if args.out:
    with open(args.out, "a") as f:
        f.write("\n".join(lines) + "\n")
