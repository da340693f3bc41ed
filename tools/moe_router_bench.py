"""The fused router (moe_route: one gptq_moe_router launch) against the transformers composition it replaces (F.linear, .float(), softmax, topk, sum,
div -- MixtralTopKRouter.forward, operation for operation), A/B in ONE process on the GPU:

  alone     each variant captured as a graph of its own and replayed
  +experts  each variant in front of moe_forward (random 4-bit g128 experts, post_init(decode_copy=True, batch=True): decode path up to 4 tokens, batch
            path up to 64, grouped above), router and experts captured as ONE graph per variant

Shapes (E, topk, H, I): Mixtral-8x7B (8, 2, 4096, 14336), (60, 4, 2048, 1408), (64, 8, 3584, 2560), (128, 8, 2048, 768); T = 1, 4, 16, 64, 2048; fp16.
Per sample ONE pair of device events around --reps back-to-back replays of one graph, divided by --reps; the two variants alternate sample by sample;
--samples samples each after warm-up (default 30 x 10 = 300 replays per variant and cell).  Reported: median [p10 .. p90] in microseconds and the ratio of the
medians (composition / fused: above 1 the fused router is faster).  The input is fixed across replays, so the routing is too (a warm-cache number for the
experts; both variants see the same one).  The comparison is between the two variants of the same run; there is no absolute target.

    python tools/moe_router_bench.py [--samples 30] [--reps 10] [--out profiles/moe_router_ab.log] [--no-experts] [--shapes mixtral8x7b,e128]
"""
import argparse
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from autogptq_amd import moe as M  # noqa: E402
from autogptq_amd.moe import moe_forward, moe_route  # noqa: E402

SHAPES = {"mixtral8x7b": (8, 2, 4096, 14336), "e60": (60, 4, 2048, 1408), "e64": (64, 8, 3584, 2560), "e128": (128, 8, 2048, 768)}
TS = (1, 4, 16, 64, 2048)
DEV = "cuda:0"


def composition(x, w, topk):
    logits = F.linear(x, w)
    probs = F.softmax(logits.float(), dim=-1)
    val, idx = torch.topk(probs, topk, dim=-1)
    val /= val.sum(dim=-1, keepdim=True)
    return logits, val, idx


def fused(x, w, topk):
    return moe_route(x, w, topk, renorm=True, return_logits=True)


def capture(fn):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.no_grad(), torch.cuda.stream(side):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.no_grad(), torch.cuda.graph(g):
        out = fn()
    return g, out


def ab(graphs, samples, reps):
    """graphs: {name: graph}; alternating samples; {name: (median, p10, p90)} in microseconds per replay."""
    for g in graphs.values():
        for _ in range(2 * reps):
            g.replay()
    torch.cuda.synchronize()
    ts = {k: [] for k in graphs}
    for _ in range(samples):
        for k, g in graphs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(reps):
                g.replay()
            b.record()
            b.synchronize()
            ts[k].append(a.elapsed_time(b) * 1e3 / reps)
    out = {}
    for k, v in ts.items():
        v.sort()
        out[k] = (v[len(v) // 2], v[len(v) // 10], v[(9 * len(v)) // 10])
    return out


def fmt(r):
    return f"{r[0]:9.2f} [{r[1]:8.2f} .. {r[2]:8.2f}]"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=30)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "moe_router_ab.log"))
    ap.add_argument("--no-experts", action="store_true")
    ap.add_argument("--shapes", default=",".join(SHAPES))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "moe_router_bench.py needs the GPU"
    assert args.samples * args.reps >= 200, "at least 200 replays per variant"
    dtype = torch.float16
    lines = [f"# fused router vs transformers composition, fp16, {torch.cuda.get_device_name(0)}; microseconds per graph replay: median [p10 .. p90] of "
             f"{args.samples} samples x {args.reps} replays, variants alternating; ratio = composition / fused",
             f"# {'shape':12s} {'T':>5s} {'form':6s} | {'alone: composition':>32s} {'fused':>32s} {'ratio':>6s} | {'+experts: composition':>32s} "
             f"{'fused':>32s} {'ratio':>6s} {'saved us':>9s} experts"]
    print("\n".join(lines), flush=True)
    for name in args.shapes.split(","):
        E, topk, H, I = SHAPES[name]
        g = torch.Generator().manual_seed(E + H)
        w = (torch.randn((E, H), generator=g) / H ** 0.5).to(dtype).to(DEV)
        q = None
        if not args.no_experts:
            from test_gpu_moe import make_experts
            q = make_experts(E, H, I, 4, 128, False, dtype, seed=1, top_k=topk)
            q.post_init(decode_copy=True, batch=True)
        for T in TS:
            x = torch.randn((T, H), generator=g).to(dtype).to(DEV)
            plan = M.router_plan(T, H, E, topk, dtype, True)
            graphs, outs = {}, {}
            for k, fn in (("composition", composition), ("fused", fused)):
                graphs[k], outs[k] = capture(lambda fn=fn: fn(x, w, topk))
            same = (outs["composition"][2].sort(-1).values == outs["fused"][2].sort(-1).values).all(-1).float().mean().item()
            alone = ab(graphs, args.samples, args.reps)
            line = (f"  {name:12s} {T:5d} {plan.get('form', plan['path']):6s} | {fmt(alone['composition'])} {fmt(alone['fused'])} "
                    f"{alone['composition'][0] / alone['fused'][0]:6.2f} |")
            if q is None:
                line += " not measured"
            else:
                graphs = {}
                for k, fn in (("composition", composition), ("fused", fused)):
                    def both(fn=fn):
                        _, val, idx = fn(x, w, topk)
                        return moe_forward(q, x, idx, val)
                    graphs[k], _ = capture(both)
                full = ab(graphs, args.samples, args.reps)
                line += (f" {fmt(full['composition'])} {fmt(full['fused'])} {full['composition'][0] / full['fused'][0]:6.2f} "
                         f"{full['composition'][0] - full['fused'][0]:9.2f} {q.plan(T, topk)['path']}")
            line += f"   (same expert sets: {100 * same:.1f} % of tokens)"
            lines.append(line)
            print(line, flush=True)
        del q
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
