#!/usr/bin/env python3
"""The adapter branch of LoraQuantLinear (gptq_lora_apply: a down and an up launch) against the torch composition it replaces (INTEGRATION.md section 9:
``base(x) + s * ((x.float() @ A.t()) @ B.t()).to(x.dtype)`` on fp32 master weights) and against the base layer alone.

Per shape, r and M three hipGraphs are captured over the SAME rotation of distinct layers (together beyond the Infinity Cache, so every launch reads its
weights from HBM: BASELINE.md) -- one call per layer -- and timed by HIP events, alternating the three forms in one process, min over `--rounds` rounds.
The figure that matters is the adapter's overhead: `lora - base` against `composition - base`.  The q|k|v rows time forward_multi on three bases against
lora_forward_multi (one down and one up launch for the three adapters) and against three compositions.
usage: python tools/lora_sweep.py [--ms 1,4,16,64,2048] [--rs 16,64] [--rounds 3] [--quick]"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from autogptq_amd import LoraQuantLinear, lora_forward_multi  # noqa: E402
from autogptq_amd.qlinear_mi355x import forward_multi  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--ms", default="1,4,16,64,2048")
ap.add_argument("--rs", default="16,64")
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--reps", type=int, default=5, help="replays per timed window")
ap.add_argument("--cold-mb", type=int, default=320, help="packed weights of one rotation")
ap.add_argument("--quick", action="store_true", help="4096 x 4096 only, two layers per rotation")
args = ap.parse_args()
dev = torch.device("cuda:0")
SHAPES = [(4096, 4096), (4096, 11008), (11008, 4096)]
if args.quick:
    SHAPES = SHAPES[:1]
MS = [int(m) for m in args.ms.split(",")]
RS = [int(r) for r in args.rs.split(",")]


class Composition(torch.nn.Module):
    """INTEGRATION.md section 9's hand-rolled adapter (with the scale): what LoraQuantLinear replaces."""

    def __init__(self, lq):
        super().__init__()
        self.base, self.A, self.B, self.s = lq.base, lq.lora_A.weight, lq.lora_B.weight, lq.scaling

    def adapter(self, x):
        return (((x.float() @ self.A.t()) @ self.B.t()) * self.s).to(x.dtype)

    def forward(self, x):
        return self.base(x) + self.adapter(x)


def graph_of(fn):
    with torch.no_grad():
        fn()
        fn()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            fn()
    return g


def us(g, calls):
    bench.settle(g, dev)
    _, evt = bench.time_graph(g, args.reps, dev)
    return evt / args.reps / calls * 1e6


def adapters(bases, r):
    out = []
    for i, q in enumerate(bases):
        lq = LoraQuantLinear(q, r, 2 * r).eval()
        with torch.no_grad():
            lq.lora_B.weight.copy_(torch.randn(lq.lora_B.weight.shape, device=dev, generator=torch.Generator(device=dev).manual_seed(i)) * 0.05)
        out.append(lq)
    return out


def measure(forms, calls):
    best = {k: float("inf") for k in forms}
    for _ in range(args.rounds):
        for k, g in forms.items():
            best[k] = min(best[k], us(g, calls))
    return best


def report(tag, r, M, best, err):
    over_l, over_c = best["lora"] - best["base"], best["comp"] - best["base"]
    print(f"{tag:22s} r={r:<2d} M={M:<4d}  base {best['base']:8.2f} us  lora {best['lora']:8.2f}  comp {best['comp']:8.2f}   overhead: lora {over_l:7.2f}  "
          f"comp {over_c:7.2f}  ratio {over_l / over_c if over_c > 0 else float('nan'):5.2f}  {'ok' if over_l < over_c else 'COMPOSITION WINS'}  rel.diff {err:.1e}", flush=True)


for K, N in SHAPES:
    n = 2 if args.quick else max(4, -(-(args.cold_mb << 20) // (K * N // 2)))
    bases = [bench.make_layer(K, N, dev, seed=9000 + i) for i in range(n)]
    for r in RS:
        lqs = adapters(bases, r)
        comps = [Composition(l) for l in lqs]
        for M in MS:
            x = (torch.rand(M, K, device=dev) - 0.5).half()
            forms = {"base": graph_of(lambda: [q(x) for q in bases]), "lora": graph_of(lambda: [l(x) for l in lqs]),
                     "comp": graph_of(lambda: [c(x) for c in comps])}
            best = measure(forms, n)
            with torch.no_grad():
                a, b = lqs[0](x).float(), comps[0](x).float()
            report(f"{K}x{N} int4 g128 f16", r, M, best, float((a - b).abs().max() / b.abs().max()))
            del forms
        del lqs, comps
    del bases
    torch.cuda.empty_cache()

# q|k|v: three 4096 x 4096 projections that share x, decode rows
K = 4096
n = 2 if args.quick else max(2, -(-(args.cold_mb << 20) // (3 * K * K // 2)))
groups = [[bench.make_layer(K, K, dev, seed=9500 + 3 * i + j) for j in range(3)] for i in range(n)]
for r in RS:
    lgroups = [adapters(g, r) for g in groups]
    cgroups = [[Composition(l) for l in g] for g in lgroups]
    for M in (1, 4):
        x = (torch.rand(M, K, device=dev) - 0.5).half()
        forms = {"base": graph_of(lambda: [forward_multi(g, x) for g in groups]), "lora": graph_of(lambda: [lora_forward_multi(g, x) for g in lgroups]),
                 "comp": graph_of(lambda: [[y + c.adapter(x) for y, c in zip(forward_multi(g, x), cg)] for g, cg in zip(groups, cgroups)])}
        best = measure(forms, n)
        with torch.no_grad():
            a, b = lora_forward_multi(lgroups[0], x)[2].float(), cgroups[0][2](x).float()
        report("q|k|v 3 x 4096x4096", r, M, best, float((a - b).abs().max() / b.abs().max()))
        del forms
    del lgroups, cgroups
