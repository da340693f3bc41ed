#!/usr/bin/env python3
"""Forward + backward of one QuantMoEExperts under grad: the grouped backward (post_init(backward=True): one autograd node, one gptq_moe_backward call)
against the per-expert composition it replaces (the default under grad: a Python loop over the experts with a host sync each, 3 E autograd nodes).

Mixtral-8x7B shapes (E = 8, topk = 2, H = 4096, I = 14336), int4 g128 fp16, T = 512 and 2048; hidden_states and top_k_weights both require grad.  Both forms
run in this one process on the SAME module (re-post-initialised between them), eagerly -- the composition synchronises the host and cannot be captured --
timed by HIP events around `--reps` forward + backward pairs, min over `--rounds` rounds, the two forms alternating.
usage: python tools/moe_backward_sweep.py [--ts 512,2048] [--rounds 3] [--reps 3] [--quick]"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from autogptq_amd.moe import QuantMoEExperts  # noqa: E402
from autogptq_amd.qlinear_mi355x import reserve_workspace  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--ts", default="512,2048")
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--reps", type=int, default=3, help="forward + backward pairs per timed window")
ap.add_argument("--quick", action="store_true", help="H = 1024, I = 3584")
args = ap.parse_args()
dev = torch.device("cuda:0")
E, TOPK, BITS, GS = 8, 2, 4, 128
H, I = (1024, 3584) if args.quick else (4096, 14336)
TS = [int(t) for t in args.ts.split(",")]


def fill(lin, gen):
    lin.qweight = torch.randint(-2 ** 31, 2 ** 31 - 1, lin.qweight.shape, generator=gen, dtype=torch.int64).to(torch.int32)
    lin.qzeros = torch.randint(-2 ** 31, 2 ** 31 - 1, lin.qzeros.shape, generator=gen, dtype=torch.int64).to(torch.int32)
    lin.scales = (torch.rand(lin.scales.shape, generator=gen) * 0.004 + 0.001).to(lin.scales.dtype)
    lin.g_idx = torch.arange(lin.infeatures, dtype=torch.int32) // lin.group_size


def step(q, x, idx, w, gy):
    x.grad = w.grad = None
    q(x, idx, w).backward(gy)


def ms(q, x, idx, w, gy):
    step(q, x, idx, w, gy)                              # warm: workspace, allocator
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(args.reps):
        step(q, x, idx, w, gy)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / args.reps


gen = torch.Generator().manual_seed(0)
q = QuantMoEExperts(E, H, I, BITS, GS, top_k=TOPK, weight_dtype=torch.float16)
for e in range(E):
    for l in q[e].layers():
        fill(l, gen)
q = q.to(dev)
for T in TS:
    x = (torch.rand((T, H), generator=gen) - 0.5).half().to(dev).requires_grad_(True)
    gy = (torch.rand((T, H), generator=gen) - 0.5).half().to(dev)
    idx = torch.stack([torch.randperm(E, generator=gen)[:TOPK] for _ in range(T)]).to(dev)
    w = torch.rand((T, TOPK), generator=gen).to(dev)
    w = (w / w.sum(-1, keepdim=True)).requires_grad_(True)
    best, grads = {"grouped": float("inf"), "composition": float("inf")}, {}
    for _ in range(args.rounds):
        for form in best:
            q.post_init(backward=form == "grouped")
            if form == "grouped":
                reserve_workspace(dev, max(q.backward_workspace_bytes(T, TOPK), q.workspace_bytes(T, TOPK)))
            best[form] = min(best[form], ms(q, x, idx, w, gy))
            want = "grouped" if form == "grouped" else None
            assert q.last_plan.get("backward") == want, q.last_plan
            grads[form] = (x.grad.float().clone(), w.grad.float().clone())
    dx = float((grads["grouped"][0] - grads["composition"][0]).abs().max() / grads["composition"][0].abs().max())
    dw = float((grads["grouped"][1] - grads["composition"][1]).abs().max() / grads["composition"][1].abs().max())
    print(f"E={E} topk={TOPK} H={H} I={I} int{BITS} g{GS} f16  T={T:<5d} forward+backward: grouped {best['grouped']:8.3f} ms  composition "
          f"{best['composition']:8.3f} ms  ratio {best['composition'] / best['grouped']:5.2f}x   rel.diff dX {dx:.1e} dw {dw:.1e}", flush=True)
