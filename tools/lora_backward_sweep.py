#!/usr/bin/env python3
"""The adapter's backward of LoraQuantLinear: one gptq_lora_backward (``fused_backward=True``) against the torch matmuls it replaces.

Per shape, r, M and dtype ONE adapted layer runs forward + backward (x, lora_A and lora_B all ask for a gradient) with the switch off and on, alternating in
one process and one session; HIP events around `--iters` eager steps, median of `--rounds` windows, after a warm-up.  Two figures per form:
  step   forward + backward of the layer (base product, gptq_grad_input and the adapter: what a training step pays per projection)
  bwd    the adapter's backward alone (the products on the tensors the forward saved: what this switch changes)
and the peak of torch's allocator over one step above the level before it (the fp32 activation-sized temporaries of the torch backward show here).
usage: python tools/lora_backward_sweep.py [--ms 512,2048,4096] [--rs 16,64] [--dtypes f16,bf16] [--iters 10] [--rounds 5] [--quick]"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from autogptq_amd import LoraQuantLinear  # noqa: E402
from autogptq_amd import lora as LR  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--ms", default="512,2048,4096")
ap.add_argument("--rs", default="16,64")
ap.add_argument("--dtypes", default="f16,bf16")
ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--quick", action="store_true", help="4096 x 4096 only")
args = ap.parse_args()
dev = torch.device("cuda:0")
SHAPES = [(4096, 4096), (4096, 11008), (11008, 4096)][:1 if args.quick else 3]
MS = [int(m) for m in args.ms.split(",")]
RS = [int(r) for r in args.rs.split(",")]
DT = {"f16": torch.float16, "bf16": torch.bfloat16}


def timed(fn):
    """Median over the rounds of (HIP-event time of `iters` calls) / iters, in microseconds."""
    for _ in range(3):
        fn()
    out = []
    for _ in range(args.rounds):
        torch.cuda.synchronize(dev)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.iters):
            fn()
        e1.record()
        torch.cuda.synchronize(dev)
        out.append(e0.elapsed_time(e1) * 1e3 / args.iters)
    return statistics.median(out)


def peak_of(fn):
    fn()
    torch.cuda.synchronize(dev)
    base = torch.cuda.memory_allocated(dev)
    torch.cuda.reset_peak_memory_stats(dev)
    fn()
    torch.cuda.synchronize(dev)
    return torch.cuda.max_memory_allocated(dev) - base


print("shape          dtype r   M     | step us: torch  fused  ratio | adapter bwd us: torch  fused  ratio | peak MB: torch  fused | rel.diff dA dB dX", flush=True)
slower = []
for K, N in SHAPES:
    for name in args.dtypes.split(","):
        T = DT[name]
        q = bench.make_layer(K, N, dev, dtype=T, seed=7000 + K % 97)
        for r in RS:
            lq = LoraQuantLinear(q, r, 2 * r)
            with torch.no_grad():
                lq.lora_B.weight.copy_(torch.randn(N, r, device=dev, generator=torch.Generator(device=dev).manual_seed(r)) * 0.05)
            for M in MS:
                x = ((torch.rand(M, K, device=dev) - 0.5).to(T)).requires_grad_(True)
                g = ((torch.rand(M, N, device=dev) - 0.5).to(T))

                def step():
                    x.grad = lq.lora_A.weight.grad = lq.lora_B.weight.grad = None
                    lq(x).backward(g)

                # the adapter's backward alone, on what a forward saves
                with torch.no_grad():
                    A16, B16 = lq.lora_A.weight.to(T), lq.lora_B.weight.to(T)
                    u = x.detach() @ A16.t()
                items = [(A16, B16, u, g, lq.scaling, True, True)]
                res = {}
                for flag in (False, True):
                    lq.fused_backward = flag
                    bwd = (lambda: LR._fused_backward(x.detach(), items, True)) if flag else (lambda: LR._torch_backward(x.detach(), items, True))
                    step()
                    grads = (lq.lora_A.weight.grad.clone(), lq.lora_B.weight.grad.clone(), x.grad.clone())
                    res[flag] = (timed(step), timed(bwd), peak_of(step), grads)
                (st, bt, pt, gt), (sf, bf, pf, gf) = res[False], res[True]
                diff = " ".join(f"{float((a.double() - b.double()).norm() / b.double().norm()):.1e}" for a, b in zip(gf, gt))
                print(f"{K:5d}x{N:<5d} int4 {name:4s} {r:<3d} {M:<5d} | {st:9.1f} {sf:7.1f} {sf / st:5.2f} | {bt:9.1f} {bf:7.1f} {bf / bt:5.2f} | "
                      f"{pt / 2**20:8.1f} {pf / 2**20:7.1f} | {diff}", flush=True)
                if bf > bt or sf > st:
                    slower.append((K, N, name, r, M, round(sf / st, 2), round(bf / bt, 2)))
            del lq
        del q
        torch.cuda.empty_cache()
print("fused slower than torch (K, N, dtype, r, M, step ratio, bwd ratio):", slower if slower else "nowhere", flush=True)
