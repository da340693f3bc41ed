#!/usr/bin/env python3
"""gptq_grad_input (dX = dY . W^T on the packed weights) against (a) torch.matmul(dY, W16.t()) on a weight dequantised once -- the dense bound -- and
(b) dequantize() + matmul per call -- the reference's training route (qlinear_cuda_old.py:291-355).  Each form is captured in a hipGraph of `--reps`
launches and timed by HIP events, min over `--rounds` interleaved rounds; every kernel output is checked against (a) (max |diff| / max |a|).
usage: python tools/grad_input_sweep.py [--ms 512,1024,2048,4096] [--quick]"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from autogptq_amd import _lib  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--ms", default="512,1024,2048,4096")
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--quick", action="store_true", help="fp16 4-bit g128 sequential on the 7B shapes only")
ap.add_argument("--launch", default="", help="K,N,M[,act]: only 20 plain launches of the fp16 4-bit g128 kernel (a target for rocprofv3 --pmc)")
args = ap.parse_args()
dev = torch.device("cuda:0")
lib = _lib.load()
PEAK = 2.5e15

SHAPES = [("7B", 4096, 4096), ("7B", 4096, 11008), ("7B", 11008, 4096), ("13B", 5120, 5120), ("13B", 5120, 13824), ("13B", 13824, 5120)]
VARIANTS = [(torch.float16, 4, 128, False), (torch.float16, 4, 128, True), (torch.bfloat16, 4, 128, False), (torch.bfloat16, 4, 128, True)]
EXTRA = [(torch.float16, 3, 32, False), (torch.float16, 8, 32, False)]          # on 4096 x 11008 only
if args.quick:
    SHAPES, VARIANTS, EXTRA = SHAPES[:3], VARIANTS[:1], []


def graph_of(fn):
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(args.reps):
            fn()
    return g


def us(g):
    bench.settle(g, dev)
    _, evt = bench.time_graph(g, 1, dev)
    return evt / args.reps * 1e6


def run(fam, K, N, dtype, bits, gs, act):
    q = bench.make_layer(K, N, dev, bits=bits, gs=gs, act_order=act, dtype=dtype, seed=K + N + bits)
    W16 = q.dequantize()
    for M in (int(m) for m in args.ms.split(",")):
        dy = (torch.randn(M, N, device=dev) * 0.5).to(dtype)
        dx = torch.empty(M, K, dtype=dtype, device=dev)
        ref = torch.empty(M, K, dtype=dtype, device=dev)
        forms = {
            "kernel": graph_of(lambda: _lib.check(lib.gptq_grad_input(q._layer_ref, dy.data_ptr(), dx.data_ptr(), M, 0, torch.cuda.current_stream().cuda_stream))),
            "dense": graph_of(lambda: torch.matmul(dy, W16.t(), out=ref)),
            "deq+mm": graph_of(lambda: torch.matmul(dy, q.dequantize().t())),
        }
        best = {k: float("inf") for k in forms}
        for _ in range(args.rounds):
            for k, g in forms.items():
                best[k] = min(best[k], us(g))
        got = q.grad_input(dy)
        torch.matmul(dy, W16.t(), out=ref)
        err = float((got.float() - ref.float()).abs().max() / ref.float().abs().max().clamp_min(1e-30))
        flop = 2.0 * M * N * K
        print(f"{fam:4s} {K:5d}x{N:<5d} {str(dtype)[6:]:8s} int{bits} g{gs:<3d} {'act' if act else 'seq'} M={M:5d}  kernel {best['kernel']:8.1f} us "
              f"({flop / best['kernel'] / 1e-6 / PEAK:.2f} of peak)  dense {best['dense']:8.1f}  deq+mm {best['deq+mm']:8.1f}  "
              f"kernel/dense {best['kernel'] / best['dense']:.2f}  rel.err {err:.1e}", flush=True)
        del forms


if args.launch:
    K, N, M, *rest = (int(v) for v in args.launch.split(","))
    q = bench.make_layer(K, N, dev, act_order=bool(rest and rest[0]), seed=1)
    dy = (torch.randn(M, N, device=dev) * 0.5).half()
    for _ in range(20):
        q.grad_input(dy)
    torch.cuda.synchronize()
    sys.exit(0)

for dtype, bits, gs, act in VARIANTS:
    for fam, K, N in SHAPES:
        run(fam, K, N, dtype, bits, gs, act)
for dtype, bits, gs, act in EXTRA:
    run("7B", 4096, 11008, dtype, bits, gs, act)
