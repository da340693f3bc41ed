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
ap.add_argument("--on-copy", action="store_true", help="with --launch: the kernel on the decode copy (post_init(grad_on_copy=True))")
ap.add_argument("--ab", action="store_true", help="rows kernel against the kernel on the decode copy, same session (profiles/grad_copy_ab.log)")
ap.add_argument("--ab-rounds", type=int, default=9)
ap.add_argument("--ab-bits", default="4:128", help="with --ab: WIDTH:GROUP_SIZE of the layers; 2, 3, 8 run under grad_on_copy=\"any_bits\" (profiles/grad_copy_bits_ab.log)")
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


def ab():
    """--ab: the rows kernel (gptq_grad_input) against the kernel on the decode copy (gptq_grad_input_ex, GPTQ_GRAD_ON_COPY) in ONE session, beside (a) dense and
    (b) deq + mm, on the four layers of DESIGN 4.7's table at M = 64 / 512 / 2048; for the plain layers also RELEASED (one copy on the device): QuantLinear.grad_input
    without the flag (rebuild pass + rows kernel) and with it.  One call per timing, HIP events around it, a 512 MiB write in front of every call (weights, dY
    and dX out of the caches); the forms alternate inside each of --ab-rounds rounds; reported: median us and the spread (min .. max) of the rounds."""
    flush = torch.empty(512 << 20, dtype=torch.uint8, device=dev)
    bits, gs = (int(v) for v in args.ab_bits.split(":"))
    on = True if bits == 4 else "any_bits"
    F = _lib.grad_copy_flags(on)
    st = lambda: torch.cuda.current_stream().cuda_stream

    def one(fn):
        flush.fill_(1)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3

    layers = [(4096, 4096, torch.float16, False), (4096, 11008, torch.float16, False), (11008, 4096, torch.float16, False), (4096, 11008, torch.bfloat16, True)]
    for K, N, dtype, act in layers:
        q = bench.make_layer(K, N, dev, bits=bits, gs=gs, act_order=act, dtype=dtype, seed=K + N)
        q.post_init(grad_on_copy=on)
        W16 = q.dequantize()
        rel = {}
        if not act:                                        # (act-order layers keep their rows: nothing to release)
            for flag in (False, True):
                rel[flag] = bench.make_layer(K, N, dev, bits=bits, gs=gs, dtype=dtype, seed=K + N)
                rel[flag].post_init(release_checkpoint_layout=True, grad_on_copy=on if flag else False)
        for M in (64, 512, 2048):
            dy = (torch.randn(M, N, device=dev) * 0.5).to(dtype)
            dx, dxc, ref = (torch.empty(M, K, dtype=dtype, device=dev) for _ in range(3))
            forms = {
                "rows": lambda: _lib.check(lib.gptq_grad_input(q._layer_ref, dy.data_ptr(), dx.data_ptr(), M, 0, st())),
                "copy": lambda: _lib.check(lib.gptq_grad_input_ex(q._layer_ref, dy.data_ptr(), dxc.data_ptr(), M, 0, F, st())),
                "dense": lambda: torch.matmul(dy, W16.t(), out=ref),
                "deq+mm": lambda: torch.matmul(dy, q.dequantize().t()),
            }
            if rel:
                forms["released rebuild+rows"] = lambda: rel[False].grad_input(dy)
                forms["released copy"] = lambda: rel[True].grad_input(dy)
            assert q.describe_grad_plan(M).startswith("kernel=grad_copy") and (not rel or rel[True].describe_grad_plan(M).startswith("kernel=grad_copy"))
            t = {k: [] for k in forms}
            for fn in forms.values():
                fn()                                       # warm-up of every form and shape
            for _ in range(args.ab_rounds):
                for k, fn in forms.items():
                    t[k].append(one(fn))
            err = float((dxc.float() - ref.float()).abs().max() / ref.float().abs().max().clamp_min(1e-30))
            med = {k: sorted(v)[len(v) // 2] for k, v in t.items()}
            cells = "  ".join(f"{k} {med[k]:7.1f} ({min(v):.1f} .. {max(v):.1f})" for k, v in t.items())
            gap = med["rows"] - med["copy"]
            spread = max(max(t[k]) - min(t[k]) for k in ("rows", "copy"))
            print(f"{K:5d}x{N:<5d} {str(dtype)[6:]:8s} int{bits} g{gs} {'act' if act else 'seq'} M={M:5d} [{q.describe_grad_plan(M)}]  {cells}  rows/copy {med['rows'] / med['copy']:.2f} "
                  f"({'beyond' if gap > spread else 'WITHIN'} the repeat spread)  copy {2.0 * M * N * K / med['copy'] / 1e-6 / PEAK:.2f} of peak  "
                  f"same bits as rows: {bool(torch.equal(dx, dxc))}  rel.err vs dense {err:.1e}", flush=True)


if args.ab:
    ab()
    sys.exit(0)

if args.launch:
    K, N, M, *rest = (int(v) for v in args.launch.split(","))
    q = bench.make_layer(K, N, dev, act_order=bool(rest and rest[0]), seed=1)
    if args.on_copy:
        q.post_init(grad_on_copy=True)
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
