#!/usr/bin/env python3
"""The opt-in int8-activation path (W4A8: gptq_forward_a8 = act_quant_kernel + gemm_a8_kernel, csrc/act_int8.hip) against the default plan of the SAME layers
in one session -- layer calls on rotating layers (so that weights come from HBM, not from the Infinity Cache) captured in a hipGraph, as tools/rows_ab.py and
dense_int2_ab.py measure.  The switch is toggled on the modules (QuantLinear._a8_rows: what post_init(act_int8=True) sets), both sides read the same tensors,
and the quantise launch is counted in: a cell is the time of one whole QuantLinear.forward call.  Every cell is measured --rounds times per side, alternating;
the log carries the best time and the repeat spread (max / min - 1) of either side, the rate of the int8 call in TOP/s (2 M K N / time), and closes with the
cells where the int8 path is slower than the default plan by more than the largest repeat spread of the run.  Nothing depends on it winning: the path is off
by default and changes numerics.
Usage: python tools/act_int8_ab.py [--shapes 4096x4096,...] [--ms 256,512,2048,4096] [--act 0,1] [--gs 128] [--dtype f16] [--out profiles/act_int8_ab.log]"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from autogptq_amd import QuantLinear, _lib  # noqa: E402
from tools.gemv_sweep import run  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default="4096x4096,4096x11008,11008x4096")
ap.add_argument("--ms", default="256,512,2048,4096")
ap.add_argument("--act", default="0,1")
ap.add_argument("--gs", type=int, default=128)
ap.add_argument("--dtype", default="f16", choices=["f16", "bf16"])
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--rotate-mib", type=int, default=384, help="bytes of decode copies the rotation covers (the Infinity Cache holds 256 MiB)")
ap.add_argument("--max-layers", type=int, default=48)
ap.add_argument("--out", default="")
a = ap.parse_args()
dev = torch.device("cuda:0")
dt = torch.float16 if a.dtype == "f16" else torch.bfloat16
log = open(a.out, "w") if a.out else None


def say(s):
    print(s, flush=True)
    if log:
        log.write(s + "\n")
        log.flush()


def make(K, N, act, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    q = QuantLinear(4, a.gs, K, N, False, weight_dtype=dt)
    G = -(-K // a.gs)
    q.qweight = torch.randint(-2**31, 2**31 - 1, (K // 8, N), dtype=torch.int64, device=dev, generator=g).to(torch.int32)
    q.qzeros = torch.randint(-2**31, 2**31 - 1, (G, N // 8), dtype=torch.int64, device=dev, generator=g).to(torch.int32)
    q.scales = (0.002 * (1 + 0.1 * torch.rand(G, N, device=dev, generator=g))).to(dt)
    gi = torch.arange(K, device=dev, dtype=torch.int32) // a.gs
    q.g_idx = (gi[torch.randperm(K, device=dev, generator=g)] if act else gi).contiguous()
    q = q.to(dev)
    q.post_init(act_int8=True, act_int8_min_rows=1)
    assert q._a8_rows == 1, "the layer was declined"
    return q


def flag(layers, on):
    for q in layers:
        q._a8_rows = 1 if on else 0
        q._ws0_mask = 0


say(f"# W4A8 (opt-in) against the default plan on the same 4-bit g{a.gs} {a.dtype} layers; us per QuantLinear.forward call (int8 side: quantise + GEMM, two "
    f"launches), best of {a.rounds} x {a.reps} graph replays over rotating layers; spread = max / min - 1 over the rounds")
warm = [make(4096, 4096, False, 99)]
xw = (torch.rand(256, 4096, device=dev) - 0.5).to(dt)
for on in (False, True, False, True):
    flag(warm, on)
    run(warm, xw, None, reps=50)
del warm, xw

cells, spreads = [], []
for act in map(int, a.act.split(",")):
    for shp in a.shapes.split(","):
        K, N = map(int, shp.split("x"))
        n = max(8, min(a.max_layers, -(-(a.rotate_mib << 20) // (K * N // 2))))
        ls = [make(K, N, bool(act), i) for i in range(n)]
        for M in map(int, a.ms.split(",")):
            x = (torch.rand(M, K, device=dev) - 0.5).to(dt)
            t = {False: [], True: []}
            for _ in range(a.rounds):
                for on in (False, True):
                    flag(ls, on)
                    t[on].append(run(ls, x, None, reps=a.reps) * 1e6)
            flag(ls, False)
            kern = _lib.describe_plan(ls[0]._layer, M)["kernel"]
            b0, b1 = min(t[False]), min(t[True])
            s0, s1 = max(t[False]) / b0 - 1, max(t[True]) / b1 - 1
            spreads += [s0, s1]
            cells.append((act, K, N, M, kern, b0, b1))
            say(f"int4 g{a.gs} {K}x{N} {a.dtype} {'act-order' if act else 'plain    '} layers={n} M={M:4d} | default [{kern:9s}] {b0:8.2f} us (spread {s0 * 100:4.1f} %) "
                f"{2e-6 * M * K * N / b0:6.0f} TFLOP/s | act_int8 {b1:8.2f} us (spread {s1 * 100:4.1f} %) {2e-6 * M * K * N / b1:6.0f} TOP/s | {b0 / b1:5.2f}x")
            del x
        del ls
        torch.cuda.empty_cache()

worst = max(spreads) if spreads else 0.0
say(f"# largest repeat spread of the run: {worst * 100:.1f} %")
lose = [c for c in cells if c[6] > c[5] * (1 + worst)]
say(f"# cells: {len(cells)}; act_int8 slower than the default plan by more than that spread: {len(lose)}")
for act, K, N, M, k, b0, b1 in lose:
    say(f"#   LOSES {K}x{N} {'act-order' if act else 'plain'} M={M} [{k}] {b0:.2f} -> {b1:.2f} us ({b0 / b1:.2f}x)")
if cells:
    r = sorted(c[5] / c[6] for c in cells)
    say(f"# default / act_int8 over all cells: min {r[0]:.2f}x, median {r[len(r) // 2]:.2f}x, max {r[-1]:.2f}x")
