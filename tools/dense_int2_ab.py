#!/usr/bin/env python3
"""Dense 2-bit layers at 5+ rows: the opt-in plan (GPTQ_COPY_ROWS_INT2: the dense forms of the low-bit routed-expert kernels on the decode copy) against the
unflagged plan of the SAME layers in one session -- layer calls on rotating layers (so that weights come from HBM, not from the Infinity Cache) captured in
a hipGraph, as tools/rows_ab.py / panel_ab.py measure.  The flag is toggled in the layers' structs, so both sides read the same tensors.  Every cell is
measured --rounds times per side; the log carries the best time and the repeat spread (max / min - 1) of either side, and closes with the cells where the
flagged plan is slower than the unflagged one by more than the largest repeat spread of the run.
--released 1 repeats the run with release_checkpoint_layout=True, where the unflagged plan pays gptq_unprepack_decode in front of every call that reads rows
(such layers carry GPTQ_COPY_ROWS_INT2_WIDE, as post_init gives it to them: the whole band of the 4-bit twin).  --force-band 1 sets that bit on resident layers
too: the measurement the plain flag's narrower region was cut from.
Usage: python tools/dense_int2_ab.py [--shapes 4096x4096,...] [--gs 128,64] [--dtypes f16,bf16] [--ms 5,8,...] [--released 0,1] [--out profiles/dense_int2_ab.log]"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from autogptq_amd import QuantLinear, _lib  # noqa: E402
from tools.gemv_sweep import run  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default="4096x4096,4096x11008,11008x4096,5120x13824,8192x8192")
ap.add_argument("--gs", default="128,64")
ap.add_argument("--dtypes", default="f16,bf16")
ap.add_argument("--ms", default="5,8,16,32,64,65,128,256,512")
ap.add_argument("--released", default="0,1")
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--rotate-mib", type=int, default=384, help="bytes of decode copies the rotation covers (the Infinity Cache holds 256 MiB)")
ap.add_argument("--max-layers", type=int, default=96)
ap.add_argument("--force-band", type=int, default=0, help="1: GPTQ_COPY_ROWS_INT2_WIDE on resident layers too (the whole band of the 4-bit twin)")
ap.add_argument("--out", default="")
a = ap.parse_args()
dev = torch.device("cuda:0")
log = open(a.out, "w") if a.out else None


def say(s):
    print(s, flush=True)
    if log:
        log.write(s + "\n")
        log.flush()


def make(K, N, gs, dt, seed, released):
    g = torch.Generator(device=dev).manual_seed(seed)
    q = QuantLinear(2, gs, K, N, False, weight_dtype=dt)
    G = -(-K // gs)
    q.qweight = torch.randint(-2**31, 2**31 - 1, (K // 32 * 2, N), dtype=torch.int64, device=dev, generator=g).to(torch.int32)
    q.qzeros = torch.randint(-2**31, 2**31 - 1, (G, N // 32 * 2), dtype=torch.int64, device=dev, generator=g).to(torch.int32)
    q.scales = (0.002 * (1 + 0.1 * torch.rand(G, N, device=dev, generator=g))).to(dt)
    q.g_idx = (torch.arange(K, device=dev, dtype=torch.int32) // gs).contiguous()
    q = q.to(dev)
    q.post_init(release_checkpoint_layout=bool(released), low_bit_rows=False)
    assert q._qweight_tiled is not None
    return q


def flag(layers, on):
    """The opt-in bit of every layer's struct (post_init(low_bit_rows=...) sets the same bit); the per-row-count caches of the module are dropped."""
    for q in layers:
        wide = _lib.COPY_ROWS_INT2_WIDE if (q._released or a.force_band) else 0
        q._layer.tiled_cols = _lib.STRIP_COLS | ((_lib.COPY_ROWS_INT2 | wide) if on else 0)
        q._ws_need, q._ws0_mask, q._rows_need = {}, 0, {}


say("# dense 2-bit layers, 5+ rows: unflagged plan (= the parent's, kernel for kernel) against the opt-in plan on the same tensors; us per layer call, best of "
    f"{a.rounds} x {a.reps} graph replays over rotating layers; spread = max / min - 1 over the rounds"
    + ("; --force-band 1: the whole band of the 4-bit twin on resident layers too" if a.force_band else ""))
warm = [make(4096, 4096, 128, torch.float16, 99, 0)]
xw = (torch.rand(256, 4096, device=dev) - 0.5).half()
for _ in range(3):
    run(warm, xw, None, reps=100)
del warm, xw

cells, spreads = [], []
for rel in map(int, a.released.split(",")):
    for dname in a.dtypes.split(","):
        dt = torch.float16 if dname == "f16" else torch.bfloat16
        for gs in map(int, a.gs.split(",")):
            for shp in a.shapes.split(","):
                K, N = map(int, shp.split("x"))
                n = max(8, min(a.max_layers, -(-(a.rotate_mib << 20) // (K * N // 4))))
                ls = [make(K, N, gs, dt, i, rel) for i in range(n)]
                for M in map(int, a.ms.split(",")):
                    x = (torch.rand(M, K, device=dev) - 0.5).to(dt)
                    t = {False: [], True: []}
                    kern = {}
                    for _ in range(a.rounds):
                        for on in (False, True):
                            flag(ls, on)
                            d = _lib.describe_plan(ls[0]._layer, M)
                            kern[on] = d["kernel"] + ("/lowbit" if d.get("body") == "lowbit" else "")
                            t[on].append(run(ls, x, None, reps=a.reps) * 1e6)
                    flag(ls, False)
                    b0, b1 = min(t[False]), min(t[True])
                    s0, s1 = max(t[False]) / b0 - 1, max(t[True]) / b1 - 1
                    spreads += [s0, s1]
                    same = kern[True] == kern[False]
                    say(f"int2 g{gs} {K}x{N} {dname} released={rel} layers={n} M={M:4d} | unflagged [{kern[False]:12s}] {b0:7.2f} us (spread {s0 * 100:4.1f} %) | "
                        f"flagged [{kern[True]:12s}] {b1:7.2f} us (spread {s1 * 100:4.1f} %) | " + ("same plan" if same else f"{b0 / b1:5.2f}x"))
                    if not same:
                        cells.append((gs, K, N, dname, rel, M, kern[True], b0, b1))
                    del x
                del ls
                torch.cuda.empty_cache()

worst = max(spreads) if spreads else 0.0
say(f"# largest repeat spread of the run: {worst * 100:.1f} %")
lose = [c for c in cells if c[8] > c[7] * (1 + worst)]
say(f"# cells where the planner takes the low-bit forms: {len(cells)}; flagged slower than unflagged by more than that spread: {len(lose)}")
for gs, K, N, dname, rel, M, k, b0, b1 in lose:
    say(f"#   LOSES int2 g{gs} {K}x{N} {dname} released={rel} M={M} [{k}] {b0:.2f} -> {b1:.2f} us ({b0 / b1:.2f}x)")
if cells:
    r = sorted(c[7] / c[8] for c in cells)
    say(f"# unflagged / flagged over those cells: min {r[0]:.2f}x, median {r[len(r) // 2]:.2f}x, max {r[-1]:.2f}x")
