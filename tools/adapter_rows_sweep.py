#!/usr/bin/env python3
"""Per-row adapter banks (LoraBankQuantLinear: one routing per step, a down and an up launch per layer) against the host loop over adapters they replace
and against the base layer alone.

The host loop is what serves a mixed batch without the bank kernels: per adapter present in the batch an ``index_select`` of its rows of x and of the base
output, a ``gptq_lora_apply`` on the subset and an ``index_copy`` back.  Here the row sets are fixed tensors, so the loop captures into a graph at all --
in a server they change every step and the loop cannot be one hipGraph; the figure below is its floor.

Per M and number of distinct adapters three hipGraphs are captured over the SAME rotation of distinct 4096 x 4096 layers (together beyond the Infinity
Cache, so every launch reads its weights from HBM: BASELINE.md) -- one call per layer -- and timed by HIP events, alternating the forms in one process, min
over `--rounds` rounds.  The bank form's graph holds ONE routing launch for the whole rotation (one routing serves every layer of a step).  The figure that
matters is the adapter's overhead: `bank - base` against `loop - base`.
usage: python tools/adapter_rows_sweep.py [--ms 8,16,64] [--present 1,4,8] [--r 16] [--rounds 3] [--quick]"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from autogptq_amd import AdapterRouting, LoraBankQuantLinear, LoraQuantLinear  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--ms", default="8,16,64")
ap.add_argument("--present", default="1,4,8", help="distinct adapters in the batch")
ap.add_argument("--r", type=int, default=16)
ap.add_argument("--slots", type=int, default=8)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--reps", type=int, default=5, help="replays per timed window")
ap.add_argument("--cold-mb", type=int, default=320, help="packed weights of one rotation")
ap.add_argument("--quick", action="store_true", help="two layers per rotation")
args = ap.parse_args()
dev = torch.device("cuda:0")
K = N = 4096
MS = [int(m) for m in args.ms.split(",")]
PRESENT = [int(p) for p in args.present.split(",")]
R, SLOTS = args.r, args.slots


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


def measure(forms, calls):
    best = {k: float("inf") for k in forms}
    for _ in range(args.rounds):
        for k, g in forms.items():
            best[k] = min(best[k], us(g, calls))
    return best


class HostLoop:
    """One LoraQuantLinear per slot around the same base (fp16 masters: the kernels read the parameters themselves), applied adapter by adapter."""

    def __init__(self, bank: LoraBankQuantLinear):
        self.base = bank.base
        self.singles = []
        for s in range(bank.num_slots):
            lq = LoraQuantLinear(bank.base, bank.r, float(bank.scales[s]) * bank.r, adapter_dtype=torch.float16).eval()
            with torch.no_grad():
                lq.lora_A.weight.copy_(bank.lora_A_bank[s])
                lq.lora_B.weight.copy_(bank.lora_B_bank[s])
            self.singles.append(lq)

    def __call__(self, x, rows_of):
        y = self.base(x)
        for s, rows in rows_of.items():
            lq = self.singles[s]
            ys = y.index_select(0, rows)
            lq._adapter_(ys, x.index_select(0, rows), *lq._kernel_weights(x.dtype))
            y.index_copy_(0, rows, ys)
        return y


n = 2 if args.quick else max(4, -(-(args.cold_mb << 20) // (K * N // 2)))
bases = [bench.make_layer(K, N, dev, seed=9000 + i) for i in range(n)]
banks = []
for i, q in enumerate(bases):
    b = LoraBankQuantLinear(q, R, SLOTS).eval()
    g = torch.Generator().manual_seed(i)
    for s in range(SLOTS):
        b.load_slot(s, torch.randn(R, K, generator=g) / K ** 0.5, torch.randn(N, R, generator=g) * 0.05, 2.0 * R)
    banks.append(b)
loops = [HostLoop(b) for b in banks]
routing = AdapterRouting(max(MS), SLOTS, dev)
for b in banks:
    b.routing = routing

print(f"{K}x{N} int4 g128 f16, r={R}, {SLOTS} slots, {n} layers per rotation; us per layer call")
for M in MS:
    x = (torch.rand(M, K, device=dev) - 0.5).half()
    for present in PRESENT:
        if present > min(M, SLOTS):
            continue
        ids = torch.arange(M) % present
        rows_of = {s: torch.nonzero(ids == s).flatten().to(dev) for s in range(present)}
        routing.set(ids)

        def bank_form():
            routing.set()
            return [b(x) for b in banks]

        forms = {"base": graph_of(lambda: [q(x) for q in bases]), "bank": graph_of(bank_form), "loop": graph_of(lambda: [l(x, rows_of) for l in loops])}
        best = measure(forms, n)
        with torch.no_grad():
            same = torch.equal(banks[0](x), loops[0](x, rows_of))
        over_b, over_l = best["bank"] - best["base"], best["loop"] - best["base"]
        print(f"M={M:<3d} adapters={present}  base {best['base']:8.2f} us  bank {best['bank']:8.2f}  loop {best['loop']:8.2f}   overhead: bank {over_b:7.2f}  "
              f"loop {over_l:7.2f}  ratio {over_b / over_l if over_l > 0 else float('nan'):5.2f}  {'ok' if over_b < over_l else 'HOST LOOP WINS'}  "
              f"bit-identical {same}", flush=True)
        del forms
