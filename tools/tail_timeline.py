#!/usr/bin/env python3
"""Per-wave s_memtime timeline of gemv_tiled_kernel on the four launches of a Llama-7B decoder block (q|k|v as one launch, o, gate|up as one launch, down;
M = 1, fp16, HBM-cold rotating layers inside a hipGraph, as tools/tiled_sweep.py builds them).

Needs the lab library: tools/ab_tiled.sh STAMPS -DGPTQ_TILED_STAMPS, then
    GPTQ_MI355X_LIB=tools/libgptq_STAMPS.so python tools/tail_timeline.py
Every wave of four workgroups (first, second, middle, last of the grid) stamps: 0 entry, 1 first weight loads issued, 2 staging barrier passed, 3 last weight
chunk landed, 4 K loop left, 5 reduction barrier passed, 6 output store issued (shader cycles), and s_memrealtime (100 MHz) at entry and exit.  The counters
are per XCD: only differences on one wave's own clock are formed.  Printed: the median over the stamped waves of each span, in cycles and in ns at the clock
the two counters give.  The stamps cost time themselves (each is read at once: a scalar round trip); the same stamps in two builds compare, the absolute
spans are upper bounds."""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench import make_layer
from autogptq_amd.qlinear_mi355x import forward_multi

SPANS = [("entry -> first weight loads issued", 0, 1), ("entry -> staging barrier passed", 0, 2), ("first loads issued -> last chunk landed", 1, 3),
         ("last chunk landed -> K loop left", 3, 4), ("K loop left -> reduction barrier passed", 4, 5), ("reduction barrier -> store issued", 5, 6),
         ("last chunk landed -> store issued", 3, 6), ("entry -> store issued", 0, 6)]


def main():
    dev = torch.device("cuda:0")
    K0, I = 4096, 11008
    launches = [("q|k|v", K0, (K0, K0, K0)), ("o", K0, (K0,)), ("gate|up", K0, (I, I)), ("down", I, (K0,))]
    print(f"# library: {os.environ.get('GPTQ_MI355X_LIB', 'autogptq_amd/libgptq_mi355x.so')}")
    for name, K, Ns in launches:
        per = K * sum(Ns) // 2
        ng = max(4, min(48, (400 << 20) // per))                                  # > 256 MiB of weights: every launch reads HBM
        groups = [[make_layer(K, n, dev, seed=100 * gi + i) for i, n in enumerate(Ns)] for gi in range(ng)]
        x = (torch.rand(1, K, device=dev) - 0.5).half()
        stamps = torch.zeros(4 * 16 * 16, dtype=torch.int64, device=dev)
        os.environ["GPTQ_TILED_STAMPS_PTR"] = hex(stamps.data_ptr())
        run = lambda: [forward_multi(grp, x) for grp in groups]
        with torch.no_grad():
            run()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g), torch.no_grad():
            keep = run()
        rows = {k: [] for k in range(len(SPANS))}
        clocks, nw = [], 0
        for _ in range(5):                                                        # the buffer holds the last launch of a replay: five replays, five samples per wave
            g.replay()
            torch.cuda.synchronize()
            st = stamps.cpu().view(4, 16, 16)
            for b in range(4):
                for w in range(16):
                    s = st[b, w].tolist()
                    if s[0] == 0 or s[6] == 0:
                        continue
                    nw += 1
                    for k, (_, a, z) in enumerate(SPANS):
                        rows[k].append(s[z] - s[a])
                    if s[8] > s[7]:
                        clocks.append((s[6] - s[0]) / ((s[8] - s[7]) * 10.0))       # cycles per ns
        del os.environ["GPTQ_TILED_STAMPS_PTR"]
        ghz = statistics.median(clocks) if clocks else float("nan")
        print(f"== {name}: K={K} N={Ns}, {ng} rotating groups, {nw} wave samples, clock ~{ghz:.2f} GHz")
        for k, (label, _, _) in enumerate(SPANS):
            v = sorted(rows[k])
            if not v:
                continue
            med = statistics.median(v)
            print(f"   {label:44s} median {med:8.0f} cyc = {med / ghz:7.0f} ns   (min {v[0]:6d}, max {v[-1]:6d})")
        sys.stdout.flush()
        del groups, keep, g
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
