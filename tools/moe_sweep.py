"""Grouped routed-expert path (gptq_moe_forward) against the per-expert composition of QuantLinear calls, on the Mixtral-8x7B block (E 8, topk 2,
H 4096, I 14336) and a 60-expert shape (topk 4, H 2048, I 1408), 4-bit g128 fp16, seeded random routing.  Per T: median microseconds over hipEvent-timed
calls after warm-up, the expert weight bytes touched / time as a fraction of 8 TB/s, FLOP / time as a fraction of 2.5 PF.  Writes profiles/moe_sweep.log.

    python tools/moe_sweep.py [--reps 20] [--out profiles/moe_sweep.log]
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from autogptq_amd.moe import _per_expert, moe_forward  # noqa: E402
from test_gpu_moe import _routing, make_experts  # noqa: E402

SHAPES = {"mixtral8x7b": (8, 2, 4096, 14336), "e60": (60, 4, 2048, 1408)}
TS = (1, 2, 4, 16, 64, 256, 1024, 2048)


def _time(fn, reps):
    for _ in range(3):
        fn()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    ts.sort()
    return ts[len(ts) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "moe_sweep.log"))
    ap.add_argument("--per-expert-max-t", type=int, default=2048)
    args = ap.parse_args()
    lines = [f"# tools/moe_sweep.py: 4-bit g128 fp16 experts, median of {args.reps} hipEvent-timed calls; bytes = packed weights + scales / zeros of the hit "
             "experts; frac_bw = bytes / t / 8 TB/s, frac_pf = 2 * 3 * H * I * T * topk / t / 2.5 PF"]
    for name, (E, topk, H, I) in SHAPES.items():
        q = make_experts(E, H, I, 4, 128, False, torch.float16, seed=1, top_k=topk)
        per_expert_bytes = 3 * (H * I // 2 + (H // 128) * I * 2 + (H // 128) * I // 2)     # ~ (4-bit words + fp16 scales + zeros) per projection
        for T in TS:
            x = (torch.rand((T, H), generator=torch.Generator().manual_seed(T)) - 0.5).half().cuda()
            idx, w = _routing(T, E, topk, T)
            hit = int(torch.unique(idx).numel())
            with torch.no_grad():
                tg = _time(lambda: moe_forward(q, x, idx, w), args.reps)
                tp = _time(lambda: _per_expert(q, x, idx, w), max(3, args.reps // 4)) if T <= args.per_expert_max_t else float("nan")
            byt = hit * per_expert_bytes
            flop = 2.0 * 3 * H * I * T * topk
            plan = q.plan(T, topk)
            lines.append(f"{name} T={T} hit={hit} grouped_us={tg:.1f} per_expert_us={tp:.1f} speedup={tp / tg:.2f} frac_bw={byt / (tg * 1e-6) / 8e12:.3f} "
                         f"frac_pf={flop / (tg * 1e-6) / 2.5e15:.4f} bm={plan['bm']} tiles={plan['tiles']} ksplit={plan['ksplit']}")
            print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
