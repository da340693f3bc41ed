"""3-bit routed experts on the grouped path (post_init(low_bit=True)) against the per-expert composition of the same experts (switch off) and against the
4-bit grouped call on the same shape: the Mixtral-8x7B block (E 8, topk 2, H 4096, I 14336), g128 fp16, seeded random routing, T = 1, 64, 2048.  Per T:
median microseconds over hipEvent-timed calls after warm-up, one process, the three calls timed in turn.  Writes profiles/moe_lowbit.log.

    python tools/moe_lowbit_bench.py [--reps 20] [--out profiles/moe_lowbit.log]
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

E, TOPK, H, I = 8, 2, 4096, 14336
TS = (1, 64, 2048)


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
    ap.add_argument("--bits", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "moe_lowbit.log"))
    args = ap.parse_args()
    lines = [f"# tools/moe_lowbit_bench.py: E {E} topk {TOPK} H {H} I {I} g128 fp16, seeded random routing, median of {args.reps} hipEvent-timed calls after 3 "
             f"warm-up calls; grouped{args.bits} = {args.bits}-bit experts with low_bit=True, per_expert{args.bits} = the same experts with the switch off, "
             "grouped4 = 4-bit experts of the same shape"]
    on = make_experts(E, H, I, args.bits, 128, False, torch.float16, seed=1, top_k=TOPK)
    off = make_experts(E, H, I, args.bits, 128, False, torch.float16, seed=1, top_k=TOPK)
    q4 = make_experts(E, H, I, 4, 128, False, torch.float16, seed=1, top_k=TOPK)
    on.post_init(low_bit=True)
    for T in TS:
        x = (torch.rand((T, H), generator=torch.Generator().manual_seed(T)) - 0.5).half().cuda()
        idx, w = _routing(T, E, TOPK, T)
        assert on.plan(T)["path"] == "grouped" and off.plan(T)["path"] == "per_expert" and q4.plan(T)["path"] == "grouped"
        with torch.no_grad():
            tl = _time(lambda: moe_forward(on, x, idx, w), args.reps)
            tp = _time(lambda: _per_expert(off, x, idx, w), args.reps)
            t4 = _time(lambda: moe_forward(q4, x, idx, w), args.reps)
        lines.append(f"T={T} grouped{args.bits}_us={tl:.1f} per_expert{args.bits}_us={tp:.1f} grouped4_us={t4:.1f} "
                     f"ratio_{args.bits}bit_over_4bit={tl / t4:.3f} speedup_vs_per_expert={tp / tl:.2f}")
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
