"""The prefill path of the routed experts (post_init(prefill=True): gptq_moe_prefill_forward, 64-row panels on the decode copy) against the grouped path and the
per-expert composition of the SAME experts with the flag off, on the Mixtral-8x7B block (E 8, topk 2, H 4096, I 14336) and the 60-expert block (E 60, topk 4,
H 2048, I 1408), int4 g128 fp16, seeded random routing, T = 128, 256, 1024, 2048.  Per point: median microseconds of hipEvent-timed calls after warm-up, one
process, and the largest |prefill - grouped| over the outputs; rows/expert = T topk / E.  Writes profiles/moe_prefill.log.

    python tools/moe_prefill_bench.py [--reps 20] [--out profiles/moe_prefill.log]
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

BLOCKS = (("mixtral", 8, 2, 4096, 14336), ("e60", 60, 4, 2048, 1408))
TS = (128, 256, 1024, 2048)


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "moe_prefill.log"))
    args = ap.parse_args()
    lines = [f"# tools/moe_prefill_bench.py: int4 g128 fp16, seeded random routing, median of {args.reps} hipEvent-timed calls after 3 warm-up calls, one process; "
             "prefill = post_init(prefill=True), grouped / per_expert = the same experts with the flag off; maxdiff = max |prefill - grouped| over the outputs"]
    for name, E, topk, H, I in BLOCKS:
        q = make_experts(E, H, I, 4, 128, False, torch.float16, seed=1, top_k=topk)
        cases = []
        for T in TS:
            x = (torch.rand((T, H), generator=torch.Generator().manual_seed(T)) - 0.5).half().cuda()
            cases.append((T, x) + _routing(T, E, topk, T))
        q.post_init(prefill=True)
        tp, outs = {}, {}
        with torch.no_grad():
            for T, x, idx, w in cases:
                assert q.plan(T)["path"] == "prefill", q.plan(T)
                tp[T] = _time(lambda: moe_forward(q, x, idx, w), args.reps)
                outs[T] = moe_forward(q, x, idx, w).float()
        q.post_init()
        with torch.no_grad():
            for T, x, idx, w in cases:
                assert q.plan(T)["path"] == "grouped", q.plan(T)
                tg = _time(lambda: moe_forward(q, x, idx, w), args.reps)
                te = _time(lambda: _per_expert(q, x, idx, w), args.reps)
                diff = float((outs[T] - moe_forward(q, x, idx, w).float()).abs().max())
                lines.append(f"{name} E={E} topk={topk} H={H} I={I} T={T} rows/expert={T * topk / E:.1f} prefill_us={tp[T]:.1f} grouped_us={tg:.1f} "
                             f"per_expert_us={te:.1f} grouped/prefill={tg / tp[T]:.2f} per_expert/prefill={te / tp[T]:.2f} maxdiff={diff:.3e}")
                print(lines[-1], flush=True)
        del q, cases, outs
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
