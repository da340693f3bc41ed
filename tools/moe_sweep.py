"""Grouped routed-expert path (gptq_moe_forward) against the per-expert composition of QuantLinear calls, on the Mixtral-8x7B block (E 8, topk 2,
H 4096, I 14336) and a 60-expert shape (topk 4, H 2048, I 1408), 4-bit g128 fp16, seeded random routing.  Per T: median microseconds over hipEvent-timed
calls after warm-up, the expert weight bytes touched / time as a fraction of 8 TB/s, FLOP / time as a fraction of 2.5 PF.  Writes profiles/moe_sweep.log.

    python tools/moe_sweep.py [--reps 20] [--out profiles/moe_sweep.log]

--decode: the decode path (gptq_moe_decode_forward, experts with a decode copy) against the grouped path and the per-expert composition on experts WITHOUT
a copy (what a plain post_init gives), T = 1, 2, 4 on both shapes, in one process: per repeat the three paths are timed one after the other (alternating),
each as CALL time (one event pair around --reps back-to-back eager calls) and, for the two one-call paths, as the time of a captured graph replayed
(kernel-side time); reported are the median over --repeats repeats and their spread (min .. max).  Two routings:
"fixed" (the same experts every call: the two hit experts of the Mixtral block are 176 MB and fit the 256 MiB Infinity Cache, a warm-cache number) and
"rotated" (the expert indices advance by one from call to call, so all E experts are walked).  frac_bw = bytes of the hit experts / time / 8 TB/s.
Writes profiles/moe_decode_sweep.log.  --trace-only T: only run a few decode calls at T tokens on the Mixtral block (for a rocprofv3 --kernel-trace run).

    python tools/moe_sweep.py --decode [--reps 20] [--repeats 5] [--out profiles/moe_decode_sweep.log]

--batch: the batch path (gptq_moe_batch_forward, experts post-initialised with batch=True) against the grouped path and the per-expert composition on experts
WITHOUT a copy, T = 5, 8, 16, 32, 64 on both shapes, in the protocol of --decode (one process, the paths timed in turn per repeat, eager CALL time and
graph-replayed time, median of --repeats repeats [min .. max]).  Routing: rotated -- eight routings whose expert indices advance by ceil(E / 8) from call to
call, so all E experts are walked.  frac_bw = bytes of the hit experts / graph time / 8 TB/s.  Writes profiles/moe_batch_sweep.log.
--trace-only T --batch: a few batch calls at T tokens on the Mixtral block (for a rocprofv3 --kernel-trace run).

    python tools/moe_sweep.py --batch [--reps 20] [--repeats 5] [--out profiles/moe_batch_sweep.log]
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


def _time_rot(fn, routings, reps):
    """CALL time in microseconds: ONE pair of hipEvents around a batch of `reps` back-to-back calls of fn(idx, w), divided by reps -- the queue stays full, so this
    is the device time per call unless the host enqueue is slower than the kernels (then it is the enqueue time; the per-kernel split comes from the
    rocprofv3 kernel trace).  The routing advances from call to call (one entry: fixed routing)."""
    n = len(routings)
    for k in range(3):
        fn(*routings[k % n])
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for k in range(reps):
        fn(*routings[(3 + k) % n])
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / reps


def _time_graph(fn, x_routings, reps):
    """KERNEL-side time of the decode path: the call captured once into a graph per routing, the graphs replayed in turn (no host work per call but the replay)."""
    graphs = []
    for (i, ww) in x_routings:
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            fn(i, ww)
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            fn(i, ww)
        graphs.append(g)
    for g in graphs[:3]:
        g.replay()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for k in range(reps):
        graphs[k % len(graphs)].replay()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / reps


def decode_sweep(args):
    from test_gpu_moe_decode import make_experts as make_dc
    lines = [f"# tools/moe_sweep.py --decode: 4-bit g128 fp16 experts; per repeat the paths are timed in turn (decode, decode_graph, grouped, grouped_graph, per_expert); "
             f"*_us = CALL time: one event pair around {args.reps} back-to-back eager calls / {args.reps}; *_graph_us = the same call captured in a hipGraph per routing and "
             f"replayed (kernel-side time); value = median over {args.repeats} repeats [min .. max]; decode = experts with a decode copy, grouped / per_expert = experts "
             "post-initialised without one; bytes = packed weights + scales / zeros of the hit experts; frac_bw = bytes / graph time / 8 TB/s"]
    for name, (E, topk, H, I) in SHAPES.items():
        qd = make_dc(E, H, I, 4, 128, False, torch.float16, seed=1, top_k=topk, decode_copy=True)
        qp = make_dc(E, H, I, 4, 128, False, torch.float16, seed=1, top_k=topk, decode_copy=False)
        per_expert_bytes = 3 * (H * I // 2 + (H // 128) * I * 2 + (H // 128) * I // 2)
        for T in (1, 2, 4):
            x = (torch.rand((T, H), generator=torch.Generator().manual_seed(T)) - 0.5).half().cuda()
            idx, w = _routing(T, E, topk, T)
            hit = int(torch.unique(idx).numel())
            assert qd.plan(T, topk)["path"] == "decode" and qp.plan(T, topk)["path"] == "grouped"
            for mode, routings in (("fixed", [(idx, w)]), ("rotated", [((idx + k) % E, w) for k in range(E)])):
                fd, fg = (lambda i, ww: moe_forward(qd, x, i, ww)), (lambda i, ww: moe_forward(qp, x, i, ww))
                fns = {"decode": lambda: _time_rot(fd, routings, args.reps), "decode_graph": lambda: _time_graph(fd, routings, args.reps),
                       "grouped": lambda: _time_rot(fg, routings, args.reps), "grouped_graph": lambda: _time_graph(fg, routings, args.reps),
                       "per_expert": lambda: _time_rot(lambda i, ww: _per_expert(qp, x, i, ww), routings, max(5, args.reps // 2))}
                got = {k: [] for k in fns}
                with torch.no_grad():
                    for _ in range(args.repeats):
                        for k, fn in fns.items():
                            got[k].append(fn())
                med = {k: sorted(v)[len(v) // 2] for k, v in got.items()}
                byt = hit * per_expert_bytes
                lines.append(f"{name} T={T} hit={hit} routing={mode} " + " ".join(f"{k}_us={med[k]:.1f}[{min(got[k]):.1f}..{max(got[k]):.1f}]" for k in fns)
                             + f" decode_frac_bw={byt / (med['decode_graph'] * 1e-6) / 8e12:.3f} grouped_frac_bw={byt / (med['grouped_graph'] * 1e-6) / 8e12:.3f}"
                             + f" call_speedup_vs_grouped={med['grouped'] / med['decode']:.2f} call_speedup_vs_per_expert={med['per_expert'] / med['decode']:.2f}"
                             + f" graph_speedup_vs_grouped={med['grouped_graph'] / med['decode_graph']:.2f}")
                print(lines[-1], flush=True)
        del qd, qp
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


def _make_batch(E, H, I, topk, batch):
    from test_gpu_moe import _fill
    from autogptq_amd.moe import QuantMoEExperts
    gen = torch.Generator().manual_seed(1)
    q = QuantMoEExperts(E, H, I, 4, 128, top_k=topk, weight_dtype=torch.float16)
    for e in range(E):
        for l in q[e].layers():
            _fill(l, gen, False)
    q = q.cuda()
    q.post_init(batch=batch)
    return q


def batch_sweep(args):
    lines = [f"# tools/moe_sweep.py --batch: 4-bit g128 fp16 experts; per repeat the paths are timed in turn (batch, batch_graph, grouped, grouped_graph, per_expert); "
             f"*_us = CALL time: one event pair around {args.reps} back-to-back eager calls / {args.reps}; *_graph_us = the same call captured in a hipGraph per routing and "
             f"replayed (kernel-side time); value = median over {args.repeats} repeats [min .. max]; batch = experts post-initialised with batch=True, grouped / per_expert = "
             "experts post-initialised without a copy; routing rotated over all E experts (8 routings, indices advanced by ceil(E / 8)); bytes = packed weights + "
             "scales / zeros of the hit experts; frac_bw = bytes / graph time / 8 TB/s"]
    for name, (E, topk, H, I) in SHAPES.items():
        qb = _make_batch(E, H, I, topk, True)
        qp = _make_batch(E, H, I, topk, False)
        per_expert_bytes = 3 * (H * I // 2 + (H // 128) * I * 2 + (H // 128) * I // 2)
        step = (E + 7) // 8
        for T in (5, 8, 16, 32, 64):
            x = (torch.rand((T, H), generator=torch.Generator().manual_seed(T)) - 0.5).half().cuda()
            idx, w = _routing(T, E, topk, T)
            hit = int(torch.unique(idx).numel())
            assert qb.plan(T, topk)["path"] == "batch" and qp.plan(T, topk)["path"] == "grouped"
            routings = [((idx + k * step) % E, w) for k in range(8)]
            fb, fg = (lambda i, ww: moe_forward(qb, x, i, ww)), (lambda i, ww: moe_forward(qp, x, i, ww))
            fns = {"batch": lambda: _time_rot(fb, routings, args.reps), "batch_graph": lambda: _time_graph(fb, routings, args.reps),
                   "grouped": lambda: _time_rot(fg, routings, args.reps), "grouped_graph": lambda: _time_graph(fg, routings, args.reps),
                   "per_expert": lambda: _time_rot(lambda i, ww: _per_expert(qp, x, i, ww), routings, max(5, args.reps // 2))}
            got = {k: [] for k in fns}
            with torch.no_grad():
                for _ in range(args.repeats):
                    for k, fn in fns.items():
                        got[k].append(fn())
            med = {k: sorted(v)[len(v) // 2] for k, v in got.items()}
            byt = hit * per_expert_bytes
            wins = max(got["batch"]) < min(got["grouped"]) and max(got["batch"]) < min(got["per_expert"]) and max(got["batch_graph"]) < min(got["grouped_graph"])
            lines.append(f"{name} T={T} hit={hit} " + " ".join(f"{k}_us={med[k]:.1f}[{min(got[k]):.1f}..{max(got[k]):.1f}]" for k in fns)
                         + f" batch_frac_bw={byt / (med['batch_graph'] * 1e-6) / 8e12:.3f} grouped_frac_bw={byt / (med['grouped_graph'] * 1e-6) / 8e12:.3f}"
                         + f" call_speedup_vs_grouped={med['grouped'] / med['batch']:.2f} call_speedup_vs_per_expert={med['per_expert'] / med['batch']:.2f}"
                         + f" graph_speedup_vs_grouped={med['grouped_graph'] / med['batch_graph']:.2f} wins_beyond_spread={'yes' if wins else 'NO'}")
            print(lines[-1], flush=True)
        del qb, qp
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


def trace_only(T, batch=False):
    from test_gpu_moe_decode import make_experts as make_dc
    E, topk, H, I = SHAPES["mixtral8x7b"]
    qd = _make_batch(E, H, I, topk, True) if batch else make_dc(E, H, I, 4, 128, False, torch.float16, seed=1, top_k=topk, decode_copy=True)
    x = (torch.rand((T, H), generator=torch.Generator().manual_seed(T)) - 0.5).half().cuda()
    idx, w = _routing(T, E, topk, T)
    with torch.no_grad():
        for k in range(40):
            moe_forward(qd, x, (idx + k) % E, w)
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--per-expert-max-t", type=int, default=2048)
    ap.add_argument("--decode", action="store_true")
    ap.add_argument("--batch", action="store_true")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--trace-only", type=int, default=0)
    args = ap.parse_args()
    if args.trace_only:
        return trace_only(args.trace_only, args.batch)
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "moe_batch_sweep.log" if args.batch else ("moe_decode_sweep.log" if args.decode else "moe_sweep.log"))
    if args.batch:
        return batch_sweep(args)
    if args.decode:
        return decode_sweep(args)
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
