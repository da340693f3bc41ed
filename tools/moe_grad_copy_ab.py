#!/usr/bin/env python3
"""The routed experts' backward on the decode copy (gptq_moe_backward_ex with GPTQ_GRAD_ON_COPY: the grouped mode of grad_copy_kernel) against the rows
form (flags = 0: moe_grad_kernel on the checkpoint rows) of the SAME experts in one session, as tools/act_int8_ab.py measures: whole calls captured in a
hipGraph over rotating expert blocks with weights of their own (so that the weights come from HBM, not from the Infinity Cache), --rounds rounds per side,
alternating; the log carries the median time of either side with its repeat spread (max / min - 1) and closes with the cells where the copy form is slower
than the rows form by more than the largest spread of the run.  Each cell also counts the dX elements whose bits differ between the two forms (every
matrix sum runs in the rows form's order and the down stage's scalar epilogue mirrors its instruction forms: DESIGN 4.8).  Nothing depends on the copy form winning: it is
off by default.  With --parent-lib (a libgptq_mi355x.so built from the parent commit) the log also carries the dense A/B the shared kernel symbol asks
for: gptq_grad_input_ex with the flag on, parent library against this one, same tensors, alternating, dX compared bit for bit.
Usage: python tools/moe_grad_copy_ab.py [--models mixtral,qwen] [--ts 512,2048,8192] [--act 0,1] [--parent-lib PATH] [--out profiles/moe_grad_copy_ab.log]"""
import argparse
import ctypes
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from autogptq_amd import QuantLinear, _lib  # noqa: E402
from autogptq_amd.moe import QuantMoEExperts  # noqa: E402

MODELS = {"mixtral": (4096, 14336, 8, 2), "qwen": (2048, 1408, 60, 4)}      # H, I, E, topk: Mixtral-8x7B block, Qwen1.5-MoE-A2.7B experts
ap = argparse.ArgumentParser()
ap.add_argument("--models", default="mixtral,qwen")
ap.add_argument("--ts", default="512,2048,8192")
ap.add_argument("--act", default="0,1")
ap.add_argument("--gs", type=int, default=128)
ap.add_argument("--bits", type=int, default=4, help="the experts' width; 2, 3, 8 run under backward_on_copy = \"any_bits\" (profiles/grad_copy_bits_ab.log)")
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--blocks", type=int, default=2, help="expert blocks the graph rotates over (one block is already larger than the 256 MiB Infinity Cache)")
ap.add_argument("--parent-lib", default="")
ap.add_argument("--out", default="")
a = ap.parse_args()
dev, dt = torch.device("cuda:0"), torch.float16
lib = _lib.load()
FLAGS = _lib.grad_copy_flags(True if a.bits == 4 else "any_bits")
log = open(a.out, "w") if a.out else None


def say(s):
    print(s, flush=True)
    if log:
        log.write(s + "\n")
        log.flush()


def fill(l, act, g):
    K, N, G = l.infeatures, l.outfeatures, -(-l.infeatures // a.gs)
    l.qweight = torch.randint(-2**31, 2**31 - 1, (K // 32 * a.bits, N), dtype=torch.int64, device=dev, generator=g).to(torch.int32)
    l.qzeros = torch.randint(-2**31, 2**31 - 1, (G, N // 32 * a.bits), dtype=torch.int64, device=dev, generator=g).to(torch.int32)
    l.scales = (0.002 * (1 + 0.1 * torch.rand(G, N, device=dev, generator=g))).to(dt)
    gi = torch.arange(K, device=dev, dtype=torch.int32) // a.gs
    l.g_idx = (gi[torch.randperm(K, device=dev, generator=g)] if act else gi).contiguous()


def block(H, I, E, topk, act, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    q = QuantMoEExperts(E, H, I, a.bits, a.gs, top_k=topk, weight_dtype=dt)
    for e in range(E):
        gate, up, down = q[e].layers()
        fill(gate, act, g), fill(up, act, g), fill(down, act, g)
        if act:
            up.g_idx = gate.g_idx.clone()          # one order for gate and up, as a GPTQ checkpoint has them
    q = q.to(dev)
    q.backward_on_copy = True if a.bits == 4 else "any_bits"
    q.post_init(backward=True, low_bit=a.bits < 4, low_bit_decode=a.bits < 4)
    assert q._backward_on_copy, "the experts were declined"
    return q


def timed(fn, reps):
    """Median-ready time of one call (seconds): `reps` replays of a graph that holds one call per block."""
    fn()
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        n = fn()
    gr.replay()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        gr.replay()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) * 1e-3 / (reps * n)


def ab(sides, reps):
    """{name: [seconds per round]} for the callables of `sides`, alternating."""
    t = {k: [] for k in sides}
    for _ in range(a.rounds):
        for k, fn in sides.items():
            t[k].append(timed(fn, reps))
    return t


def stat(ts):
    return statistics.median(ts), max(ts) / min(ts) - 1


say(f"# MoE backward: rows form (flags = 0) against the copy form (GPTQ_GRAD_ON_COPY) on the same {a.bits}-bit g{a.gs} fp16 experts; ms per whole call (route, "
    f"recompute, down, up, combine), median of {a.rounds} rounds x {a.reps} graph replays over {a.blocks} rotating expert blocks; spread = max / min - 1")
cells, spreads = [], []
for name in filter(None, a.models.split(",")):      # (--models "" with --parent-lib: the dense A/B alone)
    H, I, E, topk = MODELS[name]
    for act in map(int, a.act.split(",")):
        qs = [block(H, I, E, topk, bool(act), 10 * b + act) for b in range(a.blocks)]
        for T in map(int, a.ts.split(",")):
            g = torch.Generator(device=dev).manual_seed(T)
            x, dout = ((torch.rand((T, H), device=dev, generator=g) - 0.5).to(dt) for _ in range(2))
            idx = torch.rand((T, E), device=dev, generator=g).topk(topk, dim=-1).indices.contiguous()
            w = torch.full((T, topk), 1.0 / topk, device=dev)
            need = int(lib.gptq_moe_backward_workspace_bytes(ctypes.byref(qs[0]._moe), T, topk))
            ws = torch.zeros(need, dtype=torch.uint8, device=dev)
            dx = {f: torch.empty((T, H), dtype=dt, device=dev) for f in (0, FLAGS)}
            dw = torch.empty((T, topk), dtype=torch.float32, device=dev)
            st = torch.cuda.current_stream

            def call(flags):
                for q in qs:
                    _lib.check(lib.gptq_moe_backward_ex(ctypes.byref(q._moe), q._table.data_ptr(), q._grad_table.data_ptr(), q._decode_table.data_ptr(),
                                                        x.data_ptr(), idx.data_ptr(), w.data_ptr(), dout.data_ptr(), T, topk, dx[flags].data_ptr(),
                                                        dw.data_ptr(), None, ws.data_ptr(), need, flags, st(dev).cuda_stream))
                return len(qs)

            t = ab({"rows": lambda: call(0), "copy": lambda: call(FLAGS)}, a.reps)
            nd, md = int((dx[0] != dx[FLAGS]).sum()), float((dx[0].float() - dx[FLAGS].float()).abs().max())
            (m0, s0), (m1, s1) = stat(t["rows"]), stat(t["copy"])
            spreads += [s0, s1]
            plan = _lib.describe_moe_backward_plan_ex(qs[0]._moe, T, topk, FLAGS)
            cells.append((name, act, T, m0, m1))
            say(f"{name:7s} H={H} I={I} E={E} topk={topk} {'act-order' if act else 'plain    '} T={T:5d} launches={plan['launches']} | rows {m0 * 1e3:8.3f} ms "
                f"(spread {s0 * 100:4.1f} %) | copy {m1 * 1e3:8.3f} ms (spread {s1 * 100:4.1f} %) | {m0 / m1:5.2f}x | dX: {nd} of {T * H} elements differ, max |diff| {md:.1e}")
            del x, dout, ws, dx
        del qs
        torch.cuda.empty_cache()
worst = max(spreads) if spreads else 0.0
say(f"# largest repeat spread of the run: {worst * 100:.1f} %")
lose = [c for c in cells if c[4] > c[3] * (1 + worst)]
say(f"# cells: {len(cells)}; copy form slower than the rows form by more than that spread: {len(lose)}")
for name, act, T, m0, m1 in lose:
    say(f"#   LOSES {name} {'act-order' if act else 'plain'} T={T} {m0 * 1e3:.3f} -> {m1 * 1e3:.3f} ms ({m0 / m1:.2f}x)")
say("# down and up stages alone (kernel trace): not measured")

if a.parent_lib:
    par = ctypes.CDLL(a.parent_lib)
    for L in (par, lib):
        L.gptq_grad_input_ex.argtypes = [ctypes.POINTER(_lib.GptqLayer), ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    say("# dense gptq_grad_input_ex (GPTQ_GRAD_ON_COPY), parent library against this one: us per call, same layers and dY, alternating")
    for K, N in ((4096, 4096), (4096, 11008)):
        n = max(4, -(-(384 << 20) // (K * N // 2)))
        ls = []
        for i in range(n):
            q = QuantLinear(4, a.gs, K, N, False, weight_dtype=dt)
            fill(q, False, torch.Generator(device=dev).manual_seed(i))
            ls.append(q.to(dev).post_init(grad_on_copy=True))
        for M in (512, 2048):
            dy = (torch.rand((M, N), device=dev) - 0.5).to(dt)
            out = {k: torch.empty((M, K), dtype=dt, device=dev) for k in ("parent", "this")}

            def dense(L, k):
                for q in ls:
                    assert L.gptq_grad_input_ex(ctypes.byref(q._layer), dy.data_ptr(), out[k].data_ptr(), M, 0, 1, torch.cuda.current_stream(dev).cuda_stream) == 0
                return len(ls)

            t = ab({"parent": lambda: dense(par, "parent"), "this": lambda: dense(lib, "this")}, 5)
            (m0, s0), (m1, s1) = stat(t["parent"]), stat(t["this"])
            say(f"dense {K}x{N} M={M:4d} layers={n} | parent {m0 * 1e6:8.2f} us (spread {s0 * 100:4.1f} %) | this {m1 * 1e6:8.2f} us (spread {s1 * 100:4.1f} %) | "
                f"{m0 / m1:5.3f}x | dX bits {'equal' if torch.equal(out['parent'], out['this']) else 'DIFFER'}")
        del ls
