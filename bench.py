#!/usr/bin/env python3
"""bench.py -- int4 g128 QuantLinear forward on Llama-7B linear shapes (BASELINE.json metric).

One STEP = one token (M = 1 rows) pushed through every quantized linear of a Llama-7B decoder
stack: 32 blocks x {q,k,v,o: 4096->4096, gate,up: 4096->11008, down: 11008->4096} = 224 distinct
layers = 3.37 GB of packed weights, so every launch streams its weights from HBM (the working set
is 13x the 256 MiB Infinity Cache -- a single-layer repeat loop would measure the cache instead).
The 224 launches are captured once in a hipGraph (through torch's stream capture; the kernels are
enqueued by libgptq_mi355x.so on the capturing stream) and replayed per step.

  value      = algorithmic GB/s over the whole job (SURVEY App. C byte formula), inputs resident in HBM
  tokens/s   = steps / time ("linear-only": attention/norm/sampling are not part of this path)
  roofline   = dominant kernel: algorithmic bytes per launch / mean launch duration from HIP events
               bracketing a graph that holds only that kernel's launches (rotating weights)
  cpu_baseline = the oracle (port of the reference's CPU QuantLinear.forward) timed on host cores

N > 1 (launched by torch.distributed.run, one rank per GPU): every rank streams its own token
through its own copy of the stack -- independent requests, no data-path collective ("weak").  The
optional out_features tensor-parallel mode (one RCCL all-gather per layer) is timed separately and
reported under "tp" (Llama-2-70B shapes, BASELINE config 4).

Workloads: --workload decode (default) | prefill (M = 2048, act-order, MFMA path, reports TFLOP/s).

A plain run builds the stack, warms up, times --steps replays and prints the headline line.  Everything else (the roofline per launch type,
the check of the timed outputs against a second kernel family, the eager / fused / MLP / prefill / config 5 / batched / warm-cache blocks,
the CPU baseline, the per-layer tensor-parallel entries) runs only with --full.  --dump-outputs DIR writes what the timed path returned in
its last step as DIR/<block>_<layer>.npy (float32; inputs and weights are seeded, so two builds compare output for output).
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0        # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec (6.29 TB/s measured copy)
MFMA_PEAK_TFLOPS = 2500.0    # dense fp16/bf16 MFMA peak

LLAMA7B_BLOCK = [("q_proj", 4096, 4096), ("k_proj", 4096, 4096), ("v_proj", 4096, 4096), ("o_proj", 4096, 4096),
                 ("gate_proj", 4096, 11008), ("up_proj", 4096, 11008), ("down_proj", 11008, 4096)]
LLAMA70B_TP = [("attn", 8192, 8192), ("gate_up", 8192, 28672)]


def algorithmic_bytes(K, N, M, bits=4, gs=128, act_order=False, dtype_bytes=2, bias=False):
    G = -(-K // gs)
    b = K * N * bits // 8 + G * N * bits // 8 + G * N * dtype_bytes + dtype_bytes * M * K + dtype_bytes * M * N
    if act_order:
        b += 4 * K
    if bias:
        b += dtype_bytes * N
    return b


def make_layer(K, N, device, bits=4, gs=128, act_order=False, dtype=torch.float16, seed=0, order_seed=None):
    """Synthetic layer, generated on the device: random packed words (every bit pattern is legal),
    scales 0.002*(1+0.1*rand) -- the recipe of SURVEY section 8(d) / tests/test_q4.py:1086-1112.
    order_seed: the activation order (g_idx permutation) from its own seed -- layers that read the same input get the same one, as GPTQ
    produces them (the order is the argsort of the Hessian diagonal of the layers' common input; the reference's fused q/k/v caller relies on it)."""
    import autogptq_amd

    g = torch.Generator(device=device).manual_seed(seed)
    q = autogptq_amd.QuantLinear(bits, gs, K, N, False, weight_dtype=dtype)
    G = -(-K // gs)
    q.qweight = torch.randint(-2**31, 2**31 - 1, (K // 32 * bits, N), dtype=torch.int64, device=device, generator=g).to(torch.int32)
    q.qzeros = torch.randint(-2**31, 2**31 - 1, (G, N // 32 * bits), dtype=torch.int64, device=device, generator=g).to(torch.int32)
    q.scales = (0.002 * (1 + 0.1 * torch.rand(G, N, device=device, generator=g))).to(dtype)
    gi = torch.arange(K, device=device, dtype=torch.int32) // gs
    if act_order:
        go = g if order_seed is None else torch.Generator(device=device).manual_seed(order_seed)
        gi = gi[torch.randperm(K, device=device, generator=go)]
    q.g_idx = gi.contiguous()
    q = q.to(device)
    q.post_init()
    return q


def build_stack(device, n_blocks, M, act_order, dtype=torch.float16):
    layers = []
    for b in range(n_blocks):
        for i, (name, K, N) in enumerate(LLAMA7B_BLOCK):
            # q / k / v read one input and so do gate / up: one activation order per group of a block (o and down have their own)
            grp = {"q_proj": 0, "k_proj": 0, "v_proj": 0, "gate_proj": 1, "up_proj": 1}.get(name, 2 + i)
            layers.append((name, K, N, make_layer(K, N, device, act_order=act_order, dtype=dtype, seed=b * 16 + i, order_seed=10_000 + b * 16 + grp)))
    gx = torch.Generator(device=device).manual_seed(20_000)
    xs = {K: (torch.rand(M, K, device=device, generator=gx) - 0.5).to(dtype) for K in (4096, 11008)}
    return layers, xs


def stack_output_names(blocks):
    """<block>_<layer> for every layer of `blocks` decoder blocks, in stack order (the order of the flattened outputs)."""
    return [f"b{b:02d}_{name}" for b in range(blocks) for name, _, _ in LLAMA7B_BLOCK]


def flatten_outputs(outs):
    """One tensor per layer: a grouped launch (gptq_forward_multi) returns its layers' outputs as a list."""
    return [t for y in outs for t in (y if isinstance(y, (list, tuple)) else [y])]


def dump_outputs(path, names, tensors, budget=60_000_000):
    """Write each output as <path>/<name>.npy in float32.  Outputs of more than `budget` bytes in all keep the same seeded sample of rows in
    every array (sorted row indices from a fixed seed), so the files stay under 64 MB and two builds still compare row for row."""
    import numpy as np
    assert len(names) == len(tensors), (len(names), len(tensors))
    os.makedirs(path, exist_ok=True)
    rows = tensors[0].shape[0]
    per_row = 4 * sum(t[0].numel() for t in tensors)
    keep = max(1, min(rows, budget // per_row))
    idx = None
    if keep < rows:
        idx = torch.from_numpy(np.sort(np.random.default_rng(0).choice(rows, keep, replace=False)))
    for name, t in zip(names, tensors):
        y = t if idx is None else t.index_select(0, idx.to(t.device))
        np.save(os.path.join(path, name + ".npy"), y.float().cpu().numpy())


def group_stack(layers):
    """The same layers, grouped the way a decoder block calls them: [q, k, v] and [gate, up] read the same activations and go
    through gptq_forward_multi (ONE launch per group for decode rows, the checkpoint tensors untouched); o and down stay single
    calls.  Entries: (name, K, N_total, layer | [layers])."""
    out, i = [], 0
    while i < len(layers):
        name = layers[i][0]
        if name == "q_proj" and i + 2 < len(layers) and layers[i + 2][0] == "v_proj":
            grp = layers[i:i + 3]
            out.append(("qkv", grp[0][1], sum(g[2] for g in grp), [g[3] for g in grp]))
            i += 3
        elif name == "gate_proj" and i + 1 < len(layers) and layers[i + 1][0] == "up_proj":
            grp = layers[i:i + 2]
            out.append(("gate_up", grp[0][1], sum(g[2] for g in grp), [g[3] for g in grp]))
            i += 2
        else:
            out.append(layers[i])
            i += 1
    return out


def call(q, x):
    if isinstance(q, list):
        from autogptq_amd.qlinear_mi355x import forward_multi
        return forward_multi(q, x)
    return q(x)


def entry_bytes(ent, M, act_order=False):
    name, K, N, q = ent
    if isinstance(q, list):
        return sum(algorithmic_bytes(K, l.outfeatures, M, act_order=act_order) for l in q)
    return algorithmic_bytes(K, N, M, act_order=act_order)


def make_fused_block(device, seed):
    """The same Llama-7B block as four launches: [q|k|v] (4096 -> 12288), o, [gate|up] with the SiLU*mul epilogue
    (4096 -> 22016, output 11008) and down -- the reference's fused attention / fused MLP callers."""
    import autogptq_amd

    def mk(K, N, epilogue, sd):
        g = torch.Generator(device=device).manual_seed(sd)
        q = autogptq_amd.QuantLinear(4, 128, K, N, False, epilogue=epilogue)
        G = K // 128
        q.qweight = torch.randint(-2**31, 2**31 - 1, (K // 8, N), dtype=torch.int64, device=device, generator=g).to(torch.int32)
        q.qzeros = torch.randint(-2**31, 2**31 - 1, (G, N // 8), dtype=torch.int64, device=device, generator=g).to(torch.int32)
        q.scales = (0.002 * (1 + 0.1 * torch.rand(G, N, device=device, generator=g))).half()
        q = q.to(device)
        q.post_init()
        return q
    return [("qkv", 4096, 12288, mk(4096, 12288, "none", seed)), ("o", 4096, 4096, mk(4096, 4096, "none", seed + 1)),
            ("gate_up", 4096, 22016, mk(4096, 22016, "silu_mul", seed + 2)), ("down", 11008, 4096, mk(11008, 4096, "none", seed + 3))]


def bench_fused(device, n_blocks, steps):
    layers = []
    for b in range(n_blocks):
        layers += make_fused_block(device, 1000 + 8 * b)
    xs = {K: (torch.rand(1, K, device=device) - 0.5).half() for K in (4096, 11008)}
    g, outs = capture(layers, xs, device)
    settle(g, device)
    wall, ev = time_graph(g, steps, device)
    bytes_step = sum(algorithmic_bytes(K, N, 1) for _, K, N, _ in layers)
    return {"launches_per_step": len(layers), "ms_per_step": round(1e3 * ev / steps, 4), "GB_per_s": round(bytes_step * steps / ev / 1e9, 1),
            "tokens_per_s": round(steps / ev, 1),
            "note": "same weights volume as the headline run, 4 launches per block: [q|k|v], o, [gate|up]+SiLU*mul epilogue, down"}


def bench_mlp_call(flat_layers, xs, device, steps):
    """The gated MLP of every block through gptq_mlp_forward (ONE C-ABI call per block: gate|up launch, SiLU*mul, down) as a hipGraph over all blocks
    (rotating, HBM-cold weights).  The activation really flows from gate/up into down here (the headline stack feeds down an independent x)."""
    from autogptq_amd.qlinear_mi355x import mlp_forward, exchange_error
    blocks, i = [], 0
    while i + 2 < len(flat_layers):
        if flat_layers[i][0] == "gate_proj" and flat_layers[i + 1][0] == "up_proj" and flat_layers[i + 2][0] == "down_proj":
            blocks.append((flat_layers[i][3], flat_layers[i + 1][3], flat_layers[i + 2][3]))
            i += 3
        else:
            i += 1
    x = xs[4096]
    res = {"blocks": len(blocks)}
    wbytes = sum(algorithmic_bytes(4096, 11008, 1) * 2 + algorithmic_bytes(11008, 4096, 1) for _ in blocks[:1])
    for name in ("default_three_steps",):
        try:
            with torch.no_grad():
                for g_, u_, d_ in blocks:
                    mlp_forward(g_, u_, d_, x)
            torch.cuda.synchronize(device)
            gr = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gr), torch.no_grad():
                keep = [mlp_forward(g_, u_, d_, x) for g_, u_, d_ in blocks]
            for _ in range(3):
                gr.replay()
            _, ev = time_graph(gr, max(3, steps // 2), device)
            per = ev / (max(3, steps // 2) * len(blocks))
            res[name] = {"us_per_mlp": round(per * 1e6, 2), "GB_per_s": round(wbytes / per / 1e9, 1), "frac": round(wbytes / per / 1e9 / HBM_PEAK_GBS, 4),
                         "bounded_wait_gave_up": bool(exchange_error(device))}
            del gr, keep
        except Exception as e:
            res[name] = {"error": repr(e)[:200]}
    return res


def bench_mlp_prefill(device, steps, M=2048, n_blocks=4):
    """The gated MLP of act-order (desc_act) Llama-7B blocks at prefill rows through gptq_mlp_forward: round 6 writes silu(g) * u straight in the order down's
    re-sequenced rows expect (one pass instead of SiLU * mul + down's own permute launch).  Timed against the two passes of round 5 (lab knob 54), interleaved
    graph replays over rotating blocks; `down_part_us` = the call minus its [gate | up] launches timed on their own."""
    from autogptq_amd import _lib
    from autogptq_amd.qlinear_mi355x import mlp_forward, forward_multi
    blocks = []
    for b in range(n_blocks):
        g_ = make_layer(4096, 11008, device, act_order=True, seed=3000 + 3 * b, order_seed=3500 + b)
        u_ = make_layer(4096, 11008, device, act_order=True, seed=3001 + 3 * b, order_seed=3500 + b)
        d_ = make_layer(11008, 4096, device, act_order=True, seed=3002 + 3 * b)
        blocks.append((g_, u_, d_))
    x = (torch.rand(M, 4096, device=device) - 0.5).half()
    two = _lib.GptqTuning()
    two.reserved[_lib.LAB.GEMM_VARIANT] = _lib.LAB.VARIANT_MLP_TWO_PASSES
    graphs = {}
    for name, tn in (("fused_permute", None), ("two_passes", two)):
        with torch.no_grad():
            for g_, u_, d_ in blocks:
                mlp_forward(g_, u_, d_, x, tuning=tn)
        torch.cuda.synchronize(device)
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr), torch.no_grad():
            keep = [mlp_forward(g_, u_, d_, x, tuning=tn) for g_, u_, d_ in blocks]
        graphs[name] = (gr, keep)
    with torch.no_grad():
        for g_, u_, _ in blocks:
            forward_multi([g_, u_], x)
    torch.cuda.synchronize(device)
    gu = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gu), torch.no_grad():
        keep_gu = [forward_multi([g_, u_], x) for g_, u_, _ in blocks]
    graphs["gate_up_only"] = (gu, keep_gu)
    best = {}
    reps = max(3, steps // 2)
    for _ in range(3):                                    # interleaved rounds, minimum per variant
        for name, (gr, _) in graphs.items():
            gr.replay()
            _, ev = time_graph(gr, reps, device)
            best[name] = min(best.get(name, 1e9), ev / (reps * len(blocks)))
    res = {"M": M, "blocks": len(blocks), "plan": _lib.describe_mlp_plan(blocks[0][0]._layer, blocks[0][1]._layer, blocks[0][2]._layer, M),
           "us_per_mlp": round(best["fused_permute"] * 1e6, 2), "us_per_mlp_two_passes": round(best["two_passes"] * 1e6, 2),
           "gate_up_us": round(best["gate_up_only"] * 1e6, 2),
           "down_part_us": round((best["fused_permute"] - best["gate_up_only"]) * 1e6, 2), "down_part_us_two_passes": round((best["two_passes"] - best["gate_up_only"]) * 1e6, 2),
           "TFLOP_s": round(2 * M * 3 * 4096 * 11008 / best["fused_permute"] / 1e12, 1)}
    same = all(torch.equal(a, b) for a, b in zip(graphs["fused_permute"][1], graphs["two_passes"][1]))
    res["fused_equals_two_passes_bitwise"] = bool(same)
    del graphs, blocks
    torch.cuda.empty_cache()
    return res


def capture(layers, xs, device):
    """Capture one forward of every layer into a graph; returns (graph, keepalive outputs)."""
    from autogptq_amd.qlinear_mi355x import reserve_workspace
    import ctypes
    from autogptq_amd import _lib

    side = torch.cuda.Stream(device=device)
    side.wait_stream(torch.cuda.current_stream(device))
    with torch.cuda.stream(side), torch.no_grad():       # warm-up run (allocator, lazy init, scratch of the largest need)
        for _, K, N, q in layers:
            call(q, xs[K])
    torch.cuda.current_stream(device).wait_stream(side)
    torch.cuda.synchronize(device)
    g = torch.cuda.CUDAGraph()
    outs = []
    with torch.cuda.graph(g), torch.no_grad():
        for _, K, N, q in layers:
            outs.append(call(q, xs[K]))
    return g, outs


def verify_timed_outputs(layers, outs, xs, max_entries=8):
    """What the timed graph wrote, against a SECOND kernel family of this library on the same inputs: the first entries of every launch type are
    recomputed through layers rebuilt WITHOUT the decode copy (post_init(tiled=False): the checkpoint-layout kernels of rounds 1-3) and compared -- a
    wrong strip index or a stale side copy in the launches the headline times cannot pass unnoticed.  Not a parity claim (that is tests/, against the
    oracle); the oracle is not touched here.  fp16 / bf16: different summation orders, so a tolerance: 2e-3 / 1.6e-2 of the largest output."""
    import autogptq_amd
    seen, worst, checked = set(), 0.0, 0
    try:
        for (name, K, N, q), y in zip(layers, outs):
            qs = q if isinstance(q, list) else [q]
            key = (name, K, N)
            if key in seen or checked >= max_entries:
                continue
            seen.add(key)
            ys = y if isinstance(y, (list, tuple)) else [y]
            for l, yy in zip(qs, ys):
                twin = autogptq_amd.QuantLinear(l.bits, l.group_size, l.infeatures, l.outfeatures, False, weight_dtype=l.scales.dtype)
                twin.qweight, twin.qzeros, twin.scales, twin.g_idx = l.qweight, l.qzeros, l.scales, l.g_idx
                twin = twin.to(l.qweight.device)
                twin.post_init(tiled=False)
                with torch.no_grad():
                    ref = twin(xs[K])
                scale = float(ref.float().abs().max()) or 1.0
                worst = max(worst, float((yy.float() - ref.float()).abs().max()) / scale)
                del twin
            checked += 1
        tol = 1.6e-2 if any((q[0] if isinstance(q, list) else q).scales.dtype == torch.bfloat16 for _, _, _, q in layers) else 2e-3
        return {"launch_types_checked": checked, "max_err_over_max_out": round(worst, 6), "tolerance": tol, "ok": bool(worst <= tol),
                "against": "the same layers through the checkpoint-layout kernels (post_init(tiled=False)); parity with the reference: tests/, oracle"}
    except Exception as e:
        return {"error": repr(e)[:200]}


def settle(g, device, seconds=0.05):
    """Untimed replays for a fixed wall time: after an idle gap on the host side (layer construction, a device -> host check) the GPU is back at its idle
    clocks, and a measurement of a few milliseconds would time the ramp (a q|k|v launch read 27.6 us behind such a gap, 7.5 us otherwise)."""
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < seconds:
        for _ in range(10):
            g.replay()
        torch.cuda.synchronize(device)


def time_graph(g, reps, device, dist_barrier=None):
    """Wall clock (barrier + synchronize on both sides) and HIP events around `reps` replays."""
    torch.cuda.synchronize(device)
    if dist_barrier:
        dist_barrier()
    torch.cuda.synchronize(device)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    for _ in range(reps):
        g.replay()
    e1.record()
    torch.cuda.synchronize(device)
    if dist_barrier:
        dist_barrier()
    t1 = time.perf_counter()
    return t1 - t0, e0.elapsed_time(e1) * 1e-3


def time_graph_each(g, reps, device):
    """Seconds of each of `reps` replays (HIP events between consecutive replays): the spread behind a mean (p10 / p50 / p90 per launch type)."""
    torch.cuda.synchronize(device)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(reps + 1)]
    ev[0].record()
    for i in range(reps):
        g.replay()
        ev[i + 1].record()
    torch.cuda.synchronize(device)
    return [ev[i].elapsed_time(ev[i + 1]) * 1e-3 for i in range(reps)]


def _pctl(v, q):
    v = sorted(v)
    return v[min(len(v) - 1, max(0, int(round(q * (len(v) - 1)))))]


def pmc_traffic(kernel, K, N, M, exact=False):
    """HBM-side bytes per launch of the dominant kernel from the committed rocprofv3 --pmc FETCH_SIZE/WRITE_SIZE
    passes (profiles/pmc_traffic.json, produced by tools/pmc_traffic.py from separate counter-only runs of this
    same command -- the prefill kernels from one run per shape, tools/session_r05_prof.sh; FETCH_SIZE already doubled as
    MI355X_MICROARCH.md prescribes for gfx950).  exact: the rocprof kernel name has to be THIS template instantiation (the round-4 line
    reported the int3 kernel's bytes for the 4-bit act-order one: a substring match on "gemm").  None if absent."""
    path = os.path.join(ROOT, "profiles", "pmc_traffic.json")
    if not os.path.exists(path):
        return None
    norm = lambda t: t.replace(" ", "")
    try:
        with open(path) as f:
            d = json.load(f)
        for ent in d.get("kernels", []):
            same = norm(ent["kernel"]) == norm(kernel) if exact else (ent["kernel"] in kernel or kernel in ent["kernel"])
            if same and ent["K"] == K and ent["N"] == N and ent["M"] == M:
                return ent["hbm_bytes_per_launch"]
    except Exception:
        return None
    return None


def rocprof_gemm_kernel(plan, dtype="f16", group_size=128, bits=4):
    """The name rocprofv3 reports (tools/rocprof_summary.py: demangled, without the argument list) for the prefill kernel of a plan dict
    (gptq_describe_plan): what profiles/r05_kernel_stats.txt and profiles/pmc_traffic.json key their rows by."""
    k = plan.get("kernel")
    g128 = "true" if group_size % 128 == 0 else "false"
    if k == "wide_sk":
        if bits != 4 or group_size == 32:          # csrc/gemm_wide_sk_b38.hip: <T, BITS, group mode 0 / 1 / 2 = groups of 128 / 64 multiples / 32>
            return f"gptq::wide::gemm_wide_skb_kernel<{dtype}, {bits}, {0 if group_size % 128 == 0 else (1 if group_size % 64 == 0 else 2)}>"
        return f"gptq::wide::gemm_wide_sk_kernel<{dtype}, {g128}>"
    if k == "wide_copy":
        return f"gptq::wide::gemm_wide_kernel<{dtype}, true, true, {g128}>"
    if k == "wide":
        return f"gptq::wide::gemm_wide_kernel<{dtype}, {'true' if plan.get('dma') else 'false'}, false, false>"
    if k == "tiled":
        dma = "true" if plan.get("dma") else "false"
        return f"gptq::gemm_kernel<4, {dtype}, {plan.get('mt')}, {plan.get('bk')}, 1, {dma}, {dma}, {plan.get('kg')}, {'true' if plan.get('tail') else 'false'}>"
    return "gptq::" + str(k)


def _time_layers(layers, xs, device, reps):
    """Mean seconds per launch of a graph that holds exactly these layers (HIP events around `reps` replays)."""
    gg, oo = capture(layers, xs, device)
    settle(gg, device)
    _, evt = time_graph(gg, reps, device)
    del gg, oo
    return evt / (reps * len(layers))


def bench_prefill(device, steps):
    """BASELINE config 3 + north_star's M = 4096 target inside the default run: 4 decoder blocks of int4 g128 desc_act=True
    layers at M = 2048 (28 launches + their x permutations, one hipGraph), then the dominant GEMM on its own, then one
    M = 4096 4096x4096 layer (no act-order).  flops = 2*M*K*N per layer; peak = dense fp16 MFMA 2.5 PFLOP/s."""
    M = 2048
    layers, xs = build_stack(device, 4, M, True)
    g, outs = capture(layers, xs, device)
    settle(g, device)
    _, ev = time_graph(g, steps, device)
    flops_step = sum(2 * M * K * N for _, K, N, _ in layers)
    by_type = {}
    for ent in layers:
        by_type.setdefault((ent[1], ent[2]), []).append(ent)
    per_type, best = {}, None
    for (K, N), ls in by_type.items():
        per = _time_layers(ls, xs, device, max(2, steps // 2))
        per_type[f"{K}x{N}"] = {"us": round(per * 1e6, 2), "TFLOP_s": round(2 * M * K * N / per / 1e12, 1)}
        if best is None or per * len(ls) > best[0]:
            best = (per * len(ls), K, N, per)
    _, K, N, per = best
    ach = 2 * M * K * N / per / 1e12
    plan = _plan_of(layers, K, N, M)
    pd = _plan_dict(layers, K, N, M)
    kname = rocprof_gemm_kernel(pd)
    roof = {"bound": "mfma", "achieved": round(ach, 1), "peak": MFMA_PEAK_TFLOPS, "unit": "TFLOP/s", "frac": round(ach / MFMA_PEAK_TFLOPS, 4),
            "traffic": pmc_traffic(kname, K, N, M, exact=True), "kernel": kname, "plan": plan, "shape": f"K={K} N={N} M={M} desc_act",
            "us_per_launch_events": round(per * 1e6, 2), "flops_per_launch": 2 * M * K * N,
            "note": "per-launch time is the whole layer call: x permutation (if the plan has a separate pass) + GEMM"}
    del g, outs
    torch.cuda.empty_cache()
    # north_star: (batch x seq = 4096, 4096 -> 4096), int4 g128, sequential groups; 40 distinct layers (> 256 MiB with x / out)
    M2 = 4096
    ls = [("q", 4096, 4096, make_layer(4096, 4096, device, seed=900 + i)) for i in range(8)]
    xs2 = {4096: (torch.rand(M2, 4096, device=device) - 0.5).half()}
    per2 = _time_layers(ls, xs2, device, max(2, steps // 2))
    ach2 = 2 * M2 * 4096 * 4096 / per2 / 1e12
    pd2 = _plan_dict(ls, 4096, 4096, M2)
    k2 = rocprof_gemm_kernel(pd2)
    out = {"workload": "Llama-7B shapes x 4 blocks, int4 g128 desc_act=True, M=2048 (BASELINE config 3), 28 layers in one hipGraph",
           "TFLOP_s": round(flops_step * steps / ev / 1e12, 1), "ms_per_step": round(1e3 * ev / steps, 3), "tokens_per_s": round(M * steps / ev, 1),
           "by_shape": per_type, "roofline": roof,
           "m4096_4096x4096": {"us_per_launch_events": round(per2 * 1e6, 2), "TFLOP_s": round(ach2, 1), "frac": round(ach2 / MFMA_PEAK_TFLOPS, 4),
                               "plan": _plan_of(ls, 4096, 4096, M2), "kernel": k2, "traffic": pmc_traffic(k2, 4096, 4096, M2, exact=True)}}
    del ls, xs2
    torch.cuda.empty_cache()
    # row counts that leave a remainder round of 128 x 256 tiles (balanced tail): the planner's default against whole tiles only
    try:
        from autogptq_amd import _lib
        off = _lib.GptqTuning()
        off.path, off.reserved[3] = 3, 41
        rem = {}
        for (K, N, Mx, act) in ((4096, 11008, 2304, True), (4096, 11008, 1536, True), (4096, 4096, 2176, False)):
            ls = [("q", K, N, make_layer(K, N, device, act_order=act, seed=950 + i)) for i in range(6)]
            x = (torch.rand(Mx, K, device=device) - 0.5).half()
            graphs = []
            for tn in (None, off):                      # the planner's default, then whole tiles only
                gg = torch.cuda.CUDAGraph()
                with torch.no_grad():
                    ls[0][3](x, tuning=tn)
                    torch.cuda.synchronize(device)
                    with torch.cuda.graph(gg):
                        keep = [q(x, tuning=tn) for _, _, _, q in ls]
                graphs.append((gg, keep))
            reps = max(2, steps // 6)
            best = [1e9, 1e9]
            for _ in range(2):                          # interleaved, minimum of two rounds each
                for i, (gg, _) in enumerate(graphs):
                    gg.replay()
                    _, evt = time_graph(gg, reps, device)
                    best[i] = min(best[i], evt / (reps * len(ls)))
            per, per_off = best
            rem[f"{K}x{N}_M{Mx}" + ("_desc_act" if act else "")] = {
                "us": round(per * 1e6, 2), "TFLOP_s": round(2 * Mx * K * N / per / 1e12, 1), "frac": round(2 * Mx * K * N / per / 1e12 / MFMA_PEAK_TFLOPS, 4),
                "us_whole_tiles_only": round(per_off * 1e6, 2), "plan": _plan_of(ls, K, N, Mx)}
            del graphs, gg, keep, ls, x
            torch.cuda.empty_cache()
        out["remainder_rounds"] = rem
    except Exception as e:
        out["remainder_rounds"] = {"error": repr(e)[:200]}
    # the same stack as a decoder block calls it: q|k|v and gate|up through gptq_forward_multi, which permutes x ONCE for layers that share their
    # activation order (4 permute launches per block instead of 7)
    grouped = None
    try:
        gl = group_stack(layers)
        gg, go = capture(gl, xs, device)
        settle(gg, device)
        _, evg = time_graph(gg, steps, device)
        grouped = {"TFLOP_s": round(flops_step * steps / evg / 1e12, 1), "ms_per_step": round(1e3 * evg / steps, 3),
                   "note": "q|k|v and gate|up of a block through gptq_forward_multi: one shared permuted x per group (they carry one g_idx, as GPTQ produces them)"}
        del gg, go
    except Exception as e:
        grouped = {"error": repr(e)[:200]}
    out["grouped"] = grouped
    del layers
    torch.cuda.empty_cache()
    return out


def _kernel_of(ent, M):
    """Name of the kernel a stack entry launches (host-side plan query)."""
    from autogptq_amd import _lib
    q = ent[3]
    if isinstance(q, list):                           # gptq_forward_multi: plain 4-bit layers, M <= 4 -- the decode-copy kernel when the layers carry the copy
        return f"gptq::gemv_tiled_kernel<{q[0].bits}," if all(getattr(l, "_qweight_tiled", None) is not None for l in q) else "gptq::gemv_q4_stream_kernel"
    d = _lib.describe_plan(q._layer, M)
    return {"stream": "gptq::gemv_q4_stream_kernel", "mfma": "gptq::gemv_q4_f16_mfma_kernel", "mfma_generic": "gptq::gemv_mfma_generic_kernel",
            "strips": f"gptq::gemv_tiled_kernel<{q.bits},", "tiled": "gptq::gemm_kernel"}.get(d.get("kernel"), "gptq::" + str(d.get("kernel")))


def _plan_dict(layers, K, N, M):
    from autogptq_amd import _lib
    for _, k, n, q in layers:
        if (k, n) == (K, N):
            return _lib.describe_plan(q._layer, M)
    return {}


def _plan_of(layers, K, N, M):
    return " ".join(f"{a}={b}" for a, b in _plan_dict(layers, K, N, M).items())


def bench_config5(device, steps):
    """BASELINE config 5: int3 / int8, group_size 32, Llama-7B shapes, M = 1 decode.  Per shape: a graph of distinct layers whose
    packed weights exceed the 256 MiB Infinity Cache, HIP events, algorithmic GB/s (SURVEY App. C formula).  On 4096 x 11008 also the
    act-order (desc_act=True) decode and the M = 2048 prefill of the same packing."""
    res = {}
    for bits in (3, 8):
        for K, N in ((4096, 4096), (4096, 11008), (11008, 4096)):
            wbytes = K * N * bits // 8
            n = max(4, -(-(320 << 20) // wbytes))
            ls = [(f"b{bits}", K, N, make_layer(K, N, device, bits=bits, gs=32, seed=5000 + i)) for i in range(n)]
            xs = {K: (torch.rand(1, K, device=device) - 0.5).half()}
            per = _time_layers(ls, xs, device, max(3, steps // 2))
            ab = algorithmic_bytes(K, N, 1, bits=bits, gs=32)
            res[f"int{bits}_g32_{K}x{N}"] = {"us": round(per * 1e6, 2), "GB_per_s": round(ab / per / 1e9, 1), "frac": round(ab / per / 1e9 / HBM_PEAK_GBS, 4),
                                              "plan": _plan_of(ls, K, N, 1)}
            if (K, N) == (4096, 11008):
                # the same packing on the other two paths of the config: act-order decode (desc_act=True) and M = 2048 prefill
                xp = {K: (torch.rand(2048, K, device=device) - 0.5).half()}
                perp = _time_layers(ls[:4], xp, device, 3)
                res[f"int{bits}_g32_{K}x{N}_prefill_M2048"] = {"us": round(perp * 1e6, 1), "TFLOP_s": round(2 * 2048 * K * N / perp / 1e12, 1),
                                                               "frac": round(2 * 2048 * K * N / perp / 1e12 / MFMA_PEAK_TFLOPS, 4),
                                                               "plan": _plan_of(ls, K, N, 2048)}
                del xp
                # batched decode rows on this packing (int8: the 8-bit form of gemm_mid_kernel; int3: skinny / tiled)
                for Mb in (16, 64):
                    xb = {K: (torch.rand(Mb, K, device=device) - 0.5).half()}
                    perb = _time_layers(ls, xb, device, max(3, steps // 2))
                    abb = algorithmic_bytes(K, N, Mb, bits=bits, gs=32)
                    res[f"int{bits}_g32_{K}x{N}_M{Mb}"] = {"us": round(perb * 1e6, 2), "GB_per_s": round(abb / perb / 1e9, 1), "frac": round(abb / perb / 1e9 / HBM_PEAK_GBS, 4),
                                                         "plan": _plan_of(ls, K, N, Mb)}
                    del xb
                la = [(f"b{bits}a", K, N, make_layer(K, N, device, bits=bits, gs=32, act_order=True, seed=6000 + i)) for i in range(n)]
                pera = _time_layers(la, xs, device, max(3, steps // 2))
                aba = algorithmic_bytes(K, N, 1, bits=bits, gs=32, act_order=True)
                res[f"int{bits}_g32_{K}x{N}_desc_act"] = {"us": round(pera * 1e6, 2), "GB_per_s": round(aba / pera / 1e9, 1),
                                                          "frac": round(aba / pera / 1e9 / HBM_PEAK_GBS, 4), "plan": _plan_of(la, K, N, 1)}
                del la
            del ls, xs
            torch.cuda.empty_cache()
        # the block's fused callers on this packing: q|k|v and gate|up through gptq_forward_multi (one streamed launch per group)
        for gname, K, Ns in (("qkv", 4096, (4096, 4096, 4096)), ("gate_up", 4096, (11008, 11008))):
            wbytes = K * sum(Ns) * bits // 8
            n = max(3, -(-(320 << 20) // wbytes))
            gs_ = [(gname, K, sum(Ns), [make_layer(K, nn, device, bits=bits, gs=32, seed=8000 + 10 * i + j) for j, nn in enumerate(Ns)]) for i in range(n)]
            xs = {K: (torch.rand(1, K, device=device) - 0.5).half()}
            per = _time_layers(gs_, xs, device, max(3, steps // 2))
            ab = sum(algorithmic_bytes(K, nn, 1, bits=bits, gs=32) for nn in Ns)
            res[f"int{bits}_g32_{gname}_one_launch"] = {"us": round(per * 1e6, 2), "GB_per_s": round(ab / per / 1e9, 1), "frac": round(ab / per / 1e9 / HBM_PEAK_GBS, 4),
                                                        "plan": "gptq_forward_multi: " + " | ".join(f"{K}x{nn}" for nn in Ns)}
            del gs_, xs
            torch.cuda.empty_cache()
    return res


def bench_batched(device, steps):
    """Batched decode (the reference's kernel switch sits at 8 / 50 rows: qlinear_cuda.py:34, q_gemm.cu:118): M = 16, 64 and 128 on the
    three Llama-7B shapes, int4 g128, distinct layers beyond the Infinity Cache, HIP events, algorithmic GB/s (and the MFMA fraction: at 128 rows
    the two rooflines cross)."""
    res = {}
    for M in (16, 64, 128):
        for K, N in ((4096, 4096), (4096, 11008), (11008, 4096)):
            n = max(4, -(-(320 << 20) // (K * N // 2)))
            ls = [("b", K, N, make_layer(K, N, device, seed=7000 + i)) for i in range(n)]
            xs = {K: (torch.rand(M, K, device=device) - 0.5).half()}
            per = _time_layers(ls, xs, device, max(3, steps // 2))
            ab = algorithmic_bytes(K, N, M)
            res[f"M{M}_{K}x{N}"] = {"us": round(per * 1e6, 2), "GB_per_s": round(ab / per / 1e9, 1), "frac": round(ab / per / 1e9 / HBM_PEAK_GBS, 4),
                                     "TFLOP_s": round(2 * M * K * N / per / 1e12, 1), "mfma_frac": round(2 * M * K * N / per / 1e12 / MFMA_PEAK_TFLOPS, 4),
                                     "plan": _plan_of(ls, K, N, M)}
            del ls, xs
            torch.cuda.empty_cache()
    # short prompts / large batches (a few hundred rows; round 6: the whole-K panel kernel, csrc/gemm_panel.hip, where its 64-row tiles fill the chip): 256 rows on
    # two shapes, 512 rows on all three
    for M, K, N in ((256, 4096, 4096), (256, 11008, 4096), (512, 4096, 4096), (512, 4096, 11008), (512, 11008, 4096)):
        n = max(4, -(-(320 << 20) // (K * N // 2)))
        ls = [("b", K, N, make_layer(K, N, device, seed=7100 + i)) for i in range(n)]
        xs = {K: (torch.rand(M, K, device=device) - 0.5).half()}
        per = _time_layers(ls, xs, device, max(3, steps // 2))
        res[(f"short_prompt_M{M}_{K}x{N}" if M == 256 else f"M{M}_{K}x{N}")] = {"us": round(per * 1e6, 2), "TFLOP_s": round(2 * M * K * N / per / 1e12, 1),
                                                                               "mfma_frac": round(2 * M * K * N / per / 1e12 / MFMA_PEAK_TFLOPS, 4), "plan": _plan_of(ls, K, N, M)}
        del ls, xs
        torch.cuda.empty_cache()
    # round 6: the other decode forms of the copy -- bf16 layers at 1 / 4 rows (4 rows: the zero-point on the matrix core) and 2-bit layers (their own copy since
    # round 6), 4096 -> 11008, HBM-cold rotating layers
    for tag, bits, dt, M in (("bf16_M1", 4, torch.bfloat16, 1), ("bf16_M4", 4, torch.bfloat16, 4), ("f16_M4", 4, torch.float16, 4), ("int2_M1", 2, torch.float16, 1), ("int2_M4", 2, torch.float16, 4)):
        K, N = 4096, 11008
        n = max(4, -(-(320 << 20) // (K * N * bits // 8)))
        ls = [("b", K, N, make_layer(K, N, device, bits=bits, dtype=dt, seed=7200 + i)) for i in range(n)]
        xs = {K: (torch.rand(M, K, device=device) - 0.5).to(dt)}
        per = _time_layers(ls, xs, device, max(3, steps // 2))
        ab = algorithmic_bytes(K, N, M, bits=bits)
        res[f"{tag}_{K}x{N}"] = {"us": round(per * 1e6, 2), "GB_per_s": round(ab / per / 1e9, 1), "frac": round(ab / per / 1e9 / HBM_PEAK_GBS, 4), "plan": _plan_of(ls, K, N, M)}
        del ls, xs
        torch.cuda.empty_cache()
    return res


def bench_warm_l3(device, steps, M=1):
    """"warm / L3 number reported separately".  ONE decoder block (its seven layers = 105 MB of packed weights: inside the 256 MiB Infinity
    Cache) as the same four launches the headline times, replayed back to back -- from the second replay on the weights come out of the cache, not the HBM.
    us per launch type (16 copies of the block's four launches per graph, median of `steps`+ replays) and the block's GB/s; the headline (cold, 224
    distinct layers = 3.37 GB) is the number to compare against: the difference is what the HBM costs the decode launches over the cache."""
    layers, xs = build_stack(device, 1, M, False)
    grouped = group_stack(layers)
    out = {"rows_per_step": M, "resident_bytes": int(sum(entry_bytes(e, M) for e in grouped)), "us_per_launch_by_shape": {}}
    total = 0.0
    for ent in grouped:
        name, K, N, q = ent
        g, o = capture([ent] * 16, xs, device)
        settle(g, device)
        ts = time_graph_each(g, max(20, steps), device)
        us = 1e6 * _pctl(ts, 0.5) / 16
        key = f"{name}:{K}x{N}" if isinstance(q, list) else f"{K}x{N}"
        out["us_per_launch_by_shape"][key] = round(us, 3)
        total += us
        del g, o
    out["us_per_block"] = round(total, 3)
    out["GB_per_s"] = round(out["resident_bytes"] / (total * 1e-6) / 1e9, 1)
    out["frac_of_hbm_peak"] = round(out["GB_per_s"] / HBM_PEAK_GBS, 4)
    return out


def bench_eager(layers, xs, device, steps):
    """The same 224 layers called one by one through QuantLinear.forward with no graph: what the reference's callers do
    (generate() under inference_mode, auto_gptq/modeling/_base.py:415-418).  Wall clock per call incl. Python + ctypes."""
    # One timed pass is a few milliseconds of host work (128 calls x ~6 us x steps): a single collector pause or scheduler hiccup inside it read as 10 - 17 us
    # per call on boxes whose other passes read 6.5 (profiles/r05_bench*.json).  Five passes with the cyclic collector off; the MEDIAN pass is reported, the
    # spread beside it.
    import gc
    passes = []
    with torch.no_grad():
        for _ in range(2):
            for _, K, N, q in layers:
                call(q, xs[K])
        torch.cuda.synchronize(device)
        gc_was = gc.isenabled()
        gc.disable()
        try:
            for _ in range(5):
                t0 = time.perf_counter()
                for _ in range(steps):
                    for _, K, N, q in layers:
                        call(q, xs[K])
                t_issue = time.perf_counter() - t0
                torch.cuda.synchronize(device)
                passes.append((time.perf_counter() - t0, t_issue))
        finally:
            if gc_was:
                gc.enable()
    passes.sort()
    t, t_issue = passes[len(passes) // 2]
    M = next(iter(xs.values())).shape[0]
    bytes_step = sum(entry_bytes(e, M) for e in layers)
    n_calls = steps * len(layers)
    return {"calls_per_step": len(layers), "us_per_call": round(1e6 * t / n_calls, 2),
            "host_us_per_call": round(1e6 * t_issue / n_calls, 2),
            "us_per_call_min_max": [round(1e6 * passes[0][0] / n_calls, 2), round(1e6 * passes[-1][0] / n_calls, 2)],
            "GB_per_s": round(bytes_step * steps / t / 1e9, 1), "tokens_per_s": round(M * steps / t, 1),
            "note": "eager calls (torch.empty + C-ABI call + launch per call), no hipGraph; median of 5 passes, cyclic GC off while timing"}


def cpu_baseline(M, act_order, budget_s=20.0, device=None):
    """Time the oracle (a port of the reference's pure-PyTorch CPU QuantLinear.forward: materialise
    the unpacked ints, dequantise, torch.matmul) on the host cores, on a bounded sample: the three
    distinct Llama-7B layer shapes, a few repetitions each.  With a device: the SAME three layers and inputs also go through the product's
    default plan (the kernels the headline times) and every output is compared with what the CPU computed -- the oracle as the checker of
    the measured path ("gpu_vs_cpu"), at the reference's own tolerance for this comparison (tests/test_q4.py: 1e-3 relative + absolute on
    outputs of this size)."""
    from oracle import gptq_oracle as O

    # the reference class was timed on 8 threads in the build container; 128 threads make these small tensor ops
    # slower, not faster (measured here: 4096 x 4096 77 ms on 128 threads against ~35 ms on 8-16)
    threads = min(16, torch.get_num_threads())
    torch.set_num_threads(threads)
    total_b, total_t, reps_done = 0, 0.0, []
    gpu_check = {"shapes": 0, "outputs": 0, "max_err_over_max_out": 0.0, "tolerance": "1e-3 * max|y_cpu| + 1e-3 * |y_cpu| per output", "ok": True,
                 "what": "the product's default plan on the same layers and inputs, every output against the CPU result timed here"}
    per_shape = budget_s / 3
    # Where GPTQ_REFERENCE names a reference tree its OWN class is what is timed -- kind "reference": auto_gptq/nn_modules/qlinear/qlinear_cuda_old.py
    # (qlinear_cuda.py for act-order) loaded by file path, as tools/time_reference_cpu.py does.  Without it, the port (kind "port").
    ref_cls = None
    ref_root = os.environ.get("GPTQ_REFERENCE", "")
    ref_file = os.path.join(ref_root, "auto_gptq/nn_modules/qlinear", "qlinear_cuda.py" if act_order else "qlinear_cuda_old.py")
    if ref_root and os.path.exists(ref_file):
        try:
            import importlib.util
            spec = importlib.util.spec_from_file_location("ref_qlinear_for_bench", ref_file)
            mod = importlib.util.module_from_spec(spec)
            spec.loader.exec_module(mod)
            ref_cls = mod.QuantLinear
        except Exception:
            ref_cls = None
    for K, N in ((4096, 4096), (4096, 11008), (11008, 4096)):
        L = O.random_quant_layer(K, N, 4, 128, act_order=act_order, seed=1)
        x = (torch.rand(M, K) - 0.5).half()
        mode = O.reference_zero_mode(act_order, 4)
        gi = L["g_idx"] if act_order else None
        if ref_cls is not None:
            q = ref_cls(4, 128, K, N, False)
            q.qweight, q.qzeros, q.scales, q.g_idx = L["qweight"], L["qzeros"], L["scales"], L["g_idx"]
            fwd = lambda: q(x)                                        # noqa: E731
        else:
            fwd = lambda: O.forward_fast(x, L["qweight"], L["qzeros"], L["scales"], gi, None, 4, mode)      # noqa: E731
        with torch.no_grad():
            fwd()                                                    # warm-up
            n, t_acc = 0, 0.0
            while t_acc < per_shape and n < 200:                     # ~ 15-20 s of host work in total
                t0 = time.perf_counter()
                fwd()
                t_acc += time.perf_counter() - t0
                n += 1
        total_b += n * algorithmic_bytes(K, N, M, act_order=act_order)
        total_t += t_acc
        reps_done.append(f"{K}x{N}x{n}")
        if device is not None:
            try:
                import autogptq_amd
                with torch.no_grad():
                    y_cpu = fwd().float()
                    g = autogptq_amd.QuantLinear(4, 128, K, N, False)
                    g.qweight, g.qzeros, g.scales, g.g_idx = L["qweight"].clone(), L["qzeros"].clone(), L["scales"].clone(), L["g_idx"].clone()
                    g = g.to(device)
                    g.post_init()
                    y_gpu = g(x.to(device)).float().cpu()
                    del g
                err = (y_gpu - y_cpu).abs()
                bound = 1e-3 * float(y_cpu.abs().max()) + 1e-3 * y_cpu.abs()
                gpu_check["shapes"] += 1
                gpu_check["outputs"] += int(err.numel())
                gpu_check["max_err_over_max_out"] = round(max(gpu_check["max_err_over_max_out"], float(err.max()) / (float(y_cpu.abs().max()) or 1.0)), 6)
                gpu_check["ok"] = bool(gpu_check["ok"] and bool((err <= bound).all()))
            except Exception as e:
                gpu_check["error"] = repr(e)[:200]
                gpu_check["ok"] = False
    # SURVEY 8(d) "reference CPU path timed beside it": also one thread, and fp32 inputs (the reference's CPU path computes in the input's type), on
    # 4096 x 4096: 3 warm-ups + 10 repetitions each, wall clock, ms per forward (median)
    extra = {}
    try:
        K = N = 4096
        L = O.random_quant_layer(K, N, 4, 128, act_order=act_order, seed=1)
        mode = O.reference_zero_mode(act_order, 4)
        gi = L["g_idx"] if act_order else None

        def timed_ms(xin, scales, nthreads):
            torch.set_num_threads(nthreads)
            f = lambda: O.forward_fast(xin, L["qweight"], L["qzeros"], scales, gi, None, 4, mode)      # noqa: E731
            with torch.no_grad():
                for _ in range(3):
                    f()
                ts = []
                for _ in range(10):
                    t0 = time.perf_counter()
                    f()
                    ts.append(time.perf_counter() - t0)
            return round(1e3 * sorted(ts)[len(ts) // 2], 2)
        x16 = (torch.rand(M, K) - 0.5).half()
        extra["ms_4096x4096_fp16_threads_%d" % threads] = timed_ms(x16, L["scales"], threads)
        extra["ms_4096x4096_fp16_threads_1"] = timed_ms(x16, L["scales"], 1)
        extra["ms_4096x4096_fp32_threads_%d" % threads] = timed_ms(x16.float(), L["scales"].float(), threads)
        extra["ms_4096x4096_fp32_threads_1"] = timed_ms(x16.float(), L["scales"].float(), 1)
    except Exception as e:
        extra["error"] = repr(e)[:200]
    finally:
        torch.set_num_threads(threads)
    return {"value": round(total_b / total_t / 1e9, 4), "unit": "GB/s", "cores": threads, "kind": "reference" if ref_cls is not None else "port",
            "protocol_8d": extra,
            "sample": (("the reference's own QuantLinear.forward (%s, loaded by path), " % os.path.basename(ref_file)) if ref_cls is not None else
                       "oracle.forward_fast = the reference's own broadcast shift+mask unpack (qlinear_cuda_old.py:295-349) + torch.matmul, ") +
                      "torch CPU fp16, M=%d, shapes x reps: %s" % (M, ", ".join(reps_done)),
            "ms_per_layer_mean": round(1e3 * total_t / sum(int(r.split('x')[2]) for r in reps_done), 2),
            # the reference CLASS itself (qlinear_cuda_old.QuantLinear.forward, loaded from the reference tree) timed on 8 cores,
            # ms per forward on 4096x4096 / 4096x11008 / 11008x4096: it cannot run on the GPU box, so this port is what is timed here
            "reference_class_ms_build_container": [30.4, 768, 305],
            **({"gpu_vs_cpu": gpu_check} if device is not None else {})}


def bench_tp(device, rank, world, steps, peer_store=False):
    """Column-parallel Llama-2-70B shapes (BASELINE config 4): local kernel + one all-gather, M = 1 (decode) and M = 2048
    (prefill); and the Megatron pairing of an MLP block -- column-parallel gate / up without gather feeding a row-parallel
    down projection: ONE all-reduce per block.  Eager calls (RCCL on the layer's stream), HIP events, max over ranks; the M = 1
    entries again as hipGraph replays (`*_graph`: eight calls per graph, the collective captured with the kernels).
    peer_store (--tp-exchange peer_store, experimental): the M = 1 layers again with the direct peer-store exchange of
    csrc/peer.hip instead of the collective (never exercised across GPUs by the builder: 1-GPU boxes only)."""
    import torch.distributed as dist
    from autogptq_amd.tensor_parallel import ColumnParallelQuantLinear, RowParallelQuantLinear

    def timed(fn, n):
        for _ in range(3):
            fn()
        torch.cuda.synchronize(device)
        dist.barrier()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            out = fn()
        e1.record()
        torch.cuda.synchronize(device)
        return e0.elapsed_time(e1) * 1e-3 / n, out

    def graphed(fn, calls=8, reps=10):
        """`calls` forward calls captured in ONE hipGraph (the collective included: RCCL captures like any other stream work), `reps` replays
        between HIP events; (seconds per call, None) or (None, reason).  Every rank replays or none does: the capture verdicts are reduced first."""
        ok, why, g, keep = 1, None, None, None
        try:
            side = torch.cuda.Stream(device=device)
            side.wait_stream(torch.cuda.current_stream(device))
            with torch.cuda.stream(side), torch.no_grad():
                fn()                                  # workspace / communicator / exchange buffers exist before the capture
            torch.cuda.current_stream(device).wait_stream(side)
            torch.cuda.synchronize(device)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=side), torch.no_grad():
                keep = [fn() for _ in range(calls)]
        except Exception as e:
            ok, why = 0, "capture: " + repr(e)[:160]
        flag = torch.tensor([ok], device=device, dtype=torch.int32)
        dist.all_reduce(flag, op=dist.ReduceOp.MIN)
        if int(flag.item()) == 0:
            return None, why or "capture failed on another rank"
        for _ in range(2):
            g.replay()
        torch.cuda.synchronize(device)
        dist.barrier()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            g.replay()
        e1.record()
        torch.cuda.synchronize(device)
        del keep
        return e0.elapsed_time(e1) * 1e-3 / (reps * calls), None

    def put_graphed(ent, key, fn):
        try:
            t_g, why = graphed(fn)
            if t_g is None:
                ent[key + "_error"] = why
            else:
                t = torch.tensor([t_g], device=device)
                dist.all_reduce(t, op=dist.ReduceOp.MAX)
                ent[key] = round(t.item() * 1e6, 2)
        except Exception as e:
            ent[key + "_error"] = repr(e)[:200]

    res = {}
    for name, K, N in LLAMA70B_TP:
        nl = N // world
        local = make_layer(K, nl, device, seed=rank)
        mod = ColumnParallelQuantLinear(local, N)
        ent = {"K": K, "N": N, "tp": world}
        for M, n in ((1, steps), (2048, max(3, steps // 10))):
            try:
                x = (torch.rand(M, K, device=device) - 0.5).half()
                with torch.no_grad():
                    t_all, y = timed(lambda: mod(x), n)
                    t_loc, _ = timed(lambda: local(x), n)
                t = torch.tensor([t_all, t_loc], device=device)
                dist.all_reduce(t, op=dist.ReduceOp.MAX)
                key = "" if M == 1 else f"_m{M}"
                ent["us_per_layer_with_allgather" + key] = round(t[0].item() * 1e6, 2)
                ent["us_local_only" + key] = round(t[1].item() * 1e6, 2)
                ent["out_cols"] = int(y.shape[-1])
                if M == 1:                            # decode is launch-bound: the number that matters is the graph-captured one
                    put_graphed(ent, "us_per_layer_with_allgather_graph", lambda: mod(x))
                    put_graphed(ent, "us_local_only_graph", lambda: local(x))
            except Exception as e:
                ent[f"error_m{M}"] = repr(e)[:200]
        if peer_store:
            try:
                modp = ColumnParallelQuantLinear(local, N, exchange="peer_store", max_rows=1)
                x = (torch.rand(1, K, device=device) - 0.5).half()
                with torch.no_grad():
                    t_ps, yp = timed(lambda: modp(x), steps)
                modp._px.check_timeout()
                t = torch.tensor([t_ps], device=device)
                dist.all_reduce(t, op=dist.ReduceOp.MAX)
                ent["us_per_layer_with_peer_store"] = round(t[0].item() * 1e6, 2)
                ent["peer_store_equals_allgather"] = bool(torch.equal(yp, mod(x)))
                put_graphed(ent, "us_per_layer_with_peer_store_graph", lambda: modp(x))      # kernels only: local kernel (scatter in its epilogue) + collect
                ent["peer_store_scatter_fused_into_kernel"] = bool(modp.fused_calls > 0)
                if modp.fused_calls > 0:            # the round-3 form beside it: local kernel + scatter launch + collect launch
                    fused_fn, modp._fused_peer_forward = modp._fused_peer_forward, (lambda x_: None)
                    try:
                        put_graphed(ent, "us_per_layer_with_peer_store_unfused_graph", lambda: modp(x))
                    finally:
                        modp._fused_peer_forward = fused_fn
                modp._px.check_timeout()
                dist.barrier()
                del modp
            except Exception as e:
                ent["error_peer_store"] = repr(e)[:200]
        res[name] = ent
        del local, mod
    try:      # MLP block 8192 -> 28672 -> 8192: gate/up column shards (no gather) -> down row shard (one all-reduce)
        K, I = 8192, 28672
        gate = make_layer(K, I // world, device, seed=100 + rank)
        up = make_layer(K, I // world, device, seed=200 + rank)
        down = RowParallelQuantLinear(make_layer(I // world, K, device, seed=300 + rank), (rank * (I // world), (rank + 1) * (I // world)))
        ent = {"K": K, "I": I, "tp": world}
        for M, n in ((1, steps), (2048, max(3, steps // 10))):
            x = (torch.rand(M, K, device=device) - 0.5).half()

            def block():
                return down(torch.nn.functional.silu(gate(x)) * up(x))
            with torch.no_grad():
                t_blk, _ = timed(block, n)
            t = torch.tensor([t_blk], device=device)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            ent["us_per_block" + ("" if M == 1 else f"_m{M}")] = round(t[0].item() * 1e6, 2)
            if M == 1:
                put_graphed(ent, "us_per_block_graph", block)
        res["mlp_column_row_pair"] = ent
    except Exception as e:
        res["mlp_column_row_pair"] = {"error": repr(e)[:200]}
    return res


LLAMA70B_BLOCK = [("q_proj", 8192, 8192), ("k_proj", 8192, 1024), ("v_proj", 8192, 1024), ("o_proj", 8192, 8192),
                  ("gate_proj", 8192, 28672), ("up_proj", 8192, 28672), ("down_proj", 28672, 8192)]


def bench_tp_stack(device, rank, world, n_blocks, M, steps, warmup, exchange="all_gather", outputs=None):
    """BASELINE config 4 as a STACK (round 6: the N > 1 headline): the seven quantized linears of `n_blocks` Llama-2-70B decoder blocks (GQA: 1024-column k / v),
    every layer split over out_features across the ranks (north_star: "the per-layer matmul shards naturally over out_features ... a single RCCL all-gather") --
    rank r holds columns [r N / T, (r + 1) N / T) of every layer, runs its shard's kernel and the layer's outputs are all-gathered.  One step = M rows through all
    7 n_blocks layers, ONE hipGraph per rank (the collectives captured with the kernels: RCCL captures like any other stream work); `steps` replays between
    barrier + synchronize, MAX over ranks.  value = the algorithmic bytes of ALL shards per second (whole job).  The same graph WITHOUT the exchange is timed
    beside it: what the all-gathers cost.  Falls back to eager calls when a capture fails (then launch-bound, and says so).
    outputs: a list that receives the gathered outputs of the last timed step with the exchange, one tensor per layer in stack order."""
    import torch.distributed as dist
    from autogptq_amd.tensor_parallel import ColumnParallelQuantLinear
    mods, shard_bytes = [], 0
    for b in range(n_blocks):
        for i, (name, K, N) in enumerate(LLAMA70B_BLOCK):
            local = make_layer(K, N // world, device, seed=(b * 16 + i) * 64 + rank)
            mods.append((K, local, ColumnParallelQuantLinear(local, N, exchange=exchange, max_rows=max(1, M))))
            shard_bytes += algorithmic_bytes(K, N // world, M)
    gx = torch.Generator(device=device).manual_seed(30_000)
    xs = {K: (torch.rand(M, K, device=device, generator=gx) - 0.5).half() for K in (8192, 28672)}

    def step_with():
        return [m(xs[K]) for K, _, m in mods]

    def step_local():
        return [l(xs[K]) for K, l, _ in mods]

    def run(fn, last=None):
        """(seconds per step, max over ranks; 'graph' | 'eager: <why>'); `last` (a list) receives the outputs of the last timed step"""
        how, g, keep = "graph", None, None
        ok = 1
        try:
            side = torch.cuda.Stream(device=device)
            side.wait_stream(torch.cuda.current_stream(device))
            with torch.cuda.stream(side), torch.no_grad():
                fn()
            torch.cuda.current_stream(device).wait_stream(side)
            torch.cuda.synchronize(device)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=side), torch.no_grad():
                keep = fn()
        except Exception as e:
            ok, how = 0, "eager: capture failed (" + repr(e)[:120] + ")"
        flag = torch.tensor([ok], device=device, dtype=torch.int32)
        dist.all_reduce(flag, op=dist.ReduceOp.MIN)
        use_graph = int(flag.item()) == 1
        if not use_graph and ok:
            how = "eager: capture failed on another rank"
        with torch.no_grad():
            one = (lambda: g.replay()) if use_graph else fn
            for _ in range(max(1, warmup)):
                one()
            torch.cuda.synchronize(device)
            dist.barrier()
            torch.cuda.synchronize(device)
            t0 = time.perf_counter()
            for _ in range(steps):
                ys = one()
            torch.cuda.synchronize(device)
            dist.barrier()
            wall = time.perf_counter() - t0
        t = torch.tensor([wall], device=device)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        if last is not None:
            last.extend(keep if use_graph else ys)
        del keep
        return t.item() / steps, how

    t_with, how_with = run(step_with, outputs)
    t_loc, how_loc = run(step_local)
    devs = [None] * world
    dist.all_gather_object(devs, {"rank": rank, "device": str(device), "name": torch.cuda.get_device_name(device),
                                  "pci": getattr(torch.cuda.get_device_properties(device), "pci_bus_id", None)})
    res = {"workload": "Llama-2-70B linear shapes (8192->8192 x2, 8192->1024 x2 (GQA k / v), 8192->28672 x2, 28672->8192) x %d blocks = %d layers, int4 g128, "
                       "every layer split over out_features across %d ranks + one all-gather per layer, M=%d rows per step" % (n_blocks, len(mods), world, M),
           "tp": world, "blocks": n_blocks, "layers": len(mods), "rows_per_step": M, "exchange": exchange,
           "backend": dist.get_backend(), "nccl_world": dist.get_world_size(), "rank_devices": devs,
           "ms_per_step": round(1e3 * t_with, 4), "ms_per_step_local_kernels_only": round(1e3 * t_loc, 4),
           "exchange_ms_per_step": round(1e3 * (t_with - t_loc), 4), "exchange_share": round(max(0.0, t_with - t_loc) / t_with, 4),
           "timed_as": how_with, "local_timed_as": how_loc,
           "algorithmic_bytes_per_step_per_rank": shard_bytes,
           "GB_per_s_per_gpu": round(shard_bytes / t_with / 1e9, 1), "GB_per_s": round(world * shard_bytes / t_with / 1e9, 1),
           "GB_per_s_local_kernels_only": round(world * shard_bytes / t_loc / 1e9, 1),
           "frac_per_gpu": round(shard_bytes / t_with / 1e9 / HBM_PEAK_GBS, 4),
           "tokens_per_s": round(M / t_with, 1)}
    del mods, xs
    torch.cuda.empty_cache()
    return res


def _watchdog(seconds: float):
    """A wedged GPU call never returns to Python; a timer thread (the GIL is released inside HIP calls) ends the process
    instead of letting the launcher's own limit expire on a hung box."""
    import threading

    def fire():
        sys.stderr.write(f"bench.py: no result after {seconds:.0f} s -- aborting (BENCH_WATCHDOG_S to change)\n")
        sys.stderr.flush()
        os._exit(3)
    t = threading.Timer(seconds, fire)
    t.daemon = True
    t.start()
    return t


def _deadline(seconds: float, on_expire):
    """Run `on_expire` on a timer thread unless the returned finish() is called first; finish() says whether it won the race."""
    import threading
    lock, state = threading.Lock(), {"done": False}

    def fire():
        with lock:
            if state["done"]:
                return
            state["done"] = True
        on_expire()
    t = threading.Timer(seconds, fire)
    t.daemon = True
    t.start()

    def finish():
        with lock:
            if state["done"]:
                return False
            state["done"] = True
        t.cancel()
        return True
    return finish


def main():
    _watchdog(float(os.environ.get("BENCH_WATCHDOG_S", "900")))
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--workload", default="decode", choices=["decode", "prefill"])
    ap.add_argument("--blocks", type=int, default=32, help="decoder blocks in the stack (32 = Llama-7B)")
    ap.add_argument("--m", type=int, default=0, help="rows per step (default 1 for decode, 2048 for prefill)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-tp", action="store_true")
    ap.add_argument("--backend", default="nccl", help="torch.distributed backend (nccl = RCCL; gloo only for launcher smoke tests)")
    ap.add_argument("--same-device", action="store_true", help="testing only: every rank uses cuda:0 (needs --backend gloo)")
    ap.add_argument("--no-fused", action="store_true", help="skip the extra fused-callers measurement (decode, 1 GPU only)")
    ap.add_argument("--per-layer", action="store_true", help="decode: 224 separate launches per step (no gptq_forward_multi grouping)")
    ap.add_argument("--no-extras", action="store_true", help="decode, 1 GPU: skip the prefill / config5 / eager blocks of the default line")
    ap.add_argument("--tp-blocks", type=int, default=16, help="N > 1: Llama-2-70B decoder blocks in the tensor-parallel stack (80 = the whole model)")
    ap.add_argument("--no-tp-layers", action="store_true", help="N > 1: skip the per-layer tensor-parallel entries (roofline.tp<N>_attn_* ...), keep the stack")
    ap.add_argument("--tp-exchange", default="all_gather", choices=["all_gather", "peer_store"],
                    help="tp block: also time the experimental direct peer-store exchange (csrc/peer.hip) next to the collective")
    ap.add_argument("--full", action="store_true",
                    help="also run everything beside the headline: roofline per launch type, timed-output check, eager / fused / MLP / prefill / config 5 / "
                         "batched / warm-cache blocks, CPU baseline, per-layer tensor-parallel entries (the --no-* options still trim it)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the timed path returned in its last step as DIR/<block>_<layer>.npy (float32, <= 64 MB in all)")
    args = ap.parse_args()

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if args.gpus != world:
        if world == 1 and args.gpus > 1:
            sys.exit("bench.py --gpus N>1 must be launched with torch.distributed.run (one rank per GPU)")
    if args.same_device:
        local_rank = 0
    torch.cuda.set_device(local_rank)
    device = torch.device("cuda", local_rank)
    barrier = None
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if args.backend == "nccl":
            dist.init_process_group("nccl", device_id=device)
        else:
            dist.init_process_group(args.backend)
        barrier = dist.barrier

    prefill = args.workload == "prefill"
    M = args.m or (2048 if prefill else 1)
    act_order = prefill                      # BASELINE config 3: desc_act=True on the prefill path
    n_blocks = args.blocks if not prefill else min(args.blocks, 4)
    flat_layers, xs = build_stack(device, n_blocks, M, act_order)
    # decode: the block's q/k/v and gate/up go through gptq_forward_multi (one launch per group); --per-layer keeps 224 launches
    layers = flat_layers if (prefill or args.per_layer) else group_stack(flat_layers)
    g, outs = capture(layers, xs, device)

    # A fresh box can take a few hundred milliseconds to leave its idle clocks (one first-command run of this bench read 3050 GB/s where the next two read
    # 3470 / 3480): part of the untimed setup is therefore a fixed 0.25 s of replays -- then the W warm-up steps and the K timed steps the contract names.
    settle(g, device, 0.25)
    for _ in range(args.warmup):
        g.replay()
    wall, ev = time_graph(g, args.steps, device, barrier)
    if world > 1:
        t = torch.tensor([wall], device=device)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        wall = t.item()
    # --dump-outputs: the timed graph's outputs hold its last step; with N > 1 and the tensor-parallel stack as the headline, that stack's are written instead
    dump_here = args.dump_outputs and rank == 0 and not (world > 1 and not args.no_tp and not prefill)
    if dump_here:
        dump_outputs(args.dump_outputs, stack_output_names(n_blocks), flatten_outputs(outs))

    bytes_step = sum(entry_bytes(e, M, act_order) for e in layers)
    flops_step = sum(2 * M * K * N for _, K, N, _ in layers)
    launches = len(layers)

    # ---- roofline of the dominant kernel: a graph holding only that layer type --------------------
    roof = None
    if rank == 0 and args.full:
      try:
        by_type = {}
        for ent in layers:
            by_type.setdefault((ent[0] if isinstance(ent[3], list) else "", ent[1], ent[2]), []).append(ent)
        best = None
        per_type, spread = {}, {}
        for (gname, K, N), ls in by_type.items():
            gg, oo = capture(ls, xs, device)
            settle(gg, device)
            reps = max(3, args.steps // 2)
            _, evt = time_graph(gg, reps, device)
            per = evt / (reps * len(ls))
            share = per * len(ls)
            ent = dict(K=K, N=N, per_launch_s=per, share=share, n=len(ls), gname=gname, bytes=entry_bytes(ls[0], M, act_order),
                       kernel=_kernel_of(ls[0], M))
            per_type[(gname + ":" if gname else "") + f"{K}x{N}"] = round(per * 1e6, 3)
            each = [t / len(ls) for t in time_graph_each(gg, max(20, 4 * reps), device)]      # per launch, one value per replay of the type's graph
            spread[(gname + ":" if gname else "") + f"{K}x{N}"] = [round(_pctl(each, q) * 1e6, 3) for q in (0.1, 0.5, 0.9)]
            if best is None or share > best["share"]:
                best = ent
            del gg, oo
        K, N = best["K"], best["N"]
        if prefill:
            ach = 2 * M * K * N / best["per_launch_s"] / 1e12
            roof = {"bound": "mfma", "achieved": round(ach, 2), "peak": MFMA_PEAK_TFLOPS, "unit": "TFLOP/s",
                    "frac": round(ach / MFMA_PEAK_TFLOPS, 4), "traffic": None}
        else:
            ach = best["bytes"] / best["per_launch_s"] / 1e9
            roof = {"bound": "hbm", "achieved": round(ach, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                    "frac": round(ach / HBM_PEAK_GBS, 4), "traffic": None}
        roof["kernel"] = "gptq::gemm_kernel<4, f16, 4, 64>" if prefill else best["kernel"]
        roof["traffic"] = pmc_traffic(roof["kernel"], K, N, M)
        if roof["kernel"].endswith(","):
            roof["kernel"] += " MT, U, T, MAXW>"
        roof["shape"] = (f"{best['gname']}: " if best["gname"] else "") + f"K={K} N={N} M={M}" + (" (layers of one gptq_forward_multi launch)" if best["gname"] else "")
        roof["us_per_launch_events"] = round(best["per_launch_s"] * 1e6, 3)
        roof["us_per_launch_by_shape"] = per_type
        roof["us_per_launch_p10_p50_p90_by_shape"] = spread
        roof["algorithmic_bytes_per_launch"] = best["bytes"]
        if prefill and act_order:
            roof["note"] = "per-launch time includes the x column-permute launch of act-order layers (rocprof splits them: profiles/)"
      except Exception as e:
        roof = {"error": repr(e)[:300]}

    out = None
    if rank == 0:
        if prefill:
            value, unit, metric = flops_step * args.steps * world / wall / 1e12, "TFLOP/s", \
                "int4 g128 QuantLinear fwd TFLOP/s, Llama-7B shapes, prefill (desc_act)"
        else:
            value, unit, metric = bytes_step * args.steps * world / wall / 1e9, "GB/s", \
                "int4 g128 QuantLinear fwd GB/s + tokens/s, Llama-7B shapes"
        out = {
            "metric": metric, "value": round(value, 2), "unit": unit, "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": round(1e3 * wall / args.steps, 4), "higher_is_better": True,
            "scaling": "weak", "vs_baseline": None, "dtype": "f16", "data": "synthetic",
            "config": {"workload": ("Llama-7B linear shapes (4096->4096 x4, 4096->11008 x2, 11008->4096) x %d blocks = %d layers, int4 g128 %s, "
                                    "M=%d rows per step, %d launches/step in one hipGraph%s" %
                                    (n_blocks, len(flat_layers), "desc_act=True" if act_order else "no act-order", M, launches,
                                     "" if launches == len(flat_layers) else " (q|k|v and gate|up of a block: one gptq_forward_multi launch each)")),
                       "rows_per_step": M, "layers": len(flat_layers), "launches": launches, "parallelism": f"dp{world}" if world > 1 else "single"},
            "tokens_per_s": round(M * args.steps * world / wall, 1),
            "tokens_per_s_note": "linear-only (the %d quantized linears of the stack; no attention/norm)" % len(flat_layers),
            "event_ms_per_step_rank0": round(1e3 * ev / args.steps, 4),
            "algorithmic_bytes_per_step": bytes_step,
        }
        if args.full:
            verify = verify_timed_outputs(layers, outs, xs)      # behind every timed region of the headline (it idles the GPU)
            out["roofline"], out["verify"] = roof, verify
            if isinstance(roof, dict) and isinstance(verify, dict) and "ok" in verify:
                roof["timed_outputs_verified"] = verify["ok"]
    # The tensor-parallel block is extra information: it runs with the headline already built, under a deadline of its own -- a hung or failed
    # collective (one rank raising inside a capture while the others wait) costs the `tp` object, never the line the driver reads.
    if world > 1 and not args.no_tp and not prefill:
        tp_limit = float(os.environ.get("BENCH_TP_DEADLINE_S", "240"))

        def tp_expired():
            if rank == 0:
                out["tp"] = {"error": f"tp block did not finish within {tp_limit:.0f} s (a rank hung or a collective failed); skipped"}
                if isinstance(roof, dict):
                    roof["tp"] = out["tp"]
                print(json.dumps(out))
                sys.stdout.flush()
            os._exit(0)
        finish = _deadline(tp_limit, tp_expired)
        tp_outs = []
        try:
            tp = {}
            # the N > 1 HEADLINE (round 6): the tensor-parallel stack of BASELINE config 4 -- north_star's partitioning, timed with its exchange
            try:
                tp["stack"] = bench_tp_stack(device, rank, world, args.tp_blocks, M, args.steps, args.warmup, exchange=args.tp_exchange, outputs=tp_outs)
            except Exception as e:
                tp["stack"] = {"error": repr(e)[:300]}
            if args.full and not args.no_tp_layers:
                tp.update(bench_tp(device, rank, world, 50, peer_store=(args.tp_exchange == "peer_store")))
        except Exception as e:                       # the headline line must still be printed
            tp = {"error": repr(e)[:300]}
        if not finish():
            time.sleep(3600)                          # the timer thread is printing the line and ending the process
        if rank == 0:
            out["tp"] = tp
            st = tp.get("stack")
            if isinstance(st, dict) and "GB_per_s" in st:
                # The tensor-parallel stack becomes the line's value; the data-parallel replicas (each rank its own Llama-7B stack: trivially linear) move
                # to `dp_replicas`.  Scaling is STRONG: the model is fixed, every added rank takes a smaller shard of every layer.
                out["dp_replicas"] = {k: out[k] for k in ("value", "unit", "ms_per_step", "tokens_per_s", "algorithmic_bytes_per_step") if k in out}
                out["dp_replicas"]["workload"] = out["config"]["workload"]
                out["value"], out["ms_per_step"], out["tokens_per_s"] = st["GB_per_s"], st["ms_per_step"], st["tokens_per_s"]
                out["algorithmic_bytes_per_step"] = st["algorithmic_bytes_per_step_per_rank"] * world
                out["scaling"] = "strong"
                out["metric"] = "int4 g128 QuantLinear fwd GB/s + tokens/s, Llama-2-70B shapes split over out_features (TP=%d) + one all-gather per layer" % world
                out["config"] = {"workload": st["workload"], "rows_per_step": M, "layers": st["layers"], "launches": st["layers"],
                                 "parallelism": f"tp{world}", "exchange": st["exchange"], "backend": st["backend"], "nccl_world": st["nccl_world"],
                                 "rank_devices": st["rank_devices"], "timed_as": st["timed_as"]}
                out["tokens_per_s_note"] = "linear-only (the %d quantized linears of %d Llama-2-70B blocks; no attention/norm)" % (st["layers"], st["blocks"])
            else:
                out["config"]["parallelism"] = f"dp{world} (the tensor-parallel stack failed: {str((st or {}).get('error'))[:120]}); tp{world} layer entries in roofline.tp{world}_*"
            if args.dump_outputs:
                if isinstance(st, dict) and "GB_per_s" in st and tp_outs:
                    dump_outputs(args.dump_outputs, [f"b{b:02d}_{name}" for b in range(args.tp_blocks) for name, _, _ in LLAMA70B_BLOCK], tp_outs)
                else:
                    dump_outputs(args.dump_outputs, stack_output_names(n_blocks), flatten_outputs(outs))
            if isinstance(roof, dict):
                roof["tp"] = tp                       # the driver keeps `roofline` whole and drops unknown top-level keys
                # BASELINE config 4 (Llama-2-70B shapes, out_features split over the ranks + one all-gather) as flat scalars beside the DP headline
                try:
                    pre = f"tp{world}_"
                    for lname, ent in tp.items():
                        if not isinstance(ent, dict):
                            continue
                        short = {"attn_qkvo": "attn", "mlp_gate_up": "gate_up", "mlp_column_row_pair": "mlp_pair"}.get(lname, lname)
                        for k, v in ent.items():
                            if isinstance(v, (int, float)) and k.startswith("us_"):
                                roof[pre + short + "_" + k[3:]] = v
                    for short in ("attn", "gate_up"):
                        ent = tp.get(short) or {}
                        w_ = ent.get("us_per_layer_with_allgather_graph", ent.get("us_per_layer_with_allgather"))
                        l_ = ent.get("us_local_only_graph", ent.get("us_local_only"))
                        if w_ is not None:
                            roof[pre + short + "_us"] = w_
                        if short == "attn" and w_ is not None and l_ is not None:
                            roof[pre + "local_us"], roof[pre + "allgather_us"] = l_, round(w_ - l_, 2)
                    if isinstance(st, dict) and "GB_per_s" in st:
                        for k in ("ms_per_step", "ms_per_step_local_kernels_only", "exchange_ms_per_step", "exchange_share", "GB_per_s", "GB_per_s_per_gpu",
                                  "GB_per_s_local_kernels_only", "frac_per_gpu"):
                            roof[pre + "stack_" + k] = st[k]
                        roof["dp_value_GB_per_s"] = out["dp_replicas"].get("value")
                except Exception as e:
                    roof["tp_flat_keys_error"] = repr(e)[:200]

    if rank == 0:
        if args.full and not prefill and world == 1 and not args.no_extras:
            try:
                out["eager"] = bench_eager(layers, xs, device, max(3, args.steps // 4))
                if launches != len(flat_layers):
                    # the r1 headline for comparison: one launch per layer, same graph / timing protocol
                    g2, o2 = capture(flat_layers, xs, device)
                    for _ in range(3):
                        g2.replay()
                    _, ev2 = time_graph(g2, args.steps, device)
                    out["per_layer_launches"] = {"launches_per_step": len(flat_layers), "ms_per_step": round(1e3 * ev2 / args.steps, 4),
                                                 "GB_per_s": round(bytes_step * args.steps / ev2 / 1e9, 1), "tokens_per_s": round(M * args.steps / ev2, 1)}
                    del g2, o2
                    out["eager_per_layer"] = bench_eager(flat_layers, xs, device, max(3, args.steps // 4))
            except Exception as e:
                out["eager"] = {"error": repr(e)[:300]}
        if args.full and not prefill and world == 1 and not args.no_extras:
            try:
                out["mlp_call"] = bench_mlp_call(flat_layers, xs, device, args.steps)
            except Exception as e:
                out["mlp_call"] = {"error": repr(e)[:300]}
        if args.full and not prefill and world == 1 and not args.no_fused:
            try:
                del g, outs, layers, flat_layers
                torch.cuda.empty_cache()
                out["fused_callers"] = bench_fused(device, n_blocks, args.steps)
            except Exception as e:
                out["fused_callers"] = {"error": repr(e)[:300]}
        if args.full and not prefill and world == 1 and not args.no_extras:
            for name, fn in (("prefill", lambda: bench_prefill(device, max(3, args.steps // 4))),
                             ("mlp_prefill", lambda: bench_mlp_prefill(device, max(3, args.steps // 4))),
                             ("config5", lambda: bench_config5(device, args.steps)),
                             ("batched_decode", lambda: bench_batched(device, args.steps)),
                             ("warm_l3", lambda: bench_warm_l3(device, args.steps))):
                try:
                    torch.cuda.empty_cache()
                    out[name] = fn()
                except Exception as e:
                    out[name] = {"error": repr(e)[:300]}
        # The driver keeps `roofline` whole and drops unknown top-level keys: the second headline (prefill, MFMA-bound), BASELINE config 5 and
        # the batched-decode fractions are therefore repeated INSIDE it.
        if isinstance(roof, dict) and "error" not in roof:
            pf = out.get("prefill")
            if isinstance(pf, dict) and "roofline" in pf:
                r2 = dict(pf["roofline"])
                r2["layer_call_includes"] = "x permutation launch + GEMM (desc_act=True)"
                roof["prefill"] = r2
                roof["prefill_m4096_4096x4096"] = dict(bound="mfma", unit="TFLOP/s", peak=MFMA_PEAK_TFLOPS, achieved=pf["m4096_4096x4096"]["TFLOP_s"],
                                                       frac=pf["m4096_4096x4096"]["frac"], us_per_launch_events=pf["m4096_4096x4096"]["us_per_launch_events"])
                roof["prefill_stack_TFLOP_s"] = pf.get("TFLOP_s")
                if isinstance(pf.get("grouped"), dict) and "TFLOP_s" in pf["grouped"]:
                    roof["prefill_stack_grouped_TFLOP_s"] = pf["grouped"]["TFLOP_s"]        # q|k|v, gate|up via gptq_forward_multi: one permuted x per group
                if isinstance(pf.get("remainder_rounds"), dict):
                    roof["prefill_remainder_rounds"] = pf["remainder_rounds"]
            byc = {}
            c5 = out.get("config5")
            if isinstance(c5, dict):
                for k, v in c5.items():
                    if isinstance(v, dict) and "frac" in v:
                        byc["config5:" + k] = {"frac": v["frac"], "us": v["us"], "bound": "mfma" if "TFLOP_s" in v else "hbm"}
            bd = out.get("batched_decode")
            if isinstance(bd, dict):
                for k, v in bd.items():
                    if isinstance(v, dict) and "frac" in v:
                        byc["batched_decode:" + k] = {"frac": v["frac"], "us": v["us"], "bound": "hbm"}
                    elif isinstance(v, dict) and "mfma_frac" in v:
                        byc["batched_decode:" + k] = {"frac": v["mfma_frac"], "us": v["us"], "bound": "mfma"}
            mc = out.get("mlp_call")
            if isinstance(mc, dict):
                for k, v in mc.items():
                    if isinstance(v, dict) and "frac" in v:
                        byc["mlp_call:" + k] = {"frac": v["frac"], "us": v["us_per_mlp"], "bound": "hbm"}
            if byc:
                roof["by_config"] = byc
            # ... and once more as FLAT scalars: a parser that keeps only scalar members of `roofline` still records the second headline
            try:
                roof["stack_frac"] = round(out["value"] / HBM_PEAK_GBS, 4)
                if not prefill and roof.get("bound") == "hbm":
                    # the line's fraction is the WHOLE STACK's (every launch type, launch boundaries included: what a decoded token pays); the dominant
                    # launch type's own figures -- the ones rocprof's average duration of that kernel has to agree with -- stay beside it
                    roof["dominant_launch_frac"], roof["dominant_launch_achieved"] = roof["frac"], roof["achieved"]
                    roof["frac"], roof["achieved"] = roof["stack_frac"], round(out["value"], 1)
                    roof["frac_is"] = "stack (all launch types of a step / 8 TB/s); dominant_launch_* = the [gate|up] launch alone (us_per_launch_events)"

                roof["stack_GB_per_s"] = out["value"]
                for nm, v in (roof.get("us_per_launch_by_shape") or {}).items():
                    roof["us_" + nm.replace(":", "_")] = v
                if isinstance(pf, dict) and "roofline" in pf:
                    roof["prefill_frac"] = pf["roofline"]["frac"]
                    roof["prefill_us"] = pf["roofline"]["us_per_launch_events"]
                    roof["prefill_TFLOP_s"] = pf["roofline"]["achieved"]
                    roof["prefill_shape"] = pf["roofline"]["shape"]
                    roof["prefill_m4096_frac"] = pf["m4096_4096x4096"]["frac"]
                    roof["prefill_m4096_us"] = pf["m4096_4096x4096"]["us_per_launch_events"]
                    roof["prefill_m4096_TFLOP_s"] = pf["m4096_4096x4096"]["TFLOP_s"]
                    roof["prefill_kernel"] = pf["roofline"]["kernel"]
                    roof["m4096_frac"], roof["m4096_us"] = pf["m4096_4096x4096"]["frac"], pf["m4096_4096x4096"]["us_per_launch_events"]
                    roof["m4096_kernel"] = pf["m4096_4096x4096"].get("kernel")
                    tr = pf["roofline"].get("traffic")
                    roof["prefill_traffic"] = tr
                    if tr:
                        K_, N_ = [int(t[2:]) for t in pf["roofline"]["shape"].split()[:2]]
                        roof["prefill_traffic_ratio"] = round(tr / algorithmic_bytes(K_, N_, 2048, act_order=True), 3)
                    tr2 = pf["m4096_4096x4096"].get("traffic")
                    roof["m4096_traffic"] = tr2
                    if tr2:
                        roof["m4096_traffic_ratio"] = round(tr2 / algorithmic_bytes(4096, 4096, 4096), 3)
                    for nm, v in (pf.get("by_shape") or {}).items():
                        roof["prefill_us_" + nm] = v["us"]
                        roof["prefill_TFLOP_s_" + nm] = v["TFLOP_s"]
                if isinstance(c5, dict):
                    for bits in (3, 8):
                        fr = [v["frac"] for k, v in c5.items() if isinstance(v, dict) and k.startswith(f"int{bits}_g32_") and k.count("_") == 2 and "frac" in v]
                        if fr:
                            roof[f"cfg5_int{bits}_frac_min"], roof[f"cfg5_int{bits}_frac_max"] = min(fr), max(fr)
                        for k, v in c5.items():
                            if isinstance(v, dict) and k.startswith(f"int{bits}_g32_") and k.endswith("_prefill_M2048"):
                                roof[f"cfg5_int{bits}_prefill_frac"] = v["frac"]
                if isinstance(bd, dict):
                    for k, v in bd.items():
                        if isinstance(v, dict) and "us" in v:
                            roof["mid_" + k.lower() + "_us"] = v["us"]
                    if isinstance(bd.get("M64_4096x4096"), dict):
                        roof["m64_us_4096"] = bd["M64_4096x4096"].get("us")
                eg = out.get("eager")
                if isinstance(eg, dict):
                    for k in ("host_us_per_call", "us_per_call", "GB_per_s"):
                        if k in eg:
                            roof["eager_" + k] = eg[k]
                fc = out.get("fused_callers")
                if isinstance(fc, dict) and "ms_per_step" in fc:
                    roof["fused_ms_per_step"] = fc["ms_per_step"]
                    roof["fused_GB_per_s"] = fc.get("GB_per_s")
                if isinstance(mc, dict) and isinstance(mc.get("default_three_steps"), dict) and "us_per_mlp" in mc["default_three_steps"]:
                    roof["mlp_call_us"] = mc["default_three_steps"]["us_per_mlp"]
                    roof["mlp_call_frac"] = mc["default_three_steps"]["frac"]
                mp = out.get("mlp_prefill")
                if isinstance(mp, dict) and "us_per_mlp" in mp:      # desc_act MLP at 2048 rows through gptq_mlp_forward: down without a permute launch of its own
                    for k in ("us_per_mlp", "us_per_mlp_two_passes", "down_part_us", "down_part_us_two_passes"):
                        roof["mlp_prefill_" + k] = mp[k]
                wl = out.get("warm_l3")
                if isinstance(wl, dict) and "GB_per_s" in wl:      # the cache-warm number beside the cold headline
                    roof["warm_l3_GB_per_s"] = wl["GB_per_s"]
                    roof["warm_l3_us_per_launch_by_shape"] = wl["us_per_launch_by_shape"]
                bd2 = out.get("batched_decode")
                if isinstance(bd2, dict):
                    for k in ("short_prompt_M256_4096x4096", "M512_4096x4096", "M512_4096x11008", "M512_11008x4096", "M128_4096x11008", "M128_4096x4096"):
                        if isinstance(bd2.get(k), dict) and "us" in bd2[k]:
                            roof[k.lower() + "_us"] = bd2[k]["us"]
            except Exception as e:
                roof["flat_keys_error"] = repr(e)[:200]
        if args.full and not args.no_cpu_baseline and world == 1:      # rank 0 at N = 1 only (bounded sample, ~25 s of host time)
            out["cpu_baseline"] = cpu_baseline(1 if not prefill else 16, act_order, device=device)
        print(json.dumps(out))
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
