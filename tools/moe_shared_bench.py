"""A Qwen-MoE block behind inject_shared_expert (router + moe_shared_forward) against the composition it replaces, A/B in ONE process on the GPU.

  (A) composition   fused router (moe_route), the routed experts through moe_forward on their decode copy (decode kernels up to 4 tokens, batch kernels up
                    to 64, prefill kernels above), the shared MLP through mlp_forward, then torch linear / sigmoid / mul / add
  (B) fused         fused router, then moe_shared_forward with the fused call allowed up to 4 tokens: ONE gptq_moe_shared_decode_forward call (T <= 4 only)
  (C) combine       fused router, then moe_shared_forward with the fused call switched off: the experts and the shared MLP as in (A) and ONE
                    gptq_moe_shared_combine launch for the tail (what the injected block runs above 4 tokens, and where (B) is not the faster one)

Shape: the block of Qwen1.5-MoE-A2.7B (H 2048, E 60, topk 4, I 1408, I_s 5632), 4-bit g128 fp16, T = 1, 2, 3, 4, 16, 128.
ROTATING WEIGHTS: --blocks independent blocks (weights, router and gate vector of their own) run back to back in one captured graph per variant, so that a
replay streams more weight bytes than the 256 MB Infinity Cache holds (T = 1 touches about 35 MB per block: 16 blocks are 560 MB) and a block does not find its own weights there from the previous replay; reported times
are per block (graph time / blocks).  Per sample ONE pair of device events around --reps replays of one graph; the variants alternate sample by sample;
median [p10 .. p90] in microseconds and the ratios of the medians (A / B, A / C: above 1 the injected block is faster).  Launches per block: the device kernels
torch.profiler records for one eager call of one block.  Both variants are checked against each other before they are timed.

    python tools/moe_shared_bench.py [--samples 30] [--reps 5] [--blocks 16] [--out profiles/moe_shared_ab.log]
"""
import argparse
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from autogptq_amd.moe import QuantMoEExperts, moe_forward, moe_route, moe_shared_forward  # noqa: E402
from autogptq_amd.qlinear_mi355x import QuantLinear, mlp_forward  # noqa: E402

E, TOPK, H, I, IS, BITS, GS = 60, 4, 2048, 1408, 5632, 4, 128
TS = (1, 2, 3, 4, 16, 128)
DEV = "cuda:0"
DTYPE = torch.float16


def _fill(lin, gen):
    lin.qweight = torch.randint(-2 ** 31, 2 ** 31 - 1, lin.qweight.shape, generator=gen, dtype=torch.int64).to(torch.int32)
    lin.qzeros = torch.randint(-2 ** 31, 2 ** 31 - 1, lin.qzeros.shape, generator=gen, dtype=torch.int64).to(torch.int32)
    lin.scales = (torch.rand(lin.scales.shape, generator=gen) * 0.004 + 0.001).to(lin.scales.dtype)
    lin.g_idx = torch.arange(lin.infeatures, dtype=torch.int32) // lin.group_size


class Block:
    def __init__(self, seed):
        gen = torch.Generator().manual_seed(seed)
        q = QuantMoEExperts(E, H, I, BITS, GS, top_k=TOPK, weight_dtype=DTYPE)
        for e in range(E):
            for l in q[e].layers():
                _fill(l, gen)
        self.experts = q.to(DEV).post_init(decode_copy=True, batch=True, prefill=True)
        layers = []
        for k, n in ((H, IS), (H, IS), (IS, H)):
            l = QuantLinear(BITS, GS, k, n, False, weight_dtype=DTYPE)
            _fill(l, gen)
            l = l.to(DEV)
            l.post_init()
            layers.append(l)
        self.shared = tuple(layers)
        self.router_w = (torch.randn((E, H), generator=gen) * 0.05).to(DTYPE).to(DEV)
        self.gate_w = (torch.randn((1, H), generator=gen) * 0.05).to(DTYPE).to(DEV)

    def composition(self, x):
        _, w, idx = moe_route(x, self.router_w, TOPK, renorm=True, return_logits=True)
        routed = moe_forward(self.experts, x, idx, w)
        shared = mlp_forward(*self.shared, x)
        return routed + torch.sigmoid(F.linear(x, self.gate_w)) * shared

    def injected(self, x, fused_max):
        self.experts.shared_decode_max_tokens = fused_max
        _, w, idx = moe_route(x, self.router_w, TOPK, renorm=True, return_logits=True)
        return moe_shared_forward(self.experts, self.shared, self.gate_w, x, idx, w)


def capture(fn):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.no_grad(), torch.cuda.stream(side):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.no_grad(), torch.cuda.graph(g):
        out = fn()
    return g, out


def sample(g, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        g.replay()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / reps


def pct(v, p):
    v = sorted(v)
    return v[min(len(v) - 1, int(p * len(v)))]


def launches(fn):
    """Device kernels of one eager call, as torch.profiler records them."""
    from torch.profiler import ProfilerActivity, profile
    with torch.no_grad():
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
    return sum(1 for ev in prof.events() if str(ev.device_type).endswith("CUDA") and "memcpy" not in ev.name.lower() and "memset" not in ev.name.lower())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=30)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--blocks", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "moe_shared_ab.log"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "moe_shared_bench.py needs the GPU"
    blocks = [Block(100 + i) for i in range(args.blocks)]
    lines = [f"# Qwen1.5-MoE-A2.7B block (H {H}, E {E}, topk {TOPK}, I {I}, I_s {IS}), {BITS}-bit g{GS} fp16; {args.blocks} blocks with weights of their own per "
             f"graph (rotating weights), {args.samples} samples x {args.reps} replays per variant and T, the variants alternating; us per block: median [p10 .. p90]",
             "# (A) fused router + moe_forward (decode copy: decode / batch / prefill kernels) + mlp_forward + torch linear / sigmoid / mul / add",
             "# (B) fused router + ONE gptq_moe_shared_decode_forward (T <= 4)",
             "# (C) fused router + (A)'s experts and MLP + ONE gptq_moe_shared_combine",
             f"# {'T':>4} {'A us':>24} {'B us':>24} {'C us':>24} {'A/B':>6} {'A/C':>6} {'launches A B C':>14} {'max |A-B| |A-C|':>18}"]
    for T in TS:
        x = ((torch.rand((T, H), generator=torch.Generator().manual_seed(T)) - 0.5)).to(DTYPE).to(DEV)
        variants = {"A": lambda b: b.composition(x), "C": lambda b: b.injected(x, 0)}
        if T <= 4:
            variants["B"] = lambda b: b.injected(x, 4)
        graphs, outs, times, counts = {}, {}, {}, {}
        for k, fn in variants.items():
            graphs[k], outs[k] = capture(lambda fn=fn: [fn(b) for b in blocks])
            graphs[k].replay()
            torch.cuda.synchronize()
            want = {"A": None, "B": "decode", "C": "combine"}[k]
            assert want is None or blocks[0].experts.last_plan.get("shared") == want, (k, blocks[0].experts.last_plan)
            times[k] = []
        scale = max(float(a.float().abs().max()) for a in outs["A"])
        diff = {k: max(float((a.float() - b.float()).abs().max()) for a, b in zip(outs["A"], outs[k])) for k in variants if k != "A"}
        assert all(d <= 2e-2 * max(1.0, scale) for d in diff.values()), (T, diff, scale)
        for _ in range(5):
            for k in variants:
                sample(graphs[k], args.reps)
        for _ in range(args.samples):
            for k in variants:
                times[k].append(sample(graphs[k], args.reps) / args.blocks)
        for k, fn in variants.items():
            counts[k] = launches(lambda fn=fn: fn(blocks[0]))
        med = {k: pct(v, 0.5) for k, v in times.items()}
        cell = lambda k: f"{med[k]:>8.2f} [{pct(times[k], 0.1):>6.2f} .. {pct(times[k], 0.9):>6.2f}]" if k in med else f"{'-':>24}"      # noqa: E731
        ratio = lambda k: f"{med['A'] / med[k]:>6.3f}" if k in med else f"{'-':>6}"      # noqa: E731
        lines.append(f"  {T:>4} {cell('A')} {cell('B')} {cell('C')} {ratio('B')} {ratio('C')} "
                     f"{' '.join(str(counts.get(k, '-')) for k in 'ABC'):>14} {' '.join(f'{diff[k]:.2e}' if k in diff else '-' for k in 'BC'):>18}")
        print(lines[-1], flush=True)
        del graphs, outs
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
