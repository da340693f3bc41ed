"""2- and 3-bit routed experts at 1..4 tokens: the decode path (post_init(low_bit_decode=True): gptq_moe_decode_forward, two launches of the 2- / 3-bit
forms of moe_shared_kernel on the decode copy) against the grouped low-bit path (post_init(low_bit=True): gptq_moe_forward, four launches on the checkpoint
rows) and against 4-bit decode of the same shape -- and the A/B that shows the existing forms of moe_shared_kernel unharmed by the forms it gained.
ONE checkout per process (--tree): run it once per tree, alternating the trees, and read the lines side by side (profiles/moe_lowbit_decode_ab.log).

  --what feature   blocks Mixtral-8x7B (E 8, topk 2, H 4096, I 14336) and Qwen1.5-MoE-A2.7B (E 60, topk 4, H 2048, I 1408), g128 fp16, 3 and 2 bits,
                   T = 1..4.  Per (block, bits, T) the SAME expert sets run every path the tree has: "grouped" (low_bit=True, decode switched off through
                   low_bit_decode_max_tokens = 0 where the tree has the decode path) and "decode"; the paths alternate sample by sample.  "decode4":
                   4-bit experts of the same shape on the decode path.  A tree without low_bit_decode (the parent) reports "grouped" alone.
  --what shared    the A2.7B block with its shared expert (I_s 5632), 4-bit g128 fp16, through moe_shared_forward: the fused call at T = 1, 2
                   (moe_shared_kernel forms 0..7) and the combine form at T = 16 (form 8); checksums of the outputs (equal across trees: same values).

ROTATING WEIGHTS: --sets expert sets (weights and routing of their own) run back to back in one captured graph, so that a replay streams more than the
256 MB Infinity Cache holds (A2.7B at 2 bits touches 8.6 MB per layer and token: 32 sets; Mixtral at 2 bits 88 MB: 4 sets); times are per layer
(graph time / sets).  Per sample one pair of device events around --reps replays; median [p10 .. p90] of --samples samples after 5 warm-up samples.

    python tools/moe_lowbit_decode_bench.py --what feature --tree /path/to/checkout --label parent [--out profiles/moe_lowbit_decode_ab.log]
"""
import argparse
import inspect
import os
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--label", default="this tree")
ap.add_argument("--what", choices=("feature", "shared"), default="feature")
ap.add_argument("--blocks", default="mixtral,a2.7b")
ap.add_argument("--bits", default="3,2")
ap.add_argument("--samples", type=int, default=30)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--out", default=None)
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.tree))

import torch  # noqa: E402

import autogptq_amd  # noqa: E402
from autogptq_amd.moe import QuantMoEExperts, moe_forward, moe_shared_forward  # noqa: E402
from autogptq_amd.qlinear_mi355x import QuantLinear  # noqa: E402

assert os.path.abspath(autogptq_amd.__file__).startswith(os.path.abspath(args.tree)), autogptq_amd.__file__
assert torch.cuda.is_available(), "moe_lowbit_decode_bench.py needs the GPU"
DEV = "cuda:0"
SHAPES = {"a2.7b": (60, 4, 2048, 1408, 32), "mixtral": (8, 2, 4096, 14336, 4)}
HAS_DECODE = "low_bit_decode" in inspect.signature(QuantMoEExperts.post_init).parameters
lines = []


def emit(s):
    lines.append(s)
    print(s, flush=True)


def fill(lin, gen):
    lin.qweight = torch.randint(-2 ** 31, 2 ** 31 - 1, lin.qweight.shape, generator=gen, dtype=torch.int64).to(torch.int32)
    lin.qzeros = torch.randint(-2 ** 31, 2 ** 31 - 1, lin.qzeros.shape, generator=gen, dtype=torch.int64).to(torch.int32)
    lin.scales = (torch.rand(lin.scales.shape, generator=gen) * 0.004 + 0.001).to(lin.scales.dtype)
    lin.g_idx = torch.arange(lin.infeatures, dtype=torch.int32) // lin.group_size


def experts(E, H, I, topk, bits, seed):
    gen = torch.Generator().manual_seed(seed)
    q = QuantMoEExperts(E, H, I, bits, 128, top_k=topk, weight_dtype=torch.float16)
    for e in range(E):
        for l in q[e].layers():
            fill(l, gen)
    q = q.to(DEV)
    if bits in (4, 8):
        return q.post_init(decode_copy=True)
    return q.post_init(low_bit=True, low_bit_decode=True) if HAS_DECODE else q.post_init(low_bit=True)


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


def sample(g):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(args.reps):
        g.replay()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / args.reps


def measure(graphs, per):
    """{name: graph} -> {name: (median, p10, p90)} in us / per, the graphs alternating sample by sample."""
    ts = {k: [] for k in graphs}
    for s in range(args.samples + 5):
        for k, g in graphs.items():
            t = sample(g)
            if s >= 5:
                ts[k].append(t / per)
    out = {}
    for k, v in ts.items():
        v.sort()
        out[k] = (v[len(v) // 2], v[len(v) // 10], v[len(v) * 9 // 10])
    return out


def feature():
    for name in args.blocks.split(","):
        E, topk, H, I, nsets = SHAPES[name]
        for bits in [int(b) for b in args.bits.split(",")] + ([4] if HAS_DECODE else []):
            sets = [experts(E, H, I, topk, bits, 10 + i) for i in range(nsets)]
            for T in (1, 2, 3, 4):
                x = (torch.rand((T, H), generator=torch.Generator().manual_seed(T)) - 0.5).half().to(DEV)
                g0 = torch.Generator().manual_seed(T)
                routes = []
                for _ in sets:
                    idx = torch.stack([torch.randperm(E, generator=g0)[:topk] for _ in range(T)]).to(DEV)
                    routes.append((idx, torch.full((T, topk), 1.0 / topk, device=DEV)))

                def run():
                    return [moe_forward(q, x, i, w) for q, (i, w) in zip(sets, routes)]

                graphs, outs = {}, {}
                paths = ["decode4"] if bits == 4 else (["grouped", "decode"] if HAS_DECODE else ["grouped"])
                for p in paths:
                    if HAS_DECODE and bits != 4:
                        for q in sets:
                            q.low_bit_decode_max_tokens = 0 if p == "grouped" else 4
                    graphs[p], outs[p] = capture(run)
                    assert sets[0].last_plan["path"] == ("grouped" if p == "grouped" else "decode"), (p, sets[0].last_plan)
                res = measure(graphs, len(sets))
                for p in paths:
                    chk = float(sum(o.float().abs().sum() for o in outs[p]))
                    m, lo, hi = res[p]
                    emit(f"{args.label:>10} {name:>8} int{bits} T={T} {p:>8}: {m:8.2f} us per layer [{lo:8.2f} .. {hi:8.2f}]  checksum {chk:.6e}")
                if len(paths) == 2:
                    emit(f"{args.label:>10} {name:>8} int{bits} T={T} grouped / decode = {res['grouped'][0] / res['decode'][0]:.2f}")
                del graphs, outs
            del sets
            torch.cuda.empty_cache()


def shared():
    E, topk, H, I, Is, nblocks = 60, 4, 2048, 1408, 5632, 16
    blocks = []
    for i in range(nblocks):
        gen = torch.Generator().manual_seed(100 + i)
        q = experts(E, H, I, topk, 4, 100 + i)
        layers = []
        for k, n in ((H, Is), (H, Is), (Is, H)):
            l = QuantLinear(4, 128, k, n, False, weight_dtype=torch.float16)
            fill(l, gen)
            l = l.to(DEV)
            l.post_init()
            layers.append(l)
        gw = (torch.randn((1, H), generator=gen) * 0.05).half().to(DEV)
        blocks.append((q, tuple(layers), gw))
    for T, want in ((1, "decode"), (2, "decode"), (16, "combine")):
        x = (torch.rand((T, H), generator=torch.Generator().manual_seed(T)) - 0.5).half().to(DEV)
        g0 = torch.Generator().manual_seed(T)
        routes = []
        for _ in blocks:
            idx = torch.stack([torch.randperm(E, generator=g0)[:topk] for _ in range(T)]).to(DEV)
            routes.append((idx, torch.full((T, topk), 1.0 / topk, device=DEV)))

        def run():
            return [moe_shared_forward(q, ls, gw, x, i, w) for (q, ls, gw), (i, w) in zip(blocks, routes)]

        g, out = capture(run)
        assert blocks[0][0].last_plan["shared"] == want, blocks[0][0].last_plan
        m, lo, hi = measure({"s": g}, len(blocks))["s"]
        chk = float(sum(o.float().abs().sum() for o in out))
        emit(f"{args.label:>10} a2.7b+shared int4 T={T} {want:>8}: {m:8.2f} us per block [{lo:8.2f} .. {hi:8.2f}]  checksum {chk:.6e}")
        del g, out


feature() if args.what == "feature" else shared()
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write("\n".join(lines) + "\n")
