"""2- and 3-bit routed experts at 65 tokens and more: the prefill path (QuantMoEExperts.low_bit_prefill = True: gptq_moe_prefill_forward,
moe_panel_lowbit_kernel on the decode copy) against the grouped low-bit path (post_init(low_bit=True): gptq_moe_forward on the checkpoint rows), with the
unchanged 4-bit prefill path as a reference row -- and the A/Bs against the parent library: the 4-bit prefill path (its kernels must be what they were)
and the two kernels whose template parameter became a launch argument to pay for the new ones (gemm_reduce_kernel's dtype, gemm_f32_kernel's BITS).
After tools/moe_lowbit_batch_bench.py, same protocol: ONE checkout per process (--tree): run it once per tree, alternating the trees, and read the lines
side by side (profiles/moe_lowbit_prefill_ab.log).

  --what feature   blocks Mixtral-8x7B (E 8, topk 2, H 4096, I 14336) and Qwen1.5-MoE-A2.7B (E 60, topk 4, H 2048, I 1408), g128 fp16, 3 and 2 bits,
                   T = 65, 128, 256, 512, 2048.  Per (block, bits, T) the SAME expert sets run every path the tree has: "grouped" (low_bit=True, the
                   prompt band closed through low_bit_prefill_min_tokens) and "prefill"; the paths alternate sample by sample.  "prefill4": 4-bit experts
                   of the same shape on the prefill path (post_init(prefill=True)), with the checksum of their outputs (equal across trees: same
                   kernels).  A tree without low_bit_prefill (the parent) reports "grouped" and "prefill4".
  --what folds     4-bit g128 fp16 and bf16 QuantLinears WITHOUT a decode copy (post_init(tiled=False)) at 16, 48 and 128 rows -- the K-split strip16 /
                   skinny / tiled GEMMs, each followed by gemm_reduce_kernel -- on 4096 -> 4096 and 4096 -> 11008, and fp32 layers of 4 and 3 bits at
                   256 rows on the matrix-core fp32 GEMM (gemm_f32_kernel); checksums of the outputs (equal across trees: bit-identical values).

ROTATING WEIGHTS: --sets expert sets (weights and routing of their own) run back to back in one captured graph, so that a replay streams more than the
256 MB Infinity Cache holds; times are per layer (graph time / sets).  Per sample one pair of device events around --reps replays; median [p10 .. p90] of
--samples samples after 5 warm-up samples.

    python tools/moe_lowbit_prefill_bench.py --what feature --tree /path/to/checkout --label parent [--out profiles/moe_lowbit_prefill_ab.log]
"""
import argparse
import os
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--label", default="this tree")
ap.add_argument("--what", choices=("feature", "folds"), default="feature")
ap.add_argument("--blocks", default="mixtral,a2.7b")
ap.add_argument("--bits", default="3,2,4")
ap.add_argument("--tokens", default="65,128,256,512,2048")
ap.add_argument("--samples", type=int, default=20)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--out", default=None)
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.tree))

import torch  # noqa: E402

import autogptq_amd  # noqa: E402
from autogptq_amd import _lib  # noqa: E402
from autogptq_amd.moe import QuantMoEExperts, moe_forward  # noqa: E402
from autogptq_amd.qlinear_mi355x import QuantLinear  # noqa: E402

assert os.path.abspath(autogptq_amd.__file__).startswith(os.path.abspath(args.tree)), autogptq_amd.__file__
assert torch.cuda.is_available(), "moe_lowbit_prefill_bench.py needs the GPU"
DEV = "cuda:0"
SHAPES = {"a2.7b": (60, 4, 2048, 1408, 16), "mixtral": (8, 2, 4096, 14336, 3)}      # (E, topk, H, I, sets): > 256 MB of packed experts at 2 bits
HAS_PREFILL = hasattr(_lib, "MOE_LOW_BIT_PREFILL")
CLOSED = 1 << 30                                    # low_bit_prefill_min_tokens that no call reaches
lines = []


def emit(s):
    lines.append(s)
    print(s, flush=True)


def fill(lin, gen, act=False):
    """Random packed tensors made ON the device (gen: a device generator; the same seed gives the same layer in every tree)."""
    lin.qweight = torch.randint(-2 ** 31, 2 ** 31 - 1, lin.qweight.shape, generator=gen, dtype=torch.int64, device=DEV).to(torch.int32)
    lin.qzeros = torch.randint(-2 ** 31, 2 ** 31 - 1, lin.qzeros.shape, generator=gen, dtype=torch.int64, device=DEV).to(torch.int32)
    lin.scales = (torch.rand(lin.scales.shape, generator=gen, device=DEV) * 0.004 + 0.001).to(lin.scales.dtype)
    gi = torch.arange(lin.infeatures, dtype=torch.int32, device=DEV) // lin.group_size
    lin.g_idx = gi[torch.randperm(lin.infeatures, generator=gen, device=DEV)].contiguous() if act else gi


def experts(E, H, I, topk, bits, seed):
    gen = torch.Generator(device=DEV).manual_seed(seed)
    with torch.device("meta"):
        q = QuantMoEExperts(E, H, I, bits, 128, top_k=topk, weight_dtype=torch.float16)
    q = q.to_empty(device=DEV)
    for e in range(E):
        for l in q[e].layers():
            fill(l, gen)
    if bits in (4, 8):
        return q.post_init(prefill=True)
    q.low_bit_prefill = True        # (an attribute the parent does not read)
    return q.post_init(low_bit=True)


def capture(fn):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.no_grad(), torch.cuda.stream(side):
        for _ in range(2):
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
        for bits in [int(b) for b in args.bits.split(",")]:
            sets = [experts(E, H, I, topk, bits, 10 + i) for i in range(nsets)]
            for T in [int(t) for t in args.tokens.split(",")]:
                x = (torch.rand((T, H), generator=torch.Generator().manual_seed(T)) - 0.5).half().to(DEV)
                g0 = torch.Generator().manual_seed(T)
                routes = []
                for _ in sets:
                    idx = torch.stack([torch.randperm(E, generator=g0)[:topk] for _ in range(T)]).to(DEV)
                    routes.append((idx, torch.full((T, topk), 1.0 / topk, device=DEV)))

                def run():
                    return [moe_forward(q, x, i, w) for q, (i, w) in zip(sets, routes)]

                graphs, outs = {}, {}
                paths = ["prefill4"] if bits == 4 else (["grouped", "prefill"] if HAS_PREFILL else ["grouped"])
                for p in paths:
                    if HAS_PREFILL and bits != 4:
                        for q in sets:
                            q.low_bit_prefill_min_tokens = CLOSED if p == "grouped" else 65
                    graphs[p], outs[p] = capture(run)
                    assert sets[0].last_plan["path"] == ("grouped" if p == "grouped" else "prefill"), (p, sets[0].last_plan)
                res = measure(graphs, len(sets))
                for p in paths:
                    chk = float(sum(o.float().abs().sum() for o in outs[p]))
                    m, lo, hi = res[p]
                    emit(f"{args.label:>10} {name:>8} int{bits} T={T:<4} {p:>8}: {m:9.2f} us per layer [{lo:9.2f} .. {hi:9.2f}]  checksum {chk:.6e}")
                if len(paths) == 2:
                    emit(f"{args.label:>10} {name:>8} int{bits} T={T:<4} grouped / prefill = {res['grouped'][0] / res['prefill'][0]:.2f}")
                del graphs, outs
            del sets
            torch.cuda.empty_cache()


def folds():
    gen = torch.Generator(device=DEV).manual_seed(0)
    graphs, outs, keep = {}, {}, []          # keep: the graphs hold raw pointers, so every operand stays referenced until the last replay
    for dtype in (torch.float16, torch.bfloat16):
        for K, N in ((2048, 512), (4096, 1024), (4096, 11008)):
            lin = QuantLinear(4, 128, K, N, True, weight_dtype=dtype).to(DEV)
            fill(lin, gen)
            lin.bias = (torch.rand(N, generator=gen, device=DEV) - 0.5).to(dtype)
            lin.post_init(tiled=False)       # checkpoint rows only: the K-split GEMMs and their reduction kernel
            for M in (16, 48, 128):
                d = _lib.describe_plan(lin._layer, M)
                if d["ksplit"] <= 1 or not d["kernel"].startswith(("strip16", "skinny", "tiled")):
                    continue                 # (the plan's own choice is a kernel that sums its K slices itself: no reduction launch)
                x = (torch.rand((M, K), generator=gen, device=DEV) - 0.5).to(dtype)
                keep.append((lin, x))
                k = f"{str(dtype)[6:]} {K}x{N} M={M} {d['kernel']} ksplit={d['ksplit']}"
                graphs[k], outs[k] = capture(lambda lin=lin, x=x: lin(x))
    for bits in (4, 3):
        lin = QuantLinear(bits, 128, 4096, 4096, False, weight_dtype=torch.float32).to(DEV)
        fill(lin, gen)
        lin.post_init()
        d = _lib.describe_plan(lin._layer, 256)
        assert d["kernel"] == "f32_mfma", d      # the matrix-core fp32 GEMM is the plan's own choice at this size
        x = torch.rand((256, 4096), generator=gen, device=DEV) - 0.5
        keep.append((lin, x))
        k = f"float32 4096x4096 int{bits} M=256 f32_mfma"
        graphs[k], outs[k] = capture(lambda lin=lin, x=x: lin(x))
    res = measure(graphs, 1)
    for k, (m, lo, hi) in res.items():
        emit(f"{args.label:>10} {k:>52}: {m:8.2f} us [{lo:8.2f} .. {hi:8.2f}]  checksum {float(outs[k].float().abs().sum()):.6e}")


feature() if args.what == "feature" else folds()
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write("\n".join(lines) + "\n")
