"""2- and 3-bit routed experts at 5..64 tokens: the batch path (QuantMoEExperts.low_bit_batch = True: gptq_moe_batch_forward, moe_rows_lowbit_kernel on
the decode copy) against the grouped low-bit path (post_init(low_bit=True): gptq_moe_forward on the checkpoint rows), with the unchanged 4-bit batch path
as a reference row -- and the two A/Bs against the parent library: the 4-bit batch path (its kernels must be what they were) and the act-order row
permutes whose SLOT template argument became a launch argument to pay for the new kernels.  After tools/moe_lowbit_decode_bench.py, same protocol:
ONE checkout per process (--tree): run it once per tree, alternating the trees, and read the lines side by side (profiles/moe_lowbit_batch_ab.log).

  --what feature   blocks Mixtral-8x7B (E 8, topk 2, H 4096, I 14336) and Qwen1.5-MoE-A2.7B (E 60, topk 4, H 2048, I 1408), g128 fp16, 3 and 2 bits,
                   T = 5, 8, 16, 32, 64.  Per (block, bits, T) the SAME expert sets run every path the tree has: "grouped" (low_bit=True, the batch band
                   closed through low_bit_batch_max_tokens = 0) and "batch"; the paths alternate sample by sample.  "batch4": 4-bit experts of the same
                   shape on the batch path (post_init(batch=True)), with the checksum of their outputs (equal across trees: same kernels).  A tree
                   without low_bit_batch (the parent) reports "grouped" and "batch4".
  --what permute   gptq_permute_columns (the pre-pass of an act-order dense layer, natural order) on 16 and 2048 rows of K = 4096 and 2048 rows of
                   K = 11008, and one act-order 4096 -> 4096 4-bit g128 QuantLinear forward at 16 and 2048 rows (whatever order its plan asks of the
                   pre-pass); checksums of the outputs (equal across trees: bit-identical values).

ROTATING WEIGHTS: --sets expert sets (weights and routing of their own) run back to back in one captured graph, so that a replay streams more than the
256 MB Infinity Cache holds; times are per layer (graph time / sets).  Per sample one pair of device events around --reps replays; median [p10 .. p90] of
--samples samples after 5 warm-up samples.

    python tools/moe_lowbit_batch_bench.py --what feature --tree /path/to/checkout --label parent [--out profiles/moe_lowbit_batch_ab.log]
"""
import argparse
import os
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--label", default="this tree")
ap.add_argument("--what", choices=("feature", "permute"), default="feature")
ap.add_argument("--blocks", default="mixtral,a2.7b")
ap.add_argument("--bits", default="3,2,4")
ap.add_argument("--tokens", default="5,8,16,32,64")
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
assert torch.cuda.is_available(), "moe_lowbit_batch_bench.py needs the GPU"
DEV = "cuda:0"
SHAPES = {"a2.7b": (60, 4, 2048, 1408, 16), "mixtral": (8, 2, 4096, 14336, 3)}      # (E, topk, H, I, sets): > 256 MB of packed experts at 2 bits
HAS_BATCH = hasattr(_lib, "MOE_LOW_BIT_BATCH")
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
        return q.post_init(batch=True)
    q.low_bit_batch = True          # (an attribute the parent does not read)
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
                paths = ["batch4"] if bits == 4 else (["grouped", "batch"] if HAS_BATCH else ["grouped"])
                for p in paths:
                    if HAS_BATCH and bits != 4:
                        for q in sets:
                            q.low_bit_batch_max_tokens = 0 if p == "grouped" else 64
                    graphs[p], outs[p] = capture(run)
                    assert sets[0].last_plan["path"] == ("grouped" if p == "grouped" else "batch"), (p, sets[0].last_plan)
                res = measure(graphs, len(sets))
                for p in paths:
                    chk = float(sum(o.float().abs().sum() for o in outs[p]))
                    m, lo, hi = res[p]
                    emit(f"{args.label:>10} {name:>8} int{bits} T={T:<2} {p:>8}: {m:8.2f} us per layer [{lo:8.2f} .. {hi:8.2f}]  checksum {chk:.6e}")
                if len(paths) == 2:
                    emit(f"{args.label:>10} {name:>8} int{bits} T={T:<2} grouped / batch = {res['grouped'][0] / res['batch'][0]:.2f}")
                del graphs, outs
            del sets
            torch.cuda.empty_cache()


def permute():
    lib = _lib.load()
    gen = torch.Generator(device=DEV).manual_seed(0)
    graphs, outs, keep = {}, {}, []          # keep: the graphs hold raw pointers, so every operand stays referenced until the last replay
    for M, K in ((16, 4096), (2048, 4096), (2048, 11008)):
        x = (torch.rand((M, K), generator=gen, device=DEV) - 0.5).half()
        perm = torch.randperm(K, generator=gen, device=DEV).to(torch.int32)
        out = torch.empty_like(x)
        keep.append((x, perm, out))

        def run(x=x, perm=perm, out=out, M=M, K=K):
            _lib.check(lib.gptq_permute_columns(x.data_ptr(), perm.data_ptr(), M, K, _lib.GPTQ_F16, out.data_ptr(), torch.cuda.current_stream().cuda_stream))
            return out

        graphs[f"permute_columns {M}x{K}"], outs[f"permute_columns {M}x{K}"] = capture(run)
    lin = QuantLinear(4, 128, 4096, 4096, False, weight_dtype=torch.float16).to(DEV)
    fill(lin, gen, act=True)
    lin.post_init()
    for M in (16, 2048):
        x = (torch.rand((M, 4096), generator=gen, device=DEV) - 0.5).half()
        keep.append(x)
        graphs[f"act-order layer {M} rows"], outs[f"act-order layer {M} rows"] = capture(lambda x=x: lin(x))
    res = measure(graphs, 1)
    for k, (m, lo, hi) in res.items():
        emit(f"{args.label:>10} {k:>28}: {m:8.2f} us [{lo:8.2f} .. {hi:8.2f}]  checksum {float(outs[k].float().abs().sum()):.6e}")


feature() if args.what == "feature" else permute()
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write("\n".join(lines) + "\n")
