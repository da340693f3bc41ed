"""A/B of the ungated epilogues (RELU / GELU / GELU_TANH): one process per line block, appended to --log as JSON lines.

  --part gated     what the change may cost: the SiLU pair layer 4096 -> 2x11008 at 1 and 4 rows and Gemma-2-9B's MLP call (mlp_forward(act='gelu_tanh')).  Run it
                   alternately with GPTQ_MI355X_LIB pointing at a build of the parent commit and at this commit's library (--tag parent_run1, new_run1, ...).
  --part feature   what the change buys (this commit's library): fc1 + act as ONE launch against the composition (the plain layer call + the torch activation
                   on its output), and the whole MLP fc1 + act, fc2 in two launches against three, at 1 / 2 / 4 rows of the OPT-6.7B, Falcon-7B, GPT-NeoX-20B
                   and Phi-2 shapes (fp16, 4-bit).

Every figure: captured graphs over ROTATING copies of the layers (together larger than the 256 MiB Infinity Cache: the weights come from HBM), 7 timed windows
of ~300 calls each between HIP events after 0.3 s of untimed replays; the two sides of a comparison alternate window by window."""
import argparse
import json
import os
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from autogptq_amd import _lib                                             # noqa: E402
from autogptq_amd.qlinear_mi355x import QuantLinear, mlp_forward          # noqa: E402
from oracle import gptq_oracle as O                                       # noqa: E402

DEV = "cuda:0"
ACT_FN = {"relu": F.relu, "gelu": F.gelu, "gelu_tanh": lambda y: F.gelu(y, approximate="tanh")}


def copies(K, N, gs, bias, n, epilogue="none", seed=0):
    """n modules holding clones of ONE random layer (distinct device memory), initialised."""
    L = O.random_quant_layer(K, N, 4, gs, seed=seed, bias=bias)
    out = []
    for _ in range(n):
        q = QuantLinear(4, gs, K, N, bias, epilogue=epilogue)
        q.qweight, q.qzeros, q.scales, q.g_idx = L["qweight"].clone(), L["qzeros"].clone(), L["scales"].clone(), L["g_idx"].clone()
        if bias:
            q.bias = L["bias"].clone()
        q = q.to(DEV)
        q.post_init()
        out.append(q)
    return out


def capture(calls):
    """One graph that runs every callable of `calls` once."""
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s), torch.no_grad():
        for _ in range(2):
            for c in calls:
                c()
        s.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            for c in calls:
                c()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    return g


def timed(graphs, per_replay, windows=7, calls=300):
    """us per call of each graph of `graphs`, their windows alternating."""
    reps = max(1, calls // per_replay)
    t0 = time.time()
    while time.time() - t0 < 0.3:
        for g in graphs:
            g.replay()
    torch.cuda.synchronize()
    res = [[] for _ in graphs]
    for _ in range(windows):
        for i, g in enumerate(graphs):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(reps):
                g.replay()
            b.record()
            torch.cuda.synchronize()
            res[i].append(round(a.elapsed_time(b) * 1e3 / (reps * per_replay), 3))
    return res


def part_gated(tag, emit):
    n = 8
    layers = copies(4096, 2 * 11008, 128, False, n, epilogue="silu_mul")
    for M in (1, 4):
        x = (torch.rand(M, 4096) - 0.5).half().to(DEV)
        assert _lib.describe_plan(layers[0]._layer, M)["epilogue"] == "fused"
        (us,) = timed([capture([lambda q=q: q(x) for q in layers])], n)
        emit({"what": "silu pair layer 4096->2x11008 int4 g128 fp16", "tag": tag, "M": M, "us_per_call": us})
    del layers
    n = 6
    H, I = 3584, 14336
    gate, up, down = copies(H, I, 128, False, n, seed=1), copies(H, I, 128, False, n, seed=2), copies(I, H, 128, False, n, seed=3)
    for M in (1, 4):
        x = (torch.rand(M, H) - 0.5).half().to(DEV)
        (us,) = timed([capture([lambda i=i: mlp_forward(gate[i], up[i], down[i], x, act="gelu_tanh") for i in range(n)])], n)
        emit({"what": "Gemma-2-9B MLP call 3584/14336 int4 g128 fp16 (mlp_forward act=gelu_tanh)", "tag": tag, "M": M, "us_per_call": us})


MODELS = [("OPT-6.7B", 4096, 16384, 128, True, "relu"), ("Falcon-7B", 4544, 18176, 64, False, "gelu"),
          ("GPT-NeoX-20B", 6144, 24576, 128, False, "gelu"), ("Phi-2", 2560, 10240, 128, True, "gelu_tanh")]


def part_feature(tag, emit):
    for name, H, I, gs, bias, act in MODELS:
        n = max(4, -(-(400 << 20) // (H * I)))                  # fc1 + fc2 of a block: H I bytes at 4 bits; 400 MiB of rotating blocks
        fused = copies(H, I, gs, bias, n, epilogue=act)
        plain = copies(H, I, gs, bias, n)
        fc2 = copies(I, H, gs, bias, n, seed=5)
        fn = ACT_FN[act]
        for M in (1, 2, 4):
            x = (torch.rand(M, H) - 0.5).half().to(DEV)
            plan = _lib.describe_plan(fused[0]._layer, M)
            a, b = timed([capture([lambda q=q: q(x) for q in fused]), capture([lambda q=q: fn(q(x)) for q in plain])], n)
            c, d = timed([capture([lambda i=i: fc2[i](fused[i](x)) for i in range(n)]), capture([lambda i=i: fc2[i](fn(plain[i](x))) for i in range(n)])], n)
            emit({"what": f"{name} fc1 {H}->{I} g{gs} {act}{' bias' if bias else ''} int4 fp16", "tag": tag, "M": M, "plan": plan["epilogue"] + " pair=" + str(plan.get("pair")),
                  "fc1_act_one_launch_us": a, "fc1_then_torch_act_us": b, "mlp_two_launches_us": c, "mlp_three_launches_us": d})
        del fused, plain, fc2
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", required=True, choices=["gated", "feature"])
    ap.add_argument("--tag", required=True)
    ap.add_argument("--log", required=True)
    a = ap.parse_args()
    _lib.load()

    def emit(d):
        line = json.dumps(d)
        print(line, flush=True)
        with open(a.log, "a") as f:
            f.write(line + "\n")
    (part_gated if a.part == "gated" else part_feature)(a.tag, emit)


if __name__ == "__main__":
    main()
