"""The fused grouped-sigmoid router (moe_route_grouped: one gptq_moe_router_grouped launch) against the transformers composition it replaces
(DeepseekV3TopkRouter.forward, operation for operation: two casts, linear, sigmoid, add, view / topk / sum, topk, zeros_like, scatter_, expand / reshape,
masked_fill, topk, gather, sum, add, div, mul), A/B in ONE process on the GPU:

  router  each variant captured as ONE graph over L routers with weights and correction biases of their own -- L chosen so that the weights together exceed
          the 256 MiB Infinity Cache (at most 320 routers) -- microseconds per router
  block   a whole DeepSeek-V3-style block (transformers' DeepseekV3MoE on random 4-bit g128 experts and shared experts): the un-injected class forward
          (eager router, QuantMoEExperts, the shared MLP as three QuantLinear calls, add) against the injected one (inject_fused_router + inject_shared_expert
          after autogptq_post_init(expert_decode_copy=True)), each captured as one graph; the input is fixed across replays, so the routing is too (a
          warm-cache number for the experts; both variants see the same one)

Router shapes (E, topk, G, kg, H): DeepSeek-V3 (256, 8, 8, 4, 7168) and a GLM-4.5-Air-like router (128, 8, 1, 1, 4096); T = 1, 2, 4, 16, 64, 512; fp16.
Block: H 4096, I 1408, I_s 1408, E 128, topk 8, G 8, kg 4; T = 1, 2, 4, 16.  Per sample ONE pair of device events around --reps back-to-back replays; the
variants alternate sample by sample; median [p10 .. p90] and the ratio of the medians (composition / fused: above 1 the fused form is faster).  The kernel is
measured in every cell (``GROUPED_SLOW_TILES = None``); "default plan" says whether moe_route_grouped runs it there by default.

    python tools/moe_router_grouped_bench.py [--samples 30] [--reps 10] [--out profiles/moe_router_grouped_ab.log] [--no-block]
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from autogptq_amd import moe as M  # noqa: E402
from autogptq_amd.moe import _route_grouped_composition, moe_route_grouped  # noqa: E402
from moe_router_bench import ab, capture, fmt  # noqa: E402

SHAPES = {"deepseek-v3": (256, 8, 8, 4, 7168), "glm-4.5-air": (128, 8, 1, 1, 4096)}      # (E, topk, G, kg, H)
TS = (1, 2, 4, 16, 64, 512)
BLOCK = dict(H=4096, I=1408, I_s=1408, E=128, topk=8, G=8, kg=4)
BLOCK_TS = (1, 2, 4, 16)
SCALE = 2.5
DEV = "cuda:0"
DEFAULT_SLOW_TILES = M.GROUPED_SLOW_TILES


def router_rows(name, samples, reps, dtype):
    E, topk, G, kg, H = SHAPES[name]
    L = min(320, -(-320 * 2 ** 20 // (E * H * 2)))
    g = torch.Generator().manual_seed(E + H)
    ws = [(torch.randn((E, H), generator=g) / H ** 0.5).to(dtype).to(DEV) for _ in range(L)]
    bs = [(0.05 * torch.randn((E,), generator=g)).to(DEV) for _ in range(L)]
    rows = []
    for T in TS:
        x = torch.randn((T, H), generator=g).to(dtype).to(DEV)

        def comp():
            return [_route_grouped_composition(x, w, b, topk, G, kg, True, SCALE, True) for w, b in zip(ws, bs)][-1]

        def fused():
            return [moe_route_grouped(x, w, b, topk, G, kg, renorm=True, scale=SCALE) for w, b in zip(ws, bs)][-1]

        M.GROUPED_SLOW_TILES = DEFAULT_SLOW_TILES
        default = M.router_grouped_plan(T, H, E, topk, G, kg, dtype, True)["path"]          # what moe_route_grouped does by default at this cell
        M.GROUPED_SLOW_TILES = None                 # ... the kernel is measured in every cell
        graphs, outs = {}, {}
        graphs["composition"], outs["composition"] = capture(comp)
        graphs["fused"], outs["fused"] = capture(fused)
        assert M.last_route_plan["path"] == "router_grouped", M.last_route_plan
        for gr in graphs.values():                  # (a capture runs nothing: the outputs hold values after a replay)
            gr.replay()
        torch.cuda.synchronize()
        same = (outs["composition"][2].sort(-1).values == outs["fused"][2].sort(-1).values).all(-1).float().mean().item()
        r = {k: tuple(v / L for v in t) for k, t in ab(graphs, samples, reps).items()}
        rows.append(f"  router {name:12s} T={T:<4d} {M.last_route_plan['form']:5s} L={L:<3d} | composition {fmt(r['composition'])}  fused {fmt(r['fused'])}  "
                    f"ratio {r['composition'][0] / r['fused'][0]:6.2f}   (same expert sets: {100 * same:.1f} % of tokens; default plan: "
                    f"{'fused' if default == 'router_grouped' else 'composition'})")
        print(rows[-1], flush=True)
        del graphs
    return rows


def make_block(dtype):
    """transformers' DeepseekV3MoE with random 4-bit g128 QuantMoEExperts / QuantLinear shared experts and a random router, on the GPU."""
    from transformers import DeepseekV3Config
    from transformers.models.deepseek_v3.modeling_deepseek_v3 import DeepseekV3MoE
    from autogptq_amd.qlinear_mi355x import QuantLinear
    from test_gpu_moe import _fill, make_experts
    c = BLOCK
    cfg = DeepseekV3Config(hidden_size=c["H"], intermediate_size=c["I"], moe_intermediate_size=c["I"], n_shared_experts=c["I_s"] // c["I"],
                           n_routed_experts=c["E"], num_experts_per_tok=c["topk"], n_group=c["G"], topk_group=c["kg"], routed_scaling_factor=SCALE,
                           norm_topk_prob=True, num_hidden_layers=1, num_attention_heads=4, num_key_value_heads=4, vocab_size=64)
    with torch.device("meta"):
        blk = DeepseekV3MoE(cfg)
    blk.experts = make_experts(c["E"], c["H"], c["I"], 4, 128, False, dtype, seed=1, top_k=c["topk"])
    gen = torch.Generator().manual_seed(2)
    for nm, (k, n) in zip(("gate_proj", "up_proj", "down_proj"), ((c["H"], c["I_s"]), (c["H"], c["I_s"]), (c["I_s"], c["H"]))):
        l = QuantLinear(4, 128, k, n, False, weight_dtype=dtype)
        _fill(l, gen, False)
        setattr(blk.shared_experts, nm, l.to(DEV))
    blk.gate.to_empty(device=DEV)
    blk.gate.weight.data = (torch.randn((c["E"], c["H"]), generator=gen) / c["H"] ** 0.5).to(dtype).to(DEV)
    blk.gate.e_score_correction_bias.data = (0.05 * torch.randn((c["E"],), generator=gen)).to(dtype).to(DEV)
    return blk.eval()


def block_rows(samples, reps, dtype):
    from autogptq_amd.model_utils import autogptq_post_init
    blk = make_block(dtype)
    holder = torch.nn.ModuleList([blk])
    assert M.inject_shared_expert(holder) == 1                      # before post_init: its scratch then covers the fused call
    autogptq_post_init(holder, max_input_length=64, expert_decode_copy=True)
    M.remove_shared_expert(holder)
    rows = []
    for T in BLOCK_TS:
        x = (torch.randn((1, T, BLOCK["H"]), generator=torch.Generator().manual_seed(T)) * 0.5).to(dtype).to(DEV)
        graphs = {}
        graphs["class forward"], ref = capture(lambda: blk(x))
        assert M.inject_fused_router(holder) == 1 and M.inject_shared_expert(holder) == 1
        graphs["injected"], out = capture(lambda: blk(x))
        plan = dict(blk.experts.last_plan)
        assert M.last_route_plan["path"] == "router_grouped" and plan["shared"] in ("decode", "combine"), (M.last_route_plan, plan)
        M.remove_fused_router(holder), M.remove_shared_expert(holder)
        for gr in graphs.values():
            gr.replay()
        torch.cuda.synchronize()
        err = (out.float() - ref.float()).abs().max().item() / max(1.0, ref.float().abs().max().item())
        r = ab(graphs, samples, reps)
        rows.append(f"  block  H={BLOCK['H']} I={BLOCK['I']} E={BLOCK['E']} T={T:<3d} shared={plan['shared']:7s} experts={plan['path']:7s} | class forward "
                    f"{fmt(r['class forward'])}  injected {fmt(r['injected'])}  ratio {r['class forward'][0] / r['injected'][0]:6.2f}  "
                    f"saved {r['class forward'][0] - r['injected'][0]:8.2f} us   (max |diff| / scale {err:.1e})")
        print(rows[-1], flush=True)
        del graphs
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=30)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "moe_router_grouped_ab.log"))
    ap.add_argument("--no-block", action="store_true")
    ap.add_argument("--shapes", default=",".join(SHAPES))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "moe_router_grouped_bench.py needs the GPU"
    assert args.samples * args.reps >= 200, "at least 200 replays per variant"
    dtype = torch.float16
    M.GROUPED_SLOW_TILES = None                     # (the block rows too)
    lines = [f"# fused grouped-sigmoid router vs the transformers composition (DeepseekV3TopkRouter.forward), fp16, {torch.cuda.get_device_name(0)}; "
             f"microseconds: median [p10 .. p90] of {args.samples} samples x {args.reps} replays, variants alternating; ratio = composition / fused",
             "# router rows: one graph over L routers with weights of their own (together above the Infinity Cache), per router; block rows: one "
             "DeepseekV3MoE block on 4-bit g128 experts, per block, fixed input (warm cache for the experts, the same for both variants)"]
    print("\n".join(lines), flush=True)
    for name in args.shapes.split(","):
        lines += router_rows(name, args.samples, args.reps, dtype)
        torch.cuda.empty_cache()
    if not args.no_block:
        lines += block_rows(args.samples, args.reps, dtype)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
