"""The softmax form of the router (gptq_moe_router) of the parent commit's library against this tree's: the grouped-sigmoid form is a launch-uniform mode of
the same two kernels, so the softmax form has to keep its bits and its time.  One process per line group, alternating ("parent", "this tree", twice):
each imports autogptq_amd from ONE checkout (--parent-root: a built checkout of the parent commit), prints sha256 prefixes of gptq_moe_router's outputs on
the inputs of tests/test_gpu_moe_router.py (every shape, dtype, token count, renorm on and off) and times moe_route as a captured graph over --layers routers with weights of their own: median [p10 .. p90] of
--samples samples x --reps replays, microseconds per router.  tests/test_gpu_moe_router_grouped.py compares this tree's checksums with the "parent
checksum" lines of the log.

    python tools/moe_router_softmax_ab.py --parent-root <built checkout of the parent commit> [--out profiles/moe_router_softmax_form_ab.log]
"""
import argparse
import hashlib
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SHAPES = {"mixtral8x7b": (8, 2, 4096), "e60": (60, 4, 2048), "e128": (128, 8, 2048), "e256": (256, 8, 512)}      # (E, topk, H)
TS = (1, 4, 8, 16, 64, 2048)


def softmax_form_checksums():
    """{key: sha256 prefix} of gptq_moe_router's outputs on the inputs of tests/test_gpu_moe_router.py: its shapes, dtypes and token counts, renorm on and
    off.  (autogptq_amd and tests/ must be importable.)"""
    import torch
    from autogptq_amd import moe as M
    from test_gpu_moe_router import DTYPES, SHAPES as TEST_SHAPES, TS as TEST_TS, _inputs
    out = {}
    for E, topk, H in TEST_SHAPES:
        for dtype in DTYPES:
            xf, w = _inputs(E, H, dtype)
            for T in TEST_TS:
                if T == 0:
                    continue
                for renorm in (False, True):
                    res = M.moe_route(xf[:T], w, topk, renorm=renorm)
                    assert M.last_route_plan["path"] == "router"
                    h = hashlib.sha256()
                    for t in res:
                        h.update(t.contiguous().view(torch.uint8).cpu().numpy().tobytes())
                    out[f"E={E} topk={topk} H={H} {str(dtype)[6:]} T={T} renorm={int(renorm)}"] = h.hexdigest()[:16]
    return out


def child(label, root, layers, samples, reps):
    for p in (os.path.join(root, "tools"), os.path.join(root, "tests"), root):
        sys.path.insert(0, p)
    import torch
    from autogptq_amd import moe as M
    from autogptq_amd.moe import moe_route
    from moe_router_bench import ab, capture, fmt
    assert os.path.abspath(M.__file__).startswith(os.path.abspath(root) + os.sep), M.__file__
    dev, dtype = "cuda:0", torch.float16
    for k, v in softmax_form_checksums().items():
        print(f"{label:>9s} checksum {k} {v}", flush=True)
    for name, (E, topk, H) in SHAPES.items():
        g = torch.Generator().manual_seed(E + H)
        ws = [(torch.randn((E, H), generator=g) / H ** 0.5).to(dtype).to(dev) for _ in range(layers)]
        for T in TS:
            x = torch.randn((T, H), generator=g).to(dtype).to(dev)

            def run():
                return [moe_route(x, w, topk, renorm=True) for w in ws][-1]

            graph, _ = capture(run)
            assert M.last_route_plan["path"] == "router"
            r = ab({"g": graph}, samples, reps)["g"]
            print(f"{label:>9s} {name:>12s} T={T:<5d} {M.last_route_plan['form']:5s}: {fmt(tuple(v / layers for v in r))} us per router", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-root")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "moe_router_softmax_form_ab.log"))
    ap.add_argument("--layers", type=int, default=16)
    ap.add_argument("--samples", type=int, default=30)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--child", nargs=2, metavar=("LABEL", "ROOT"))
    args = ap.parse_args()
    if args.child:
        return child(args.child[0], args.child[1], args.layers, args.samples, args.reps)
    assert args.parent_root and os.path.isdir(args.parent_root), "--parent-root: a built checkout of the parent commit"
    lines = ["# tools/moe_router_softmax_ab.py, one process per line group, alternating: gptq_moe_router (the softmax form) of the parent commit's library "
             '("parent") and of this commit\'s ("this tree"); MI355X, fp16, moe_route in a captured graph over '
             f"{args.layers} routers with weights of their own,",
             f"# median [p10 .. p90] of {args.samples} samples x {args.reps} replays, us per router; checksum: sha256 prefix of (logits, weights, indices) on the "
             "inputs of tests/test_gpu_moe_router.py -- equal between the two: the same bits"]
    for label, root in (("parent", args.parent_root), ("this tree", ROOT)) * 2:
        env = dict(os.environ)
        env.pop("GPTQ_MI355X_LIB", None)
        env.pop("PYTHONPATH", None)
        res = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", label, os.path.abspath(root), "--layers", str(args.layers),
                              "--samples", str(args.samples), "--reps", str(args.reps)], env=env, capture_output=True, text=True, timeout=600,
                             cwd=os.path.abspath(root))
        if res.returncode:                        # nothing more is started after a failure
            print(res.stdout[-2000:], res.stderr[-4000:], sep="\n", file=sys.stderr)
            return res.returncode
        out = res.stdout
        got = [ln for ln in out.splitlines() if ln.startswith(f"{label:>9s} ")]
        print("\n".join(got), flush=True)
        lines += got
    sums = {}
    for ln in lines:
        if " checksum " in ln:
            label, rest = ln.split(" checksum ")
            key, val = rest.rsplit(" ", 1)
            sums.setdefault(key, set()).add(val)
    differ = [k for k, v in sums.items() if len(v) != 1]
    lines.append(f"# checksums: {len(sums)} cells, {len(differ)} differ between the parent and this tree" + (": " + "; ".join(differ[:8]) if differ else ""))
    print(lines[-1])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
