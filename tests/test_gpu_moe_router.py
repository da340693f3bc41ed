"""GPU: the fused mixture-of-experts router (gptq_moe_router through moe_route / inject_fused_router) against the contract in include/gptq_mi355x.h.

For every token, no exclusions:
  (1) logits against the fp64 product with the project's error model (test_gpu_error_model.py; C = 16: an unbroken chain over the whole K)
          |l - l64| <= (1/2 + 1/64) ulp_D(l64) + C sqrt(H) 2^-24 (|x| . |w|^T)                                                      =: b
  (2) the selection IS the rule: a stable sort of the kernel's own logits by (logit descending, index ascending) reproduces topk_idx bit for bit
  (3) the selection is a true top-k of the exact logits up to the bound: with kappa the k-th largest fp64 logit, every selected expert has
      l64 + 2 b >= kappa and every unselected one l64 - 2 b <= kappa (no near-tie exclusion list)
  (4) weights against the fp64 formulas on the emitted logits and indices: relative error <= (16 + 2 span + E / 2) 2^-23, span = max logit - smallest
      selected logit (exp, the rounding of its argument, a sequential fp32 sum of E terms)
plus exact ties, row independence, guard bands, graph capture in front of moe_forward, and a tiny Mixtral with the router injected.  The worst
error-to-bound ratios are printed (pytest -s) per row regime."""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from autogptq_amd import _lib  # noqa: E402
from autogptq_amd import moe as M  # noqa: E402
from autogptq_amd.moe import moe_forward, moe_route  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
C = 16.0
SHAPES = [(8, 2, 256), (60, 4, 320), (256, 8, 512), (3, 1, 64), (8, 8, 256)]      # (E, topk, H)
TS = [0, 1, 2, 7, 8, 9, 16, 17, 300]
DTYPES = [torch.float16, torch.bfloat16]
WORST = {}                                   # (regime, what) -> worst ratio to its bound seen so far (printed)


def _ulp(y64, dtype):
    mant, emin = (10, -14) if dtype == torch.float16 else (7, -126)
    e = torch.floor(torch.log2(y64.abs().clamp_min(2.0 ** emin)))
    return torch.pow(torch.tensor(2.0, dtype=torch.float64, device=y64.device), e - mant)


@functools.lru_cache(maxsize=None)
def _inputs(E, H, dtype, wscale=1.0, rows=300):
    """x ~ N(0, 1) [rows, H], w ~ N(0, 1) / sqrt(H) * wscale [E, H], seeded on the CPU; never modified."""
    g = torch.Generator().manual_seed(1000 * E + H)
    x = torch.randn((rows, H), generator=g).to(dtype)
    w = (torch.randn((E, H), generator=g) / H ** 0.5 * wscale).to(dtype)
    return x.to(DEV), w.to(DEV)


def _note(regime, what, ratio):
    key = (regime, what)
    WORST[key] = max(WORST.get(key, 0.0), float(ratio))


def check_route(x, w, topk, renorm, logits, wts, idx, what=""):
    """Checks (1) - (4) for every token of one call."""
    T, H = x.shape
    E = w.shape[0]
    dtype = x.dtype
    assert logits.shape == (T, E) and logits.dtype == dtype
    assert wts.shape == (T, topk) and wts.dtype == torch.float32 and idx.shape == (T, topk) and idx.dtype == torch.int64
    if T == 0:
        return
    regime = "rows" if T <= 8 else "tiles"
    x64, w64 = x.double(), w.double()
    l64 = x64 @ w64.t()
    b = (0.5 + 1.0 / 64) * _ulp(l64, dtype) + C * H ** 0.5 * 2.0 ** -24 * (x64.abs() @ w64.abs().t())
    lk = logits.double()
    # (1)
    r1 = ((lk - l64).abs() / b).max().item()
    _note(regime, "logits", r1)
    print(f"router {what} T={T} E={E} H={H} {dtype} [{regime}] logits err/bound {r1:.3f}")
    assert r1 <= 1.0, (what, T, r1)
    # (2)
    assert ((idx >= 0) & (idx < E)).all()
    order = torch.sort(logits.float(), dim=-1, descending=True, stable=True).indices[:, :topk]
    assert torch.equal(idx, order), (what, T)
    # (3)
    kappa = torch.topk(l64, topk, dim=-1).values[:, -1:]
    sel = torch.zeros((T, E), dtype=torch.bool, device=x.device).scatter_(1, idx, True)
    assert sel.sum(-1).eq(topk).all()                                                # distinct
    assert ((l64 + 2 * b >= kappa) | ~sel).all(), (what, T)
    assert ((l64 - 2 * b <= kappa) | sel).all(), (what, T)
    # (4)
    p64 = torch.softmax(lk, dim=-1).gather(1, idx)
    if renorm:
        p64 = p64 / p64.sum(-1, keepdim=True)
    span = lk.max(-1).values - lk.gather(1, idx).min(-1).values
    tol = (16 + 2 * span + E / 2) * 2.0 ** -23
    rel = ((wts.double() - p64).abs() / p64).max(-1).values
    r4 = (rel / tol).max().item()
    _note(regime, "weights", r4)
    print(f"router {what} T={T} E={E} H={H} {dtype} [{regime}] weights rel err {rel.max().item() / 2.0 ** -23:.2f} x 2^-23, err/bound {r4:.3f}")
    assert torch.isfinite(wts).all() and r4 <= 1.0, (what, T, r4)


def route(x, w, topk, renorm):
    logits, wts, idx = moe_route(x, w, topk, renorm=renorm)
    assert M.last_route_plan["path"] == "router" and M.last_route_plan["form"] == ("rows" if x.shape[0] <= 8 else "tiles"), M.last_route_plan
    return logits, wts, idx


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
@pytest.mark.parametrize("E,topk,H", SHAPES)
def test_router_against_fp64(E, topk, H, dtype):
    xf, w = _inputs(E, H, dtype)
    for T in TS:
        x = xf[:T]
        outs = {}
        for renorm in (False, True):
            logits, wts, idx = route(x, w, topk, renorm)
            check_route(x, w, topk, renorm, logits, wts, idx, what=f"renorm={int(renorm)}")
            outs[renorm] = (logits, wts, idx)
        # the flag changes the weights only
        assert torch.equal(outs[False][0], outs[True][0]) and torch.equal(outs[False][2], outs[True][2])
        if T:
            assert (outs[True][1].sum(-1) - 1).abs().max().item() <= 8 * 2.0 ** -23
    print("worst ratios so far:", WORST)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
def test_wide_logit_spans(dtype):
    """w scaled by 6: logit spans of about 17, where the rounding of exp's argument dominates the weights' error."""
    E, topk, H = 60, 4, 320
    xf, w = _inputs(E, H, dtype, wscale=6.0)
    for T in (7, 17, 300):
        for renorm in (False, True):
            logits, wts, idx = route(xf[:T], w, topk, renorm)
            check_route(xf[:T], w, topk, renorm, logits, wts, idx, what=f"x6 renorm={int(renorm)}")
    span = (logits.float().max(-1).values - logits.float().min(-1).values).max().item()
    assert span > 12, span
    print("worst ratios so far:", WORST)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
def test_exact_ties_follow_the_written_rule(dtype):
    """x, w in {-1, 0, 1}: the logits are small integers, exact in both dtypes, and many tokens tie at the selection boundary."""
    H, E, topk, T = 64, 12, 2, 64
    g = torch.Generator().manual_seed(0)
    x = torch.randint(-1, 2, (T, H), generator=g).to(dtype)
    w = torch.randint(-1, 2, (E, H), generator=g).to(dtype)
    ints = x.long() @ w.long().t()                                                   # CPU, exact
    ref = torch.sort(ints, dim=-1, descending=True, stable=True)
    tied = (ref.values[:, topk - 1] == ref.values[:, topk]).float().mean().item()
    print(f"exact ties: {100 * tied:.0f} % of tokens tie at the selection boundary")
    assert tied > 0.05
    xd, wd = x.to(DEV), w.to(DEV)
    for rows in (T, 8, 1):                                                           # both regimes
        logits, wts, idx = route(xd[:rows], wd, topk, True)
        assert torch.equal(logits.cpu().long(), ints[:rows]) and torch.equal(logits.cpu().float(), ints[:rows].float())
        assert torch.equal(idx.cpu(), ref.indices[:rows, :topk])


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
def test_row_independence_and_reproducibility(dtype):
    E, topk, H = 60, 4, 320
    xf, w = _inputs(E, H, dtype)
    full8 = route(xf[:8], w, topk, True)
    for t in range(8):
        one = route(xf[t:t + 1].clone(), w, topk, True)
        assert all(torch.equal(a[t:t + 1], b) for a, b in zip(full8, one)), t
    full = route(xf[:300], w, topk, True)
    for t0 in range(0, 300, 16):
        part = route(xf[t0:t0 + 16].clone(), w, topk, True)
        assert all(torch.equal(a[t0:t0 + 16], b) for a, b in zip(full, part)), t0
    for T in (8, 300):
        again = route(xf[:T], w, topk, True)
        assert all(torch.equal(a, b) for a, b in zip(full8 if T == 8 else full, again))


@pytest.mark.parametrize("T", [17, 7])
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
def test_guard_bands(dtype, T):
    from _guarded import IN_GUARD, Guarded, guard_for, guarded_like
    E, topk, H = 60, 4, 320
    xf, w = _inputs(E, H, dtype)
    lib = _lib.load()
    enum = _lib.DTYPE_ENUM[dtype]
    stream = torch.cuda.current_stream(DEV).cuda_stream
    for inf_row in (False, True):
        xin = xf[:T].clone()
        if inf_row:
            xin[T // 2] = float("inf")
        gx, xv = guarded_like(xin, guard_for(2 * H), IN_GUARD)
        gw, wv = guarded_like(w, guard_for(2 * H), IN_GUARD)
        gl = Guarded(T * E * 2, guard_for(2 * E), device=DEV)
        gi = Guarded(T * topk * 8, guard_for(8 * topk), device=DEV)
        gp = Guarded(T * topk * 4, guard_for(4 * topk), device=DEV)
        _lib.check(lib.gptq_moe_router(gx.ptr, gw.ptr, T, H, E, topk, enum, _lib.ROUTER_RENORM, gl.ptr, gi.ptr, gp.ptr, stream))
        torch.cuda.synchronize()
        for g, name in ((gx, "x"), (gw, "w"), (gl, "logits_out"), (gi, "topk_idx"), (gp, "topk_w")):
            g.assert_intact(name)
        logits, idx, wts = gl.view(dtype, (T, E)), gi.view(torch.int64, (T, topk)), gp.view(torch.float32, (T, topk))
        assert ((idx >= 0) & (idx < E)).all()
        assert torch.zeros((T, E), dtype=torch.bool, device=DEV).scatter_(1, idx, True).sum(-1).eq(topk).all()      # distinct, the Inf row included
        keep = torch.ones(T, dtype=torch.bool, device=DEV)
        if inf_row:
            keep[T // 2] = False
        assert torch.isfinite(logits[keep]).all() and torch.isfinite(wts[keep]).all()      # the NaN guards of x and w reached no output
        if not inf_row:
            check_route(xv, wv, topk, True, logits, wts, idx, what="guarded")
            # NULL logits_out: same choices and weights
            gi2 = Guarded(T * topk * 8, guard_for(8 * topk), device=DEV)
            gp2 = Guarded(T * topk * 4, guard_for(4 * topk), device=DEV)
            _lib.check(lib.gptq_moe_router(gx.ptr, gw.ptr, T, H, E, topk, enum, _lib.ROUTER_RENORM, None, gi2.ptr, gp2.ptr, stream))
            torch.cuda.synchronize()
            gi2.assert_intact("topk_idx"), gp2.assert_intact("topk_w")
            assert torch.equal(gi2.view(torch.int64, (T, topk)), idx) and torch.equal(gp2.view(torch.float32, (T, topk)), wts)


def test_graph_capture_in_front_of_the_experts():
    from test_gpu_moe import make_experts
    dtype, T, E, H = torch.float16, 4, 8, 256
    q = make_experts(E, H, 512, 4, 128, False, dtype, seed=3)
    q.post_init(decode_copy=True)
    assert q.plan(T, 2)["path"] == "decode"
    gate = (torch.randn((E, H), generator=torch.Generator().manual_seed(5)) / H ** 0.5).to(dtype).to(DEV)
    x = torch.zeros((T, H), dtype=dtype, device=DEV)

    def step(inp):
        _, wts, idx = moe_route(inp, gate, 2, renorm=True)
        return moe_forward(q, inp, idx, wts), idx

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.no_grad(), torch.cuda.stream(side):
        step(x)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.no_grad(), torch.cuda.graph(g):
        out, idx = step(x)
    assert M.last_route_plan["path"] == "router"
    for r in range(3):
        xn = (torch.rand((T, H), generator=torch.Generator().manual_seed(r)) - 0.5).to(dtype).to(DEV) * 4
        x.copy_(xn)
        g.replay()
        torch.cuda.synchronize()
        with torch.no_grad():
            eager, eidx = step(xn)
        assert torch.equal(idx, eidx) and torch.equal(out, eager), r


def test_tiny_mixtral_with_the_router_injected(tmp_path):
    from transformers import StaticCache
    from autogptq_amd.model_utils import capture_decode_step
    from test_gpu_moe import _tiny
    TM, model, _ = _tiny(tmp_path, False)
    layers = len(model.model.layers)
    assert M.inject_fused_router(model) == layers
    seen = []
    hooks = [layer.mlp.gate.register_forward_hook(lambda m, args, out: seen.append((m, args[0], out))) for layer in model.model.layers]
    ids = torch.randint(0, 512, (1, 12), generator=torch.Generator().manual_seed(0)).to(DEV)
    with torch.no_grad():
        res = model(ids, output_router_logits=True)
    for h in hooks:
        h.remove()
    assert torch.isfinite(res.logits.float()).all() and len(seen) == layers and len(res.router_logits) == layers
    assert M.last_route_plan["path"] == "router"
    assert model.model.layers[0].mlp.experts.last_plan["path"] == "grouped"
    for (m, hs, (logits, scores, idx)), rl in zip(seen, res.router_logits):
        assert scores.dtype == torch.float32 and torch.equal(rl, logits)
        check_route(hs.reshape(-1, TM.H), m.weight, TM.TOPK, True, logits, scores, idx, what="tiny mixtral")
    ids = torch.randint(0, 512, (1, 8), generator=torch.Generator().manual_seed(1)).to(DEV)
    with torch.no_grad():
        ref = model.generate(ids, max_new_tokens=8, do_sample=False)[0, 8:]
    cache = StaticCache(config=model.config, max_cache_len=64)
    with torch.no_grad():
        logits = model(ids, past_key_values=cache, use_cache=True).logits
    tok = logits[:, -1].argmax(-1)
    step = capture_decode_step(model, cache)
    got = [tok.item()]
    for _ in range(7):
        tok = step(tok.view(1, 1))[:, -1].argmax(-1)
        got.append(tok.item())
    assert got == ref.tolist()
    assert M.remove_fused_router(model) == layers
    for layer in model.model.layers:
        assert "forward" not in layer.mlp.gate.__dict__ and layer.mlp.gate.forward.__func__ is type(layer.mlp.gate).forward
