"""GPU: the grouped-sigmoid router (gptq_moe_router_grouped, through the C ABI and through moe_route_grouped) against the contract in
include/gptq_mi355x.h.  For every token of every call:

  (1) logits against the fp64 product:  |l - l64| <= C sqrt(H) 2^-24 (|x| . |w|^T) + 2^-24 |l64|  =: b   (C = 16: the project's error model for an unbroken
      chain, without a rounding to the layer dtype -- the logits stay fp32)
  (2) scores against the fp64 sigmoid of the kernel's OWN logits: relative error <= 4 * 2^-23 (expf at 1 ulp, one add, one divide at up to 1 ulp, and a
      factor of margin)
  (3) the selection IS the rule: from the emitted s, in fp32 on the host, c = s + bias, group scores = largest + second largest, a stable descending sort
      of the groups, a stable descending sort of c masked outside the kg first groups -- topk_idx equals that bit for bit, no exclusions
  (4) the selection against fp64 from x and w alone: with bc = b / 4 + 8 * 2^-24 (the sigmoid's Lipschitz constant is 1/4; the score's own rounding and the
      bias add) and bmax = max_e bc, a token is AMBIGUOUS when its fp64 margin between the kg-th and the (kg + 1)-th group score is below 4 bmax or that
      between the topk-th and the (topk + 1)-th masked c is below 2 bmax; every other token selects exactly the fp64 set, and at most 5 % of the 300 rows
      may be ambiguous per (shape, dtype) -- a condition on the inputs, not a measurement
  (5) weights against the fp64 formula on the emitted s and idx: relative error <= (topk + 4) 2^-23; renormalised with scale 1 they sum to 1 within 8 * 2^-23
plus flag independence, exact ties, row independence, guard bands, graph capture in front of moe_forward, and the softmax form's checksums against the ones
recorded from the parent commit (profiles/moe_router_softmax_form_ab.log).  The worst error-to-bound ratios are printed (pytest -s)."""
import functools
import os
import re
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from autogptq_amd import _lib  # noqa: E402
from autogptq_amd import moe as M  # noqa: E402
from autogptq_amd.moe import moe_forward, moe_route_grouped  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
C = 16.0
# (E, G, kg, topk, H): ordinary groups; the largest E and topk, a full wave; no groups; one lane slot; Eg = 20 (no power of two, no multiple of 4, more
# than two lane slots); every group stays and topk takes most experts; the smallest Eg
SHAPES = [(16, 4, 2, 4, 256), (256, 8, 4, 8, 512), (64, 1, 1, 6, 320), (8, 1, 1, 2, 256), (160, 8, 3, 6, 320), (12, 4, 4, 8, 64), (4, 2, 1, 2, 64)]
TS = [0, 1, 2, 7, 8, 9, 16, 17, 300]
DTYPES = [torch.float16, torch.bfloat16]
WORST = {}


@functools.lru_cache(maxsize=None)
def _inputs(E, H, dtype):
    """x ~ N(0, 1) [300, H], w ~ N(0, 1) / sqrt(H) [E, H], bias ~ 0.05 N(0, 1) [E] fp32, seeded on the CPU in this order; never modified."""
    g = torch.Generator().manual_seed(1000 * E + H)
    x = torch.randn((300, H), generator=g).to(dtype)
    w = (torch.randn((E, H), generator=g) / H ** 0.5).to(dtype)
    bias = 0.05 * torch.randn((E,), generator=g)
    return x.to(DEV), w.to(DEV), bias.to(DEV)


@functools.lru_cache(maxsize=None)
def _ref64(E, H, dtype):
    """(l64, b) of the 300 rows: the exact logits and the bound of check (1)."""
    x, w, _ = _inputs(E, H, dtype)
    x64, w64 = x.double(), w.double()
    l64 = x64 @ w64.t()
    b = C * H ** 0.5 * 2.0 ** -24 * (x64.abs() @ w64.abs().t()) + 2.0 ** -24 * l64.abs()
    return l64, b


def _note(what, ratio):
    WORST[what] = max(WORST.get(what, 0.0), float(ratio))


def route_c(x, w, bias, topk, G, kg, renorm, scale, outputs=True):
    """gptq_moe_router_grouped through the C ABI: (logits, scores, weights, indices); without ``outputs`` the two optional ones are NULL (None)."""
    T, H = x.shape
    E = w.shape[0]
    logits = torch.full((T, E), float("nan"), dtype=torch.float32, device=DEV) if outputs else None
    scores = torch.full((T, E), float("nan"), dtype=torch.float32, device=DEV) if outputs else None
    idx = torch.full((T, topk), -1, dtype=torch.int64, device=DEV)
    wts = torch.full((T, topk), float("nan"), dtype=torch.float32, device=DEV)
    d = _lib.describe_moe_router_grouped_plan(T, H, E, topk, G, kg, _lib.DTYPE_ENUM[x.dtype], _lib.ROUTER_RENORM if renorm else 0)
    assert d["path"] == "router_grouped" and d["form"] == ("rows" if T <= 8 else "tiles") and d["groups"] == G, d
    def ptr(t):                                  # (an empty tensor has a NULL data pointer: T = 0 validates and launches nothing, so any aligned one serves)
        return t.data_ptr() or w.data_ptr()

    _lib.check(_lib.load().gptq_moe_router_grouped(ptr(x), w.data_ptr(), _lib.ptr(bias), T, H, E, topk, G, kg, scale, _lib.DTYPE_ENUM[x.dtype],
                                                   _lib.ROUTER_RENORM if renorm else 0, _lib.ptr(logits), _lib.ptr(scores), ptr(idx), ptr(wts),
                                                   torch.cuda.current_stream(DEV).cuda_stream))
    return logits, scores, wts, idx


def rule_fp32(s, bias, G, kg, topk):
    """Check (3)'s host side: the contract's selection from the scores s, single fp32 operations only."""
    T, E = s.shape
    c = s + bias if bias is not None else s
    if G > 1:
        top2 = torch.topk(c.view(T, G, E // G), 2, dim=-1).values
        gs = top2[..., 0] + top2[..., 1]
        keep = torch.sort(gs, dim=-1, descending=True, stable=True).indices[:, :kg]
        gmask = torch.zeros((T, G), dtype=torch.bool, device=s.device).scatter_(1, keep, True)
        c = c.masked_fill(~gmask.repeat_interleave(E // G, dim=1), float("-inf"))
    return torch.sort(c, dim=-1, descending=True, stable=True).indices[:, :topk]


def ambiguous64(l64, b, bias, G, kg, topk):
    """Check (4)'s reference: (the fp64 selection as a [T, E] mask, the [T] mask of ambiguous tokens)."""
    T, E = l64.shape
    c = torch.sigmoid(l64) + (bias.double() if bias is not None else 0.0)
    bmax = (0.25 * b + 8 * 2.0 ** -24).max(-1).values
    amb = torch.zeros(T, dtype=torch.bool, device=l64.device)
    if G > 1:
        gs = torch.topk(c.view(T, G, E // G), 2, dim=-1).values.sum(-1)
        order = torch.sort(gs, dim=-1, descending=True, stable=True)
        if kg < G:
            amb |= (order.values[:, kg - 1] - order.values[:, kg]) < 4 * bmax
        gmask = torch.zeros((T, G), dtype=torch.bool, device=l64.device).scatter_(1, order.indices[:, :kg], True)
        c = c.masked_fill(~gmask.repeat_interleave(E // G, dim=1), float("-inf"))
    order = torch.sort(c, dim=-1, descending=True, stable=True)
    if topk < E:
        amb |= (order.values[:, topk - 1] - order.values[:, topk]) < 2 * bmax      # (the (topk + 1)-th may be -inf: an infinite margin)
    sel = torch.zeros((T, E), dtype=torch.bool, device=l64.device).scatter_(1, order.indices[:, :topk], True)
    return sel, amb


def check_route(x, w, bias, topk, G, kg, renorm, scale, outs, l64, b, what=""):
    """Checks (1) - (5) for every token of one call; returns the number of ambiguous tokens."""
    logits, s, wts, idx = outs
    T, H = x.shape
    E = w.shape[0]
    assert logits.shape == (T, E) and s.shape == (T, E) and logits.dtype == s.dtype == torch.float32
    assert wts.shape == (T, topk) and wts.dtype == torch.float32 and idx.shape == (T, topk) and idx.dtype == torch.int64
    if T == 0:
        return 0
    regime = "rows" if T <= 8 else "tiles"
    # (1)
    r1 = ((logits.double() - l64).abs() / b).max().item()
    _note(f"{regime} logits", r1)
    assert torch.isfinite(logits).all() and r1 <= 1.0, (what, T, r1)
    # (2)
    s64 = torch.sigmoid(logits.double())
    r2 = (((s.double() - s64).abs() / s64).max() / (4 * 2.0 ** -23)).item()
    _note(f"{regime} scores", r2)
    assert r2 <= 1.0, (what, T, r2)
    # (3)
    assert ((idx >= 0) & (idx < E)).all()
    assert torch.equal(idx, rule_fp32(s, bias, G, kg, topk)), (what, T)
    # (4)
    sel64, amb = ambiguous64(l64, b, bias, G, kg, topk)
    sel = torch.zeros((T, E), dtype=torch.bool, device=x.device).scatter_(1, idx, True)
    assert sel.sum(-1).eq(topk).all()                                                # distinct
    wrong = (sel != sel64).any(-1) & ~amb
    assert not wrong.any(), (what, T, wrong.nonzero().flatten().tolist())
    # (5)
    w64 = s.double().gather(1, idx)
    if renorm:
        w64 = w64 / (w64.sum(-1, keepdim=True) + 1e-20)
    w64 = w64 * scale
    r5 = (((wts.double() - w64).abs() / w64).max() / ((topk + 4) * 2.0 ** -23)).item()
    _note(f"{regime} weights", r5)
    assert torch.isfinite(wts).all() and r5 <= 1.0, (what, T, r5)
    if renorm and scale == 1.0:
        assert (wts.sum(-1) - 1).abs().max().item() <= 8 * 2.0 ** -23
    print(f"grouped router {what} T={T} E={E} G={G} kg={kg} topk={topk} H={H} {str(x.dtype)[6:]} [{regime}] err/bound: logits {r1:.3f} scores {r2:.3f} "
          f"weights {r5:.3f}; ambiguous {int(amb.sum())}")
    return int(amb.sum())


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
@pytest.mark.parametrize("E,G,kg,topk,H", SHAPES)
def test_grouped_router_against_fp64(E, G, kg, topk, H, dtype):
    xf, w, bias = _inputs(E, H, dtype)
    l64f, bf = _ref64(E, H, dtype)
    zero = torch.zeros_like(bias)
    for T in TS:
        x, l64, b = xf[:T], l64f[:T], bf[:T]
        for use_bias in (True, False):
            outs = {}
            for renorm in (False, True):
                for scale in (1.0, 2.5):
                    o = route_c(x, w, bias if use_bias else None, topk, G, kg, renorm, scale)
                    amb = check_route(x, w, bias if use_bias else None, topk, G, kg, renorm, scale, o, l64, b, what=f"bias={int(use_bias)} renorm={int(renorm)} scale={scale}")
                    if T == 300:
                        print(f"ambiguous rows: {amb} of 300")
                        assert amb <= 0.05 * 300, (amb, use_bias)
                    outs[(renorm, scale)] = o
            # renorm and scale change the weights only
            first = outs[(False, 1.0)]
            for o in outs.values():
                assert torch.equal(o[0], first[0]) and torch.equal(o[1], first[1]) and torch.equal(o[3], first[3])
            if not use_bias:                                                         # a NULL bias is a zero bias, bit for bit
                z = route_c(x, w, zero, topk, G, kg, True, 2.5)
                assert all(torch.equal(a, b_) for a, b_ in zip(z, outs[(True, 2.5)]))
        # moe_route_grouped is that call
        logits, wts, idx = moe_route_grouped(x, w, bias, topk, G, kg, renorm=True, scale=2.5)
        assert M.last_route_plan["path"] == "router_grouped" and M.last_route_plan["form"] == ("rows" if T <= 8 else "tiles"), M.last_route_plan
        ref = route_c(x, w, bias, topk, G, kg, True, 2.5)
        assert torch.equal(logits, ref[0]) and torch.equal(wts, ref[2]) and torch.equal(idx, ref[3])
    print("worst ratios so far:", WORST)


def test_python_entry_bias_copy_declines_and_composition():
    E, G, kg, topk, H = SHAPES[0]
    x, w, bias = _inputs(E, H, torch.float16)
    ref = moe_route_grouped(x[:5], w, bias, topk, G, kg)
    got = moe_route_grouped(x[:5], w, bias.double(), topk, G, kg)                    # not fp32: read through the cached copy (the values are the same)
    assert M.last_route_plan["path"] == "router_grouped" and all(torch.equal(a, b) for a, b in zip(ref, got))
    assert moe_route_grouped(x[:5], w, bias, topk, G, kg, return_logits=False)[0] is None
    nob = moe_route_grouped(x[:5], w, None, topk, G, kg)
    assert M.last_route_plan["path"] == "router_grouped" and torch.equal(nob[0], ref[0])
    # what the kernel does not take runs the composition, with the reason
    comp = moe_route_grouped(x[:5].float(), w.float(), bias, topk, G, kg)
    assert M.last_route_plan["path"] == "none" and "fp32" in M.last_route_plan["reason"]
    assert comp[0].dtype == torch.float32 and comp[2].shape == (5, topk)
    moe_route_grouped(x[:5], w.float(), bias, topk, G, kg)
    assert M.last_route_plan["path"] == "none" and "weight torch.float32" in M.last_route_plan["reason"]
    moe_route_grouped(x[:5], w.t().contiguous().t(), bias, topk, G, kg)
    assert M.last_route_plan["path"] == "none" and "contiguous" in M.last_route_plan["reason"]
    wp = w.clone().requires_grad_(True)
    _, val, _ = moe_route_grouped(x[:5], wp, bias, topk, G, kg)
    assert M.last_route_plan["path"] == "none" and "grad" in M.last_route_plan["reason"] and val.requires_grad
    # the composition picks the same experts where the fp64 check calls the token unambiguous
    l64, b = _ref64(E, H, torch.float16)
    _, amb = ambiguous64(l64[:300], b[:300], bias, G, kg, topk)
    fused = moe_route_grouped(x, w, bias, topk, G, kg, scale=2.5)
    with torch.no_grad():
        comp = M._route_grouped_composition(x, w, bias, topk, G, kg, True, 2.5, True)
    same = (fused[2].sort(-1).values == comp[2].sort(-1).values).all(-1)
    assert (same | amb).all()


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
def test_exact_ties_follow_the_written_rule(dtype):
    """x, w in {-1, 0, 1}: the logits are small integers, exact in fp32 in any order, equal logits give equal scores, and with a bias in {0, +-0.25} many
    tokens tie at the boundary between the experts and at the boundary between the groups."""
    E, G, kg, topk, H = 16, 4, 2, 4, 256
    T = 300
    g = torch.Generator().manual_seed(0)
    x = (torch.randint(-1, 2, (T, H), generator=g) * (torch.rand((T, H), generator=g) < 1 / 32)).to(dtype)      # sparse: logits within +-5, many equal
    w = (torch.randint(-1, 2, (E, H), generator=g) * (torch.rand((E, H), generator=g) < 1 / 4)).to(dtype)
    bias = (torch.randint(-1, 2, (E,), generator=g) * 0.25).float()
    ints = x.long() @ w.long().t()                                                   # CPU, exact
    xd, wd, bd = x.to(DEV), w.to(DEV), bias.to(DEV)
    tied_e = tied_g = None
    for rows in (T, 8, 1):                                                           # both regimes
        logits, s, wts, idx = route_c(xd[:rows], wd, bd, topk, G, kg, True, 1.0)
        assert torch.equal(logits.cpu(), ints[:rows].float())
        # equal logits give equal scores
        lc, sc = logits.flatten(), s.flatten()
        o = torch.argsort(lc)
        eq = lc[o][1:] == lc[o][:-1]
        assert torch.equal(sc[o][1:][eq], sc[o][:-1][eq])
        if rows == T:
            c = s + bd
            top2 = torch.topk(c.view(T, G, E // G), 2, dim=-1).values
            gsort = torch.sort(top2[..., 0] + top2[..., 1], dim=-1, descending=True, stable=True)
            tied_g = (gsort.values[:, kg - 1] == gsort.values[:, kg]).float().mean().item()
            gmask = torch.zeros((T, G), dtype=torch.bool, device=DEV).scatter_(1, gsort.indices[:, :kg], True)
            cm = torch.sort(c.masked_fill(~gmask.repeat_interleave(E // G, dim=1), float("-inf")), dim=-1, descending=True, stable=True).values
            tied_e = (cm[:, topk - 1] == cm[:, topk]).float().mean().item()
            print(f"exact ties: {100 * tied_e:.0f} % of tokens tie at the expert boundary, {100 * tied_g:.0f} % at the group boundary")
            assert tied_e > 0.05 and tied_g > 0.05
        assert torch.equal(idx, rule_fp32(s, bd, G, kg, topk))


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
def test_row_independence_and_reproducibility(dtype):
    E, G, kg, topk, H = 160, 8, 3, 6, 320
    xf, w, bias = _inputs(E, H, dtype)

    def route(x):
        return route_c(x, w, bias, topk, G, kg, True, 2.5)

    full8 = route(xf[:8])
    for t in range(8):
        one = route(xf[t:t + 1].clone())
        assert all(torch.equal(a[t:t + 1], b) for a, b in zip(full8, one)), t
    full = route(xf[:300])
    for t0 in range(0, 300, 16):
        part = route(xf[t0:t0 + 16].clone())
        assert all(torch.equal(a[t0:t0 + 16], b) for a, b in zip(full, part)), t0
    for T in (8, 300):
        again = route(xf[:T])
        assert all(torch.equal(a, b) for a, b in zip(full8 if T == 8 else full, again))


@pytest.mark.parametrize("T", [17, 7])
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
def test_guard_bands(dtype, T):
    from _guarded import IN_GUARD, Guarded, guard_for, guarded_like
    E, G, kg, topk, H = 160, 8, 3, 6, 320
    xf, w, bias = _inputs(E, H, dtype)
    l64, b = _ref64(E, H, dtype)
    lib = _lib.load()
    enum = _lib.DTYPE_ENUM[dtype]
    stream = torch.cuda.current_stream(DEV).cuda_stream
    gx, xv = guarded_like(xf[:T], guard_for(2 * H), IN_GUARD)
    gw, wv = guarded_like(w, guard_for(2 * H), IN_GUARD)
    gb, bv = guarded_like(bias, guard_for(4 * E), IN_GUARD)
    gl = Guarded(T * E * 4, guard_for(4 * E), device=DEV)
    gs = Guarded(T * E * 4, guard_for(4 * E), device=DEV)
    gi = Guarded(T * topk * 8, guard_for(8 * topk), device=DEV)
    gp = Guarded(T * topk * 4, guard_for(4 * topk), device=DEV)
    _lib.check(lib.gptq_moe_router_grouped(gx.ptr, gw.ptr, gb.ptr, T, H, E, topk, G, kg, 2.5, enum, _lib.ROUTER_RENORM, gl.ptr, gs.ptr, gi.ptr, gp.ptr, stream))
    torch.cuda.synchronize()
    for g, name in ((gx, "x"), (gw, "w"), (gb, "bias"), (gl, "logits_out"), (gs, "scores_out"), (gi, "topk_idx"), (gp, "topk_w")):
        g.assert_intact(name)
    outs = (gl.view(torch.float32, (T, E)), gs.view(torch.float32, (T, E)), gp.view(torch.float32, (T, topk)), gi.view(torch.int64, (T, topk)))
    assert all(torch.isfinite(o).all() for o in outs[:3])                            # every element written, the NaN guards of the inputs reached none
    check_route(xv, wv, bv, topk, G, kg, True, 2.5, outs, l64[:T], b[:T], what="guarded")
    # both optional outputs NULL: same choices and weights
    gi2 = Guarded(T * topk * 8, guard_for(8 * topk), device=DEV)
    gp2 = Guarded(T * topk * 4, guard_for(4 * topk), device=DEV)
    _lib.check(lib.gptq_moe_router_grouped(gx.ptr, gw.ptr, gb.ptr, T, H, E, topk, G, kg, 2.5, enum, _lib.ROUTER_RENORM, None, None, gi2.ptr, gp2.ptr, stream))
    torch.cuda.synchronize()
    for g, name in ((gx, "x"), (gw, "w"), (gb, "bias"), (gi2, "topk_idx"), (gp2, "topk_w")):
        g.assert_intact(name)
    assert torch.equal(gi2.view(torch.int64, (T, topk)), outs[3]) and torch.equal(gp2.view(torch.float32, (T, topk)), outs[2])


def test_graph_capture_in_front_of_the_experts():
    from test_gpu_moe import make_experts
    dtype, T, E, G, kg, topk, H = torch.float16, 4, 16, 4, 2, 4, 256
    q = make_experts(E, H, 512, 4, 128, False, dtype, seed=3, top_k=topk)
    q.post_init(decode_copy=True)
    assert q.plan(T, topk)["path"] == "decode"
    gen = torch.Generator().manual_seed(5)
    gate = (torch.randn((E, H), generator=gen) / H ** 0.5).to(dtype).to(DEV)
    bias = (0.05 * torch.randn((E,), generator=gen)).half().to(DEV)                  # fp16, as after model.half(): the cached fp32 copy is read
    x = torch.zeros((T, H), dtype=dtype, device=DEV)

    def step(inp):
        _, wts, idx = moe_route_grouped(inp, gate, bias, topk, G, kg, renorm=True, scale=2.5)
        return moe_forward(q, inp, idx, wts), idx

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.no_grad(), torch.cuda.stream(side):
        step(x)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.no_grad(), torch.cuda.graph(g):
        out, idx = step(x)
    assert M.last_route_plan["path"] == "router_grouped"
    for r in range(3):
        xn = (torch.rand((T, H), generator=torch.Generator().manual_seed(r)) - 0.5).to(dtype).to(DEV) * 4
        x.copy_(xn)
        g.replay()
        torch.cuda.synchronize()
        with torch.no_grad():
            eager, eidx = step(xn)
        assert torch.equal(idx, eidx) and torch.equal(out, eager), r


# ---------------------------------------------------------------- the softmax form keeps its bits
def test_softmax_form_keeps_the_parent_commits_bits():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from moe_router_softmax_ab import softmax_form_checksums      # the function that recorded them
    log = open(os.path.join(ROOT, "profiles", "moe_router_softmax_form_ab.log")).read()
    recorded = dict(re.findall(r"^\s*parent checksum (E=.*?renorm=\d) ([0-9a-f]{16})$", log, flags=re.M))
    mine = softmax_form_checksums()
    assert len(recorded) == len(mine) == 5 * 2 * 8 * 2, (len(recorded), len(mine))
    bad = [k for k in mine if recorded.get(k) != mine[k]]
    assert not bad, bad[:5]
