"""GPU (-m gpu): dense 2-bit layers at 5+ rows on their decode copy (opt-in: QuantLinear.post_init(low_bit_rows=True) = GPTQ_COPY_ROWS_INT2 in tiled_cols) --
the DENSE forms of moe_rows_lowbit_kernel<T, 2> (16-row tiles x 4 strips x the whole K) and moe_panel_lowbit_kernel<T, 2> (64-row tiles x 128 columns x the
whole K): no tables, tile t = rows [BM t, min(BM t + BM, M)), out = T(sum + bias).

Forced with the lab knobs ROWS_ON / PANEL_ON on shapes chosen for the seams (one chunk, a one-row last tile, the last strip group, 32- / 64- / 128- / 256-wide
groups and one group for the whole K, act-order, uneven chunk ranges per wave, idle waves), and left to the planner on the shapes where it takes them by itself.
Every case: the plan, EVERY output against x (fp64) @ W_oracle (fp64) + bias under the project's per-output bound (tests/_error_model.py: C from
constant_for, the K weight roundings of the matrix-core GEMM families as explicit terms -- nothing fitted), a repeated call bit-identical, one-hot rows
through every tile = the oracle's exact dequantised rows, a row's bits independent of the other rows of its call, both zero-point conventions."""
import ctypes
import functools

import pytest
import torch
import torch.nn.functional as F

import _error_model as EM
import _guarded as G
from autogptq_amd import _lib
from autogptq_amd.qlinear_mi355x import QuantLinear, forward_multi, mlp_forward
from oracle import gptq_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DT_IDS = {torch.float16: "fp16", torch.bfloat16: "bf16"}

# (K, N, group_size, M, act_order, what the shape exercises)
ROWS_CASES = [
    (128, 64, 128, 7, False, "one chunk, one wave: the ring is never refilled"),
    (512, 64, 128, 5, False, "4 chunks on 2 waves, 5 rows of one tile"),
    (1024, 192, 128, 17, False, "the second tile has ONE row; three strip groups"),
    (2048, 256, 32, 33, False, "32-wide groups (one per k-slot), 33 rows = three tiles"),
    (1536, 192, 64, 64, True, "64-wide groups, act-order (x permuted in natural order by the pre-pass), four full tiles"),
    (4096, 128, 256, 50, False, "groups of 256 (two chunks per group), a 2-row last tile"),
    (1280, 128, 1280, 48, True, "one group for the whole K, a permuted g_idx"),
    (11008, 64, 128, 31, False, "86 chunks: uneven chunk ranges per wave"),
]
# N is a whole number of the panel form's 128-column tiles (NT = 4 blocks of 32) in every case of the issue
PANEL_CASES = [
    (128, 128, 128, 65, False, "two 64-deep steps: six of the eight waves idle; the second tile has ONE row"),
    (512, 512, 128, 129, False, "one step per wave, three tiles (the last: one row), four column tiles"),
    (256, 1024, 64, 333, True, "64-wide groups (constants every step), act-order, a 13-row last tile"),
    (768, 256, 768, 767, True, "one group for the whole K, a permuted g_idx, a 63-row last tile"),
    (4096, 128, 128, 256, False, "eight steps per wave, four full tiles"),
    (16384, 128, 128, 100, False, "32 steps per wave: the deepest K loop"),
]


def _ids(cases):
    return [f"{c[0]}x{c[1]}g{c[2]}M{c[3]}{'act' if c[4] else ''}" for c in cases]


def _tune(knob):
    t = _lib.GptqTuning()
    t.path, t.reserved[_lib.LAB.GEMM_VARIANT] = 3, knob
    return t


def _rows_on():
    return _tune(_lib.LAB.VARIANT_ROWS_ON)


def _panel_on():
    return _tune(_lib.LAB.VARIANT_PANEL_ON)


@functools.lru_cache(maxsize=None)
def _layer(K, N, gs, act, dtype, seed):
    """The oracle's random 2-bit layer with a bias (CPU tensors; shared by the tests, never modified)."""
    return O.random_quant_layer(K, N, 2, gs, act_order=act, seed=seed, bias=True, dtype=dtype)


def _module(Lq, dtype, zero_mode="auto", flag=True, release=False, bias=True, wide=False):
    """wide: GPTQ_COPY_ROWS_INT2_WIDE on a layer with both layouts resident (the C ABI's bit; post_init sets it by itself on a released layer)."""
    q = QuantLinear(2, Lq["group_size"], Lq["K"], Lq["N"], bias, weight_dtype=dtype, zero_mode=zero_mode)
    q.qweight, q.qzeros, q.scales, q.g_idx = Lq["qweight"].clone(), Lq["qzeros"].clone(), Lq["scales"].clone(), Lq["g_idx"].clone().to(torch.int32)
    if bias:
        q.bias = Lq["bias"].clone()
    q = q.to(DEV)
    q.post_init(low_bit_rows=flag, release_checkpoint_layout=release)
    assert q._qweight_tiled is not None
    assert bool(q._layer.tiled_cols & _lib.COPY_ROWS_INT2) == flag and _lib.copy_cols(q._layer.tiled_cols) == _lib.STRIP_COLS
    assert bool(q._layer.tiled_cols & _lib.COPY_ROWS_INT2_WIDE) == (flag and release and not q.act_order)
    if wide:
        q._layer.tiled_cols |= _lib.COPY_ROWS_INT2_WIDE
    return q


def _mode(q):
    return O.ZERO_NOWRAP if q.resolved_zero_mode() == _lib.ZERO_NOWRAP else O.ZERO_WRAP


def _x(M, K, dtype, seed):
    return (torch.rand(M, K, generator=torch.Generator().manual_seed(seed)) - 0.5).to(dtype).to(DEV)


def _within_the_model(q, Lq, x, y, plan, what):
    """EVERY output inside the per-output bound of the project's error model; returns worst err / bound."""
    K, gs, dtype = Lq["K"], Lq["group_size"], q._w_dtype
    W64 = EM.w64(Lq, 2, _mode(q), DEV)
    x64 = x.double()
    y64 = x64 @ W64 + (Lq["bias"].to(DEV).double() if q.bias is not None else 0.0)
    A = x64.abs() @ EM.abs_weights(Lq, 2, dtype, W64)
    assert plan["path"] == "gemm" and EM.rounds_each_weight(plan, dtype)
    bnd = EM.bound(y64, A, K, dtype, EM.constant_for(plan, dtype, -1 if gs >= K else gs), ((x64, W64),))
    err = (y.double() - y64).abs()
    ratio = float((err / bnd).max())
    print(f"{what}: worst err / bound = {ratio:.3f}")
    bad = err > bnd
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} / {bad.numel()} outputs outside the error model, worst err / bound = {ratio:.3f} at {torch.nonzero(bad)[0].tolist()}"
    return ratio


def _forced_case(case, dtype, t, kernel, bm, cols):
    K, N, gs, M, act, _ = case
    Lq = _layer(K, N, gs, act, dtype, K + N + M)
    for zm in (("auto",) if act else ("wrap", "nowrap")):
        q = _module(Lq, dtype, zm)
        what = f"{kernel} int2 {K}x{N} g{gs} M={M} act={act} {DT_IDS[dtype]} zero={zm}"
        plan = _lib.describe_plan(q._layer, M, t)
        assert plan["kernel"] == kernel and plan.get("body") == "lowbit" and plan["tiles"] == f"{-(-M // bm)}x{N // cols}" and plan["ksplit"] == 1, plan
        assert plan["perm"] == (1 if q.act_order else 0), plan
        need = int(_lib.load().gptq_workspace_bytes_ex(ctypes.byref(q._layer), M, ctypes.byref(t)))
        assert need == (65536 + (M * K * 2 + 255) // 256 * 256 if q.act_order else 0), (what, need)      # nothing, or the header + the permuted x
        x = _x(M, K, dtype, M)
        with torch.no_grad():
            y, y2 = q(x, tuning=t), q(x, tuning=t)
        assert y.shape == (M, N) and torch.equal(y, y2), f"{what}: not bit-reproducible"
        _within_the_model(q, Lq, x, y, plan, what)
        # one-hot rows through every tile: the oracle's exact dequantised weight rows (bias off for the call)
        W = O.dequantize(Lq["qweight"], Lq["qzeros"], Lq["scales"], Lq["g_idx"], 2, _mode(q)).to(DEV)
        rows = torch.arange(M, device=DEV)
        hot = torch.zeros(M, K, dtype=dtype, device=DEV)
        hot[rows, (rows * 37 + 5) % K] = 1.0
        saved, q._layer.bias = q._layer.bias, None
        with torch.no_grad():
            yh = q(hot, tuning=t)
        q._layer.bias = saved
        assert torch.equal(yh, W[(rows * 37 + 5) % K]), f"{what}: one-hot rows are not the exact dequantised weight rows"
        # a row's bits do not depend on the other rows of its call: the same row alone (M = 1, forced onto the form by the knob) and in a 5-row call
        for r in sorted({0, M // 2, M - 1}):
            assert _lib.describe_plan(q._layer, 1, t).get("body") == "lowbit"
            with torch.no_grad():
                y1 = q(x[r:r + 1].contiguous(), tuning=t)
            assert torch.equal(y1[0], y[r]), f"{what}: row {r} alone differs from row {r} of the {M}-row call"
        five = torch.tensor([M - 1, 0, M // 2, M - 1, 1 % M], device=DEV)
        with torch.no_grad():
            y5 = q(x[five].contiguous(), tuning=t)
        assert torch.equal(y5, y[five]), f"{what}: rows in a 5-row call differ from the same rows of the {M}-row call"


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("case", ROWS_CASES, ids=_ids(ROWS_CASES))
def test_rows_form_forced_every_output(case, dtype):
    _forced_case(case, dtype, _rows_on(), "rows", 16, 64)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("case", PANEL_CASES, ids=_ids(PANEL_CASES))
def test_panel_form_forced_every_output(case, dtype):
    _forced_case(case, dtype, _panel_on(), "panel", 64, 128)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
def test_the_planners_own_choice(dtype):
    """No tuning: a flagged 1024 x 1024 g128 layer whose rows are not resident (released: the whole band) runs the rows form at 5, 16 and 64 rows, a resident
    flagged 1024 x 8192 one at 5 and 16 rows (the measured region of the plain flag) but not at 64, and a 2048 x 2048 one the panel form at 256 rows (panel_pays
    takes its 4-bit twin there: asserted on the host by test_dense_int2_host.py); the unflagged twin of the same tensors keeps the kernel it had.  Both inside
    the bound."""
    for K, N, Ms, kernel, release in ((1024, 1024, (5, 16, 64), "rows", True), (1024, 8192, (5, 16), "rows", False), (2048, 2048, (256,), "panel", False)):
        Lq = _layer(K, N, 128, False, dtype, K + 1)
        q, u = _module(Lq, dtype, release=release), _module(Lq, dtype, flag=False)
        if (K, N) == (1024, 8192):
            assert "body" not in _lib.describe_plan(q._layer, 64)
        for M in Ms:
            plan, old = _lib.describe_plan(q._layer, M), _lib.describe_plan(u._layer, M)
            assert plan["kernel"] == kernel and plan.get("body") == "lowbit", plan
            assert old["kernel"] not in ("rows", "panel") and "body" not in old, old
            x = _x(M, K, dtype, M + 3)
            with torch.no_grad():
                y, y2, yu = q(x), q(x), u(x)
            assert torch.equal(y, y2)
            _within_the_model(q, Lq, x, y, plan, f"planner {kernel} {K}x{N} M={M} {DT_IDS[dtype]}")
            _within_the_model(u, Lq, x, yu, old, f"unflagged {old['kernel']} {K}x{N} M={M} {DT_IDS[dtype]}")


# ---- guard bands ---------------------------------------------------------------------------------------------------------------------------------------
GUARD_CASES = [("rows", ROWS_CASES[2]), ("rows", ROWS_CASES[4]), ("panel", PANEL_CASES[0])]      # a one-row last tile + the last strip group; act-order (workspace); the panel form's one-row tile


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("form,case", GUARD_CASES, ids=[f"{f}-{i}" for (f, c), i in zip(GUARD_CASES, _ids([c for _, c in GUARD_CASES]))])
def test_nothing_outside_the_buffers_is_touched(form, case, dtype):
    """The copy, its constants, x, the bias, out and an exact workspace each sit between guard bands (tests/_guarded.py): the call through the C ABI leaves every
    guard as it was, writes every output, and equals the module call."""
    K, N, gs, M, act, _ = case
    t = _rows_on() if form == "rows" else _panel_on()
    q = _module(_layer(K, N, gs, act, dtype, K + N + M), dtype)
    x = _x(M, K, dtype, M)
    with torch.no_grad():
        y_mod = q(x, tuning=t)
    L = _lib.GptqLayer()
    ctypes.pointer(L)[0] = q._layer
    es = 2
    gw, _ = G.guarded_like(q._qweight_tiled, G.guard_for())
    gc, _ = G.guarded_like(q._qconst_tiled, G.guard_for())
    gb, _ = G.guarded_like(q.bias, G.guard_for())
    gx, _ = G.guarded_like(x, G.guard_for(K * es))
    L.qweight_tiled, L.qconst_tiled, L.bias = gw.ptr, gc.ptr, gb.ptr
    assert _lib.describe_plan(L, M, t).get("body") == "lowbit"
    need = int(_lib.load().gptq_workspace_bytes_ex(ctypes.byref(L), M, ctypes.byref(t)))
    assert (need > 0) == bool(q.act_order)
    ws = G.Guarded(need, max(64 << 10, (need + 255) // 256 * 256), 0x00, G.OUT_GUARD, DEV) if need else None
    go = G.Guarded(M * N * es, G.guard_for(N * es), 0xFF, G.OUT_GUARD, DEV)
    _lib.check(_lib.load().gptq_forward_ex(ctypes.byref(L), gx.ptr, go.ptr, M, ws.ptr if ws else None, need, torch.cuda.current_stream(DEV).cuda_stream, ctypes.byref(t)))
    torch.cuda.synchronize()
    for name, g in (("qweight_tiled", gw), ("qconst_tiled", gc), ("bias", gb), ("x", gx), ("out", go)) + ((("workspace", ws),) if ws else ()):
        g.assert_intact(f"{form} {K}x{N} M={M}: {name}")
    y = go.view(dtype, (M, N))
    assert not bool(y.isnan().any()) and torch.equal(y, y_mod)


# ---- the memory contract, graphs, callers ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
def test_released_layer_needs_no_rebuilt_rows(dtype, monkeypatch):
    """release_checkpoint_layout=True with low_bit_rows=True at 16 rows: the plan reads the copy, so no gptq_unprepack_decode runs in front of the call; the
    output equals, bit for bit, that of the same layer with both layouts resident, and state_dict() is what it was."""
    K = N = 1024
    Lq = _layer(K, N, 128, False, dtype, 77)
    both, rel = _module(Lq, dtype, wide=True), _module(Lq, dtype, release=True)
    assert rel._released and rel.qweight.device.type == "cpu"
    assert _lib.describe_plan(both._layer, 16) == _lib.describe_plan(rel._layer, 16) and _lib.describe_plan(rel._layer, 16)["body"] == "lowbit"
    x = _x(16, K, dtype, 16)
    with torch.no_grad():
        want = both(x)
    lib = _lib.load()
    calls = []
    real = lib.gptq_unprepack_decode
    monkeypatch.setattr(lib, "gptq_unprepack_decode", lambda *a: (calls.append(1), real(*a))[1])
    with torch.no_grad():
        got = rel(x)
    assert rel._rows_need[16] is False and not calls
    assert torch.equal(got, want)
    sd = rel.state_dict()
    for k in ("qweight", "qzeros", "scales", "g_idx", "bias"):
        assert torch.equal(sd[k].cpu(), Lq[k].to(sd[k].dtype)), k
    # without the flag the same released layer rebuilds its rows at 16 rows (what the flag removes)
    plain = _module(Lq, dtype, flag=False, release=True)
    with torch.no_grad():
        plain(x)
    assert plain._rows_need[16] is True and calls


def test_captured_graph_replays_the_eager_bits():
    K = N = 1024
    dtype = torch.float16
    q = _module(_layer(K, N, 128, False, dtype, 78), dtype, wide=True)
    M = 16
    assert _lib.describe_plan(q._layer, M).get("body") == "lowbit"
    xs = [_x(M, K, dtype, 100 + i) for i in range(3)]
    with torch.no_grad():
        eager = [q(x) for x in xs]
    buf = xs[0].clone()
    torch.cuda.synchronize()
    s = torch.cuda.Stream(DEV)
    with torch.cuda.stream(s), torch.no_grad():
        q(buf)                                                # warm-up on the capture stream (whatever it allocates exists before the capture)
        s.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            out = q(buf)
    torch.cuda.synchronize()
    for x, want in zip(xs, eager):
        buf.copy_(x)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, want)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
def test_callers_run_flagged_layers_as_single_calls(dtype):
    """forward_multi of three flagged layers and mlp_forward on flagged gate / up / down at 8 rows: each layer's own low-bit call.  forward_multi: the bits of
    the single calls (which the tests above hold to the oracle).  mlp_forward: the oracle composition down(silu(g) * u) with g, u the single calls' values --
    the bound of the down call on h64 = silu(g) u plus one ulp of h carried through |W_down| (h is rounded to T once; expf and the product are fp32)."""
    K, I, M = 1024, 2048, 8
    Ls = [_layer(K, n, 128, False, dtype, 200 + i) for i, n in enumerate((1024, 2048, 1024))]
    qs = [_module(L, dtype, wide=True) for L in Ls]
    x = _x(M, K, dtype, 9)
    for q in qs:
        assert _lib.describe_plan(q._layer, M).get("body") == "lowbit"
    with torch.no_grad():
        singles = [q(x) for q in qs]
        multi = forward_multi(qs, x)
    for a, b in zip(singles, multi):
        assert torch.equal(a, b)
    Lg, Lu, Ld = _layer(K, I, 128, False, dtype, 210), _layer(K, I, 128, False, dtype, 211), _layer(I, K, 128, False, dtype, 212)
    gate, up, down = _module(Lg, dtype, wide=True), _module(Lu, dtype, wide=True), _module(Ld, dtype, wide=True)
    assert _lib.describe_plan(down._layer, M).get("body") == "lowbit"
    with torch.no_grad():
        g, u = gate(x), up(x)
        y = mlp_forward(gate, up, down, x)
    h64 = F.silu(g.double()) * u.double()
    W64 = EM.w64(Ld, 2, _mode(down), DEV)
    y64 = h64 @ W64 + Ld["bias"].to(DEV).double()
    A = h64.abs() @ EM.abs_weights(Ld, 2, dtype, W64)
    plan = _lib.describe_plan(down._layer, M)
    bnd = EM.bound(y64, A, I, dtype, EM.constant_for(plan, dtype, 128), ((h64, W64),)) + EM.ulp(h64, dtype) @ W64.abs()
    err = (y.double() - y64).abs()
    print(f"mlp_forward {DT_IDS[dtype]}: worst err / bound = {float((err / bnd).max()):.3f}")
    assert bool((err <= bnd).all()), float((err / bnd).max())
