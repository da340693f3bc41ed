"""GPU (-m gpu): every kernel stays inside the buffers it is handed.

The other GPU tests check VALUES through the module path, where every output is a fresh torch.empty, x lives in the caching allocator's segment and the
workspace is never smaller than 1 MiB.  Here every call goes through the C ABI with x / dy / u / routing, the outputs and the workspace in guard-band buffers
(tests/_guarded.py): one allocation [low guard | body | high guard], the body exactly as large as the header (include/gptq_mi355x.h) or the matching
*_workspace_bytes* query says, output bodies pre-filled with 0xFF (an unwritten element is a NaN), input guards 0xFF (NaN / -1), workspace bodies zeroed.

Every case
  1. runs the call TWICE on the same guarded workspace (the second launch sees the non-zero second half of the header),
  2. asserts that all guards are intact,
  3. asserts that both outputs are bit-identical (torch.equal) to the ordinary module call on the same inputs.
The parity tests own the correctness of the module path; this file owns the claim that the module path does not depend on slack.  No tolerance anywhere.
Dense single-layer cases run once more with one x row (the last: the last row of a partial tile where there is one) set to NaN: every other output row must
keep its bits -- leakage across rows in the LDS meet / the K-slice combines -- and the guards stay intact.

A damaged guard is a finding, not a GPU fault: the guards are sized (max(64 KiB, 128 rows); a workspace: max(64 KiB, its own size)) so that a whole stray tile
lands in memory the test owns.  The report names the side, the first / last damaged body-relative byte offset and the count."""
import collections
import ctypes
import itertools

import pytest
import torch

import _guarded as G
import test_gpu_panel as TP
import test_gpu_rows as TR
import test_gpu_tiled as TT
import test_gpu_wide_sk as TW
from autogptq_amd import _lib
from autogptq_amd.qlinear_mi355x import QuantLinear, forward_multi, mlp_forward
from oracle import gptq_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DT_IDS = {torch.float16: "fp16", torch.bfloat16: "bf16", torch.float32: "fp32"}
MFMA_GEMMS_ON_CHECKPOINT_ROWS = {"tiled", "skinny64", "strip16", "mid", "stream64", "wide"}
RAN = collections.defaultdict(list)          # class key -> labels of the dense cases that ran it (the closing test reads this)


def _stream():
    return torch.cuda.current_stream(DEV).cuda_stream


def _es(dtype):
    return torch.tensor([], dtype=dtype).element_size()


def _copy_struct(L):
    c = _lib.GptqLayer()
    ctypes.pointer(c)[0] = L
    return c


def _rand(M, K, dtype, seed):
    return (torch.rand(M, K, generator=torch.Generator().manual_seed(seed)) - 0.5).to(dtype).to(DEV)


def _out(rows, cols, dtype):
    es = _es(dtype)
    return G.Guarded(rows * cols * es, G.guard_for(cols * es), 0xFF, G.OUT_GUARD, DEV)


def _workspace(need):
    """An exact, zeroed workspace inside guards of max(64 KiB, its own size); None when the call needs none."""
    return G.Guarded(need, max(64 << 10, (need + 255) // 256 * 256), 0x00, G.OUT_GUARD, DEV) if need else None


def _class_key(d):
    """(kernel, K slices, pair form, act-order x staged in the workspace, epilogue) of a gptq_describe_plan answer."""
    staged = (d["path"] == "gemm" and d["perm"] == 1) or d["perm"] == 2
    return (d["kernel"], int(d["ksplit"]) > 1, int(d.get("pair", 0)), bool(staged), d["epilogue"])


def _make(K, N, bits, gs, act, dtype, seed, copy=True, bias=True, epilogue="none", zero_mode="auto"):
    Lq = O.random_quant_layer(K, N, bits, gs, act_order=act, seed=seed, bias=bias, dtype=dtype)
    q = QuantLinear(bits, gs, K, N, bias, weight_dtype=dtype, zero_mode=zero_mode, epilogue=epilogue)
    q.qweight, q.qzeros, q.scales, q.g_idx = Lq["qweight"], Lq["qzeros"], Lq["scales"], Lq["g_idx"]
    if bias:
        q.bias = Lq["bias"]
    q = q.to(DEV)
    q.post_init(tiled=copy)
    return q


# ====================================================================================================================== dense, single layer
def _dense_call(L, x_ptr, M, n_out, dtype, ws, need, tref):
    go = _out(M, n_out, dtype)
    _lib.check(_lib.load().gptq_forward_ex(ctypes.byref(L), x_ptr, go.ptr, M, ws.ptr if ws else None, need, _stream(), tref))
    return go


def _dense_case(q, M, tuning=None, what="", layer=None, expect=None):
    """The three steps of the module docstring + the poisoned row, for gptq_forward_ex on (q, M, tuning).  ``layer``: a struct to call with instead of a
    copy of the module's (the decode-copy test points qweight_tiled / qconst_tiled at guarded bodies).  Returns the plan's class key."""
    lib = _lib.load()
    K, n_out, dtype = q.infeatures, q._n_out, q._w_dtype
    L = layer if layer is not None else _copy_struct(q._layer)
    tref = ctypes.byref(tuning) if tuning is not None else None
    plan = _lib.describe_plan(L, M, tuning)
    key = _class_key(plan)
    if expect is not None:
        assert key == expect, f"{what}: the planner answers {key} for the real layer, {expect} on the host grid ({plan})"
    what = f"{what} M={M} {plan['kernel']} ksplit={plan['ksplit']}"
    need = int(lib.gptq_workspace_bytes_ex(ctypes.byref(L), M, tref))
    x = _rand(M, K, dtype, M + K)
    gx, xv = G.guarded_like(x, G.guard_for(K * _es(dtype)))
    ws = _workspace(need)
    with torch.no_grad():
        y_mod = q(x, tuning=tuning)
    assert y_mod.shape == (M, n_out)
    outs = [_dense_call(L, gx.ptr, M, n_out, dtype, ws, need, tref) for _ in range(2)]
    gx.assert_intact(f"{what}: x")
    if ws:
        ws.assert_intact(f"{what}: workspace ({need} bytes = gptq_workspace_bytes_ex)")
    for i, go in enumerate(outs):
        go.assert_intact(f"{what}: out (launch {i + 1})")
        y = go.view(dtype, (M, n_out))
        assert not bool(y.isnan().any()), f"{what}: launch {i + 1} left {int(y.isnan().sum())} output elements unwritten (or NaN)"
        assert torch.equal(y, y_mod), f"{what}: launch {i + 1} on exact buffers differs from the module call in {int((y != y_mod).sum())} outputs"
    # one poisoned row: the last one
    r = M - 1
    xv[r] = float("nan")
    gp = _dense_call(L, gx.ptr, M, n_out, dtype, ws, need, tref)
    yp = gp.view(dtype, (M, n_out))
    gx.assert_intact(f"{what}: x (poisoned row)")
    gp.assert_intact(f"{what}: out (poisoned row)")
    if ws:
        ws.assert_intact(f"{what}: workspace (poisoned row)")
    assert torch.equal(yp[:r], y_mod[:r]), f"{what}: a NaN in x row {r} changed {int((yp[:r] != y_mod[:r]).any(dim=1).sum())} other output rows"
    assert bool(yp[r].isnan().all()), f"{what}: x row {r} is NaN but {int((~yp[r].isnan()).sum())} of its outputs are not"
    RAN[key].append(what)
    return key


# ---------------------------------------------------------------------------------------------------------------------- the forced tables
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("case", TR.CASES, ids=[f"{c[0]}x{c[1]}g{c[2]}M{c[3]}{'act' if c[4] else ''}" for c in TR.CASES])
def test_rows_table(case, dtype):
    K, N, gs, M, act, _ = case
    q = _make(K, N, 4, gs, act, dtype, K + N + M)
    for rb, s in TR._geoms(4):
        key = _dense_case(q, M, TR._tune(rb, s), f"rows RB={rb} S={s} {K}x{N} g{gs} act={act} {DT_IDS[dtype]}")
        assert key[0] == "rows"


@pytest.mark.parametrize("bits,gs", [(3, 32), (8, 64)])
def test_rows_table_3_and_8_bit(bits, gs):
    K, N, _, M, act, _ = TR.CASES[1]                      # 10 strips: the last strip group runs past N; two row tiles for RB = 1
    q = _make(K, N, bits, gs, act, torch.float16, K + N + bits)
    for rb, s in TR._geoms(bits):
        assert _dense_case(q, M, TR._tune(rb, s), f"rows int{bits} RB={rb} S={s} {K}x{N} g{gs}")[0] == "rows"


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("case", TP.CASES, ids=[f"{c[0]}x{c[1]}g{c[2]}M{c[3]}{'act' if c[4] else ''}" for c in TP.CASES])
def test_panel_table(case, dtype):
    K, N, gs, M, act, _ = case
    q = _make(K, N, 4, gs, act, dtype, K + N + M)
    for geom in TP.GEOMS:
        assert _dense_case(q, M, TP._tune(geom), f"panel geom {geom} {K}x{N} g{gs} act={act} {DT_IDS[dtype]}")[0] == "panel"


@pytest.mark.parametrize("case", TP.CASES_B38[:6], ids=[f"int{c[0]}_{c[1]}x{c[2]}g{c[3]}M{c[4]}{'act' if c[5] else ''}" for c in TP.CASES_B38[:6]])
def test_panel_table_3_and_8_bit(case):
    bits, K, N, gs, M, act, _ = case
    q = _make(K, N, bits, gs, act, torch.float16, K + N + M + bits)
    for geom in (TP.GEOMS[:3] if bits == 8 else TP.GEOMS):
        assert _dense_case(q, M, TP._tune(geom), f"panel int{bits} geom {geom} {K}x{N} g{gs} act={act}")[0] == "panel"


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("case", TW.CASES, ids=[f"{c[0]}x{c[1]}g{c[2]}M{c[3]}{'act' if c[4] else ''}" for c in TW.CASES])
def test_wide_sk_table(case, dtype):
    K, N, gs, M, act, _ = case
    q = _make(K, N, 4, gs, act, dtype, K + N + M)
    assert _dense_case(q, M, TW._tune(TW.WIDE_SK_ON), f"wide_sk {K}x{N} g{gs} act={act} {DT_IDS[dtype]}")[0] == "wide_sk"


@pytest.mark.parametrize("case", [c for c in TW.CASES_B38 if c[4] < 1000], ids=lambda c: f"int{c[0]}_{c[1]}x{c[2]}g{c[3]}M{c[4]}{'act' if c[5] else ''}")
def test_wide_sk_table_3_and_8_bit(case):
    bits, K, N, gs, M, act, _ = case
    q = _make(K, N, bits, gs, act, torch.float16, K + N + M)
    assert _dense_case(q, M, TW._tune(TW.WIDE_SK_ON), f"wide_sk int{bits} {K}x{N} g{gs} act={act}")[0] == "wide_sk"


TT_LEAN = [(4, 2), (4, 4), (8, 2), (8, 4), (16, 2)]          # (waves, chunks in flight) of test_gpu_tiled_tail.py
TT_GENERIC = [(2, 4), (3, 4), (1, 2)]
RAGGED_K = [(4160, 96, 32), (1056, 64, 1056)]          # test_gpu_tiled_tail.py: K is no whole number of chunks -- the decode copy has padding


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("K,N,gs", RAGGED_K, ids=["ragged-k", "ragged-k-one-group"])
def test_decode_tail_ragged_k_table(K, N, gs, dtype):
    """The decode-copy kernel on ragged K: every straight-line arm, the run-time loops, and K slices (the granules of the cold block) forced."""
    q = _make(K, N, 4, gs, False, dtype, K + N)
    sliced = 0
    for waves, u, ks in [(w, u, 0) for w, u in TT_LEAN + TT_GENERIC] + [(8, 4, 4), (4, 4, 3), (16, 2, 2), (2, 4, 2)]:
        t = TT._tune(waves, u, ks)
        for M in (1, 2, 3, 4):
            key = _dense_case(q, M, t, f"strips waves={waves} u={u} ks={ks} {K}x{N} g{gs} {DT_IDS[dtype]}")
            assert key[0] == "strips"
            sliced += key[1]
    assert sliced, "no forced K-slice geometry was taken with K slices"


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
def test_decode_tail_pair_form_ragged_k(dtype):
    """[gate | up] with the SiLU * mul epilogue of the decode-copy kernel on ragged K (2112 = 16.5 chunks), 22 strips per half."""
    q = _make(2112, 704, 4, 64, False, dtype, 7, epilogue="silu_mul")
    for t in (None, TT._tune(16, 2), TT._tune(8, 4), TT._tune(4, 4), TT._tune(2, 2)):
        for M in (1, 2, 3, 4):
            key = _dense_case(q, M, t, f"pair form {DT_IDS[dtype]} tuning={'default' if t is None else (t.waves, t.reserved[_lib.LAB.DEPTH])}")
            assert key[0] == "strips" and key[2] == 1 and key[4] == "fused", key


# ---------------------------------------------------------------------------------------------------------------------- default plans on a host-built grid
GRID_K = (96, 160, 256, 1056, 2112)
GRID_N = (32, 96, 544, 1056, 2048)
GRID_BITS = (4, 8, 3, 2)
GRID_GROUPS = (32, 128, 0)                                # 0: one group over the whole K
GRID_DTYPES = (torch.float16, torch.bfloat16, torch.float32)
GRID_M = (1, 3, 4, 5, 8, 9, 17, 33, 65, 129, 300, 767, 1024)
RAGGED_N = (96, 544, 1056)
_FAKE = 0x10000                                           # gptq_describe_plan dereferences nothing but the struct


def _fake_layer(K, N, bits, gs, act, copy, dtype, epi=0):
    L = _lib.GptqLayer()
    L.epilogue = _lib.EPI_SILU_MUL if epi else _lib.EPI_NONE
    L.qweight = L.qzeros = L.scales = L.bias = _FAKE
    L.K, L.N, L.bits, L.group_size = K, N, bits, gs
    L.dtype = _lib.DTYPE_ENUM[dtype]
    L.zero_mode = _lib.ZERO_NOWRAP if (act or bits == 3) else _lib.ZERO_WRAP
    if act:
        L.g_idx = L.qweight_seq = L.perm = _FAKE
    if copy:
        tb, cb = ctypes.c_size_t(0), ctypes.c_size_t(0)
        if _lib.load().gptq_prepack_decode_bytes(ctypes.byref(L), ctypes.byref(tb), ctypes.byref(cb)) != 0:
            return None                                   # no decode copy for this layer: the same layer as copy = False
        L.qweight_tiled = L.qconst_tiled = _FAKE
        L.tiled_cols = _lib.STRIP_COLS
    return L


def _build_grid():
    """{class key: sorted members} of the planner's answers over the grid.  A member = (K N, M, K, N, bits order, group_size, act, copy, dtype order, epilogue).
    The issue's grid has plain layers only; the layers whose N splits into [gate | up] halves of whole 32-column blocks (N = 2048) are planned a second time
    with the SiLU * mul epilogue -- fused into the kernel or staged in the workspace in front of the inner call's body, a workspace bug area before
    (test_gpu_parity.py: test_unfused_epilogue_inner_k_split_uses_the_real_ticket_header)."""
    classes = collections.defaultdict(list)
    for K, N, (bi, bits), g, act, copy, (di, dtype), epi in itertools.product(GRID_K, GRID_N, enumerate(GRID_BITS), GRID_GROUPS, (False, True), (False, True),
                                                                           enumerate(GRID_DTYPES), (0, 1)):
        gs = g or K
        if act and gs >= K:                               # a shuffled g_idx of ONE group is the default order
            continue
        if epi and N % 64:
            continue
        L = _fake_layer(K, N, bits, gs, act, copy, dtype, epi)
        if L is None:
            continue
        for M in GRID_M:
            classes[_class_key(_lib.describe_plan(L, M))].append((K * N, M, K, N, bi, gs, act, copy, di, epi))
    for v in classes.values():
        v.sort()
    return classes


def _select(classes):
    """Per class: its smallest member (by K N, then M), the smallest member with a ragged N and a partial last row tile where the class has one, and -- an
    addition to the issue's rule, the kernels being instantiated per bit width -- the smallest member of every bit width the class holds."""
    picked = {}
    for key, members in classes.items():
        chosen = [members[0]]
        ragged = [m for m in members if m[3] in RAGGED_N and m[1] not in (1, 4, 8, 1024)]
        if ragged:
            chosen.append(ragged[0])
        for bi in range(len(GRID_BITS)):
            of_bits = [m for m in members if m[4] == bi]
            if of_bits:
                chosen.append(of_bits[0])
        for m in dict.fromkeys(chosen):
            picked.setdefault(m, key)
    return picked


GRID_CLASSES = _build_grid()
GRID_PICKED = _select(GRID_CLASSES)
_GRID_LAYERS = collections.defaultdict(list)              # one module per layer, its row counts in one test
for _m, _key in sorted(GRID_PICKED.items()):
    _GRID_LAYERS[_m[2:]].append((_m[1], _key))


def _grid_id(lay):
    K, N, bi, gs, act, copy, di, epi = lay
    return f"{K}x{N}_int{GRID_BITS[bi]}_g{gs}_{'act' if act else 'seq'}_{'copy' if copy else 'rows'}_{DT_IDS[GRID_DTYPES[di]]}{'_silu_mul' if epi else ''}"


@pytest.mark.parametrize("lay", sorted(_GRID_LAYERS), ids=_grid_id)
def test_default_plan_grid(lay):
    K, N, bi, gs, act, copy, di, epi = lay
    q = _make(K, N, GRID_BITS[bi], gs, act, GRID_DTYPES[di], K + N + bi + di, copy=copy, epilogue="silu_mul" if epi else "none")
    assert (q._qweight_tiled is not None) == copy
    for M, key in _GRID_LAYERS[lay]:
        _dense_case(q, M, None, f"default plan {_grid_id(lay)}", expect=key)


# ====================================================================================================================== forward_multi / mlp_forward
def _multi_case(qs, M, what):
    lib = _lib.load()
    n, K, dtype = len(qs), qs[0].infeatures, qs[0]._w_dtype
    x = _rand(M, K, dtype, M)
    with torch.no_grad():
        ys_mod = forward_multi(qs, x)                     # (first: the group's act-order layers are pointed at ONE perm here)
    arr = (ctypes.POINTER(_lib.GptqLayer) * n)(*[ctypes.pointer(q._layer) for q in qs])
    need = int(lib.gptq_workspace_bytes_multi(arr, n, M))
    gx, _ = G.guarded_like(x, G.guard_for(K * _es(dtype)))
    ws = _workspace(need)
    for launch in (1, 2):
        gos = [_out(M, q._n_out, dtype) for q in qs]
        optrs = (ctypes.c_void_p * n)(*[g.ptr for g in gos])
        _lib.check(lib.gptq_forward_multi(arr, n, gx.ptr, optrs, M, ws.ptr if ws else None, need, _stream()))
        gx.assert_intact(f"{what}: x")
        if ws:
            ws.assert_intact(f"{what}: workspace ({need} bytes = gptq_workspace_bytes_multi)")
        for i, (go, q, ym) in enumerate(zip(gos, qs, ys_mod)):
            go.assert_intact(f"{what}: outs[{i}] (launch {launch})")
            y = go.view(dtype, (M, q._n_out))
            assert torch.equal(y, ym), f"{what}: outs[{i}] of launch {launch} on exact buffers differs from forward_multi in {int((y != ym).sum())} outputs"


MULTI_M = (1, 4, 5, 40, 130)
MULTI_SETS = [
    # (bits, K, group_size, act, widths, copy)
    (4, 2048, 128, False, (512, 288, 64), True),          # the widths of test_gpu_tiled_tail.py: the layer selector per workgroup
    (4, 2048, 128, False, (512, 288), False),             # checkpoint rows only: the streamed / 17..128-row multi-layer kernels
    (4, 1056, 32, True, (512, 288, 64, 96), True),        # ragged K, act-order of ONE activation order: one permuted x for the group
    (8, 1056, 32, False, (288, 512), True),
    (3, 2112, 64, True, (64, 544, 96), True),
]


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("mset", MULTI_SETS, ids=[f"int{s[0]}_{s[1]}_g{s[2]}_{'act' if s[3] else 'seq'}_{'x'.join(map(str, s[4]))}_{'copy' if s[5] else 'rows'}" for s in MULTI_SETS])
def test_forward_multi(mset, dtype):
    bits, K, gs, act, widths, copy = mset
    qs, g0 = [], None
    for i, N in enumerate(widths):
        Lq = O.random_quant_layer(K, N, bits, gs, act_order=act, seed=11 * N + i + bits, bias=(i != 1), dtype=dtype)
        if act:
            g0 = Lq["g_idx"] if g0 is None else g0
            Lq["g_idx"] = g0.clone()                      # one activation order for the group, as GPTQ produces q / k / v
        q = QuantLinear(bits, gs, K, N, i != 1, weight_dtype=dtype)
        q.qweight, q.qzeros, q.scales, q.g_idx = Lq["qweight"], Lq["qzeros"], Lq["scales"], Lq["g_idx"]
        if i != 1:
            q.bias = Lq["bias"]
        q = q.to(DEV)
        q.post_init(tiled=copy)
        qs.append(q)
    for M in MULTI_M:
        _multi_case(qs, M, f"forward_multi int{bits} K={K} g{gs} act={act} widths={widths} copy={copy} {DT_IDS[dtype]} M={M}")


MLP_SETS = [(4, 512, 1056, 288, 32, False), (4, 512, 1056, 288, 32, True), (8, 256, 544, 96, 64, False), (3, 1056, 544, 160, 32, True)]


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("mset", MLP_SETS, ids=[f"int{s[0]}_{s[1]}_{s[2]}_{s[3]}_g{s[4]}_{'act' if s[5] else 'seq'}" for s in MLP_SETS])
def test_mlp_forward(mset, dtype):
    """gptq_mlp_forward with its two staging rows, the inner calls' bodies and (act-order down) the permuted h in an exact workspace."""
    bits, K, I, N, gs, act = mset
    lib = _lib.load()
    gate, up, down = _make(K, I, bits, gs, act, dtype, 1, bias=False), _make(K, I, bits, gs, act, dtype, 2, bias=False), _make(I, N, bits, gs, act, dtype, 3)
    if act:
        up.g_idx = gate.g_idx.clone()                     # gate / up of a checkpoint share their activation order
        up.post_init()
    for M in MULTI_M:
        what = f"mlp_forward int{bits} {K}->{I}->{N} g{gs} act={act} {DT_IDS[dtype]} M={M}"
        x = _rand(M, K, dtype, M)
        with torch.no_grad():
            y_mod = mlp_forward(gate, up, down, x)
        need = int(lib.gptq_workspace_bytes_mlp(gate._layer_ref, up._layer_ref, down._layer_ref, M))
        assert need > 0
        gx, _ = G.guarded_like(x, G.guard_for(K * _es(dtype)))
        ws = _workspace(need)
        for launch in (1, 2):
            go = _out(M, N, dtype)
            _lib.check(lib.gptq_mlp_forward(gate._layer_ref, up._layer_ref, down._layer_ref, gx.ptr, go.ptr, M, ws.ptr, need, _stream()))
            gx.assert_intact(f"{what}: x")
            ws.assert_intact(f"{what}: workspace ({need} bytes = gptq_workspace_bytes_mlp)")
            go.assert_intact(f"{what}: out (launch {launch})")
            y = go.view(dtype, (M, N))
            assert torch.equal(y, y_mod), f"{what}: launch {launch} on exact buffers differs from mlp_forward in {int((y != y_mod).sum())} outputs"


# ====================================================================================================================== the decode copy
DECODE_K = (96, 160, 1056, 4160)                          # no whole number of chunks (128 k; 8 bits: 64 k, where 160 and 1056 are ragged too): the copy has padding


@pytest.mark.parametrize("act", [False, True], ids=["seq", "act"])
@pytest.mark.parametrize("bits", [2, 3, 4, 8])
@pytest.mark.parametrize("K", DECODE_K)
def test_decode_copy_is_fully_written_and_its_kernels_stay_inside(K, bits, act):
    """WHICH OF THE TWO HOLDS: gptq_prepack_decode writes EVERY byte of both buffers (k past K are stored as 0, every record byte is a scale or a zero-point):
    the copies built over a 0x00 and over a 0xFF body are byte-identical, so no result can depend on what the allocator handed post_init.  The forwards at
    1..4 rows then run FROM the guarded copy (exact gptq_prepack_decode_bytes sizes: a read past its end that reached a result would differ from the module's
    call on its own copy), gptq_unprepack_decode rebuilds the packed rows bit for bit into an exact buffer, and gptq_permute_columns / gptq_dequant write
    exactly their outputs."""
    lib = _lib.load()
    N, gs, dtype = 96, 32, torch.float16
    q = _make(K, N, bits, gs, act, dtype, K + bits)
    assert q._qweight_tiled is not None and q.act_order == act
    L = _copy_struct(q._layer)
    tb, cb = ctypes.c_size_t(0), ctypes.c_size_t(0)
    _lib.check(lib.gptq_prepack_decode_bytes(ctypes.byref(L), ctypes.byref(tb), ctypes.byref(cb)))
    assert (tb.value, cb.value) == (q._qweight_tiled.numel(), q._qconst_tiled.numel())
    what = f"int{bits} {K}x{N} g{gs} act={act}"
    copies = []
    for fill in (0x00, 0xFF):
        gt = G.Guarded(tb.value, max(64 << 10, tb.value), fill, G.OUT_GUARD, DEV)
        gc = G.Guarded(cb.value, max(64 << 10, cb.value), fill, G.OUT_GUARD, DEV)
        _lib.check(lib.gptq_prepack_decode(ctypes.byref(L), gt.ptr, gc.ptr, _stream()))
        gt.assert_intact(f"{what}: qweight_tiled_out (body pre-filled with {fill:#x})")
        gc.assert_intact(f"{what}: qconst_tiled_out (body pre-filled with {fill:#x})")
        copies.append((gt, gc))
    (t0, c0), (t1, c1) = copies
    assert torch.equal(t0.body, t1.body), f"{what}: gptq_prepack_decode leaves {int((t0.body != t1.body).sum())} bytes of qweight_tiled unwritten"
    assert torch.equal(c0.body, c1.body), f"{what}: gptq_prepack_decode leaves {int((c0.body != c1.body).sum())} bytes of qconst_tiled unwritten"
    assert torch.equal(t0.body, q._qweight_tiled) and torch.equal(c0.body, q._qconst_tiled)
    # the forwards from the guarded copy (the 0xFF one: whatever lies behind it is 0xA5, not zero)
    L.qweight_tiled, L.qconst_tiled = t1.ptr, c1.ptr
    for M in (1, 2, 3, 4):
        key = _dense_case(q, M, None, f"decode copy in guards {what}", layer=L)
        assert key[0] == "strips", key
    t1.assert_intact(f"{what}: qweight_tiled after the forwards")
    c1.assert_intact(f"{what}: qconst_tiled after the forwards")
    # the inverse: released layers call it before every row-reading launch
    rows = q._layer.qweight_seq or q._layer.qweight
    src = next(t for t in q._keepalive if t is not None and t.data_ptr() == rows)
    gq = G.Guarded(src.numel() * 4, G.guard_for(N * 4), 0xFF, G.OUT_GUARD, DEV)
    _lib.check(lib.gptq_unprepack_decode(t1.ptr, K, N, bits, gq.ptr, _stream()))
    gq.assert_intact(f"{what}: gptq_unprepack_decode qweight_out")
    assert torch.equal(gq.view(torch.int32, tuple(src.shape)), src), f"{what}: gptq_unprepack_decode does not reproduce the packed rows"
    # gptq_dequant / gptq_permute_columns into exact outputs
    gw = _out(K, N, dtype)
    _lib.check(lib.gptq_dequant(ctypes.byref(L), gw.ptr, _stream()))
    gw.assert_intact(f"{what}: gptq_dequant W_out")
    assert torch.equal(gw.view(dtype, (K, N)), q.dequantize())
    perm = torch.randperm(K, generator=torch.Generator().manual_seed(K)).to(torch.int32).to(DEV)
    for dt in (torch.float16, torch.float32):
        for M in (1, 5, 129):
            x = _rand(M, K, dt, M)
            gx, _ = G.guarded_like(x, G.guard_for(K * _es(dt)))
            gp = _out(M, K, dt)
            _lib.check(lib.gptq_permute_columns(gx.ptr, perm.data_ptr(), M, K, _lib.DTYPE_ENUM[dt], gp.ptr, _stream()))
            gx.assert_intact(f"{what}: gptq_permute_columns x")
            gp.assert_intact(f"{what}: gptq_permute_columns x_out M={M} {dt}")
            assert torch.equal(gp.view(dt, (M, K)), x[:, perm.long()])


# ====================================================================================================================== gptq_grad_input
@pytest.mark.parametrize("act", [False, True], ids=["seq", "act"])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16, torch.float32], ids=["fp16", "bf16", "fp32"])
@pytest.mark.parametrize("bits", [2, 3, 4, 8])
@pytest.mark.parametrize("K,N", [(160, 96), (1056, 544)])
def test_grad_input(K, N, bits, dtype, act):
    lib = _lib.load()
    q = _make(K, N, bits, 32, act, dtype, K + N + bits, bias=False)
    es = _es(dtype)
    for M in (1, 63, 65, 129):
        dy = _rand(M, N, dtype, M)
        dx0 = _rand(M, K, dtype, M + 1)
        for acc in (0, 1):
            what = f"grad_input int{bits} {K}x{N} act={act} {DT_IDS[dtype]} M={M} accumulate={acc}"
            ref = q.grad_input(dy, dx0.clone() if acc else None)
            gdy, _ = G.guarded_like(dy, G.guard_for(N * es))
            for launch in (1, 2):
                gdx = _out(M, K, dtype)
                if acc:
                    gdx.view(dtype, (M, K)).copy_(dx0)
                _lib.check(lib.gptq_grad_input(q._layer_ref, gdy.ptr, gdx.ptr, M, acc, _stream()))
                gdy.assert_intact(f"{what}: dy")
                gdx.assert_intact(f"{what}: dx (launch {launch})")
                dx = gdx.view(dtype, (M, K))
                assert torch.equal(dx, ref), f"{what}: differs from QuantLinear.grad_input in {int((dx != ref).sum())} elements"


# ====================================================================================================================== LoRA
def _lora_structs(K, widths, ranks, dtype, seed):
    gen = torch.Generator().manual_seed(seed)
    keep, structs = [], []
    for N, r in zip(widths, ranks):
        A = (torch.randn(r, K, generator=gen) * 0.05).to(dtype).to(DEV)
        B = (torch.randn(N, r, generator=gen) * 0.05).to(dtype).to(DEV)
        L = _lib.GptqLora()
        L.A, L.B, L.K, L.N, L.r, L.dtype, L.scale = A.data_ptr(), B.data_ptr(), K, N, r, _lib.DTYPE_ENUM[dtype], 2.0
        keep.append((A, B))
        structs.append(L)
    arr = (ctypes.POINTER(_lib.GptqLora) * len(structs))(*[ctypes.pointer(s) for s in structs])
    return arr, structs, keep


def _ptrs(items):
    return (ctypes.c_void_p * len(items))(*[i.ptr if isinstance(i, G.Guarded) else i.data_ptr() for i in items])


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("n", [1, 4])
@pytest.mark.parametrize("r", [8, 64])
@pytest.mark.parametrize("K,N", [(96, 16), (1056, 1056)])
def test_lora_entries(K, N, r, n, dtype):
    """gptq_lora_down / _up / _apply with u_i and out_i in guards.  The ordinary call is the one lora.py makes: the same entry on fresh torch tensors.  The
    8-byte read-modify-write of lora_up must not touch the guard next to the last row (N = 16: one 32-byte row)."""
    lib = _lib.load()
    widths = [N, 16, N, 32][:n]
    ranks = [r, 72 - r, 16, r][:n]
    arr, structs, keep = _lora_structs(K, widths, ranks, dtype, K + N + r + n)
    es = _es(dtype)
    for M in (1, 8, 9, 17):
        what = f"lora K={K} widths={widths} ranks={ranks} {DT_IDS[dtype]} M={M}"
        x = _rand(M, K, dtype, M)
        y0 = [_rand(M, w, dtype, M + w + i) for i, w in enumerate(widths)]
        # the ordinary calls
        u_ref = [torch.empty((M, rk), dtype=dtype, device=DEV) for rk in ranks]
        _lib.check(lib.gptq_lora_down(arr, n, x.data_ptr(), _ptrs(u_ref), M, _stream()))
        y_ref = [y.clone() for y in y0]
        _lib.check(lib.gptq_lora_up(arr, n, _ptrs(u_ref), _ptrs(y_ref), M, _stream()))
        ua_ref = [torch.empty((M, rk), dtype=dtype, device=DEV) for rk in ranks]
        ya_ref = [y.clone() for y in y0]
        _lib.check(lib.gptq_lora_apply(arr, n, x.data_ptr(), _ptrs(ua_ref), _ptrs(ya_ref), M, _stream()))
        for a, b in zip(ya_ref + ua_ref, y_ref + u_ref):
            assert torch.equal(a, b), f"{what}: apply is not down + up"
        gx, _ = G.guarded_like(x, G.guard_for(K * es))
        for launch in (1, 2):
            # down: u_i are outputs
            gus = [_out(M, rk, dtype) for rk in ranks]
            _lib.check(lib.gptq_lora_down(arr, n, gx.ptr, _ptrs(gus), M, _stream()))
            # up: u_i are inputs (NaN guards), out_i read-modify-write
            gui = [G.guarded_like(u, G.guard_for(rk * es))[0] for u, rk in zip(u_ref, ranks)]
            gys = [_out(M, w, dtype) for w in widths]
            for g, y, w in zip(gys, y0, widths):
                g.view(dtype, (M, w)).copy_(y)
            _lib.check(lib.gptq_lora_up(arr, n, _ptrs(gui), _ptrs(gys), M, _stream()))
            # apply: both
            gua = [_out(M, rk, dtype) for rk in ranks]
            gya = [_out(M, w, dtype) for w in widths]
            for g, y, w in zip(gya, y0, widths):
                g.view(dtype, (M, w)).copy_(y)
            _lib.check(lib.gptq_lora_apply(arr, n, gx.ptr, _ptrs(gua), _ptrs(gya), M, _stream()))
            gx.assert_intact(f"{what}: x")
            for i in range(n):
                gus[i].assert_intact(f"{what}: down u[{i}] (launch {launch})")
                gui[i].assert_intact(f"{what}: up u[{i}]")
                gys[i].assert_intact(f"{what}: up outs[{i}] (launch {launch})")
                gua[i].assert_intact(f"{what}: apply u[{i}] (launch {launch})")
                gya[i].assert_intact(f"{what}: apply outs[{i}] (launch {launch})")
                assert torch.equal(gus[i].view(dtype, (M, ranks[i])), u_ref[i]), f"{what}: down u[{i}]"
                assert torch.equal(gys[i].view(dtype, (M, widths[i])), y_ref[i]), f"{what}: up outs[{i}]"
                assert torch.equal(gua[i].view(dtype, (M, ranks[i])), u_ref[i]), f"{what}: apply u[{i}]"
                assert torch.equal(gya[i].view(dtype, (M, widths[i])), y_ref[i]), f"{what}: apply outs[{i}]"


def test_lora_module_path_is_the_guarded_call():
    """The LoraQuantLinear path (base output from QuantLinear, u from torch.empty) against gptq_lora_apply on guarded u / out, 1056 -> 1056."""
    from autogptq_amd.lora import LoraQuantLinear
    lib = _lib.load()
    dtype, K, N, r = torch.float16, 1056, 1056, 64
    base = _make(K, N, 4, 32, False, dtype, 5)
    lq = LoraQuantLinear(base, r, 2 * r, adapter_dtype=dtype).to(DEV)
    with torch.no_grad():
        lq.lora_B.weight.copy_((torch.randn(N, r, generator=torch.Generator().manual_seed(1)) * 0.05).to(dtype))
    A16, B16 = lq._kernel_weights(dtype)
    L = _lib.GptqLora()
    L.A, L.B, L.K, L.N, L.r, L.dtype, L.scale = A16.data_ptr(), B16.data_ptr(), K, N, r, _lib.DTYPE_ENUM[dtype], float(lq.scaling)
    arr = (ctypes.POINTER(_lib.GptqLora) * 1)(ctypes.pointer(L))
    for M in (1, 8, 9, 17):
        x = _rand(M, K, dtype, M)
        with torch.no_grad():
            y_mod, y_base = lq(x), base(x)
        gx, _ = G.guarded_like(x, G.guard_for(K * 2))
        gu, gy = _out(M, r, dtype), _out(M, N, dtype)
        gy.view(dtype, (M, N)).copy_(y_base)
        _lib.check(lib.gptq_lora_apply(arr, 1, gx.ptr, _ptrs([gu]), _ptrs([gy]), M, _stream()))
        for g, nm in ((gx, "x"), (gu, "u"), (gy, "out")):
            g.assert_intact(f"LoraQuantLinear M={M}: {nm}")
        assert torch.equal(gy.view(dtype, (M, N)), y_mod)


# ====================================================================================================================== the three MoE entries
MOE_E, MOE_TOPK, MOE_H, MOE_I = 8, 2, 256, 512


def _moe_routings(T, seed):
    """(name, topk_idx, topk_w): a random routing, one with indices E and -1 (dropped), and at 70 tokens one that sends every token to ONE expert (tiles 64 + 6)."""
    from test_gpu_moe import _routing
    idx, w = _routing(T, MOE_E, MOE_TOPK, seed)
    out = [("random", idx, w)]
    edge = idx.clone()
    edge[::3, 0] = MOE_E
    edge[1::4, 1] = -1
    if T >= 8:
        edge[7] = torch.tensor([MOE_E, -1], device=DEV)   # a token with no valid expert gets 0
    out.append(("E-and-minus-1", edge, w))
    if T == 70:
        one = torch.full((T, MOE_TOPK), MOE_E, dtype=torch.int64, device=DEV)
        one[:, 0] = 5
        one[1::2, 1] = -1
        out.append(("all-to-one-expert", one, w))
    return out


def _moe_case(experts, entry, ws_query, table, T, dtype, what):
    from autogptq_amd.moe import moe_forward
    lib = _lib.load()
    es, R = _es(dtype), T * MOE_TOPK
    m = ctypes.byref(experts._moe)
    need = int(ws_query(m, T, MOE_TOPK))
    assert need > 0, what
    x = _rand(T, MOE_H, dtype, T)
    for name, idx, w in _moe_routings(T, T + MOE_E):
        tag = f"{what} T={T} routing={name}"
        with torch.no_grad():
            y_mod, hs_mod, pos_mod = moe_forward(experts, x, idx, w, return_intermediate=True)
        gx, _ = G.guarded_like(x, G.guard_for(MOE_H * es))
        gi, _ = G.guarded_like(idx, G.guard_for(MOE_TOPK * 8))
        gw, _ = G.guarded_like(w, G.guard_for(MOE_TOPK * 4))
        ws = _workspace(need)
        valid = pos_mod >= 0
        for launch in (1, 2):
            go = _out(T, MOE_H, dtype)
            gh = G.Guarded(R * MOE_I * es + 4 * R, G.guard_for(MOE_I * es), 0xFF, G.OUT_GUARD, DEV)
            _lib.check(entry(m, table.data_ptr(), gx.ptr, gi.ptr, gw.ptr, T, MOE_TOPK, go.ptr, gh.ptr, ws.ptr, need, _stream()))
            for g, nm in ((gx, "x"), (gi, "topk_idx"), (gw, "topk_w"), (go, "out"), (gh, "h_out"), (ws, f"workspace ({need} bytes = its query)")):
                g.assert_intact(f"{tag}: {nm} (launch {launch})")
            y = go.view(dtype, (T, MOE_H))
            assert torch.equal(y, y_mod), f"{tag}: launch {launch} on exact buffers differs from moe_forward in {int((y != y_mod).sum())} outputs"
            pos = gh.body[R * MOE_I * es:].view(torch.int32).view(T, MOE_TOPK)
            hs = gh.body[:R * MOE_I * es].view(dtype).view(R, MOE_I)
            assert torch.equal(pos, pos_mod), f"{tag}: pos"
            assert torch.equal(hs[pos[valid].long()], hs_mod[pos_mod[valid].long()]), f"{tag}: the H rows in use"


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("act", [False, True], ids=["seq", "act"])
@pytest.mark.parametrize("bits", [4, 8])
def test_moe_entries(bits, act, dtype):
    """gptq_moe_forward (7 / 70 / 300 tokens), then -- the same experts with their decode copy -- gptq_moe_decode_forward (1 / 4) and gptq_moe_batch_forward
    (5 / 17 / 64): x, topk_idx, topk_w, out, h_out (R I es + 4 R bytes) and an exact workspace in guards."""
    from test_gpu_moe import make_experts
    lib = _lib.load()
    experts = make_experts(MOE_E, MOE_H, MOE_I, bits, 128, act, dtype, seed=bits + act, top_k=MOE_TOPK)
    what = f"int{bits} act={act} {DT_IDS[dtype]}"
    for T in (7, 70, 300):
        assert experts.plan(T, MOE_TOPK)["path"] == "grouped"
        _moe_case(experts, lib.gptq_moe_forward, lib.gptq_moe_workspace_bytes, experts._table, T, dtype, f"gptq_moe_forward {what}")
    experts.post_init(decode_copy=True, batch=True)
    for T in (1, 4):
        assert experts.plan(T, MOE_TOPK)["path"] == "decode"
        _moe_case(experts, lib.gptq_moe_decode_forward, lib.gptq_moe_decode_workspace_bytes, experts._decode_table, T, dtype, f"gptq_moe_decode_forward {what}")
    for T in (5, 17, 64):
        assert experts.plan(T, MOE_TOPK)["path"] == "batch"
        _moe_case(experts, lib.gptq_moe_batch_forward, lib.gptq_moe_batch_workspace_bytes, experts._decode_table, T, dtype, f"gptq_moe_batch_forward {what}")


# ====================================================================================================================== the alignment contract
def _odd_view(t):
    """A contiguous copy of t that starts one element into a flat arena: data_ptr() % 16 == 2 for the 16-bit types."""
    flat = torch.empty(t.numel() + 8, dtype=t.dtype, device=t.device)
    v = flat[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == t.element_size()
    return v


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
def test_misaligned_x_is_copied_by_every_wrapper(dtype):
    """x = flat[1 : 1 + M K].view(M, K) through QuantLinear (the Python path and, on a row count it serves, the C++ fast path), forward_multi, mlp_forward,
    moe_forward and a LoraQuantLinear: bit-identical to the aligned clone's result.  The C ABI refuses such a pointer (no kernel is ever launched on it), so a
    wrapper that passed it on would raise here."""
    from autogptq_amd.lora import LoraQuantLinear
    from autogptq_amd.moe import moe_forward
    from test_gpu_moe import _routing, make_experts
    lib = _lib.load()
    K = 1056
    q = _make(K, 544, 4, 32, False, dtype, 1)
    qa = _make(K, 544, 4, 32, True, dtype, 2)
    for M in (1, 3, 8, 40, 300):
        x = _rand(M, K, dtype, M)
        xo = _odd_view(x)
        for lay in (q, qa):
            with torch.no_grad():
                ref = lay(x)
                for _ in range(2):                        # the second call finds the row count in the fast path's mask where it needs no workspace
                    assert torch.equal(lay(xo), ref)
                assert torch.equal(lay(xo.view(1, M, K)), ref.view(1, M, -1))
        L = _copy_struct(q._layer)
        out = torch.empty((M, 544), dtype=dtype, device=DEV)
        wsb = torch.zeros(1 << 20, dtype=torch.uint8, device=DEV)
        assert lib.gptq_forward(ctypes.byref(L), xo.data_ptr(), out.data_ptr(), M, wsb.data_ptr(), wsb.numel(), _stream()) == 3      # refused, not launched
        assert "16-byte aligned" in lib.gptq_last_error().decode()
    assert q._ws0_mask or _lib.fwd is None, "no row count of this test reached the C++ fast path"
    # grouped and MLP wrappers
    gate, up, down = _make(K, 544, 4, 32, False, dtype, 3, bias=False), _make(K, 544, 4, 32, False, dtype, 4, bias=False), _make(544, 288, 4, 32, False, dtype, 5)
    for M in (1, 4, 5, 40):
        x = _rand(M, K, dtype, M)
        xo = _odd_view(x)
        with torch.no_grad():
            for _ in range(2):
                for a, b in zip(forward_multi([gate, up], xo), forward_multi([gate, up], x)):
                    assert torch.equal(a, b)
            assert torch.equal(mlp_forward(gate, up, down, xo), mlp_forward(gate, up, down, x))
    # LoRA around a QuantLinear
    lq = LoraQuantLinear(q, 16, 32, adapter_dtype=dtype).to(DEV)
    with torch.no_grad():
        lq.lora_B.weight.normal_(0, 0.05)
        for M in (1, 9):
            x = _rand(M, K, dtype, M)
            assert torch.equal(lq(_odd_view(x)), lq(x))
    # routed experts: every path
    experts = make_experts(MOE_E, MOE_H, MOE_I, 4, 128, False, dtype, seed=9, top_k=MOE_TOPK)
    for phase in (0, 1):
        if phase:
            experts.post_init(decode_copy=True, batch=True)
        for T in (2, 7, 70):
            x = _rand(T, MOE_H, dtype, T)
            idx, w = _routing(T, MOE_E, MOE_TOPK, T)
            with torch.no_grad():
                assert torch.equal(moe_forward(experts, _odd_view(x), idx, w), moe_forward(experts, x, idx, w)), (phase, T, experts.last_plan)


# ====================================================================================================================== closing
def test_the_guards_reached_every_plan_class():
    """Runs last in this file: every class the planner returned on the grid was run, and the run as a whole (grid + forced tables) included the decode-copy
    kernel, the batched-decode, panel and stream-K kernels, the fp32-math GEMV, an MFMA GEMM on the checkpoint rows, K slices on the decode-copy kernel and
    on a GEMM, and an act-order case whose workspace holds the permuted x."""
    if not RAN:
        pytest.skip("run together with the dense cases of this file")
    missing = set(GRID_CLASSES) - set(RAN)
    assert not missing, f"classes of the grid that no case ran: {sorted(missing)}"
    kernels = {k[0] for k in RAN}
    assert {"strips", "rows", "panel", "wide_sk", "generic"} <= kernels, kernels
    assert kernels & MFMA_GEMMS_ON_CHECKPOINT_ROWS, kernels
    assert any(k[0] == "strips" and k[1] for k in RAN), "no K-slice launch of the decode-copy kernel"
    assert any(k[0] in MFMA_GEMMS_ON_CHECKPOINT_ROWS | {"wide_sk", "panel", "rows", "wide_copy"} and k[1] for k in RAN), "no K-slice launch of a GEMM kernel"
    assert any(k[3] for k in RAN), "no act-order case with the permuted x in the workspace"
