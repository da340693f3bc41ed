"""GPU: per-row adapter banks -- gptq_adapter_route / gptq_adapter_rows_apply (csrc/adapter_rows.hip), AdapterRouting, LoraBankQuantLinear and the model
helpers (autogptq_amd/adapter_bank.py).

Arithmetic contract, for a row m whose id a = ids[m] lies in [0, slots): u_m = T(x[m] . A[a]^T) and out[m] = T(out[m] + scales[a] * u_m . B[a]^T), fp32
products and sums, one rounding each; any other id leaves out[m] untouched bit for bit.  The error model is the one tests/test_gpu_lora.py states and derives
(C = 16: the kernels are lora.hip's matrix-core regime -- chains of K / 256 matrix-core steps plus 8 partial sums met in LDS -- on gathered rows), applied per
row with THAT row's slot:

    |u - u64|      <=  (1/2 + 1/64) ulp(u64)    +  C * sqrt(K) * 2^-24 * (|x[m]| . |A[a]|^T)
    |out - out64|  <=  (1/2 + 1/64) ulp(out64)  +  C * sqrt(r) * 2^-24 * |scales[a]| * (|u_m| . |B[a]|^T)     out64 = y + scales[a] * u_m . B[a]^T on the u, y fed in

u comes back in SORTED-row order (routed rows ordered by slot, the rows of one slot by ascending m: include/gptq_mi355x.h); the tests map it back through
pos[m], recomputed here from the ids by that rule.  The module prints the worst err / bound per dtype at its end.

The tiny-Llama test compares whole-model logits: the premise (one id vector run twice gives identical logits) is asserted first."""
import ctypes
import math

import pytest
import torch

import _tiny_llama as TL
import autogptq_amd as A
from _guarded import Guarded, guard_for, guarded_like
from autogptq_amd import _lib
from autogptq_amd.qlinear_mi355x import QuantLinear
from oracle import gptq_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
C = 16.0
KS = (96, 352)                       # 3 and 11 k-steps over 8 waves
NS = (48, 512)                       # a partial and two full column blocks
RS = (8, 24, 64)
SLOTS = (1, 3, 5)
MS = (1, 5, 16, 17, 33, 50)
PATTERNS = ("one", "robin", "hole", "random", "none")
DTYPES = [torch.float16, torch.bfloat16]
IDS = ["f16", "bf16"]
SCALES = (2.0, 0.5, 1.0, -1.5, 0.75)
WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _report_worst():
    yield
    print("\nadapter rows error model: worst err / bound:", {k: round(v, 3) for k, v in sorted(WORST.items())})


# ---------------------------------------------------------------- helpers
def _ulp(v64, dtype):
    mant, emin = {torch.float16: (10, -14), torch.bfloat16: (7, -126)}[dtype]
    e = torch.floor(torch.log2(v64.abs().clamp_min(2.0 ** emin)))
    return torch.pow(torch.tensor(2.0, dtype=torch.float64, device=v64.device), e - mant)


def _randn(*shape, dtype=torch.float16, seed=0, mul=1.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * mul).to(dtype).to(DEV)


def _ids(pattern, M, slots, seed=0):
    """The id patterns of the issue, as an int64 CPU tensor."""
    if pattern == "one":                                   # all one slot: M = 33 gives tiles of 16 + 16 + 1
        return torch.full((M,), slots - 1, dtype=torch.int64)
    if pattern == "robin":
        return torch.arange(M, dtype=torch.int64) % slots
    if pattern == "hole":                                  # one slot (the first) has no rows; with one slot that leaves no routed row
        return torch.arange(M, dtype=torch.int64) % (slots - 1) + 1 if slots > 1 else torch.full((M,), -1, dtype=torch.int64)
    if pattern == "none":
        return torch.full((M,), -1, dtype=torch.int64)
    g = torch.Generator().manual_seed(seed + 31 * M + slots)
    ids = torch.randint(0, slots, (M,), generator=g)
    ids[torch.rand(M, generator=g) < 0.25] = -1            # about a quarter without an adapter
    if M >= 2:
        where = torch.randperm(M, generator=g)[:2]
        ids[where[0]] = slots                              # just past the bank
        ids[where[1]] = -7
    return ids


def _pos(ids, slots):
    """pos[m] by the documented order: routed rows sorted by slot, the rows of one slot by ascending m; -1 for a row without an adapter."""
    valid = (ids >= 0) & (ids < slots)
    order = torch.argsort(torch.where(valid, ids, torch.full_like(ids, slots)), stable=True)
    pos = torch.full_like(ids, -1)
    n = int(valid.sum())
    pos[order[:n]] = torch.arange(n, dtype=ids.dtype)
    return pos, valid


def _bank_tensors(slots, r, K, N, dtype, seed):
    a = _randn(slots, r, K, dtype=dtype, seed=seed, mul=1.0 / math.sqrt(K))
    b = _randn(slots, N, r, dtype=dtype, seed=seed + 1, mul=0.25)
    s = torch.tensor(SCALES[:slots], dtype=torch.float32, device=DEV)
    return a, b, s


def _struct(a, b, s):
    L = _lib.GptqAdapterBank()
    L.A, L.B, L.scales = a.data_ptr(), b.data_ptr(), s.data_ptr()
    L.slots, L.r, L.K = a.shape[0], a.shape[1], a.shape[2]
    L.N, L.dtype = b.shape[1], _lib.DTYPE_ENUM[a.dtype]
    return L


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _route(ids_dev, slots, route=None):
    lib = _lib.load()
    M = ids_dev.numel()
    need = lib.gptq_adapter_route_bytes(M, slots)
    if route is None:
        route = torch.zeros(need, dtype=torch.uint8, device=DEV)
    _lib.check(lib.gptq_adapter_route(ids_dev.data_ptr(), M, slots, route.data_ptr(), need, _stream()))
    return route


def _apply(banks, x, outs, ids_dev, us=None, route=None):
    """One gptq_adapter_route + one gptq_adapter_rows_apply for the banks [(A, B, scales)]; returns (outs, us)."""
    M = x.shape[0]
    slots = banks[0][0].shape[0]
    route = _route(ids_dev, slots, route)
    structs = [_struct(*bk) for bk in banks]
    arr = (ctypes.POINTER(_lib.GptqAdapterBank) * len(structs))(*[ctypes.pointer(s) for s in structs])
    if us is None:
        us = [torch.full((M, bk[0].shape[1]), float("nan"), dtype=x.dtype, device=DEV) for bk in banks]
    uptr = (ctypes.c_void_p * len(us))(*[u.data_ptr() for u in us])
    optr = (ctypes.c_void_p * len(outs))(*[o.data_ptr() for o in outs])
    _lib.check(_lib.load().gptq_adapter_rows_apply(arr, len(structs), x.data_ptr(), uptr, optr, route.data_ptr(), M, _stream()))
    return outs, us


def _check_rows(x, y, out, u, bank, ids, dtype, key):
    """Error model (routed rows, each with its slot) and the untouched rows of one single-bank call; ids on the CPU."""
    a, b, s = bank
    slots, r, K = a.shape
    pos, valid = _pos(ids, slots)
    vd = valid.to(DEV)
    nv = int(valid.sum())
    assert torch.equal(out[~vd], y[~vd])                                           # untouched bit for bit (with all ids -1: the whole output)
    assert bool(torch.isnan(u[nv:]).all())                                         # u rows past the routed count are not written
    if nv == 0:
        return
    rows = torch.nonzero(valid).flatten().to(DEV)
    sl = ids[valid].to(DEV)
    ur = u[pos[valid].to(DEV)]                                                     # u of the routed rows, in the order of `rows`
    assert not bool(torch.isnan(ur).any())
    xr, a64, b64 = x[rows].double(), a[sl].double(), b[sl].double()                # [R, K], [R, r, K], [R, N, r]
    u64 = torch.einsum("mk,mjk->mj", xr, a64)
    ubound = (0.5 + 1 / 64) * _ulp(u64, dtype) + C * math.sqrt(K) * 2.0 ** -24 * torch.einsum("mk,mjk->mj", xr.abs(), a64.abs())
    sc = s[sl].double()[:, None]
    term = sc * torch.einsum("mj,mnj->mn", ur.double(), b64)
    out64 = y[rows].double() + term
    obound = (0.5 + 1 / 64) * _ulp(out64, dtype) + C * math.sqrt(r) * 2.0 ** -24 * sc.abs() * torch.einsum("mj,mnj->mn", ur.double().abs(), b64.abs())
    assert float(term.norm()) >= 0.1 * float(y[rows].double().norm())              # a wrong adapter term cannot hide under y's rounding
    for name, got, want, bound in (("down", ur, u64, ubound), ("up", out[rows], out64, obound)):
        ratio = float(((got.double() - want).abs() / bound).max())
        k = f"{name} {key}"
        WORST[k] = max(WORST.get(k, 0.0), ratio)
        assert ratio <= 1.0, (k, ratio)


# ---------------------------------------------------------------- 1 + 2. error model per row, untouched rows
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_error_model_per_row_and_untouched_rows(dtype, K):
    key = IDS[DTYPES.index(dtype)]
    xs = {M: _randn(M, K, dtype=dtype, seed=1000 + M) for M in MS}
    combo = 0
    for N in NS:
        ys = {M: _randn(M, N, dtype=dtype, seed=3000 + M) for M in MS}
        for r in RS:
            banks = {slots: _bank_tensors(slots, r, K, N, dtype, seed=K + N + r + slots) for slots in SLOTS}
            for M in MS:
                for slots in SLOTS:
                    for pattern in PATTERNS:
                        ids = _ids(pattern, M, slots, seed=combo)
                        combo += 1
                        (out,), (u,) = _apply([banks[slots]], xs[M], [ys[M].clone()], ids.to(DEV))
                        _check_rows(xs[M], ys[M], out, u, banks[slots], ids, dtype, key)
    print(f"  {key} K={K}: worst err / bound down {WORST[f'down {key}']:.3f} up {WORST[f'up {key}']:.3f} over {combo} calls")


# ---------------------------------------------------------------- 3. row independence
@pytest.mark.parametrize("M", [17, 50])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_rows_do_not_depend_on_each_other(dtype, M):
    K, N, r, slots = 352, 512, 24, 5
    bank = _bank_tensors(slots, r, K, N, dtype, seed=7)
    x, y = _randn(M, K, dtype=dtype, seed=M), _randn(M, N, dtype=dtype, seed=M + 1)
    ids = _ids("random", M, slots, seed=3)
    (out,), _ = _apply([bank], x, [y.clone()], ids.to(DEV))
    assert not torch.equal(out, y)
    # permuted rows of (x, ids, out): the same permutation of the result
    perm = torch.randperm(M, generator=torch.Generator().manual_seed(M))
    pd = perm.to(DEV)
    (outp,), _ = _apply([bank], x[pd].contiguous(), [y[pd].contiguous()], ids[perm].to(DEV))
    assert torch.equal(outp, out[pd])
    # row m keeps its bits when every other row's id is replaced
    for m in (0, M // 2, M - 1):
        for other in (-1, 0, slots - 1):
            ids2 = torch.full((M,), other, dtype=torch.int64)
            ids2[m] = ids[m]
            (out2,), _ = _apply([bank], x, [y.clone()], ids2.to(DEV))
            assert torch.equal(out2[m], out[m]), (m, other)


# ---------------------------------------------------------------- 4. repeat calls
def test_two_calls_give_identical_results():
    K, N, r, slots = 352, 512, 64, 3
    bank = _bank_tensors(slots, r, K, N, torch.float16, seed=9)
    for M in (1, 5, 33, 50):
        x, y = _randn(M, K, seed=M), _randn(M, N, seed=M + 1)
        ids = _ids("random", M, slots, seed=M).to(DEV)
        (a,), (ua,) = _apply([bank], x, [y.clone()], ids)
        (b,), (ub,) = _apply([bank], x, [y.clone()], ids)
        assert torch.equal(a, b) and torch.equal(ua.view(torch.int16), ub.view(torch.int16)), M


# ---------------------------------------------------------------- 5. multi-bank calls
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_a_three_bank_call_equals_three_single_calls(dtype):
    K, slots = 352, 3
    shapes = ((512, 64), (64, 24), (48, 8))                              # q|k|v-like: (N, r) per bank
    banks = [_bank_tensors(slots, r, K, N, dtype, seed=10 + 3 * i) for i, (N, r) in enumerate(shapes)]
    for M in (1, 5, 17, 50):
        x = _randn(M, K, dtype=dtype, seed=M)
        ys = [_randn(M, N, dtype=dtype, seed=30 + i) for i, (N, _) in enumerate(shapes)]
        ids = _ids("random" if M > 1 else "one", M, slots, seed=M).to(DEV)
        multi, mu = _apply(banks, x, [y.clone() for y in ys], ids)
        for i in range(3):
            (single,), (su,) = _apply(banks[i:i + 1], x, [ys[i].clone()], ids)
            assert torch.equal(mu[i].view(torch.int16), su.view(torch.int16)) and torch.equal(multi[i], single), (M, i)
            assert not torch.equal(single, ys[i])


# ---------------------------------------------------------------- 6. guard bands
@pytest.mark.parametrize("M", [1, 17, 50])
def test_every_buffer_between_guards(M):
    K, N, r, slots, dtype = 352, 48, 24, 3, torch.bfloat16
    lib = _lib.load()
    a, b, s = _bank_tensors(slots, r, K, N, dtype, seed=M)
    ids = _ids("random" if M > 1 else "one", M, slots, seed=M)
    gx, xv = guarded_like(_randn(M, K, dtype=dtype, seed=M + 1), guard_for(2 * K))
    gi, iv = guarded_like(ids.to(DEV), guard_for(8))
    ga, av = guarded_like(a, guard_for(2 * K))
    gb, bv = guarded_like(b, guard_for(2 * r))
    gs, sv = guarded_like(s, guard_for(4))
    gu = Guarded(M * r * 2, guard_for(2 * r), 0xFF, device=DEV)
    go = Guarded(M * N * 2, guard_for(2 * N), 0xFF, device=DEV)
    need = lib.gptq_adapter_route_bytes(M, slots)
    gr = Guarded(need, guard_for(need, 1), 0x00, device=DEV)
    y = _randn(M, N, dtype=dtype, seed=M + 2)
    uv, ov = gu.view(dtype, (M, r)), go.view(dtype, (M, N))
    ov.copy_(y)
    assert bool((uv.view(torch.int16) == -1).all())                       # the 0xFF fill
    (out,), (u,) = _apply([(av, bv, sv)], xv, [ov], iv, us=[uv], route=gr.view(torch.uint8, (need,)))
    for g, name in ((gx, "x"), (gi, "ids"), (ga, "A bank"), (gb, "B bank"), (gs, "scales"), (gu, "u"), (go, "out"), (gr, "route")):
        g.assert_intact(f"{name} (M = {M})")
    pos, valid = _pos(ids, slots)
    nv = int(valid.sum())
    written = ~(uv.view(torch.int16) == -1).all(dim=1)
    assert bool(written[:nv].all()) and not bool(written[nv:].any())     # exactly the routed rows of u (sorted-row order: the first nv)
    # and the values are those of the same call on plain tensors
    (ref,), (uref,) = _apply([(a, b, s)], xv.clone(), [y.clone()], ids.to(DEV))
    assert torch.equal(out, ref) and torch.equal(u[:nv].view(torch.int16), uref[:nv].view(torch.int16))


# ---------------------------------------------------------------- 7. the module against the fp64 composition
def _ql(K, N, bits, gs, dtype=torch.float16, act=False, seed=0, bias=False):
    L = O.random_quant_layer(K, N, bits, gs, dtype=dtype, seed=seed, act_order=act, bias=bias)
    q = QuantLinear(bits, gs, K, N, bias, weight_dtype=dtype)
    q.qweight, q.qzeros, q.scales = L["qweight"].clone(), L["qzeros"].clone(), L["scales"].clone()
    q.g_idx = L["g_idx"].clone().to(torch.int32)
    if bias:
        q.bias = L["bias"].clone()
    q = q.to(DEV)
    q.post_init()
    return q


def _bank_layer(q, r, slots, seed, ranks=None):
    """A LoraBankQuantLinear with every slot loaded (slot i: rank ranks[i], alpha = 2 * rank * (i + 1))."""
    bq = A.LoraBankQuantLinear(q, r, slots).eval()
    g = torch.Generator().manual_seed(seed)
    for i in range(slots):
        rank = ranks[i] if ranks else r
        bq.load_slot(i, torch.randn(rank, q.infeatures, generator=g) / math.sqrt(q.infeatures), torch.randn(q.outfeatures, rank, generator=g) * 0.05,
                     2.0 * rank * (i + 1))
    return bq


CONFIGS = [(4, 32, False), (4, 32, True), (8, 32, False), (3, 32, False)]


@pytest.mark.parametrize("KN", [(256, 64), (1024, 512)], ids=["256x64", "1024x512"])
@pytest.mark.parametrize("cfg", CONFIGS, ids=["int4", "int4-act", "int8", "int3"])
def test_module_against_the_composition(cfg, KN):
    """Bound, per row with its slot a: the layer's forward tolerance (4e-3 * max(1, |ref|max)) for the base term, plus the up bound on the exact u, plus what
    the ONE rounding of u (and the down kernel's fp32 error: the down bound) can move the output by: |scales[a]| * down_bound . |B[a]|^T.  Rows without an
    adapter equal the base layer's output bit for bit."""
    bits, gs, act = cfg
    K, N = KN
    dtype, r, slots = torch.float16, 24, 3
    q = _ql(K, N, bits, gs, dtype, act, seed=K + bits, bias=True)
    bq = _bank_layer(q, r, slots, seed=7, ranks=(24, 8, 16))
    assert [float(v) for v in bq.scales] == [2.0, 4.0, 6.0]
    W64 = q.dequantize().double()
    for M in (1, 4, 64):
        x = _randn(M, K, dtype=dtype, seed=M)
        ids = {1: torch.tensor([1]), 4: torch.tensor([2, -1, 0, 1])}.get(M)                 # mixed ids; 64 rows: the seeded random pattern
        if ids is None:
            ids = _ids("random", M, slots, seed=M)
        routing = A.AdapterRouting(64, slots, DEV).set(ids)
        bq.routing = routing
        with torch.no_grad():
            y = bq(x)
            base = q(x)
        assert y.dtype == x.dtype and y.shape == (M, N)
        pos, valid = _pos(ids, slots)
        vd = valid.to(DEV)
        assert torch.equal(y[~vd], base[~vd])
        rows, sl = torch.nonzero(valid).flatten().to(DEV), ids[valid].to(DEV)
        xr, a64, b64 = x[rows].double(), bq.lora_A_bank[sl].double(), bq.lora_B_bank[sl].double()
        sc = bq.scales[sl].double()[:, None]
        base64 = xr @ W64 + q.bias.double()
        u64 = torch.einsum("mk,mjk->mj", xr, a64)
        dbound = (0.5 + 1 / 64) * _ulp(u64, dtype) + C * math.sqrt(K) * 2.0 ** -24 * torch.einsum("mk,mjk->mj", xr.abs(), a64.abs())
        term = sc * torch.einsum("mj,mnj->mn", u64, b64)
        ref = base64 + term
        bound = 4e-3 * max(1.0, float(ref.abs().max())) + (0.5 + 1 / 64) * _ulp(ref, dtype) \
            + C * math.sqrt(r) * 2.0 ** -24 * sc * torch.einsum("mj,mnj->mn", u64.abs(), b64.abs()) + sc * torch.einsum("mj,mnj->mn", dbound, b64.abs())
        err = (y[rows].double() - ref).abs()
        assert bool((err <= bound).all()), (M, float((err / bound).max()))
        # and the adapter is really in there: without it the output would be off by the whole term
        assert float((y[rows].double() - base64).norm()) >= 0.5 * float(term.norm()) > 0, M
    # a 3-D input whose leading dims multiply to the routed rows; anything else raises
    bq.routing = A.AdapterRouting(64, slots, DEV).set([0, -1, 2], rows_per_seq=2)
    x3 = _randn(3, 2, K, dtype=dtype, seed=11)
    with torch.no_grad():
        y3 = bq(x3)
        base3 = q(x3)
        assert y3.shape == (3, 2, N) and torch.equal(y3[1], base3[1]) and not torch.equal(y3[0], base3[0]) and not torch.equal(y3[2], base3[2])
        with pytest.raises(ValueError, match="routing holds 6 rows"):
            bq(_randn(5, K, dtype=dtype, seed=12))
        bq.routing = None
        assert torch.equal(bq(x3), base3)


# ---------------------------------------------------------------- 8. graph capture
def test_routing_and_multi_forward_as_one_graph():
    K, M, slots = 256, 5, 3
    layers = [_bank_layer(_ql(K, n, 4, 32, seed=40 + i), r, slots, seed=50 + i) for i, (n, r) in enumerate(((512, 64), (64, 8), (64, 24)))]
    routing = A.AdapterRouting(8, slots, DEV)
    for l in layers:
        l.routing = routing
    x = _randn(M, K, seed=1)
    routing.set([0, 1, 2, -1, 0])
    with torch.no_grad():
        warm = A.lora_bank_forward_multi(layers, x)
        single = [l(x) for l in layers]
    assert all(torch.equal(m, s) for m, s in zip(warm, single))          # the multi call equals the per-layer calls
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g), torch.no_grad():
        routing.set()                                                    # the routing kernel alone: ids are whatever the static buffer holds at replay
        outs = A.lora_bank_forward_multi(layers, x)
    for vec in ([2, 2, -1, 1, 0], [-1, -1, -1, -1, -1], [1, 0, 0, 2, 3]):
        routing.ids[:M].copy_(torch.tensor(vec, device=DEV))
        for y in outs:
            y.zero_()
        g.replay()
        torch.cuda.synchronize()
        got = [y.clone() for y in outs]
        routing.set(vec)
        with torch.no_grad():
            eager = A.lora_bank_forward_multi(layers, x)
            bases = [l.base(x) for l in layers]
        assert all(torch.equal(a, b) for a, b in zip(got, eager)), vec
        if all(v < 0 for v in vec):
            assert all(torch.equal(a, b) for a, b in zip(got, bases))
        else:
            assert not any(torch.equal(a, b) for a, b in zip(got, bases))


# ---------------------------------------------------------------- 9. tiny Llama
def test_tiny_llama_mixed_adapter_batch(tmp_path):
    """Whole-model logits (the premise holds: one id vector run twice gives identical logits, asserted first)."""
    from autogptq_amd.model_utils import autogptq_post_init
    m = TL.fresh_model(3)
    TL.quantize_and_pack(m, False)
    TL.save_checkpoint(m, str(tmp_path), False)
    del m
    qm, _, _ = TL.load_checkpoint(str(tmp_path))
    qm = autogptq_post_init(qm.to(DEV), use_act_order=False, max_input_length=64).eval()
    Bt, S, slots = 4, 6, 3
    tok = torch.randint(0, 512, (Bt, S), generator=torch.Generator().manual_seed(5)).to(DEV)
    with torch.no_grad():
        plain = qm(tok).logits.clone()
    targets = ["q_proj", "k_proj", "v_proj", "o_proj", "gate_proj", "up_proj", "down_proj"]
    layers = A.inject_lora_bank(qm, targets, r=16, num_slots=slots)
    assert len(layers) == 7 * 2
    gen = torch.Generator().manual_seed(9)
    for s, rank in enumerate((16, 8, 16)):                               # three peft-format state dicts with random lora_B
        sd = {}
        for n, l in layers.items():
            sd[f"base_model.model.{n}.lora_A.weight"] = torch.randn(rank, l.in_features, generator=gen) / math.sqrt(l.in_features)
            sd[f"base_model.model.{n}.lora_B.weight"] = torch.randn(l.out_features, rank, generator=gen) * 0.05
        A.load_adapter_slot(qm, s, sd, {"r": rank, "lora_alpha": 2 * rank, "target_modules": targets})
    routing = A.AdapterRouting(Bt * S, slots, DEV)
    A.attach_routing(qm, routing)

    def run(vec):
        routing.set(vec, rows_per_seq=S)
        with torch.no_grad():
            return qm(tok).logits.clone()

    mixed = [1, -1, 0, 2]
    got = run(mixed)
    assert torch.equal(got, run(mixed))                                  # the premise: the model is bit-reproducible here
    whole = {s: run([s] * Bt) for s in (-1, 0, 1, 2)}
    for i, s in enumerate(mixed):
        assert torch.equal(got[i], whole[s][i]), (i, s)                  # sequence i does not see its neighbours' adapters
    assert torch.equal(whole[-1], plain)                                 # no adapter anywhere: the un-injected model, bit for bit
    for s in range(slots):
        assert not torch.equal(whole[s], plain), s
        for i in range(Bt):
            assert not torch.equal(whole[s][i], plain[i]), (s, i)
