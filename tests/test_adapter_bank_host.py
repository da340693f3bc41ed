"""CPU: per-row adapter banks -- the C ABI (gptq_adapter_*: exports, struct layout, the route buffer's size, the host-only plan and every decline reason),
the built code objects (the adapter_rows_* kernels are the four intended instantiations, scratch-free, the lora_* kernels are still four and the library
stays inside its kernel budget), and the module logic of autogptq_amd/adapter_bank.py that needs no kernel (buffers, slots, peft-format keys, the refusals)."""
import ctypes
import os
import re
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import autogptq_amd as A  # noqa: E402
from autogptq_amd import _lib  # noqa: E402
from autogptq_amd import adapter_bank as AB  # noqa: E402
from autogptq_amd.qlinear_mi355x import QuantLinear  # noqa: E402

SYMBOLS = ("gptq_adapter_route_bytes", "gptq_adapter_route", "gptq_adapter_rows_apply", "gptq_describe_adapter_rows_plan")
FAKE = 0x1000                              # never dereferenced: every call below returns before a launch


def _bank(K=4096, N=4096, r=16, slots=4, dtype=_lib.GPTQ_F16):
    L = _lib.GptqAdapterBank()
    L.A = L.B = L.scales = FAKE
    L.K, L.N, L.r, L.slots, L.dtype = K, N, r, slots, dtype
    return L


def _arr(banks):
    return (ctypes.POINTER(_lib.GptqAdapterBank) * len(banks))(*[ctypes.pointer(b) for b in banks])


def _ptrs(n, v=FAKE):
    return (ctypes.c_void_p * n)(*[v] * n)


def _err():
    return _lib.load().gptq_last_error().decode()


# ---------------------------------------------------------------- ABI
def test_symbols_exported_and_declared_abi_still_8():
    header = open(os.path.join(ROOT, "include", "gptq_mi355x.h")).read()
    declared = set(re.findall(r"\b(gptq_[a-z_0-9]+)\s*\(", header))
    lib = _lib.load()
    for s in SYMBOLS:
        assert s in declared and s in _lib.EXPORTS and hasattr(lib, s), s
    assert declared == set(_lib.EXPORTS)
    assert "typedef struct gptq_adapter_bank_t" in header and "} gptq_adapter_bank_t;" in header
    assert lib.gptq_abi_version() == 8 and _lib.ABI_VERSION == 8
    assert "#define GPTQ_MI355X_ABI_VERSION 8" in header
    for name in ("AdapterRouting", "LoraBankQuantLinear", "inject_lora_bank", "load_adapter_slot", "attach_routing", "lora_bank_forward_multi"):
        assert getattr(A, name) is getattr(AB, name)


def test_struct_layout_matches_header():
    # 3 pointers, 6 x int32 (include/gptq_mi355x.h: gptq_adapter_bank_t)
    S = _lib.GptqAdapterBank
    assert ctypes.sizeof(S) == 3 * 8 + 6 * 4 == 48
    assert [getattr(S, f).offset for f in ("A", "B", "scales", "K", "N", "r", "slots", "dtype", "reserved")] == [0, 8, 16, 24, 28, 32, 36, 40, 44]
    header = open(os.path.join(ROOT, "include", "gptq_mi355x.h")).read()
    body = header[header.index("typedef struct gptq_adapter_bank_t"):header.index("} gptq_adapter_bank_t;")]
    order = [body.index(t) for t in ("*A;", "*B;", "*scales;", "int32_t K, N, r, slots, dtype, reserved;")]
    assert order == sorted(order)
    assert _lib.ADAPTER_MAX_SLOTS == 256


def test_route_bytes_is_monotone_and_refuses_what_route_refuses():
    lib = _lib.load()
    for slots in (1, 2, 5, 64, 256):
        sizes = [lib.gptq_adapter_route_bytes(M, slots) for M in (0, 1, 15, 16, 17, 64, 65, 1000, 100000)]
        assert sizes == sorted(sizes) and sizes[0] > 0 and sizes[-1] >= 8 * 100000, (slots, sizes)        # pos + row_assign alone are 8 bytes a row
        assert all(s % 16 == 0 for s in sizes)
    for M in (1, 16, 17, 64, 5000):
        sizes = [lib.gptq_adapter_route_bytes(M, s) for s in (1, 2, 5, 63, 64, 65, 256)]
        assert sizes == sorted(sizes), (M, sizes)
    assert lib.gptq_adapter_route_bytes(-1, 4) == 0 and lib.gptq_adapter_route_bytes(8, 0) == 0 and lib.gptq_adapter_route_bytes(8, 257) == 0


# ---------------------------------------------------------------- the plan
@pytest.mark.parametrize("slots", [1, 5])
@pytest.mark.parametrize("M", [1, 16, 17, 64])
def test_plan_workgroup_counts(M, slots):
    tiles = M // 16 + min(slots, M)                                       # the grid's bound: full tiles plus one partial tile per slot that has rows
    for dtype in (_lib.GPTQ_F16, _lib.GPTQ_BF16):
        for K, N, r in ((4096, 4096, 16), (4096, 11008, 64), (96, 48, 8), (352, 512, 24)):
            d = _lib.describe_adapter_rows_plan([_bank(K, N, r, slots, dtype)], M)
            assert d["path"] == "adapter_rows" and d["launches"] == 2 and d["tiles"] == tiles, d
            assert d["wg_down"] == tiles * -(-r // 16) and d["wg_up"] == tiles * -(-N // 256), d
    group = [_bank(4096, 4096, 64, slots), _bank(4096, 1024, 24, slots), _bank(4096, 1040, 8, slots)]   # q|k|v-like: n = 3 banks in one call
    d = _lib.describe_adapter_rows_plan(group, M)
    assert d["path"] == "adapter_rows" and d["tiles"] == tiles, d
    assert d["wg_down"] == tiles * (4 + 2 + 1) and d["wg_up"] == tiles * (16 + 4 + 5), d
    singles = [_lib.describe_adapter_rows_plan([g], M) for g in group]
    assert d["wg_down"] == sum(s["wg_down"] for s in singles) and d["wg_up"] == sum(s["wg_up"] for s in singles)


def test_plan_at_zero_rows():
    d = _lib.describe_adapter_rows_plan([_bank()], 0)
    assert d["path"] == "adapter_rows" and d["tiles"] == 0 and d["wg_down"] == 0 and d["wg_up"] == 0, d


@pytest.mark.parametrize("kw,n,frag", [
    (dict(dtype=_lib.GPTQ_F32), 1, "fp32"),
    (dict(r=4), 1, "r = 4"),
    (dict(r=72), 1, "r = 72"),
    (dict(r=12), 1, "r = 12"),
    (dict(K=4112), 1, "K = 4112"),
    (dict(N=4104), 1, "N = 4104"),
    (dict(slots=0), 1, "slots = 0"),
    (dict(slots=257), 1, "slots = 257"),
    (dict(), 5, "n = 5"),
])
def test_plan_declines_with_a_reason(kw, n, frag):
    lib = _lib.load()
    group = [_bank(**kw) for _ in range(n)]
    d = _lib.describe_adapter_rows_plan(group, 4)
    assert d["path"] == "none" and frag.replace(" ", "_").replace("=", "_") in d["reason"], d
    rc = lib.gptq_adapter_rows_apply(_arr(group), n, FAKE, _ptrs(n), _ptrs(n), FAKE, 4, None)
    assert rc == 3 and frag in _err(), (rc, _err())                       # GPTQ_ERR_UNSUPPORTED, before any launch


@pytest.mark.parametrize("field,other,frag", [("K", 2048, "share K, dtype and slots"), ("dtype", _lib.GPTQ_BF16, "share K, dtype and slots"),
                                              ("slots", 3, "share K, dtype and slots")])
def test_banks_of_one_call_must_agree(field, other, frag):
    lib = _lib.load()
    b = _bank()
    setattr(b, field, other)
    group = [_bank(), b]
    d = _lib.describe_adapter_rows_plan(group, 4)
    assert d["path"] == "none" and frag.replace(" ", "_").replace("=", "_") in d["reason"], d
    assert lib.gptq_adapter_rows_apply(_arr(group), 2, FAKE, _ptrs(2), _ptrs(2), FAKE, 4, None) == 3 and frag in _err()


def test_misaligned_pointers_decline():
    lib = _lib.load()
    one = _bank()
    arr, good, odd = _arr([one]), _ptrs(1), _ptrs(1, 0x1008)
    assert lib.gptq_adapter_rows_apply(arr, 1, 0x1008, good, good, FAKE, 4, None) == 3 and "x must be 16-byte aligned" in _err()
    assert lib.gptq_adapter_rows_apply(arr, 1, FAKE, odd, good, FAKE, 4, None) == 3 and "u[0]" in _err() and "16-byte aligned" in _err()
    assert lib.gptq_adapter_rows_apply(arr, 1, FAKE, good, odd, FAKE, 4, None) == 3 and "outs[0]" in _err() and "16-byte aligned" in _err()
    assert lib.gptq_adapter_rows_apply(arr, 1, FAKE, good, good, 0x1008, 4, None) == 3 and "route must be 16-byte aligned" in _err()
    for f in ("A", "B"):
        bad = _bank()
        setattr(bad, f, 0x1008)
        d = _lib.describe_adapter_rows_plan([bad], 4)
        assert d["path"] == "none" and "A_/_B_must_be_16-byte_aligned" in d["reason"], d
        assert lib.gptq_adapter_rows_apply(_arr([bad]), 1, FAKE, good, good, FAKE, 4, None) == 3 and "A / B must be 16-byte aligned" in _err()
    assert lib.gptq_adapter_rows_apply(arr, 1, None, good, good, FAKE, 4, None) == 1                 # GPTQ_ERR_NULL
    assert lib.gptq_adapter_rows_apply(arr, 1, FAKE, good, good, FAKE, -1, None) == 2                # GPTQ_ERR_SHAPE


def test_route_declines():
    lib = _lib.load()
    need = lib.gptq_adapter_route_bytes(50, 5)
    assert lib.gptq_adapter_route(FAKE, 50, 0, FAKE, need, None) == 3 and "slots = 0" in _err()
    assert lib.gptq_adapter_route(FAKE, 50, 257, FAKE, 1 << 30, None) == 3 and "slots = 257" in _err()
    assert lib.gptq_adapter_route(FAKE, 50, 5, 0x1008, need, None) == 3 and "route must be 16-byte aligned" in _err()
    assert lib.gptq_adapter_route(FAKE, 50, 5, FAKE, need - 1, None) == 3 and "too small" in _err()
    assert lib.gptq_adapter_route(FAKE, 50, 5, FAKE, 0, None) == 3 and "too small" in _err()
    assert lib.gptq_adapter_route(None, 50, 5, FAKE, need, None) == 1                                # GPTQ_ERR_NULL
    assert lib.gptq_adapter_route(FAKE, -1, 5, FAKE, need, None) == 2                                # GPTQ_ERR_SHAPE


def test_zero_rows_launch_nothing_and_dereference_nothing():
    lib = _lib.load()
    assert lib.gptq_adapter_route(FAKE, 0, 5, FAKE, 0, None) == 0
    assert lib.gptq_adapter_route(None, 0, 5, None, 0, None) == 0
    assert lib.gptq_adapter_rows_apply(_arr([_bank()]), 1, FAKE, _ptrs(1), _ptrs(1), FAKE, 0, None) == 0
    group = [_bank(), _bank(N=1024, r=8), _bank(N=1024, r=8)]
    assert lib.gptq_adapter_rows_apply(_arr(group), 3, FAKE, _ptrs(3), _ptrs(3), FAKE, 0, None) == 0


# ---------------------------------------------------------------- built code objects
def test_adapter_rows_kernels_are_the_four_intended_and_scratch_free():
    from test_kernel_resources import _kernels
    ks = _kernels()
    down = sorted(n for n in ks if "adapter_rows_down_kernel" in n)
    up = sorted(n for n in ks if "adapter_rows_up_kernel" in n)
    mine = {n: v for n, v in ks.items() if "adapter_rows" in n}
    assert len(down) == 2 and len(up) == 2 and len(mine) == 4, sorted(mine)               # two kernels x fp16 / bf16
    for n, v in mine.items():
        assert not (v["spill"] or 0) and not (v["scratch"] or 0), (n, v)
        assert (v["vgpr"] or 0) <= 128 and (v["lds"] or 0) <= 8192, (n, v)
        assert "gptq8adapters" in n and "lora_" not in n, n                               # namespace gptq::adapters; no name the lora_* count would pick up
    assert sum(1 for n in ks if re.search(r"lora_\w*kernel", n)) == 4
    assert sum(1 for n in ks if "moe_route_kernel" in n) == 1                              # the routing kernel is reused, not copied
    assert len(ks) <= 1160, len(ks)


# ---------------------------------------------------------------- module logic (no kernel)
class _Block(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.q_proj = QuantLinear(4, 32, 64, 64, False)
        self.k_proj = QuantLinear(4, 32, 64, 32, False)
        self.o_proj = QuantLinear(4, 32, 64, 64, False)
        self.dense = torch.nn.Linear(64, 64)


class _Model(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.layers = torch.nn.ModuleList([_Block(), _Block()])
        self.head = torch.nn.Linear(64, 8)


def test_buffers_shapes_and_names():
    bq = A.LoraBankQuantLinear(QuantLinear(4, 32, 64, 32, False), 16, 3)
    bufs = dict(bq.named_buffers(recurse=False))
    assert set(bufs) == {"lora_A_bank", "lora_B_bank", "scales"}
    assert bufs["lora_A_bank"].shape == (3, 16, 64) and bufs["lora_B_bank"].shape == (3, 32, 16) and bufs["scales"].shape == (3,)
    assert bufs["lora_A_bank"].dtype == bufs["lora_B_bank"].dtype == torch.float16 and bufs["scales"].dtype == torch.float32
    assert not any(bool(b.any()) for b in bufs.values())                                  # all zero at construction
    assert isinstance(bq.base, QuantLinear) and bq.routing is None and not list(bq.parameters(recurse=False))
    assert {"lora_A_bank", "lora_B_bank", "scales", "base.qweight"} <= set(bq.state_dict())
    bb = A.LoraBankQuantLinear(QuantLinear(4, 32, 64, 32, False, weight_dtype=torch.bfloat16), 8, 1)
    assert bb.lora_A_bank.dtype == torch.bfloat16 and bb.scales.dtype == torch.float32


def test_load_slot_pads_and_scales_and_clear_slot_zeroes():
    torch.manual_seed(0)
    bq = A.LoraBankQuantLinear(QuantLinear(4, 32, 64, 32, False), 16, 3)
    ptrs = [b.data_ptr() for b in (bq.lora_A_bank, bq.lora_B_bank, bq.scales)]
    a8, b8 = torch.randn(8, 64), torch.randn(32, 8)
    a16, b16 = torch.randn(16, 64), torch.randn(32, 16)
    bq.load_slot(1, a16, b16, 32.0)
    bq.load_slot(2, a16, b16, 8.0)
    bq.load_slot(2, a8, b8, 4.0)                                                           # a smaller rank over a larger one: the padding is re-zeroed
    assert torch.equal(bq.lora_A_bank[1], a16.half()) and torch.equal(bq.lora_B_bank[1], b16.half()) and float(bq.scales[1]) == 2.0
    assert torch.equal(bq.lora_A_bank[2, :8], a8.half()) and not bool(bq.lora_A_bank[2, 8:].any())
    assert torch.equal(bq.lora_B_bank[2, :, :8], b8.half()) and not bool(bq.lora_B_bank[2, :, 8:].any())
    assert float(bq.scales[2]) == 0.5                                                      # alpha / the adapter's own rank, not the bank's r
    assert not bool(bq.lora_A_bank[0].any()) and float(bq.scales[0]) == 0.0                # other slots untouched
    bq.clear_slot(1)
    assert not bool(bq.lora_A_bank[1].any()) and not bool(bq.lora_B_bank[1].any()) and float(bq.scales[1]) == 0.0
    assert float(bq.scales[2]) == 0.5
    assert ptrs == [b.data_ptr() for b in (bq.lora_A_bank, bq.lora_B_bank, bq.scales)]     # written in place: the addresses never move
    with pytest.raises(ValueError, match="rank 24"):
        bq.load_slot(0, torch.randn(24, 64), torch.randn(32, 24), 1.0)
    with pytest.raises(ValueError, match="expects"):
        bq.load_slot(0, torch.randn(8, 32), torch.randn(32, 8), 1.0)
    with pytest.raises(ValueError, match="expects"):
        bq.load_slot(0, torch.randn(8, 64), torch.randn(32, 16), 1.0)
    for bad in (-1, 3):
        with pytest.raises(IndexError):
            bq.load_slot(bad, a8, b8, 1.0)
        with pytest.raises(IndexError):
            bq.clear_slot(bad)


def test_refusals():
    with pytest.raises(ValueError, match="silu_mul"):
        A.LoraBankQuantLinear(QuantLinear(4, 32, 64, 128, False, epilogue="silu_mul"), 8, 2)
    with pytest.raises(TypeError):
        A.LoraBankQuantLinear(torch.nn.Linear(64, 64), 8, 2)
    for r in (0, 4, 12, 72):
        with pytest.raises(ValueError, match="r = "):
            A.LoraBankQuantLinear(QuantLinear(4, 32, 64, 64, False), r, 2)
    for s in (0, 257):
        with pytest.raises(ValueError, match="num_slots"):
            A.LoraBankQuantLinear(QuantLinear(4, 32, 64, 64, False), 8, s)
    with pytest.raises(ValueError, match="fp16 / bf16"):
        A.LoraBankQuantLinear(QuantLinear(4, 32, 64, 64, False, weight_dtype=torch.float32), 8, 2)
    bq = A.LoraBankQuantLinear(QuantLinear(4, 32, 64, 64, False), 8, 2)
    with pytest.raises(RuntimeError, match="inference only"):                              # before the base is touched
        bq(torch.randn(2, 64, dtype=torch.float16, requires_grad=True))


class _FakeRouting:
    def __init__(self, rows, num_slots):
        self.rows, self.num_slots = rows, num_slots


def test_forward_checks_rows_against_the_routing():
    bq = A.LoraBankQuantLinear(QuantLinear(4, 32, 64, 64, False), 8, 2)
    bq.routing = _FakeRouting(6, 2)
    with torch.no_grad():
        assert bq._rows_of(torch.zeros(6, 64)) == 6 and bq._rows_of(torch.zeros(2, 3, 64)) == 6
        for shape in ((5, 64), (2, 4, 64), (6, 32)):
            with pytest.raises(ValueError, match="routing holds 6 rows"):
                bq._rows_of(torch.zeros(*shape))
        bq.routing = _FakeRouting(6, 3)
        with pytest.raises(ValueError, match="3 slots"):
            bq._rows_of(torch.zeros(6, 64))
        bq.routing = _FakeRouting(0, 2)
        assert bq._rows_of(torch.zeros(5, 64)) == 0                                        # an empty routing: the layer is its base
        bq.routing = None
        assert bq._rows_of(torch.zeros(5, 64)) == 0


def test_inject_and_attach():
    m = _Model()
    before = set(m.state_dict())
    got = A.inject_lora_bank(m, ["q_proj", "k_proj", "dense"], r=8, num_slots=3)
    assert sorted(got) == ["layers.0.k_proj", "layers.0.q_proj", "layers.1.k_proj", "layers.1.q_proj"]          # `dense` is no QuantLinear
    for name, mod in got.items():
        assert isinstance(mod, A.LoraBankQuantLinear) and m.get_submodule(name) is mod and isinstance(mod.base, QuantLinear)
        assert mod.lora_A_bank.shape == (3, 8, 64) and mod.lora_B_bank.shape == (3, mod.base.outfeatures, 8)
    assert isinstance(m.layers[0].o_proj, QuantLinear)
    assert {k.replace("q_proj.", "q_proj.base.").replace("k_proj.", "k_proj.base.") for k in before} <= set(m.state_dict())
    assert A.inject_lora_bank(m, ["q_proj"], r=8, num_slots=3) == {}                                            # nothing is wrapped twice
    rt = _FakeRouting(4, 3)
    A.attach_routing(m, rt)
    assert all(mod.routing is rt for mod in got.values())
    with pytest.raises(ValueError, match="slots"):
        A.attach_routing(m, _FakeRouting(4, 2))
    A.attach_routing(m, None)
    assert all(mod.routing is None for mod in got.values())


def test_load_adapter_slot_key_handling():
    torch.manual_seed(1)
    m = _Model()
    got = A.inject_lora_bank(m, ["q_proj", "k_proj"], r=16, num_slots=2)
    q_names = [n for n in got if n.endswith("q_proj")]
    sd = {}
    for n in q_names:                                                                      # a rank-8 adapter on q_proj only
        sd[f"base_model.model.{n}.lora_A.weight"] = torch.randn(8, 64)
        sd[f"base_model.model.{n}.lora_B.weight"] = torch.randn(64, 8)
    cfg = {"r": 8, "lora_alpha": 16, "target_modules": ["q_proj"]}
    for mod in got.values():
        mod.load_slot(1, torch.ones(16, 64), torch.ones(mod.out_features, 16), 16.0)       # stale contents the load must replace or clear
    written = A.load_adapter_slot(m, 1, sd, cfg)
    assert sorted(written) == sorted(q_names)
    for n, mod in got.items():
        if n in q_names:
            assert torch.equal(mod.lora_A_bank[1, :8], sd[f"base_model.model.{n}.lora_A.weight"].half()) and not bool(mod.lora_A_bank[1, 8:].any())
            assert torch.equal(mod.lora_B_bank[1, :, :8], sd[f"base_model.model.{n}.lora_B.weight"].half()) and float(mod.scales[1]) == 2.0
        else:
            assert not bool(mod.lora_A_bank[1].any()) and not bool(mod.lora_B_bank[1].any()) and float(mod.scales[1]) == 0.0   # cleared
        assert not bool(mod.lora_A_bank[0].any())                                          # the other slot untouched
    # peft's in-memory key form, and keys without the prefix
    A.load_adapter_slot(m, 0, {k.replace(".weight", ".default.weight"): v for k, v in sd.items()}, cfg)
    assert all(torch.equal(got[n].lora_A_bank[0], got[n].lora_A_bank[1]) for n in q_names)
    A.load_adapter_slot(m, 0, {k[len("base_model.model."):]: v * 2 for k, v in sd.items()}, cfg)
    assert all(torch.equal(got[n].lora_A_bank[0], (sd[f"base_model.model.{n}.lora_A.weight"] * 2).half().new_zeros(16, 64).index_copy_(
        0, torch.arange(8), (sd[f"base_model.model.{n}.lora_A.weight"] * 2).half())) for n in q_names)
    with pytest.raises(KeyError, match="lacks"):
        A.load_adapter_slot(m, 0, {k: v for k, v in sd.items() if "lora_B" not in k}, cfg)
    with pytest.raises(KeyError, match="no bank layer"):
        A.load_adapter_slot(m, 0, dict(sd, **{"base_model.model.layers.0.o_proj.lora_A.weight": torch.zeros(8, 64)}), cfg)
    with pytest.raises(KeyError, match="unexpected key"):
        A.load_adapter_slot(m, 0, dict(sd, **{"base_model.model.layers.0.q_proj.weight": torch.zeros(8, 64)}), cfg)
    with pytest.raises(RuntimeError, match="no adapter banks"):
        A.load_adapter_slot(_Model(), 0, sd, cfg)
