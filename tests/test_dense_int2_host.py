"""CPU (-m "not gpu"): dense 2-bit layers at 5+ rows on their decode copy, the opt-in GPTQ_COPY_ROWS_INT2 (0x100, OR-ed into gptq_layer_t.tiled_cols;
QuantLinear.post_init(low_bit_rows=True)).

* Plans of flagged layers (fake pointers, host arithmetic): `rows` / `panel` with body=lowbit where the planner gives the 4-bit layer of the same shape its rows
  / panel kernel, the unflagged plan key for key everywhere else (1 - 4 rows, N % 64, a group size the forms do not take), the workspace of the same route.
* The flag on 3-, 4- and 8-bit layers and on layers without a copy changes nothing: every query equal for M = 1 .. 1100.
* No behaviour change without the flag: tests/golden/plans_int2_parent.json was recorded from a build of the PARENT commit
  (tests/golden/make_plans_int2_parent.py); this build reproduces it exactly.
* The ABI: version 8, the struct's size, the header names the flag, the Python switches default to off.
* The built library: no new kernel (<= 1160, 4 + 4 low-bit routed-expert kernels, no scratch, <= 128 / <= 256 registers), the in-flight lint clean on the four
  kernels that carry the dense form.
* A numpy restatement of the dense forms' indexing (tile -> rows and the clamp past M, strip group / column tile -> columns, lane -> k, chunk / step -> group)
  over the 2-bit copy model of test_moe_lowbit_batch_host.py (Deq1_2 on a shifted word, every fp16 intermediate exact), against oracle.gptq_oracle on the
  shapes of the GPU tests."""
import ctypes
import importlib.util
import inspect
import json
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

import make_plans_int2_parent as GEN  # noqa: E402
from autogptq_amd import _lib  # noqa: E402
from oracle import gptq_oracle as O  # noqa: E402
from test_moe_lowbit_batch_host import _Exact, _frag2  # noqa: E402

FLAG = getattr(_lib, "COPY_ROWS_INT2", 0x100)          # (the parent has no such name: the tests below then fail on what the library answers)
WIDE = getattr(_lib, "COPY_ROWS_INT2_WIDE", 0x200)     # with FLAG: the whole band of the 4-bit twin (a layer whose checkpoint rows are not resident)
ROWS_ON, PANEL_ON = 50, 52


def _layer(K=4096, N=4096, gs=128, dtype=0, bits=2, copy=True, act=False, flag=True, wide=False):
    return GEN.layer(K, N, gs, dtype, copy, act, tiled_cols=16 | (FLAG if flag else 0) | (WIDE if wide else 0), bits=bits)


def _plan(L, M, knob=0):
    return _lib.describe_plan(L, M, GEN.tuning(knob))


def _ws(L, M, knob=0):
    t = GEN.tuning(knob)
    return int(_lib.load().gptq_workspace_bytes_ex(ctypes.byref(L), M, ctypes.byref(t) if t is not None else None))


def _a256(b):
    return (b + 255) // 256 * 256


# ---- plans of flagged layers ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [0, 1], ids=["f16", "bf16"])
@pytest.mark.parametrize("act", [False, True], ids=["plain", "act"])
def test_flagged_layers_plan_the_low_bit_forms_where_the_4_bit_twin_has_rows_or_panel(act, dtype):
    """FLAG | WIDE: the whole band borrowed from the 4-bit twin.  FLAG alone: the part of it that measured faster with both layouts resident
    (profiles/dense_int2_ab.log): rows form 5 .. 16 rows where N >= 8192 and K <= 4096, panel form from 256 rows and from 128 rows where N >= 8192."""
    for K, N, gs, Ms, kernel, wide in ((4096, 4096, 128, (5, 16, 64), "rows", True), (4096, 11008, 128, (128, 256), "panel", True), (4096, 4096, 64, (8, 33), "rows", True),
                                       (4096, 4096, 32, (16,), "rows", True), (4096, 4096, 64, (128,), "panel", True), (4096, 11008, 128, (65,), "panel", True),
                                       (4096, 11008, 128, (5, 8, 16), "rows", False), (4096, 11008, 128, (128, 256), "panel", False),
                                       (4096, 4096, 64, (256, 512), "panel", False), (1024, 8192, 128, (16,), "rows", False)):
        L, U, T4 = _layer(K, N, gs, dtype, act=act, wide=wide), _layer(K, N, gs, dtype, act=act, flag=False), _layer(K, N, gs, dtype, bits=4, act=act, flag=False)
        for M in Ms:
            d, d4 = _plan(L, M), _plan(T4, M)
            assert d4["kernel"] in ("rows", "panel"), (K, N, M, d4)                  # the borrowed rule: the 4-bit twin is served by that family
            assert d["path"] == "gemm" and d["kernel"] == kernel and d["body"] == "lowbit" and d["ksplit"] == 1 and d["perm"] == int(act), (K, N, gs, M, d)
            bm, cols = (16, 64) if kernel == "rows" else (64, 128)
            assert d["tiles"] == f"{-(-M // bm)}x{N // cols}" and d["waves"] == (8 if kernel == "panel" else min(8, K // 256)), d      # rows form: two chunks per wave at least
            assert "body" not in _plan(U, M) and _plan(U, M)["kernel"] not in ("rows", "panel")
            # the same route plan answers the workspace queries: nothing for a plain layer, the header + the permuted x for an act-order one
            want = _lib.WS_HEADER_BYTES + _a256(M * K * 2) if act else 0
            assert _ws(L, M) == want and int(_lib.load().gptq_workspace_bytes(ctypes.byref(L), M)) == want
        for M in (1, 2, 3, 4):                                                       # decode rows: the unflagged layer's plan, key for key
            assert _plan(L, M) == _plan(U, M) and _ws(L, M) == _ws(U, M)
    # FLAG alone outside its measured region (inside the twin's band): the unflagged plan, key for key; WIDE without FLAG means nothing
    for K, N, Ms in ((4096, 4096, (5, 16, 64, 65, 128)), (4096, 11008, (17, 32, 64, 65, 127)), (11008, 4096, (5, 64, 128)), (8192, 8192, (5, 16, 64, 65, 127))):
        L, U, W = _layer(K, N, 128, dtype, act=act), _layer(K, N, 128, dtype, act=act, flag=False), _layer(K, N, 128, dtype, act=act, flag=False, wide=True)
        for M in Ms:
            assert _plan(L, M) == _plan(U, M) == _plan(W, M) and _ws(L, M) == _ws(U, M) == _ws(W, M), (K, N, M, _plan(L, M))


def test_outside_the_bands_and_the_shapes_the_forms_take_the_plan_is_the_unflagged_one():
    lib = _lib.load()
    same = [dict(K=4096, N=4096 + 32), dict(K=4096, N=4096, gs=96), dict(K=4096 + 32, N=4096), dict(K=4096, N=4096, dtype=2), dict(K=4096, N=4096, copy=False)]
    for kw in same:
        if kw.get("copy") is False:
            L, U = _layer(**kw), _layer(**kw)
            L.tiled_cols, U.tiled_cols = FLAG, 0                                     # the flag without a copy means nothing (and is no error)
        else:
            L, U = _layer(wide=True, **kw), _layer(flag=False, **kw)
        for M in (1, 4, 5, 16, 64, 65, 128, 256, 1024):
            for knob in (0, ROWS_ON, PANEL_ON):
                try:
                    a = _plan(L, M, knob)
                except _lib.GptqError as e:
                    with pytest.raises(_lib.GptqError, match=re.escape(str(e))):
                        _plan(U, M, knob)
                    continue
                assert a == _plan(U, M, knob) and "body" not in a, (kw, M, knob, a)
                assert _ws(L, M, knob) == _ws(U, M, knob)
    # the knobs: any legal shape (here one below the planner's own band), either form; the OFF knobs keep the forms away
    L = _layer(512, 256)
    assert all("body" not in _plan(L, M) for M in (5, 16, 64, 65, 128))
    assert _plan(L, 1, ROWS_ON)["kernel"] == "rows" and _plan(L, 1, PANEL_ON)["kernel"] == "panel" and _plan(L, 700, ROWS_ON)["body"] == "lowbit"
    big = _layer(wide=True)
    assert "body" in _plan(big, 16) and "body" in _plan(big, 256) and "body" not in _plan(big, 16, 51) and "body" not in _plan(big, 256, 53)
    assert _plan(_layer(512, 192), 16, PANEL_ON) == _plan(_layer(512, 192, flag=False), 16, PANEL_ON)       # N % 128: no panel form
    assert _plan(_layer(512, 192), 16, ROWS_ON)["body"] == "lowbit"                                            # ... but N % 64: the rows form
    assert _plan(_layer(512, 256, gs=32), 16, PANEL_ON) == _plan(_layer(512, 256, gs=32, flag=False), 16, PANEL_ON)      # 32-wide groups: rows form only
    # a group of flagged layers in the band: no one-launch kernel takes it -- the single calls' needs
    arr = (ctypes.POINTER(_lib.GptqLayer) * 3)(*[ctypes.pointer(_layer(4096, n, wide=True)) for n in (4096, 4096, 11008)])
    assert int(lib.gptq_workspace_bytes_multi(arr, 3, 16)) == 0
    arr = (ctypes.POINTER(_lib.GptqLayer) * 2)(*[ctypes.pointer(_layer(4096, n, act=True, wide=True)) for n in (4096, 4096)])
    assert int(lib.gptq_workspace_bytes_multi(arr, 2, 16)) == _lib.WS_HEADER_BYTES + _a256(16 * 4096 * 2)


@pytest.mark.parametrize("bits", [3, 4, 8])
def test_the_flag_on_other_widths_changes_nothing(bits):
    lib = _lib.load()
    buf_a, buf_b = ctypes.create_string_buffer(1024), ctypes.create_string_buffer(1024)
    for K, N, gs, act in ((4096, 4096, 128, False), (4096, 11008, 128, True), (11008, 4096, 64, False), (1024, 1024, 32, False)):
        if bits == 3 and gs % 32:
            continue
        L, U = _layer(K, N, gs, bits=bits, act=act, wide=(K == 4096)), _layer(K, N, gs, bits=bits, act=act, flag=False)
        pa = (ctypes.POINTER(_lib.GptqLayer) * 2)(ctypes.pointer(L), ctypes.pointer(L))
        pb = (ctypes.POINTER(_lib.GptqLayer) * 2)(ctypes.pointer(U), ctypes.pointer(U))
        assert int(lib.gptq_workspace_bytes_max(ctypes.byref(L), 1100)) == int(lib.gptq_workspace_bytes_max(ctypes.byref(U), 1100))
        for M in range(1, 1101):
            assert lib.gptq_describe_plan(ctypes.byref(L), M, None, buf_a, 1024) == lib.gptq_describe_plan(ctypes.byref(U), M, None, buf_b, 1024) == 0
            assert buf_a.value == buf_b.value and b"body=" not in buf_a.value, (bits, K, N, M, buf_a.value)
            assert int(lib.gptq_workspace_bytes(ctypes.byref(L), M)) == int(lib.gptq_workspace_bytes(ctypes.byref(U), M))
            assert int(lib.gptq_workspace_bytes_multi(pa, 2, M)) == int(lib.gptq_workspace_bytes_multi(pb, 2, M))


# ---- no behaviour change without the flag -----------------------------------------------------------------------------------------------------------------
def test_unflagged_2_bit_layers_answer_as_the_parent_commit_did():
    want = json.load(open(os.path.join(ROOT, "tests", "golden", "plans_int2_parent.json")))
    assert len(want) == 24 and all(len(v["rows"]) == 13 for v in want.values())
    for c in GEN.cases():
        got = GEN.query(GEN.layer(*c))
        ref = want[GEN.key(*c)]
        assert got["max"] == ref["max"], GEN.key(*c)
        for M, row in ref["rows"].items():
            assert got["rows"][M] == row, (GEN.key(*c), M, got["rows"][M], row)


# ---- ABI ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_abi_is_unchanged_and_the_switches_default_to_off():
    from autogptq_amd.model_utils import autogptq_post_init
    from autogptq_amd.qlinear_mi355x import QuantLinear
    header = open(os.path.join(ROOT, "include", "gptq_mi355x.h")).read()
    assert "#define GPTQ_COPY_ROWS_INT2_WIDE 0x200" in header and _lib.COPY_ROWS_INT2_WIDE == 0x200 and _lib.copy_cols(16 | 0x300) == 16
    assert "#define GPTQ_COPY_ROWS_INT2 0x100" in header and "#define GPTQ_MI355X_ABI_VERSION 8" in header and "GPTQ_COPY_COLS(tiled_cols)" in header
    assert _lib.load().gptq_abi_version() == 8 and _lib.ABI_VERSION == 8
    assert ctypes.sizeof(_lib.GptqLayer) == 5 * 8 + 6 * 4 + 2 * 8 + 2 * 4 + 2 * 8
    assert _lib.COPY_ROWS_INT2 == 0x100 and _lib.copy_cols(16 | 0x100) == 16 == _lib.STRIP_COLS and _lib.copy_cols(0x100) == 0
    assert inspect.signature(autogptq_post_init).parameters["low_bit_rows"].default is False
    assert inspect.signature(QuantLinear.post_init).parameters["low_bit_rows"].default is None and QuantLinear.LOW_BIT_ROWS is False
    # tiled_cols of another strip width is still refused, with or without the flag
    for tc in (32, 32 | FLAG, 32 | FLAG | WIDE):
        L = _layer()
        L.tiled_cols = tc
        with pytest.raises(_lib.GptqError, match="tiled_cols"):
            _lib.describe_plan(L, 1)


# ---- the built library --------------------------------------------------------------------------------------------------------------------------------------
def test_no_new_kernel_and_the_low_bit_kernels_keep_their_budgets():
    from test_kernel_resources import _kernels
    ks = _kernels()
    assert len(ks) <= 1160, len(ks)
    rows = {n: v for n, v in ks.items() if "moe_rows_lowbit_kernel" in n}
    panel = {n: v for n, v in ks.items() if "moe_panel_lowbit_kernel" in n}
    assert len(rows) == 4 and len(panel) == 4, (sorted(rows), sorted(panel))
    for n, v in list(rows.items()) + list(panel.items()):
        assert not (v["spill"] or 0) and not (v["scratch"] or 0), (n, v)
    assert all((v["vgpr"] or 0) <= 128 for v in rows.values()) and all((v["vgpr"] or 0) <= 256 for v in panel.values())
    assert len({n for n in ks if "moe_rows_kernel" in n}) == 4 and len({n for n in ks if "moe_panel_kernel" in n}) == 4
    assert not any("gemm_rows_kernel" in n and "Li2E" in n.split("gemm_rows_kernel")[1][:12] for n in ks)      # no dense 2-bit instantiation


def test_in_flight_lint_is_clean_on_the_four_kernels_that_carry_the_dense_form():
    from test_kernel_resources import LLVM, MAGIC, SO
    tools = [os.path.join(LLVM, t) for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-objdump")]
    if not os.path.exists(SO) or not all(os.path.exists(t) for t in tools):
        pytest.skip("built library or ROCm LLVM tools not present")
    spec = importlib.util.spec_from_file_location("isa_inflight_lint", os.path.join(ROOT, "tools", "isa_inflight_lint.py"))
    lint = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(lint)
    seen = 0
    with tempfile.TemporaryDirectory() as d:
        fat = os.path.join(d, "fat.bin")
        subprocess.check_call([tools[0], f"--dump-section=.hip_fatbin={fat}", SO, os.path.join(d, "copy.so")])
        blob = open(fat, "rb").read()
        starts = [m.start() for m in re.finditer(re.escape(MAGIC), blob)]
        for i, a in enumerate(starts):
            chunk = blob[a:starts[i + 1] if i + 1 < len(starts) else len(blob)]
            fams = [f for f in ("moe_rows_lowbit_kernel", "moe_panel_lowbit_kernel") if f.encode() in chunk]
            if not fams:
                continue
            part, co = os.path.join(d, f"b{i}.bin"), os.path.join(d, f"co{i}.o")
            open(part, "wb").write(chunk)
            r = subprocess.run([tools[1], "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--input={part}", f"--output={co}"], capture_output=True)
            if r.returncode != 0 or not os.path.exists(co) or os.path.getsize(co) == 0:
                continue
            asm = subprocess.run([tools[2], "-d", "--no-show-raw-insn", co], capture_output=True, text=True).stdout
            for fam in fams:
                assert not lint.lint(asm, fam), lint.lint(asm, fam)[:5]
                for name, body in re.findall(rf"<(_Z\w*{fam}\w*Li2E\w*)>:\n(.*?)(?=\n[0-9a-f]+ <_Z|\Z)", asm, flags=re.S):
                    # the dense form's bias comes by a 2-byte load; the only dwordx4 loads stay the x DMAs
                    assert "global_load_dwordx2" in body and "global_load_dwordx4 v" not in body.replace("global_load_lds_dwordx4", ""), name
                    seen += 1
    assert seen == 4, seen


# ---- the dense forms' indexing, restated ----------------------------------------------------------------------------------------------------------------------
def _scales64(raw, dtype):
    """[..., 2] uint8 (little endian) -> float64 of the layer dtype's value."""
    u = raw[..., 0].astype(np.uint32) | (raw[..., 1].astype(np.uint32) << 8)
    if dtype == torch.float16:
        return u.astype(np.uint16).view(np.float16).astype(np.float64)
    return (u << np.uint32(16)).view(np.float32).astype(np.float64)


def _model_weights(form, Lq, dtype, mode):
    """W [K, N] in float64 as the dense form reads it off the decode copy (of the re-sequenced rows): workgroup (tile, column group) -> strips, lane (k-slot g,
    column r) of chunk c -> the lane's two words, MFMA step ks -> k = 128 c + 32 g + 8 ks + j, the group of (c, g) -> the record's scale and zero-point."""
    K, N, gs = Lq["K"], Lq["N"], Lq["group_size"]
    perm = O.sequential_permutation(Lq["g_idx"])
    w_seq = O.unpack_weights(Lq["qweight"], 2)[perm]
    tiled = O.decode_copy_weights(torch.from_numpy(O.pack_rows(w_seq.astype(np.uint32), 2).view(np.int32)), 2).numpy().view(np.uint32)      # [S, C, 4, 16, 2]
    cst = O.decode_copy_consts(Lq["qzeros"], Lq["scales"], mode, 2).numpy()                                                                # [S, G, 48]
    S, C = tiled.shape[:2]
    G = cst.shape[1]
    assert K % 128 == 0 and C == K // 128 and G == -(-K // gs)
    c_i, g_i = np.meshgrid(np.arange(C), np.arange(4), indexing="ij")
    if form == "rows":                                       # moe_rows_body.inc: gm = 0 (128 2^n or one group), 1 (64), 2 (32)
        assert N % 64 == 0
        per_wg = 4
        if gs >= 128:
            gshift = 31 if gs >= K else (gs // 128).bit_length() - 1
            grp = np.minimum(c_i >> gshift, G - 1)
        else:
            grp = 2 * c_i + (g_i >> 1) if gs == 64 else 4 * c_i + g_i
    else:                                                    # moe_panel_body.inc: 64-deep step kt = 2 c + (g >> 1), half = g & 1; group = min(kt >> gsh, G - 1)
        assert N % 128 == 0 and (gs >= K or gs % 64 == 0)
        per_wg = 8
        gsh = 30 if gs >= K else (gs // 64).bit_length() - 1
        grp = np.minimum((2 * c_i + (g_i >> 1)) >> gsh, G - 1)
    assert grp.max() == G - 1 and grp.min() == 0
    ex = _Exact()
    W = np.full((K, N), np.nan)
    hit = np.zeros((K, N), dtype=np.int32)
    for wg in range(S // per_wg):                            # column group of the workgroup -> its strips -> columns 16 strip + r
        for v in range(per_wg):
            s = wg * per_wg + v
            rec = cst[s][grp]                                # [C, 4, 48]
            scale = _scales64(rec[..., :32].reshape(C, 4, 16, 2), dtype)      # lane r: bytes 2 r, 2 r + 1
            z = rec[..., 32:48].astype(np.int64)             # lane r: byte 32 + r
            words = tiled[s]                                 # [C, 4, 16, 2]
            for ks in range(4):
                val = np.full((C, 4, 16, 8), np.nan)
                for zv in np.unique(z):
                    f = _frag2(ex, words, ks, int(zv))
                    val = np.where((z == zv)[..., None], f, val)
                k = (128 * c_i + 32 * g_i + 8 * ks)[..., None, None] + np.arange(8)[None, None, None, :]
                n = (16 * s + np.arange(16))[None, None, :, None]
                k, n = np.broadcast_arrays(k, n)
                W[k, n] = (scale[..., None] * val)
                np.add.at(hit, (k, n), 1)
    assert (hit == 1).all() and not np.isnan(W).any()        # every (k, n) read by exactly one (workgroup column group, strip, lane, step, element)
    return W, perm


def _tile_rows(form, M):
    """[(row0, rows, source row of every staged row)] per tile: rows past M repeat a row of the tile and are not stored."""
    bm = 16 if form == "rows" else 64
    out = []
    for t in range(-(-M // bm)):
        row0, rows = bm * t, min(bm, M - bm * t)
        if form == "rows":                                   # row r of the tile <- x[row0 + min(r, rows - 1)]
            src = [row0 + min(r, rows - 1) for r in range(bm)]
        else:                                                # DMA i, lane r8: LDS row 8 i + r8 <- row 8 min(i, imax) + (i >= imax ? min(r8, rlast) : r8)
            imax, rlast = (rows - 1) >> 3, (rows - 1) & 7
            src = [row0 + 8 * min(i, imax) + (min(r8, rlast) if i >= imax else r8) for i in range(8) for r8 in range(8)]
        out.append((row0, rows, src))
    return out


def _dense_cases():
    from test_gpu_dense_int2 import PANEL_CASES, ROWS_CASES
    return [("rows",) + c[:5] for c in ROWS_CASES] + [("panel",) + c[:5] for c in PANEL_CASES]


@pytest.mark.parametrize("case", _dense_cases(), ids=lambda c: f"{c[0]}-{c[1]}x{c[2]}g{c[3]}M{c[4]}{'act' if c[5] else ''}")
def test_dense_form_indexing_restated_against_the_oracle(case):
    form, K, N, gs, M, act = case
    for dtype in ((torch.float16, torch.bfloat16) if K <= 1536 else (torch.float16,)):
        Lq = O.random_quant_layer(K, N, 2, gs, act_order=act, seed=K + N + M, bias=True, dtype=dtype)
        mode = O.ZERO_NOWRAP if act and gs < K else O.ZERO_WRAP
        W, perm = _model_weights(form, Lq, dtype, mode)
        # the copy holds the re-sequenced rows: row i of W is the oracle's row perm[i], exactly (w - z exact, the scale applied in float64 on both sides)
        w = O.unpack_weights(Lq["qweight"], 2).astype(np.int64)
        z = O.unpack_zeros(Lq["qzeros"], 2, mode).astype(np.int64)
        g = Lq["g_idx"].numpy().astype(np.int64)
        W_or = Lq["scales"].double().numpy()[g] * (w - z[g])
        assert np.array_equal(W, W_or[perm])
        # tiles: every output row is stored by exactly one tile, from its own row of x; the rows past M re-read rows of their own tile
        x = (torch.rand(M, K, generator=torch.Generator().manual_seed(M)) - 0.5).to(dtype)
        xp = x.double().numpy()[:, perm]                     # the permute pre-pass (the identity for a plain layer)
        out = np.full((M, N), np.nan)
        stored = np.zeros(M, dtype=np.int32)
        for row0, rows, src in _tile_rows(form, M):
            assert all(row0 <= s < row0 + rows for s in src) and src[:rows] == list(range(row0, row0 + rows))
            acc = xp[src] @ W + Lq["bias"].double().numpy()
            out[row0:row0 + rows] = acc[:rows]
            stored[row0:row0 + rows] += 1
        assert (stored == 1).all()
        ref = O.forward_f64(x, Lq["qweight"], Lq["qzeros"], Lq["scales"], Lq["g_idx"], Lq["bias"], 2, mode).numpy()
        assert np.allclose(out, ref, rtol=1e-11, atol=1e-11 * float(np.abs(ref).max()))      # float64 on both sides: only the order of the K sums differs
