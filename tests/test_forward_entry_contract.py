"""CPU: the contract of the dense forward entry points of the C ABI, pinned string for string.  For host-built gptq_layer_t structs with dummy pointers
(tests/_moe_host_structs.py: the host-only queries never dereference them) tests/golden/forward_entry_contract.json holds

* single layer: the full gptq_describe_plan string -- or its return code and the gptq_last_error() text where it declines -- and gptq_workspace_bytes_ex,
  over bits x group size x dtype x act-order form x decode copy x M x shape under default tuning, and over every forced route (tuning.path, the
  tuning.reserved[2] kernels of path 3, the ROWS_ON / PANEL_ON lab knobs) on the fp16 shapes; gptq_workspace_bytes_max(L, 299) for a dozen layers;
* layer groups: gptq_workspace_bytes_multi_ex for q|k|v and gate|up groups (plain, act-order behind one shared perm pointer, act-order behind distinct
  ones) under default and forced tuning, and gptq_workspace_bytes_mlp for the gate|up groups with their down projection;
* two forward probes: gptq_forward_ex with tuning.path = 8 on a layer without a copy and tuning.path = 6 on an 8-bit act-order layer, return code and error text.
  Both are declined before the I/O check; x and out are NULL, so a route that got past the decline stops at that check and nothing can launch.  No other
  forward entry point is called from here.

The file is kept small by tables: "formats" holds the key lists of the describe strings, "strings" each distinct string as [format, values...] (an
error text as it is), "answers" each distinct [string, workspace bytes] -- [string, workspace bytes, return code] where describe declines, the string
is then the error text -- and "single_rows" / "group_rows" each distinct row: the answers (the byte counts) over the row's M list.  "single" and
"groups" name the row of every case.

The fixture was recorded from the revision before launch, workspace query and describe were made consumers of one route (``python
tests/test_forward_entry_contract.py --record`` rewrites it from whatever library is built); the tests only ever read it.  Record again only for a change
that is meant to alter an answer, and review the JSON diff.

Where the recorded revision's describe string, workspace number and the route gptq_forward_ex actually ran disagreed with one another, the route that
runs is what all three answer now; the fixture still holds the recorded answer, and DISAGREED below names every such case with both."""
import ctypes
import json
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from autogptq_amd import _lib  # noqa: E402
from _moe_host_structs import layer  # noqa: E402

FIXTURE = os.path.join(ROOT, "tests", "golden", "forward_entry_contract.json")
DTYPES = {"f16": _lib.GPTQ_F16, "bf16": _lib.GPTQ_BF16, "f32": _lib.GPTQ_F32}
MS = (1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 64, 65, 128, 129, 256, 512, 768, 2048, 4096)
MS_THIN = (1, 2, 4, 5, 8, 16, 64, 128, 512, 4096)            # the fp32 and raw act-order blocks
MS_FORCED = (1, 4, 5, 8, 16, 64, 128, 512)
SHAPES = ((4096, 4096, 0), (4096, 11008, 0), (11008, 4096, 0), (8192, 1024, 0), (5120, 13824, 0), (4096, 22016, _lib.EPI_SILU_MUL))      # (K, N, epilogue)
SHAPES_THIN = ((4096, 4096, 0), (4096, 11008, 0))
SHAPES_FORCED = SHAPES[:4]


def tuning(name):
    """"default" -> None; "p<path>", "p3r2_<reserved[2]>", "p3rows", "p3panel" -> a gptq_tuning_t."""
    if name == "default":
        return None
    t = _lib.GptqTuning()
    t.path = int(name[1])
    if "r2_" in name:
        t.reserved[2] = int(name.split("r2_")[1])
    if name.endswith("rows"):
        t.reserved[3] = _lib.LAB.VARIANT_ROWS_ON
    if name.endswith("panel"):
        t.reserved[3] = _lib.LAB.VARIANT_PANEL_ON
    return t


FORCED = tuple(f"p{p}" for p in (1, 2, 3, 4, 5, 6, 8)) + tuple(f"p3r2_{k}" for k in (1, 2, 3, 4, 5)) + ("p3rows", "p3panel")
FORCED_MULTI = ("p8", "p6", "p3r2_4", "p3r2_5", "p3rows")


def build(K, N, epi, bits, gs, dt, act, copy):
    """One layer, or None where ``copy`` is asked for and gptq_prepack_decode_bytes declines the layer.  act: "none", "raw" (g_idx alone), "seq"."""
    L = layer(K, N, bits=bits, gs=gs, dtype=DTYPES[dt], copy=False, act=act == "seq", epilogue=epi)
    if act == "raw":
        L.g_idx = 0x2000
    if copy:
        a, b = ctypes.c_size_t(), ctypes.c_size_t()
        if _lib.load().gptq_prepack_decode_bytes(ctypes.byref(L), ctypes.byref(a), ctypes.byref(b)) != 0:
            return None
        L.qweight_tiled, L.qconst_tiled, L.tiled_cols = 0x5000, 0x6000, _lib.STRIP_COLS
    return L


def single_rows():
    """{row name: (layer arguments, tuning name, M list)} of the single-layer part, in the fixture's order."""
    rows = {}
    for K, N, epi in SHAPES:
        for bits in (2, 3, 4, 8):
            for gs in (32, 128):
                for dt in DTYPES:
                    for act in ("none", "raw", "seq"):
                        thin = dt == "f32" or act == "raw"
                        if thin and (K, N, epi) not in SHAPES_THIN:
                            continue
                        for copy in (False, True):
                            args = (K, N, epi, bits, gs, dt, act, copy)
                            if build(*args) is not None:
                                rows[f"{K}x{N}{'-silu' if epi else ''}-b{bits}-g{gs}-{dt}-{act}-{'copy' if copy else 'rows'}"] = (args, "default", MS_THIN if thin else MS)
    for K, N, epi in SHAPES_FORCED:
        for bits in (3, 4, 8):
            for act in ("none", "seq"):
                for copy in (False, True):
                    for tn in FORCED:
                        rows[f"{K}x{N}-b{bits}-g128-f16-{act}-{'copy' if copy else 'rows'}-{tn}"] = ((K, N, epi, bits, 128, "f16", act, copy), tn, MS_FORCED)
    return rows


def single_answers(args, tn, ms):
    """Per M: (describe string, workspace bytes), or (error text, workspace bytes, return code) where describe declines."""
    lib, L, t = _lib.load(), build(*args), tuning(tn)
    tp = ctypes.byref(t) if t is not None else None
    out = []
    for M in ms:
        buf = ctypes.create_string_buffer(512)
        rc = lib.gptq_describe_plan(ctypes.byref(L), M, tp, buf, len(buf))
        ws = int(lib.gptq_workspace_bytes_ex(ctypes.byref(L), M, tp))
        out.append((buf.value.decode(), ws) if rc == 0 else (lib.gptq_last_error().decode(), ws, int(rc)))
    return out


WS_MAX = [(4096, 4096, 0, 4, 128, "f16", "none", False), (4096, 4096, 0, 4, 128, "f16", "none", True), (4096, 11008, 0, 4, 128, "f16", "seq", True),
          (11008, 4096, 0, 4, 128, "bf16", "none", True), (4096, 11008, 0, 8, 128, "f16", "none", False), (4096, 11008, 0, 3, 128, "f16", "seq", False),
          (4096, 4096, 0, 2, 128, "f16", "none", True), (4096, 11008, 0, 4, 128, "f32", "none", False), (4096, 11008, 0, 4, 128, "f16", "raw", False),
          (8192, 1024, 0, 4, 32, "f16", "none", True), (5120, 13824, 0, 4, 128, "f16", "seq", False), (4096, 22016, _lib.EPI_SILU_MUL, 4, 128, "f16", "none", True)]


def ws_max_answers():
    return [int(_lib.load().gptq_workspace_bytes_max(ctypes.byref(build(*a)), 299)) for a in WS_MAX]


# (row, M) -> (the answer the fixture was recorded with, the answer now): the recorded revision contradicted itself on these calls, the route that RAN stays
DISAGREED = {}
# 1. An act-order [gate | up] layer whose epilogue runs as a pass of its own, 1..4 rows: the inner call ran the x permute + the streamed GEMV on the
#    re-sequenced rows, and the workspace query counted it; describe skipped that step for layers with an epilogue and named the GEMV.
_gemv = "path=gemv kernel=mfma_generic ln=4 waves=16 u={u} ksplit=1 mt={mt} strips=1376 pair=0 perm=2 epilogue=separate deq=magic"
_stream = "path=gemv kernel=stream ln=8 waves={w} u={u} ksplit={ks} mt={mt} strips=688 pair=0 perm=2 epilogue=none"
for _row, _ms, _gu, _st in (("4096x22016-silu-b2-g32-f16-seq-rows", (2, 3, 4), 1, dict(w=8, u=2, ks=1)), ("4096x22016-silu-b2-g128-f16-seq-rows", (2, 3, 4), 1, dict(w=8, u=4, ks=1)),
                            ("4096x22016-silu-b8-g32-f16-seq-rows", (1, 2, 3, 4), 4, dict(w=4, u=2, ks=2)), ("4096x22016-silu-b8-g128-f16-seq-rows", (1, 2, 3, 4), 4, dict(w=4, u=2, ks=2))):
    for _M in _ms:
        _mt, _ws = (1, 2, 4, 4)[_M - 1], 65536 + 228352 * _M      # (the byte count is the same before and after)
        DISAGREED[_row, _M] = ((_gemv.format(u=_gu, mt=_mt), _ws), (_stream.format(mt=_mt, **_st), _ws))
# 2. tuning.path = 8 on an act-order layer with a decode copy, 5..8 rows: the decode-copy kernel ran (and describe named it), which needs no body; the
#    workspace query answered with the permuted x of the rows GEMM that the planner would have taken without the forced path.
_strips = "path=gemv kernel=strips ln=4 waves=8 u=4 ksplit=1 mt=8 strips=688 pair=0 perm=0 epilogue=none aligned=0"
for _row in ("4096x11008-b4-g128-f16-seq-copy-p8", "4096x11008-b8-g128-f16-seq-copy-p8"):
    for _M in (5, 8):
        DISAGREED[_row, _M] = ((_strips, 65536 + _M * 4096 * 2), (_strips, 0))


# ---------------------------------------------------------------------------------------------------------------- layer groups
GROUPS = {"qkv": (4096, (4096, 4096, 4096)), "gqa": (4096, (4096, 1024, 1024)), "gu7b": (4096, (11008, 11008)), "gu70b": (8192, (28672, 28672))}      # K, the Ns


def group_rows():
    """{row name: (group, bits, act, copy, tuning name)}; act: "none", "shared" (one perm pointer), "own" (distinct ones)."""
    return {f"{g}-b{bits}-{act}-{'copy' if copy else 'rows'}-{tn}": (g, bits, act, copy, tn)
            for g in GROUPS for bits in (3, 4, 8) for act in ("none", "shared", "own") for copy in (False, True) for tn in ("default",) + FORCED_MULTI}


def group_layers(g, bits, act, copy):
    K, Ns = GROUPS[g]
    Ls = [build(K, N, 0, bits, 128, "f16", "seq" if act != "none" else "none", copy) for N in Ns]
    if act == "own":
        for i, L in enumerate(Ls):
            L.perm = 0x4000 + 0x100 * i
    return Ls


def group_answers(g, bits, act, copy, tn):
    """Per M: gptq_workspace_bytes_multi_ex, and under default tuning for a gate|up group also gptq_workspace_bytes_mlp with the down projection."""
    lib, Ls, t = _lib.load(), group_layers(g, bits, act, copy), tuning(tn)
    arr = (ctypes.POINTER(_lib.GptqLayer) * len(Ls))(*[ctypes.pointer(L) for L in Ls])
    out = [int(lib.gptq_workspace_bytes_multi_ex(arr, len(Ls), M, ctypes.byref(t) if t is not None else None)) for M in MS]
    if tn == "default" and g.startswith("gu"):
        K, Ns = GROUPS[g]
        down = build(Ns[0], K, 0, bits, 128, "f16", "seq" if act != "none" else "none", copy)
        out += [int(lib.gptq_workspace_bytes_mlp(ctypes.byref(Ls[0]), ctypes.byref(Ls[1]), ctypes.byref(down), M)) for M in MS]
    return out


# ---------------------------------------------------------------------------------------------------------------- the two forward probes
PROBES = {"path8_no_copy": ((4096, 4096, 0, 4, 128, "f16", "none", False), "p8"), "path6_int8": ((4096, 4096, 0, 8, 128, "f16", "seq", False), "p6")}


def probe_answer(name):
    """gptq_forward_ex with NULL x and out (see the module docstring): [return code, error text]."""
    args, tn = PROBES[name]
    lib, L, t = _lib.load(), build(*args), tuning(tn)
    rc = lib.gptq_forward_ex(ctypes.byref(L), None, None, 1, None, 0, None, ctypes.byref(t))
    return [int(rc), lib.gptq_last_error().decode()]


# ---------------------------------------------------------------------------------------------------------------- the fixture's encoding
def pack_string(s, formats):
    """A describe string "k=v k=v ..." as [index of its key list in ``formats``, values...] (numbers as numbers); any other text as it is."""
    toks = [t.partition("=") for t in s.split(" ")]
    if not s.startswith("path=") or not all(sep and v for _, sep, v in toks):
        return s
    keys = [k for k, _, _ in toks]
    if keys not in formats:
        formats.append(keys)
    packed = [formats.index(keys)] + [int(v) if v.isdigit() and str(int(v)) == v else v for _, _, v in toks]
    assert unpack_string(packed, formats) == s, s
    return packed


def unpack_string(e, formats):
    return e if isinstance(e, str) else " ".join(f"{k}={v}" for k, v in zip(formats[e[0]], e[1:]))


def split_name(name):
    """Row name -> (section key, key inside the section): single rows by shape, bits, group size and dtype; group rows by group and bits."""
    cut = re.search(r"-(none|raw|seq|shared|own)-", name).start()
    return name[:cut], name[cut + 1:]


@pytest.fixture(scope="module")
def pinned():
    """The fixture with every table put back: {"single": {row: single_answers()}, "groups": {row: group_answers()}, "ws_max": [...], "probes": {...}}."""
    with open(FIXTURE) as f:
        raw = json.load(f)
    strings = [unpack_string(e, raw["formats"]) for e in raw["strings"]]
    answers = [(strings[a[0]],) + tuple(a[1:]) for a in raw["answers"]]
    single = {f"{sec}-{key}": [answers[i] for i in raw["single_rows"][r]] for sec, rows in raw["single"].items() for key, r in rows.items()}
    groups = {f"{sec}-{key}": raw["group_rows"][r] for sec, rows in raw["groups"].items() for key, r in rows.items()}
    return {"single": single, "groups": groups, "ws_max": raw["ws_max"], "probes": raw["probes"]}


# ---------------------------------------------------------------------------------------------------------------- the tests
def test_the_fixture_covers_exactly_these_cases(pinned):
    rows = single_rows()
    assert sorted(pinned["single"]) == sorted(rows)
    assert all(len(pinned["single"][name]) == len(ms) for name, (_, _, ms) in rows.items())
    assert sorted(pinned["groups"]) == sorted(group_rows())
    assert len(pinned["ws_max"]) == len(WS_MAX) and sorted(pinned["probes"]) == sorted(PROBES)
    assert os.path.getsize(FIXTURE) < 150 * 1024


@pytest.mark.parametrize("shape", [f"{K}x{N}{'-silu' if epi else ''}-" for K, N, epi in SHAPES])
@pytest.mark.parametrize("forced", (False, True), ids=("default", "forced"))
def test_single_layer_answers_as_pinned(pinned, shape, forced):
    n = 0
    for name, (args, tn, ms) in single_rows().items():
        if name.startswith(shape) and (tn != "default") == forced:
            got, want = single_answers(args, tn, ms), pinned["single"][name]
            for M, g, w in zip(ms, got, want):
                if (name, M) in DISAGREED:
                    assert w == DISAGREED[name, M][0], (name, M, w)      # the fixture is the recorded one
                    w = DISAGREED[name, M][1]
                assert g == w, (name, M, g, w)
            n += 1
    assert n or forced


def test_workspace_max_as_pinned(pinned):
    assert ws_max_answers() == pinned["ws_max"]


@pytest.mark.parametrize("g", sorted(GROUPS))
def test_layer_group_answers_as_pinned(pinned, g):
    for name, args in group_rows().items():
        if args[0] == g:
            got, want = group_answers(*args), pinned["groups"][name]
            assert got == want, (name, [(M, a, b) for M, a, b in zip(MS + MS, got, want) if a != b])


@pytest.mark.parametrize("name", sorted(PROBES))
def test_forward_probe_declines_as_pinned(pinned, name):
    assert probe_answer(name) == pinned["probes"][name]


def test_the_fixture_pins_what_it_is_meant_to(pinned):
    """The fixture itself: every kernel name the describe string can print occurs, forced routes decline somewhere with a message, the group rows hold
    queries with and without a body, and both probes are declines issued before the I/O check."""
    kernels = set()
    for row in pinned["single"].values():
        for e in row:
            if len(e) == 2:
                kernels.add(e[0].split(" kernel=")[1].split(" ")[0])
            else:
                assert e[2] in (2, 3) and e[0], e
    assert kernels == {"mfma", "mfma_generic", "generic", "strips", "stream", "stream64", "strip16", "skinny64", "mid", "rows", "panel", "tiled", "wide",
                       "wide_copy", "wide_sk", "f32_mfma"}, kernels
    assert any(len(e) == 3 and "retired" in e[0] for row in pinned["single"].values() for e in row)
    flat = [b for row in pinned["groups"].values() for b in row]
    assert 0 in flat and any(b > _lib.WS_HEADER_BYTES for b in flat)
    assert pinned["probes"]["path8_no_copy"][0] == 3 and "tuning.path = 8" in pinned["probes"]["path8_no_copy"][1]
    assert pinned["probes"]["path6_int8"][0] == 3 and "tuning.path = 6" in pinned["probes"]["path6_int8"][1]


def record():
    formats, strings, answers = [], {}, {}
    line = lambda v: json.dumps(v, separators=(",", ":"))      # noqa: E731  (one row, one string per line: a diff names what moved)

    def table(answers_by_row):
        """(the distinct rows, {section: {key: index of the row}}) of one part."""
        rows, names = {}, {}
        for name, row in answers_by_row.items():
            sec, key = split_name(name)
            names.setdefault(sec, {})[key] = rows.setdefault(line(row), len(rows))
        return "[" + ",\n".join(rows) + "]", "{" + ",\n".join(f"{json.dumps(k)}:{line(v)}" for k, v in names.items()) + "}"

    single = {name: [answers.setdefault((strings.setdefault(a[0], len(strings)),) + tuple(a[1:]), len(answers)) for a in single_answers(*case)]
              for name, case in single_rows().items()}
    single_table, single_names = table(single)
    group_table, group_names = table({name: group_answers(*args) for name, args in group_rows().items()})
    packed = [pack_string(s, formats) for s in strings]
    parts = {"single": single_names, "single_rows": single_table, "groups": group_names, "group_rows": group_table,
             "ws_max": line(ws_max_answers()), "probes": line({name: probe_answer(name) for name in PROBES}),
             "answers": "[" + ",\n".join(line(list(a)) for a in answers) + "]", "strings": "[" + ",\n".join(line(e) for e in packed) + "]",
             "formats": "[" + ",\n".join(line(f) for f in formats) + "]"}
    with open(FIXTURE, "w") as f:
        f.write("{" + ",\n".join(f'"{sec}":\n{text}' for sec, text in parts.items()) + "}\n")
    print(f"{FIXTURE}: {os.path.getsize(FIXTURE)} bytes, {sum(len(r) for r in single.values())} single-layer cases in {len(single)} rows, "
          f"{len(strings)} strings, {len(group_rows())} group rows")


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: python tests/test_forward_entry_contract.py --record   (rewrites the fixture from the library that is built)")
    record()
