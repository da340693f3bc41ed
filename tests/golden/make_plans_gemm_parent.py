#!/usr/bin/env python3
"""Generator of tests/golden/plans_gemm_parent.json: what the library answers for dense calls over a grid that crosses every rule of plan_gemm
(csrc/gemm.hip) -- gptq_describe_plan's raw line or its error text, gptq_workspace_bytes_ex / _max / _multi_ex -- recorded from a build of the commit BEFORE
the planner was split into one function per rung (its parent), so that tests/test_gemm_plan_host.py can hold every later build to "no decision changed".
Host arithmetic on fake pointers: no GPU (no initialised device: the stream-K grid cap takes its 256-CU default, which is what an MI355X reports).

Recorded with (the file is copied next to a built checkout of the parent commit, e.g. a `git worktree` of it, and run there):

    python tests/golden/make_plans_gemm_parent.py --out plans_gemm_parent.json

It uses nothing the parent does not have.  Per layer: "max"; per (layer, row count): the full answers without tuning ("none": [line, workspace_bytes_ex,
workspace_bytes_multi_ex of [L, L]]) and ONE sha256 over the answers of the whole knob sweep ("knobs").  A hash that differs names the layer and the row count;
this generator run against both builds (--out, then diff with --full, which writes the sweep's answers instead of their hash) gives the difference."""
import argparse
import ctypes
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from autogptq_amd import _lib  # noqa: E402

F16, BF16, F32 = 0, 1, 2
FLAG, WIDE = 0x100, 0x200            # GPTQ_COPY_ROWS_INT2, GPTQ_COPY_ROWS_INT2_WIDE (in tiled_cols)
ODD = (4128, 4160, 32)               # N % 256 != 0 and K % 64 != 0: the 32-deep K step and no balanced tail
# (K, N, group_size, bits, dtype, copy, act-order, tiled_cols).  Not the full cross of the axes (the file would pass the size limit for committed files): every
# width, dtype, shape, {no copy, copy} and {plain, act-order} occurs, 4-bit fp16 -- the layers most rules were fitted on -- on every shape.
LAYERS = (
    [(K, N, 128, 4, F16, c, a, 16) for K, N in ((4096, 4096), (4096, 11008), (11008, 4096), (8192, 8192)) for c, a in ((0, 0), (1, 0), (1, 1))]
    + [(5120, 13824, 64, 4, BF16, 1, 0, 16), (5120, 13824, 64, 4, BF16, 0, 1, 16), (1024, 1024, 32, 4, F16, 1, 0, 16), (1024, 1024, 32, 4, BF16, 0, 1, 16),
       ODD + (4, F16, 0, 0, 16), ODD + (4, F16, 1, 1, 16), (4096, 11008, 128, 4, BF16, 1, 1, 16), (4096, 11008, 128, 4, BF16, 0, 0, 16)]
    + [s for b in (2, 3, 8) for s in ((4096, 11008, 128, b, F16, 0, 0, 16), (4096, 11008, 128, b, F16, 1, 0, 16), (11008, 4096, 128, b, F16, 1, 1, 16),
                                      ODD + (b, F16, 0, 0, 16), (8192, 8192, 128, b, BF16, 0, 1, 16))]
    + [(4096, 4096, 128, 4, F32, 0, 0, 16), (4096, 11008, 128, 3, F32, 0, 1, 16)]
    + [s for tc in (16 | FLAG, 16 | FLAG | WIDE) for s in ((4096, 11008, 128, 2, F16, 1, 0, tc), (8192, 8192, 128, 2, F16, 1, 1, tc), (4096, 4096, 128, 2, BF16, 1, 0, tc))]
)
# the thresholds of the rules and their neighbours; 767 / 768 / 1024 / 2176 / 2560: the balanced-tail cases, 2048 / 4096 / 8192: whole rounds
ROWS = (3, 4, 5, 8, 9, 16, 17, 32, 33, 64, 65, 96, 127, 128, 129, 256, 320, 384, 512, 767, 768, 1024, 2048, 2176, 2560, 4096, 8192)
MAX_ROWS = 8192
# name -> (path, ksplit, reserved[0..3]) of gptq_tuning_t (include/gptq_mi355x_lab.h)
KNOBS = {f"kernel{v}": (3, 0, (0, 0, v, 0)) for v in (1, 2, 3, 4, 5)}
KNOBS.update({f"variant{v}": (3, 0, (0, 0, 0, v)) for v in (1, 2, 3, 5, 6, 7) + tuple(range(40, 54))})
KNOBS.update({"bk32": (3, 0, (0, 32, 0, 0)), "bk32_auto": (0, 0, (0, 32, 0, 0))})
KNOBS.update({f"ksplit{v}": (3, v, (0, 0, 0, 0)) for v in (1, 2, 4)})
KNOBS.update({"rows_on_geom": (3, 0, (2, 2, 0, 50)), "panel_on_geom": (3, 0, (22, 0, 0, 52))})
KNOBS.update({f"auto_variant{v}": (0, 0, (0, 0, 0, v)) for v in (41, 44, 48, 50, 51, 53)})      # path = 0: the `path != 3 || knob == 0` clause
MULTI_KNOBS = ("kernel4", "kernel5", "variant50")        # the knobs the layer-group route decodes


def layer(K, N, gs, bits, dtype, copy, act, tiled_cols=16):
    L = _lib.GptqLayer()
    L.qweight = L.qzeros = L.scales = 0x1000
    L.K, L.N, L.bits, L.group_size, L.dtype, L.zero_mode = K, N, bits, gs, dtype, 0
    if act:
        L.g_idx = L.qweight_seq = L.perm = 0x1000
    if copy:
        L.qweight_tiled = L.qconst_tiled = 0x2000
        L.tiled_cols = tiled_cols
    return L


def tuning(knob):
    t = _lib.GptqTuning()
    t.path, t.ksplit = knob[0], knob[1]
    for i, v in enumerate(knob[2]):
        t.reserved[i] = v
    return t


def cases():
    return iter(LAYERS)


def key(K, N, gs, bits, dtype, copy, act, tiled_cols):
    return f"{K}x{N}-g{gs}-b{bits}-{('f16', 'bf16', 'f32')[dtype]}-{f'copy{tiled_cols:#x}' if copy else 'nocopy'}-{'act' if act else 'plain'}"


def _answer(lib, L, pair, M, tp, buf, multi):
    rc = lib.gptq_describe_plan(ctypes.byref(L), M, tp, buf, len(buf))
    out = [buf.value.decode() if rc == 0 else f"rc={rc} {lib.gptq_last_error().decode()}", int(lib.gptq_workspace_bytes_ex(ctypes.byref(L), M, tp))]
    if multi:
        out.append(int(lib.gptq_workspace_bytes_multi_ex(pair, 2, M, tp)))
    return out


def query(L, full=False):
    """{"max": gptq_workspace_bytes_max, "rows": {M: {"none": [line or error, workspace_bytes_ex, workspace_bytes_multi_ex], "knobs": sha256 of the sweep}}}"""
    lib = _lib.load()
    lib.gptq_workspace_bytes_ex.restype = lib.gptq_workspace_bytes_max.restype = lib.gptq_workspace_bytes_multi_ex.restype = ctypes.c_size_t
    out = {"max": int(lib.gptq_workspace_bytes_max(ctypes.byref(L), MAX_ROWS)), "rows": {}}
    pair = (ctypes.POINTER(_lib.GptqLayer) * 2)(ctypes.pointer(L), ctypes.pointer(L))
    buf = ctypes.create_string_buffer(1024)
    tunings = {name: tuning(knob) for name, knob in KNOBS.items()}
    for M in ROWS:
        sweep = [[name] + _answer(lib, L, pair, M, ctypes.byref(t), buf, name in MULTI_KNOBS) for name, t in tunings.items()]
        out["rows"][str(M)] = {"none": _answer(lib, L, pair, M, None, buf, True),
                               "knobs": sweep if full else hashlib.sha256(json.dumps(sweep).encode()).hexdigest()}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--full", action="store_true", help="the knob sweep's answers instead of their hash (to diff two builds; not the committed form)")
    a = ap.parse_args()
    doc = {key(*c): query(layer(*c), a.full) for c in cases()}
    assert len(doc) == len(LAYERS)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{len(doc)} layers x {len(ROWS)} row counts x (none + {len(KNOBS)} knobs) -> {a.out}")


if __name__ == "__main__":
    main()
