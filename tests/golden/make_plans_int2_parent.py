#!/usr/bin/env python3
"""Generator of tests/golden/plans_int2_parent.json: what the library answers for UNFLAGGED dense 2-bit layers -- gptq_describe_plan's raw line and
gptq_workspace_bytes_ex / _max / _multi -- recorded from a build of the commit BEFORE the opt-in GPTQ_COPY_ROWS_INT2 existed (its parent), so that
tests/test_dense_int2_host.py can hold every later build to "no behaviour change without the flag".  Host arithmetic on fake pointers: no GPU.

Recorded with (the file is copied next to a built checkout of the parent commit, e.g. a `git worktree` of it, and run there):

    python tests/golden/make_plans_int2_parent.py --out plans_int2_parent.json

It uses nothing the parent does not have (no flag, no new name).  cases(): six shapes x {no copy, copy} x {plain, act-order} x 13 row counts x the knobs
{none, ROWS_ON, PANEL_ON}; the test imports cases() and query() from here, so head is asked exactly what the parent was asked."""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from autogptq_amd import _lib  # noqa: E402

# (K, N, group_size, dtype enum): the 7B / 13B shapes of the A/B tool, a small layer with 32-wide groups, a bf16 one
SHAPES = [(4096, 4096, 128, 0), (4096, 11008, 128, 0), (11008, 4096, 128, 0), (5120, 13824, 64, 1), (8192, 8192, 128, 0), (1024, 1024, 32, 1)]
ROWS = (1, 2, 4, 5, 8, 16, 33, 64, 65, 128, 256, 512, 1024)
KNOBS = {"none": 0, "rows_on": 50, "panel_on": 52}          # tuning.path = 3, reserved[3] = GPTQ_LAB_VARIANT_ROWS_ON / PANEL_ON (include/gptq_mi355x_lab.h)
MAX_ROWS = 1024


def layer(K, N, gs, dtype, copy, act, tiled_cols=16, bits=2):
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
    if not knob:
        return None
    t = _lib.GptqTuning()
    t.path, t.reserved[3] = 3, knob
    return t


def cases():
    for K, N, gs, dtype in SHAPES:
        for copy in (False, True):
            for act in (False, True):
                yield K, N, gs, dtype, copy, act


def query(L):
    """{"max": gptq_workspace_bytes_max, "rows": {M: {knob: [describe line or error, workspace_bytes_ex], "multi": gptq_workspace_bytes_multi of [L, L]}}}"""
    lib = _lib.load()
    lib.gptq_workspace_bytes_ex.restype = lib.gptq_workspace_bytes_max.restype = lib.gptq_workspace_bytes_multi.restype = ctypes.c_size_t
    out = {"max": int(lib.gptq_workspace_bytes_max(ctypes.byref(L), MAX_ROWS)), "rows": {}}
    pair = (ctypes.POINTER(_lib.GptqLayer) * 2)(ctypes.pointer(L), ctypes.pointer(L))
    buf = ctypes.create_string_buffer(1024)
    for M in ROWS:
        row = {"multi": int(lib.gptq_workspace_bytes_multi(pair, 2, M))}
        for name, knob in KNOBS.items():
            t = tuning(knob)
            tp = ctypes.byref(t) if t is not None else None
            rc = lib.gptq_describe_plan(ctypes.byref(L), M, tp, buf, len(buf))
            line = buf.value.decode() if rc == 0 else f"rc={rc} {lib.gptq_last_error().decode()}"
            row[name] = [line, int(lib.gptq_workspace_bytes_ex(ctypes.byref(L), M, tp))]
        out["rows"][str(M)] = row
    return out


def key(K, N, gs, dtype, copy, act):
    return f"{K}x{N}-g{gs}-{'bf16' if dtype else 'f16'}-{'copy' if copy else 'nocopy'}-{'act' if act else 'plain'}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    doc = {key(*c): query(layer(*c)) for c in cases()}
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{len(doc)} layers x {len(ROWS)} row counts x {len(KNOBS)} knobs -> {a.out}")


if __name__ == "__main__":
    main()
