"""CPU: the contract of the routed-expert entry layer of the C ABI, pinned string for string.  For host-built structs (tests/_moe_host_structs.py) and all
six families -- grouped, grouped backward, decode, shared decode, batch, prefill -- tests/golden/moe_entry_contract.json holds the full describe string and
the workspace byte count, and for every call a checker declines also the return code and the gptq_last_error() text of the family's forward entry point (a
declined forward returns before it reads a pointer or touches the GPU).  The cases: one struct per decline cause, two-fault structs that pin the ORDER of
the checks, and a matrix of accepted shapes.

The file is kept small: "strings" is a table, an answer is [0, describe string, workspace bytes] where the family accepts and [return code, last error]
where it declines -- the describe string of a declined call is "path=<none | per_expert> reason=<the error with ' ' and '=' as '_'>" and its workspace 0,
which expand() puts back -- and a case of the accepted matrix whose answers equal an earlier case's in full names that case instead.

The fixture was recorded from the revision before the six families' host-side entry code was folded into one checker (``python
tests/test_moe_entry_contract.py --record`` rewrites it from whatever library is built); the tests only ever read it.  Record again only for a change that is
meant to alter an answer, and review the JSON diff."""
import ctypes
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from autogptq_amd import _lib  # noqa: E402
from _moe_host_structs import PTR, drop_copy, expert, moe, shared  # noqa: E402

FIXTURE = os.path.join(ROOT, "tests", "golden", "moe_entry_contract.json")
F16, BF16, F32 = _lib.GPTQ_F16, _lib.GPTQ_BF16, _lib.GPTQ_F32
LOW = _lib.MOE_LOW_BIT | _lib.MOE_LOW_BIT_DECODE
BIG = 1 << 40          # a workspace size no plan exceeds

# family -> (describe symbol, workspace-bytes symbol, forward symbol)
FAMILIES = {
    "grouped": ("gptq_describe_moe_plan", "gptq_moe_workspace_bytes", "gptq_moe_forward"),
    "backward": ("gptq_describe_moe_backward_plan", "gptq_moe_backward_workspace_bytes", "gptq_moe_backward"),
    "decode": ("gptq_describe_moe_decode_plan", "gptq_moe_decode_workspace_bytes", "gptq_moe_decode_forward"),
    "shared": ("gptq_describe_moe_shared_decode_plan", "gptq_moe_shared_decode_workspace_bytes", "gptq_moe_shared_decode_forward"),
    "batch": ("gptq_describe_moe_batch_plan", "gptq_moe_batch_workspace_bytes", "gptq_moe_batch_forward"),
    "prefill": ("gptq_describe_moe_prefill_plan", "gptq_moe_prefill_workspace_bytes", "gptq_moe_prefill_forward"),
}


def answers(m, sh, T, topk):
    """{family: {"describe", "ws"} (+ {"rc", "err"} of the forward entry point where the describe string declines)} for one struct."""
    lib = _lib.load()
    mp = ctypes.byref(m) if m is not None else None
    sp = ctypes.byref(sh) if sh is not None else None
    out = {}
    for fam, (describe, ws_bytes, forward) in FAMILIES.items():
        head = (mp, sp) if fam == "shared" else (mp,)
        buf = ctypes.create_string_buffer(512)
        assert getattr(lib, describe)(*head, T, topk, buf, len(buf)) == 0
        rec = out[fam] = {"describe": buf.value.decode(), "ws": int(getattr(lib, ws_bytes)(*head, T, topk))}
        if rec["describe"].startswith(("path=none ", "path=per_expert ")):
            if fam == "backward":      # (moe, table, grad_table, x, idx, w, dout, T, topk, dx, dw, dgu_out, ws, ws_bytes, stream)
                rc = lib.gptq_moe_backward(mp, PTR, PTR, PTR, PTR, PTR, PTR, T, topk, PTR, PTR, None, PTR, BIG, None)
            else:                      # (moe, [shared,] table, x, idx, w, T, topk, out, h_out, ws, ws_bytes, stream)
                rc = getattr(lib, forward)(*head, PTR, PTR, PTR, PTR, T, topk, PTR, None, PTR, BIG, None)
            rec["rc"], rec["err"] = int(rc), lib.gptq_last_error().decode()
    return out


# ---------------------------------------------------------------------------------------------------------------- the declined structs
def _edited(proj, e, m=None, **fields):
    """A default struct with members of one expert's layer overwritten."""
    m = m or moe()
    for k, v in fields.items():
        setattr(expert(m, proj, e), k, v)
    return m


def _without(m, **members):
    for k, v in members.items():
        setattr(m, k, v)
    return m


def _no_copy(m, proj, e):
    drop_copy(expert(m, proj, e))
    return m


def _null_expert(m, proj, e):
    m._keep[1][proj][e] = ctypes.POINTER(_lib.GptqLayer)()
    return m


def _shared_edit(sh, i, **fields):
    for k, v in fields.items():
        setattr(sh._keep[i], k, v)
    return sh


# name -> () -> (moe or None, shared or None: the default shared expert of the struct's H, T, topk)
DECLINES = {
    # -- moe_check, in the order of its checks
    "moe_null": lambda: (None, None, 1, 2),
    "flags_unknown": lambda: (moe(flags=0x40), None, 1, 2),
    "flags_known_both": lambda: (moe(flags=LOW), None, 1, 2),                     # accepted: the two known bits
    "E_0": lambda: (_without(moe(E=1), E=0), None, 1, 2),
    "E_257": lambda: (_without(moe(E=1), E=257), None, 1, 2),
    "topk_0": lambda: (moe(), None, 1, 0),
    "topk_9": lambda: (moe(), None, 1, 9),
    "T_negative": lambda: (moe(), None, -1, 2),
    "T_5": lambda: (moe(), None, 5, 2),
    "T_65": lambda: (moe(), None, 65, 2),
    "rows_65536": lambda: (moe(), None, 8192, 8),
    "T_too_large": lambda: (moe(), None, 40000000, 8),
    "gate_null": lambda: (_without(moe(), gate=None), None, 1, 2),
    "up_null": lambda: (_without(moe(), up=None), None, 1, 2),
    "down_null": lambda: (_without(moe(), down=None), None, 1, 2),
    "gate0_null": lambda: (_null_expert(moe(), 0, 0), None, 1, 2),
    "gate0_bits_5": lambda: (_edited(0, 0, bits=5), None, 1, 2),
    "gate0_qweight_null": lambda: (_edited(0, 0, qweight=None), None, 1, 2),
    "fp32": lambda: (moe(dtype=F32), None, 1, 2),
    "bits_3": lambda: (moe(bits=3), None, 1, 2),
    "bits_2": lambda: (moe(bits=2), None, 1, 2),
    "bits_3_low_bit": lambda: (moe(bits=3, flags=_lib.MOE_LOW_BIT), None, 1, 2),
    "bits_3_low_bit_decode": lambda: (moe(bits=3, flags=_lib.MOE_LOW_BIT_DECODE), None, 1, 2),
    "bits_2_both_flags_T5": lambda: (moe(bits=2, flags=LOW), None, 5, 2),
    "H_96": lambda: (moe(H=96, I=512, gs=32), None, 1, 2),
    "I_320": lambda: (moe(H=256, I=320), None, 1, 2),                             # a multiple of 64, not of 128
    # -- moe_check_proj, per expert
    "expert_null": lambda: (_null_expert(moe(), 1, 3), None, 1, 2),
    "expert_scales_null": lambda: (_edited(2, 5, scales=None), None, 1, 2),
    "expert_shape": lambda: (_edited(1, 4, N=256), None, 1, 2),
    "expert_bits_differ": lambda: (_edited(0, 2, bits=8), None, 1, 2),
    "up_bits_differ_from_gate": lambda: (moe(up=dict(bits=8)), None, 1, 2),
    "down_bits_differ_from_gate": lambda: (moe(down=dict(bits=8)), None, 1, 2),
    "expert_group_size_differs": lambda: (_edited(2, 1, group_size=64), None, 1, 2),
    "expert_dtype_differs": lambda: (_edited(1, 6, dtype=BF16), None, 1, 2),
    "expert_zero_mode_differs": lambda: (_edited(0, 7, zero_mode=1), None, 1, 2),
    "expert_bias": lambda: (_edited(2, 3, bias=0x7000), None, 1, 2),
    "expert_epilogue": lambda: (_edited(0, 1, epilogue=_lib.EPI_SILU_MUL), None, 1, 2),
    "raw_act_order": lambda: (_edited(1, 2, g_idx=0x2000), None, 1, 2),
    "group_size_48": lambda: (moe(H=384, I=768, gs=48), None, 1, 2),
    "group_size_32": lambda: (moe(gs=32), None, 1, 2),                            # the prefill path's group rule
    "group_size_16": lambda: (moe(gs=16), None, 1, 2),                            # ... and everyone's
    "no_copy": lambda: (moe(copy=False), None, 1, 2),
    "one_expert_no_copy": lambda: (_no_copy(moe(), 2, 5), None, 1, 2),
    "copy_misaligned": lambda: (_edited(0, 3, qweight_tiled=0x5008), None, 1, 2),
    "gate_up_group_size": lambda: (moe(up=dict(gs=64)), None, 1, 2),
    "gate_up_zero_mode": lambda: (moe(up=dict(zero_mode=1)), None, 1, 2),
    "lds_fit": lambda: (moe(E=1, H=98304, I=128), None, 1, 2),
    "lds_fit_down": lambda: (moe(E=1, H=128, I=98304), None, 1, 2),
    # -- moe_shared_check on top of the decode check
    "shared_low_bit_routed": lambda: (moe(bits=3, flags=LOW), shared(bits=3), 1, 2),
    "shared_null": lambda: (moe(), False, 1, 2),
    "shared_flags": lambda: (moe(), _without(shared(), flags=1), 1, 2),
    "shared_reserved": lambda: (moe(), _without(shared(), reserved=1), 1, 2),
    "shared_up_null": lambda: (moe(), _without(shared(), up=None), 1, 2),
    "shared_Is_1056": lambda: (moe(), shared(Is=1056), 1, 2),
    "shared_layer_bits_5": lambda: (moe(), _shared_edit(shared(), 0, bits=5), 1, 2),
    "shared_shape": lambda: (moe(), _shared_edit(shared(), 1, K=512), 1, 2),
    "shared_bits_8": lambda: (moe(), shared(bits=8), 1, 2),
    "shared_down_bits_8": lambda: (moe(), shared(down=dict(bits=8)), 1, 2),
    "shared_dtype": lambda: (moe(), shared(dtype=BF16), 1, 2),
    "shared_bias": lambda: (moe(), _shared_edit(shared(), 2, bias=0x7000), 1, 2),
    "shared_up_no_copy": lambda: (moe(), shared(up=dict(copy=False)), 1, 2),
    "shared_group_size_48": lambda: (moe(H=384, I=768), shared(H=384, Is=768, gs=48), 1, 2),
    "shared_gate_up_group_size": lambda: (moe(), shared(up=dict(gs=64)), 1, 2),
    "shared_gate_w_misaligned": lambda: (moe(), _without(shared(), gate_w=0x1008), 1, 2),
    "shared_lds_fit": lambda: (moe(), shared(Is=98304), 1, 2),
    # -- two faults in one struct: which one is named pins the order of the checks
    "order_T5_bits3": lambda: (moe(bits=3), None, 5, 2),
    "order_shape_no_copy": lambda: (_no_copy(_edited(0, 4, N=256), 0, 4), None, 1, 2),
    "order_gate_up_group_size_down_bias": lambda: (_edited(2, 3, m=moe(up=dict(gs=64)), bias=0x7000), None, 1, 2),
    "order_flags_E0": lambda: (_without(moe(E=1, flags=0x40), E=0), None, 1, 2),
    "order_fp32_I320": lambda: (moe(I=320, dtype=F32), None, 1, 2),
    "order_bias_no_copy": lambda: (_no_copy(_edited(1, 2, bias=0x7000), 1, 2), None, 1, 2),
    "order_topk9_T_negative": lambda: (moe(), None, -1, 9),
    "order_group_size_32_no_copy": lambda: (moe(gs=32, copy=False), None, 1, 2),
    "order_up_expert_bits_gate_up_group_size": lambda: (_edited(1, 5, m=moe(up=dict(gs=64)), bits=8), None, 1, 2),
    "order_shared_T5_shared_null": lambda: (moe(), False, 5, 2),
    "order_shared_bits_no_copy": lambda: (moe(), shared(gate=dict(bits=8, copy=False)), 1, 2),
}


def build_decline(name):
    m, sh, T, topk = DECLINES[name]()
    if sh is None:
        sh = shared(H=expert(m, 0, 0).K if m is not None and m.gate else 256)
    return m, (sh or None), T, topk


# ---------------------------------------------------------------------------------------------------------------- the accepted matrix
SHAPES = ((8, 2, 256, 512), (60, 4, 2048, 1408), (8, 2, 4096, 14336))          # (E, topk, H, I)
TOKENS = (0, 1, 4, 5, 64, 65, 1000)
ACCEPTS = [(shape, dt, bits, act) for shape in SHAPES for dt in ("fp16", "bf16") for bits in (4, 8, 2, 3) for act in (False, True)]


def accept_id(case):
    (E, topk, H, I), dt, bits, act = case
    return f"E{E}_k{topk}_H{H}_I{I}-{dt}-b{bits}-{'act' if act else 'seq'}"


def build_accept(case):
    """(moe, shared, topk): 2- and 3-bit experts carry both low-bit flags; the shared expert is twice as wide as a routed one."""
    (E, topk, H, I), dt, bits, act = case
    kw = dict(bits=bits, dtype=F16 if dt == "fp16" else BF16, act=act)
    return moe(E, H, I, flags=LOW if bits in (2, 3) else 0, **kw), shared(H, 2 * I, **kw), topk


def accept_answers(case):
    m, sh, topk = build_accept(case)
    return {f"T{T}": answers(m, sh, T, topk) for T in TOKENS}


# ---------------------------------------------------------------------------------------------------------------- the fixture's encoding
DECLINE_PATH = {"grouped": "per_expert", "backward": "per_expert", "decode": "none", "shared": "none", "batch": "none", "prefill": "none"}


def compact(by_family, strings):
    """One struct's answers as the fixture holds them: a list in FAMILIES order (see the module docstring)."""
    out = []
    for fam in FAMILIES:
        rec = by_family[fam]
        if "rc" in rec:
            assert rec == expand([rec["rc"], 0], fam, [rec["err"]]), (fam, rec)          # the derived fields really are derived
            out.append([rec["rc"], strings.setdefault(rec["err"], len(strings))])
        else:
            out.append([0, strings.setdefault(rec["describe"], len(strings)), rec["ws"]])
    return out


def expand(entry, fam, strings):
    if entry[0] == 0:
        return {"describe": strings[entry[1]], "ws": entry[2]}
    err = strings[entry[1]]
    return {"describe": f"path={DECLINE_PATH[fam]} reason={err.replace(' ', '_').replace('=', '_')}", "ws": 0, "rc": entry[0], "err": err}


# ---------------------------------------------------------------------------------------------------------------- the tests
@pytest.fixture(scope="module")
def pinned():
    """The fixture, expanded to what answers() returns: {"declines": {name: {family: answer}}, "accepts": {case: {"T<n>": {family: answer}}}}."""
    with open(FIXTURE) as f:
        raw = json.load(f)
    strings = raw["strings"]
    one = lambda entries: {fam: expand(e, fam, strings) for fam, e in zip(FAMILIES, entries)}      # noqa: E731
    accepts = {}
    for case, byT in raw["accepts"].items():
        accepts[case] = accepts[byT] if isinstance(byT, str) else {f"T{T}": one(entries) for T, entries in zip(TOKENS, byT)}
    return {"declines": {name: one(entries) for name, entries in raw["declines"].items()}, "accepts": accepts}


def _same(got, want, where):
    for fam in FAMILIES:
        assert got[fam] == want[fam], (where, fam, got[fam], want[fam])


def test_the_fixture_covers_exactly_these_cases(pinned):
    assert sorted(pinned["declines"]) == sorted(DECLINES)
    assert sorted(pinned["accepts"]) == sorted(accept_id(c) for c in ACCEPTS)
    assert all(sorted(v) == sorted(f"T{T}" for T in TOKENS) for v in pinned["accepts"].values())


@pytest.mark.parametrize("name", sorted(DECLINES))
def test_declined_struct_answers_as_pinned(pinned, name):
    _same(answers(*build_decline(name)), pinned["declines"][name], name)


@pytest.mark.parametrize("case", ACCEPTS, ids=accept_id)
def test_accepted_matrix_answers_as_pinned(pinned, case):
    got, want = accept_answers(case), pinned["accepts"][accept_id(case)]
    for T in TOKENS:
        _same(got[f"T{T}"], want[f"T{T}"], (accept_id(case), T))


def test_the_fixture_pins_what_it_is_meant_to(pinned):
    """The fixture itself: every decline names a reason and an error code, every family declines and accepts somewhere, the two-fault structs name the
    first fault, and the matrix really holds accepted plans of every family."""
    d = pinned["declines"]
    for name, fams in d.items():
        for fam, rec in fams.items():
            if "rc" in rec:
                assert rec["rc"] in (1, 2, 3) and rec["ws"] == 0 and rec["err"] and " reason=" in rec["describe"], (name, fam, rec)
                assert rec["describe"].split(" reason=")[1] == rec["err"].replace(" ", "_").replace("=", "_"), (name, fam, rec)
    for fam in FAMILIES:
        assert any("rc" in fams[fam] for fams in d.values()) and any("rc" not in fams[fam] for fams in d.values()), fam
    first = {("order_T5_bits3", "decode"): "T = 5 tokens", ("order_shape_no_copy", "decode"): "expert 4 gate is [256 -> 256]",
             ("order_shape_no_copy", "batch"): "expert 4 gate is [256 -> 256]",
             ("order_gate_up_group_size_down_bias", "grouped"): "gate and up layers must share", ("order_gate_up_group_size_down_bias", "prefill"): "gate and up layers must share",
             ("order_flags_E0", "grouped"): "unknown flag bits", ("order_flags_E0", "backward"): "unknown flag bits", ("order_flags_E0", "decode"): "E = 0 experts",
             ("order_fp32_I320", "batch"): "fp32 experts", ("order_bias_no_copy", "decode"): "no bias", ("order_topk9_T_negative", "grouped"): "topk = 9",
             ("order_group_size_32_no_copy", "prefill"): "group_size 32", ("order_up_expert_bits_gate_up_group_size", "grouped"): "the up layers of all experts",
             ("order_shared_T5_shared_null", "shared"): "T = 5 tokens", ("order_shared_bits_no_copy", "shared"): "shared gate has 8 bits",
             ("lds_fit", "decode"): "do not fit the LDS", ("lds_fit_down", "decode"): "do not fit the LDS", ("shared_lds_fit", "shared"): "do not fit the LDS",
             ("copy_misaligned", "prefill"): "16-byte aligned", ("T_too_large", "grouped"): "is too large", ("rows_65536", "prefill"): "T topk = 65536 rows"}
    for (name, fam), text in first.items():
        assert text in d[name][fam].get("err", ""), (name, fam, d[name][fam])
    a = pinned["accepts"]
    took = {fam: sum(rec[fam]["describe"].startswith("path=" + word + " ") for byT in a.values() for rec in byT.values())
            for fam, word in (("grouped", "grouped"), ("backward", "grouped_backward"), ("decode", "decode"), ("shared", "decode_shared"), ("batch", "batch"),
                              ("prefill", "prefill"))}
    n = len(ACCEPTS)
    assert took == {"grouped": 7 * n, "backward": 7 * n, "decode": 3 * n, "shared": 3 * n // 2, "batch": 5 * n // 2, "prefill": 7 * n // 2}, took


def record():
    strings, first = {}, {}
    data = {"declines": {name: compact(answers(*build_decline(name)), strings) for name in sorted(DECLINES)}, "accepts": {}}
    for c in ACCEPTS:
        got = accept_answers(c)
        entries = [compact(got[f"T{T}"], strings) for T in TOKENS]
        data["accepts"][accept_id(c)] = first.get(json.dumps(entries), entries)
        first.setdefault(json.dumps(entries), accept_id(c))
    data["strings"] = list(strings)
    line = lambda v: json.dumps(v, separators=(",", ":"))      # noqa: E731  (one case, one string per line: a diff names what moved)
    parts = ["{" + ",\n".join(f"{json.dumps(k)}:{line(v)}" for k, v in data[sec].items()) + "}" for sec in ("declines", "accepts")]
    parts.append("[" + ",\n".join(line(v) for v in data["strings"]) + "]")
    with open(FIXTURE, "w") as f:
        f.write("{" + ",\n".join(f'"{sec}":\n{text}' for sec, text in zip(("declines", "accepts", "strings"), parts)) + "}\n")
    print(f"{FIXTURE}: {os.path.getsize(FIXTURE)} bytes, {len(data['declines'])} declined structs, {len(data['accepts'])} x {len(TOKENS)} accepted")


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: python tests/test_moe_entry_contract.py --record   (rewrites the fixture from the library that is built)")
    record()
