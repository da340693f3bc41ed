"""GPU: what ``QuantMoEExperts.post_init`` settles, pinned answer for answer against tests/golden/moe_post_init_contract.json.

The fixture was recorded (tools/record_moe_post_init_contract.py, which also holds the cases and the ``observe`` this test replays them with) from the
revision before post_init was restructured around one table of the routed copy paths: 898 cases over 2, 3, 4 and 8 bits on E = 2, top_k = 2,
H = 256, I = 512 experts -- every combination of the seven switches at g128 (backward on four of them), ten decline rows (group sizes 32, 64, 48 and
one group, I = 192, H = 192, fp32, top_k = 9, bf16 as the control, and H = 65536: the one row the metadata pre-checks pass and the decode plan declines
once the copies are built, so the one that goes round the settle loop) x nine switch sets, and the four ``*_tokens`` tunables on the everything-on 3- and
4-bit modules.  No row was dropped: the constructor takes group size 48.  Per case and once more after ``_invalidate()`` + ``_ensure_init()``: the
warnings, the two switch attributes, decode_copy_bytes, the tables, the structs' flags, the layers' copies, plan(T) and workspace_bytes(T) at
T = 1, 4, 5, 64, 65, 300, backward_workspace_bytes(300) and the scratch autogptq_post_init reserves at max_input_length 3, 40, 300 -- here: the largest
workspace_bytes over ``workspace_token_counts(rows)``, in the fixture: over the token counts the recorded revision assembled from its expert_* keywords.

Everything is compared for equality.  The one allowance -- a warning the recorded revision said twice within one post_init (it re-entered itself after
a declined plan) may be said once -- is not used by any recorded case: no recorded warning list holds a repeat, and the lists are equal as they are.

The recorded revision did not contradict itself in any case: the state after a re-initialisation equals the state after post_init everywhere.  Sixteen
cases warn again at re-initialisation (backward=True on experts the backward plan declines; low_bit_decode=True on 2- / 3-bit experts whose decode copy
the pre-check declines): those switches are replayed as asked, and so they are here.

Measured on the MI355X: recording takes 1.0 / 0.5 / 0.6 / 0.8 s for 2 / 3 / 4 / 8 bits (the first with the first-use costs), a width of this test
0.5 - 1.0 s."""
import json
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.record_moe_post_init_contract import BITS, FIXTURE, cases, make_experts, observe  # noqa: E402

pytestmark = pytest.mark.gpu


def _unique(messages):
    return list(dict.fromkeys(messages))


@pytest.mark.parametrize("bits", BITS)
def test_post_init_settles_what_it_always_did(bits):
    with open(FIXTURE) as f:
        doc = json.load(f)
    assert doc["dropped_rows"] == []
    built, wrong, checked = {}, [], 0
    for name, row, on, tunables in cases(bits):
        if row not in built:
            built[row] = make_experts(bits, row, "cuda:0")
        got = observe(built[row], on, tunables, lambda q, rows, on: q.workspace_token_counts(rows))
        want = doc["cases"][f"{bits}/{name}"]
        want = [doc["warnings"][want[0]], doc["states"][want[1]], doc["warnings"][want[2]], doc["states"][want[3]]]
        assert got[0] == want[0] or _unique(got[0]) == _unique(want[0]) and len(got[0]) < len(want[0]), (name, got[0], want[0])
        assert got[2] == want[2], (name, got[2], want[2])
        for phase in (1, 3):
            state = json.loads(json.dumps(got[phase]))          # (as the fixture holds it: tuples as lists)
            if state != want[phase]:
                wrong.append((name, phase, {k: (v, want[phase].get(k)) for k, v in state.items() if v != want[phase].get(k)}))
        checked += 1
    assert not wrong, wrong[:5]
    assert checked == len([k for k in doc["cases"] if k.startswith(f"{bits}/")]) == len(cases(bits))
