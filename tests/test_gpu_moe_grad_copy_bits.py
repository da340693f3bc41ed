"""GPU: the backward of 2-, 3- and 8-bit routed experts on their decode copy (gptq_moe_backward_ex with GPTQ_GRAD_ON_COPY | GPTQ_GRAD_COPY_ANY_BITS: the
grouped mode of grad_copy_kernel behind the other weight front-ends; opt-in through QuantMoEExperts.backward_on_copy = "any_bits").

Expert set, inputs, fp64 reference and bounds: those of tests/test_gpu_moe_grad_copy.py (E = 3, topk = 2, H = 384, I = 192 -- at 8 bits the last tile of the
down copies has ONE 64-k chunk inside I; T = 130: a full and a partial tile per expert)."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import test_gpu_moe_backward as B  # noqa: E402
import test_gpu_moe_grad_copy as C  # noqa: E402
from autogptq_amd import _lib  # noqa: E402
from test_gpu_moe import make_experts  # noqa: E402

pytestmark = pytest.mark.gpu
ANY = 5


def _run(q, *args, **kw):
    return C.run_copy(q, *args, flags=ANY, **kw)


@pytest.mark.parametrize("bits,act", [(3, False), (3, True), (8, False), (8, True), (2, False)], ids=["3-plain", "3-act", "8-plain", "8-act", "2-plain"])
def test_oracle_bounds_and_the_bits_of_the_rows_backward(monkeypatch, bits, act):
    dtype, low = torch.float16, bits < 4
    q = make_experts(C.E, C.H, C.I, bits, 64 if act else 128, act, dtype, seed=bits + 20, top_k=C.TOPK)
    q.backward_on_copy = "any_bits"
    q.post_init(backward=True, low_bit=low, low_bit_decode=low)
    assert q._backward_on_copy and q._decode_table is not None and q._grad_table is not None
    d = _lib.describe_moe_backward_plan_ex(q._moe, 130, C.TOPK, ANY)
    assert d["path"] == "grouped_backward_copy" and d["bits"] == bits and d["act"] == int(act), d
    assert _lib.describe_moe_backward_plan_ex(q._moe, 130, C.TOPK, 1)["copy_reason"] == "bits"
    args = C._inputs(130, dtype)
    rows, copy = B.run_backward(q, *args), _run(q, *args)
    assert torch.equal(rows[0], copy[0]), "dx"
    monkeypatch.setattr(B, "run_backward", _run)
    dx, dw = B.check_backward(q, *args)                  # dX and the router-weight gradient inside the propagated fp64 bounds
    assert torch.equal(dx, copy[0]) and torch.equal(dw, copy[1])
