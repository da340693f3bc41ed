#!/usr/bin/env python3
"""Golden fixture for the reference's ``GeneralQuantLinear`` shim (auto_gptq/nn_modules/qlinear/__init__.py:4-56), which wraps ANY backend's
QuantLinear by reading its attributes and buffers.  The shim is loaded by file path and run (on CPU) around this backend's QuantLinear seen
through a proxy that logs every attribute the shim asks for; what it read, what it found, and how the wrapper it built relates to the
wrapped module are stored as a list of names and recorded results (shim_general_quant_linear.json).  tests/test_end_to_end.py checks
the backend against that record.

Usage:  GPTQ_REFERENCE=<reference tree> python tests/golden/make_golden_shim.py
"""
import importlib.util
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))


class Recorder:
    """Stands in for the wrapped module: every attribute read goes to the real one and is logged (hasattr included)."""

    def __init__(self, inner):
        object.__setattr__(self, "_inner", inner)
        object.__setattr__(self, "_asked", [])

    def __getattr__(self, name):
        self._asked.append(name)
        return getattr(self._inner, name)


def main():
    ref = os.environ.get("GPTQ_REFERENCE")
    if not ref:
        sys.exit("set GPTQ_REFERENCE to the reference tree")
    from autogptq_amd import QuantLinear

    spec = importlib.util.spec_from_file_location("ref_qlinear_shim", os.path.join(ref, "auto_gptq/nn_modules/qlinear/__init__.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)

    K, N = 256, 512
    q = QuantLinear(4, 128, K, N, True)
    rec = Recorder(q)
    g = mod.GeneralQuantLinear(rec)
    asked = list(dict.fromkeys(rec._asked))
    present = [n for n in asked if hasattr(q, n)]
    scalars = {n: getattr(q, n) for n in present if isinstance(getattr(q, n), (bool, int, float, str))}
    shared = [n for n in present if isinstance(getattr(q, n), torch.Tensor) and getattr(g, n, None) is getattr(q, n)]
    buffers = sorted(n for n, _ in g.named_buffers(recurse=False))
    tensors = [n for n in present if isinstance(getattr(q, n), torch.Tensor)]
    linear_data = {f: s for f in ("weight", "bias") for s in tensors if getattr(g, f).data_ptr() == getattr(q, s).data_ptr()}

    class Holder(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.a = QuantLinear(4, 128, K, N, True)
            self.b = torch.nn.Linear(4, 4)
    h = Holder()
    mod.GeneralQuantLinear.inject_to_model(h, QuantLinear)
    out = {
        "what": "the reference's GeneralQuantLinear (auto_gptq/nn_modules/qlinear/__init__.py) run around QuantLinear(4, 128, %d, %d, bias=True)" % (K, N),
        "attributes_read": asked,                       # in the order the shim reads them (optional ones through hasattr)
        "attributes_found": present,                    # ... and which of them the backend had
        "scalars": scalars,                             # their values, copied onto the wrapper
        "tensors_shared": shared,                       # the wrapper holds the SAME tensor objects
        "wrapper_buffers": buffers,                     # registered as buffers of the wrapper
        "linear_data": linear_data,                     # nn.Linear field of the wrapper -> the wrapped module's tensor behind its .data
        "linear_features": {"in_features": g.in_features, "out_features": g.out_features},
        "forward_is_wrapped_forward": g.forward == q.forward,
        "inject_to_model": {"a": type(h.a).__name__, "b": type(h.b).__name__},
    }
    with open(os.path.join(HERE, "shim_general_quant_linear.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
