"""Fused callers of the hot path: q/k/v as one layer, gate/up as one layer with a SiLU*mul epilogue.

Both are the reference's own constructions:
* fused attention concatenates the packed q/k/v tensors along out_features into ONE QuantLinear
  (auto_gptq/nn_modules/fused_llama_attn.py:171-203) -- nothing new is needed in the kernels for that, a fused layer is
  an ordinary layer with N = N_q + N_k + N_v;
* the fused MLP computes  silu(x @ W_gate) * (x @ W_up)  in one kernel (fused_llama_mlp.py:157-242); here that is
  ``QuantLinear(..., epilogue="silu_mul")`` over the [gate | up] concatenation: for M <= 8 the matrix-core GEMV walks
  both halves in the same workgroup and writes the product (one launch, no [M, 2N] round trip), larger M stage
  y = [gate | up] in the workspace and run an elementwise pass.
"""
from __future__ import annotations

from typing import Sequence

import torch
import torch.nn as nn

from .qlinear_mi355x import GATED_ACT, MLP_ACT, QuantLinear


def fuse_quant_linears(layers: Sequence[QuantLinear], epilogue: str = "none") -> QuantLinear:
    """Concatenate quantized linears that read the same input along out_features.

    All layers must agree on in_features, bits, group_size, scales dtype and g_idx.  (With act-order every projection has
    its own g_idx; the reference's cuda backend then carries a 3*K-long g_idx, qlinear_cuda.py:300-312, and its exllama
    backend refuses, fused_llama_attn.py:176-183.  This backend refuses too.)
    """
    if len(layers) < 2:
        raise ValueError("need at least two layers to fuse")
    a = layers[0]
    for l in layers[1:]:
        if (l.infeatures, l.bits, l.group_size) != (a.infeatures, a.bits, a.group_size):
            raise ValueError("fused layers must share in_features, bits and group_size")
        if l.scales.dtype != a.scales.dtype:
            raise ValueError("fused layers must share the scales dtype")
        if (l.bias is None) != (a.bias is None):
            raise ValueError("either every fused layer has a bias or none has")
        if not torch.equal(l.g_idx.cpu(), a.g_idx.cpu()):
            raise ValueError("fused layers must share g_idx (act-order projections with different g_idx cannot be fused)")
        if l.zero_mode != a.zero_mode:
            raise ValueError("fused layers must share zero_mode")
    if epilogue in GATED_ACT and (len(layers) != 2 or layers[0].outfeatures != layers[1].outfeatures):
        raise ValueError(f"epilogue='{epilogue}' fuses exactly two layers (gate, up) of equal width")
    n_total = sum(l.outfeatures for l in layers)
    f = QuantLinear(a.bits, a.group_size, a.infeatures, n_total, a.bias is not None, weight_dtype=a.scales.dtype,
                    zero_mode=a.zero_mode, epilogue=epilogue)
    f.qweight = torch.cat([l.qweight for l in layers], dim=1).contiguous()
    f.qzeros = torch.cat([l.qzeros for l in layers], dim=1).contiguous()
    f.scales = torch.cat([l.scales for l in layers], dim=1).contiguous()
    f.g_idx = a.g_idx.clone()
    if a.bias is not None:
        f.bias = torch.cat([l.bias for l in layers], dim=0).contiguous()
    return f


def fuse_qkv(q: QuantLinear, k: QuantLinear, v: QuantLinear) -> QuantLinear:
    """One layer computing [q | k | v] (split the output with ``torch.split(y, (Nq, Nk, Nv), dim=-1)``)."""
    return fuse_quant_linears([q, k, v])


def fuse_gate_up(gate: QuantLinear, up: QuantLinear, act: str = "silu") -> QuantLinear:
    """One layer computing act(gate(x)) * up(x), act = 'silu' or 'gelu_tanh' (Gemma's GeGLU)."""
    if act not in MLP_ACT:
        raise ValueError(f"act must be 'silu' or 'gelu_tanh', got {act!r}")
    return fuse_quant_linears([gate, up], epilogue=MLP_ACT[act])


def gated_act_name(fn) -> "str | None":
    """The ``act`` of the fused MLP callers for an activation module of the host model, or None (not served: the module is left alone).
    'gelu_tanh' is the tanh approximation of GELU under any of its names -- transformers' GELUTanh / PytorchGELUTanh, ``gelu_new`` (NewGELUActivation: the
    same function written with tanh) and nn.GELU(approximate='tanh'); erf GELU is a different function and has no epilogue."""
    name = type(fn).__name__
    if name in ("SiLU", "SiLUActivation"):
        return "silu"
    if name in ("GELUTanh", "PytorchGELUTanh", "NewGELUActivation"):
        return "gelu_tanh"
    if isinstance(fn, nn.GELU) and fn.approximate == "tanh":
        return "gelu_tanh"
    return None


def plain_act_name(fn) -> "str | None":
    """The ungated epilogue ('relu', 'gelu', 'gelu_tanh') that computes an activation module of the host model, or None (not served: quick GELU, ReLU^2,
    clipped GELU, ...).  'gelu' is the erf form (transformers' GELUActivation, nn.GELU()); 'gelu_tanh' is every name gated_act_name knows for the tanh
    approximation.  BloomGelu and FastGELUActivation write the same expression with sqrt(2/pi) cut to 0.79788456 / 0.7978845608: in fp64 they differ from
    the epilogue's function by up to 2.6e-10 / 9.1e-13, not by rounding, so they are not mapped (tests/test_plain_act_host.py measures both)."""
    name = type(fn).__name__
    if name in ("ReLU", "ReLUActivation"):
        return "relu"
    if name == "GELUActivation" or (isinstance(fn, nn.GELU) and fn.approximate == "none"):
        return "gelu"
    if gated_act_name(fn) == "gelu_tanh":
        return "gelu_tanh"
    return None


# class name of the host model's module -> (its first linear, the attribute that holds its activation): the ungated MLPs, act(fc1(x) + b)
PLAIN_ACT_SITES = {
    "OPTDecoderLayer": ("fc1", "activation_fn"),
    "GPTNeoXMLP": ("dense_h_to_4h", "act"),
    "FalconMLP": ("dense_h_to_4h", "act"),
    "BloomMLP": ("dense_h_to_4h", "gelu_impl"),
    "GPTJMLP": ("fc_in", "act"),
    "CodeGenMLP": ("fc_in", "act"),
    "Starcoder2MLP": ("c_fc", "act"),
    "PhiMLP": ("fc1", "activation_fn"),
}


def inject_fused_act(model: nn.Module) -> int:
    """Fuse the activation of every ungated MLP of PLAIN_ACT_SITES into its first linear: where that linear is an mi355x QuantLinear with epilogue 'none'
    and its own g_idx and plain_act_name serves the activation, the linear gets the epilogue in place (no tensor is touched: state_dict() keys and storage
    stay) and the activation attribute becomes nn.Identity() -- the host forward runs as it is, one launch and one [M, 4H] round trip shorter at decode
    rows.  The original activation is kept in the module's __dict__ for remove_fused_act.  Returns the number of modules changed."""
    n = 0
    for mod in list(model.modules()):
        site = PLAIN_ACT_SITES.get(type(mod).__name__)
        if site is None or "_fused_act_undo" in mod.__dict__:
            continue
        lin, fn = getattr(mod, site[0], None), getattr(mod, site[1], None)
        act = plain_act_name(fn)
        if not isinstance(lin, QuantLinear) or act is None or lin.epilogue != "none" or lin.g_idx.numel() != lin.infeatures:
            continue
        _set_epilogue(lin, act)
        object.__setattr__(mod, "_fused_act_undo", fn)
        if isinstance(fn, nn.Module):
            setattr(mod, site[1], nn.Identity())
        else:                                       # a plain callable attribute
            object.__setattr__(mod, site[1], nn.Identity())
        n += 1
    return n


def remove_fused_act(model: nn.Module) -> int:
    """Undo inject_fused_act: epilogue 'none' again, the module's own activation object back in its attribute.  Returns the number of modules restored."""
    n = 0
    for mod in list(model.modules()):
        if "_fused_act_undo" not in mod.__dict__:
            continue
        fn = mod.__dict__.pop("_fused_act_undo")
        lin_name, act_name = PLAIN_ACT_SITES[type(mod).__name__]
        if act_name in mod.__dict__:
            del mod.__dict__[act_name]
        setattr(mod, act_name, fn)
        _set_epilogue(getattr(mod, lin_name), "none")
        n += 1
    return n


class _FusedQKVState:
    """y_q, y_k, y_v computed by ONE gptq_forward_multi call when the q_proj stand-in runs, handed to the k/v stand-ins."""

    def __init__(self, layers):
        self.layers = list(layers)
        self.src = None
        self.parts = None


class _QKVPart(nn.Module):
    """Stand-in for q_proj / k_proj / v_proj of an attention module whose forward calls them in that order on the same
    hidden_states (transformers' LlamaAttention.forward does): index 0 runs all three projections through
    ``forward_multi`` -- one launch for decode rows on plain layers, three ordinary calls otherwise (act-order, prefill) --
    and 1 / 2 return their results.  The three QuantLinears stay what they were: no concatenated copy of the packed tensors
    (the reference builds one, fused_llama_attn.py:171-203, and therefore cannot fuse act-order projections with different
    g_idx on its exllama path, :176-183; its cuda path carries a 3K-long g_idx, qlinear_cuda.py:300-312).  The host model's
    attention code is untouched, where the reference replaces the whole module (fused_llama_attn.py:18-135)."""

    def __init__(self, state: _FusedQKVState, index: int):
        super().__init__()
        self.index = index
        self._state = [state]                       # in a list: the shared state is not a submodule
        self.proj = state.layers[index]             # each stand-in owns its own projection: .to() / state_dict() keep working

    @staticmethod
    def _key(x):
        # Inference tensors (torch.inference_mode(): what the reference's generate() runs under, auto_gptq/modeling/_base.py:415-418) do not
        # track a version counter -- reading ._version raises there.  They cannot be modified in place outside inference mode either, so
        # storage + shape + dtype identifies the activation for the three back-to-back projection calls.
        ver = None if x.is_inference() else x._version
        return (x.data_ptr(), tuple(x.shape), x.dtype, ver)

    def forward(self, x):
        from .qlinear_mi355x import forward_multi
        st = self._state[0]
        if self.index == 0:
            st.src = self._key(x)
            st.parts = forward_multi(st.layers, x)
            return st.parts[0]
        # k_proj / v_proj: the same activation as q_proj saw?  Compared by storage, shape, dtype and version counter, not by object identity:
        # wrappers that re-wrap or move the input per call (accelerate's AlignDevicesHook, autocast) hand every projection its own tensor object.
        same = st.parts is not None and st.src == self._key(x)
        if not same:                                # a different input (or q_proj was never called): this projection on its own
            st.src = st.parts = None
            return self.proj(x)
        out = st.parts[self.index]
        if self.index == 2:
            st.src = st.parts = None                # do not keep activations alive between calls
        return out


class FusedGateUpMLP(nn.Module):
    """down(silu(gate(x)) * up(x)) (the role of FusedLlamaMLPForQuantizedModel, auto_gptq/nn_modules/fused_llama_mlp.py:131-306).
    Three mi355x QuantLinears: ONE C-ABI call (gptq_mlp_forward: gate and up in one launch for decode rows, SiLU*mul on fp32, down) over the
    three checkpoint layers as they are -- no concatenated copy of the packed tensors (the reference builds one), so nothing is held twice and
    per-projection act-order is allowed.  A non-quantized down projection: the [gate | up] layer with the SiLU*mul epilogue when gate and up
    share g_idx, else gate and up through ``forward_multi`` and an elementwise SiLU*mul.
    ``act``: 'silu' (Llama, Mistral, Qwen) or 'gelu_tanh' (Gemma's GeGLU) -- gptq_mlp_forward_act / the matching epilogue / the torch function."""

    def __init__(self, gate: QuantLinear, up: QuantLinear, down: nn.Module, act: str = "silu"):
        super().__init__()
        if act not in MLP_ACT:
            raise ValueError(f"act must be 'silu' or 'gelu_tanh', got {act!r}")
        self.act = act
        self.gate_up = None
        self.gate_proj, self.up_proj = gate, up
        if not isinstance(down, QuantLinear):
            try:
                self.gate_up = fuse_gate_up(gate, up, act).to(gate.qweight.device)
                self.gate_proj = self.up_proj = None
            except ValueError:                      # per-projection act-order
                pass
        self.down_proj = down

    def forward(self, x):
        if self.gate_up is not None:
            return self.down_proj(self.gate_up(x))
        if isinstance(self.down_proj, QuantLinear):               # three mi355x layers: one C-ABI call (gptq_mlp_forward)
            from .qlinear_mi355x import mlp_forward
            return mlp_forward(self.gate_proj, self.up_proj, self.down_proj, x, act=self.act)
        from .qlinear_mi355x import forward_multi
        g, u = forward_multi([self.gate_proj, self.up_proj], x)
        return self.down_proj(GATED_ACT[MLP_ACT[self.act]](g) * u)


def inject_fused_llama(model: nn.Module, fuse_attention: bool = True, fuse_mlp: bool = True) -> int:
    """Fuse q/k/v and gate/up of every Llama-style decoder block whose projections are mi355x QuantLinears (the reference's
    inject_to_model entry points, fused_llama_attn.py:137-231 / fused_llama_mlp.py:290-306).  Returns the number of fused modules."""
    n = 0
    for mod in list(model.modules()):
        if fuse_attention and all(isinstance(getattr(mod, a, None), QuantLinear) for a in ("q_proj", "k_proj", "v_proj")):
            q, k, v = mod.q_proj, mod.k_proj, mod.v_proj
            if q.infeatures == k.infeatures == v.infeatures and q.scales.dtype == k.scales.dtype == v.scales.dtype:
                st = _FusedQKVState((q, k, v))
                mod.q_proj, mod.k_proj, mod.v_proj = _QKVPart(st, 0), _QKVPart(st, 1), _QKVPart(st, 2)
                n += 1
        act = gated_act_name(getattr(mod, "act_fn", None)) if fuse_mlp else None
        if act is not None and all(isinstance(getattr(mod, a, None), QuantLinear) for a in ("gate_proj", "up_proj")) and hasattr(mod, "down_proj"):
            gate, up = mod.gate_proj, mod.up_proj
            if gate.infeatures == up.infeatures and gate.outfeatures == up.outfeatures and gate.bits == up.bits:
                fm = FusedGateUpMLP(gate, up, mod.down_proj, act)
                mod.forward = fm.forward
                if fm.gate_up is None:
                    # the fused caller only REFERENCES the three projections: it is kept out of the module tree (object.__setattr__), they stay
                    # registered once under their checkpoint names, and state_dict() of a fused model round-trips with the checkpoint layout
                    object.__setattr__(mod, "fused_mlp", fm)
                else:                               # non-quantized down: the concatenated [gate | up] copy replaces the two originals
                    mod.fused_mlp = fm
                    del mod.gate_proj, mod.up_proj
                n += 1
        if fuse_mlp and _inject_gate_up_proj(mod):
            n += 1
    return n


def _set_epilogue(layer: QuantLinear, epilogue: str) -> None:
    """Change the epilogue of an existing layer in place: no tensor is touched; a layer that was initialised is initialised again (its decode copy of a
    [gate | up] layer pairs the strips of the two halves: the C side decides per epilogue)."""
    was_initialised = layer._layer is not None
    layer.epilogue = epilogue
    layer._invalidate()
    if was_initialised:
        layer.post_init()


def _inject_gate_up_proj(mod: nn.Module) -> bool:
    """The MLP of Phi-3 / Phi-4 and of GLM-4's dense blocks: the checkpoint stores [gate | up] as ONE linear ``gate_up_proj`` and the forward is
    ``gate, up = y.chunk(2, -1); down(up * act(gate))`` -- what a layer with the matching gated epilogue computes.  The layer gets that epilogue in place
    (state_dict() keys and tensors unchanged) and the module's forward becomes ``down_proj(gate_up_proj(x))``; remove_fused_mlp undoes both."""
    gu = getattr(mod, "gate_up_proj", None)
    if not isinstance(gu, QuantLinear) or not hasattr(mod, "down_proj") or gu.epilogue != "none":
        return False
    act = gated_act_name(getattr(mod, "activation_fn", None)) or gated_act_name(getattr(mod, "act_fn", None))
    if act is None or gu.outfeatures % 64 != 0 or gu.g_idx.numel() != gu.infeatures:
        return False
    _set_epilogue(gu, MLP_ACT[act])

    def forward(x):
        return mod.down_proj(mod.gate_up_proj(x))
    object.__setattr__(mod, "_fused_gate_up_undo", mod.__dict__.get("forward"))      # an instance-level forward someone else bound (None: the class's)
    mod.forward = forward
    return True


def remove_fused_mlp(model: nn.Module) -> int:
    """Undo inject_fused_llama's work on ``gate_up_proj`` modules: epilogue 'none' again, the module's own forward again.  Returns the number of modules
    restored.  (The three-projection shape has no undo.)"""
    n = 0
    for mod in list(model.modules()):
        if "_fused_gate_up_undo" not in mod.__dict__:
            continue
        prev = mod.__dict__.pop("_fused_gate_up_undo")
        if prev is None:
            del mod.__dict__["forward"]
        else:
            mod.forward = prev
        _set_epilogue(mod.gate_up_proj, "none")
        n += 1
    return n


__all__ = ["fuse_quant_linears", "fuse_qkv", "fuse_gate_up", "inject_fused_llama", "remove_fused_mlp", "gated_act_name", "FusedGateUpMLP",
           "plain_act_name", "inject_fused_act", "remove_fused_act"]
