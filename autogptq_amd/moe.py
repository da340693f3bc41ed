"""Quantised mixture-of-experts layers: the experts of a Mixtral block (the reference quantises them as per-expert linears,
``block_sparse_moe.experts.{e}.w1 / w3 / w2``, auto_gptq/modeling/mixtral.py) as ONE routed call into the HIP library.

* ``QuantMoEExperts``   drop-in for a transformers-5 ``MixtralExperts`` (3-D ``gate_up_proj`` / ``down_proj``): same
                        ``forward(hidden_states, top_k_index, top_k_weights)``; its children are per-expert ``QuantLinear``s whose
                        state_dict keys are ``<path>.{e}.w1 / w3 / w2.{qweight, qzeros, scales, g_idx}``
* ``moe_forward``       the grouped path (gptq_moe_forward: routing table, grouped W1 / W3 + silu * mul, grouped W2, combine -- four
                        launches, no host round trip, capturable), the decode path for 1..4 tokens when the experts carry a decode copy
                        (gptq_moe_decode_forward: two launches on streaming kernels, the expert chosen on the device, capturable), the batch
                        path for 5..64 tokens when opted in (gptq_moe_batch_forward: the grouped formulas on the decode copy, 16-row tiles of
                        one expert over the whole K, capturable), the prefill path for 65 tokens and more when opted in
                        (gptq_moe_prefill_forward: the same formulas on the decode copy, 64-row panels of one expert over the whole K,
                        capturable), or the per-expert composition of differentiable ``QuantLinear`` calls
* ``moe_route``         the router in front of the experts as ONE launch (gptq_moe_router: logits, softmax, top-k with a written tie rule and the
                        optional renormalisation; dense fp16 / bf16 weight, no workspace, capturable); the torch composition for what it declines
* ``moe_route_grouped`` the sigmoid / group-limited router of DeepSeek-V3 and GLM-4 MoE blocks as ONE launch (gptq_moe_router_grouped: fp32 logits, sigmoid,
                        correction bias, group choice, top-k, renormalisation and scaling); the transformers composition for what it declines
* ``inject_fused_router`` / ``remove_fused_router``   bind ``moe_route`` as the forward of a model's softmax-top-k routers (Mixtral, Qwen2-MoE, Qwen3-MoE) and
                        ``moe_route_grouped`` as that of its grouped-sigmoid routers (DeepSeek-V3, GLM-4 MoE), on the instances: classes, parameters,
                        state-dict keys, hooks and transformers' output recorders stay as they are.  Opt-in.
* ``moe_shared_forward``  a Qwen-MoE block's ``experts(x, idx, w) + sigmoid(shared_expert_gate(x)) * shared_expert(x)``: at 1..2 tokens (up to 4 on request) on experts with a decode
                        copy ONE gptq_moe_shared_decode_forward call (the two decode launches in their shared form), else the experts on the path they
                        plan, the shared MLP through ``mlp_forward`` and ONE gptq_moe_shared_combine launch for the linear / sigmoid / mul / add tail
                        ``gate_weight=None``: the ungated form ``experts(x, idx, w) + shared_experts(x)`` of DeepSeek-V3 / GLM-4 MoE blocks, same paths
* ``inject_shared_expert`` / ``remove_shared_expert``   bind that as the forward of a model's ``Qwen2MoeSparseMoeBlock``s, ``DeepseekV3MoE``s and
                        ``Glm4MoeMoE``s, on the instances.  Opt-in.
* ``pack_moe_experts``  pack the dense 3-D expert parameters of a model (``quantizers`` keyed ``...mlp.experts.{e}.w1`` as ``pack_model`` takes)

Which routed path serves a call, and the switch that opens it (``QuantMoEExperts.post_init`` has the rules; every copy path is opt-in):

    path     tokens   4- / 8-bit experts      2- / 3-bit experts
    decode   1..4     decode_copy=True        low_bit_decode=True
    batch    5..64    batch=True              attribute low_bit_batch = True, set before post_init
    prefill  65..     prefill=True            attribute low_bit_prefill = True, likewise
    grouped  any      always                  low_bit=True

The per-expert composition serves what the grouped kernels do not take (2- / 3-bit experts unless ``post_init(low_bit=True)``, fp32 experts, odd group
sizes, raw act-order), CPU tensors (which ``QuantLinear`` refuses), and -- by default -- calls under grad where ``hidden_states`` or ``top_k_weights`` require grad: training through the experts gets
dX and the router-weight gradient from the existing backward of ``QuantLinear``.  After ``post_init(backward=True)`` such a call is ONE autograd node
instead: the forward runs the ordinary no-grad path, the backward is one gptq_moe_backward call (route, recompute of gate / up, two grouped transposed
dequant-GEMM stages on the checkpoint rows, combine -- five launches, nothing saved but the inputs).
"""
from __future__ import annotations

import ctypes
import types
from collections import namedtuple
from logging import getLogger

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib
from .qlinear_mi355x import QuantLinear, _raw_stream, exchange_tick, forward_multi, mlp_forward, reserve_workspace

logger = getLogger(__name__)

DEFAULT_NAMES = ("w1", "w3", "w2")          # gate, up, down (AutoGPTQ's Mixtral names)

# The routed paths of the C ABI, one record each: the describe function, the workspace-bytes and the forward symbol, the attribute that holds the table the
# forward reads -- and, for the three paths on the experts' decode copy, everything else the module knows of them: the post_init keyword that opens the
# path to 4- / 8-bit experts, the switch that opens it to 2- / 3-bit experts (decode: a keyword; batch, prefill: attributes of the module) with its flag
# bit, the token count its plan is asked at, the multiple the hidden and intermediate sizes must have, its group-size rule (base, other sizes taken, the
# message's wording; gs >= K is one group; base 0: the copy's k-chunk, 16 values at 8 bits, else 32), and its token window (first, last or None) as a
# function of the module's tunables and the width class.
_Path = namedtuple("_Path", "describe workspace forward table switch low_switch low_flag probe multiple groups window", defaults=(None,) * 7)
_PATHS = {
    "decode": _Path(_lib.describe_moe_decode_plan, "gptq_moe_decode_workspace_bytes", "gptq_moe_decode_forward", "_decode_table",
                    "decode_copy", "low_bit_decode", _lib.MOE_LOW_BIT_DECODE, 1, 64, (0, (), "the decode copy takes {} times a power of two, or one group"),
                    lambda q, low: (1, min(4, int(q.low_bit_decode_max_tokens)) if low else 4)),
    "batch": _Path(_lib.describe_moe_batch_plan, "gptq_moe_batch_workspace_bytes", "gptq_moe_batch_forward", "_decode_table",
                   "batch", "low_bit_batch", _lib.MOE_LOW_BIT_BATCH, 5, 128, (128, (32, 64), "the batch path takes 32, 64, 128 times a power of two, or one group"),
                   lambda q, low: (5, min(64, int(q.low_bit_batch_max_tokens if low else q.batch_max_tokens)))),
    "prefill": _Path(_lib.describe_moe_prefill_plan, "gptq_moe_prefill_workspace_bytes", "gptq_moe_prefill_forward", "_decode_table",
                     "prefill", "low_bit_prefill", _lib.MOE_LOW_BIT_PREFILL, 65, 128, (64, (), "the prefill path takes 64 times a power of two, or one group"),
                     lambda q, low: (max(65, int(q.low_bit_prefill_min_tokens)) if low else 65, None)),      # (it declines more than 65535 routed rows: the grouped path)
    "grouped": _Path(_lib.describe_moe_plan, "gptq_moe_workspace_bytes", "gptq_moe_forward", "_table"),
}
_COPY_PATHS = ("decode", "batch", "prefill")


def _clean_reason(d: dict) -> dict:
    """A describe answer with its reason readable: always present, the C side's '_' back to blanks."""
    d["reason"] = str(d.get("reason", "")).replace("_", " ")
    return d


class _Expert(nn.Module):
    """One expert: three QuantLinears under the projection names (gate, up, down)."""

    def __init__(self, names, bits, group_size, hidden, inter, weight_dtype, zero_mode):
        super().__init__()
        self.names = tuple(names)
        for nm, (k, n) in zip(self.names, ((hidden, inter), (hidden, inter), (inter, hidden))):
            self.add_module(nm, QuantLinear(bits, group_size, k, n, False, weight_dtype=weight_dtype, zero_mode=zero_mode))

    def layers(self):
        return tuple(getattr(self, nm) for nm in self.names)


class QuantMoEExperts(nn.Module):
    """E quantised experts behind the forward of transformers' ``MixtralExperts``: ``out[t] = sum_j w[t, j] * down(silu(gate(x_t)) * up(x_t))`` over the
    experts ``top_k_index[t, j]`` (indices outside [0, E) are dropped).  ``post_init`` (or ``autogptq_post_init``) prepares the experts' layers (without a
    decode copy unless ``decode_copy=True``) and builds the device table of per-expert pointers the grouped kernels read (and the decode kernels' own)."""

    QUANT_TYPE = "mi355x_moe"

    def __init__(self, num_experts, hidden_dim, intermediate_dim, bits, group_size, top_k=2, weight_dtype=torch.float16, names=DEFAULT_NAMES,
                 zero_mode="auto"):
        super().__init__()
        if len(names) != 3:
            raise ValueError("names: the (gate, up, down) projection names, e.g. ('w1', 'w3', 'w2')")
        self.num_experts = num_experts
        self.hidden_dim = hidden_dim
        self.intermediate_dim = intermediate_dim
        self.top_k = top_k
        self.bits = bits
        self.names = tuple(names)
        # the post_init keywords as the last post_init settled them: what _ensure_init replays (a declined switch is said once, not at every move)
        self._switches = dict(decode_copy=False, batch=False, backward=False, low_bit=False, prefill=False, low_bit_decode=False)
        self.low_bit_batch = False                  # the switch of the batch path for 2- / 3-bit experts: set before post_init (read there; see its docstring)
        self.low_bit_prefill = False                # the switch of the prefill path for 2- / 3-bit experts: set before post_init, like low_bit_batch
        self.batch_max_tokens = 64
        self.low_bit_batch_max_tokens = 64          # 2- / 3-bit experts with low_bit_batch = True: the batch path for 5..this many tokens (the kernels take 64)
        self.low_bit_prefill_min_tokens = 65        # 2- / 3-bit experts with low_bit_prefill = True: the prefill path from this many tokens on (never below 65)
        self.low_bit_decode_max_tokens = 4          # 2- / 3-bit experts with low_bit_decode=True: the decode path up to this many tokens (the kernels take 4)
        for e in range(num_experts):
            self.add_module(str(e), _Expert(self.names, bits, group_size, hidden_dim, intermediate_dim, weight_dtype, zero_mode))
        self._invalidate()

    def __getitem__(self, e) -> _Expert:
        return getattr(self, str(e))

    def __len__(self):
        return self.num_experts

    def _invalidate(self):
        self._moe = None
        self._moe_batch = None                      # the struct of the batch / prefill entry points where it is not _moe (see _moe_of)
        self._decode_table = None
        self._grad_table = None
        self._live = frozenset()                    # the copy paths ("decode", "batch", "prefill") that post_init settled on: what plan() may name
        self.decode_copy_bytes = 0
        self._keep = ()
        self._plans = {}
        self.last_plan = None

    def _apply(self, fn, *args, **kwargs):
        out = super()._apply(fn, *args, **kwargs)
        self._invalidate()
        return out

    def _load_from_state_dict(self, *args, **kwargs):
        super()._load_from_state_dict(*args, **kwargs)
        self._invalidate()

    def projections(self):
        """([gate layers], [up layers], [down layers]) in expert order."""
        ls = [self[e].layers() for e in range(self.num_experts)]
        return [l[0] for l in ls], [l[1] for l in ls], [l[2] for l in ls]

    # ------------------------------------------------------------------ post_init
    def post_init(self, decode_copy: bool = False, batch: bool = False, backward: bool = False, low_bit: bool = False, prefill: bool = False,
                  low_bit_decode: bool = False):
        """post_init every expert layer and build the pointer tables.  Default: no decode copy (1x the packed bytes; act-order layers add their
        re-sequenced rows) and every call runs the grouped kernels.  Each path below is opt-in, runs on the experts' decode copy (2x the packed bytes,
        both layouts resident; ``decode_copy_bytes`` reports the copies) and is what ``plan(T)["path"]`` names inside its token window:

            path     tokens                                      4- / 8-bit experts   2- / 3-bit experts            a decline
            decode   1..4 (low_bit_decode_max_tokens)            decode_copy=True     low_bit_decode=True           logged; no copy is built or kept: batch=, prefill=
                                                                                                                    and low_bit_decode= go with it, the two attributes
                                                                                                                    then stand alone and ask their own plans
            batch    5..64 (batch_max_tokens /                   batch=True           attribute low_bit_batch       logged; the switch is dropped (the attribute unset)
                     low_bit_batch_max_tokens, at most 64)                                                          and the experts behave as without it
            prefill  65.. (low_bit_prefill_min_tokens,           prefill=True         attribute low_bit_prefill     the same
                     at least 65)

        A switch of the other width class has no effect: ``batch=`` / ``prefill=`` on 2- / 3-bit experts are logged and dropped, the low-bit switches
        change nothing for 4- / 8-bit experts.  Any switch of a path builds the copy; 2- / 3-bit experts opened for batch or prefill alone do not ask
        the decode plan.  The attributes are set before this call (like the ``*_tokens`` tunables they survive every re-initialisation) and run
        gptq_moe_batch_forward / gptq_moe_prefill_forward with GPTQ_MOE_LOW_BIT_BATCH / _PREFILL on a struct of their own.  Outside the windows:
        the grouped path -- for 2- / 3-bit experts only with ``low_bit=True`` (forward and, with ``backward=True``, backward; nothing changes for
        4- / 8-bit experts), else the per-expert composition.  ``backward=True``: calls under grad whose ``hidden_states`` or ``top_k_weights`` require
        grad run the grouped backward (``last_plan["backward"] == "grouped"``: one autograd node, one gptq_moe_backward call on a pointer table of its
        own); experts the backward plan declines log the reason and keep the composition.  A checkpoint-layout release does not apply to expert layers."""
        dev = self[0].layers()[0].qweight.device
        if dev.type != "cuda":
            raise RuntimeError(f"mi355x QuantMoEExperts.post_init needs the module on a ROCm GPU device (got {dev}); there is no CPU path.")
        low = self.bits in (2, 3)
        sw = dict(decode_copy=bool(decode_copy), batch=bool(batch), backward=bool(backward), low_bit=bool(low_bit), prefill=bool(prefill),
                  low_bit_decode=bool(low_bit_decode))
        want_decode = sw["decode_copy"] or (sw["low_bit_decode"] and low)

        def drop(switch, why):
            """Say once that a switch has no effect, and take it back: an attribute is unset, a keyword is not replayed."""
            said = f"post_init({switch}=True)" if switch in sw else f"{switch} = True"
            logger.warning("QuantMoEExperts.%s has no effect for these experts (%s)", said, why)
            if switch in sw:
                sw[switch] = False
            else:
                setattr(self, switch, False)

        # 1. the one live switch per path for this width, as far as the layer metadata says (asked in the order the warnings have always come in: the
        #    attributes -- no effect on 4- and 8-bit experts --, then prefill= and batch=, which 2- and 3-bit experts always decline)
        live = set()
        for name, attribute in (("batch", True), ("prefill", True), ("prefill", False), ("batch", False)):
            switch = _PATHS[name].low_switch if attribute else _PATHS[name].switch
            if (low and getattr(self, switch)) if attribute else sw[switch]:
                why = self._declined(name, low_bit=attribute)
                if why:
                    drop(switch, why)
                else:
                    live.add(name)
        built = gplan = None
        while True:
            # 2. the layers (again only when the need for a decode copy changed) and the structs
            copy = want_decode or bool(live)
            why = self._declined("decode", low_bit=sw["low_bit_decode"] or bool(live)) if copy else ""
            if why:                                          # known from the metadata: no copy is built for a set the decode plan would decline
                logger.warning("QuantMoEExperts.post_init(decode_copy=True) has no effect for these experts (%s): no decode copy is built", why)
                copy = want_decode = sw["batch"] = sw["prefill"] = False
                live.clear()
            if copy != built:
                built, extra = copy, 0
                for e in range(self.num_experts):
                    for l in self[e].layers():
                        l.post_init(tiled=copy, release_checkpoint_layout=False)
                        if l._qweight_tiled is not None:
                            extra += l._qweight_tiled.numel() + l._qconst_tiled.numel()
            gate, up, down = self.projections()
            arrs = [(ctypes.POINTER(_lib.GptqLayer) * self.num_experts)(*[ctypes.pointer(l._layer) for l in ls]) for ls in (gate, up, down)]
            m = _lib.GptqMoe()
            m.E = self.num_experts
            m.flags = (_lib.MOE_LOW_BIT if sw["low_bit"] else 0) | (_lib.MOE_LOW_BIT_DECODE if sw["low_bit_decode"] else 0)
            m.gate, m.up, m.down = (ctypes.addressof(a) for a in arrs)
            mb = None
            if low and live:      # the copy paths' own struct over the same layer arrays (whichever of the two bits are on): the grouped and backward entry points refuse them
                mb = _lib.GptqMoe()
                mb.E, mb.flags, mb.gate, mb.up, mb.down = m.E, m.flags | sum(_PATHS[name].low_flag for name in live), m.gate, m.up, m.down
            if sw["backward"] and gplan is None:
                gplan = _lib.describe_moe_backward_plan(m, 1, self.top_k)
                if gplan["path"] != "grouped_backward":
                    logger.warning("QuantMoEExperts.post_init(backward=True) has no effect for these experts (%s): calls under grad keep the per-expert "
                                   "composition", _clean_reason(gplan)["reason"])
            # 3. the plans, in the order they have always been asked: the attributes' first on 2- / 3-bit experts, the decode plan first on 4- / 8-bit ones
            declined = None
            # 2- / 3-bit experts opened for the batch / the prefill path alone: the copy is those paths', the decode plan (which declines them) has no say
            ask_decode = not (low and live and not sw["low_bit_decode"])
            for name in (("batch", "prefill", "decode") if low else _COPY_PATHS):
                if copy and (name in live or (name == "decode" and ask_decode)):
                    d = _PATHS[name].describe(m if mb is None or name == "decode" else mb, _PATHS[name].probe, self.top_k)
                    if d["path"] != name:
                        declined = name
                        break
            if declined is None:
                break
            # 4. drop what declined, and what goes with it
            why = _clean_reason(d)["reason"]
            if declined == "decode":
                # declined (fp32, a group size the copy does not take, ...): nothing would read the copies -- say so and give their memory back
                logger.warning("QuantMoEExperts.post_init(decode_copy=True) has no effect for these experts (%s): no decode copy is kept", why)
                # (batch, prefill and low_bit_decode need the copy: declined with it; the low_bit_batch / low_bit_prefill attributes then stand alone and ask their plans)
                want_decode = sw["batch"] = sw["prefill"] = sw["low_bit_decode"] = False
                if not low:
                    live.clear()
            else:
                drop(getattr(_PATHS[declined], "low_switch" if low else "switch"), why)
                live.discard(declined)
        lib = _lib.load()
        table = torch.zeros(max(1, int(lib.gptq_moe_table_bytes(self.num_experts))), dtype=torch.uint8, device=dev)
        self._moe, self._moe_batch, self._keep, self._plans = m, mb, (arrs, table, gate, up, down), {}
        self._table = table
        self._decode_table = self._grad_table = None
        self._live = frozenset()                             # (set with the decode table, below)
        self.decode_copy_bytes = extra
        self._dev = torch.device("cuda", dev.index if dev.index is not None else torch.cuda.current_device())
        self._w_dtype = gate[0].scales.dtype
        sw["decode_copy"] = copy
        self._switches = sw
        with torch.cuda.device(self._dev):
            stream = _lib.current_stream_handle(self._dev)
            if _PATHS["grouped"].describe(m, 1, self.top_k)["path"] == "grouped":          # (a declined layer set has no valid table: it runs per expert)
                _lib.check(lib.gptq_moe_build_table(ctypes.byref(m), table.data_ptr(), stream))
            if gplan is not None and gplan["path"] == "grouped_backward":
                gtable = torch.zeros(max(1, int(lib.gptq_moe_grad_table_bytes(self.num_experts))), dtype=torch.uint8, device=dev)
                _lib.check(lib.gptq_moe_build_grad_table(ctypes.byref(m), gtable.data_ptr(), stream))
                self._grad_table = gtable
            if copy:
                dtable = torch.zeros(max(1, int(lib.gptq_moe_decode_table_bytes(self.num_experts))), dtype=torch.uint8, device=dev)
                _lib.check(lib.gptq_moe_build_decode_table(ctypes.byref(self._moe_of("decode_table")), dtable.data_ptr(), stream))
                self._decode_table = dtable
                self._live = frozenset(live | {"decode"} if sw["low_bit_decode"] or not low else live)
        return self

    def _ensure_init(self):
        """post_init with the settled switches when the tables were invalidated (a move, a state-dict load, a repack)."""
        if self._moe is None:
            self.post_init(**self._switches)

    def _moe_of(self, path: str):
        """The gptq_moe_t a path's entry points take ("decode_table": the one the decode table is built from): 2- / 3-bit experts with ``low_bit_batch`` /
        ``low_bit_prefill`` have one of their own for those paths (GPTQ_MOE_LOW_BIT_BATCH / GPTQ_MOE_LOW_BIT_PREFILL set, whichever are on), which also
        builds the decode table unless ``low_bit_decode`` opened ``_moe`` to it."""
        if self._moe_batch is None:
            return self._moe
        own = path in ("batch", "prefill") or (path == "decode_table" and not self._switches["low_bit_decode"])
        return self._moe_batch if own else self._moe

    def _declined(self, path: str, low_bit: bool = False) -> str:
        """Why the plan of a copy path would decline these experts, as far as the layer metadata says (empty: build the copies and ask the plan).
        ``low_bit``: a switch that opens the path to 2- / 3-bit experts is on."""
        rule = _PATHS[path]
        gate, _, down = self[0].layers()
        sizes = groups = dtype = experts = ""
        if self.hidden_dim % rule.multiple or self.intermediate_dim % rule.multiple:
            sizes = f"hidden and intermediate sizes must be multiples of {rule.multiple}"
        base, others, text = rule.groups
        base = base or (16 if self.bits == 8 else 32)
        for l in (down, gate):                               # (gate's group size is the one named where both are refused)
            gs, q = l.group_size, l.group_size // base
            if not (gs in others or gs >= l.infeatures or (gs % base == 0 and q & (q - 1) == 0)):
                groups = f"group_size {gs}: {text.format(base)}"
        wide_only = f"{self.bits}-bit experts: the {path} path takes 4 or 8 bits" if self.bits in (2, 3) and not low_bit else ""
        if path != "decode":      # the path's own rules, then the copy's in the path's name
            return sizes or groups or wide_only or self._declined("decode", low_bit).replace("the decode path", f"the {path} path")
        if gate.scales.dtype not in (torch.float16, torch.bfloat16):
            dtype = "fp32 experts: the decode path takes fp16 / bf16"
        if not 1 <= self.num_experts <= 256 or not 1 <= self.top_k <= 8:
            experts = "the decode path takes up to 256 experts and topk up to 8"
        return wide_only or dtype or sizes or experts or groups

    def workspace_token_counts(self, rows: int) -> list:
        """The token counts up to ``rows`` whose ``workspace_bytes`` a scratch for calls of 1..``rows`` tokens must cover: ``rows`` itself, the decode
        path's 1..4, and where a window of a settled copy path ends or begins below ``rows`` (a path's need grows with T: its own largest T, or the
        largest T of the paths below it)."""
        self._ensure_init()
        ts = {rows, *range(1, min(rows, 4) + 1)}
        for name in self._live:
            first, last = _PATHS[name].window(self, self.bits in (2, 3))
            ts.add(min(rows, last or first - 1))
        return sorted(ts)

    def workspace_bytes(self, T: int, top_k: "int | None" = None) -> int:
        """Scratch of one call with T tokens on the path ``plan(T)`` names."""
        self._ensure_init()
        path = self.plan(T, top_k)["path"]
        fn = _PATHS.get(path, _PATHS["grouped"]).workspace          # (per_expert: the grouped entry point's answer, 0)
        return int(getattr(_lib.load(), fn)(ctypes.byref(self._moe_of(path)), T, top_k or self.top_k))

    def backward_workspace_bytes(self, T: int, top_k: "int | None" = None) -> int:
        """Scratch of one gptq_moe_backward call with T tokens (0 when the experts have no grouped backward)."""
        self._ensure_init()
        if self._grad_table is None:
            return 0
        return int(_lib.load().gptq_moe_backward_workspace_bytes(ctypes.byref(self._moe), T, top_k or self.top_k))

    def plan(self, T: int, top_k: "int | None" = None) -> dict:
        """{"path": "decode" | "batch" | "prefill" | "grouped" | "per_expert", "reason": ...} (+ the launch / tile geometry) for T tokens: what moe_forward runs
        without grad.  A copy path only where ``post_init`` settled on it (its docstring has the switches), T lies in the path's window and its plan
        accepts; else the grouped path (or the composition)."""
        top_k = top_k or self.top_k
        if self[0].layers()[0].qweight.device.type != "cuda":
            return {"path": "per_expert", "reason": "cpu tensors"}
        self._ensure_init()
        key = (T, top_k, self.batch_max_tokens, self.low_bit_batch_max_tokens, self.low_bit_decode_max_tokens, self.low_bit_prefill_min_tokens)
        d = self._plans.get(key)
        if d is None:
            for name in _COPY_PATHS:
                if name in self._live and d is None:
                    first, last = _PATHS[name].window(self, self.bits in (2, 3))
                    if first <= T and (last is None or T <= last):
                        d = _PATHS[name].describe(self._moe_of(name), T, top_k)
                        if d["path"] != name:
                            d = None
            if d is None:
                d = _PATHS["grouped"].describe(self._moe, T, top_k)
            self._plans[key] = _clean_reason(d)
        return dict(d)


    def forward(self, hidden_states: torch.Tensor, top_k_index: torch.Tensor, top_k_weights: torch.Tensor) -> torch.Tensor:
        return moe_forward(self, hidden_states, top_k_index, top_k_weights)


def moe_forward(experts: QuantMoEExperts, x: torch.Tensor, top_k_index: torch.Tensor, top_k_weights: torch.Tensor, return_intermediate: bool = False):
    """``experts(x, top_k_index, top_k_weights)``: x [T, H] (or [..., H]), top_k_index [T, topk] (int64 as torch.topk returns it), top_k_weights [T, topk].
    The grouped path: one gptq_moe_forward call (workspace from the per-stream scratch, nothing allocated but the output); the decode path (1..4 tokens
    on experts with a decode copy): one gptq_moe_decode_forward call, same conventions; the batch path (5..64 tokens, opted in): one
    gptq_moe_batch_forward call, same conventions, rows grouped by expert as on the grouped path; the prefill path (65 tokens and more, opted in): one
    gptq_moe_prefill_forward call, the same again.  ``return_intermediate``: also (H [T topk, I], pos [T, topk] int32)
    -- the kernel's silu * mul rows and the row of each assignment (-1: dropped); rows grouped by expert on the grouped path, in assignment order on the
    decode path: ``H[pos[t, j]]`` reads the same way on both."""
    H = experts.hidden_dim
    lead = x.shape[:-1]
    x2 = x.reshape(-1, H)
    T = x2.shape[0]
    topk = top_k_index.shape[-1] if top_k_index.dim() else 1
    grad = torch.is_grad_enabled() and (x.requires_grad or top_k_weights.requires_grad)
    if x.device.type != "cuda":
        experts.last_plan = {"path": "per_expert", "reason": "cpu tensors"}
    elif grad and experts._switches["backward"] and _grouped_backward_ready(experts):
        if return_intermediate:
            raise RuntimeError("moe_forward: return_intermediate is not available under grad")
        return _MoEBackward.apply(experts, x, top_k_index, top_k_weights)
    elif grad:
        experts.last_plan = {"path": "per_expert", "reason": "grad enabled and hidden_states / top_k_weights require grad"}
    else:
        experts.last_plan = experts.plan(T, topk)
    path = experts.last_plan["path"]
    if path not in _PATHS:
        if return_intermediate:
            raise RuntimeError(f"moe_forward: return_intermediate needs the grouped, the batch, the prefill or the decode path ({experts.last_plan['reason']})")
        return _per_expert(experts, x2, top_k_index.reshape(T, topk), top_k_weights.reshape(T, topk)).reshape(lead + (H,))
    dev, w_dtype = experts._dev, experts._w_dtype
    if x.device != dev:
        raise RuntimeError(f"mi355x moe_forward: input is on {x.device}, the experts on {dev}")
    xw = _aligned(x2, w_dtype)
    idx, w = _routing(top_k_index, top_k_weights, T, topk)
    out = torch.empty((T, H), dtype=w_dtype, device=dev)
    h_out = None
    if return_intermediate:
        R, I = T * topk, experts.intermediate_dim
        es = torch.tensor([], dtype=w_dtype).element_size()
        h_out = torch.empty(R * I * es + 4 * R, dtype=torch.uint8, device=dev)
    if T:
        need = experts._plans.get(("ws", T, topk, path))
        if need is None:
            need = experts._plans[("ws", T, topk, path)] = experts.workspace_bytes(T, topk)
        buf = reserve_workspace(dev, need)
        exchange_tick(dev)
        idx_dev = experts._dev.index
        with torch.cuda.device(idx_dev):
            entry = _PATHS[path]
            rc = getattr(_lib.load(), entry.forward)(ctypes.byref(experts._moe_of(path)), getattr(experts, entry.table).data_ptr(), xw.data_ptr(), idx.data_ptr(),
                                                     w.data_ptr(), T, topk, out.data_ptr(), _lib.ptr(h_out), buf.data_ptr(), buf.numel(), _raw_stream(idx_dev))
        if rc:
            _lib.check(rc)
    res = out.to(x.dtype) if x.dtype != w_dtype else out
    res = res.reshape(lead + (H,))
    if not return_intermediate:
        return res
    R, I = T * topk, experts.intermediate_dim
    es = torch.tensor([], dtype=w_dtype).element_size()
    hs = h_out[:R * I * es].view(w_dtype).view(R, I)
    pos = h_out[R * I * es:].view(torch.int32).view(T, topk)
    return res, hs, pos


def _grouped_backward_ready(experts: QuantMoEExperts) -> bool:
    """The experts were post-initialised with backward=True and the backward plan took them (post_init runs here when the tables were invalidated)."""
    experts._ensure_init()
    return experts._grad_table is not None


def _aligned(t: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """t as a contiguous, 16-byte aligned tensor of ``dtype`` (the C ABI's rule for x / dout)."""
    if t.dtype != dtype:
        t = t.to(dtype)
    if not t.is_contiguous():
        t = t.contiguous()
    if t.data_ptr() & 15:                 # a contiguous view at an odd element offset
        t = t.clone()
    return t


def _routing(top_k_index: torch.Tensor, top_k_weights: torch.Tensor, T: int, topk: int):
    """(top_k_index, top_k_weights) as the contiguous int64 / fp32 [T, topk] pair the C ABI reads."""
    idx = top_k_index.reshape(T, topk)
    if idx.dtype != torch.int64:
        idx = idx.to(torch.int64)
    w = top_k_weights.reshape(T, topk)
    if w.dtype != torch.float32:
        w = w.to(torch.float32)
    return idx.contiguous(), w.contiguous()


class _MoEBackward(torch.autograd.Function):
    """``moe_forward`` under grad as one node: forward = the no-grad path ``plan(T)`` names (bit-identical values), backward = one gptq_moe_backward call
    that recomputes gate / up from x.  Saves x, top_k_index and top_k_weights only; no double backward."""

    @staticmethod
    def forward(ctx, experts, x, top_k_index, top_k_weights):
        with torch.no_grad():
            out = moe_forward(experts, x.detach(), top_k_index, top_k_weights.detach())
        experts.last_plan = dict(experts.last_plan, backward="grouped")
        ctx.experts = experts
        ctx.save_for_backward(x, top_k_index, top_k_weights)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        experts = ctx.experts
        x, top_k_index, top_k_weights = ctx.saved_tensors
        if not _grouped_backward_ready(experts):
            raise RuntimeError("mi355x moe backward: the experts lost their grouped backward between forward and backward")
        want_x, want_w = ctx.needs_input_grad[1], ctx.needs_input_grad[3]
        H = experts.hidden_dim
        dev, w_dtype = experts._dev, experts._w_dtype
        x2 = _aligned(x.reshape(-1, H), w_dtype)
        T = x2.shape[0]
        topk = top_k_index.shape[-1] if top_k_index.dim() else 1
        dout = _aligned(grad_out.reshape(-1, H), w_dtype)
        idx, w = _routing(top_k_index, top_k_weights, T, topk)
        dx = torch.empty((T, H), dtype=w_dtype, device=dev) if want_x else None
        dw = torch.empty((T, topk), dtype=torch.float32, device=dev) if want_w else None
        if T and (want_x or want_w):
            need = experts._plans.get(("bws", T, topk))
            if need is None:
                need = experts._plans[("bws", T, topk)] = experts.backward_workspace_bytes(T, topk)
            buf = reserve_workspace(dev, need)
            exchange_tick(dev)
            with torch.cuda.device(dev.index):
                rc = _lib.load().gptq_moe_backward(ctypes.byref(experts._moe), experts._table.data_ptr(), experts._grad_table.data_ptr(), x2.data_ptr(),
                                                   idx.data_ptr(), w.data_ptr(), dout.data_ptr(), T, topk, _lib.ptr(dx), _lib.ptr(dw), None,
                                                   buf.data_ptr(), buf.numel(), _raw_stream(dev.index))
            if rc:
                _lib.check(rc)
        gx = dx.to(x.dtype).reshape(x.shape) if want_x else None
        gw = dw.to(top_k_weights.dtype).reshape(top_k_weights.shape) if want_w else None
        return None, gx, None, gw


def _per_expert(experts: QuantMoEExperts, x: torch.Tensor, idx: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """The composition of per-expert QuantLinear calls (the shape of transformers' expert loop): differentiable in x and w, host syncs per call."""
    T, H = x.shape
    out = torch.zeros((T, H), dtype=torch.float32, device=x.device)
    for e in range(experts.num_experts):
        tok, j = torch.where(idx == e)
        if tok.numel() == 0:
            continue
        gate, up, down = experts[e].layers()
        xs = x[tok]
        g, u = forward_multi([gate, up], xs)
        y = down(F.silu(g) * u).float() * w[tok, j, None].float()
        out = out.index_add(0, tok, y)
    return out.to(x.dtype)


# ---------------------------------------------------------------------------------------------------------------- the router
_ROUTER_PLANS: dict = {}
ROUTER_CLASSES = {"MixtralTopKRouter": "mixtral", "Qwen2MoeTopKRouter": "qwen", "Qwen3MoeTopKRouter": "qwen",      # matched by class name
                  "DeepseekV3TopkRouter": "grouped", "Glm4MoeTopkRouter": "grouped"}
_GROUPED_ATTRS = ("topk_group", "norm_topk_prob", "routed_scaling_factor", "e_score_correction_bias")      # (+ num_group or n_group)


def router_plan(T: int, H: int, E: int, top_k: int, dtype: torch.dtype, renorm: bool = True) -> dict:
    """{"path": "router" | "none", "form": "rows" | "tiles", "reason": ...} for one ``moe_route`` call on GPU tensors (host-only, cached)."""
    key = (T, H, E, top_k, dtype, bool(renorm))
    d = _ROUTER_PLANS.get(key)
    if d is None:
        enum = _lib.DTYPE_ENUM.get(dtype)
        if enum is None:
            d = {"path": "none", "reason": f"dtype {dtype}: the router kernel takes fp16 / bf16"}
        else:
            d = _clean_reason(_lib.describe_moe_router_plan(T, H, E, top_k, enum, _lib.ROUTER_RENORM if renorm else 0))
        _ROUTER_PLANS[key] = d
    return dict(d)


def _route_composition(x2, weight, top_k, renorm, return_logits):
    """The routers of transformers, operation for operation (MixtralTopKRouter.forward; the Qwen routers up to their final cast)."""
    logits = F.linear(x2, weight)
    probs = F.softmax(logits, dim=-1, dtype=torch.float)
    val, idx = torch.topk(probs, top_k, dim=-1)
    if renorm:
        val = val / val.sum(dim=-1, keepdim=True)
    return (logits if return_logits else None), val, idx


def moe_route(x: torch.Tensor, weight: torch.Tensor, top_k: int, renorm: bool = True, return_logits: bool = True):
    """Router of a softmax-then-top-k mixture-of-experts layer: x [T, H] (or [..., H]), weight [E, H] -> (logits [T, E] in x's dtype or None, weights fp32
    [T, top_k], indices int64 [T, top_k]).  On the GPU, without grad, for what the plan takes (fp16 / bf16, E <= 256, top_k <= min(E, 8), H % 64 == 0): ONE
    gptq_moe_router call on the current stream -- the selection rule is written (descending logit, equal logits to the lower index), nothing is allocated
    but the outputs, nothing synchronises, and a captured graph replays it.  Everything else runs the torch composition (``last_route_plan`` says why):
    CPU tensors, what the plan declines, and calls under grad where ``x`` or ``weight`` require grad -- router training keeps autograd."""
    global last_route_plan
    E, H = weight.shape
    x2 = x.reshape(-1, H)
    T = x2.shape[0]
    if x2.device.type != "cuda" or weight.device != x2.device:
        plan = {"path": "none", "reason": "cpu tensors"}
    elif torch.is_grad_enabled() and (x.requires_grad or weight.requires_grad):
        plan = {"path": "none", "reason": "grad enabled and x / weight require grad"}
    elif x2.dtype != weight.dtype:
        plan = {"path": "none", "reason": f"x is {x2.dtype}, weight {weight.dtype}"}
    elif not weight.is_contiguous() or weight.data_ptr() & 15:
        plan = {"path": "none", "reason": "weight must be contiguous and 16-byte aligned"}
    else:
        plan = router_plan(T, H, E, top_k, x2.dtype, renorm)
    last_route_plan = plan
    if plan["path"] != "router":
        return _route_composition(x2, weight, top_k, renorm, return_logits)
    dev = x2.device
    if not x2.is_contiguous():
        x2 = x2.contiguous()
    if x2.data_ptr() & 15:                # a contiguous view at an odd element offset: the C ABI takes 16-byte aligned x
        x2 = x2.clone()
    logits = torch.empty((T, E), dtype=x2.dtype, device=dev) if return_logits else None
    idx = torch.empty((T, top_k), dtype=torch.int64, device=dev)
    w = torch.empty((T, top_k), dtype=torch.float32, device=dev)
    if T:
        with torch.cuda.device(dev.index):
            rc = _lib.load().gptq_moe_router(x2.data_ptr(), weight.data_ptr(), T, H, E, top_k, _lib.DTYPE_ENUM[x2.dtype],
                                             _lib.ROUTER_RENORM if renorm else 0, _lib.ptr(logits), idx.data_ptr(), w.data_ptr(), _raw_stream(dev.index))
        if rc:
            _lib.check(rc)
    return logits, w, idx


# ---------------------------------------------------------------------------------------------------------------- the grouped-sigmoid router
_BIAS_F32: dict = {}
# (E * H at and above which, token count up to which) moe_route_grouped leaves the 16-token (tiles) form to the composition: measured slower there
# (profiles/moe_router_grouped_ab.log: DeepSeek-V3's router, E 256 x H 7168, at 16 and 64 tokens -- one to four workgroups pull all of the weight with one
# k-step in flight per wave; faster again at 512 tokens, and at every token count on the 128 x 4096 router).  None: no region is declined for speed.
GROUPED_SLOW_TILES = (256 * 7168, 64)


def router_grouped_plan(T: int, H: int, E: int, top_k: int, n_group: int, topk_group: int, dtype: torch.dtype, renorm: bool = True) -> dict:
    """{"path": "router_grouped" | "none", "form": "rows" | "tiles", "reason": ...} for one ``moe_route_grouped`` call on GPU tensors (host-only, cached)."""
    key = ("grouped", T, H, E, top_k, n_group, topk_group, dtype, bool(renorm), GROUPED_SLOW_TILES)
    d = _ROUTER_PLANS.get(key)
    if d is None:
        enum = _lib.DTYPE_ENUM.get(dtype)
        if enum is None:
            d = {"path": "none", "reason": f"dtype {dtype}: the router kernel takes fp16 / bf16"}
        else:
            d = _clean_reason(_lib.describe_moe_router_grouped_plan(T, H, E, top_k, n_group, topk_group, enum, _lib.ROUTER_RENORM if renorm else 0))
            slow = GROUPED_SLOW_TILES
            if slow is not None and d["path"] == "router_grouped" and d["form"] == "tiles" and E * H >= slow[0] and T <= slow[1]:
                d = {"path": "none", "reason": f"the tiles form was measured slower than the composition at 9..{slow[1]} tokens with E * H >= {slow[0]}"}
        _ROUTER_PLANS[key] = d
    return dict(d)


def _route_grouped_composition(x2, weight, bias, top_k, n_group, topk_group, renorm, scale, return_logits):
    """The router of transformers' DeepSeek-V3 / GLM-4 MoE, operation for operation (DeepseekV3TopkRouter.forward)."""
    E = weight.shape[0]
    router_logits = F.linear(x2.type(torch.float32), weight.type(torch.float32))
    scores = router_logits.sigmoid()
    scores_for_choice = scores + bias if bias is not None else scores
    group_scores = scores_for_choice.view(-1, n_group, E // n_group).topk(2, dim=-1)[0].sum(dim=-1)
    group_idx = torch.topk(group_scores, k=topk_group, dim=-1, sorted=False)[1]
    group_mask = torch.zeros_like(group_scores)
    group_mask.scatter_(1, group_idx, 1)
    score_mask = group_mask.unsqueeze(-1).expand(-1, n_group, E // n_group).reshape(-1, E)
    scores_for_choice = scores_for_choice.masked_fill(~score_mask.bool(), float("-inf"))
    topk_indices = torch.topk(scores_for_choice, k=top_k, dim=-1, sorted=False)[1]
    topk_weights = scores.gather(1, topk_indices)
    if renorm:
        denominator = topk_weights.sum(dim=-1, keepdim=True) + 1e-20
        topk_weights = topk_weights / denominator
    topk_weights = topk_weights * scale
    return (router_logits if return_logits else None), topk_weights, topk_indices


def _bias_f32(bias: torch.Tensor) -> torch.Tensor:
    """``bias`` as a contiguous fp32 tensor: itself, or a copy cached on (data_ptr, _version, device) -- ``model.half()`` casts the correction-bias buffer
    too, and a cast per call would be a launch of its own in a captured step."""
    if bias.dtype == torch.float32 and bias.is_contiguous() and not bias.data_ptr() & 3:
        return bias
    key = (bias.data_ptr(), bias._version, bias.device, bias.dtype, tuple(bias.shape), tuple(bias.stride()))
    ent = _BIAS_F32.get(key)
    if ent is None:
        if len(_BIAS_F32) >= 4096:      # (buffers that were freed or updated in place leave stale entries behind)
            _BIAS_F32.clear()
        ent = _BIAS_F32[key] = bias.detach().to(torch.float32).contiguous()
    return ent


def moe_route_grouped(x: torch.Tensor, weight: torch.Tensor, bias: "torch.Tensor | None", top_k: int, n_group: int, topk_group: int, renorm: bool = True,
                      scale: float = 1.0, return_logits: bool = True):
    """Router of a DeepSeek-V3 / GLM-4 MoE layer: x [T, H] (or [..., H]), weight [E, H], bias [E] (``e_score_correction_bias``) or None -> (logits fp32
    [T, E] or None, weights fp32 [T, top_k], indices int64 [T, top_k]): fp32 logits, sigmoid scores, group-limited top-k on the biased scores, weights from
    the unbiased ones, renormalised when ``renorm`` and multiplied by ``scale`` (``routed_scaling_factor``).  On the GPU, without grad, for what the plan
    takes (``router_grouped_plan``): ONE gptq_moe_router_grouped call on the current stream -- written tie rules (equal scores to the lower group / expert
    index), nothing allocated but the outputs, nothing synchronises, a captured graph replays it.  Everything else runs the transformers composition
    (``last_route_plan`` says why): CPU tensors, what the plan declines (for its shape, or for speed: ``GROUPED_SLOW_TILES``), x and weight of different
    dtypes, a weight that is not contiguous, and calls under grad where ``x`` or ``weight`` require grad.  A bias that is not contiguous fp32 is read through a cached fp32 copy."""
    global last_route_plan
    E, H = weight.shape
    x2 = x.reshape(-1, H)
    T = x2.shape[0]
    scale = float(scale)
    if x2.device.type != "cuda" or weight.device != x2.device or (bias is not None and bias.device != x2.device):
        plan = {"path": "none", "reason": "cpu tensors"}
    elif torch.is_grad_enabled() and (x.requires_grad or weight.requires_grad):
        plan = {"path": "none", "reason": "grad enabled and x / weight require grad"}
    elif x2.dtype != weight.dtype:
        plan = {"path": "none", "reason": f"x is {x2.dtype}, weight {weight.dtype}"}
    elif not weight.is_contiguous() or weight.data_ptr() & 15:
        plan = {"path": "none", "reason": "weight must be contiguous and 16-byte aligned"}
    elif bias is not None and tuple(bias.shape) != (E,):
        plan = {"path": "none", "reason": f"bias must be [{E}]"}
    elif scale - scale != 0.0:
        plan = {"path": "none", "reason": "scale must be finite"}
    else:
        plan = router_grouped_plan(T, H, E, top_k, n_group, topk_group, x2.dtype, renorm)
    last_route_plan = plan
    if plan["path"] != "router_grouped":
        return _route_grouped_composition(x2, weight, bias, top_k, n_group, topk_group, renorm, scale, return_logits)
    dev = x2.device
    if not x2.is_contiguous():
        x2 = x2.contiguous()
    if x2.data_ptr() & 15:
        x2 = x2.clone()
    b = _bias_f32(bias) if bias is not None else None
    logits = torch.empty((T, E), dtype=torch.float32, device=dev) if return_logits else None
    idx = torch.empty((T, top_k), dtype=torch.int64, device=dev)
    w = torch.empty((T, top_k), dtype=torch.float32, device=dev)
    if T:
        with torch.cuda.device(dev.index):
            rc = _lib.load().gptq_moe_router_grouped(x2.data_ptr(), weight.data_ptr(), _lib.ptr(b), T, H, E, top_k, n_group, topk_group, scale,
                                                     _lib.DTYPE_ENUM[x2.dtype], _lib.ROUTER_RENORM if renorm else 0, _lib.ptr(logits), None, idx.data_ptr(),
                                                     w.data_ptr(), _raw_stream(dev.index))
        if rc:
            _lib.check(rc)
    return logits, w, idx


last_route_plan: dict = {}


def _fused_router_forward(self, hidden_states):
    """Bound on a router instance by inject_fused_router: the class's own triple (router_logits, router_scores, router_indices)."""
    if self._fused_router_kind == "grouped":
        n_group = self.num_group if hasattr(self, "num_group") else self.n_group
        return moe_route_grouped(hidden_states.reshape(-1, self.weight.shape[1]), self.weight, self.e_score_correction_bias, self.top_k, n_group,
                                 self.topk_group, renorm=bool(self.norm_topk_prob), scale=self.routed_scaling_factor, return_logits=True)
    qwen = self._fused_router_kind == "qwen"
    renorm = bool(getattr(self, "norm_topk_prob", True)) if qwen else True
    logits, scores, idx = moe_route(hidden_states.reshape(-1, self.weight.shape[1]), self.weight, self.top_k, renorm=renorm, return_logits=True)
    if qwen:
        scores = scores.to(logits.dtype)
    return logits, scores, idx


def _router_kind(m: nn.Module):
    kind = ROUTER_CLASSES.get(type(m).__name__)
    w = getattr(m, "weight", None)
    if kind is None or not torch.is_tensor(w) or w.dim() != 2 or not hasattr(m, "top_k") or getattr(m, "num_experts", None) != w.shape[0]:
        return None
    if kind == "grouped" and not (all(hasattr(m, a) for a in _GROUPED_ATTRS) and (hasattr(m, "num_group") or hasattr(m, "n_group"))):
        return None
    return kind


def inject_fused_router(model: nn.Module) -> int:
    """Give every MixtralTopKRouter / Qwen2MoeTopKRouter / Qwen3MoeTopKRouter of ``model`` (matched by class name, with ``weight [E, H]``, ``top_k`` and
    ``num_experts``) a forward bound on the INSTANCE that calls ``moe_route``.  The module keeps its object, class and parameters, so state-dict keys,
    hooks and transformers' ``OutputRecorder(<RouterClass>, index=0)`` (``output_router_logits=True``) keep working.  Mixtral: renormalised fp32 scores;
    Qwen 2 / 3: renormalised iff ``norm_topk_prob``, scores cast to the logits dtype.  DeepseekV3TopkRouter / Glm4MoeTopkRouter (which must also carry
    ``num_group`` or ``n_group``, ``topk_group``, ``norm_topk_prob``, ``routed_scaling_factor`` and ``e_score_correction_bias``): ``moe_route_grouped`` --
    fp32 logits, fp32 weights.  Routers of any other class are left alone.
    Returns the number of routers bound.  Nothing is injected by default."""
    n = 0
    for m in model.modules():
        kind = _router_kind(m)
        if kind is None:
            continue
        m.__dict__["_fused_router_kind"] = kind
        m.__dict__["forward"] = types.MethodType(_fused_router_forward, m)
        n += 1
    return n


def remove_fused_router(model: nn.Module) -> int:
    """Undo inject_fused_router: the class forward is back on every router it bound.  Returns their number."""
    n = 0
    for m in model.modules():
        if "_fused_router_kind" in m.__dict__:
            m.__dict__.pop("forward", None)
            del m.__dict__["_fused_router_kind"]
            n += 1
    return n


# ---------------------------------------------------------------------------------------------------------------- the shared expert
SHARED_BLOCK_CLASSES = ("Qwen2MoeSparseMoeBlock", "DeepseekV3MoE", "Glm4MoeMoE")      # matched by class name
# Up to this many tokens moe_shared_forward runs the fused call where the plan accepts; above, experts + mlp_forward + the combine launch.  The kernels take
# 1..4; the default is where the fused call was measured the fastest form on A2.7B's block (profiles/moe_shared_ab.log: at 3 and 4 tokens launch 2's
# workgroups walk the routed segments and the long shared one in sequence, and the combine form wins).  Per experts module:
# ``experts.shared_decode_max_tokens = n``.
SHARED_DECODE_MAX_TOKENS = 2


def _shared_state(experts: QuantMoEExperts, shared_layers):
    """(GptqMoeShared, key) for these experts and shared layers: the struct holds the layers' current gptq_layer_t (gate_w is set per call); cached on the
    experts, so it dies with their tables, and keyed by the layer structs, so a shared layer that was re-initialised gets a new one."""
    for l in shared_layers:
        if l._layer is None:
            l.post_init()
    key = ("shared",) + tuple(id(l._layer) for l in shared_layers)
    ent = experts._plans.get(key)
    if ent is None:
        sh = _lib.GptqMoeShared()
        sh.gate, sh.up, sh.down = (ctypes.addressof(l._layer) for l in shared_layers)
        ent = experts._plans[key] = (sh, tuple(l._layer for l in shared_layers))      # (the structs stay alive with the entry: their ids are not reused)
    return ent[0], key


def shared_plan(experts: QuantMoEExperts, shared_layers, T: int, top_k: "int | None" = None) -> dict:
    """{"path": "decode_shared" | "none", "reason": ...} (+ the launch geometry): what the fused call of ``moe_shared_forward`` would run for T tokens
    (host-only; "none" also when the experts themselves do not plan the decode path at T)."""
    top_k = top_k or experts.top_k
    if experts.plan(T, top_k)["path"] != "decode":
        return {"path": "none", "reason": "the routed experts do not run the decode path at this token count"}
    sh, key = _shared_state(experts, shared_layers)
    d = experts._plans.get(key + (T, top_k))
    if d is None:
        sh.gate_w = None
        d = experts._plans[key + (T, top_k)] = _clean_reason(_lib.describe_moe_shared_decode_plan(experts._moe, sh, T, top_k))
    return dict(d)


def shared_workspace_bytes(experts: QuantMoEExperts, shared_layers, T: int, top_k: "int | None" = None) -> int:
    """Scratch of one fused call with T tokens (0 when ``shared_plan`` declines)."""
    top_k = top_k or experts.top_k
    if shared_plan(experts, shared_layers, T, top_k)["path"] != "decode_shared":
        return 0
    sh, _ = _shared_state(experts, shared_layers)
    sh.gate_w = None
    return int(_lib.load().gptq_moe_shared_decode_workspace_bytes(ctypes.byref(experts._moe), ctypes.byref(sh), T, top_k))


def moe_shared_forward(experts: QuantMoEExperts, shared_layers, gate_weight: "torch.Tensor | None", x: torch.Tensor, top_k_index: torch.Tensor,
                       top_k_weights: torch.Tensor, return_intermediate: bool = False):
    """A Qwen-MoE block behind its router: ``experts(x, idx, w) + sigmoid(x @ gate_weight.T) * down(silu(gate(x)) * up(x))`` with
    ``shared_layers = (gate, up, down)`` QuantLinears [H -> I_s], [H -> I_s], [I_s -> H] and ``gate_weight`` the dense [1, H] (or [H]) weight of
    ``shared_expert_gate``, read in place.  ``gate_weight=None`` is the ungated block of DeepSeek-V3 / GLM-4 MoE, ``experts(x, idx, w) + shared_experts(x)``:
    the same three paths with the gate scalar 1 (the kernels take a NULL gate weight).  ``experts.last_plan["shared"]`` says what ran:

    * ``"decode"``   without grad, on the GPU, when ``experts.plan(T)["path"] == "decode"`` (experts with a decode copy), ``shared_plan`` accepts and
                     T <= ``experts.shared_decode_max_tokens`` (default SHARED_DECODE_MAX_TOKENS = 2; the kernels take up to 4): ONE
                     gptq_moe_shared_decode_forward call -- two launches for the whole block behind the router
    * ``"combine"``  every other call without grad on the GPU: ``experts`` on the path it plans, the shared MLP through ``mlp_forward``, then ONE
                     gptq_moe_shared_combine launch (gate dot product, sigmoid, mul and add, in place on the routed output)
    * ``"torch"``    calls under grad where x, the routing weights or ``gate_weight`` require grad, CPU tensors, and a ``gate_weight`` the kernels do not
                     take (another dtype than the experts', not contiguous, not 16-byte aligned): the plain torch formula of the block

    ``return_intermediate`` (the fused call only): also (H [T topk, I], pos [T, topk] int32, Hs [T, I_s], s [T] fp32) -- the kernel's silu * mul rows of the
    routed and the shared expert and the gate scalars.  Workspace comes from the per-stream scratch, as ``moe_forward`` takes it."""
    gate, up, down = shared_layers
    H = experts.hidden_dim
    lead = x.shape[:-1]
    x2 = x.reshape(-1, H)
    T = x2.shape[0]
    topk = top_k_index.shape[-1] if top_k_index.dim() else 1
    why = ""
    if x.device.type != "cuda":
        why = "cpu tensors"
    elif torch.is_grad_enabled() and (x.requires_grad or top_k_weights.requires_grad or (gate_weight is not None and gate_weight.requires_grad)):
        why = "grad enabled and hidden_states / top_k_weights / gate_weight require grad"
    else:
        w_dtype = gate.scales.dtype
        if gate_weight is not None and (gate_weight.dtype != w_dtype or gate_weight.device != x.device):
            why = f"gate_weight is {gate_weight.dtype} on {gate_weight.device}, the shared layers {w_dtype} on {x.device}"
        elif w_dtype not in (torch.float16, torch.bfloat16) or H % 8:
            why = "the shared combine kernel takes fp16 / bf16 and H % 8 == 0"
        elif gate_weight is not None and (gate_weight.numel() != H or not gate_weight.is_contiguous() or gate_weight.data_ptr() & 15):
            why = "gate_weight must be [1, H], contiguous and 16-byte aligned"
    if why:
        if return_intermediate:
            raise RuntimeError(f"moe_shared_forward: return_intermediate needs the fused decode call ({why})")
        routed = experts(x2, top_k_index.reshape(T, topk), top_k_weights.reshape(T, topk))
        shared = down(F.silu(gate(x2)) * up(x2))
        out = routed + shared if gate_weight is None else routed + torch.sigmoid(F.linear(x2, gate_weight.reshape(1, H))) * shared
        experts.last_plan = dict(experts.last_plan or {}, shared="torch", shared_reason=why)
        return out.reshape(lead + (H,))
    xw = _aligned(x2, w_dtype)
    fused = 0 < T <= min(4, experts.__dict__.get("shared_decode_max_tokens", SHARED_DECODE_MAX_TOKENS)) and \
        shared_plan(experts, shared_layers, T, topk)["path"] == "decode_shared"
    if not fused:
        if return_intermediate:
            raise RuntimeError("moe_shared_forward: return_intermediate needs the fused decode call "
                               f"({shared_plan(experts, shared_layers, T, topk).get('reason', '') if T else 'no tokens'})")
        out = moe_forward(experts, xw, top_k_index, top_k_weights)
        out = out.reshape(T, H)
        if out.dtype != w_dtype or not out.is_contiguous() or out.data_ptr() & 15 or out.data_ptr() == xw.data_ptr():
            out = out.to(w_dtype).clone()
        if T:
            ys = _aligned(mlp_forward(gate, up, down, xw), w_dtype)
            with torch.cuda.device(xw.device.index):
                rc = _lib.load().gptq_moe_shared_combine(xw.data_ptr(), _lib.ptr(gate_weight), ys.data_ptr(), out.data_ptr(), T, H, _lib.DTYPE_ENUM[w_dtype],
                                                         _raw_stream(xw.device.index))
            if rc:
                _lib.check(rc)
        experts.last_plan = dict(experts.last_plan or {}, shared="combine")
        res = out.to(x.dtype) if x.dtype != w_dtype else out
        return res.reshape(lead + (H,))
    dev = experts._dev
    if x.device != dev:
        raise RuntimeError(f"mi355x moe_shared_forward: input is on {x.device}, the experts on {dev}")
    idx, w = _routing(top_k_index, top_k_weights, T, topk)
    sh, key = _shared_state(experts, shared_layers)
    out = torch.empty((T, H), dtype=w_dtype, device=dev)
    R, I, Is = T * topk, experts.intermediate_dim, gate.outfeatures
    es = out.element_size()
    h_out = torch.empty(R * I * es + 4 * R + T * Is * es + 4 * T, dtype=torch.uint8, device=dev) if return_intermediate else None
    need = experts._plans.get(key + ("ws", T, topk))
    if need is None:
        need = experts._plans[key + ("ws", T, topk)] = shared_workspace_bytes(experts, shared_layers, T, topk)
    buf = reserve_workspace(dev, need)
    exchange_tick(dev)
    sh.gate_w = _lib.ptr(gate_weight)
    with torch.cuda.device(dev.index):
        rc = _lib.load().gptq_moe_shared_decode_forward(ctypes.byref(experts._moe), ctypes.byref(sh), experts._decode_table.data_ptr(), xw.data_ptr(),
                                                        idx.data_ptr(), w.data_ptr(), T, topk, out.data_ptr(), _lib.ptr(h_out), buf.data_ptr(), buf.numel(),
                                                        _raw_stream(dev.index))
    if rc:
        _lib.check(rc)
    experts.last_plan = dict(experts.plan(T, topk), shared="decode")
    res = out.to(x.dtype) if x.dtype != w_dtype else out
    res = res.reshape(lead + (H,))
    if not return_intermediate:
        return res
    o1, o2, o3 = R * I * es, R * I * es + 4 * R, R * I * es + 4 * R + T * Is * es
    return (res, h_out[:o1].view(w_dtype).view(R, I), h_out[o1:o2].view(torch.int32).view(T, topk), h_out[o2:o3].view(w_dtype).view(T, Is),
            h_out[o3:].view(torch.float32))


def _shared_block_forward(self, hidden_states):
    """Bound on a block instance by inject_shared_expert: the class's own result (the router is called as before, so a fused router composes)."""
    shape = hidden_states.shape
    x = hidden_states.reshape(-1, shape[-1])
    _, routing_weights, selected_experts = self.gate(x)
    if hasattr(self, "shared_expert_gate"):                       # the Qwen form
        se, gate_weight = self.shared_expert, self.shared_expert_gate.weight
    else:                                                         # the DeepSeek-V3 / GLM-4 MoE form: always on, no gate
        se, gate_weight = self.shared_experts, None
    out = moe_shared_forward(self.experts, (se.gate_proj, se.up_proj, se.down_proj), gate_weight, x, selected_experts, routing_weights)
    return out.reshape(shape)


def _shared_block_parts(m: nn.Module):
    """(experts, (gate, up, down)) of a block inject_shared_expert takes, or None."""
    if type(m).__name__ not in SHARED_BLOCK_CLASSES:
        return None
    experts, sg = getattr(m, "experts", None), getattr(m, "shared_expert_gate", None)
    gated = hasattr(m, "shared_expert_gate")                      # Qwen: shared_expert + shared_expert_gate; DeepSeek-V3 / GLM-4 MoE: shared_experts, no gate
    se = getattr(m, "shared_expert" if gated else "shared_experts", None)
    if not isinstance(experts, QuantMoEExperts) or se is None or not hasattr(m, "gate"):
        return None
    layers = tuple(getattr(se, nm, None) for nm in ("gate_proj", "up_proj", "down_proj"))
    if not all(isinstance(l, QuantLinear) for l in layers):
        return None
    H, Is = experts.hidden_dim, layers[0].outfeatures
    if [(l.infeatures, l.outfeatures) for l in layers] != [(H, Is), (H, Is), (Is, H)]:
        return None
    if gated and (not isinstance(sg, nn.Linear) or sg.bias is not None or sg.out_features != 1 or sg.in_features != H):
        return None
    return experts, layers


def inject_shared_expert(model: nn.Module) -> int:
    """Give every ``Qwen2MoeSparseMoeBlock`` of ``model`` (matched by class name; ``experts`` a QuantMoEExperts, ``shared_expert.{gate_proj, up_proj,
    down_proj}`` QuantLinears, ``shared_expert_gate`` a bias-free Linear(H, 1)) and every ``DeepseekV3MoE`` / ``Glm4MoeMoE`` (``shared_experts.{gate_proj,
    up_proj, down_proj}`` QuantLinears and no ``shared_expert_gate``) a forward bound on the INSTANCE that calls ``moe_shared_forward``.  The block
    keeps its object, class, parameters, state-dict keys and hooks; it calls ``self.gate(...)`` as before, so ``inject_fused_router`` composes;
    ``shared_expert_gate.weight`` is read in place at every call, so a later ``.to()`` is seen.  (Forward hooks on the children: ``shared_expert`` and
    ``shared_expert_gate`` are never called as modules; ``experts`` and the three shared QuantLinears only on the ``"torch"`` path.)  Order: inject, then
    ``autogptq_post_init(model, expert_decode_copy=True)`` -- its scratch then covers the fused call -- then ``capture_decode_step``.  Returns the number of
    blocks bound.  Nothing is injected by default."""
    n = 0
    for m in model.modules():
        if _shared_block_parts(m) is None:
            continue
        m.__dict__["_shared_expert_injected"] = True
        m.__dict__["forward"] = types.MethodType(_shared_block_forward, m)
        n += 1
    return n


def remove_shared_expert(model: nn.Module) -> int:
    """Undo inject_shared_expert: the class forward is back on every block it bound.  Returns their number."""
    n = 0
    for m in model.modules():
        if "_shared_expert_injected" in m.__dict__:
            m.__dict__.pop("forward", None)
            del m.__dict__["_shared_expert_injected"]
            n += 1
    return n


def injected_shared_blocks(model: nn.Module):
    """[(experts, (gate, up, down))] of the blocks inject_shared_expert has bound (autogptq_post_init sizes the scratch of their fused call)."""
    out = []
    for m in model.modules():
        if "_shared_expert_injected" in m.__dict__:
            parts = _shared_block_parts(m)
            if parts is not None:
                out.append(parts)
    return out


def _is_dense_experts(m: nn.Module) -> bool:
    gu, dn = getattr(m, "gate_up_proj", None), getattr(m, "down_proj", None)
    return torch.is_tensor(gu) and torch.is_tensor(dn) and gu.dim() == 3 and dn.dim() == 3 and hasattr(m, "num_experts")


def dense_expert_modules(model: nn.Module) -> dict:
    """{path: module} of the MixtralExperts-like modules (3-D gate_up_proj / down_proj and num_experts) of a model."""
    return {n: m for n, m in model.named_modules() if _is_dense_experts(m)}


def make_quant_experts(model: nn.Module, path: str, bits: int, group_size: int, names=DEFAULT_NAMES) -> QuantMoEExperts:
    """Swap the dense experts module at ``path`` for a QuantMoEExperts of the same shape (same device and weight dtype) and return it."""
    from .model_utils import _recurse_setattr
    m = model.get_submodule(path)
    E, I2, H = m.gate_up_proj.shape
    top_k = getattr(getattr(model, "config", None), "num_experts_per_tok", None) or 2
    q = QuantMoEExperts(E, H, I2 // 2, bits, group_size, top_k=top_k, weight_dtype=m.gate_up_proj.dtype, names=names)
    q = q.to(m.gate_up_proj.device)
    _recurse_setattr(model, path, q)
    return q


def pack_moe_experts(model: nn.Module, quantizers: dict, bits: int, group_size: int, desc_act: bool = False, names=DEFAULT_NAMES) -> None:
    """Quantise the dense experts of ``model`` in place: every MixtralExperts-like module whose experts appear in ``quantizers`` (keyed
    ``<path>.{e}.<name>``, values ``(quantizer, scale, zero, g_idx)`` as ``pack_model`` takes them) becomes a QuantMoEExperts packed from
    w1 = gate_up_proj[e, :I], w3 = gate_up_proj[e, I:], w2 = down_proj[e]."""
    for path, m in list(dense_expert_modules(model).items()):
        if not any(k.startswith(path + ".") for k in quantizers):
            continue
        gu, dn = m.gate_up_proj.data, m.down_proj.data
        I = gu.shape[1] // 2
        q = make_quant_experts(model, path, bits, group_size, names)
        for e in range(q.num_experts):
            for nm, W in zip(names, (gu[e, :I], gu[e, I:], dn[e])):
                key = f"{path}.{e}.{nm}"
                if key not in quantizers:
                    raise KeyError(f"pack_moe_experts: no quantizer for {key}")
                _, scale, zero, g_idx = quantizers[key]
                getattr(q[e], nm).pack(types.SimpleNamespace(weight=W, bias=None), scale, zero, g_idx)
        q._invalidate()


__all__ = ["QuantMoEExperts", "moe_forward", "pack_moe_experts", "dense_expert_modules", "make_quant_experts", "moe_route", "router_plan",
           "inject_fused_router", "remove_fused_router", "moe_shared_forward", "shared_plan", "shared_workspace_bytes", "inject_shared_expert",
           "remove_shared_expert", "moe_route_grouped", "router_grouped_plan"]
