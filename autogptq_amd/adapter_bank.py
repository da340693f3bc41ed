"""Per-row LoRA adapter banks on mi355x ``QuantLinear`` layers: one batch whose rows belong to different fine-tunes of one GPTQ base.

``LoraQuantLinear`` (lora.py) applies ONE adapter to every row of a call.  A server's batch mixes tenants: each row needs its own adapter, or none.  A GPTQ
layer cannot merge an adapter, so several fine-tunes of one set of packed weights can only be served at run time:

* ``LoraBankQuantLinear`` keeps ``num_slots`` adapters of a layer in three static buffers (``lora_A_bank [S, r, K]``, ``lora_B_bank [S, N, r]``,
  ``scales [S]``) beside the frozen base layer; ``load_slot`` / ``clear_slot`` write them in place, so a captured hipGraph keeps reading the same addresses;
* ``AdapterRouting`` owns the per-row slot ids of the running step (a static int64 buffer; -1 = no adapter) and the routing table the kernels read.  One
  routing serves every layer of a model step -- ``attach_routing(model, routing)`` hands it to all of them;
* a forward is the base call plus ONE ``gptq_adapter_rows_apply`` on its output (csrc/adapter_rows.hip: a down and an up launch over the routed tiles);
  ``lora_bank_forward_multi`` runs one down and one up launch for layers that share their input (q|k|v, gate|up).  Nothing reads the ids on the host:
  ``routing.set`` + the forwards capture into one graph, and a replay follows the ids then in the static buffer.

Inference only.  There is no torch composition behind the kernels: a bank they would decline (fp32 layers, r outside 8, 16, .., 64) is refused at construction."""
from __future__ import annotations

import ctypes
import math

import torch
import torch.nn as nn

from . import _lib
from .lora import _matches, parse_adapter_key
from .qlinear_mi355x import QuantLinear, _raw_stream, _warn_once, forward_multi

NO_ADAPTER = -1


class AdapterRouting:
    """The per-row adapter slots of a step and the routing table built from them.

    ``ids`` is a static int64 buffer of ``max_rows`` entries; ``set`` fills its first ``rows`` entries and launches ``gptq_adapter_route`` on the current
    stream.  Slots outside ``[0, num_slots)`` -- ``NO_ADAPTER`` (-1) by convention -- mean "base model only"."""

    def __init__(self, max_rows: int, num_slots: int, device):
        if max_rows < 1:
            raise ValueError(f"max_rows must be positive, got {max_rows}")
        if not 1 <= num_slots <= _lib.ADAPTER_MAX_SLOTS:
            raise ValueError(f"num_slots must be in 1..{_lib.ADAPTER_MAX_SLOTS}, got {num_slots}")
        self.max_rows, self.num_slots = int(max_rows), int(num_slots)
        self.device = torch.device(device)
        self.ids = torch.full((self.max_rows,), NO_ADAPTER, dtype=torch.int64, device=self.device)
        self.route_bytes = int(_lib.load().gptq_adapter_route_bytes(self.max_rows, self.num_slots))
        self.route = torch.zeros(self.route_bytes, dtype=torch.uint8, device=self.device)
        self.rows = 0

    def set(self, seq_ids=None, rows_per_seq: int = 1) -> "AdapterRouting":
        """Route a step: sequence ``i`` owns rows ``i * rows_per_seq .. (i + 1) * rows_per_seq - 1`` and runs with adapter slot ``seq_ids[i]``.

        ``seq_ids`` is a sequence of ints or an integer tensor (a device tensor is expanded and copied on the device; nothing here waits for the GPU).
        ``None`` keeps the ids already in the static buffer and the current row count: only the routing kernel runs -- what a captured step calls, so
        that a replay follows whatever was written into ``ids`` since."""
        if seq_ids is not None:
            t = torch.as_tensor(seq_ids, dtype=torch.int64).reshape(-1)
            if rows_per_seq < 1:
                raise ValueError(f"rows_per_seq must be positive, got {rows_per_seq}")
            rows = t.numel() * int(rows_per_seq)
            if rows > self.max_rows:
                raise ValueError(f"AdapterRouting: {rows} rows, the buffers hold {self.max_rows}")
            t = t.to(self.device, non_blocking=True)
            if rows_per_seq != 1:
                t = t[:, None].expand(-1, int(rows_per_seq)).reshape(-1)
            if rows:
                self.ids[:rows].copy_(t)
            self.rows = rows
        if self.rows:
            idx = self.device.index
            with torch.cuda.device(idx):
                _lib.check(_lib.load().gptq_adapter_route(self.ids.data_ptr(), self.rows, self.num_slots, self.route.data_ptr(), self.route_bytes,
                                                         _raw_stream(idx)))
        return self


class LoraBankQuantLinear(nn.Module):
    """``base(x)``, plus for every row m with a slot a = ids[m]: ``scales[a] * (x[m] @ lora_A_bank[a]^T) @ lora_B_bank[a]^T``.

    The banks are zero at construction and without a routing attached the layer is its base, bit for bit.  Ranks below ``r`` are zero-padded
    (``load_slot``); a slot's scale is ``lora_alpha / rank``."""

    def __init__(self, base: QuantLinear, r: int, num_slots: int):
        super().__init__()
        if not isinstance(base, QuantLinear):
            raise TypeError(f"LoraBankQuantLinear wraps an mi355x QuantLinear, got {type(base).__name__}")
        if getattr(base, "epilogue", "none") != "none":      # 'silu_mul' / 'gelu_tanh_mul'
            raise ValueError(f"LoraBankQuantLinear: a '{base.epilogue}' layer applies its activation inside the kernel; the adapter term belongs before the "
                             "activation -- wrap the gate and up layers instead")
        if r < 8 or r > 64 or r % 8:
            raise ValueError(f"LoraBankQuantLinear: r = {r}: the adapter kernels take r in 8, 16, .., 64 (smaller ranks are zero-padded by load_slot)")
        if not 1 <= num_slots <= _lib.ADAPTER_MAX_SLOTS:
            raise ValueError(f"LoraBankQuantLinear: num_slots must be in 1..{_lib.ADAPTER_MAX_SLOTS}, got {num_slots}")
        dtype = base.scales.dtype
        if dtype not in (torch.float16, torch.bfloat16):
            raise ValueError(f"LoraBankQuantLinear: the adapter kernels take fp16 / bf16 layers, this one is {dtype}")
        self.base = base
        self.r, self.num_slots = int(r), int(num_slots)
        self.in_features, self.out_features = base.infeatures, base.outfeatures
        if self.in_features % 32 or self.out_features % 16:
            raise ValueError(f"LoraBankQuantLinear: [{self.in_features} -> {self.out_features}]: the adapter kernels take K % 32 == 0 and N % 16 == 0")
        dev = base.qweight.device
        self.register_buffer("lora_A_bank", torch.zeros((self.num_slots, self.r, self.in_features), dtype=dtype, device=dev))
        self.register_buffer("lora_B_bank", torch.zeros((self.num_slots, self.out_features, self.r), dtype=dtype, device=dev))
        self.register_buffer("scales", torch.zeros((self.num_slots,), dtype=torch.float32, device=dev))
        for p in base.parameters():
            p.requires_grad_(False)
        self.routing = None
        self._struct = None           # (GptqAdapterBank, its pointer array, u / out pointer arrays, the data pointers it was built from)

    def extra_repr(self) -> str:
        return f"r={self.r}, num_slots={self.num_slots}"

    def _apply(self, fn, *args, **kwargs):
        self._struct = None
        return super()._apply(fn, *args, **kwargs)

    # ------------------------------------------------------------------ slots
    def _check_slot(self, slot: int) -> int:
        if not 0 <= int(slot) < self.num_slots:
            raise IndexError(f"slot {slot} outside 0..{self.num_slots - 1}")
        return int(slot)

    @torch.no_grad()
    def load_slot(self, slot: int, lora_A: torch.Tensor, lora_B: torch.Tensor, lora_alpha: float) -> None:
        """Write an adapter (peft's ``lora_A.weight [rank, K]``, ``lora_B.weight [N, rank]``, rank <= r) into ``slot``, in place; scale = alpha / rank."""
        slot = self._check_slot(slot)
        rank = lora_A.shape[0]
        if lora_A.dim() != 2 or lora_B.dim() != 2 or tuple(lora_A.shape) != (rank, self.in_features) or tuple(lora_B.shape) != (self.out_features, rank):
            raise ValueError(f"load_slot: lora_A {tuple(lora_A.shape)} / lora_B {tuple(lora_B.shape)}, the layer expects "
                             f"[rank, {self.in_features}] / [{self.out_features}, rank]")
        if not 1 <= rank <= self.r:
            raise ValueError(f"load_slot: rank {rank} does not fit the bank's r = {self.r}")
        a, b = self.lora_A_bank[slot], self.lora_B_bank[slot]
        a.zero_()
        b.zero_()
        a[:rank].copy_(lora_A)
        b[:, :rank].copy_(lora_B)
        self.scales[slot] = float(lora_alpha) / rank

    @torch.no_grad()
    def clear_slot(self, slot: int) -> None:
        slot = self._check_slot(slot)
        self.lora_A_bank[slot].zero_()
        self.lora_B_bank[slot].zero_()
        self.scales[slot] = 0.0

    # ------------------------------------------------------------------ the call
    def _bank_struct(self):
        ptrs = (self.lora_A_bank.data_ptr(), self.lora_B_bank.data_ptr(), self.scales.data_ptr())
        s = self._struct
        if s is None or s[4] != ptrs:
            L = _lib.GptqAdapterBank()
            L.A, L.B, L.scales = ptrs
            L.K, L.N, L.r, L.slots = self.in_features, self.out_features, self.r, self.num_slots
            L.dtype = _lib.DTYPE_ENUM.get(self.lora_A_bank.dtype, -1)
            arr = (ctypes.POINTER(_lib.GptqAdapterBank) * 1)(ctypes.pointer(L))
            s = self._struct = (L, arr, (ctypes.c_void_p * 1)(), (ctypes.c_void_p * 1)(), ptrs)
        return s

    def _rows_of(self, x: torch.Tensor) -> int:
        """The routed row count of this call (0: no routing attached, or an empty one), after the checks every call makes."""
        if torch.is_grad_enabled() and x.requires_grad:
            raise RuntimeError("LoraBankQuantLinear is inference only: call it under torch.no_grad() (training goes through LoraQuantLinear)")
        rt = self.routing
        if rt is None or rt.rows == 0:
            return 0
        if x.shape[-1] != self.in_features or math.prod(x.shape[:-1]) != rt.rows:
            raise ValueError(f"LoraBankQuantLinear: x is {tuple(x.shape)}; the attached routing holds {rt.rows} rows of {self.in_features} features")
        if rt.num_slots != self.num_slots:
            raise ValueError(f"LoraBankQuantLinear: the routing was built for {rt.num_slots} slots, the bank holds {self.num_slots}")
        return rt.rows

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        T = self.lora_A_bank.dtype
        x_dtype = x.dtype
        if x_dtype != T:
            _warn_once(f"LoraBankQuantLinear: activation dtype {x_dtype} != weight dtype {T}; casting the activation to {T} (the result is cast back).")
            x = x.to(T)
        M = self._rows_of(x)
        y = self.base(x)
        if M:
            y = _apply_banks([self], x, [y], self.routing, M)[0]
        return y.to(x_dtype) if x_dtype != T else y


def _apply_banks(layers, x: torch.Tensor, ys, routing: AdapterRouting, M: int):
    """ys[i] += the routed adapter term of layers[i], in place (a copy where the base output is not dense and aligned): one gptq_adapter_rows_apply per
    group of up to 4 layers."""
    x2 = x.reshape(-1, x.shape[-1])
    if not x2.is_contiguous() or x2.data_ptr() % 16:
        x2 = x2.clone(memory_format=torch.contiguous_format)
    ys = [y if y.is_contiguous() and y.data_ptr() % 16 == 0 else y.clone(memory_format=torch.contiguous_format) for y in ys]
    lib = _lib.load()
    idx = x2.device.index
    for i in range(0, len(layers), _lib.LORA_MAX):
        grp, gys = layers[i:i + _lib.LORA_MAX], ys[i:i + _lib.LORA_MAX]
        n = len(grp)
        us = [torch.empty((M, l.r), dtype=x2.dtype, device=x2.device) for l in grp]
        if n == 1:
            _, arr, uptr, optr, _ = grp[0]._bank_struct()
            uptr[0], optr[0] = us[0].data_ptr(), gys[0].data_ptr()
        else:
            arr = (ctypes.POINTER(_lib.GptqAdapterBank) * n)(*[ctypes.pointer(l._bank_struct()[0]) for l in grp])
            uptr = (ctypes.c_void_p * n)(*[u.data_ptr() for u in us])
            optr = (ctypes.c_void_p * n)(*[y.data_ptr() for y in gys])
        with torch.cuda.device(idx):
            _lib.check(lib.gptq_adapter_rows_apply(arr, n, x2.data_ptr(), uptr, optr, routing.route.data_ptr(), M, _raw_stream(idx)))
    return ys


def lora_bank_forward_multi(layers, x: torch.Tensor):
    """``[l(x) for l in layers]`` for LoraBankQuantLinears that read one input and share one routing (q|k|v, gate|up): ``forward_multi`` on the bases, then
    ONE down launch and ONE up launch for all banks (groups of up to 4).  Values are bit-identical to the per-layer calls."""
    layers = list(layers)
    if not all(isinstance(l, LoraBankQuantLinear) for l in layers):
        raise TypeError("lora_bank_forward_multi takes LoraBankQuantLinear layers")
    a = layers[0]
    T = a.lora_A_bank.dtype
    if any(l.lora_A_bank.dtype != T or l.in_features != a.in_features or l.routing is not a.routing for l in layers):
        raise RuntimeError("lora_bank_forward_multi: the layers must share the input's feature count, the weight dtype and the routing")
    if any(getattr(l.base, "_parts", None) is not None for l in layers):
        return [l(x) for l in layers]
    x_dtype = x.dtype
    xw = x.to(T) if x_dtype != T else x
    M = a._rows_of(xw)
    for l in layers[1:]:
        l._rows_of(xw)
    ys = forward_multi([l.base for l in layers], xw)
    if M:
        ys = _apply_banks(layers, xw, list(ys), a.routing, M)
    return [y.to(x_dtype) for y in ys] if x_dtype != T else list(ys)


# ---------------------------------------------------------------------- model helpers
def inject_lora_bank(model: nn.Module, target_modules, r: int, num_slots: int) -> dict:
    """Wrap every mi355x QuantLinear of ``model`` whose name is, or ends in, one of ``target_modules`` (peft's rule, as ``inject_lora``) in a
    LoraBankQuantLinear.  Returns {module name: LoraBankQuantLinear}."""
    found = {n: m for n, m in model.named_modules() if isinstance(m, QuantLinear) and _matches(n, target_modules)}
    out = {}
    for name, base in found.items():
        parent_name, _, attr = name.rpartition(".")
        parent = model.get_submodule(parent_name) if parent_name else model
        if isinstance(parent, LoraBankQuantLinear):                 # already wrapped
            continue
        wrapped = LoraBankQuantLinear(base, r, num_slots)
        wrapped.train(model.training)
        setattr(parent, attr, wrapped)
        out[name] = wrapped
    return out


def lora_bank_layers(model: nn.Module) -> dict:
    return {n: m for n, m in model.named_modules() if isinstance(m, LoraBankQuantLinear)}


def load_adapter_slot(model: nn.Module, slot: int, state_dict: dict, config: dict) -> dict:
    """Load one adapter (peft's keys, as ``load_lora_adapter`` takes them; ``config``: peft's adapter_config.json as a dict, ``lora_alpha`` is read) into
    ``slot`` of every bank layer the state dict names.  Bank layers it does not name get the slot cleared: the adapter does not touch them.  A key that
    names no bank layer, or a layer with only one of lora_A / lora_B, raises KeyError.  Returns {name: LoraBankQuantLinear} of the layers written."""
    layers = lora_bank_layers(model)
    if not layers:
        raise RuntimeError("load_adapter_slot: the model carries no adapter banks (inject_lora_bank first)")
    got: dict = {}
    for key, value in state_dict.items():
        name, which = parse_adapter_key(key, "load_adapter_slot")
        if name not in layers:
            raise KeyError(f"load_adapter_slot: {key} names no bank layer of the model")
        got.setdefault(name, {})[which] = value
    half = [n for n, d in got.items() if len(d) != 2]
    if half:
        raise KeyError(f"load_adapter_slot: the state dict lacks lora_A or lora_B of {half[:4]}{' ...' if len(half) > 4 else ''}")
    for name, layer in layers.items():
        if name in got:
            layer.load_slot(slot, got[name]["lora_A"], got[name]["lora_B"], config["lora_alpha"])
        else:
            layer.clear_slot(slot)
    return {n: layers[n] for n in got}


def attach_routing(model: nn.Module, routing: "AdapterRouting | None") -> None:
    """Hand one routing to every bank layer of the model (None detaches: the layers are their bases again)."""
    for name, m in lora_bank_layers(model).items():
        if routing is not None and routing.num_slots != m.num_slots:
            raise ValueError(f"attach_routing: {name} holds {m.num_slots} slots, the routing was built for {routing.num_slots}")
        m.routing = routing


__all__ = ["AdapterRouting", "LoraBankQuantLinear", "lora_bank_forward_multi", "inject_lora_bank", "lora_bank_layers", "load_adapter_slot",
           "attach_routing", "NO_ADAPTER"]
