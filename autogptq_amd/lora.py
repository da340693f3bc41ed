"""LoRA adapters on mi355x ``QuantLinear`` layers: ``LoraQuantLinear`` and the model helpers around it.

The capability of the reference's ``get_gptq_peft_model`` / ``GPTQLoraLinear`` (auto_gptq/utils/peft_utils.py:58-176) for this backend, without ``peft``:

* a GPTQ layer cannot merge its adapter -- ``W`` is int4 on a fixed grid, ``W + s B A`` has no packed form (``GPTQLoraLinear.merge`` raises,
  peft_utils.py:94-98) -- so every call, decode included, pays ``base(x) + s (x A^T) B^T``;
* the base product stays the ordinary ``QuantLinear`` call (any layer it takes: act-order, fused-QKV ``_parts``, released rows);
* the adapter branch is ONE ``gptq_lora_apply`` on the base output (csrc/lora.hip: a down and an up launch, fp32 sums, one rounding each, in place) --
  for layers that share their input (q|k|v, gate|up) ``lora_forward_multi`` runs one down and one up launch for all of them;
* parameters carry peft's names and shapes (``lora_A.weight [r, K]``, ``lora_B.weight [N, r]``), so ``lora_state_dict`` / ``load_lora_adapter`` speak
  peft's adapter format (``base_model.model.<name>.lora_A.weight``), dicts in and dicts out;
* gradients: the base term goes through the existing ``_GradInput`` node (gptq_grad_input), the adapter term through one autograd Function whose
  backward runs on torch matmuls in fp32 -- or, with ``fused_backward=True`` (opt-in), as ONE ``gptq_lora_backward`` (csrc/adapter_grad.hip and the
  forward's kernels on transposed copies: no activation-sized fp32 temporary).  With the flag on, ``lora_forward_multi`` under
  grad is one autograd node per group: one fused apply forward, one ``gptq_lora_backward`` with a shared dX backward.

What the kernels decline (fp32 layers, r outside 8, 16, .., 64, odd shapes) falls back to the torch composition with one warning.
"""
from __future__ import annotations

import ctypes
import math

import torch
import torch.nn as nn
from torch.autograd.function import once_differentiable

from . import _lib
from .qlinear_mi355x import QuantLinear, _raw_stream, _warn_once, forward_multi

MERGE_MESSAGE = "gptq model not support merge lora adapter"          # peft_utils.py:94-98


class _AdapterWeight(nn.Module):
    """Holder of one ``weight`` parameter, so the names are peft's: ``lora_A.weight`` / ``lora_B.weight``."""

    def __init__(self, rows: int, cols: int, dtype, device):
        super().__init__()
        self.weight = nn.Parameter(torch.zeros((rows, cols), dtype=dtype, device=device))


class LoraQuantLinear(nn.Module):
    """``base(x) + (lora_alpha / r) * (dropout(x) @ lora_A.weight^T) @ lora_B.weight^T`` around a frozen mi355x ``QuantLinear``.

    ``lora_A`` is xavier-uniform and ``lora_B`` zero at construction (peft_utils.py:89-92): a fresh adapter leaves the layer's output unchanged, bit for
    bit.  The master weights are ``adapter_dtype`` (fp32 by default); the kernels read copies in the layer dtype.  Under ``no_grad`` the copies are kept
    and refreshed IN PLACE when a parameter's ``_version`` moves, so a captured hipGraph keeps reading the same addresses: after an optimiser step call
    ``refresh_adapter()`` (or ``refresh_lora(model)``) before the next replay -- no re-capture.  Under grad they are a fresh ``.to(dtype)`` of the
    masters inside the autograd Function, whose backward hands the masters their gradient in their own dtype."""

    def __init__(self, base: QuantLinear, r: int, lora_alpha: float, lora_dropout: float = 0.0, adapter_dtype=torch.float32,
                 fused_backward: bool = False):
        super().__init__()
        if not isinstance(base, QuantLinear):
            raise TypeError(f"LoraQuantLinear wraps an mi355x QuantLinear, got {type(base).__name__}")
        if getattr(base, "epilogue", "none") != "none":      # 'silu_mul' / 'gelu_tanh_mul'
            raise ValueError(f"LoraQuantLinear: a '{base.epilogue}' layer applies its activation inside the kernel; the adapter term belongs before the "
                             "activation -- wrap the gate and up layers instead")
        if r <= 0:
            raise ValueError(f"r must be positive, got {r}")
        self.base = base
        self.r, self.lora_alpha, self.lora_dropout = int(r), lora_alpha, float(lora_dropout)
        self.scaling = lora_alpha / r
        self.in_features, self.out_features = base.infeatures, base.outfeatures
        dev = base.qweight.device
        self.lora_A = _AdapterWeight(self.r, self.in_features, adapter_dtype, dev)
        self.lora_B = _AdapterWeight(self.out_features, self.r, adapter_dtype, dev)
        nn.init.xavier_uniform_(self.lora_A.weight)
        for p in base.parameters():
            p.requires_grad_(False)
        self._copies = None           # (A16, B16, version of A, version of B)
        self._struct = None           # (GptqLora, its pointer array, u / out pointer arrays, the tensors it points to)
        self._fused = None            # None: not asked yet; True / False: gptq_lora_apply takes this adapter
        self.fused_backward = bool(fused_backward)   # opt-in: the adapter's backward as one gptq_lora_backward instead of torch matmuls
        self._fused_bwd = None        # None: not asked yet; True / False: gptq_lora_backward takes this adapter

    # ------------------------------------------------------------------ reference surface
    def merge(self):
        raise NotImplementedError(MERGE_MESSAGE)

    def unmerge(self):
        raise NotImplementedError(MERGE_MESSAGE)

    def extra_repr(self) -> str:
        return f"r={self.r}, lora_alpha={self.lora_alpha}, lora_dropout={self.lora_dropout}"

    # ------------------------------------------------------------------ 16-bit copies
    def _layer_dtype(self):
        return self.base.scales.dtype

    def _kernel_weights(self, dtype):
        """The copies of lora_A / lora_B the kernels read under no_grad: made once, refreshed in place when a parameter changed."""
        a, b = self.lora_A.weight, self.lora_B.weight
        c = self._copies
        if c is not None and c[0].dtype == dtype and c[0].device == a.device and c[0].shape == a.shape and c[1].shape == b.shape:
            if c[2] != a._version or c[3] != b._version:
                if c[0].data_ptr() != a.data_ptr():
                    c[0].copy_(a.detach())
                    c[1].copy_(b.detach())
                self._copies = c = (c[0], c[1], a._version, b._version)
            return c[0], c[1]
        if a.dtype == dtype and a.is_contiguous() and b.is_contiguous():
            A16, B16 = a.detach(), b.detach()                       # the parameters themselves: nothing to refresh
        else:
            A16, B16 = a.detach().to(dtype).contiguous(), b.detach().to(dtype).contiguous()
        self._copies = (A16, B16, a._version, b._version)
        self._struct = None
        return A16, B16

    def refresh_adapter(self) -> None:
        """Bring the kernels' copies up to date with lora_A / lora_B (in place: a captured graph reads the new values at its next replay)."""
        with torch.no_grad():
            self._kernel_weights(self._layer_dtype())

    def _apply(self, fn, *args, **kwargs):
        self._copies = self._struct = self._fused = self._fused_bwd = None
        return super()._apply(fn, *args, **kwargs)

    # ------------------------------------------------------------------ the fused call
    def _lora_struct(self, A16, B16):
        s = self._struct
        if s is None or s[4] is not A16 or s[5] is not B16:
            L = _lib.GptqLora()
            L.A, L.B = A16.data_ptr(), B16.data_ptr()
            L.K, L.N, L.r = self.in_features, self.out_features, self.r
            L.dtype = _lib.DTYPE_ENUM.get(A16.dtype, -1)
            L.scale = float(self.scaling)
            arr = (ctypes.POINTER(_lib.GptqLora) * 1)(ctypes.pointer(L))
            s = self._struct = (L, arr, (ctypes.c_void_p * 1)(), (ctypes.c_void_p * 1)(), A16, B16)
        return s

    def fused_ok(self, dtype=None) -> bool:
        """Whether gptq_lora_apply takes this adapter (host-only query, asked once): fp16 / bf16 layer, r in 8, 16, .., 64, K % 32 == 0, N % 16 == 0."""
        if self._fused is None:
            L = _lib.GptqLora()
            L.A = L.B = 0x1000
            L.K, L.N, L.r = self.in_features, self.out_features, self.r
            L.dtype = _lib.DTYPE_ENUM.get(dtype or self._layer_dtype(), -1)
            plan = _lib.describe_lora_plan([L], 1)
            self._fused = plan["path"] == "lora"
            if not self._fused:
                _warn_once(f"LoraQuantLinear: the adapter kernels decline this layer ({plan.get('reason')}); composing the adapter branch in torch")
        return self._fused

    def fused_backward_ok(self, dtype=None) -> bool:
        """Whether gptq_lora_backward takes this adapter (host-only query, asked once): as fused_ok, and N % 32 == 0 (N is a summed length there)."""
        if self._fused_bwd is None:
            L = _lib.GptqLora()
            L.K, L.N, L.r = self.in_features, self.out_features, self.r
            L.dtype = _lib.DTYPE_ENUM.get(dtype or self._layer_dtype(), -1)
            plan = _lib.describe_lora_backward_plan([L], 1)
            self._fused_bwd = plan["path"] == "lora_backward"
            if not self._fused_bwd:
                _warn_once(f"LoraQuantLinear: gptq_lora_backward declines this layer ({plan.get('reason')}); the adapter's backward runs on torch matmuls")
        return self._fused_bwd

    def _adapter_(self, y: torch.Tensor, xl: torch.Tensor, A16: torch.Tensor, B16: torch.Tensor) -> torch.Tensor:
        """y += scaling * (xl @ A16^T) @ B16^T, in place where the kernels run; returns (y, u)."""
        K, N = self.in_features, self.out_features
        x2 = xl.reshape(-1, K)
        M = x2.shape[0]
        if M == 0:
            return y, x2.new_empty((0, self.r))
        if self.fused_ok(A16.dtype) and y.is_contiguous() and y.data_ptr() % 16 == 0:
            if not x2.is_contiguous() or x2.data_ptr() % 16:
                x2 = x2.clone(memory_format=torch.contiguous_format)
            L, arr, uptr, optr, _, _ = self._lora_struct(A16, B16)
            u = torch.empty((M, self.r), dtype=A16.dtype, device=y.device)
            uptr[0], optr[0] = u.data_ptr(), y.data_ptr()
            idx = y.device.index
            with torch.cuda.device(idx):
                rc = _lib.load().gptq_lora_apply(arr, 1, x2.data_ptr(), uptr, optr, M, _raw_stream(idx))
            if rc == 0:
                return y, u
            if rc != 3:                                             # GPTQ_ERR_UNSUPPORTED falls through to the composition
                _lib.check(rc)
            _warn_once(f"LoraQuantLinear: gptq_lora_apply declined a call ({_lib.load().gptq_last_error().decode()}); composing the adapter branch in torch")
        u = x2 @ A16.t()
        y2 = y.reshape(-1, N)
        y2 += (u @ B16.t()) * self.scaling
        return y, u

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        T = self._layer_dtype()
        x_dtype = x.dtype
        if x_dtype != T:
            _warn_once(f"LoraQuantLinear: activation dtype {x_dtype} != weight dtype {T}; casting the activation to {T} (the result is cast back).")
            x = x.to(T)
        y = self.base(x)
        out = self._after_base(y, x)
        return out.to(x_dtype) if x_dtype != T else out

    def _after_base(self, y: torch.Tensor, x: torch.Tensor) -> torch.Tensor:
        """The adapter branch on the base output y (layer dtype); x is the base's input in the layer dtype."""
        xl = nn.functional.dropout(x, self.lora_dropout, True) if self.training and self.lora_dropout > 0.0 else x
        a, b = self.lora_A.weight, self.lora_B.weight
        if torch.is_grad_enabled() and (a.requires_grad or b.requires_grad or xl.requires_grad or y.requires_grad):
            return _LoraApply.apply(y, xl, a, b, self)
        A16, B16 = self._kernel_weights(y.dtype)
        if not y.is_contiguous():
            y = y.contiguous()
        return self._adapter_(y, xl, A16, B16)[0]


class _LoraApply(torch.autograd.Function):
    """out = y + scaling * (x_lora @ A^T) @ B^T through gptq_lora_apply (the same launches and values as the no_grad call, on a copy of y).  Takes the
    master weights and casts them to the layer dtype itself; saves x_lora, u and the 16-bit A / B.  Backward, with du = scaling * (dY @ B):
    dA = du^T @ x_lora,  dB = scaling * dY^T @ u,  dX_lora = du @ A,  dY passes through to the base output.  Torch matmuls in fp32 (r/N-sized corrections
    beside gptq_grad_input); dA / dB are handed to the masters in the masters' dtype, never rounded to 16 bits on the way.  No double backward.
    A layer with ``fused_backward`` that gptq_lora_backward accepts runs the same four products as ONE C call (du unscaled and rounded once to the layer
    dtype; dA / dB in fp32, so fp32 masters get them with no 16-bit hop) and honours needs_input_grad: a frozen master or an x without grad is not computed."""

    @staticmethod
    def forward(ctx, y, xl, a, b, layer):
        T = y.dtype
        A16, B16 = a.detach().to(T).contiguous(), b.detach().to(T).contiguous()
        out = y.clone(memory_format=torch.contiguous_format)
        layer._struct = None                                        # these copies live for this call only
        _, u = layer._adapter_(out, xl, A16, B16)
        layer._struct = None
        ctx.save_for_backward(xl, u, A16, B16)
        ctx.scaling = float(layer.scaling)
        ctx.master_dtypes = (a.dtype, b.dtype)
        ctx.fused = bool(layer.fused_backward) and out.is_cuda and layer.fused_backward_ok(T)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        xl, u, A16, B16 = ctx.saved_tensors
        need_y, need_x, need_a, need_b = ctx.needs_input_grad[:4]
        N, K = B16.shape[0], A16.shape[1]
        if ctx.fused and (need_x or need_a or need_b):
            res = _fused_backward(xl.reshape(-1, K), [(A16, B16, u, dy, ctx.scaling, need_a, need_b)], need_x)
            if res is not None:
                dx2, ((da, db),) = res
                return ((dy if need_y else None), (dx2.reshape(xl.shape) if need_x else None),
                        (da.to(ctx.master_dtypes[0]) if need_a else None), (db.to(ctx.master_dtypes[1]) if need_b else None), None)
        dy2 = dy.reshape(-1, N).float()
        dx = da = db = None
        if need_x or need_a:
            du = (dy2 @ B16.float()) * ctx.scaling
            if need_a:
                da = (du.t() @ xl.reshape(-1, K).float()).to(ctx.master_dtypes[0])
            if need_x:
                dx = (du @ A16.float()).to(xl.dtype).reshape(xl.shape)
        if need_b:
            db = ((dy2.t() @ u.float()) * ctx.scaling).to(ctx.master_dtypes[1])
        return (dy if need_y else None), dx, da, db, None


def _fused_backward(x2: torch.Tensor, items, need_x: bool, dx: torch.Tensor = None):
    """ONE gptq_lora_backward for up to LORA_MAX adapters that share x2 [M, K] (layer dtype).  items: (A16 [r, K], B16 [N, r], u [M, r], dY [.., N], scale,
    need_a, need_b) per adapter.  Returns (dX [M, K] or None, [(dA fp32 [r, K] or None, dB fp32 [N, r] or None)]); dx: a dX to go on adding to (the next
    group of one input).  None when the library declines the call (the caller composes the backward in torch)."""
    T, dev = x2.dtype, x2.device
    M, K = x2.shape
    n = len(items)
    if need_x and dx is None:
        dx = torch.zeros((M, K), dtype=T, device=dev)
    if M == 0:
        return (dx if need_x else None), [(torch.zeros((a.shape[0], K), dtype=torch.float32, device=dev) if na else None,
                                           torch.zeros(tuple(b.shape), dtype=torch.float32, device=dev) if nb else None) for a, b, _, _, _, na, nb in items]
    if not x2.is_contiguous() or x2.data_ptr() % 16:
        x2 = x2.clone(memory_format=torch.contiguous_format)
    lib = _lib.load()
    loras, grads, keep, outs = [], [], [], []
    for A16, B16, u, dy, scale, need_a, need_b in items:
        N, r = B16.shape
        dy2 = dy.reshape(-1, N)
        if dy2.dtype != T or not dy2.is_contiguous() or dy2.data_ptr() % 16:
            dy2 = dy2.to(T).clone(memory_format=torch.contiguous_format)
        if not u.is_contiguous() or u.data_ptr() % 16:
            u = u.clone(memory_format=torch.contiguous_format)
        At, Bt = A16.t().contiguous(), B16.t().contiguous()        # r-sized copies: the reused kernels' operands as they want them
        du = torch.empty((M, r), dtype=T, device=dev)
        da = torch.empty((r, K), dtype=torch.float32, device=dev) if need_a else None
        db = torch.empty((N, r), dtype=torch.float32, device=dev) if need_b else None
        L = _lib.GptqLora()
        L.K, L.N, L.r, L.dtype, L.scale = K, N, r, _lib.DTYPE_ENUM.get(T, -1), float(scale)
        G = _lib.GptqLoraGrad()
        G.At, G.Bt, G.u, G.dY, G.du = At.data_ptr(), Bt.data_ptr(), u.data_ptr(), dy2.data_ptr(), du.data_ptr()
        G.dA, G.dB = (da.data_ptr() if need_a else None), (db.data_ptr() if need_b else None)
        loras.append(L)
        grads.append(G)
        keep.append((At, Bt, u, dy2, du))
        outs.append((da, db))
    la = (ctypes.POINTER(_lib.GptqLora) * n)(*[ctypes.pointer(L) for L in loras])
    ga = (ctypes.POINTER(_lib.GptqLoraGrad) * n)(*[ctypes.pointer(G) for G in grads])
    idx = dev.index
    with torch.cuda.device(idx):
        nbytes = lib.gptq_lora_backward_workspace_bytes(la, n, M)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev) if nbytes else None
        rc = lib.gptq_lora_backward(la, ga, n, x2.data_ptr(), dx.data_ptr() if need_x else None, M, ws.data_ptr() if nbytes else None, nbytes,
                                    _raw_stream(idx))
    if rc == 3:                                                     # GPTQ_ERR_UNSUPPORTED: nothing was launched
        _warn_once(f"LoraQuantLinear: gptq_lora_backward declined a call ({lib.gptq_last_error().decode()}); the adapter's backward runs on torch matmuls")
        return None
    _lib.check(rc)
    return (dx if need_x else None), outs


class _LoraGroupApply(torch.autograd.Function):
    """The adapter branches of up to LORA_MAX layers that read one input, as ONE autograd node: forward is one gptq_lora_apply on copies of the base
    outputs (the values of the per-layer calls, bit for bit), backward one gptq_lora_backward with one shared dX -- x's adapter gradient is produced once
    instead of once per layer.  Arguments: (layers, x, y_0 .., a_0 .., b_0 ..); the masters are cast to the layer dtype here, as _LoraApply does."""

    @staticmethod
    def forward(ctx, layers, xw, *rest):
        n = len(layers)
        ys, As, Bs = rest[:n], rest[n:2 * n], rest[2 * n:]
        T = ys[0].dtype
        K = layers[0].in_features
        x2 = xw.reshape(-1, K)
        if not x2.is_contiguous() or x2.data_ptr() % 16:
            x2 = x2.clone(memory_format=torch.contiguous_format)
        M = x2.shape[0]
        A16 = [a.detach().to(T).contiguous() for a in As]
        B16 = [b.detach().to(T).contiguous() for b in Bs]
        outs = [y.clone(memory_format=torch.contiguous_format) for y in ys]
        us = [torch.empty((M, l.r), dtype=T, device=x2.device) for l in layers]
        structs = []
        for l, a16, b16 in zip(layers, A16, B16):
            L = _lib.GptqLora()
            L.A, L.B = a16.data_ptr(), b16.data_ptr()
            L.K, L.N, L.r, L.dtype, L.scale = K, l.out_features, l.r, _lib.DTYPE_ENUM.get(T, -1), float(l.scaling)
            structs.append(L)
        arr = (ctypes.POINTER(_lib.GptqLora) * n)(*[ctypes.pointer(s) for s in structs])
        uptr = (ctypes.c_void_p * n)(*[u.data_ptr() for u in us])
        optr = (ctypes.c_void_p * n)(*[o.data_ptr() for o in outs])
        idx = x2.device.index
        with torch.cuda.device(idx):
            _lib.check(_lib.load().gptq_lora_apply(arr, n, x2.data_ptr(), uptr, optr, M, _raw_stream(idx)))
        ctx.save_for_backward(x2, *us, *A16, *B16)
        ctx.n = n
        ctx.x_shape = xw.shape
        ctx.scalings = [float(l.scaling) for l in layers]
        ctx.master_dtypes = [(a.dtype, b.dtype) for a, b in zip(As, Bs)]
        return tuple(outs)

    @staticmethod
    @once_differentiable
    def backward(ctx, *dys):
        n = ctx.n
        saved = ctx.saved_tensors
        x2, us, A16, B16 = saved[0], saved[1:1 + n], saved[1 + n:1 + 2 * n], saved[1 + 2 * n:]
        need = ctx.needs_input_grad
        need_x, need_y, need_a, need_b = need[1], need[2:2 + n], need[2 + n:2 + 2 * n], need[2 + 2 * n:]
        dx, das, dbs = None, [None] * n, [None] * n
        if need_x or any(need_a) or any(need_b):
            items = [(A16[i], B16[i], us[i], dys[i], ctx.scalings[i], need_a[i], need_b[i]) for i in range(n)]
            res = _fused_backward(x2, items, need_x)
            if res is None:                                         # declined at call time: the same products in torch, per adapter
                res = _torch_backward(x2, items, need_x)
            dx, outs = res
            for i, (da, db) in enumerate(outs):
                das[i] = da.to(ctx.master_dtypes[i][0]) if need_a[i] else None
                dbs[i] = db.to(ctx.master_dtypes[i][1]) if need_b[i] else None
        return (None, (dx.reshape(ctx.x_shape) if need_x else None), *[(dys[i] if need_y[i] else None) for i in range(n)], *das, *dbs)


def _torch_backward(x2, items, need_x):
    """_fused_backward's contract on torch matmuls in fp32 (_LoraApply.backward's formulas)."""
    dx = torch.zeros(x2.shape, dtype=torch.float32, device=x2.device) if need_x else None
    outs = []
    for A16, B16, u, dy, scale, need_a, need_b in items:
        dy2 = dy.reshape(-1, B16.shape[0]).float()
        da = db = None
        if need_x or need_a:
            du = (dy2 @ B16.float()) * scale
            if need_a:
                da = du.t() @ x2.float()
            if need_x:
                dx += du @ A16.float()
        if need_b:
            db = (dy2.t() @ u.float()) * scale
        outs.append((da, db))
    return (dx.to(x2.dtype) if need_x else None), outs


def lora_forward_multi(layers, x: torch.Tensor):
    """``[l(x) for l in layers]`` for LoraQuantLinears that read one input (q|k|v, gate|up): ``forward_multi`` on the bases, then ONE down launch and ONE
    up launch for all adapters (groups of up to 4).  Values are bit-identical to the per-layer calls.  Dropout in training mode, a call that records
    gradients, bases that are not single layers, or adapters the kernels decline: per-layer calls.  A call that records gradients whose layers all have
    ``fused_backward`` on (and are accepted by gptq_lora_backward) stays grouped: one autograd node per group of up to 4 (_LoraGroupApply)."""
    layers = list(layers)
    plain = all(isinstance(l, LoraQuantLinear) and getattr(l.base, "_parts", None) is None for l in layers)
    if not plain or any(l.training and l.lora_dropout > 0.0 for l in layers):
        return [l(x) for l in layers]
    a = layers[0]
    T = a._layer_dtype()
    if any(l._layer_dtype() != T or l.in_features != a.in_features for l in layers):
        raise RuntimeError("lora_forward_multi: the layers must share the input's feature count and the weight dtype")
    x_dtype = x.dtype
    xw = x.to(T) if x_dtype != T else x
    ys = forward_multi([l.base for l in layers], xw)
    grad = torch.is_grad_enabled() and (xw.requires_grad or any(l.lora_A.weight.requires_grad or l.lora_B.weight.requires_grad for l in layers))
    K = a.in_features
    x2 = xw.reshape(-1, K)
    M = x2.shape[0]
    fused = not grad and M > 0 and all(l.fused_ok(T) for l in layers) and all(y.is_contiguous() and y.data_ptr() % 16 == 0 for y in ys)
    group = (grad and M > 0 and x2.is_cuda and all(l.fused_backward and l.fused_ok(T) and l.fused_backward_ok(T) for l in layers))
    if group:
        outs = []
        for i in range(0, len(layers), _lib.LORA_MAX):
            grp = tuple(layers[i:i + _lib.LORA_MAX])
            outs += list(_LoraGroupApply.apply(grp, xw, *ys[i:i + _lib.LORA_MAX], *[l.lora_A.weight for l in grp], *[l.lora_B.weight for l in grp]))
    elif not fused:
        outs = [l._after_base(y, xw) for l, y in zip(layers, ys)]
    else:
        if not x2.is_contiguous() or x2.data_ptr() % 16:
            x2 = x2.clone(memory_format=torch.contiguous_format)
        lib = _lib.load()
        idx = x2.device.index
        for i in range(0, len(layers), _lib.LORA_MAX):
            grp, gys = layers[i:i + _lib.LORA_MAX], ys[i:i + _lib.LORA_MAX]
            n = len(grp)
            structs = [l._lora_struct(*l._kernel_weights(T))[0] for l in grp]
            arr = (ctypes.POINTER(_lib.GptqLora) * n)(*[ctypes.pointer(s) for s in structs])
            us = [torch.empty((M, l.r), dtype=T, device=x2.device) for l in grp]
            uptr = (ctypes.c_void_p * n)(*[u.data_ptr() for u in us])
            optr = (ctypes.c_void_p * n)(*[y.data_ptr() for y in gys])
            with torch.cuda.device(idx):
                _lib.check(lib.gptq_lora_apply(arr, n, x2.data_ptr(), uptr, optr, M, _raw_stream(idx)))
        outs = list(ys)
    return [o.to(x_dtype) for o in outs] if x_dtype != T else outs


# ---------------------------------------------------------------------- model helpers
def _matches(name: str, target_modules) -> bool:
    if isinstance(target_modules, str):
        target_modules = [target_modules]
    return any(name == t or name.endswith("." + t) for t in target_modules)


def inject_lora(model: nn.Module, target_modules, r: int, lora_alpha: float, lora_dropout: float = 0.0, adapter_dtype=torch.float32,
                fused_backward: bool = False) -> dict:
    """Wrap every mi355x QuantLinear of ``model`` whose name is, or ends in, one of ``target_modules`` (peft's rule; get_gptq_peft_model,
    peft_utils.py:126-176) in a LoraQuantLinear.  Returns {module name: LoraQuantLinear}.  ``fused_backward``: the layers' opt-in switch (LoraQuantLinear)."""
    found = {n: m for n, m in model.named_modules() if isinstance(m, QuantLinear) and _matches(n, target_modules)}
    out = {}
    for name, base in found.items():
        parent_name, _, attr = name.rpartition(".")
        parent = model.get_submodule(parent_name) if parent_name else model
        if isinstance(parent, LoraQuantLinear):                     # already wrapped
            continue
        wrapped = LoraQuantLinear(base, r, lora_alpha, lora_dropout, adapter_dtype, fused_backward)
        wrapped.train(model.training)
        setattr(parent, attr, wrapped)
        out[name] = wrapped
    return out


def set_lora_fused_backward(model: nn.Module, on: bool = True) -> None:
    """Switch every adapted layer's backward between one gptq_lora_backward (on) and the torch matmuls (off, the default)."""
    for m in lora_layers(model).values():
        m.fused_backward = bool(on)


def lora_layers(model: nn.Module) -> dict:
    return {n: m for n, m in model.named_modules() if isinstance(m, LoraQuantLinear)}


def lora_state_dict(model: nn.Module) -> dict:
    """The adapter weights in peft's format: ``base_model.model.<name>.lora_A.weight`` / ``.lora_B.weight`` (detached, the parameters' own dtype)."""
    sd = {}
    for name, m in lora_layers(model).items():
        sd[f"base_model.model.{name}.lora_A.weight"] = m.lora_A.weight.detach().clone()
        sd[f"base_model.model.{name}.lora_B.weight"] = m.lora_B.weight.detach().clone()
    return sd


def parse_adapter_key(key: str, who: str = "parse_adapter_key"):
    """(module name, "lora_A" | "lora_B") of one key of a peft adapter state dict: ``base_model.model.<name>.lora_A.weight``, the prefix optional and the
    ``.default`` infix of peft's in-memory form accepted.  Any other key raises KeyError."""
    k = key[len("base_model.model."):] if key.startswith("base_model.model.") else key
    k = k.replace(".lora_A.default.", ".lora_A.").replace(".lora_B.default.", ".lora_B.")
    for which in ("lora_A", "lora_B"):
        suffix = f".{which}.weight"
        if k.endswith(suffix):
            return k[:-len(suffix)], which
    raise KeyError(f"{who}: unexpected key {key}")


def load_lora_adapter(model: nn.Module, state_dict: dict, config: dict) -> dict:
    """Inject the adapters ``config`` describes (``r``, ``lora_alpha``, ``target_modules``, ``lora_dropout``: peft's adapter_config.json as a dict) where
    the model does not carry them yet and load ``state_dict`` (peft's keys; the ``.default`` infix is accepted).  Returns {name: LoraQuantLinear}."""
    layers = lora_layers(model)
    if not layers:
        inject_lora(model, config["target_modules"], config["r"], config["lora_alpha"], config.get("lora_dropout", 0.0))
        layers = lora_layers(model)
    seen = set()
    for key, value in state_dict.items():
        name, which = parse_adapter_key(key, "load_lora_adapter")
        if name not in layers:
            raise KeyError(f"load_lora_adapter: {key} names no adapted layer of the model")
        p = getattr(layers[name], which).weight
        if tuple(p.shape) != tuple(value.shape):
            raise ValueError(f"load_lora_adapter: {key} is {tuple(value.shape)}, the layer expects {tuple(p.shape)}")
        with torch.no_grad():
            p.copy_(value)
        seen.add((name, which))
    missing = [f"{n}.{w}" for n in layers for w in ("lora_A", "lora_B") if (n, w) not in seen]
    if missing:
        raise KeyError(f"load_lora_adapter: the state dict lacks {missing[:4]}{' ...' if len(missing) > 4 else ''}")
    refresh_lora(model)
    return layers


def mark_only_lora_trainable(model: nn.Module) -> None:
    """requires_grad only on the lora_A / lora_B weights (peft's mark_only_lora_as_trainable)."""
    for n, p in model.named_parameters():
        p.requires_grad_(".lora_A." in "." + n or ".lora_B." in "." + n)


def refresh_lora(model: nn.Module) -> None:
    """After an optimiser step: bring every adapter's kernel copies up to date, in place -- a captured decode graph then replays with the new weights."""
    for m in lora_layers(model).values():
        if m._copies is not None:
            m.refresh_adapter()


__all__ = ["LoraQuantLinear", "parse_adapter_key", "lora_forward_multi", "inject_lora", "lora_state_dict", "load_lora_adapter", "mark_only_lora_trainable", "refresh_lora",
           "lora_layers", "set_lora_fused_backward"]
