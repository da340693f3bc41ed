"""Shared by the CPU and GPU tests of the mixture-of-experts backward (a plain helper module like _tiny_mixtral.py): the fp64 oracle of the formulas in
include/gptq_mi355x.h (gptq_moe_backward), on dense weights.

    d_r = dOut[t] W2_e^T,  dw[t, j] = <d_r, h_r>,  dg_r = w d_r u_r silu'(g_r),  du_r = w d_r silu(g_r),  dX[t] = sum_j (dg_r W1_e^T + du_r W3_e^T)

``oracle(x, idx, w, dout, W1, W3, W2)``: x [T, H], idx [T, topk] int64 (values outside [0, E) are dropped), w [T, topk], dout [T, H]; W1 / W3: E matrices
[H, I], W2: E matrices [I, H] (anything ``.double()`` takes).  Returns a namespace of fp64 tensors: ``dX`` [T, H], ``dw`` [T, topk] and, per assignment
[T, topk, I] (zero where dropped), ``g, u, h, d, dg, du`` plus the products of absolute values the error model needs: ``Ag = |x| |W1|``,
``Au = |x| |W3|``, ``Ad = |dOut| |W2^T|``; ``valid`` [T, topk] bool."""
import types

import torch


def oracle(x, idx, w, dout, W1, W3, W2):
    x, w, dout = x.double(), w.double(), dout.double()
    T, topk = idx.shape
    E, I = len(W1), W1[0].shape[1]
    dev = x.device

    def z(*shape):
        return torch.zeros(shape, dtype=torch.float64, device=dev)

    o = types.SimpleNamespace(dX=z(T, x.shape[1]), dw=z(T, topk), valid=(idx >= 0) & (idx < E))
    for nm in ("g", "u", "h", "d", "dg", "du", "Ag", "Au", "Ad"):
        setattr(o, nm, z(T, topk, I))
    for e in range(E):
        tok, j = torch.where(idx == e)
        if tok.numel() == 0:
            continue
        w1, w3, w2 = W1[e].double(), W3[e].double(), W2[e].double()
        xe, de = x[tok], dout[tok]
        g, u = xe @ w1, xe @ w3
        s = torch.sigmoid(g)
        silu = g * s
        h = silu * u
        d = de @ w2.t()
        wj = w[tok, j][:, None]
        dg = wj * d * u * (s * (1 + g * (1 - s)))
        du = wj * d * silu
        o.dw[tok, j] = (d * h).sum(-1)
        o.dX.index_add_(0, tok, dg @ w1.t() + du @ w3.t())
        for nm, v in (("g", g), ("u", u), ("h", h), ("d", d), ("dg", dg), ("du", du), ("Ag", xe.abs() @ w1.abs()), ("Au", xe.abs() @ w3.abs()),
                      ("Ad", de.abs() @ w2.abs().t())):
            getattr(o, nm)[tok, j] = v
    return o
