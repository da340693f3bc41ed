"""The SiLU outputs of the five dense sites that take the gate's activation as an argument (the pair form of the decode-copy kernel, the fused GEMV epilogue
of the checkpoint-row family, silu_mul_kernel, silu_mul2_kernel, silu_mul2_permute_rows4_kernel), on seeded layers and inputs.
tests/golden/silu_mul_bits.npz holds what the commit BEFORE the activation became an argument returned for them (written by ``python tests/_silu_bits.py OUT``
on that commit, on an MI355X); test_gpu_gated_act.py requires the same bits.  Uses only what that commit already had."""
import sys

import numpy as np
import torch

from oracle import gptq_oracle as O

DEV = "cuda:0"


def _module(L, bits, gs, dtype):
    from autogptq_amd.qlinear_mi355x import QuantLinear
    m = QuantLinear(bits, gs, L["qweight"].shape[0] * 32 // bits, L["qweight"].shape[1], True, weight_dtype=dtype)
    m.qweight, m.qzeros, m.scales, m.g_idx, m.bias = L["qweight"].clone(), L["qzeros"].clone(), L["scales"].clone(), L["g_idx"].clone(), L["bias"].clone()
    return m


def _layers(K, N, bits, gs, dtype, seed, n, mult, act=False):
    Ls = [O.random_quant_layer(K, N, bits, gs, dtype=dtype, seed=seed + i, bias=True, act_order=act) for i in range(n)]
    for L in Ls:
        L["g_idx"] = Ls[0]["g_idx"].clone()
        L["scales"] = (L["scales"].float() * mult).to(dtype)
    return Ls


def _x(M, K, dtype, seed):
    return (torch.rand(M, K, generator=torch.Generator().manual_seed(seed)) - 0.5).to(dtype).to(DEV)


def cases():
    """(name, output tensor) of every case, computed by the library that is loaded."""
    from autogptq_amd.fused import fuse_gate_up
    from autogptq_amd.qlinear_mi355x import QuantLinear, mlp_forward
    out = []
    saved = QuantLinear.TILED_DECODE
    try:
        for tiled, shapes in ((True, [(160, 32, 32, 4, torch.float16, (1, 4, 8, 130)), (160, 32, 32, 4, torch.bfloat16, (1, 4, 8, 130)),
                                      (2112, 96, 64, 4, torch.float16, (1, 2, 3, 4, 8)), (1024, 1408, 32, 3, torch.float16, (1, 4)),
                                      (1024, 1408, 32, 8, torch.bfloat16, (1, 4))]),
                              (False, [(1024, 704, 128, 4, torch.float16, (1, 2, 7, 16, 130))])):
            QuantLinear.TILED_DECODE = tiled
            for K, I, gs, bits, dtype, rows in shapes:
                Lg, Lu = _layers(K, I, bits, gs, dtype, K + I, 2, 4 / (16 if bits == 8 else 1))
                q = fuse_gate_up(_module(Lg, bits, gs, dtype), _module(Lu, bits, gs, dtype)).to(DEV)
                q.post_init()
                for M in rows:
                    with torch.no_grad():
                        out.append((f"layer_{'copy' if tiled else 'rows'}_{K}x{I}_b{bits}_{str(dtype)[6:]}_M{M}", q(_x(M, K, dtype, M))))
    finally:
        QuantLinear.TILED_DECODE = saved
    for H, I, gs, down_act, rows in ((256, 704, 64, False, (1, 4, 40)), (256, 704, 64, True, (4, 40)), (1024, 2048, 128, True, (5, 64))):
        Lg, Lu = _layers(H, I, 4, gs, torch.float16, H + I, 2, 4)
        Ld, = _layers(I, H, 4, gs, torch.float16, H + I + 2, 1, 1, act=down_act)
        mods = [_module(L, 4, gs, torch.float16).to(DEV) for L in (Lg, Lu, Ld)]
        for m in mods:
            m.post_init()
        for M in rows:
            with torch.no_grad():
                out.append((f"mlp_{H}x{I}_{'act' if down_act else 'seq'}_M{M}", mlp_forward(*mods, _x(M, H, torch.float16, 50 + M))))
    torch.cuda.synchronize()
    return out


def to_numpy(t):
    return t.detach().cpu().contiguous().view(torch.int16).numpy()      # the bits, whatever the dtype


if __name__ == "__main__":
    np.savez_compressed(sys.argv[1], **{name: to_numpy(t) for name, t in cases()})
    print("wrote", sys.argv[1])
