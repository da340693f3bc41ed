"""Host-built gptq_moe_t / gptq_moe_shared_t structs with dummy pointers, for the tests of the routed-expert entry layer that run without a GPU: the
host-only queries (describe, workspace bytes) never dereference them, and a forward call the checker declines returns before it touches one."""
import ctypes

from autogptq_amd import _lib

PTR = 0x1000          # any non-NULL, 16-byte aligned address


def layer(K, N, bits=4, gs=128, dtype=_lib.GPTQ_F16, copy=True, act=False, **fields):
    """One gptq_layer_t [K -> N]; gs <= 0: one group.  ``fields`` overwrite struct members last (``bias=PTR``, ``qweight_tiled=0x5008``, ...)."""
    L = _lib.GptqLayer()
    L.qweight = L.qzeros = L.scales = PTR
    L.K, L.N, L.bits, L.group_size, L.dtype, L.zero_mode = K, N, bits, min(gs, K) if gs > 0 else K, dtype, 0
    if copy:
        L.qweight_tiled, L.qconst_tiled, L.tiled_cols = 0x5000, 0x6000, 16
    if act:
        L.g_idx, L.qweight_seq, L.perm = 0x2000, 0x3000, 0x4000
    for k, v in fields.items():
        setattr(L, k, v)
    return L


def moe(E=8, H=256, I=512, flags=0, gate=None, up=None, down=None, **kw):
    """gptq_moe_t of E experts [H -> I], [H -> I], [I -> H]; ``kw`` goes to every layer, ``gate`` / ``up`` / ``down`` (dicts) to that projection's on top."""
    layers = [[layer(k, n, **dict(kw, **(extra or {}))) for _ in range(E)] for k, n, extra in ((H, I, gate), (H, I, up), (I, H, down))]
    arrs = [(ctypes.POINTER(_lib.GptqLayer) * max(1, E))(*[ctypes.pointer(l) for l in ls]) for ls in layers]
    m = _lib.GptqMoe()
    m.E, m.flags = E, flags
    m.gate, m.up, m.down = (ctypes.addressof(a) for a in arrs)
    m._keep = (layers, arrs)
    return m


def expert(m, proj, e):
    """The layer struct of expert ``e`` in projection ``proj`` (0 gate, 1 up, 2 down) of a struct ``moe`` built: edit it in place."""
    return m._keep[0][proj][e]


def drop_copy(L):
    L.qweight_tiled = L.qconst_tiled = None
    L.tiled_cols = 0


def shared(H=256, Is=1024, gate=None, up=None, down=None, **kw):
    """gptq_moe_shared_t with layers [H -> Is], [H -> Is], [Is -> H]; keywords as ``moe`` takes them."""
    layers = [layer(k, n, **dict(kw, **(extra or {}))) for k, n, extra in ((H, Is, gate), (H, Is, up), (Is, H, down))]
    sh = _lib.GptqMoeShared()
    sh.gate, sh.up, sh.down = (ctypes.addressof(l) for l in layers)
    sh._keep = layers
    return sh
