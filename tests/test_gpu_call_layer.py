"""GPU: the layout of an input changes nothing.  Every Python entry point prepares its input in one place (_lib._rows16 / _dense16): the result computed from
contiguous, 16-byte aligned rows in the layer dtype must come back bit for bit when the same values arrive as a 3-D tensor, as a strided view, as a
contiguous view at an odd element offset, or in fp32.  (The canonical result itself is pinned to the oracle by the parity tests.)  Also: a released layer
equals its unreleased twin through the one rows rebuild, post_init creates no attribute that _reset_derived does not declare, and grad_input without the
opt-in flag still calls the plain entry point."""
import pytest
import torch

from autogptq_amd import _lib
from autogptq_amd.moe import moe_forward
from autogptq_amd.qlinear_mi355x import QuantLinear, forward_multi, mlp_forward
from oracle import gptq_oracle as O
from test_gpu_lora import _adapter
from test_gpu_moe import _routing, make_experts

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
K = N = 128
ROWS = (0, 1, 4, 8, 64)      # the fast-path band, the first slow-path call that fills the mask, a rows-band call


def _ql(seed, act=False, epilogue="none", **post_init):
    L = O.random_quant_layer(K, N, 4, 32, dtype=torch.float16, seed=seed, act_order=act)
    q = QuantLinear(4, 32, K, N, False, weight_dtype=torch.float16, epilogue=epilogue)
    q.qweight, q.qzeros, q.scales, q.g_idx = L["qweight"].clone(), L["qzeros"].clone(), L["scales"].clone(), L["g_idx"].clone().to(torch.int32)
    return q.to(DEV).post_init(**post_init)


def _values(M, seed, width=K):
    g = torch.Generator().manual_seed(1000 * seed + M)
    return (torch.rand(M, width, generator=g) - 0.5).half().to(DEV)


def _layouts(x):
    """The same values four other ways: ([.., M', K], strided view, odd element offset, fp32)."""
    M, W = x.shape
    wide = torch.zeros(M, 2 * W, dtype=x.dtype, device=x.device)
    wide[:, ::2] = x
    buf = torch.empty(M * W + 1, dtype=x.dtype, device=x.device)
    buf[1:].copy_(x.reshape(-1))
    odd = buf[1:].view(M, W)
    assert M == 0 or (not wide[:, ::2].is_contiguous() and odd.is_contiguous() and odd.data_ptr() % 16 == 2)
    return {"3d": x.reshape((2, M // 2, W) if M % 2 == 0 else (1, M, W)), "strided": wide[:, ::2], "odd_offset": odd, "fp32": x.float()}


def _same_for_every_layout(fn, seed, width=K, rows=ROWS):
    """fn(x) -> tensor or list of tensors; x [M, width]."""
    with torch.no_grad():
        for M in rows:
            x = _values(M, seed, width)
            want = fn(x)
            want = list(want) if isinstance(want, (list, tuple)) else [want]
            for name, alt in _layouts(x).items():
                got = fn(alt)
                got = list(got) if isinstance(got, (list, tuple)) else [got]
                assert len(got) == len(want)
                for g, w in zip(got, want):      # (an fp32 call's result comes back in fp32 where the entry point casts back: exact either way)
                    assert g.dtype in (w.dtype, alt.dtype) and torch.equal(g.to(w.dtype).reshape(w.shape), w), (name, M)


@pytest.fixture(scope="module")
def layers():
    return {"q": _ql(1), "k": _ql(2), "v": _ql(3), "act": _ql(4, act=True), "down": _ql(5), "gated": _ql(6, epilogue="silu_mul")}


@pytest.mark.parametrize("which", ["q", "act"])
def test_forward(layers, which):
    _same_for_every_layout(layers[which], seed=1)


def test_forward_multi(layers):
    grp = [layers["q"], layers["k"], layers["v"]]
    _same_for_every_layout(lambda x: forward_multi(grp, x), seed=2)


def test_mlp_forward(layers):
    _same_for_every_layout(lambda x: mlp_forward(layers["q"], layers["k"], layers["down"], x), seed=3)


@pytest.mark.parametrize("which", ["q", "act"])
@pytest.mark.parametrize("accumulate", [False, True], ids=["new", "into_dx"])
def test_grad_input(layers, which, accumulate):
    q = layers[which]

    def fn(dy):
        M = dy.numel() // N
        dx0 = (torch.arange(M * K, device=DEV, dtype=torch.float32).reshape(M, K) % 7 / 8).half() if accumulate else None
        return q.grad_input(dy, dx0)

    _same_for_every_layout(fn, seed=4, width=N)


def test_plain_product_of_a_gated_layer(layers):
    _same_for_every_layout(layers["gated"]._plain_product, seed=5)


def test_a_2d_tensor_of_another_width_never_reaches_a_kernel(layers):
    """grad_input, quantize_activations and _plain_product have no width check of their own: a [3, 64] tensor (192 elements, no whole row of 128) raises in
    the reshape, and a [4, 64] one is read as [2, 128], as reshape(-1, N) always read it."""
    q, gated = layers["q"], layers["gated"]
    with torch.no_grad():
        for fn in (q.grad_input, q.quantize_activations, gated._plain_product):
            with pytest.raises(RuntimeError):
                fn(_values(3, 15, 64))
        dy = _values(4, 16, 64)
        assert torch.equal(q.grad_input(dy), q.grad_input(dy.reshape(2, N)))
        xq, sx = q.quantize_activations(dy)
        assert tuple(xq.shape) == (2, K) and tuple(sx.shape) == (2,)


def test_moe_forward():
    experts = make_experts(2, K, K, 4, 32, False, torch.float16, seed=6, top_k=2)

    def fn(x):
        T = x.numel() // K
        idx, w = _routing(T, 2, 2, seed=T)
        return moe_forward(experts, x, idx, w)

    _same_for_every_layout(fn, seed=6)


def test_lora_forward():
    lq = _adapter(_ql(7), 16, 32.0, seed=7)
    _same_for_every_layout(lq, seed=7)


def test_released_layer_equals_the_unreleased_one(layers):
    plain, rel = layers["q"], _ql(1, release_checkpoint_layout=True)
    assert rel._released and rel.qweight.device.type == "cpu" and not plain._released
    with torch.no_grad():
        for M in (5, 8, 16, 32):
            x, dy = _values(M, 8), _values(M, 9, N)
            assert torch.equal(rel(x), plain(x)), M
            assert torch.equal(rel.grad_input(dy), plain.grad_input(dy)), M
    assert any(rel._rows_need[M] for M in (5, 8, 16, 32)), rel._rows_need      # the rebuild really ran


def test_released_layer_backward_on_the_copy():
    plain, rel = _ql(1, grad_on_copy=True), _ql(1, release_checkpoint_layout=True, grad_on_copy=True)
    assert rel.describe_grad_plan(8).startswith("kernel=grad_copy") and plain.describe_grad_plan(8).startswith("kernel=grad_copy")
    dy = _values(8, 10, N)
    with torch.no_grad():
        assert torch.equal(rel.grad_input(dy), plain.grad_input(dy))


def test_post_init_creates_no_undeclared_attribute(layers):
    fresh = set(vars(QuantLinear(4, 32, K, N, False)))
    extra = [_ql(1, release_checkpoint_layout=True), _ql(1, grad_on_copy=True), _ql(1, act_int8=True)]
    with torch.no_grad():
        for q in list(layers.values()) + extra:
            q(_values(8, 11))
            q.grad_input(_values(8, 12, N))
            assert set(vars(q)) - fresh == set(), set(vars(q)) - fresh
        layers["gated"]._plain_product(_values(8, 13))
        assert set(vars(layers["gated"])) - fresh == set()


def test_grad_input_without_the_flag_calls_the_plain_entry_point(layers, monkeypatch):
    q = layers["q"]
    assert not QuantLinear.GRAD_ON_COPY and q._grad_flags == 0
    lib, asked = _lib.load(), []

    class Proxy:
        def __getattr__(self, name):
            asked.append(name)
            return getattr(lib, name)

    dy = _values(8, 14, N)
    monkeypatch.setattr(_lib, "load", lambda: Proxy())
    with torch.no_grad():
        dx = q.grad_input(dy)
    monkeypatch.undo()
    assert "gptq_grad_input" in asked and "gptq_grad_input_ex" not in asked, asked
    with torch.no_grad():
        assert torch.equal(dx, q.grad_input(dy))
