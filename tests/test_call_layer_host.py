"""CPU: the Python call layer's shared helpers -- input preparation (_lib._dense16 / _is_dense16 / _rows16), the per-row-count cache (_cached_need) and the
one declaration of QuantLinear's derived state (_reset_derived).  No GPU and no library load: data_ptr() and strides behave the same on CPU tensors."""
import pytest
import torch
import torch.nn as nn

from autogptq_amd import _lib
from autogptq_amd.qlinear_mi355x import QuantLinear, _cached_need

K = 64


def _base(rows=4):
    t = torch.arange(rows * K, dtype=torch.float32).reshape(rows, K) / 8      # exact in fp16
    assert t.data_ptr() % 16 == 0
    return t


def _odd_offset(v: torch.Tensor) -> torch.Tensor:
    """v's values as a contiguous view one element into a fresh buffer: the data pointer is 2 (fp16) or 4 (fp32) mod 16."""
    buf = torch.empty(v.numel() + 1, dtype=v.dtype)
    buf[1:].copy_(v.reshape(-1))
    t = buf[1:].view(v.shape)
    assert t.is_contiguous() and t.data_ptr() % 16 == v.element_size()
    return t


def _cases():
    """(name, tensor, dtype argument, the expected values in the target dtype)."""
    want = _base().half()
    wide = torch.zeros(4, 2 * K, dtype=torch.float16)
    wide[:, ::2] = want
    wide32 = torch.empty(4 * 2 * K + 1, dtype=torch.float32)[1:].view(4, 2 * K)
    wide32[:, ::2] = _base()
    return [
        ("strided", wide[:, ::2], None, want),
        ("odd_offset", _odd_offset(want), None, want),
        ("other_dtype", _base(), torch.float16, want),
        ("all_three", wide32[:, ::2], torch.float16, want),
    ]


def test_dense16_returns_the_tensor_itself_when_nothing_is_needed():
    t = _base().half()
    assert _lib._is_dense16(t)
    assert _lib._dense16(t) is t
    assert _lib._dense16(t, torch.float16) is t


@pytest.mark.parametrize("case", _cases(), ids=lambda c: c[0])
def test_dense16_makes_one_dense_aligned_tensor(case):
    _, t, dtype, want = case
    assert not _lib._is_dense16(t) or (dtype is not None and t.dtype != dtype)
    got = _lib._dense16(t, dtype)
    assert got is not t and got.data_ptr() != t.data_ptr()
    assert got.dtype == want.dtype and got.is_contiguous() and got.data_ptr() % 16 == 0 and _lib._is_dense16(got)
    assert torch.equal(got, want)
    assert _lib._dense16(got, dtype) is got      # prepared once, it stays


def test_is_dense16_tells_the_layouts_apart():
    names = {c[0]: c[1] for c in _cases()}
    assert not _lib._is_dense16(names["strided"])                  # not contiguous
    assert names["odd_offset"].is_contiguous() and not _lib._is_dense16(names["odd_offset"])      # contiguous, pointer 2 mod 16
    assert _lib._is_dense16(names["other_dtype"])                  # the predicate does not look at the dtype
    assert not _lib._is_dense16(names["all_three"])


def test_rows16_shapes():
    x = torch.arange(2 * 3 * K, dtype=torch.float16).reshape(2, 3, K)
    x2, M = _lib._rows16(x, K, torch.float16)
    assert tuple(x2.shape) == (6, K) and M == 6 and torch.equal(x2, x.reshape(6, K)) and x2.data_ptr() == x.data_ptr()
    x2, M = _lib._rows16(x[0, 0], K, torch.float16)
    assert tuple(x2.shape) == (1, K) and M == 1
    x2, M = _lib._rows16(torch.empty(0, K, dtype=torch.float16), K, torch.float16)
    assert tuple(x2.shape) == (0, K) and M == 0
    x2, M = _lib._rows16(_odd_offset(x.float()), K, torch.float16)      # cast, then rows: dense and aligned
    assert M == 6 and x2.dtype == torch.float16 and _lib._is_dense16(x2) and torch.equal(x2, x.reshape(6, K))
    same = x.reshape(6, K)
    assert _lib._rows16(same, K, torch.float16)[0] is same


def test_rows16_never_returns_another_width():
    """The callers hand (x2, M) to kernels that read M * K elements: a 2-D tensor of another width is re-viewed as [numel / K, K], as reshape(-1, K) always
    did, or raises -- it never passes through with its own width."""
    half = torch.arange(4 * (K // 2), dtype=torch.float16).reshape(4, K // 2)
    x2, M = _lib._rows16(half, K, torch.float16)
    assert tuple(x2.shape) == (2, K) and M == 2 and torch.equal(x2.reshape(-1), half.reshape(-1))
    x2, M = _lib._rows16(half.float(), K, torch.float16)
    assert tuple(x2.shape) == (2, K) and M == 2 and x2.dtype == torch.float16
    with pytest.raises(RuntimeError):
        _lib._rows16(torch.zeros(3, K // 2, dtype=torch.float16), K, torch.float16)      # 3 * K / 2 elements: no whole row
    with pytest.raises(RuntimeError):
        _lib._rows16(torch.zeros(1, K + 32, dtype=torch.float16), K, torch.float16)       # wider than a row, and no two rows


def test_cached_need_asks_once_per_row_count_without_a_tuning():
    calls, cache = [], {}

    def query(v):
        return lambda: (calls.append(v), v)[1]

    assert _cached_need(cache, 3, None, query(0)) == 0            # a need of 0 is an answer, not a miss
    assert _cached_need(cache, 3, None, query(99)) == 0
    assert _cached_need(cache, 5, None, query(512)) == 512
    assert _cached_need(cache, 5, None, query(99)) == 512
    assert calls == [0, 512] and cache == {3: 0, 5: 512}


def test_cached_need_with_a_tuning_asks_every_time_and_leaves_the_cache_alone():
    calls, cache, tuning = [], {5: 512}, object()

    def query():
        calls.append(1)
        return 7

    assert _cached_need(cache, 5, tuning, query) == 7              # does not read the cached 512
    assert _cached_need(cache, 5, tuning, query) == 7
    assert _cached_need(cache, 9, tuning, query) == 7
    assert len(calls) == 3 and cache == {5: 512}                   # ... and writes nothing


# What __init__ takes from its arguments (and act_order, which post_init resolves from g_idx and which has always survived _invalidate): everything else in a
# fresh instance's __dict__ is derived state.
_CONFIG = {"infeatures", "outfeatures", "bits", "group_size", "maxq", "trainable", "use_cuda_fp16", "kernel_switch_threshold", "zero_mode", "epilogue", "bias",
           "act_order"}
_KEPT = {"_released", "_a8_hold"}


def _derived_names(q):
    return set(vars(q)) - set(vars(nn.Module())) - _CONFIG


def test_invalidate_resets_every_piece_of_derived_state():
    fresh = QuantLinear(4, 32, 128, 128, False)
    q = QuantLinear(4, 32, 128, 128, False)
    names = _derived_names(fresh)
    assert _KEPT <= names and {"_layer", "_parts", "_ws_need", "_ws0_mask", "_rows_need", "_layer_plain", "_grad_plans"} <= names
    sentinel = object()
    for name in names:
        setattr(q, name, sentinel)
    q._invalidate()
    for name in sorted(names):
        if name in _KEPT:
            assert getattr(q, name) is sentinel, name
        else:
            assert getattr(q, name) is not sentinel and getattr(q, name) == getattr(fresh, name), name
    assert _derived_names(q) == names
    # the containers are the instance's own
    assert q._ws_need is not fresh._ws_need and q._rows_need is not fresh._rows_need
