"""Host-side pieces of bench.py: what the driver's multi-GPU run depends on, and the writer behind --dump-outputs (no GPU needed)."""
import importlib.util
import os
import threading
import time

import pytest


def _bench():
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_tp_deadline_runs_the_fallback_exactly_once_or_never():
    """The tensor-parallel block of `bench.py --gpus N` runs under _deadline(): either the block finishes first (finish() is True and the
    fallback never runs) or the fallback runs once -- it prints the headline without `tp` and ends the process -- and finish() is False."""
    B = _bench()
    fired = []
    finish = B._deadline(0.3, lambda: fired.append(1))
    assert finish() is True
    time.sleep(0.5)
    assert fired == [] and finish() is False            # a second finish() cannot win again

    fired2, gate = [], threading.Event()
    finish2 = B._deadline(0.05, lambda: (fired2.append(1), gate.set()))
    assert gate.wait(2.0)
    assert fired2 == [1] and finish2() is False
    time.sleep(0.2)
    assert fired2 == [1]


def test_algorithmic_bytes_formula():
    """packed weights + zero-points + scales (+ g_idx for act-order) + x + y per launch."""
    B = _bench()
    K, N, M = 4096, 11008, 1
    assert B.algorithmic_bytes(K, N, M) == K * N // 2 + (K // 128) * (N // 8) * 4 + (K // 128) * N * 2 + M * K * 2 + M * N * 2
    assert B.algorithmic_bytes(K, N, M, act_order=True) - B.algorithmic_bytes(K, N, M) == K * 4


def test_dump_outputs_writes_float32_and_samples_the_same_rows(tmp_path):
    """--dump-outputs: one float32 .npy per output; above the byte budget every array keeps the same seeded, sorted sample of rows, and a
    second dump of the same outputs is identical."""
    import numpy as np
    import torch
    B = _bench()
    g = torch.Generator().manual_seed(3)
    ts = [torch.randn(300, n, generator=g).half() for n in (64, 96, 32)]
    names = ["b00_q_proj", "b00_k_proj", "b00_down_proj"]
    B.dump_outputs(str(tmp_path / "all"), names, ts)
    for n, t in zip(names, ts):
        a = np.load(tmp_path / "all" / (n + ".npy"))
        assert a.dtype == np.float32 and np.array_equal(a, t.float().numpy())
    budget = 4 * 50 * (64 + 96 + 32)                                      # room for 50 of the 300 rows
    for run in ("s1", "s2"):
        B.dump_outputs(str(tmp_path / run), names, ts, budget=budget)
    a0 = np.load(tmp_path / "s1" / "b00_q_proj.npy")
    assert a0.shape == (50, 64) and sum(np.load(tmp_path / "s1" / (n + ".npy")).nbytes for n in names) <= budget
    rows = [int(np.nonzero((ts[0].float().numpy() == r).all(1))[0][0]) for r in a0]
    assert rows == sorted(rows) and len(set(rows)) == 50
    for n, t in zip(names, ts):
        a = np.load(tmp_path / "s1" / (n + ".npy"))
        assert np.array_equal(a, t.float().numpy()[rows]) and np.array_equal(a, np.load(tmp_path / "s2" / (n + ".npy")))


def test_stack_output_names_follow_the_flattened_outputs():
    B = _bench()
    names = B.stack_output_names(2)
    assert len(names) == 14 and names[:3] == ["b00_q_proj", "b00_k_proj", "b00_v_proj"] and names[-1] == "b01_down_proj"
    assert B.flatten_outputs([[1, 2, 3], 4, [5, 6], 7]) == [1, 2, 3, 4, 5, 6, 7]      # q|k|v, o, gate|up, down: grouped launches return lists
