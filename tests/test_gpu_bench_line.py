"""GPU (-m gpu): the plain bench.py line and --dump-outputs, on a one-block stack.  A plain run prints one JSON line with the headline fields and
none of the --full blocks, times exactly --steps steps, and writes the last timed step's outputs: one float32 array per layer of the stack, the
same in two runs of the same command (seeded weights and inputs), and equal to the same layers called one by one on the same inputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(out_dir, *extra):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--blocks", "1", "--steps", "3", "--warmup", "1", "--dump-outputs", str(out_dir), *extra]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert r.returncode == 0 and len(lines) == 1, (r.returncode, r.stdout[-2000:], r.stderr[-3000:])
    return json.loads(lines[0])


def test_plain_line_and_dumped_outputs(tmp_path):
    d = _run(tmp_path / "a")
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in d, k
    assert d["unit"] == "GB/s" and d["higher_is_better"] is True and d["dtype"] == "f16" and d["value"] > 0 and d["ms_per_step"] > 0
    assert d["steps"] == 3 and d["warmup"] == 1 and d["config"]["layers"] == 7 and d["config"]["launches"] == 4
    for k in ("roofline", "verify", "eager", "fused_callers", "prefill", "config5", "batched_decode", "warm_l3", "cpu_baseline"):
        assert k not in d, k                                                  # --full only
    names = sorted(f[:-4] for f in os.listdir(tmp_path / "a"))
    assert names == sorted(f"b00_{n}" for n in ("q_proj", "k_proj", "v_proj", "o_proj", "gate_proj", "up_proj", "down_proj"))
    a = {n: np.load(tmp_path / "a" / (n + ".npy")) for n in names}
    assert all(v.dtype == np.float32 and v.shape[0] == 1 and np.isfinite(v).all() and np.abs(v).max() > 0 for v in a.values())
    assert a["b00_gate_proj"].shape == (1, 11008) and a["b00_down_proj"].shape == (1, 4096)

    _run(tmp_path / "b")                                                      # same command, same inputs: the same outputs
    for n in names:
        assert np.array_equal(a[n], np.load(tmp_path / "b" / (n + ".npy"))), n

    # the dumped arrays are what the stack's layers return: rebuild them from the same seeds and call them one by one (no graph, no grouping)
    import torch
    sys.path.insert(0, ROOT)
    import bench
    dev = torch.device("cuda", 0)
    layers, xs = bench.build_stack(dev, 1, 1, False)
    with torch.no_grad():
        for (name, K, N, q), n in zip(layers, bench.stack_output_names(1)):
            y = q(xs[K]).float().cpu().numpy()
            scale = float(np.abs(y).max())
            assert np.abs(y - a[n]).max() <= 2e-3 * scale, (n, float(np.abs(y - a[n]).max()), scale)
