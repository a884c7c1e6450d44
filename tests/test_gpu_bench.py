"""bench.py and __graft_entry__.smoke() run end to end on a reduced problem: the JSON line carries the contract's
fields (metric / value / unit / n_gpus / steps / warmup / ms_per_step / scaling / dtype / data / config.workload) and
the roofline object, and nothing in the solver's interfaces has drifted away from what the benchmark wraps."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_small_run_emits_contract_line():
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--rows", "30000", "--steps", "3", "--warmup", "1",
                          "--full", "--no-cpu-baseline"], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert res.returncode == 0, res.stderr[-2000:]
    line = [l for l in res.stdout.strip().splitlines() if l.startswith("{")][-1]
    d = json.loads(line)
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert key in d, key
    assert d["n_gpus"] == 1 and d["steps"] == 3 and d["warmup"] == 1 and d["value"] > 0
    assert "workload" in d["config"] and d["data"] == "synthetic"
    rf = d["roofline"]
    assert rf["bound"] in ("hbm", "mfma") and rf["achieved"] > 0 and abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-9
    assert abs(d["value"] - 30000 * 8192 * 3 / (d["ms_per_step"] * 3e-3)) <= 1e-6 * d["value"]


def test_bench_plain_run_times_the_steps_and_dumps_the_solve(tmp_path):
    """A plain run (no --full) prints the headline fields only; --dump-outputs writes the timed solve's last iterate and
    its residuals, the same arrays from run to run."""
    dumps = []
    for k in range(2):
        out_dir = tmp_path / str(k)
        res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--rows", "30000", "--steps", "4", "--warmup", "1",
                              "--dump-outputs", str(out_dir)], capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert res.returncode == 0, res.stderr[-2000:]
        d = json.loads([l for l in res.stdout.strip().splitlines() if l.startswith("{")][-1])
        for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "final_loss"):
            assert key in d, key
        assert "roofline" not in d and "configs" not in d and "cpu_baseline" not in d
        assert d["steps"] == 4 and abs(d["value"] - 30000 * 8192 * 4 / (d["ms_per_step"] * 4e-3)) <= 1e-6 * d["value"]
        w, losses = np.load(out_dir / "weights.npy"), np.load(out_dir / "losses.npy")
        assert w.dtype == np.float64 and w.shape == (8192,) and np.isfinite(w).all()
        assert losses.dtype == np.float64 and losses.shape == (4,) and losses[-1] == d["final_loss"]
        dumps.append((w, losses))
    assert np.allclose(dumps[0][0], dumps[1][0], rtol=1e-9, atol=1e-12 * np.abs(dumps[0][0]).max())
    assert np.allclose(dumps[0][1], dumps[1][1], rtol=1e-9)


def test_graft_entry_smoke():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as g
    g.smoke()
