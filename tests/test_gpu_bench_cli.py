"""A plain `bench.py` run on a small shard, twice: the result line, --steps, and --dump-outputs giving the same outputs from the same arguments."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(dump):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--scenarios", "4", "--dump-outputs", dump]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_bench_run_and_its_outputs(tmp_path):
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    res = _run(a)
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in res, k
    assert res["unit"] == "agent-solves/s" and res["higher_is_better"] is True and res["dtype"] == "f64"
    assert res["steps"] == 3 and len(res["config"]["status_per_step"]) == 3
    assert res["ms_per_step"] > 0 and res["value"] > 0
    assert "roofline" not in res and "cpu_baseline" not in res       # the other legs run with --full only
    n = res["config"]["instances_per_gpu"]
    assert n == 4 * 64
    _run(b)
    files = sorted(os.listdir(a))
    assert files == sorted(os.listdir(b)) and "obj.npy" in files and "v.npy" in files
    for f in files:
        x, y = np.load(os.path.join(a, f)), np.load(os.path.join(b, f))
        assert x.dtype == np.float64 and np.array_equal(x, y, equal_nan=True), f
    obj, status = np.load(os.path.join(a, "obj.npy")), np.load(os.path.join(a, "status.npy"))
    assert obj.shape == (n,) and np.isfinite(obj[status == 0]).all()
    assert int((status == 0).sum()) == res["config"]["status_per_step"][-1]["optimal"]
