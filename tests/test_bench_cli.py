"""bench.py without a GPU: the options of a plain run and the files --dump-outputs writes."""
import os

import numpy as np
import pytest

import bench


def test_plain_run_is_the_default_and_steps_are_checked():
    args = bench.parse(["--gpus", "1", "--steps", "3", "--warmup", "2"])
    assert (args.steps, args.warmup, args.full, args.dump_outputs) == (3, 2, False, None)
    args = bench.parse(["--steps", "1", "--warmup", "0", "--full", "--dump-outputs", "out"])
    assert args.full and args.dump_outputs == "out"
    for bad in (["--steps", "0"], ["--warmup", "-1"]):
        with pytest.raises(SystemExit):
            bench.parse(bad)


class _StubModel(object):
    nv = 23


class _StubProblem(object):
    """download() of the bench shard's shape (32768 instances, n = 575)"""
    model = _StubModel()

    def __init__(self, b=32768, n=575):
        rng = np.random.Generator(np.random.PCG64(5))
        self.out = dict(v=rng.standard_normal((b, n)), obj=rng.standard_normal(b), lower_bound=rng.standard_normal(b),
                        status=rng.integers(0, 3, b).astype(np.int32), nodes=rng.integers(0, 800, b).astype(np.int32),
                        pivots=rng.integers(0, 40000, b).astype(np.int32))

    def download(self):
        return self.out


def test_dump_outputs_float64_under_64mb_and_seeded(tmp_path):
    p = _StubProblem()
    names = bench.dump_outputs(str(tmp_path / "a"), p)
    bench.dump_outputs(str(tmp_path / "b"), p)
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == sorted(k + ".npy" for k in names)
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= 64 << 20
    z = {f[:-4]: np.load(tmp_path / "a" / f) for f in files}
    assert all(a.dtype == np.float64 for a in z.values())
    for f in files:
        assert np.array_equal(z[f[:-4]], np.load(tmp_path / "b" / f))
    out = p.out
    idx, vidx = z["index"].astype(np.int64), z["v_index"].astype(np.int64)
    assert np.array_equal(idx, np.arange(32768))            # every instance of the shard fits
    assert len(vidx) == bench.DUMP_V_ROWS and np.all(np.diff(vidx) > 0)
    assert np.array_equal(z["v"], out["v"][vidx]) and np.array_equal(z["u0"], out["v"][:, :23])
    for k in ("obj", "lower_bound", "status", "nodes", "pivots"):
        assert np.array_equal(z[k], out[k].astype(np.float64)), k


def test_dump_outputs_samples_instances_of_a_large_shard(tmp_path):
    p = _StubProblem(b=262144, n=32)
    bench.dump_outputs(str(tmp_path), p)
    assert sum(os.path.getsize(tmp_path / f) for f in os.listdir(tmp_path)) <= 64 << 20
    idx = np.load(tmp_path / "index.npy").astype(np.int64)
    assert 0 < len(idx) < 262144 and np.all(np.diff(idx) > 0)
    assert np.array_equal(np.load(tmp_path / "obj.npy"), p.out["obj"][idx])
