"""MIP start from a baseline rollout (mld_warm_start_from_rollout, pyhybridcontrol_amd/simlog.py: start_from_rollout_np) at the boundary of the library and in
numpy, without a GPU: the byte rule against a plain loop, the keep rule, the NaN and ending rules, and header, binding and export agreeing on the entry."""
import ctypes as C
import os
import re

import numpy as np

from pyhybridcontrol_amd import _lib, simlog

with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mldgpu.h")) as _f:
    HDR = _f.read()
SOURCE_OF = {0: 1, 1: -1, 2: -2, -1: -3}


def _loop(v, end, bins, old=None):
    """the rule as the header states it, element by element"""
    B, nb = len(end), len(bins)
    nv = v.shape[2]
    start, source = np.zeros((B, nb), np.uint8), np.zeros(B, np.int32)
    for b in range(B):
        if old is not None and nb and old[b, 0] != 255:
            start[b], source[b] = old[b], 0
            continue
        source[b] = SOURCE_OF[int(end[b])]
        for k in range(nb):
            step, pos = divmod(int(bins[k]), nv)
            start[b, k] = (1 if v[b, step, pos] > 0.5 else 0) if end[b] == 0 else 255
    return start, source


def _case(seed, B=7, N=3, nv=5, cols=(1, 4)):
    rng = np.random.default_rng(seed)
    v = rng.uniform(size=(B, N, nv))
    v[:, :, list(cols)] = rng.integers(0, 2, (B, N, len(cols)))
    bins = np.array([s * nv + c for s in range(N) for c in cols])
    end = np.array([0, 1, 0, 2, -1, 0, 0][:B], np.int32)
    return v, end, bins


def test_against_a_plain_loop():
    for seed, kw in ((1, {}), (2, dict(B=1, N=1, nv=1, cols=(0,))), (3, dict(N=4, nv=3, cols=(0, 1, 2)))):
        v, end, bins = _case(seed, **kw)
        got, src = simlog.start_from_rollout_np(v, end, bins)
        want, wsrc = _loop(v, end, bins)
        assert got.dtype == np.uint8 and src.dtype == np.int32 and got.shape == (len(end), len(bins))
        assert np.array_equal(got, want) and np.array_equal(src, wsrc), seed
        # the rollout's own shapes: (B, S = 1, K, nv) and (B, 1)
        again, asrc = simlog.start_from_rollout_np(v[:, None], end[:, None], bins)
        assert np.array_equal(again, want) and np.array_equal(asrc, wsrc), seed
    v, end, bins = _case(1)
    got, src = simlog.start_from_rollout_np(v, end, bins)
    assert src.tolist() == [1, -1, 1, -2, -3, 1, 1]
    assert np.all(got[[1, 3, 4]] == 255) and np.all(got[[0, 2, 5, 6]] <= 1)
    # the last binary is the last double of a row of v
    assert bins[-1] == v.shape[1] * v.shape[2] - 1 and np.array_equal(got[0], v[0].reshape(-1)[bins].astype(np.uint8))


def test_the_keep_rule():
    v, end, bins = _case(4)
    B, nb = len(end), len(bins)
    old = np.full((B, nb), 255, np.uint8)
    old[0], old[1], old[4] = 1, 0, 1                 # a complete, an infeasible and an unattempted trajectory that have a start: kept all the same
    old[2, 1:] = 9                                   # first byte 255: no start, whatever follows
    got, src = simlog.start_from_rollout_np(v, end, bins, old=old)
    fresh, fsrc = simlog.start_from_rollout_np(v, end, bins)
    want, wsrc = _loop(v, end, bins, old)
    assert np.array_equal(got, want) and np.array_equal(src, wsrc)
    assert src.tolist() == [0, 0, 1, -2, 0, 1, 1]
    for b in (0, 1, 4):
        assert np.array_equal(got[b], old[b])
    for b in (2, 3, 5, 6):
        assert np.array_equal(got[b], fresh[b]) and src[b] == fsrc[b]
    assert np.all(old[2, 1:] == 9)                   # the argument is left as it is
    none_kept, nsrc = simlog.start_from_rollout_np(v, end, bins, old=np.full((B, nb), 255, np.uint8))
    assert np.array_equal(none_kept, fresh) and np.array_equal(nsrc, fsrc)


def test_nan_and_ending_rules():
    v, end, bins = _case(5)
    v[0, 0, 1], v[0, 2, 4], v[2, 1, 1] = np.nan, 0.5, 0.5 + 2.0 ** -40
    end[:] = [0, 1, 0, 2, -1, 0, 0]
    v[1], v[3], v[4] = np.nan, np.nan, np.nan        # what the rollout leaves of a trajectory that stopped at step 0
    got, src = simlog.start_from_rollout_np(v, end, bins)
    assert got[0, 0] == 0 and got[0, 5] == 0 and got[2, 2] == 1      # a NaN rounds to 0, one half is not above one half, a hair above is
    assert np.all(got[[1, 3, 4]] == 255) and src[[1, 3, 4]].tolist() == [-1, -2, -3]
    want, wsrc = _loop(v, end, bins)
    assert np.array_equal(got, want) and np.array_equal(src, wsrc)
    # no binary: empty rows, the sources still say how the trajectories ended
    got, src = simlog.start_from_rollout_np(v, end, np.zeros(0, np.int64), old=np.zeros((len(end), 0), np.uint8))
    assert got.shape == (len(end), 0) and src.tolist() == [1, -1, 1, -2, -3, 1, 1]


def _args(name):
    m = re.search(r"int\s+%s\s*\(([^;]*?)\)\s*;" % name, HDR)
    assert m, name
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_the_export_and_the_constant():
    lib = _lib.load()
    name = "mld_warm_start_from_rollout"
    assert name in _lib.EXPORTS and hasattr(lib, name)
    args = _args(name)
    assert args == ["mld_problem_t *p", "mld_problem_t *aux", "int policy", "const double *u_seq", "const double *u_prev", "int flags", "int32_t *source_out",
                    "int64_t stats[4]"]
    assert len(getattr(lib, name).argtypes) == len(args) == 8
    assert re.search(r"#define\s+MLD_START_KEEP\s+1\b", HDR) and _lib.MLD_START_KEEP == 1
    assert "controller_base.py:493" in HDR.split("MIP start from a baseline rollout")[1]      # declared with the reference lines it stands for
    assert "MIP start from a baseline rollout" in _lib.version()
    src, stats = np.full(2, 7, np.int32), np.full(4, 7, np.int64)
    rc = lib.mld_warm_start_from_rollout(None, None, 1, None, None, 0, src.ctypes.data_as(C.POINTER(C.c_int32)), stats.ctypes.data_as(C.POINTER(C.c_int64)))
    if _lib.device_count() < 1:
        assert rc == -2 and b"no HIP device" in lib.mld_last_error()               # MLD_ERR_NO_DEVICE, before anything else
    else:
        assert rc == -1 and b"no batch resident" in lib.mld_last_error()            # MLD_ERR_INVALID: no handle
    assert np.all(src == 7) and np.all(stats == 7)
