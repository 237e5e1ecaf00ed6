"""The block reductions of k_solve's selection without the LDS crossbar (block_max1_dpp, block_min1_dpp, block_argmax1_dpp: DPP row operations, a
branch-free combine of the waves' partials) against the ones they replaced in the simplex loop (block_max1, block_min1, block_argmax1 over __shfl_down),
on caller-supplied vectors of 512 (value, index) lanes through the internal entry mld_debug_reduce: one workgroup per vector runs both.

The rule of the arg-max is: the largest value; among equal values the smallest index >= 0; -1 when no lane with the largest value has an index.  Both
versions must return EQUAL BITS on every vector (values are compared as uint64), and both are checked against the same rule in numpy.
"""
import ctypes as C

import numpy as np
import pytest

from pyhybridcontrol_amd import _lib

pytestmark = pytest.mark.gpu

NT = 512
INF = np.inf


def _reduce(values, index):
    values = np.ascontiguousarray(values, dtype=np.float64).reshape(-1, NT)
    index = np.ascontiguousarray(index, dtype=np.int32).reshape(-1, NT)
    nv = values.shape[0]
    assert index.shape[0] == nv
    mx, arg, val = np.zeros(4 * nv), np.zeros(2 * nv, dtype=np.int32), np.zeros(2 * nv)
    lib = _lib.load()
    lib.mld_debug_reduce.restype = C.c_int
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    lib.mld_debug_reduce.argtypes = [dp, ip, C.c_int, dp, ip, dp]
    _lib.check(lib.mld_debug_reduce(values.ctypes.data_as(dp), index.ctypes.data_as(ip), nv, mx.ctypes.data_as(dp), arg.ctypes.data_as(ip), val.ctypes.data_as(dp)))
    return dict(max=mx[:2 * nv].reshape(nv, 2), min=mx[2 * nv:].reshape(nv, 2), arg=arg.reshape(nv, 2), val=val.reshape(nv, 2))


def _rule(values, index):
    """the arg-max rule in numpy: (index, value) per vector"""
    out_i, out_v = [], []
    for v, i in zip(values.reshape(-1, NT), index.reshape(-1, NT)):
        m = v.max()
        cand = i[(v == m) & (i >= 0)]
        out_i.append(int(cand.min()) if cand.size else -1)
        out_v.append(m)
    return np.array(out_i, dtype=np.int32), np.array(out_v)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _check(values, index, tag):
    values = np.asarray(values, dtype=np.float64).reshape(-1, NT)
    index = np.asarray(index, dtype=np.int32).reshape(-1, NT)
    r = _reduce(values, index)
    ri, rv = _rule(values, index)
    for k in ("max", "min", "val"):
        assert np.array_equal(_bits(r[k][:, 0]), _bits(r[k][:, 1])), (tag, k, np.flatnonzero(_bits(r[k][:, 0]) != _bits(r[k][:, 1]))[:8].tolist())
    assert np.array_equal(r["arg"][:, 0], r["arg"][:, 1]), (tag, np.flatnonzero(r["arg"][:, 0] != r["arg"][:, 1])[:8].tolist())
    assert np.array_equal(r["arg"][:, 1], ri), (tag, np.flatnonzero(r["arg"][:, 1] != ri)[:8].tolist())
    assert np.array_equal(_bits(r["val"][:, 1]), _bits(rv)), tag
    assert np.array_equal(_bits(r["max"][:, 1]), _bits(values.max(axis=1))), tag
    assert np.array_equal(_bits(r["min"][:, 1]), _bits(values.min(axis=1))), tag
    return r


def _no_candidate(nv, sentinel):
    return np.full((nv, NT), sentinel), np.full((nv, NT), -1, dtype=np.int32)


def test_seeded_random_vectors():
    """pricing-like vectors: a score > 0 with its lane as the index, or -inf and -1; 200 vectors with 0 .. 512 candidates"""
    rng = np.random.default_rng(20261019)
    nv = 200
    v = rng.uniform(1e-12, 10.0, size=(nv, NT)) ** 2
    keep = rng.uniform(size=(nv, NT)) < rng.uniform(0.0, 1.0, size=(nv, 1))
    v = np.where(keep, v, -INF)
    i = np.where(keep, np.arange(NT)[None, :], -1)
    r = _check(v, i, "random")
    assert (r["arg"][:, 1] >= 0).sum() > 150


def test_all_values_equal_smallest_index_wins():
    v = np.full((3, NT), 2.5)
    i = np.stack([np.arange(NT), np.arange(NT)[::-1], np.roll(np.arange(NT), 77) + 1000])
    r = _check(v, i, "equal")
    assert r["arg"][:, 1].tolist() == [0, 0, 1000]


@pytest.mark.parametrize("lane", [0, 31, 32, 63, 64, 511])
def test_one_candidate_alone(lane):
    """the entering column's convention (-1.0, -1 without a candidate) and the pricing one (-inf, -1)"""
    v, i = _no_candidate(2, -1.0)
    v[1, :] = -INF
    v[:, lane] = [0.375, 1e-30]
    i[:, lane] = lane + 3
    r = _check(v, i, "alone %d" % lane)
    assert r["arg"][:, 1].tolist() == [lane + 3, lane + 3]


def test_winner_in_each_wave_and_ties():
    """the winner in each of the eight waves; ties across waves, inside one 16-lane row, across the rows and halves of a wave: the smallest index wins
    wherever it sits; indices out of lane order"""
    rng = np.random.default_rng(7)
    vs, ids = [], []
    for wave in range(8):      # one winner, in every wave, at several lanes of it
        for lane in (0, 15, 16, 47, 63):
            v = rng.uniform(0.1, 1.0, size=NT); v[wave * 64 + lane] = 3.0
            vs.append(v); ids.append(np.arange(NT))
    for lanes in ([5, 9], [3, 12, 14], [15, 16], [31, 32], [0, 63], [63, 64], [10, 74, 138, 202, 266, 330, 394, 458], [511, 0], [200, 100, 300]):
        for order in (1, -1):      # the tied lanes hold the largest value; their indices ascend or descend with the lane
            v = rng.uniform(0.1, 1.0, size=NT); v[lanes] = 7.0
            idx = np.arange(NT) if order == 1 else 5000 - np.arange(NT)
            vs.append(v); ids.append(idx)
    for _ in range(20):        # indices a random permutation, many ties
        vs.append(rng.integers(1, 4, size=NT).astype(np.float64)); ids.append(rng.permutation(NT) + 17)
    for _ in range(10):        # a lane with the largest value and no index loses to an equal one with an index, wins the value against smaller ones
        v = rng.integers(1, 4, size=NT).astype(np.float64); idx = rng.permutation(NT)
        idx[rng.uniform(size=NT) < 0.7] = -1
        vs.append(v); ids.append(idx)
    _check(np.array(vs), np.array(ids), "ties")


def test_no_candidate_gives_minus_one_and_the_sentinel():
    for sentinel in (-1.0, -INF):
        v, i = _no_candidate(2, sentinel)
        r = _check(v, i, "none")
        assert r["arg"].tolist() == [[-1, -1], [-1, -1]]
        assert np.all(r["val"] == sentinel)


def test_infinities_and_subnormals():
    rng = np.random.default_rng(11)
    sub = 5e-324
    vs, ids = [], []
    v = np.full(NT, -INF); v[100] = sub; vs.append(v); ids.append(np.where(v > -INF, np.arange(NT), -1))
    v = rng.uniform(1, 2, size=NT) * 1e-310; vs.append(v); ids.append(np.arange(NT))                 # all subnormal
    v = rng.uniform(1, 2, size=NT); v[[70, 300]] = INF; vs.append(v); ids.append(np.arange(NT))       # +inf twice
    v = -rng.uniform(1, 2, size=NT) * 1e-310; v[400] = -INF; vs.append(v); ids.append(np.arange(NT))  # negative subnormals (the negated ratios), -inf
    v = np.full(NT, -INF); v[[3, 259]] = [sub, 2 * sub]; vs.append(v); ids.append(np.arange(NT))
    v = -rng.uniform(0.5, 2, size=NT); v[rng.uniform(size=NT) < 0.5] = -INF; vs.append(v); ids.append(np.arange(NT))
    _check(np.array(vs), np.array(ids), "inf / subnormal")
