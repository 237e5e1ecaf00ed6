"""Two consecutive dual-simplex pivots in one dictionary pass (k_solve: s_pivot_pair) against one pass per pivot.

mld_opts.reserved bit 21 (MLD_DBG_NO_PIVOT_PAIRS) switches the pairs off on the same binary and the same problem handle.  The pair applies the
same operations to every dictionary entry in the same order, so every result must be EQUAL BIT FOR BIT (objective, plan, status, node and pivot
counts, lower bound); only telemetry()["rows_updated"] -- the (row, sector) pairs actually moved -- may differ, and it must fall.  Where the
pairs cannot engage (quadratic cost; a shape whose hot arrays are not all in LDS) the count must not move either.
"""
import numpy as np
import pytest

from pyhybridcontrol_amd import gpu, host, synthetic as syn

pytestmark = pytest.mark.gpu

NO_PAIRS = 1 << 21
KEYS = ("obj", "v", "status", "nodes", "pivots", "lower_bound")


class Case(object):
    """one model of a synthetic configuration, its instances and one problem handle"""

    def __init__(self, name, batch, quadratic=False, **opts):
        wl = syn.make_workload(name, batch=batch, quadratic=quadratic)
        ag = wl["agents"][0]
        self.x0, self.om = ag["x0"], ag["omega"]
        self.model = gpu.GpuModel([ag["mats"]], ag["dims"])
        self.prob = gpu.GpuProblem(self.model, wl["N_p"], wl["N_tilde"], host.cost_from_atoms(ag["atoms"], ag["dims"], wl["N_p"], wl["N_tilde"]), **opts)
        self.shape = self.prob.debug_shape()

    def run(self, reserved, batch=None, **opts):
        """results and rows_updated of one solve of the first `batch` instances with opts.reserved = reserved"""
        b = self.x0.shape[0] if batch is None else batch
        keep = {k: getattr(self.prob.opts, k) for k in opts}
        self.prob.set_opts(reserved=reserved, **opts)
        try:
            out = self.prob.solve(self.x0[:b], self.om[:b])
            rows = self.prob.telemetry()["rows_updated"].copy()
        finally:
            self.prob.set_opts(reserved=0, **keep)
        return out, rows

    def both(self, batch=None, **opts):
        return self.run(0, batch, **opts), self.run(NO_PAIRS, batch, **opts)

    def close(self):
        self.prob.close()
        self.model.close()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def _assert_same_bits(on, off, tag):
    for k in KEYS:
        a, b = _bits(on[k]), _bits(off[k])
        assert a.shape == b.shape, (tag, k, a.shape, b.shape)
        diff = np.flatnonzero(np.any((a != b).reshape(a.shape[0], -1), axis=1))
        assert diff.size == 0, (tag, k, "instances that differ:", diff[:8].tolist())


def _assert_fused(case, res, tag):
    """bit-identical results; the pairs engaged: never more (row, sector) pairs moved, and fewer on at least one instance"""
    (on, rows_on), (off, rows_off) = res
    assert case.shape["all_lds"] and case.shape["lPair"] >= 0, (tag, case.shape)
    _assert_same_bits(on, off, tag)
    print("%s: rows_updated %d with pairs, %d without (%.1f %% fewer); pivots %d, nodes %d, status %s" % (
        tag, rows_on.sum(), rows_off.sum(), 100.0 * (1.0 - rows_on.sum() / max(1, rows_off.sum())), on["pivots"].sum(), on["nodes"].sum(),
        np.bincount(on["status"].astype(np.int64)).tolist()))
    assert np.all(rows_on <= rows_off), (tag, np.flatnonzero(rows_on > rows_off)[:8])
    assert np.any(rows_on < rows_off), tag


def _assert_not_fused(res, tag):
    (on, rows_on), (off, rows_off) = res
    _assert_same_bits(on, off, tag)
    assert np.array_equal(rows_on, rows_off), (tag, np.flatnonzero(rows_on != rows_off)[:8])
    assert rows_on.sum() > 0, tag


@pytest.fixture(scope="module")
def cfg3():
    c = Case("cfg3", 32, max_nodes=30, max_pivots=300)
    yield c
    c.close()


@pytest.fixture(scope="module")
def cfg3_limited(cfg3):
    """cfg3, 32 instances, NodeLimit 30, IterationLimit 300 -- with and without the pairs, computed once"""
    return cfg3.both()


@pytest.mark.parametrize("opts", ({}, dict(cut_rounds=1)), ids=("default", "one_cut_round"))
def test_cfg2_branch_and_bound_with_a_node_limit(opts):
    """cfg2 (n = 275: 35 sectors, at most three sector groups), 64 instances, NodeLimit 50: root LP, cut rounds and re-solves; with one cut round
    only, most instances branch and several searches end at the node limit in the middle of a dive"""
    c = Case("cfg2", 64, max_nodes=50, **opts)
    try:
        _assert_fused(c, c.both(), "cfg2 %s" % (opts or "default"))
    finally:
        c.close()


def test_cfg3_node_and_pivot_limits(cfg3, cfg3_limited):
    """cfg3 (n = 575: 72 sectors -- every sector-group count of the update, two row chunks per wave); IterationLimit 300 ends LPs between the two
    pivots of a pair"""
    assert cfg3.shape["n"] == 575, cfg3.shape
    _assert_fused(cfg3, cfg3_limited, "cfg3")


def test_cfg3_pivot_limit_of_the_other_parity(cfg3, cfg3_limited):
    """the same instances with IterationLimit one below the pivot count at which a finished instance ended: that instance now meets the limit one
    pivot early, at the other parity of its pivot count"""
    on = cfg3_limited[0][0]
    done = np.flatnonzero((on["status"] == 0) & (on["pivots"] > 2) & (on["pivots"] < 300))
    assert done.size, "an instance that finished below the limit is needed"
    pick = done[np.argmax(on["pivots"][done])]
    limit = int(on["pivots"][pick]) - 1
    res = cfg3.both(max_pivots=limit)
    _assert_fused(cfg3, res, "cfg3 IterationLimit %d" % limit)
    assert res[0][0]["pivots"][pick] <= limit, (pick, limit, res[0][0]["pivots"][pick])


def test_cfg3_with_a_time_limit(cfg3):
    """a generous TimeLimit: the deadline branch of the loop is evaluated (and never fires); results equal"""
    res = cfg3.both(batch=16, time_limit=120.0)
    _assert_fused(cfg3, res, "cfg3 TimeLimit")


def test_quadratic_cost_never_pairs():
    """cfg3 MIQP, 8 instances: the simplicial decomposition owns the cost row between pivots -- no pairs, so rows_updated does not move"""
    c = Case("cfg3", 8, quadratic=True, max_nodes=10, max_pivots=3000)
    try:
        _assert_not_fused(c.both(), "cfg3 MIQP")
    finally:
        c.close()


def test_shape_outside_lds_never_pairs():
    """cfg5 (n = 2303), one instance: the bounds do not fit LDS, the generic pivot loop runs and there is no room for the second pivot's buffers"""
    c = Case("cfg5", 1, max_nodes=3, max_pivots=3000)
    try:
        assert not c.shape["all_lds"] and c.shape["lPair"] == -1, c.shape
        _assert_not_fused(c.both(), "cfg5")
    finally:
        c.close()
