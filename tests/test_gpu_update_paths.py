"""k_solve's row update with a unit (one row x 16 sectors) cut down to its payload -- s_update_rows_r7 / s_update_rows2_r7, what the default
instantiation of the dual simplex runs -- against the two templates it had before.

mld_opts.reserved bit 28 (MLD_DBG_UPDATE_R7) takes the loop into its legacy instantiation with the earlier templates, on the same binary and the
same problem handle.  Every element sees the same operations in the same order on both paths, so every result must be EQUAL BIT FOR BIT (objective,
plan, status, node and pivot counts, lower bound) on every instance, and telemetry()["rows_updated"] must be equal too.  The fixtures are those of
tests/test_gpu_pivot_sync.py.  Every case checks that pivots were made; on the shapes whose pivots can pair (cfg2, cfg3) the default run must also
have moved fewer (row, sector) pairs than a run without pairs, i.e. the pair's update ran.
"""
import numpy as np
import pytest

from pyhybridcontrol_amd import gpu, host, synthetic as syn
from pyhybridcontrol_amd._lib import MLD_DBG_UPDATE_R7

pytestmark = pytest.mark.gpu

NO_PIVOT_PAIRS = 1 << 21
NO_LONG_STEP = 1 << 14
REFACTOR_ALWAYS = 1 << 1
BASES = (0, NO_PIVOT_PAIRS, NO_LONG_STEP, REFACTOR_ALWAYS)
BASE_IDS = ("alone", "no_pivot_pairs", "no_long_step", "refactor_always")
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

    def run(self, reserved, handoff=None):
        """results and rows_updated of one solve with opts.reserved = reserved"""
        self.prob.set_opts(reserved=reserved)
        try:
            if handoff:
                return self.prob.solve_handoff_device(self.x0, self.om, **handoff), None
            out = self.prob.solve(self.x0, self.om)
            return out, self.prob.telemetry()["rows_updated"].copy()
        finally:
            self.prob.set_opts(reserved=0)

    def close(self):
        self.prob.close()
        self.model.close()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def _assert_same_bits(new, old, tag):
    for k in KEYS:
        a, b = _bits(new[k]), _bits(old[k])
        assert a.shape == b.shape, (tag, k, a.shape, b.shape)
        diff = np.flatnonzero(np.any((a != b).reshape(a.shape[0], -1), axis=1))
        assert diff.size == 0, (tag, k, "instances that differ:", diff[:8].tolist())


def _assert_equal_paths(case, tag, base, pairs_possible):
    """the default update (reserved = base) against the earlier templates (base | MLD_DBG_UPDATE_R7): bit-identical on every instance"""
    (new, rows_new), (old, rows_old) = case.run(base), case.run(base | MLD_DBG_UPDATE_R7)
    print("%s (m0 %d, mcap %d): pivots %d, nodes %d, rows_updated %d, status %s" % (
        tag, case.shape["m0"], case.shape["mcap"], new["pivots"].sum(), new["nodes"].sum(), rows_new.sum(), np.bincount(new["status"].astype(np.int64)).tolist()))
    _assert_same_bits(new, old, tag)
    assert np.array_equal(rows_new, rows_old), (tag, np.flatnonzero(rows_new != rows_old)[:8].tolist())
    assert new["pivots"].sum() > 0 and rows_new.sum() > 0, tag
    if pairs_possible and base == 0:      # pairs ran: without them more (row, sector) pairs are moved
        _, rows_single = case.run(NO_PIVOT_PAIRS)
        print("%s: rows_updated %d with pairs, %d without" % (tag, rows_new.sum(), rows_single.sum()))
        assert rows_new.sum() < rows_single.sum(), (tag, rows_new.sum(), rows_single.sum())


@pytest.fixture(scope="module")
def cfg2():
    c = Case("cfg2", 64, max_nodes=50)
    yield c
    c.close()


@pytest.fixture(scope="module")
def cfg3():
    c = Case("cfg3", 32, max_nodes=30, max_pivots=300)
    yield c
    c.close()


@pytest.fixture(scope="module")
def cfg3_miqp():
    c = Case("cfg3", 8, quadratic=True, max_nodes=10, max_pivots=3000)
    yield c
    c.close()


@pytest.fixture(scope="module")
def cfg5():
    c = Case("cfg5", 4, max_nodes=3, max_pivots=3000)
    yield c
    c.close()


@pytest.mark.parametrize("base", BASES, ids=BASE_IDS)
def test_cfg2(cfg2, base):
    """cfg2 (n = 275: 35 sectors, up to three groups), 64 instances, NodeLimit 50: the typed all-LDS loop with pairs"""
    assert cfg2.shape["all_lds"] and cfg2.shape["lPair"] >= 0, cfg2.shape
    _assert_equal_paths(cfg2, "cfg2 %d" % base, base, True)


@pytest.mark.parametrize("base", BASES, ids=BASE_IDS)
def test_cfg3(cfg3, base):
    """cfg3 (n = 575, the benchmark's shape: 73 sectors, up to five groups), 32 instances, NodeLimit 30, 300 pivots"""
    assert cfg3.shape["all_lds"] and cfg3.shape["lPair"] >= 0, cfg3.shape
    _assert_equal_paths(cfg3, "cfg3 %d" % base, base, True)


@pytest.mark.parametrize("base", BASES, ids=BASE_IDS)
def test_cfg3_quadratic_cost(cfg3_miqp, base):
    """cfg3 MIQP, 8 instances: no pairs; the primal simplex of the simplicial decomposition pivots through s_pivot, which picks its update at run time"""
    _assert_equal_paths(cfg3_miqp, "cfg3 MIQP %d" % base, base, False)


@pytest.mark.parametrize("base", BASES, ids=BASE_IDS)
def test_cfg5_generic_pointers(cfg5, base):
    """cfg5 (n = 2303: 288 sectors, 18 groups in chunks of four), 4 instances, NodeLimit 3: the generic-pointer instantiation, no pairs"""
    s = cfg5.shape
    assert s["n"] == 2303 and not s["all_lds"] and s["lPair"] == -1, s
    _assert_equal_paths(cfg5, "cfg5 %d" % base, base, False)


def test_cfg3_handoff_inside_the_launch(cfg3):
    """the in-kernel hand-off with a first pass of 3 nodes: items are published and solved by other workgroups"""
    ho = dict(first_nodes=3, sub_nodes=12, max_gen=8, max_children=64, max_tree=100000, room_factor=64.0)
    (new, _), (old, _) = cfg3.run(0, handoff=ho), cfg3.run(MLD_DBG_UPDATE_R7, handoff=ho)
    print("cfg3 hand-off:", new["handoff"], old["handoff"])
    assert new["handoff"]["items"] >= 1 and new["handoff"] == old["handoff"], (new["handoff"], old["handoff"])
    _assert_same_bits(new, old, "cfg3 hand-off")
    assert new["pivots"].sum() > 0
