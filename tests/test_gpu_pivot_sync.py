"""k_solve's pivot with half its block barriers -- three in its first half (s_pivot_head) instead of six, the sector and row lists of the update in
one exchange of per-wave counts (s_pivot_update, s_pivot_pair: list_counts) instead of two barriers per 512-wide chunk and two block sums -- against
the barrier sequence it had before.

mld_opts.reserved bit 26 (MLD_DBG_PIVOT_SYNC_R5) keeps the earlier sequence selectable on the same binary and the same problem handle.  Only the
synchronisation differs: the same operations run on the same operands in the same order and the lists come out in the same order, so every result
must be EQUAL BIT FOR BIT (objective, plan, status, node and pivot counts, lower bound) on every instance, and telemetry()["rows_updated"] -- the
(row, sector) pairs moved, which the pair derives from the exchanged counts -- must be equal too.  Every case also checks that its path ran: pivots
were made, the shape takes the instantiation and the number of row chunks the case is about, and on cfg3's root LP the long-step ratio test made a
difference.
"""
import numpy as np
import pytest

from pyhybridcontrol_amd import gpu, host, synthetic as syn

pytestmark = pytest.mark.gpu

SYNC_R5 = 1 << 26
NO_PIVOT_PAIRS = 1 << 21
NO_LONG_STEP = 1 << 14
REFACTOR_ALWAYS = 1 << 1
BASES = (0, NO_PIVOT_PAIRS, NO_LONG_STEP, REFACTOR_ALWAYS)
BASE_IDS = ("default", "no_pivot_pairs", "no_long_step", "refactor_always")
KEYS = ("obj", "v", "status", "nodes", "pivots", "lower_bound")
CHUNK = 512      # rows per chunk of the row list (SOL_NT)


class Case(object):
    """one model of a synthetic configuration, its instances and one problem handle"""

    def __init__(self, name, batch, quadratic=False, **opts):
        wl = syn.make_workload(name, batch=batch, quadratic=quadratic)
        ag = wl["agents"][0]
        self.x0, self.om = ag["x0"], ag["omega"]
        self.model = gpu.GpuModel([ag["mats"]], ag["dims"])
        self.prob = gpu.GpuProblem(self.model, wl["N_p"], wl["N_tilde"], host.cost_from_atoms(ag["atoms"], ag["dims"], wl["N_p"], wl["N_tilde"]), **opts)
        self.shape = self.prob.debug_shape()

    def run(self, reserved, batch=None, handoff=None, **opts):
        """results and rows_updated of one solve of the first `batch` instances with opts.reserved = reserved"""
        b = self.x0.shape[0] if batch is None else batch
        keep = {k: getattr(self.prob.opts, k) for k in opts}
        self.prob.set_opts(reserved=reserved, **opts)
        try:
            if handoff:
                return self.prob.solve_handoff_device(self.x0[:b], self.om[:b], **handoff), None
            out = self.prob.solve(self.x0[:b], self.om[:b])
            return out, self.prob.telemetry()["rows_updated"].copy()
        finally:
            self.prob.set_opts(reserved=0, **keep)

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


def _assert_equal_paths(case, tag, base=0, **kw):
    """the halved barrier sequence (reserved = base) against the earlier one (base | MLD_DBG_PIVOT_SYNC_R5): bit-identical on every instance"""
    (new, rows_new), (old, rows_old) = case.run(base, **kw), case.run(base | SYNC_R5, **kw)
    print("%s (m0 %d, mcap %d): pivots %d, nodes %d, rows_updated %d, status %s" % (
        tag, case.shape["m0"], case.shape["mcap"], new["pivots"].sum(), new["nodes"].sum(), rows_new.sum(), np.bincount(new["status"].astype(np.int64)).tolist()))
    _assert_same_bits(new, old, tag)
    assert np.array_equal(rows_new, rows_old), (tag, np.flatnonzero(rows_new != rows_old)[:8].tolist())
    assert new["pivots"].sum() > 0 and rows_new.sum() > 0, tag
    return new


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
def test_cfg2_one_row_chunk(cfg2, base):
    """cfg2 (n = 275), 64 instances, NodeLimit 50: the original rows are well inside one chunk of the row list"""
    assert cfg2.shape["all_lds"] and cfg2.shape["lPair"] >= 0 and cfg2.shape["m0"] <= CHUNK, cfg2.shape
    _assert_equal_paths(cfg2, "cfg2 %d" % base, base=base)


@pytest.mark.parametrize("base", BASES, ids=BASE_IDS)
def test_cfg3_one_and_two_row_chunks(cfg3, base):
    """cfg3 (n = 575, the benchmark's shape), 32 instances: the original rows fit one chunk, the cut rows take the dictionary into a second one"""
    assert cfg3.shape["all_lds"] and cfg3.shape["lPair"] >= 0 and cfg3.shape["m0"] <= CHUNK < cfg3.shape["mcap"], cfg3.shape
    out = _assert_equal_paths(cfg3, "cfg3 %d" % base, base=base)
    if base == 0:      # the long-step ratio test of the root LP ran: without it the pivot counts differ
        plain, _ = cfg3.run(NO_LONG_STEP)
        print("cfg3: pivots %d with the long-step ratio test, %d without" % (out["pivots"].sum(), plain["pivots"].sum()))
        assert np.any(out["pivots"] != plain["pivots"])
        # (cut rows took an instance's dictionary past the first chunk: the cut rows of instances 0 .. 3, from solves of the first 1 .. 4 instances)
        cuts = np.diff([0] + [int(cfg3.run(0, batch=b)[0]["stats"]["cuts"]) for b in range(1, 5)])
        print("cfg3: cut rows derived by instances 0..3:", cuts.tolist())
        assert cfg3.shape["m0"] + cuts.max() > CHUNK, cuts


@pytest.mark.parametrize("base", BASES, ids=BASE_IDS)
def test_cfg3_quadratic_cost(cfg3_miqp, base):
    """cfg3 MIQP, 8 instances: no pairs; the primal simplex of the simplicial decomposition pivots through s_pivot, the generic-pointer instantiation"""
    _assert_equal_paths(cfg3_miqp, "cfg3 MIQP %d" % base, base=base)


@pytest.mark.parametrize("base", BASES, ids=BASE_IDS)
def test_cfg5_four_row_chunks_generic_pointers(cfg5, base):
    """cfg5 (n = 2303: 288 sectors), 4 instances, NodeLimit 3: four row chunks, the hot arrays outside LDS -- the generic-pointer instantiation, no pairs"""
    s = cfg5.shape
    print("cfg5: m0 %d, mcap %d" % (s["m0"], s["mcap"]))
    assert s["n"] == 2303 and not s["all_lds"] and s["lPair"] == -1, s
    assert 3 * CHUNK < s["m0"] <= 4 * CHUNK and s["mcap"] <= 8 * CHUNK, s      # (four chunks from the first pivot on; the exchange holds eight)
    _assert_equal_paths(cfg5, "cfg5 %d" % base, base=base)


def test_cfg3_handoff_inside_the_launch(cfg3):
    """the in-kernel hand-off with a first pass of 3 nodes: items are published and solved by other workgroups"""
    ho = dict(first_nodes=3, sub_nodes=12, max_gen=8, max_children=64, max_tree=100000, room_factor=64.0)
    (new, _), (old, _) = cfg3.run(0, handoff=ho), cfg3.run(SYNC_R5, handoff=ho)
    print("cfg3 hand-off:", new["handoff"], old["handoff"])
    assert new["handoff"]["items"] >= 1 and new["handoff"] == old["handoff"], (new["handoff"], old["handoff"])
    _assert_same_bits(new, old, "cfg3 hand-off")
    assert new["pivots"].sum() > 0


def test_cfg3_with_a_time_limit(cfg3):
    """a generous TimeLimit: the deadline branch of the loop and of the pair's look-ahead is evaluated (and never fires); results equal"""
    _assert_equal_paths(cfg3, "cfg3 TimeLimit", batch=16, time_limit=120.0)
