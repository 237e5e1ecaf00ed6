"""k_solve's choice of (row, column) -- block reductions over DPP row operations with a branch-free combine of the waves' partials, pass 1 of the ratio
test with its loads hoisted and a branch-free eligibility (one call for up to two columns per thread, groups of four column chunks beyond) -- against
the selection it replaces.

mld_opts.reserved bit 27 (MLD_DBG_SELECT_R6) keeps the earlier code selectable on the same binary and the same problem handle.  The choice itself must
not change: every result must be EQUAL BIT FOR BIT (objective, plan, status, node and pivot counts, lower bound) on every instance, and
telemetry()["rows_updated"] must be equal too.  Every case also checks that its path ran: pivots were made and the shape has the number of row chunks
of the pricing (512 rows each) and of columns per thread (512 threads) the case is about.
"""
import numpy as np
import pytest

from pyhybridcontrol_amd import gpu, host, synthetic as syn

pytestmark = pytest.mark.gpu

SELECT_R6 = 1 << 27
NO_PIVOT_PAIRS = 1 << 21
NO_LONG_STEP = 1 << 14
NO_PERTURB = 1 << 13
REFACTOR_ALWAYS = 1 << 1
BASES = (0, NO_PIVOT_PAIRS, NO_LONG_STEP, NO_PERTURB, REFACTOR_ALWAYS)
BASE_IDS = ("default", "no_pivot_pairs", "no_long_step", "no_perturbation", "refactor_always")
KEYS = ("obj", "v", "status", "nodes", "pivots", "lower_bound")
NT = 512         # threads of a workgroup: rows per chunk of the pricing scan, columns per chunk of the ratio test
PAIR = 2         # columns per thread up to which pass 1 of the ratio test is one call (s_ratio_pass1<L, 2>); wider rows take groups of four chunks


class Case(object):
    """one model of a synthetic configuration, its instances and one problem handle"""

    def __init__(self, name, batch, quadratic=False, **opts):
        wl = syn.make_workload(name, batch=batch, quadratic=quadratic)
        ag = wl["agents"][0]
        self.x0, self.om = ag["x0"], ag["omega"]
        self.model = gpu.GpuModel([ag["mats"]], ag["dims"])
        self.prob = gpu.GpuProblem(self.model, wl["N_p"], wl["N_tilde"], host.cost_from_atoms(ag["atoms"], ag["dims"], wl["N_p"], wl["N_tilde"]), **opts)
        self.shape = self.prob.debug_shape()
        self.quadratic = quadratic
        self.default = None      # results and rows_updated of reserved = 0 (the no-perturbation case compares its counters with them)

    def run(self, reserved, batch=None, handoff=None, **opts):
        """results and rows_updated of one solve of the first `batch` instances with opts.reserved = reserved"""
        b = self.x0.shape[0] if batch is None else batch
        keep = {k: getattr(self.prob.opts, k) for k in opts}
        self.prob.set_opts(reserved=reserved, **opts)
        try:
            if handoff:      # (no telemetry after a hand-off: mld_download_telemetry answers "nothing solved")
                return self.prob.solve_handoff_device(self.x0[:b], self.om[:b], **handoff), None
            out = self.prob.solve(self.x0[:b], self.om[:b])
            return out, self.prob.telemetry()["rows_updated"].copy()
        finally:
            self.prob.set_opts(reserved=0, **keep)

    def chunks(self):
        """(row chunks of the original rows, row chunks at capacity, columns per thread)"""
        s = self.shape
        return -(-s["m0"] // NT), -(-s["mcap"] // NT), -(-s["n"] // NT)

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
    """the present selection (reserved = base) against the earlier one (base | MLD_DBG_SELECT_R6): bit-identical on every instance"""
    (new, rows_new), (old, rows_old) = case.run(base, **kw), case.run(base | SELECT_R6, **kw)
    print("%s (n %d, m0 %d, mcap %d): pivots %d, nodes %d, rows_updated %d, status %s" % (
        tag, case.shape["n"], case.shape["m0"], case.shape["mcap"], new["pivots"].sum(), new["nodes"].sum(), rows_new.sum(), np.bincount(new["status"].astype(np.int64)).tolist()))
    _assert_same_bits(new, old, tag)
    assert np.array_equal(rows_new, rows_old), (tag, np.flatnonzero(rows_new != rows_old)[:8].tolist())
    assert new["pivots"].sum() > 0 and rows_new.sum() > 0, tag
    if base == 0 and not kw:
        case.default = (new, rows_new)
    if base == NO_PERTURB and not kw and not case.quadratic:
        # Bland's rule ran: the switch is read in one place only (s_dual_simplex_impl in csrc/problem.inc: `pert_ok = !w.P && !(w.dbg & MLD_DBG_NO_PERTURB)`, used at
        # `if (stall > 30 && pert_ok && !sh.perturbed)` just before `bland = stall > 30`; a second use of the bit would void this argument), where a solve that has stalled for more than 30 pivots would perturb its costs.  Without the
        # perturbation the loop goes on under Bland's rule from there, so counters that differ from the default's -- pivots, nodes or the rows the updates
        # moved -- say that `stall > 30` was reached.  (With a quadratic cost there is no perturbation in either run: a stalled solve pivots under Bland's
        # rule in both.)
        if case.default is None:
            case.default = case.run(0)
        ref, rows_ref = case.default
        changed = int(np.count_nonzero((new["pivots"] != ref["pivots"]) | (new["nodes"] != ref["nodes"]) | (rows_new != rows_ref)))
        print("%s: instances whose pivots, nodes or rows_updated differ from the default's (stall > 30 reached, Bland's rule ran): %d" % (tag, changed))
        assert changed > 0, tag
    return new


@pytest.fixture(scope="module")
def cfg2():
    c = Case("cfg2", 32, max_nodes=50)
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
    c = Case("cfg5", 8, max_nodes=3, max_pivots=3000)
    yield c
    c.close()


@pytest.mark.parametrize("base", BASES, ids=BASE_IDS)
def test_cfg2_one_row_chunk_one_column(cfg2, base):
    """cfg2 (n = 275), 32 instances, NodeLimit 50: m < 512 -- one row chunk in the pricing scan; one column per thread"""
    m0c, _, cols = cfg2.chunks()
    assert cfg2.shape["all_lds"] and cfg2.shape["lPair"] >= 0 and cfg2.shape["m0"] < NT and m0c == 1 and cols == 1, cfg2.shape
    _assert_equal_paths(cfg2, "cfg2 %d" % base, base=base)


@pytest.mark.parametrize("base", BASES, ids=BASE_IDS)
def test_cfg3_two_row_chunks_two_columns(cfg3, base):
    """cfg3 (n = 575, the benchmark's shape), 32 instances: two columns per thread (pass 1 in one call); the original rows fit one chunk of the
    pricing scan and the cut rows take the dictionary into a second one"""
    m0c, capc, cols = cfg3.chunks()
    assert cfg3.shape["all_lds"] and cfg3.shape["lPair"] >= 0 and m0c == 1 and capc == 2 and cols == PAIR, cfg3.shape
    _assert_equal_paths(cfg3, "cfg3 %d" % base, base=base)
    if base == 0:      # (cut rows took an instance's dictionary past the first chunk: the cut rows of instances 0 .. 3, from solves of the first 1 .. 4 instances)
        cuts = np.diff([0] + [int(cfg3.run(0, batch=b)[0]["stats"]["cuts"]) for b in range(1, 5)])
        print("cfg3: cut rows derived by instances 0..3:", cuts.tolist())
        assert cfg3.shape["m0"] + cuts.max() > NT, cuts


@pytest.mark.parametrize("base", BASES, ids=BASE_IDS)
def test_cfg3_quadratic_cost(cfg3_miqp, base):
    """cfg3 MIQP, 8 instances: no pairs and no look-ahead; the dual simplex of the LP bounds between the primal simplex runs of the decomposition"""
    _, _, cols = cfg3_miqp.chunks()
    assert cols == PAIR, cfg3_miqp.shape
    _assert_equal_paths(cfg3_miqp, "cfg3 MIQP %d" % base, base=base)


@pytest.mark.parametrize("base", BASES, ids=BASE_IDS)
def test_cfg5_groups_of_four_row_chunks_five_columns(cfg5, base):
    """cfg5 (n = 2303), 8 instances, NodeLimit 3: five columns per thread -- pass 1 runs two groups of four
    column chunks; four row chunks and more with cuts; hot arrays outside LDS, generic pointers"""
    s = cfg5.shape
    m0c, capc, cols = cfg5.chunks()
    print("cfg5: m0 %d, mcap %d" % (s["m0"], s["mcap"]))
    assert s["n"] == 2303 and not s["all_lds"] and s["lPair"] == -1, s
    assert cols == 5 and cols > PAIR and m0c == 4 and capc > 4, s
    _assert_equal_paths(cfg5, "cfg5 %d" % base, base=base)


def test_cfg3_handoff_inside_the_launch(cfg3):
    """the in-kernel hand-off with a first pass of 3 nodes: items are published and solved by other workgroups"""
    ho = dict(first_nodes=3, sub_nodes=12, max_gen=8, max_children=64, max_tree=100000, room_factor=64.0)
    m0c, capc, cols = cfg3.chunks()
    assert cfg3.shape["all_lds"] and m0c == 1 and capc == 2 and cols == PAIR, cfg3.shape
    (new, _), (old, _) = cfg3.run(0, handoff=ho), cfg3.run(SELECT_R6, handoff=ho)
    print("cfg3 hand-off:", new["handoff"], old["handoff"])
    assert new["handoff"]["items"] >= 1 and new["handoff"] == old["handoff"], (new["handoff"], old["handoff"])
    _assert_same_bits(new, old, "cfg3 hand-off")
    assert new["pivots"].sum() > 0


def test_cfg3_with_a_time_limit(cfg3):
    """a generous TimeLimit: the deadline branch of the loop and of the pair's look-ahead is evaluated (and never fires); results equal"""
    m0c, capc, cols = cfg3.chunks()
    assert cfg3.shape["all_lds"] and cfg3.shape["lPair"] >= 0 and m0c == 1 and capc == 2 and cols == PAIR, cfg3.shape
    _assert_equal_paths(cfg3, "cfg3 TimeLimit", batch=16, time_limit=120.0)


def test_cfg3_hot_arrays_out_of_lds(monkeypatch):
    """cfg3 on a handle whose hot arrays are all forced out of LDS (MLD_SOL_SLOT=all while it is created): the generic-pointer instantiation of the loop
    on a shape with two columns per thread, no pairs"""
    monkeypatch.setenv("MLD_SOL_SLOT", "all")
    try:
        c = Case("cfg3", 8, max_nodes=30, max_pivots=300)
    finally:
        monkeypatch.delenv("MLD_SOL_SLOT", raising=False)
    try:
        s = c.shape
        assert not s["all_lds"] and s["slot_mask"] != 0 and s["lXB"] == -1 and s["lDw"] == -1 and s["lBasic"] == -1, s
        assert c.chunks()[2] == PAIR, s
        _assert_equal_paths(c, "cfg3 slot")
    finally:
        c.close()
