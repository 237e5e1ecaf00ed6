"""k_solve's phases outside the pivot loop with their loads in flight -- grouped row dot products (refresh, residual check, leaf check), grouped
thread-per-row walks over the sparse copy (presolve, dead rows, reset scatter, initial refresh, residual check), four rows at a time in the x_B
update of a bound list, the c-MIR screen by columns and its pipelined pass 1 -- against the one-load-at-a-time code they replace.

mld_opts.reserved bit 24 (MLD_DBG_WALKS_SERIAL) keeps the earlier loops selectable on the same binary and the same problem handle.  The new loops
issue their loads earlier and in groups but apply the same operations to the same operands in the same order, so every result must be EQUAL BIT FOR
BIT (objective, plan, status, node and pivot counts, lower bound) on every instance.  Every case also checks that its path ran at all: the node or
pivot counts differ from a solve of the same instances without cut rounds, and the shape flags say which instantiation the handle takes.
"""
import numpy as np
import pytest

from pyhybridcontrol_amd import gpu, host, synthetic as syn

pytestmark = pytest.mark.gpu

WALKS_SERIAL = 1 << 24
REFACTOR_ALWAYS = 1 << 1
NO_PRESOLVE = 1 << 12
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

    def run(self, reserved, rows=None, handoff=None, **opts):
        """results of one solve of the instances (all, or the given rows) with opts.reserved = reserved"""
        keep = {k: getattr(self.prob.opts, k) for k in opts}
        self.prob.set_opts(reserved=reserved, **opts)
        x0, om = (self.x0, self.om) if rows is None else (self.x0[rows], self.om[rows])
        try:
            if handoff:
                return self.prob.solve_handoff_device(x0, om, **handoff)
            return self.prob.solve(x0, om)
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


def _assert_cuts_derived(case, out, tag, base=0, **kw):
    """the cut loop did something: node or pivot counts differ from a solve of the same instances without cut rounds"""
    none = case.run(base, cut_rounds=0, **kw)
    print("%s: pivots %d, nodes %d with cut rounds; %d, %d without; status %s" % (
        tag, out["pivots"].sum(), out["nodes"].sum(), none["pivots"].sum(), none["nodes"].sum(), np.bincount(out["status"].astype(np.int64)).tolist()))
    assert out["nodes"].sum() != none["nodes"].sum() or out["pivots"].sum() != none["pivots"].sum(), tag


def _assert_equal_paths(case, tag, base=0, **kw):
    """grouped walks (reserved = base) against the serial ones (base | MLD_DBG_WALKS_SERIAL): bit-identical on every instance; and cuts were derived"""
    new, old = case.run(base, **kw), case.run(base | WALKS_SERIAL, **kw)
    _assert_same_bits(new, old, tag)
    _assert_cuts_derived(case, new, tag, base=base, **kw)
    return new


def _assert_typed_sparse_paths(case, tag):
    """the handle takes the typed instantiations (every hot array and the per-wave lines in LDS) -- with the sparse copy the handle was built with (presolve bit
    2, the default) that is the screen by columns and the pipelined pass 1"""
    assert case.shape["all_lds"] and case.shape["lMirCache"] >= 0, (tag, case.shape)
    assert int(case.prob.opts.presolve) & 4, (tag, int(case.prob.opts.presolve))


@pytest.fixture(scope="module")
def cfg3():
    c = Case("cfg3", 32, max_nodes=30, max_pivots=300)
    yield c
    c.close()


def test_cfg2_five_column_chunks():
    """cfg2 (n = 275: five column chunks, 19 live lanes in the last; short rows: remainder groups under 8), 64 instances, NodeLimit 50; some end at the root"""
    c = Case("cfg2", 64, max_nodes=50)
    try:
        assert c.shape["n"] == 275, c.shape
        _assert_typed_sparse_paths(c, "cfg2")
        out = _assert_equal_paths(c, "cfg2")
        assert (out["nodes"] <= 1).any(), np.bincount(out["nodes"])      # (instances that end at the root)
    finally:
        c.close()


def test_cfg3_benchmark_shape(cfg3):
    """cfg3 (n = 575, the benchmark's shape: rows of up to 25 entries -- three groups and a remainder --, columns of up to 52), NodeLimit 30, IterationLimit 300"""
    assert cfg3.shape["n"] == 575, cfg3.shape
    _assert_typed_sparse_paths(cfg3, "cfg3")
    _assert_equal_paths(cfg3, "cfg3")


def test_cfg3_refactor_at_every_verification(cfg3):
    """MLD_DBG_REFACTOR_ALWAYS: s_refactor -> s_reset_dictionary -> s_refresh and the residual check at every verification, with cut rows present; the
    number of cut rows is no multiple of 4 for at least one instance (a tail group of the row dot products)"""
    _assert_equal_paths(cfg3, "cfg3 refactor always", base=REFACTOR_ALWAYS)
    cuts = [int(cfg3.run(REFACTOR_ALWAYS, rows=slice(s, s + 1))["stats"]["cuts"]) for s in range(4)]
    print("cfg3 refactor always: cut rows derived by instances 0..3:", cuts)
    assert any(k > 0 for k in cuts) and any(k % 4 != 0 for k in cuts), cuts


def test_cfg3_without_presolve(cfg3):
    """MLD_DBG_NO_PRESOLVE: s_mark_dead from act_max, no implied bounds (the sparse copy still serves the walks)"""
    _assert_equal_paths(cfg3, "cfg3 no presolve", base=NO_PRESOLVE)


def test_cfg3_without_sparse_copy():
    """a handle built without the presolve's sparse copy (presolve = 2: bit 2 off): the dense screen and the dense pass 1 under both settings"""
    c = Case("cfg3", 32, max_nodes=30, max_pivots=300, presolve=2)
    try:
        assert not (int(c.prob.opts.presolve) & 4), int(c.prob.opts.presolve)
        _assert_equal_paths(c, "cfg3 presolve=2")
    finally:
        c.close()


def test_cfg3_quadratic_cost():
    """cfg3 MIQP, 8 instances, the settings of the other MIQP cases"""
    c = Case("cfg3", 8, quadratic=True, max_nodes=10, max_pivots=3000)
    try:
        _assert_equal_paths(c, "cfg3 MIQP")
    finally:
        c.close()


def test_cfg5_several_passes_generic_pointers():
    """cfg5 (n = 2303), one instance: the row dot products take several passes, the per-wave lines are outside LDS, the generic instantiations run"""
    c = Case("cfg5", 1, max_nodes=3, max_pivots=3000)
    try:
        assert c.shape["n"] == 2303 and c.shape["lMirCache"] == -1 and not c.shape["all_lds"], c.shape
        _assert_equal_paths(c, "cfg5")
    finally:
        c.close()


def test_cfg3_handoff_inside_the_launch(cfg3):
    """the in-kernel hand-off with a first pass of 3 nodes: items are published -- fixings at set-up, long bound lists, tails of fewer than 4 rows"""
    ho = dict(first_nodes=3, sub_nodes=12, max_gen=8, max_children=64, max_tree=100000, room_factor=64.0)
    new, old = cfg3.run(0, handoff=ho), cfg3.run(WALKS_SERIAL, handoff=ho)
    print("cfg3 hand-off:", new["handoff"], old["handoff"])
    assert new["handoff"]["items"] >= 1 and new["handoff"] == old["handoff"], (new["handoff"], old["handoff"])
    _assert_same_bits(new, old, "cfg3 hand-off")
    none = cfg3.run(0, handoff=ho, cut_rounds=0)
    assert new["nodes"].sum() != none["nodes"].sum() or new["pivots"].sum() != none["pivots"].sum()


def test_cfg3_per_round_caps(cfg3):
    """three Gomory and three rounding cuts per round: a change in the candidate list of the screen would change which cuts are kept"""
    _assert_equal_paths(cfg3, "cfg3 3+3 cuts per round", cuts_per_round=3, mir_per_round=3)


def test_cfg3_cut_rows_run_out_inside_a_round():
    """21 cut rows in all: the cap is reached inside the first round"""
    c = Case("cfg3", 32, max_nodes=30, max_pivots=300, max_cuts=21)
    try:
        assert c.shape["first_cap"] == c.shape["m0"] + 21, c.shape
        _assert_typed_sparse_paths(c, "cfg3 max_cuts=21")
        _assert_equal_paths(c, "cfg3 max_cuts=21")
    finally:
        c.close()
