"""The cut rounds of k_solve with grouped loads and LDS-typed views (s_gmi_round, s_mir_round phase B) against round 4's code paths.

mld_opts.reserved bit 22 (MLD_DBG_CUTS_R4) keeps round 4's loops selectable on the same binary and the same problem handle.  The new paths issue
their loads earlier and in larger groups but apply the same operations to the same operands in the same order, so every result must be EQUAL BIT
FOR BIT (objective, plan, status, node and pivot counts, lower bound).  Every case also checks that cuts were derived at all: the node or pivot
counts differ from a solve of the same instances without cut rounds -- otherwise an empty cut loop would pass.
"""
import numpy as np
import pytest

from pyhybridcontrol_amd import gpu, host, synthetic as syn

pytestmark = pytest.mark.gpu

CUTS_R4 = 1 << 22
GMI_SERIAL = 1 << 5
MIR_SERIAL = 1 << 15
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

    def run(self, reserved, **opts):
        """results of one solve of the instances with opts.reserved = reserved"""
        keep = {k: getattr(self.prob.opts, k) for k in opts}
        self.prob.set_opts(reserved=reserved, **opts)
        try:
            return self.prob.solve(self.x0, self.om)
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


def _assert_cuts_derived(case, out, tag, **opts):
    """the cut loop did something: node or pivot counts differ from a solve of the same instances without cut rounds"""
    none = case.run(0, **dict(opts, cut_rounds=0))
    print("%s: pivots %d, nodes %d with cut rounds; %d, %d without; status %s" % (
        tag, out["pivots"].sum(), out["nodes"].sum(), none["pivots"].sum(), none["nodes"].sum(), np.bincount(out["status"].astype(np.int64)).tolist()))
    assert out["nodes"].sum() != none["nodes"].sum() or out["pivots"].sum() != none["pivots"].sum(), tag


def _assert_equal_paths(case, tag, base=0, **opts):
    """new paths (reserved = base) against round 4's (base | MLD_DBG_CUTS_R4): bit-identical; and cuts were derived"""
    new, old = case.run(base, **opts), case.run(base | CUTS_R4, **opts)
    _assert_same_bits(new, old, tag)
    _assert_cuts_derived(case, new, tag, **opts)


def _assert_typed_paths_run(case, tag):
    """the shape takes the typed, grouped instantiations: every hot array of the pivot loop and the per-wave lines are in LDS"""
    assert case.shape["all_lds"] and case.shape["lMirCache"] >= 0, (tag, case.shape)


@pytest.fixture(scope="module")
def cfg3():
    c = Case("cfg3", 32, max_nodes=30, max_pivots=300)
    yield c
    c.close()


@pytest.mark.parametrize("opts", ({}, dict(cut_rounds=1)), ids=("default", "one_cut_round"))
def test_cfg2_five_column_chunks(opts):
    """cfg2 (n = 275: five column chunks, 19 live lanes in the last), 64 instances, NodeLimit 50"""
    c = Case("cfg2", 64, max_nodes=50, **opts)
    try:
        assert c.shape["n"] == 275, c.shape
        _assert_typed_paths_run(c, "cfg2")
        _assert_equal_paths(c, "cfg2 %s" % (opts or "default"))
    finally:
        c.close()


def test_cfg3_benchmark_shape(cfg3):
    """cfg3 (n = 575, the benchmark's shape: nine column chunks, 63 live lanes in the last), NodeLimit 30, IterationLimit 300"""
    assert cfg3.shape["n"] == 575, cfg3.shape
    _assert_typed_paths_run(cfg3, "cfg3")
    _assert_equal_paths(cfg3, "cfg3")


def test_cfg3_per_round_caps_cut_a_batch(cfg3):
    """three Gomory and three rounding cuts per round: the caps cut a batch of eight waves in the middle (before < room), where the commit order of
    the batch decides which cuts are kept"""
    _assert_equal_paths(cfg3, "cfg3 3+3 cuts per round", cuts_per_round=3, mir_per_round=3)


def test_cfg3_cut_rows_run_out_inside_a_round():
    """21 cut rows in all: cut_cap is reached in the third batch of the first round"""
    c = Case("cfg3", 32, max_nodes=30, max_pivots=300, max_cuts=21)
    try:
        assert c.shape["first_cap"] == c.shape["m0"] + 21, c.shape
        _assert_typed_paths_run(c, "cfg3 max_cuts=21")
        _assert_equal_paths(c, "cfg3 max_cuts=21")
    finally:
        c.close()


def test_cfg3_quadratic_cost():
    """cfg3 MIQP, 8 instances: the cut rounds run before the QP relaxation"""
    c = Case("cfg3", 8, quadratic=True, max_nodes=10, max_pivots=3000)
    try:
        _assert_equal_paths(c, "cfg3 MIQP")
    finally:
        c.close()


def test_cfg5_lines_outside_lds():
    """cfg5 (n = 2303), one instance: the per-wave lines do not fit LDS -- round 4's Gomory round and the block-wide c-MIR build run under both settings"""
    c = Case("cfg5", 1, max_nodes=3, max_pivots=3000)
    try:
        assert c.shape["lMirCache"] == -1 and not c.shape["all_lds"], c.shape
        _assert_equal_paths(c, "cfg5")
    finally:
        c.close()


@pytest.mark.parametrize("serial", (GMI_SERIAL, MIR_SERIAL), ids=("gmi_serial", "mir_serial"))
def test_cfg3_serial_paths_untouched(cfg3, serial):
    """one-at-a-time Gomory cuts / block-wide rounding cuts combined with the new bit and without it: equal within the pair"""
    _assert_equal_paths(cfg3, "cfg3 serial bit %d" % serial, base=serial)
