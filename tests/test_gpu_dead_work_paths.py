"""k_solve's bound changes without the work nobody reads, against the code they replace.

A bound change (s_set_bounds, s_set_bounds_list) updates x_B of the MAINTAINED rows only: a row that can never bind (s_mark_dead) or a cut row that
s_purge_slack_cuts retired keeps a stale dictionary row and an x_B nobody reads.  mld_opts.reserved bit 29 (MLD_DBG_DEAD_WORK_R8) keeps the earlier
walk over every row on the same binary and the same problem handle.  Every value that is read sees the same operations in the same order on both paths,
so every result must be EQUAL BIT FOR BIT: obj, v, lower_bound, status, nodes, pivots and rows_updated per instance, cuts and refactors as totals.  The
pools are built by tests/_dead_work.py from those of tests/_history.py and tests/_paths.py, as tests/test_gpu_history.py builds its own.

Every case checks on the GPU's own counts that the bound-change path ran: the pool branches (more nodes than instances); the cases that name it have
an instance with more than 20 nodes and a node-limited one.  tests/test_dead_work_pools.py makes the same check with the CPU oracle.
"""
import ctypes as C

import numpy as np
import pytest

import _dead_work as dw
import _history as hist
from pyhybridcontrol_amd import _lib
from pyhybridcontrol_amd._lib import MLD_DBG_DEAD_WORK_R8

pytestmark = pytest.mark.gpu

KEEP_DEAD_ROWS, NO_ORDER = 1 << 4, 1 << 3
R8 = MLD_DBG_DEAD_WORK_R8


def _pair(pool, opts, base=0, idx=None):
    """the pool (or its instances idx, in that order) on ONE handle with reserved = base and base | R8"""
    h = pool.handle(**opts)
    try:
        idx = np.arange(pool.size) if idx is None else idx
        h.prob.set_opts(reserved=base)
        new = h.run(idx)
        h.prob.set_opts(reserved=base | R8)
        old = h.run(idx)
        h.prob.set_opts(reserved=base)
        again = h.run(idx)          # (and back: the handle has just held the other path's dictionaries)
        return new, old, again, h.prob.debug_shape()
    finally:
        h.close()


def _assert_equal(new, old, tag):
    n = len(new["status"])
    hist.assert_same_bits(new, {k: old[k] for k in hist.KEYS}, np.arange(n), tag)
    for k in ("cuts", "refactors"):
        assert int(new["stats"][k]) == int(old["stats"][k]), (tag, k, int(new["stats"][k]), int(old["stats"][k]))


def _check(pool, opts, tag, base=0, idx=None, deep=False, limited=False, branches=True):
    new, old, again, shape = _pair(pool, opts, base, idx)
    nodes, status = new["nodes"].astype(np.int64), new["status"].astype(np.int64)
    print("%s (n %d, m0 %d, all_lds %d): nodes %d (max %d), pivots %d, cuts %d, rows_updated %d, status %s" % (
        tag, shape["n"], shape["m0"], shape["all_lds"], nodes.sum(), nodes.max(), new["pivots"].sum(), int(new["stats"]["cuts"]), new["rows_updated"].sum(),
        np.bincount(status).tolist()))
    _assert_equal(new, old, tag + ": default against MLD_DBG_DEAD_WORK_R8")
    _assert_equal(again, old, tag + ": default after MLD_DBG_DEAD_WORK_R8 on the same handle")
    assert new["pivots"].sum() > 0, tag
    if branches:
        assert nodes.sum() > len(nodes), (tag, "the pool does not branch", nodes.sum(), len(nodes))
    if deep:
        assert nodes.max() > 20, (tag, "no instance with more than 20 nodes", nodes.max())
    if limited:
        assert (status == 2).any(), (tag, "no node-limited instance", np.bincount(status).tolist())
    return new, shape


def test_p35_multi_model_hard_rows():
    """P35 (n = 35), six hard-row models on one handle, generous budgets"""
    _, s = _check(dw.p35(), dw.GENEROUS, "P35", deep=True)
    assert s["n"] == 35


def test_p35_node_limit_of_three():
    """the same under NodeLimit 3: node-limited instances unwind their stacks through s_set_bounds_list"""
    _check(dw.p35(), dict(max_nodes=3, max_pivots=400000), "P35 NodeLimit 3", limited=True)


def test_p35_even_n():
    """P35 at N_tilde = 6 (n = 42, 36 rows: another row count against the walk's groups of four rows per wave)"""
    _, s = _check(dw.p35(N=6), dw.GENEROUS, "P35 N_tilde 6")
    assert s["n"] == 42


def test_p35_fixings_starts_and_cutoffs():
    """uploaded fixings, MIP starts, cutoffs and a per-instance cost: s_set_bounds_list through the fixings, the start's leaf and RINS"""
    _check(dw.p35("inputs"), dw.GENEROUS, "P35 inputs")


def test_p35_without_the_sparse_copy():
    """presolve without bit 2: no sparse copy of the rows and no per-instance presolve, so other rows are dead"""
    _check(dw.p35(), dict(dw.GENEROUS, presolve=2), "P35 presolve 2")


def test_p35_quadratic_cost():
    _check(dw.p35("quadratic"), dw.GENEROUS, "P35 MIQP")


def test_p35_slot_that_has_just_held_another_kind():
    """one slot, the queue in upload order, the instances of two models alternating: every dictionary is built in a slot that has just held an instance
    of the OTHER model, whose dead rows and retired cut rows are others.  Each position equals the same instance solved in a batch of its own under the
    earlier walk."""
    pool = dw.p35()
    midx = hist.p35()["midx"]
    a, b = np.flatnonzero(midx == 0), np.flatnonzero(midx == 3)
    order = np.ravel(np.column_stack([a, b]))
    h = pool.handle(n_slots=1, reserved=NO_ORDER, **dw.GENEROUS)
    try:
        assert h.prob.debug_shape()["n_slots"] == 1
        chain = h.run(order)
        h.prob.set_opts(reserved=NO_ORDER | R8)
        alone = [h.run([i]) for i in order]
    finally:
        h.close()
    ref = {k: np.concatenate([np.atleast_1d(o[k]) for o in alone]) for k in hist.KEYS}
    hist.assert_same_bits(chain, ref, np.arange(len(order)), "P35 alternating models on one slot")
    for k in ("cuts", "refactors"):
        assert int(chain["stats"][k]) == sum(int(o["stats"][k]) for o in alone), k
    assert chain["pivots"].sum() > 0


@pytest.mark.parametrize("base", (0, KEEP_DEAD_ROWS), ids=("alone", "keep_dead_rows"))
def test_cfg2(base):
    """cfg2 (n = 275), 64 instances, NodeLimit 50.  MLD_DBG_KEEP_DEAD_ROWS leaves no original row to skip: both walks then cover the same rows"""
    _check(dw.medium("cfg2", 64), dict(max_nodes=50), "cfg2 base %d" % base, base=base)


def test_cfg2_without_cut_rounds():
    """cut_rounds = 0: no cut rows, so no retired ones"""
    new, _ = _check(dw.medium("cfg2", 64), dict(max_nodes=50, cut_rounds=0), "cfg2 cut_rounds 0")
    assert int(new["stats"]["cuts"]) == 0


@pytest.mark.parametrize("max_nodes", (50, 800))
def test_cfg3(max_nodes):
    """cfg3 (n = 575, the benchmark's shape), 16 instances at NodeLimit 50 and 800: those of a batch of 64 on which the oracle makes the most nodes"""
    _, s = _check(dw.medium("cfg3", 64), dict(max_nodes=max_nodes), "cfg3 NodeLimit %d" % max_nodes, idx=np.asarray(dw.CFG3_HARD), deep=True, limited=max_nodes == 50)
    assert s["n"] == 575 and s["all_lds"]


def test_cfg3_multi_model():
    _check(dw.medium("cfg3", 4, 3), dict(max_nodes=30, max_pivots=3000), "cfg3 three models")


def test_cfg3_quadratic_cost():
    """cfg3 MIQP, 8 instances: the primal simplex ratio-tests every live row"""
    _check(dw.medium("cfg3", 8, 1, True), dict(max_nodes=10, max_pivots=3000), "cfg3 MIQP", limited=True)


def test_phase_clocks_are_still_reported():
    """mld_debug_profile after a plain solve (what bench.py --full and scripts/gpu_*_prof.py read): the pivot_update, simplex_select, set_bounds and
    setup slots are non-zero and together stay below the summed in-kernel latency (wall_clock64 ticks of 10 ns; the four cover disjoint stretches of
    thread 0's time)"""
    pool = dw.medium("cfg3", 64)
    h = pool.handle(max_nodes=50)
    try:
        out = h.run(np.asarray(dw.CFG3_HARD))
        prof = (C.c_int64 * 8)()
        _lib.check(_lib.load().mld_debug_profile(h.prob._h, prof))
        lat_ns = int(h.prob.telemetry()["latency_ns"].sum())
    finally:
        h.close()
    ticks = dict(zip(("pivot_update", "simplex_select", "cuts", "leaf", "set_bounds", "residual/refactor", "setup"), [int(prof[k]) for k in range(7)]))
    print("clocks", ticks, "summed latency [ticks]", lat_ns // 10, "nodes", int(out["nodes"].sum()))
    for k in ("pivot_update", "simplex_select", "set_bounds", "setup"):
        assert ticks[k] > 0, (k, ticks)
    assert sum(ticks[k] for k in ("pivot_update", "simplex_select", "set_bounds", "setup")) * 10 < lat_ns, (ticks, lat_ns)
