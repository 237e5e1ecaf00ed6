"""The hard-row families of tests/_hard.py on the CPU: the class counts that keep tests/test_gpu_hard_rows.py from going hollow -- conditions, so that a
change to _paths.fuzz_mld that empties a class fails here instead of quietly shrinking the GPU tests -- and the C oracle (the restatement of the
kernel's algorithm) against scipy's HiGHS on every classified instance, with its presolve on and off."""
import numpy as np
import pytest

import _hard
import orc

NODES, PIVOTS = 50000, 400000


def _refs(family):
    return [_hard.reference("T3")] if family == "T3" else [_hard.reference(family, s) for s in _hard.SEEDS]


@pytest.mark.parametrize("family, min_feasible, min_infeasible", [("F5", 40, 10), ("F8", 40, 10), ("T3", 8, 8)])
def test_class_counts_keep_the_gpu_tests_from_going_hollow(family, min_feasible, min_infeasible):
    refs = _refs(family)
    feas, infeas, dropped = _hard.counts(refs)
    print("%s: %d feasible, %d infeasible, %d dropped" % (family, feas, infeas, dropped))
    assert dropped <= _hard.MAX_DROPPED * (feas + infeas + dropped), (family, dropped)
    assert feas >= min_feasible and infeas >= min_infeasible, (family, feas, infeas)


@pytest.mark.parametrize("presolve", [0, 1])
@pytest.mark.parametrize("family", ["F5", "F8", "T3"])
def test_oracle_agrees_with_highs(family, presolve):
    """status as classified, objective inside the sandwich lo - 1e-6 s <= obj <= opt + 1e-6 s; no budget reached"""
    worst, branched, searched = 0.0, 0, 0
    for seed, ref in enumerate(_refs(family)):
        t = ref["tight"]
        for s, c in enumerate(ref["inst"]):
            if c["cls"] == "dropped":
                continue
            o = orc.solve_milp(c["qt"], t["G"], c["ht"], t["lb"], t["ub"], t["is_bin"], max_nodes=NODES, max_pivots=PIVOTS, presolve=presolve)
            if c["cls"] == "infeasible":
                assert o["status"] == "infeasible" and o["x"] is None, (family, seed, s, o["status"], o["obj"])
                searched += o["nodes"] > 1
                continue
            assert o["status"] == "optimal", (family, seed, s, o["status"], o["nodes"], o["pivots"])
            ok, rel = _hard.sandwich(c, o["obj"] + c["r"])
            assert ok, (family, seed, s, o["obj"], c["opt"], c["lo"])
            worst = max(worst, abs(rel))
            branched += o["nodes"] > 1
    print("%s presolve %d: worst |obj - opt| / s %.2e, %d feasible instances branch, %d infeasible ones are proven by the search" %
          (family, presolve, worst, branched, searched))


def test_presolve_off_proves_infeasibility_in_the_search_on_the_seeds_the_gpu_test_names():
    """the premise of the MLD_DBG_NO_PRESOLVE mode of tests/test_gpu_hard_rows.py: without its presolve the oracle needs more than one node on at
    least one infeasible instance of the chosen F5 seeds"""
    n = 0
    for seed in _hard.F5_ROUTE_SEEDS:
        ref = _hard.reference("F5", seed)
        t = ref["tight"]
        for c in ref["inst"]:
            if c["cls"] == "infeasible":
                o = orc.solve_milp(c["qt"], t["G"], c["ht"], t["lb"], t["ub"], t["is_bin"], max_nodes=NODES, max_pivots=PIVOTS, presolve=0)
                n += o["status"] == "infeasible" and o["nodes"] > 1
    assert n >= 1
