"""The solvers on models with HARD rows, where an instance can be truly infeasible, against scipy's HiGHS on the ORIGINAL rows.

Every other comparison with an independent solver in this suite (tests/test_gpu_fuzz.py, the bench shards) uses models whose every row has a slack: no
instance is ever infeasible there, and a cut, a presolve fixing, a tightened big-M or a ratio-test decision that wrongly removes part of the feasible
set still leaves a point to return.  Here the families of tests/_hard.py (F5, F8: the fuzz models with the slack taken off most / half of the rows; T3:
three tanks with hard comfort bounds) are classified by HiGHS with a margin of 1e-3 of the row scale (instances on the feasibility boundary are dropped:
they stay in the batch and nothing is asserted on them), and per classified instance

* infeasible: status 1, objective +inf (no plan);
* feasible:   status 0, lo + r - 1e-6 s <= obj <= opt + r + 1e-6 s (opt = HiGHS at h, lo = HiGHS at h + 1e-6 rs, r the cost constant,
              s = max(1, |opt + r|)), every binary exactly 0 or 1, G v - h <= 1e-6 rs on the original rows, the hard ones included.

Both bounds of the sandwich come from the reference and from the residual tolerance tests/test_gpu_fuzz.py asserts, none from the kernel.  Every handle
has finite budgets (50000 nodes, 400000 pivots); NODE_LIMIT or NUMERICAL on a classified instance fails.  tests/test_hard_refs.py holds the class
counts and the oracle's agreement on the CPU.

Seeds named here (HiGHS classes of tests/_hard.py): F5 has infeasible instances at seeds 1 (all six), 4, 9, 11; F8 at seeds 1, 9, 11.
"""
import numpy as np
import pytest

import _hard
from pyhybridcontrol_amd import _lib, gpu, host

pytestmark = pytest.mark.gpu

NODES, PIVOTS = 50000, 400000
NO_LP_LDS, LP_LDS_K24 = 1 << 8, 1 << 9
NO_PRESOLVE, FIRST_FRACTIONAL, LAZY_START, NO_SWEEP = 1 << 12, 1 << 6, 1 << 17, 1 << 19
NO_PIVOT_PAIRS, PIVOT_SYNC_R5, SELECT_R6 = 1 << 21, 1 << 26, 1 << 27

F5_ROUTE_SEEDS = _hard.F5_ROUTE_SEEDS      # (1, 4, 9, 11, 0, 2): the four F5 seeds with infeasible instances and two without
F5_START_SEEDS = (4, 9)                    # mixed outcomes: three infeasible instances of six each
F8_HANDOFF_SEEDS = (1, 9, 11)              # the F8 seeds with infeasible instances
LP_FIX_SEED = 1                            # binaries fixed from default_rng([1, seed]): HiGHS alone finds 31 of the 72 LPs infeasible, 41 feasible, none dropped
SMALL_N, SMALL_XS = 2, 1.5                 # F5's models at N_tilde = 2 with the family's own x0 scale: HiGHS finds 63 feasible, 9 infeasible, none dropped


def _solve(ref, cost_atoms=None, warm_start=None, fixed_bin=None, handoff=None, **opts):
    d = ref["dims"]
    o = dict(max_nodes=NODES, max_pivots=PIVOTS)
    o.update(opts)
    m = gpu.GpuModel([ref["mats"]], d)
    p = gpu.GpuProblem(m, ref["N_p"], ref["N"], host.cost_from_atoms(cost_atoms or ref["atoms"], d, ref["N_p"], ref["N"]), **o)
    try:
        if handoff:
            out = p.solve_handoff_device(ref["x0"], ref["om"], fixed_bin=fixed_bin, **handoff)
        else:
            out = p.solve(ref["x0"], ref["om"], fixed_bin=fixed_bin, warm_start=warm_start)
        out["small"] = p.small_lds_stats()
    finally:
        p.close(); m.close()
    return out


def _check(ref, out, tag, inst=None, stats=True):
    """the contract of the module docstring on every classified instance; returns the worst |obj - opt - r| / s of the feasible ones"""
    raw, rs = ref["raw"], ref["rs"]
    bins = raw["is_bin"]
    inst = ref["inst"] if inst is None else inst
    worst, n_feas, n_inf = 0.0, 0, 0
    for s, c in enumerate(inst):
        st, obj = int(out["status"][s]), float(out["obj"][s])
        what = (tag, s, c["cls"], st, obj, int(out["nodes"][s]), int(out["pivots"][s]))
        if c["cls"] == "dropped":
            continue
        if c["cls"] == "infeasible":
            n_inf += 1
            assert st == 1 and obj == np.inf, what
            continue
        n_feas += 1
        assert st == 0, what
        ok, rel = _hard.sandwich(c, obj)
        print("%s instance %d: obj %.12g  HiGHS %.12g  (obj - opt) / s %.2e" % (tag, s, obj, c["opt"] + c["r"], rel))
        assert ok, what + (c["lo"] + c["r"], c["opt"] + c["r"])
        worst = max(worst, abs(rel))
        v = out["v"][s]
        assert np.all((v[bins] == 0) | (v[bins] == 1)), what
        assert np.all(raw["G"] @ v - c["h"] <= _hard.RESID * rs), what + (float(((raw["G"] @ v - c["h"]) / rs).max()),)
    if stats:      # (the counts of the downloaded statuses: with every classified instance held to its class above, the class counts)
        got = out["stats"]
        assert got["n_infeasible"] == int((out["status"] == 1).sum()) and got["n_optimal"] == int((out["status"] == 0).sum()), (tag, got, out["status"])
        if not any(c["cls"] == "dropped" for c in inst):
            assert got["n_infeasible"] == n_inf and got["n_optimal"] == n_feas, (tag, got, n_feas, n_inf)
    print("%s: %d feasible, %d infeasible, worst |obj - opt| / s %.2e" % (tag, n_feas, n_inf, worst))
    return worst


_base = {}


def _default(family, seed=0):
    """item 1's result of one (family, seed), solved once and shared with the modes that compare against it"""
    if (family, seed) not in _base:
        _base[(family, seed)] = _solve(_hard.reference(family, seed))
    return _base[(family, seed)]


# ---- 1. parity, default options -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", _hard.SEEDS)
@pytest.mark.parametrize("family", ["F5", "F8"])
def test_parity_with_highs_default_options(family, seed):
    _check(_hard.reference(family, seed), _default(family, seed), "%s seed %d" % (family, seed))


def test_parity_with_highs_three_tanks_with_hard_comfort_bounds():
    ref = _hard.reference("T3")
    assert len(ref["inst"]) == 24 and ref["raw"]["G"].shape[1] == 18
    _check(ref, _default("T3"), "T3")


# ---- 2. the same contract under each route that decides feasibility differently ---------------------------------------------------------------
def test_without_presolve_infeasibility_comes_from_the_lp_and_the_search():
    """MLD_DBG_NO_PRESOLVE: nothing is caught before the first pivot.  The oracle with presolve = 0 needs 55, 27 and 22 nodes on instances 2, 3, 4 of
    seed 1 and 6 on instances 3, 5 of seed 4 (tests/test_hard_refs.py asserts that premise); here at least one infeasible instance takes more than one."""
    searched = 0
    for seed in F5_ROUTE_SEEDS:
        ref = _hard.reference("F5", seed)
        out = _solve(ref, reserved=NO_PRESOLVE)
        _check(ref, out, "F5 seed %d no presolve" % seed)
        searched += sum(1 for s, c in enumerate(ref["inst"]) if c["cls"] == "infeasible" and out["nodes"][s] > 1)
    print("infeasible instances proven by the search: %d" % searched)
    assert searched >= 1


@pytest.mark.parametrize("seed", F5_ROUTE_SEEDS)
def test_without_cuts_the_answers_are_the_same(seed):
    """cut_rounds = 0 against the default: equal statuses, both objectives inside the sandwich -- an invalid cut on a row without a slack would show as
    a status 1 or a worse optimum under the default options"""
    ref = _hard.reference("F5", seed)
    base, out = _default("F5", seed), _solve(ref, cut_rounds=0)
    _check(ref, base, "F5 seed %d default" % seed)
    _check(ref, out, "F5 seed %d no cuts" % seed)
    assert np.array_equal(out["status"], base["status"]), (seed, out["status"], base["status"])


@pytest.mark.parametrize("seed", F5_ROUTE_SEEDS)
def test_earlier_pivot_loop_and_selection_give_the_same_bits(seed):
    """MLD_DBG_NO_PIVOT_PAIRS | MLD_DBG_PIVOT_SYNC_R5 | MLD_DBG_SELECT_R6: the infeasible exit of the rewritten pivot loop and selection"""
    ref = _hard.reference("F5", seed)
    base, out = _default("F5", seed), _solve(ref, reserved=NO_PIVOT_PAIRS | PIVOT_SYNC_R5 | SELECT_R6)
    _check(ref, out, "F5 seed %d earlier pivot loop" % seed)
    assert np.array_equal(out["status"], base["status"]) and np.array_equal(out["nodes"], base["nodes"]), (seed, out["status"], base["status"], out["nodes"], base["nodes"])
    assert np.array_equal(out["obj"].view(np.uint64), base["obj"].view(np.uint64)), (seed, out["obj"], base["obj"])


@pytest.mark.parametrize("seed", F5_ROUTE_SEEDS)
def test_first_fractional_branching(seed):
    ref = _hard.reference("F5", seed)
    _check(ref, _solve(ref, reserved=FIRST_FRACTIONAL), "F5 seed %d first fractional" % seed)


# ---- 3. LPs -----------------------------------------------------------------------------------------------------------------------------------
_lp = {}


def _lp_cases(seed):
    """(fixed binaries (6, n_bin), per instance the class of the LP by scipy's linprog with the margin guard) of one F8 seed, computed once"""
    if seed not in _lp:
        ref = _hard.reference("F8", seed)
        raw = ref["raw"]
        bins = np.where(raw["is_bin"])[0]
        fixed = (np.random.default_rng([LP_FIX_SEED, seed]).random((_hard.NB, len(bins))) < 0.5).astype(np.uint8)
        inst = []
        for s, c in enumerate(ref["inst"]):
            lb, ub = raw["lb"].copy(), raw["ub"].copy()
            lb[bins] = ub[bins] = fixed[s]
            k = _hard.classify_lp(raw, c["h"], c["q"], lb, ub)
            k.update(h=c["h"], r=c["r"])
            inst.append(k)
        _lp[seed] = (fixed, inst)
    return _lp[seed]


@pytest.mark.parametrize("seed", _hard.SEEDS)
def test_relaxations_with_hard_rows_on_the_lp_kernels(seed):
    """F8's models with every binary fixed at a seeded random value: k_lp_lds, the dense-dictionary kernel (MLD_DBG_NO_LP_LDS) and k_lp_lds with a
    working basis of 24 (MLD_DBG_LP_LDS_K24) against scipy's linprog with the same margin guard"""
    ref = _hard.reference("F8", seed)
    fixed, inst = _lp_cases(seed)
    for name, reserved in (("k_lp_lds", 0), ("dense", NO_LP_LDS), ("k_lp_lds K24", LP_LDS_K24)):
        _check(ref, _solve(ref, fixed_bin=fixed, reserved=reserved), "F8 seed %d LP %s" % (seed, name), inst=inst)


def test_the_lp_set_holds_infeasible_lps():
    """a condition on the reference alone: at least 10 of the 72 LPs are infeasible for HiGHS beyond the margin"""
    n = sum(k["cls"] == "infeasible" for seed in _hard.SEEDS for k in _lp_cases(seed)[1])
    print("infeasible LPs: %d" % n)
    assert n >= 10


# ---- 4. MIP start -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reserved", [0, LAZY_START], ids=["eager", "lazy"])
@pytest.mark.parametrize("seed", F5_START_SEEDS)
def test_mip_starts_that_violate_hard_rows_and_starts_that_are_optimal(seed, reserved):
    ref = _hard.reference("F5", seed)
    raw = ref["raw"]
    bins = np.where(raw["is_bin"])[0]
    violated = 0
    for val in (0, 1):      # (a) all-zero and all-one binaries
        start = np.full((_hard.NB, len(bins)), val, np.uint8)
        for c in ref["inst"]:
            if c["cls"] == "feasible":
                lb, ub = raw["lb"].copy(), raw["ub"].copy()
                lb[bins] = ub[bins] = float(val)
                violated += _hard.classify_lp(raw, c["h"], c["q"], lb, ub)["cls"] == "infeasible"      # no completion of the start within 1e-3 rs of the rows
        _check(ref, _solve(ref, warm_start=start, reserved=reserved), "F5 seed %d start all %d" % (seed, val))
    assert violated >= 1, "premise: a start that violates a hard row by more than 1e-3 rs on a feasible instance"
    start = np.full((_hard.NB, len(bins)), 255, np.uint8)      # (b) HiGHS's optimal binaries where there is an optimum; no start elsewhere
    for s, c in enumerate(ref["inst"]):
        if c["cls"] == "feasible":
            start[s] = np.rint(c["x"][bins]).astype(np.uint8)
    _check(ref, _solve(ref, warm_start=start, reserved=reserved), "F5 seed %d start at the optimum" % seed)


# ---- 5. in-kernel hand-off --------------------------------------------------------------------------------------------------------------------
HANDOFF = dict(first_nodes=2, sub_nodes=32, max_gen=8, max_children=64, max_tree=100000, room_factor=64.0)


@pytest.mark.parametrize("seed", F8_HANDOFF_SEEDS)
def test_in_kernel_handoff_on_hard_rows(seed):
    """F8 with a first node limit of 2: the feasible instances that branch split into items and end status 0 inside the sandwich.  F8's infeasible
    instances are all closed at the root (presolve, or the first LP without it), so none of them splits here: they are held to status 1 alone (and see
    the next test)."""
    ref = _hard.reference("F8", seed)
    out = _solve(ref, handoff=HANDOFF)
    print("F8 seed %d hand-off: %s" % (seed, out["handoff"]))
    assert out["handoff"]["items"] > 0 and out["handoff"]["unfinished"] == 0 and out["handoff"]["given_up"] == 0, out["handoff"]
    _check(ref, out, "F8 seed %d hand-off" % seed, stats=False)


def test_in_kernel_handoff_when_infeasibility_is_proven_by_the_search():
    """F5 seed 1 without presolve: every instance is infeasible and three are proven only by the search (55, 27 and 22 nodes in the oracle; 25, 21
    and 21 on the device).  Held to the statuses alone: no such tree splits at any first node limit >= 2, with or without the closing sweep
    (MLD_DBG_NO_SWEEP) -- a search without an incumbent is given at least 16 nodes of deepening passes and then a rescue dive of 3 n_bin + 10 nodes
    whatever the limit (s_next_phase), and these trees close inside that.  The merge of a tree whose every ITEM closes without a point is therefore
    not reached by this family."""
    ref = _hard.reference("F5", 1)
    assert all(c["cls"] == "infeasible" for c in ref["inst"])
    for name, reserved in (("", NO_PRESOLVE), (" and sweep", NO_PRESOLVE | NO_SWEEP)):
        out = _solve(ref, handoff=HANDOFF, reserved=reserved)
        print("F5 seed 1 hand-off without presolve%s: %s nodes %s" % (name, out["handoff"], out["nodes"].tolist()))
        assert out["handoff"]["unfinished"] == 0 and out["handoff"]["given_up"] == 0, out["handoff"]
        assert np.any(out["nodes"] > HANDOFF["first_nodes"])
        _check(ref, out, "F5 seed 1 hand-off without presolve%s" % name, stats=False)


# ---- 6. quadratic cost: NOT HERE ---------------------------------------------------------------------------------------------------------------
# Q_x = 1e-3 I on F5 seeds 1, 4, 7 (all infeasible, mixed, all feasible) against the C oracle's MIQP: seeds 1 and 4 pass (status as classified, optimum
# within 2e-6), but on all six instances of seed 7 kernel and oracle alike return UNBOUNDED (status 4, objective -inf; instance 0 after 34 nodes) where
# the problem is bounded: HiGHS's optimum under the linear cost is -4.18243672 on each, and a positive semidefinite term cannot take that bound away.
# The model has two free auxiliaries z whose direction in the null space of B3 costs nothing; the solver rests such variables on its artificial
# box of 1e7, which the linear path tells from a ray by the reduced cost (s_leaf_eval), while the quadratic path calls any free variable on the box
# unbounded.  Deciding it on the linearisation at the point is not enough (the simplicial decomposition does not converge among vertices of that
# size, and the objective loses digits: -4.18261 reported for a point worth -4.18242), so the mode waits for free variables that do not rest on
# the box under a quadratic cost.


# ---- 7. small-problem path --------------------------------------------------------------------------------------------------------------------
def test_small_problem_path_on_hard_rows():
    """F5's models at N_tilde = 2 (x0 scale 1.5) with MLD_SMALL_LDS: classified again at that horizon; every eligible model runs"""
    eligible, refs = [], []
    worst = 0.0
    for seed in _hard.SEEDS:
        ref = _hard.reference("F5", seed, N=SMALL_N, xs=SMALL_XS)
        out = _solve(ref, flags=_lib.MLD_SMALL_LDS)
        st = out["small"]
        if not st["eligible"]:
            continue
        eligible.append(seed); refs.append(ref)
        assert st["lds"] + st["dense"] == _hard.NB, (seed, st)
        worst = max(worst, _check(ref, out, "F5 seed %d N_tilde 2 small path %s" % (seed, st)))
    feas, infeas, dropped = _hard.counts(refs)
    print("small path: eligible seeds %s, %d feasible, %d infeasible, %d dropped, worst %.2e" % (eligible, feas, infeas, dropped, worst))
    assert len(eligible) >= 4, eligible
    assert infeas >= 4 and feas >= 20, (feas, infeas)
