"""A solve's bits do not depend on what its workgroup ran before ("a solve is bit-reproducible whatever slot, batch position or
launch it runs in").

k_solve is a persistent workgroup: it takes entries off a queue and solves one after another in the same Shared struct, the same LDS and the same
workspace slot, and what the next entry needs fresh is reset by hand (s_setup_entry).  A field that is not reset changes the next answer only after
SOME predecessors, and every A/B test of the suite compares two code paths on the same batch in the same order, where both sides inherit the same stale
state.  Here the predecessor is what varies:

* every instance is solved ALONE (a batch of one) -- one instance per kind on a fresh handle, all of them on one reused reference handle, and the two
  must agree: that is the reference;
* the instances are labelled with KINDS (how the single solve ended: proven at the root, after branching, infeasible, at the node or the pivot limit;
  which model; which per-instance inputs) and uploaded as a chain in which every ordered pair of kinds is a pair of neighbours
  (tests/_history.py: an Eulerian circuit), on a handle with ONE slot and the queue in upload order (MLD_DBG_NO_ORDER), so that kind a runs directly
  before kind b in the same workgroup for all a, b; again with two and three slots, where timing decides the predecessor, and once reversed;
* every position of every chain must equal its single solve BIT FOR BIT (objective, plan, lower bound, status, nodes, pivots, rows_updated; cuts and
  refactors as totals).  No tolerance anywhere in these comparisons.
* so that "chain and single solve agree" cannot mean "both wrong", the chains on the pool P35 with generous limits are also held to HiGHS on the
  original rows (the margin guard and the sandwich of tests/_hard.py).

Every test asserts that the kinds it claims to chain are PRESENT before it compares anything.  The medium shapes (cfg2, cfg3, cfg3 multi-model, cfg3
MIQP, cfg3 in the legacy instantiation of the loop) are those whose LDS placement and pivot pairs the hot path runs; then three launches on one handle
(cut rows, counters and the learnt queue order of another batch size left in the workspace), the in-kernel hand-off under three slot counts and two
upload orders, and k_lp_lds.  k_small_milp, k_rollout, time_limit and multi-rank gathers are not here (they have their own tests or are
timing-dependent by design).

Recorded on an MI355X (kinds found, ordered pairs covered; every chain on 1, 2 and 3 slots and reversed; all equal to the single solves):

    P35 (a) default            10 kinds: root m0 m3 m5, tree m1 m2 m4 m5, infeasible m1 m2 m4                                   100 pairs
    P35 (b) no presolve        the same 10; the infeasible ones made 17 .. 1757 pivots                                          100 pairs
    P35 (c) max_nodes 3        11 kinds: node_limit m1 m2 m4 m5, root m0 m3 m5, tree m5, infeasible m1 m2 m4                     121 pairs
    P35 (d) max_pivots 71      9 kinds: pivot_limit m1 m2 m4 m5 (15 of the 29 feasible instances), root m0 m3 m5, infeasible     81 pairs
    P35 (e) inputs             17 kinds (variant, +lin, /inf)                                                                   289 pairs
    P35 (f) quadratic cost     10 kinds: root m0 m3, tree m1 .. m5, infeasible m1 m2 m4                                         100 pairs
    P35 LPs                    8 kinds (proven m0 m3 m5, infeasible m1 .. m5), batch 4160; none overflows under K24               64 pairs
    P35 LPs, N_tilde 12, K24   10 kinds: proven m0, proven+dense m5, infeasible m2 m3 m4, infeasible+dense m1 .. m5 (21 of 36
                               re-solved by the dense kernel), batch 4141                                                        100 pairs
    cfg2 x64                   3 kinds: root/long, root/short, tree/long                                                          9 pairs + the pool twice
    cfg3 x32, and legacy loop  3 kinds: node_limit/long, root/long, root/short                                                    9 pairs + the pool twice
    cfg3 x8 MIQP               4 kinds: node_limit/long, root/long, root/short, tree/short                                       16 pairs + the pool twice
    cfg3, 3 models x 4         5 kinds: root m0 m1 m2, tree m0 m1                                                                25 pairs + the pool twice

That the comparison can fail was tried on scratch builds with one reset of a plain value taken out of s_setup_entry:

* without `sh.since_check = 0` every chain still passed.  That is an observation on these pools, not an invariant: the infeasible, iteration-limit and
  cutoff exits leave the counter at any value, and a stale one moves the verification at 512 pivots and decides whether the one at the optimum runs;
  the bits change only if a moved or skipped check would have refactored, which no instance here does.
* without `sh.refactors = 0` seven of the ten tests tried failed, but in the REFERENCE, before any chain ("instance 0 alone on a fresh handle against
  the reused reference handle", 'refactors', 1 against 0; on cfg3 -1712303461 against 0): a launch starts on uninitialised LDS.
* without `sh.rows = 0ull`, and with the fresh-handle half of the reference skipped, all seven chains tried (b, d, cfg2, cfg3, legacy loop, MIQP,
  multi-model) failed in the chain comparison, at every position; e.g. "cfg3 x8 MIQP, 1 slot(s), upload order [1, 1, 4, 1]...: position 1
  (instance 1, kind 'node_limit/long', after instance 1 of kind 'node_limit/long') differs from its single solve in 'rows_updated': chain
  13215518, alone 6607759" -- the predecessor's count carried over, exactly twice the single solve's.

So a stale COUNTER is caught, in the chain, with the line that names the predecessor.  No mutation that changes an answer (objective, plan, status)
only after some predecessors was run: the one tried, leaving the skip marks of purged cut rows in place, alters a loop bound and was not made.
"""
import numpy as np
import pytest

import _hard
import _history as hist
from pyhybridcontrol_amd import gpu, host, synthetic as syn
from pyhybridcontrol_amd._lib import MLD_DBG_PIVOT_SYNC_R5, MLD_DBG_SELECT_R6, MLD_DBG_UPDATE_R7

pytestmark = pytest.mark.gpu

NO_ORDER, LP_LDS_K24, NO_PRESOLVE = 1 << 3, 1 << 9, 1 << 12
LEGACY = MLD_DBG_UPDATE_R7 | MLD_DBG_SELECT_R6 | MLD_DBG_PIVOT_SYNC_R5
GENEROUS = dict(max_nodes=50000, max_pivots=400000)          # (the budgets of tests/test_gpu_hard_rows.py)
STATUS = {0: "proven", 1: "infeasible", 2: "node_limit", 3: "numerical", 4: "unbounded"}


class Pool(object):
    """instances that share one handle layout: models, cost, inputs, and optional per-instance arrays (fixed, warm, cutoff, lin_v: one row per instance)"""

    def __init__(self, name, mats_list, dims, cost, N_p, N, x0, om, midx=None, fixed=None, warm=None, cutoff=None, lin_v=None):
        self.name, self.mats_list, self.dims, self.cost, self.N_p, self.N = name, mats_list, dims, cost, N_p, N
        self.x0, self.om, self.midx, self.fixed, self.warm, self.cutoff, self.lin_v = x0, om, midx, fixed, warm, cutoff, lin_v
        self.size = len(x0)

    def handle(self, after=None, **opts):
        return Handle(self, after, opts)


class Handle(object):
    def __init__(self, pool, after, opts):
        self.pool = pool
        self.model = gpu.GpuModel(pool.mats_list, pool.dims)
        self.prob = gpu.GpuProblem(self.model, pool.N_p, pool.N, pool.cost, **opts)
        if after:
            self.prob.set_opts(**after)

    def run(self, idx, handoff=None):
        """the instances idx of the pool as one batch, in that order: results, rows_updated and the launch's statistics"""
        P, p = self.pool, self.prob
        idx = np.atleast_1d(np.asarray(idx, np.int64))
        pick = lambda a: None if a is None else np.ascontiguousarray(a[idx])
        if handoff:
            return p.solve_handoff_device(P.x0[idx], P.om[idx], pick(P.midx), pick(P.fixed), **handoff)
        p.upload(P.x0[idx], P.om[idx], pick(P.midx), pick(P.fixed))
        if P.lin_v is not None:
            p.upload_instance_cost(lin_v=pick(P.lin_v))
        p.set_warm_start(pick(P.warm))
        p.set_cutoffs(pick(P.cutoff))
        stats = p.solve_resident()
        out = p.download()
        out["rows_updated"] = p.telemetry()["rows_updated"].copy()
        out["stats"] = stats
        return out

    def close(self):
        self.prob.close()
        self.model.close()


# ---- the reference: every instance alone ------------------------------------------------------------------------------------------------------------
_alone_cache = {}


def _key(opts, after):
    return (tuple(sorted(opts.items())), tuple(sorted((after or {}).items())))


def _alone(pool, opts, kinds_fn, after=None):
    """the single solves of every instance of the pool under `opts` (then set_opts(**after)), computed once per (pool, options): arrays with one row per
    instance, per-instance cuts / refactors, and kinds = kinds_fn(those arrays).  All on one reused handle; the first instance of every kind once more on
    a fresh handle, which must return the same bits (the reference itself does not depend on the launch or the handle)."""
    key = (pool.name,) + _key(opts, after)
    if key in _alone_cache:
        return _alone_cache[key]
    ref = pool.handle(after, **opts)
    try:
        rows = [ref.run([i]) for i in range(pool.size)]
    finally:
        ref.close()
    alone = {k: np.concatenate([r[k] for r in rows]) for k in hist.KEYS}
    alone["cuts"] = np.array([r["stats"]["cuts"] for r in rows], np.int64)
    alone["refactors"] = np.array([r["stats"]["refactors"] for r in rows], np.int64)
    kinds = alone["kinds"] = kinds_fn(alone)
    firsts = [kinds.index(lab) for lab in sorted(set(kinds), key=repr)]
    for i in firsts:
        fresh = pool.handle(after, **opts)
        try:
            one = fresh.run([i])
        finally:
            fresh.close()
        one["stats"] = dict(one["stats"])
        hist.assert_same_bits(one, alone, [i], "%s %s: instance %d alone on a fresh handle against the reused reference handle" % (pool.name, opts, i), kinds=kinds)
    _alone_cache[key] = alone
    return alone


def _ending(alone, i):
    st = int(alone["status"][i])
    if st == 0:
        return "root" if alone["nodes"][i] <= 1 else "tree"
    return STATUS[st]


def _need(kinds, *endings):
    """every ending named begins the first part of a kind that is present"""
    have = set(k.split("/")[0] for k in kinds)
    for e in endings:
        assert any(h.startswith(e) for h in have), ("a kind this chain claims is missing", e, sorted(have))


def _chains(pool, opts, alone, tag, expect=None, slots=(1, 2, 3), after=None, whole_pool=False):
    """the all-pairs chain over alone["kinds"] on one slot in upload order, on two and three slots, and reversed on one slot: every position equals its
    single solve bit for bit (and HiGHS's verdict where `expect` is given).  whole_pool: also every instance once on one slot, in the pool's order and
    in a seeded permutation (the neighbours the kinds do not tell apart).  Returns (kinds, pairs)."""
    kinds = alone["kinds"]
    order, labels = hist.chain(kinds)
    pairs = hist.assert_all_pairs(order, kinds)
    assert pairs == len(labels) ** 2 and len(order) == pairs + 1
    print("%s: %d kinds %s, %d ordered pairs, chain of %d" % (tag, len(labels), labels, pairs, len(order)))
    runs = [(n, order) for n in slots] + [(1, order[::-1].copy())]
    if whole_pool:
        runs += [(1, np.arange(pool.size)), (1, np.random.default_rng(pool.size).permutation(pool.size))]
    for n_slots, o in runs:
        h = pool.handle(after, n_slots=n_slots, **dict(opts, reserved=opts.get("reserved", 0) | NO_ORDER))
        try:
            assert h.prob.debug_shape()["n_slots"] == n_slots
            out = h.run(o)
        finally:
            h.close()
        name = "%s, %d slot(s), upload order %s..." % (tag, n_slots, o[:4].tolist())
        hist.assert_same_bits(out, alone, o, name, kinds=kinds)
        if expect is not None:
            print("%s: HiGHS agrees on %d feasible and %d infeasible positions" % ((name,) + hist.assert_anchor(out, o, expect, name)))
    return labels, pairs


# ---- P35 ------------------------------------------------------------------------------------------------------------------------------------------
_pools = {}


def _p35(variant="plain", N=hist.P35_N):
    if ("p35", variant, N) in _pools:
        return _pools[("p35", variant, N)]
    P = hist.p35(N)
    d = P["dims"]
    costs = []
    for m in P["models"]:
        atoms = dict(m["atoms"])
        if variant == "quadratic":
            atoms["Q_u"] = 0.05 * np.eye(d["nu"])          # (the small case of tests/test_gpu_miqp.py)
        costs.append(host.cost_from_atoms(atoms, d, P["N_p"], P["N"]))
    extra = {}
    if variant == "inputs":
        inp = hist.p35_inputs()
        extra = {k: inp[k] for k in ("fixed", "warm", "cutoff", "lin_v")}
    if variant == "lp":
        extra = dict(fixed=hist.p35_lp_fixings(N=N)[0])
    pool = Pool("P35 %s%s" % (variant, "" if N == hist.P35_N else " N_tilde %d" % N), [m["mats"] for m in P["models"]], d, host.stack_costs(costs), P["N_p"], P["N"], P["x0"], P["om"], midx=P["midx"], **extra)
    _pools[("p35", variant, N)] = pool
    return pool


def _by_ending_and_model(alone):
    midx = hist.p35()["midx"]
    return ["%s/m%d" % (_ending(alone, i), midx[i]) for i in range(len(midx))]


def _other_model_before_each_ending(alone, order):
    """for each ending, a position whose predecessor belongs to another model (the all-pairs chain over (ending, model) kinds has one by construction)"""
    midx, kinds = hist.p35()["midx"], alone["kinds"]
    seen = set(kinds[order[p]].split("/")[0] for p in range(1, len(order)) if midx[order[p]] != midx[order[p - 1]])
    assert seen == set(k.split("/")[0] for k in kinds), (sorted(seen), sorted(set(kinds)))


def test_p35_default_options():
    """(a) proven at the root, proven after branching, infeasible (here: found by the presolve, no dictionary was set up), each after every other and
    after another model's"""
    pool, opts = _p35(), dict(GENEROUS)
    alone = _alone(pool, opts, _by_ending_and_model)
    _need(alone["kinds"], "root", "tree", "infeasible")
    _other_model_before_each_ending(alone, hist.chain(alone["kinds"])[0])
    _chains(pool, opts, alone, "P35 (a) default", expect=hist.p35()["inst"])


def test_p35_without_presolve_the_infeasible_ones_leave_a_pivoted_dictionary():
    """(b) MLD_DBG_NO_PRESOLVE: infeasibility comes from the LP or the search, so the successor inherits a pivoted dictionary, cut rows and a stack"""
    pool, opts = _p35(), dict(GENEROUS, reserved=NO_PRESOLVE)
    alone = _alone(pool, opts, _by_ending_and_model)
    _need(alone["kinds"], "root", "tree", "infeasible")
    inf = alone["status"] == 1
    print("P35 (b): pivots of the infeasible instances %s" % alone["pivots"][inf].tolist())
    assert np.any(alone["pivots"][inf] > 0)
    _other_model_before_each_ending(alone, hist.chain(alone["kinds"])[0])
    _chains(pool, opts, alone, "P35 (b) no presolve", expect=hist.p35()["inst"])


def test_p35_node_limit_of_three():
    """(c) max_nodes = 3: searches that stop with a stack and cut rows in place next to proven ones"""
    pool, opts = _p35(), dict(GENEROUS, max_nodes=3)
    alone = _alone(pool, opts, _by_ending_and_model)
    _need(alone["kinds"], "node_limit")
    assert any(k.split("/")[0] in ("root", "tree") for k in alone["kinds"]), sorted(set(alone["kinds"]))
    _chains(pool, opts, alone, "P35 (c) max_nodes 3")


def _pivot_limit():
    """the median of the pivots the feasible instances need under generous limits (from the single solves of chain (a), never a constant)"""
    base = _alone(_p35(), dict(GENEROUS), _by_ending_and_model)
    feas = np.array([c["cls"] == "feasible" for c in hist.p35()["inst"]])
    return max(1, int(np.median(base["pivots"][feas]))), feas


def test_p35_pivot_limit_in_the_middle_of_an_lp():
    """(d) max_pivots = the median need of the feasible instances: between a quarter and three quarters of them stop at it, at least one in the middle
    of an LP (exactly max_pivots pivots made, not proven)"""
    cap, feas = _pivot_limit()
    pool, opts = _p35(), dict(GENEROUS, max_pivots=cap)

    def kinds_fn(alone):
        midx = hist.p35()["midx"]
        return ["%s/m%d" % ("pivot_limit" if alone["pivots"][i] >= cap else _ending(alone, i), midx[i]) for i in range(len(midx))]
    alone = _alone(pool, opts, kinds_fn)
    stopped = alone["pivots"] >= cap
    print("P35 (d): max_pivots %d, %d of %d feasible instances stop at it; statuses there %s" % (
        cap, int(stopped[feas].sum()), int(feas.sum()), np.bincount(alone["status"][stopped].astype(np.int64)).tolist()))
    assert 0.25 * feas.sum() <= stopped[feas].sum() <= 0.75 * feas.sum(), (cap, int(stopped[feas].sum()), int(feas.sum()))
    assert np.any((alone["pivots"] == cap) & (alone["status"] != 0)), "an ending at the iteration limit in the middle of an LP"
    _need(alone["kinds"], "pivot_limit")
    assert any(k.split("/")[0] in ("root", "tree") for k in alone["kinds"]), sorted(set(alone["kinds"]))
    _chains(pool, opts, alone, "P35 (d) max_pivots %d" % cap)


def test_p35_per_instance_inputs():
    """(e) MIP starts (own optimum, one that violates a hard row, none), partial and contradicting fixings, cutoffs just above and below the optimum,
    a per-instance linear cost on half of the instances -- the kinds are the combinations present (tests/_history.p35_inputs: the variant, "+lin"
    with a cost row, "/inf" on an instance of the pool that is infeasible)"""
    inp = hist.p35_inputs()
    pool, opts = _p35("inputs"), dict(GENEROUS)
    alone = _alone(pool, opts, lambda a: list(inp["kind"]))
    present = set(inp["variant"])
    assert present >= set(hist.FEASIBLE_VARIANTS), present
    assert inp["violated"].any() and any("+lin" in k for k in inp["kind"]) and any("+lin" not in k for k in inp["kind"])
    _chains(pool, opts, alone, "P35 (e) per-instance inputs", expect=inp["expect"])


def _quadratic_expect(pool):
    """HiGHS on (f): Q_u weighs binaries only and is diagonal, and u'Wu = sum W_kk u_k on binaries, so the MIQP is the MILP with diag(W) added to the
    linear cost (asserted on the cost the handle gets); the infeasible instances keep their class, which no cost changes"""
    P = hist.p35()
    expect = []
    for c in P["inst"]:
        m = P["models"][c["model"]]
        W = np.asarray(pool.cost["quad_v"][c["model"]]).reshape(len(c["q"]), len(c["q"]))
        w = np.diag(W)
        assert not (W - np.diag(w)).any() and not w[~m["raw"]["is_bin"].astype(bool)].any() and w.any()
        e = dict(c) if c["cls"] != "feasible" else _hard.classify(m["raw"], c["h"], c["q"] + w)
        e["r"] = c["r"]
        expect.append(e)
    return expect


def test_p35_quadratic_cost():
    """(f) Q_u = 0.05 I: the QP relaxation's vertex set and the primal simplex's state are what the predecessor leaves behind"""
    pool, opts = _p35("quadratic"), dict(GENEROUS)
    alone = _alone(pool, opts, _by_ending_and_model)
    print("P35 (f): statuses %s" % np.bincount(alone["status"].astype(np.int64)).tolist())
    _need(alone["kinds"], "root", "tree", "infeasible")
    _other_model_before_each_ending(alone, hist.chain(alone["kinds"])[0])
    _chains(pool, opts, alone, "P35 (f) quadratic cost", expect=_quadratic_expect(pool))


def _launch_history(pool, opts, kinds_fn, tag, n_slots=2):
    """three launches on ONE handle: chain X with the default options, chain Y (other instances, another batch size) with cut_rounds = 0, chain X again
    -- and once more, now in the queue order learnt from the third launch.  X is the same bits every time and equal to its single solves; Y equals its
    own single solves (on a handle that went through the same set_opts)."""
    alone = _alone(pool, opts, kinds_fn)
    x, _ = hist.chain(alone["kinds"])
    h = pool.handle(n_slots=n_slots, **opts)
    try:
        default_rounds = int(h.prob.opts.cut_rounds)
        assert default_rounds > 0 and len(x) > n_slots
        no_cuts = _alone(pool, opts, kinds_fn, after=dict(cut_rounds=0))
        y, _ = hist.chain(no_cuts["kinds"], reverse=True)
        y = y[:-3] if len(y) - 3 != len(x) else y[:-4]
        first = h.run(x)
        h.prob.set_opts(cut_rounds=0)
        second = h.run(y)
        h.prob.set_opts(cut_rounds=default_rounds)
        third, fourth = h.run(x), h.run(x)
    finally:
        h.close()
    print("%s: X %d instances, cuts %d; Y %d instances, cuts %d" % (tag, len(x), first["stats"]["cuts"], len(y), second["stats"]["cuts"]))
    assert len(x) != len(y) and first["stats"]["cuts"] > 0 and second["stats"]["cuts"] == 0
    hist.assert_same_bits(first, alone, x, tag + ", launch 1", kinds=alone["kinds"])
    hist.assert_same_bits(second, no_cuts, y, tag + ", launch 2 (cut_rounds 0)", kinds=no_cuts["kinds"])
    hist.assert_same_bits(third, alone, x, tag + ", launch 3", kinds=alone["kinds"])
    hist.assert_same_bits(fourth, alone, x, tag + ", launch 4 (learnt order)", kinds=alone["kinds"])
    for k in hist.KEYS:
        assert np.array_equal(hist._bits(first[k]), hist._bits(third[k])), (tag, k)


def test_p35_launch_history_on_one_handle():
    _launch_history(_p35(), dict(GENEROUS), _by_ending_and_model, "P35 launch history")


# ---- k_lp_lds -------------------------------------------------------------------------------------------------------------------------------------
LP_TILE = 4096      # k_lp_lds's grid is min(batch, CUs of the device) and the handle does not report it: the batch the issue names for that case


@pytest.mark.parametrize("N,reserved", [(hist.P35_N, 0), (hist.P35_N, LP_LDS_K24), (12, LP_LDS_K24)], ids=["P35", "P35_K24", "P35_N12_K24"])
def test_relaxations_on_the_lp_kernel(N, reserved):
    """every binary fixed at seeded random values: k_lp_lds, whose workgroups also solve one LP after another.  No option sets its grid, so the
    all-pairs chain is tiled to LP_TILE LPs (they are tiny); every position equals its single solve and scipy's linprog agrees (the margin of
    _hard.classify_lp).  Under MLD_DBG_LP_LDS_K24 the working basis holds 24 columns and the LPs that outgrow it leave k_lp_lds early and are re-solved
    by the dense kernel.  None of P35's does (asserted: the kinds say which LPs were re-solved), so P35's models at N_tilde = 12 (n = 84, 72 rows)
    run under it too: there overflowing and fitting LPs, feasible and infeasible, of every model follow each other in a workgroup -- both kinds must be
    PRESENT among the single solves, and a fitting LP after an overflowing one is a pair of the chain."""
    fixed, inst = hist.p35_lp_fixings(N=N)
    assert sum(k["cls"] == "infeasible" for k in inst) >= 1 and sum(k["cls"] == "feasible" for k in inst) >= 1
    pool, opts = _p35("lp", N), dict(GENEROUS, reserved=reserved)
    midx = pool.midx

    def kinds_fn(alone):      # (rows_updated is zeroed by the LP path and counted by the dense kernel: > 0 marks a re-solved LP)
        return ["%s%s/m%d" % (STATUS[int(alone["status"][i])], "+dense" if alone["rows_updated"][i] > 0 else "", midx[i]) for i in range(pool.size)]
    alone = _alone(pool, opts, kinds_fn)
    kinds = alone["kinds"]
    assert alone["pivots"].sum() > 0
    dense = alone["rows_updated"] > 0
    print("LPs at N_tilde %d (reserved %d): kinds %s, re-solved by the dense kernel: %d of %d" % (N, reserved, sorted(set(kinds)), int(dense.sum()), pool.size))
    _need(kinds, "proven", "infeasible")
    if N == hist.P35_N:
        assert not dense.any(), "the LP path ran and no working basis outgrew its capacity"
    else:
        assert dense.any() and not dense.all(), "overflowing and fitting LPs, both present"
        assert any(dense[midx == k].any() and not dense[midx == k].all() for k in range(6)), "both within one model"
    order, labels = hist.chain(kinds)
    pairs = hist.assert_all_pairs(order, kinds)
    if dense.any():
        after = [(dense[order[p - 1]], dense[order[p]]) for p in range(1, len(order))]
        assert (True, False) in after and (False, True) in after, "a fitting LP directly after an overflowing one, and the reverse, in upload order"
    tiled = np.tile(order, -(-LP_TILE // len(order)))
    h = pool.handle(**opts)
    try:
        out = h.run(tiled)
    finally:
        h.close()
    tag = "LPs at N_tilde %d, reserved %d, %d kinds, %d pairs, batch %d" % (N, reserved, len(labels), pairs, len(tiled))
    hist.assert_same_bits(out, alone, tiled, tag, kinds=kinds)
    print("%s: HiGHS agrees on %d feasible and %d infeasible positions" % ((tag,) + hist.assert_anchor(out, tiled, inst, tag)))


# ---- the medium shapes ----------------------------------------------------------------------------------------------------------------------------
def _medium(name, batch, n_agents=1, quadratic=False):
    key = (name, batch, n_agents, quadratic)
    if key in _pools:
        return _pools[key]
    wl = syn.make_workload(name, batch=batch, n_agents=n_agents, quadratic=quadratic)
    ags = wl["agents"]
    d = ags[0]["dims"]
    costs = [host.cost_from_atoms(a["atoms"], d, wl["N_p"], wl["N_tilde"]) for a in ags]
    x0, om = np.concatenate([a["x0"] for a in ags]), np.concatenate([a["omega"] for a in ags])
    midx = None
    if n_agents > 1:      # interleaved: every instance follows another model's
        perm = np.arange(n_agents * batch).reshape(n_agents, batch).T.ravel()
        x0, om, midx = x0[perm], om[perm], (perm // batch).astype(np.int32)
    pool = Pool("%s x%d%s%s" % (name, batch, " MIQP" if quadratic else "", " %d models" % n_agents if n_agents > 1 else ""), [a["mats"] for a in ags], d,
                host.stack_costs(costs) if n_agents > 1 else costs[0], wl["N_p"], wl["N_tilde"], x0, om, midx=midx)
    _pools[key] = pool
    return pool


def _by_ending_and_work(alone):
    """status, nodes > 1 and rows_updated above / below the median"""
    med = np.median(alone["rows_updated"])
    return ["%s/%s" % (_ending(alone, i), "long" if alone["rows_updated"][i] > med else "short") for i in range(len(alone["status"]))]


def _shape(pool, opts):
    h = pool.handle(**opts)
    try:
        return h.prob.debug_shape()
    finally:
        h.close()


MEDIUM = {"cfg2": (("cfg2", 64), dict(max_nodes=50)),
          "cfg3": (("cfg3", 32), dict(max_nodes=30, max_pivots=300)),
          "cfg3_legacy_loop": (("cfg3", 32), dict(max_nodes=30, max_pivots=300, reserved=LEGACY)),
          "cfg3_multi_model": (("cfg3", 4, 3), dict(max_nodes=30, max_pivots=300)),
          "cfg3_miqp": (("cfg3", 8, 1, True), dict(max_nodes=10, max_pivots=3000))}


@pytest.mark.parametrize("case", sorted(MEDIUM))
def test_medium_shapes(case):
    """cfg2 (64 instances, NodeLimit 50: the fixture of tests/test_gpu_update_paths.py), cfg3 (32, NodeLimit 30, 300 pivots), cfg3 in the legacy
    instantiation of the loop (a second copy with its own state handling), three cfg3 models interleaved, cfg3 MIQP (8, NodeLimit 10)"""
    args, opts = MEDIUM[case]
    pool = _medium(*args)
    s = _shape(pool, opts)
    assert s["all_lds"], s
    if not pool.name.count("MIQP"):
        assert s["lPair"] >= 0, s
    if pool.midx is not None:      # (ending and model: every ending of every model after every other)
        alone = _alone(pool, opts, lambda a: ["%s/m%d" % (_ending(a, i), pool.midx[i]) for i in range(pool.size)])
        assert len(set(k.split("/")[1] for k in alone["kinds"])) == 3 and np.all(pool.midx[1:] != pool.midx[:-1])
    else:
        alone = _alone(pool, opts, _by_ending_and_work)
        assert set(k.split("/")[1] for k in alone["kinds"]) == {"long", "short"}, sorted(set(alone["kinds"]))
    assert alone["pivots"].sum() > 0 and alone["rows_updated"].sum() > 0
    assert len(set(alone["kinds"])) >= 2
    _chains(pool, opts, alone, pool.name + (" legacy loop" if opts.get("reserved") else ""), whole_pool=True)


def test_cfg3_launch_history_on_one_handle():
    _launch_history(_medium("cfg3", 32), dict(max_nodes=30, max_pivots=300), _by_ending_and_work, "cfg3 launch history")


# ---- in-kernel hand-off ---------------------------------------------------------------------------------------------------------------------------
HANDOFF = dict(first_nodes=3, sub_nodes=12, max_gen=8, max_children=64, max_tree=100000, room_factor=64.0)


def test_in_kernel_handoff_whatever_the_slots_and_the_upload_order():
    """cfg2, 16 instances, the settings of test_in_kernel_handoff_with_a_tiny_first_pass_equals_the_unlimited_search.  The queue's room scales with the
    batch, so a single solve is no reference here: the SAME batch with one slot, three slots and the automatic count, uploaded in two orders, gives
    equal bits per instance and equal hand-off statistics -- provided no tree was given up for a full queue (the one order-dependent case)."""
    pool = _medium("cfg2", 16)
    opts = dict(gap_rel=0.0, max_nodes=100000, cut_rounds=1, reserved=NO_ORDER)
    orders = (np.arange(16), np.random.default_rng(16).permutation(16))
    base, base_tag = None, None
    for n_slots in (1, 3, 0):
        h = pool.handle(n_slots=n_slots, **opts)
        try:
            for o in orders:
                out = h.run(o, handoff=HANDOFF)
                tag = "hand-off, n_slots %d, order %s" % (n_slots, o[:4].tolist())
                print(tag, out["handoff"], np.bincount(out["status"].astype(np.int64)).tolist())
                assert out["handoff"]["queue_full"] == 0 and out["handoff"]["items"] >= 3, out["handoff"]
                back = np.argsort(o)          # results per INSTANCE
                per = {k: out[k][back] for k in ("obj", "v", "status", "lower_bound")}
                per["handoff"] = out["handoff"]
                if base is None:
                    base, base_tag = per, tag
                    continue
                for k in ("obj", "v", "status", "lower_bound"):
                    diff = np.flatnonzero(np.any((hist._bits(per[k]) != hist._bits(base[k])).reshape(16, -1), axis=1))
                    assert diff.size == 0, (tag, "against", base_tag, k, "instances", diff.tolist())
                assert per["handoff"] == base["handoff"], (tag, per["handoff"], base_tag, base["handoff"])
        finally:
            h.close()
