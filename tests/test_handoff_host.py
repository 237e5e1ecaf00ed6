"""GpuProblem.solve_handoff's bookkeeping (no GPU): the host-driven sub-tree hand-off on a toy device (_handoff_toy) whose trees are small enough to
enumerate, driven to every ending -- proven, rounds used up, trees given up by max_open, the max_sub break, nodes dropped because they came
back unsplit twice or UNBOUNDED -- and checked per tree against the enumerated optimum: the bound is a bound, the incumbent belongs to the
reported objective, an unfinished tree is counted once."""
import itertools

import numpy as np
import pytest

from _handoff_toy import FREE, ToyProblem, ToyTree

N_BIN = 6
SEEDS = (1, 2, 3, 4)
FIRST_NODES = (1, 3)
SUB_NODES = (2, 5)
ROUNDS = (1, 2, 3, 30)
MAX_OPEN = (None, 1, 2)
MAX_SUB = (None, 6)
INJECT = (None, "unsplit", "status4")
GAP_ABS = {1: 0.0, 2: 0.0, 3: 0.75, 4: 0.0}          # one seed with a gap wider than the leaves' grid (0.5)
KEEP_NODES = 1000


def _trees(seed):
    """8 trees of 4-6 free binaries (the others fixed from the start: the fixed_bin route); tree 0 has no finite leaf, trees 5 and 6 start with a
    search that returns a point and no stack"""
    return [ToyTree(1000 * seed + t, N_BIN, (4, 5, 6, 6, 5, 6, 4, 6)[t], all_inf=(t == 0), dive_first=t in (5, 6)) for t in range(8)]


def _run(seed, first_nodes, sub_nodes, rounds, max_open, max_sub, inject):
    trees = _trees(seed)
    p = ToyProblem.make(trees, gap_abs=GAP_ABS[seed], max_nodes=KEEP_NODES, inject=inject, pick=seed)
    x0 = np.arange(len(trees), dtype=np.float64)[:, None]
    out = p.solve_handoff(x0, np.zeros((len(trees), 0)), fixed_bin=np.stack([t.base for t in trees]), rounds=rounds, first_nodes=first_nodes,
                          sub_nodes=sub_nodes, max_sub=max_sub, max_open=max_open)
    return dict(case=(seed, first_nodes, sub_nodes, rounds, max_open, max_sub, inject), trees=trees, p=p, out=out)


@pytest.fixture(scope="module")
def sweep():
    return [_run(*c) for c in itertools.product(SEEDS, FIRST_NODES, SUB_NODES, ROUNDS, MAX_OPEN, MAX_SUB, INJECT)]


def test_every_result_is_valid_against_the_enumerated_optimum(sweep):
    for r in sweep:
        out, p = r["out"], r["p"]
        tol_of = lambda obj: max(p.opts.gap_abs, p.opts.gap_rel * abs(obj))
        for i, tree in enumerate(r["trees"]):
            opt, obj, lb, st = tree.optimum(), out["obj"][i], out["lower_bound"][i], int(out["status"][i])
            where = (r["case"], i, st, lb, opt, obj)
            assert st in (0, 1, 2), where
            assert lb <= opt <= obj, where
            if st == 0:
                assert np.isfinite(obj) and obj - opt <= tol_of(obj), where
            if st == 1:
                assert not np.isfinite(opt) and not np.isfinite(obj), where
            if np.isfinite(obj):                    # v is the leaf whose value is obj, inside the fixings the tree was posed with
                bits = out["v"][i, 1:]
                assert np.all((bits == 0) | (bits == 1)) and np.all((tree.base == FREE) | (tree.base == bits)), where
                assert tree.leaf_of(bits) == obj and out["v"][i, 0] == obj, where


def test_unfinished_counts_every_unfinished_tree_once(sweep):
    for r in sweep:
        out, p = r["out"], r["p"]
        ho = out["handoff"]
        assert ho["handed_off"] == int((p.log["first_status"] == 2).sum()), r["case"]
        assert np.all(out["status"][p.log["first_status"] != 2] == p.log["first_status"][p.log["first_status"] != 2]), r["case"]
        assert ho["unfinished"] == int((out["status"] == 2).sum()), (r["case"], ho, out["status"])
        assert np.all(out["nodes"] >= 1) and np.array_equal(out["pivots"], 7 * out["nodes"]), r["case"]      # every pass is summed


def test_generous_limits_prove_every_tree(sweep):
    n = 0
    for r in sweep:
        seed, first_nodes, sub_nodes, rounds, max_open, max_sub, inject = r["case"]
        if inject is None and rounds == 30 and max_open is None and max_sub is None:
            n += 1
            assert np.all(r["out"]["status"] != 2) and r["out"]["handoff"]["unfinished"] == 0, (r["case"], r["out"]["status"])
            assert len(r["out"]["handoff"]["rounds"]) >= 2, r["case"]
    assert n == len(SEEDS) * len(FIRST_NODES) * len(SUB_NODES)


def test_limits_and_cutoffs_are_restored(sweep):
    for r in sweep:
        p = r["p"]
        assert p.opts.max_nodes == KEEP_NODES and p.log["cutoffs_cleared"] and not p.recording, r["case"]


def test_the_sweep_reaches_every_ending(sweep):
    """without these the assertions above prove nothing"""
    dropped_beside_open = given_up = max_sub_break = rounds_used_up = dropped = 0
    for r in sweep:
        seed, first_nodes, sub_nodes, rounds, max_open, max_sub, inject = r["case"]
        ho, log = r["out"]["handoff"], r["p"].log
        dropped += ho.get("dropped", 0)
        assert ho.get("dropped", 0) == (0 if inject is None else min(1, ho.get("dropped", 0)))
        if ho.get("dropped", 0):
            assert log["injected_returns"] == (2 if inject == "unsplit" else 1), r["case"]      # retried once, then dropped; status 4 at once
            dropped_beside_open += log["dropped_beside_open"]
        given_up += ho.get("given_up", 0)
        if inject is None:
            left = ho["unfinished"] - ho.get("given_up", 0)         # trees that end NODE_LIMIT with nodes still in the open list
            if left and len(ho["rounds"]) < rounds:
                assert max_sub is not None, r["case"]
                max_sub_break += 1
            if left and len(ho["rounds"]) == rounds:
                rounds_used_up += 1
    print("reach: dropped %d (beside open nodes %d), given up %d, max_sub breaks %d, rounds used up %d"
          % (dropped, dropped_beside_open, given_up, max_sub_break, rounds_used_up))
    assert dropped_beside_open >= 1 and given_up >= 1 and max_sub_break >= 1 and rounds_used_up >= 1
