"""The helpers of the history tests (tests/_history.py) on the CPU: the all-pairs sequence, the pool P35 and its HiGHS classes, the per-instance
inputs, and the comparator on a planted one-bit difference."""
import numpy as np
import pytest

import _hard
import _history as hist


@pytest.mark.parametrize("k", range(1, 9))
def test_the_sequence_has_every_ordered_pair_as_neighbours(k):
    seq = hist.all_pairs_sequence(k)
    assert len(seq) == k * k + 1 and set(seq) == set(range(k))
    assert hist.pairs_of(seq) == {(a, b) for a in range(k) for b in range(k)}
    assert hist.pairs_of(seq[::-1]) == hist.pairs_of(seq)          # (the reversed chain covers them too)


def test_a_chain_takes_the_instances_of_a_kind_in_turn():
    kinds = ["a", "b", "a", "c", "b", "a"]
    order, labels = hist.chain(kinds)
    assert labels == ["a", "b", "c"] and len(order) == 10
    assert hist.assert_all_pairs(order, kinds, required=("a", "b", "c")) == 9
    assert [i for i in order if kinds[i] == "a"][:4] == [0, 2, 5, 0]
    rev, _ = hist.chain(kinds, reverse=True)
    assert np.array_equal(rev, order[::-1])
    with pytest.raises(AssertionError, match="lacks kind"):
        hist.assert_all_pairs(order, kinds, required=("d",))
    with pytest.raises(AssertionError, match="never neighbours"):
        hist.assert_all_pairs(order[:-1], kinds)


def test_p35_has_equal_dimensions_and_both_classes():
    pool = hist.p35()
    assert len(pool["models"]) == 6 and len(pool["inst"]) == 36
    for m in pool["models"]:
        assert m["dims"] == pool["dims"]
        assert m["raw"]["G"].shape == (30, 35) and int(m["raw"]["is_bin"].sum()) == 20
        assert np.array_equal(m["raw"]["is_bin"], pool["models"][0]["raw"]["is_bin"])
    feas, infeas, dropped = hist.classes(pool["inst"])
    per_seed = ["".join(c["cls"][0] for c in pool["inst"][6 * k:6 * k + 6]) for k in range(6)]
    print("P35: %d feasible, %d infeasible, %d dropped; per seed %s" % (feas, infeas, dropped, per_seed))
    assert infeas >= 5 and feas >= 20 and dropped <= _hard.MAX_DROPPED * 36, (feas, infeas, dropped)
    assert np.array_equal(pool["midx"], np.repeat(np.arange(6), 6))


def test_the_per_instance_inputs_hold_every_variant():
    pool, inp = hist.p35(), hist.p35_inputs()
    present = set(inp["variant"])
    print("variants:", sorted(inp["kind"]))
    assert present >= set(hist.FEASIBLE_VARIANTS), present
    assert inp["violated"].any(), "premise: a start that HiGHS's LP cannot complete within the margin, on a feasible instance"
    for i, (v, e) in enumerate(zip(inp["variant"], inp["expect"])):
        has_start, n_fixed = inp["warm"][i, 0] != 255, int((inp["fixed"][i] != 255).sum())
        assert has_start == (v in ("own_start", "bad_start", "other_start")), (i, v)
        if pool["inst"][i]["cls"] == "feasible":
            assert bool(inp["violated"][i]) == (v == "bad_start"), (i, v)
        assert n_fixed in {"fix_partial": (7,), "fix_contra": (1,)}.get(v, (0,)), (i, v, n_fixed)
        assert np.isfinite(inp["cutoff"][i]) == (v in ("cut_above", "cut_below")), (i, v)
        assert bool(inp["lin_v"][i].any()) == ("+lin" in inp["kind"][i])
        if v == "fix_contra":
            assert e["cls"] == "infeasible" and pool["inst"][i]["cls"] == "feasible"
        if v == "cut_below":
            assert e["cls"] == "cut_below"
    assert sum("+lin" in k for k in inp["kind"]) == 18 and any("/inf" in k for k in inp["kind"])
    assert len(set(inp["kind"])) >= 10


@pytest.mark.parametrize("N", [hist.P35_N, 12])
def test_the_lp_fixings_hold_an_infeasible_lp(N):
    fixed, inst = hist.p35_lp_fixings(N=N)
    assert fixed.shape == (36, 4 * N) and np.all(fixed <= 1)
    assert hist.p35(N)["models"][0]["raw"]["G"].shape == (6 * N, 7 * N)
    feas, infeas, dropped = hist.classes(inst)
    print("P35 LPs at N_tilde %d: %d feasible, %d infeasible, %d dropped" % (N, feas, infeas, dropped))
    assert infeas >= 1 and feas >= 1


def _fake(order, n_inst=5, n=3):
    rng = np.random.default_rng(0)
    alone = dict(obj=rng.standard_normal(n_inst), v=rng.standard_normal((n_inst, n)), lower_bound=rng.standard_normal(n_inst),
                 status=np.zeros(n_inst, np.int32), nodes=np.arange(n_inst, dtype=np.int32), pivots=np.arange(n_inst, dtype=np.int32) * 7,
                 rows_updated=np.arange(n_inst, dtype=np.int64) * 100, cuts=np.arange(n_inst), refactors=np.ones(n_inst, np.int64))
    out = {k: np.array(alone[k][order]) for k in hist.KEYS}
    out["stats"] = dict(cuts=int(alone["cuts"][order].sum()), refactors=int(alone["refactors"][order].sum()))
    return out, alone


def test_the_comparator_names_position_instance_and_predecessor_of_a_planted_bit():
    kinds = ["root", "tree", "infeasible", "tree", "root"]
    order, _ = hist.chain(kinds)
    out, alone = _fake(order)
    hist.assert_same_bits(out, alone, order, "clean", kinds=kinds)
    pos = 6
    out["v"][pos].view(np.uint64)[1] ^= np.uint64(1)           # one bit of one double: equal under any tolerance
    assert np.allclose(out["v"], alone["v"][order], rtol=1e-15, atol=0)
    with pytest.raises(AssertionError) as err:
        hist.assert_same_bits(out, alone, order, "planted", kinds=kinds)
    msg = str(err.value)
    want = "position %d (instance %d, kind %r, after instance %d of kind %r) differs from its single solve in 'v'" % (
        pos, order[pos], kinds[order[pos]], order[pos - 1], kinds[order[pos - 1]])
    assert want in msg, msg
    out, alone = _fake(order)
    alone["obj"][order[0]] = 0.0
    out["obj"][np.flatnonzero(order == order[0])] = -0.0       # -0.0 against 0.0: equal as numbers, not as bits
    with pytest.raises(AssertionError, match="position 0 .*after nothing.* in 'obj'"):
        hist.assert_same_bits(out, alone, order, "signed zero", kinds=kinds)
    out, alone = _fake(order)
    out["stats"]["cuts"] += 1
    with pytest.raises(AssertionError, match="cuts"):
        hist.assert_same_bits(out, alone, order, "totals", kinds=kinds)


def test_the_anchor_holds_a_status_to_the_class():
    e = [dict(cls="feasible", opt=1.0, lo=1.0 - 1e-9, r=0.5), dict(cls="infeasible", r=0.0), dict(cls="dropped", r=0.0), dict(cls="cut_below", r=0.0)]
    out = dict(status=np.array([0, 1, 3, 1]), obj=np.array([1.5, np.inf, 0.0, np.inf]))
    assert hist.assert_anchor(out, [0, 1, 2, 3], e, "ok") == (1, 2)
    for bad in (dict(status=np.array([0, 0, 0, 1]), obj=out["obj"]), dict(status=out["status"], obj=np.array([1.6, np.inf, 0.0, np.inf])),
                dict(status=np.array([1, 1, 0, 1]), obj=out["obj"])):
        with pytest.raises(AssertionError):
            hist.assert_anchor(bad, [0, 1, 2, 3], e, "bad")
