"""Sub-tree hand-off under a quadratic cost (MIQP): the in-kernel form (mld_set_handoff, GpuProblem.solve_handoff_device, MpcController(...,
handoff=...)) and the host-driven form (mld_record_open_nodes / mld_set_cutoffs, GpuProblem.solve_handoff).  An open node under a quadratic
cost is closed only on a proven lower bound -- its LP(q) value or the simplicial-decomposition bound of its QP relaxation --
so the merged answer must be what the plain search of every instance returns: checked against the plain solve, the C oracle, and on every
point against the ORIGINAL rows and the point's own quadratic objective."""
import numpy as np
import pytest

import condense_np as cn
import orc
import tighten_np
import pyhybridcontrol_amd as phc
from pyhybridcontrol_amd import gpu, host, synthetic as syn

pytestmark = pytest.mark.gpu

GAP = 1e-6


def _quad(cfg, batch, **opts):
    wl = syn.make_workload(cfg, batch=batch, quadratic=True)
    ag = wl["agents"][0]
    d = ag["dims"]
    m = gpu.GpuModel([ag["mats"]], d)
    p = gpu.GpuProblem(m, wl["N_p"], wl["N_tilde"], host.cost_from_atoms(ag["atoms"], d, wl["N_p"], wl["N_tilde"]), **opts)
    return wl, ag, m, p


def _check_points(wl, ag, out, ref):
    """every instance proven, at ref's objective within the gap, bound below the objective; every point binary-exact, feasible for the original
    (un-tightened) rows, and its objective 1/2 v'Pv + q.v + r is the reported one"""
    nb = len(out["obj"])
    assert np.all(out["status"] == 0), np.unique(out["status"], return_counts=True)
    scale = np.maximum(1.0, np.abs(ref["obj"]))
    assert np.all(np.abs(out["obj"] - ref["obj"]) <= 2 * GAP * scale), np.abs(out["obj"] - ref["obj"]).max()
    assert np.all(out["lower_bound"] <= out["obj"] + 1e-9 * scale)
    d = ag["dims"]
    sf = cn.standard_form(ag["mats"], ag["atoms"], wl["N_p"], wl["N_tilde"], nu_l=d["nu_l"])
    isb = sf["is_bin"].astype(bool)
    rown = np.maximum(1.0, np.abs(sf["G"]).max(axis=1))
    for s in range(nb):
        x0, om = ag["x0"][s], ag["omega"][s]
        v = out["v"][s]
        assert np.all((v[isb] == 0) | (v[isb] == 1)), s
        h = cn.rhs(sf["evo"], x0, om)
        assert np.all((sf["G"] @ v - h) / rown <= 1e-6), s
        q, r = cn.lin_cost(sf["cost"], x0, om), cn.cost_const(sf["cost"]["const_terms"], x0, om)
        val = 0.5 * v @ sf["cost"]["P"] @ v + q @ v + r
        assert abs(val - out["obj"][s]) <= 1e-6 * max(1.0, abs(out["obj"][s])), (s, val, out["obj"][s])


def test_in_kernel_handoff_of_a_quadratic_cost_with_a_tiny_first_pass_equals_the_plain_search():
    """cfg2 shape with the quadratic atoms, 48 instances at gap 1e-6: 3 nodes per instance, 12 per item, items split again up to eight generations
    deep.  The instances that need a tree publish their open nodes (measured on an MI355X: 947 items); the merged result per instance is the plain
    search's optimum, a second run returns the same bits, and a plain solve afterwards is the plain solve"""
    wl, ag, m, p = _quad("cfg2", 48, gap_rel=GAP, max_nodes=100000, cut_rounds=1)
    ref = p.solve(ag["x0"], ag["omega"])
    assert np.all(ref["status"] == 0)
    kw = dict(first_nodes=3, sub_nodes=12, max_gen=8, max_children=64, max_tree=100000, room_factor=64.0)
    out = p.solve_handoff_device(ag["x0"], ag["omega"], **kw)
    print("MIQP in-kernel handoff:", out["handoff"], "plain nodes max %d" % ref["nodes"].max())
    assert out["handoff"]["items"] >= 3
    _check_points(wl, ag, out, ref)
    again = p.solve_handoff_device(ag["x0"], ag["omega"], **kw)
    assert np.array_equal(again["obj"], out["obj"]) and np.array_equal(again["v"], out["v"]) and np.array_equal(again["status"], out["status"]), "reproducible whatever the queue order"
    assert p.opts.max_nodes == 100000
    plain = p.solve(ag["x0"], ag["omega"])
    assert np.array_equal(plain["obj"], ref["obj"]) and np.array_equal(plain["v"], ref["v"]) and np.array_equal(plain["status"], ref["status"])
    p.close(); m.close()


def test_host_driven_handoff_of_a_quadratic_cost_with_a_tiny_first_pass_equals_the_plain_search():
    """the same instances through solve_handoff: the open nodes of the stopped searches, read off their stacks, solved as instances of their own under
    the parent's incumbent as cutoff, several rounds deep"""
    wl, ag, m, p = _quad("cfg2", 48, gap_rel=GAP, max_nodes=100000, cut_rounds=1)
    ref = p.solve(ag["x0"], ag["omega"])
    assert np.all(ref["status"] == 0)
    out = p.solve_handoff(ag["x0"], ag["omega"], first_nodes=3, sub_nodes=12, rounds=30, max_open=None)
    print("MIQP host-driven handoff:", out["handoff"])
    assert out["handoff"]["handed_off"] >= 3 and len(out["handoff"]["rounds"]) >= 2
    _check_points(wl, ag, out, ref)
    assert p.opts.max_nodes == 100000
    p.close(); m.close()


def test_cutoff_semantics_under_a_quadratic_cost():
    """under a cutoff only better points count, the quadratic constant included: a cutoff above the optimum changes nothing, one below it ends
    INFEASIBLE ("nothing better": the root is closed on its LP(q) value or on its QP relaxation's bound), and an upload clears the cutoffs"""
    wl, ag, m, p = _quad("cfg2", 16, gap_rel=1e-9, max_nodes=100000)
    ref = p.solve(ag["x0"], ag["omega"])
    assert np.all(ref["status"] == 0)
    scale = np.maximum(1.0, np.abs(ref["obj"]))
    p.upload(ag["x0"], ag["omega"])
    p.set_cutoffs(ref["obj"] + 1.0)
    p.solve_resident(); hi = p.download()
    assert np.all(hi["status"] == 0) and np.all(np.abs(hi["obj"] - ref["obj"]) <= 2e-9 * scale), np.abs(hi["obj"] - ref["obj"]).max()
    p.upload(ag["x0"], ag["omega"])
    p.set_cutoffs(ref["obj"] - 1e-6 * scale)
    p.solve_resident(); lo = p.download()
    assert np.all(lo["status"] == 1) and not np.any(np.isfinite(lo["obj"]))
    p.upload(ag["x0"], ag["omega"])
    p.solve_resident(); again = p.download()
    assert np.array_equal(again["obj"], ref["obj"]) and np.array_equal(again["v"], ref["v"])
    p.close(); m.close()


def test_in_kernel_handoff_on_the_cfg3_miqp_shape_against_the_oracle():
    """64 instances of the BASELINE cfg3 shape with Q_x = 1e-3 I at gap 1e-6, in-kernel hand-off after a first pass of 200 nodes: at least what the
    plain search proves, every proven objective at the oracle's optimum, no incumbent worse than the plain one beyond the gap contract"""
    nb = 64
    wl, ag, m, p = _quad("cfg3", nb, gap_rel=GAP, max_nodes=20000, max_pivots=400000)
    plain = p.solve(ag["x0"], ag["omega"])
    out = p.solve_handoff_device(ag["x0"], ag["omega"], first_nodes=200, sub_nodes=200, max_gen=8)
    print("MIQP cfg3 in-kernel handoff:", out["handoff"], "proven plain %d handoff %d  kernel ms plain %.1f handoff %.1f" %
          ((plain["status"] == 0).sum(), (out["status"] == 0).sum(), plain["stats"]["solve_ms"], out["stats"]["solve_ms"]))
    p.close(); m.close()
    assert (out["status"] == 0).sum() >= (plain["status"] == 0).sum()
    assert np.all(out["obj"] <= plain["obj"] + GAP * np.maximum(1.0, np.abs(plain["obj"])))
    d = ag["dims"]
    sft = cn.standard_form(tighten_np.tighten(ag["mats"], d, nu_l=d["nu_l"]), ag["atoms"], wl["N_p"], wl["N_tilde"], nu_l=d["nu_l"])
    worst = 0.0
    for s in np.flatnonzero(out["status"] == 0):
        x0, om = ag["x0"][s], ag["omega"][s]
        q, r = cn.lin_cost(sft["cost"], x0, om), cn.cost_const(sft["cost"]["const_terms"], x0, om)
        ref = orc.solve_miqp(sft["cost"]["P"], q, sft["G"], cn.rhs(sft["evo"], x0, om), sft["lb"], sft["ub"], sft["is_bin"],
                             max_nodes=20000, presolve=0, gap_rel=GAP)
        assert ref["status"] == "optimal", (s, ref["status"])
        tot = ref["obj"] + r
        worst = max(worst, abs(out["obj"][s] - tot) / max(1.0, abs(tot)))
        assert abs(out["obj"][s] - tot) <= 2 * GAP * max(1.0, abs(tot)), (s, out["obj"][s], tot)
        assert out["lower_bound"][s] <= tot + GAP * max(1.0, abs(tot)), s
    print("worst |obj - oracle| %.2e" % worst)


def test_controller_with_a_quadratic_atom_hands_off():
    """batch 1 through MpcController with Q_x set: with handoff=... the hardest instances of a plain batch solve publish items, and the objective is the
    one of the same controller without the hand-off, within the gap"""
    wl, ag, m, p = _quad("cfg3", 64, gap_rel=GAP, max_nodes=20000, max_pivots=400000)
    assert ag["atoms"].get("Q_x") is not None
    plain = p.solve(ag["x0"], ag["omega"])
    p.close(); m.close()
    hard = [int(i) for i in np.argsort(-plain["nodes"], kind="stable")[:3]]
    print("hard instances", hard, "plain nodes", plain["nodes"][hard])
    d = ag["dims"]
    opts = dict(gap_rel=GAP, max_nodes=20000, max_pivots=400000)
    ctrls = {}
    for ho in (None, dict(first_nodes=50, sub_nodes=100)):
        c = phc.MpcController(phc.MldModel(ag["mats"], nu_l=d["nu_l"]), N_p=wl["N_p"], handoff=ho, **opts)
        c.set_std_obj_atoms(**ag["atoms"])
        c.build()
        ctrls[ho is not None] = c
    items = []
    for i in hard:
        a = ctrls[False].solve(0, x_k=ag["x0"][i], omega_tilde_k=ag["omega"][i], warm_start=False)
        assert ctrls[False]._status == "optimal"
        b = ctrls[True].solve(0, x_k=ag["x0"][i], omega_tilde_k=ag["omega"][i], warm_start=False)
        assert ctrls[True]._status == "optimal"
        items.append(ctrls[True]._problem.handoff_stats()["items"])
        assert abs(a - b) <= 2 * GAP * max(1.0, abs(a)), (i, a, b)
    print("controller items per hard instance:", items)
    assert max(items) > 0
