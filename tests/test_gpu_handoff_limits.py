"""The sub-tree hand-off's UNFINISHED endings, against HiGHS.  The other hand-off tests drive both forms to the one ending where every tree is
proven; here one limit at a time binds -- rounds, max_open, max_sub on the host route, max_gen, max_children, max_tree inside the launch, and the
donation policy -- so instances come back NODE_LIMIT with an incumbent and a lower bound, and every such answer is checked per instance: the
bound is a bound of the true optimum (scipy.optimize.milp on the oracle's standard form of the original rows, not this solver), the point
returned is the point of the reported objective, nothing is worse than what the first pass alone returns, and the counters count trees once.
The small limits come from the ladder {1, 2, 4}: the largest rung at which the case still reaches its ending on this batch."""
import numpy as np
import pytest

import condense_np as cn
from pyhybridcontrol_amd import MldGpuError, gpu, host, synthetic as syn

pytestmark = pytest.mark.gpu

BATCH, FIRST, SUB, TOL = 48, 3, 12, 1e-6
GENEROUS = dict(max_gen=8, max_children=64, max_tree=100000, room_factor=64.0)

# name -> (route, arguments, reach): reach(handoff statistics) must hold or the case checks nothing
CASES = {
    "host-rounds-1": ("host", dict(rounds=1, max_open=None), lambda ho: ho["unfinished"] >= 1 and len(ho["rounds"]) == 1),
    "host-rounds-2": ("host", dict(rounds=2, max_open=None), lambda ho: len(ho["rounds"]) == 2),
    "host-max-open": ("host", dict(rounds=30, max_open=4), lambda ho: ho.get("given_up", 0) >= 1),
    "host-max-sub": ("host", dict(rounds=30, max_open=None, max_sub=4), lambda ho: len(ho["rounds"]) == 0 and ho["unfinished"] == ho["handed_off"] >= 1),
    "device-max-gen": ("device", dict(GENEROUS, max_gen=1), lambda ho: ho["items"] >= 1 and ho["unfinished"] >= 1 and ho["given_up"] == 0),
    "device-max-children": ("device", dict(GENEROUS, max_children=4), lambda ho: ho["items"] >= 1 and ho["unfinished"] >= 1 and ho["given_up"] == 0),
    "device-max-tree": ("device", dict(GENEROUS, max_tree=4), lambda ho: ho["given_up"] >= 1),
    "donate-1-rounds-1": ("device", dict(GENEROUS, donate=1, rounds=1), lambda ho: ho["items"] >= 1),
    "donate-2-rounds-3": ("device", dict(GENEROUS, donate=2, rounds=3), lambda ho: ho["items"] >= 1),
}


class _Ctx(object):
    pass


def make_ctx(batch=BATCH, cut_rounds=1):
    """the batch, its problem, the HiGHS optimum of every instance and the plain solve with the first pass's node limit"""
    from scipy.optimize import Bounds, LinearConstraint, milp
    c = _Ctx()
    wl = syn.make_workload("cfg2", batch=batch)
    ag = c.ag = wl["agents"][0]
    d = ag["dims"]
    c.m = gpu.GpuModel([ag["mats"]], d)
    c.p = gpu.GpuProblem(c.m, wl["N_p"], wl["N_tilde"], host.cost_from_atoms(ag["atoms"], d, wl["N_p"], wl["N_tilde"]),
                         gap_rel=0.0, max_nodes=100000, cut_rounds=cut_rounds)
    sf = c.sf = cn.standard_form(ag["mats"], ag["atoms"], wl["N_p"], wl["N_tilde"], nu_l=d["nu_l"])
    c.h = np.stack([cn.rhs(sf["evo"], ag["x0"][s], ag["omega"][s]) for s in range(batch)])
    c.q = np.stack([cn.lin_cost(sf["cost"], ag["x0"][s], ag["omega"][s]) for s in range(batch)])
    c.r = np.array([cn.cost_const(sf["cost"]["const_terms"], ag["x0"][s], ag["omega"][s]) for s in range(batch)])
    c.opt = np.zeros(batch)
    for s in range(batch):
        ref = milp(c.q[s], constraints=LinearConstraint(sf["G"], -np.inf, c.h[s]), integrality=sf["is_bin"].astype(int),
                   bounds=Bounds(sf["lb"], sf["ub"]), options=dict(mip_rel_gap=0.0, time_limit=60))
        assert ref.status == 0, (s, ref.status, ref.message)
        c.opt[s] = ref.fun + c.r[s]
    c.sc = np.maximum(1.0, np.abs(c.opt))
    c.p.set_opts(max_nodes=FIRST)
    c.first = c.p.solve(ag["x0"], ag["omega"])
    c.p.set_opts(max_nodes=100000)
    return c


@pytest.fixture(scope="module")
def ctx():
    c = make_ctx()
    yield c
    c.p.close(); c.m.close()


def run_case(c, route, kw):
    if route == "host":
        return c.p.solve_handoff(c.ag["x0"], c.ag["omega"], first_nodes=FIRST, sub_nodes=SUB, **kw)
    return c.p.solve_handoff_device(c.ag["x0"], c.ag["omega"], first_nodes=FIRST, sub_nodes=SUB, **kw)


def figures(c, out):
    """what the summary reports per case"""
    ho = out["handoff"]
    fin = np.isfinite(out["obj"])
    return dict(items=ho.get("items"), handed_off=ho.get("handed_off"), given_up=ho.get("given_up", 0), unfinished=ho["unfinished"],
                status2=int((out["status"] == 2).sum()), proven=int((out["status"] == 0).sum()),
                max_lb_minus_opt=float(((out["lower_bound"] - c.opt) / c.sc).max()),
                max_opt_minus_obj=float(((c.opt - out["obj"])[fin] / c.sc[fin]).max()) if fin.any() else None)


def check_case(c, out):
    obj, lb, st, v, sf = out["obj"], out["lower_bound"], out["status"], out["v"], c.sf
    assert np.all((st == 0) | (st == 2)), np.unique(st, return_counts=True)       # every instance of this batch is feasible
    assert np.all(obj >= c.opt - TOL * c.sc), (np.argmin(obj - c.opt), (obj - c.opt).min())
    assert np.all(lb <= c.opt + TOL * c.sc), (np.argmax(lb - c.opt), (lb - c.opt).max())
    assert np.all(lb <= obj + 1e-9)
    assert np.all(np.abs(obj - c.opt)[st == 0] <= 2e-6 * c.sc[st == 0])
    gscale = np.maximum(1.0, np.abs(sf["G"]).max(axis=1))
    for s in np.flatnonzero(np.isfinite(obj)):             # the point belongs to the objective: NODE_LIMIT (the given-up trees' root points above all) and proven alike
        assert np.all((v[s][sf["is_bin"]] == 0) | (v[s][sf["is_bin"]] == 1)), s
        assert np.all(sf["G"] @ v[s] - c.h[s] <= 1e-6 * gscale), (s, st[s])
        assert abs(c.q[s] @ v[s] + c.r[s] - obj[s]) <= 1e-7 * max(1.0, abs(obj[s])), (s, st[s], c.q[s] @ v[s] + c.r[s], obj[s])
    assert np.all(obj <= c.first["obj"] + 1e-9 * c.sc), "an incumbent worse than the first pass's own"
    assert np.all(lb >= c.first["lower_bound"] - 1e-9 * c.sc), "a bound weaker than the first pass's own"
    assert int((st == 2).sum()) == out["handoff"]["unfinished"], ((st == 2).sum(), out["handoff"])


@pytest.mark.parametrize("name", list(CASES))
def test_ending(ctx, name):
    """one limit binds, every other one is generous (batch 48, cut_rounds=1; rung 4 of the ladder reaches each ending here: 13 of 48 instances are
    handed off, max_open / max_tree = 4 give 3 trees up, max_children = 4 leaves 3 split trees unfinished, max_sub = 4 is below the first
    sub-batch of 13).  In-kernel and donation cases must return the same bits when called again; the donation cases must prove everything."""
    route, kw, reach = CASES[name]
    out = run_case(ctx, route, kw)
    print(name, kw, figures(ctx, out))
    assert reach(out["handoff"]), out["handoff"]
    check_case(ctx, out)
    assert ctx.p.opts.max_nodes == 100000
    if route == "device":
        again = run_case(ctx, route, kw)
        for k in ("obj", "v", "lower_bound"):
            assert np.array_equal(again[k].view(np.uint64), out[k].view(np.uint64)), k
        assert np.array_equal(again["status"], out["status"]) and again["handoff"] == out["handoff"]
    if name.startswith("donate"):
        assert np.all(out["status"] == 0) and out["handoff"]["unfinished"] == 0
        assert np.all(np.abs(out["obj"] - ctx.opt) <= 2e-6 * ctx.sc)


def test_set_handoff_drops_the_resident_batch_on_the_handle_too(ctx):
    """mld_set_handoff frees the resident batch whenever the switch (or room_factor) changes; the Python handle must not go on believing in it"""
    p, ag = ctx.p, ctx.ag
    ref = p.solve(ag["x0"], ag["omega"])
    assert p.upload(ag["x0"], ag["omega"]) == BATCH and p.batch == BATCH
    p.set_handoff(True, sub_nodes=SUB)
    assert p.batch == 0
    with pytest.raises(MldGpuError):
        p.solve_resident()
    p.upload(ag["x0"], ag["omega"])
    p.set_handoff(True, sub_nodes=SUB, max_gen=4)              # limits alone change nothing that is laid out: the batch stays
    assert p.batch == BATCH
    p.set_handoff(True, sub_nodes=SUB, room_factor=8.0)        # another room_factor does
    assert p.batch == 0
    with pytest.raises(MldGpuError):
        p.solve_resident()
    p.upload(ag["x0"], ag["omega"])
    p.set_handoff(False)
    assert p.batch == 0
    with pytest.raises(MldGpuError):
        p.solve_resident()
    plain = p.solve(ag["x0"], ag["omega"])
    for k in ("obj", "v", "lower_bound", "status"):
        assert np.array_equal(plain[k], ref[k]), k
    assert np.all(plain["status"] == 0) and np.all(np.abs(plain["obj"] - ctx.opt) <= 2e-6 * ctx.sc)
