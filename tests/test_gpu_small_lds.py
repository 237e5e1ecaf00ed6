"""The small-problem path (mld_opts.flags & MLD_SMALL_LDS): k_small_milp, an LDS-resident dual simplex with depth-first branch-and-bound, one wave per
instance, for problems whose whole dense dictionary fits a wave's share of LDS; what it declines is re-solved by the dense kernel in the same call.

References, all code the path does not touch: the dense path of the same problem on a second handle without the flag; scipy.optimize.milp on the ORIGINAL
rows; the closed form of tests/_aux_ref.py; GpuProblem.evaluate().  Tolerances are the project's (tests/test_gpu_aux.py, tests/test_gpu_sim_resolve.py):
objective within 1e-6 max(1, |obj|), residual on the original rows <= 1e-6 max(1, max|x|), binaries exactly 0 / 1, mu >= -1e-9, statuses equal.
Every test asserts through small_lds_stats() that the path it means to test ran.

Shapes (n unknowns x m rows): the horizon-1 auxiliaries of make_agent(3) 8 x 12, make_agent(7) 16 x 20, make_agent(15) 32 x 36; cfg1 at N_tilde = 5
15 x 10; make_agent(3) at N_tilde = 2 and 3, 22 x 24 and 33 x 36 -- the last one the largest eligible, 33 columns across two lane groups.  Batches are
no multiple of the four waves of a workgroup, model_idx is interleaved."""
import numpy as np
import pytest

import _aux_ref
import condense_np as cn
from pyhybridcontrol_amd import gpu, host, synthetic as syn, _lib
from pyhybridcontrol_amd.aux_resolve import BatchAuxResolver

pytestmark = pytest.mark.gpu

SMALL = _lib.MLD_SMALL_LDS
OPTIMAL, INFEASIBLE = 0, 1
AUX_SHAPES = dict(a10=(3, 3, 10, 8101), a1=(3, 3, 1, 8102), b9=(7, 2, 9, 8103), c5=(15, 2, 5, 8104))      # n_h, models, batch, seed of the triples
MPC_SHAPES = dict(cfg1=(1, 2, 5, 7, False, 8225), a3n2=(3, 2, 2, 9, True, 8202), a3n3=(3, 2, 3, 9, True, 8203))      # n_h, models, N_tilde, batch, tie, seed
# (the seeds of the MPC shapes: with them the C oracle without cut rounds branches on at least one instance of every shape -- cfg1 7 nodes on instance 5 --,
# so a search without cuts has real branch-and-bound to do)
RESULT = ("v", "obj", "status", "lower_bound", "nodes", "pivots")


def _tol(v):
    return 1e-6 * np.maximum(1.0, np.abs(v))


# ---- horizon-1 auxiliaries ---------------------------------------------------------------------------------------------------------------------------------
def aux_case(name, hard=False):
    """models, dims, interleaved model_idx and the drawn triples of an auxiliary shape (numpy only)"""
    n_h, n_models, B, seed = AUX_SHAPES[name]
    mats, oms = [], []
    for k in range(n_models):
        rng = np.random.default_rng(7700 + 10 * n_h + k)
        m, d, _ = syn.make_agent(n_h, rng, tie=True)
        _, om = syn.make_scenarios(n_h, 1, 16, rng, tie=True)
        mats.append(m); oms.append(om)
    midx = (np.arange(B) % n_models).astype(np.int32)
    x, u, w = _aux_ref.draw_triples(dict(dims=d, omega=oms[0]), B, np.random.default_rng(seed))
    if hard:
        hv = [_aux_ref.hard_variant(m, d) for m in mats]
        mats, d = [h[0] for h in hv], hv[0][1]
    return mats, d, midx, x, u, w


def _closed_form(mats, d, midx, x, u, w):
    out = None
    for k, m in enumerate(mats):
        cf = _aux_ref.closed_form(m, d, x, u, w)
        if out is None:
            out = {n: np.zeros_like(a) for n, a in cf.items()}
        for n in cf:
            out[n][midx == k] = cf[n][midx == k]
    return out


@pytest.mark.parametrize("name", list(AUX_SHAPES))
def test_auxiliaries_equal_the_closed_form(name):
    mats, d, midx, x, u, w = aux_case(name)
    B = len(midx)
    cf = _closed_form(mats, d, midx, x, u, w)
    assert np.all(np.abs(cf["y"]) >= 1e-3)                                   # the closed form is unique there; no instance is left out
    R = BatchAuxResolver(mats, d, small_lds=True)
    try:
        got = R.resolve(x, u, w, midx)
        st = R.problem.small_lds_stats()
        assert st == dict(eligible=True, lds=B, dense=0), st
        assert np.all(got["status"] == OPTIMAL)
        assert np.array_equal(got["delta"], cf["delta"])
        tot = cf["mu"].sum(axis=1)
        err_mu = np.abs(got["mu"].sum(axis=1) - tot) / np.maximum(1.0, tot)
        res = np.array([_aux_ref.residual(mats[midx[b]], d, x[b], u[b], w[b], got["delta"][b], got["z"][b], got["mu"][b]).max() / max(1.0, np.abs(x[b]).max())
                        for b in range(B)])
        print("%s: worst |sum(mu) - closed| / max(1, sum) %.3g, worst residual / max(1, max|x|) %.3g" % (name, err_mu.max(), res.max()))
        assert np.all(err_mu <= 1e-6) and np.all(res <= 1e-6)
        assert np.all(got["mu"] >= -1e-9)
        out = R.problem.download()
        assert np.all(out["nodes"] >= 1) and np.all(out["pivots"] >= 1)
    finally:
        R.close()


def test_fp32_right_hand_sides_compose_with_the_flag():
    """MLD_F32 | MLD_SMALL_LDS: K3 in fp32, the solver in fp64 -- against the dense path under the same flag, which reads the same right-hand sides"""
    mats, d, midx, x, u, w = aux_case("a10")
    Rs, Rd = BatchAuxResolver(mats, d, small_lds=True, flags=_lib.MLD_F32), BatchAuxResolver(mats, d, flags=_lib.MLD_F32)
    try:
        assert Rs.problem.opts.flags == _lib.MLD_F32 | SMALL
        a, b = Rs.resolve(x, u, w, midx), Rd.resolve(x, u, w, midx)
        assert Rs.problem.small_lds_stats() == dict(eligible=True, lds=len(midx), dense=0)
        assert Rd.problem.small_lds_stats() == dict(eligible=False, lds=0, dense=0)
        assert np.array_equal(a["status"], b["status"]) and np.array_equal(a["delta"], b["delta"])
        sa, sb = a["mu"].sum(axis=1), b["mu"].sum(axis=1)
        assert np.all(np.abs(sa - sb) <= _tol(sb))
        with pytest.raises(TypeError):
            Rs.problem.set_opts(flags=_lib.MLD_F32)                          # fixed at creation
    finally:
        Rs.close(); Rd.close()


def test_infeasible_auxiliaries():
    mats, d, midx, x, u, w = aux_case("a10", hard=True)
    B = len(midx)
    hot = np.zeros(B, bool)
    hot[[1, 4, 7]] = True
    x = np.clip(x, 51.0, 64.0)                                               # every other tank inside its hard bounds
    x[hot, 0] = 90.0
    Rs, Rd = BatchAuxResolver(mats, d, small_lds=True), BatchAuxResolver(mats, d)
    try:
        assert Rs.nv2 == 2
        a, b = Rs.resolve(x, u, w, midx), Rd.resolve(x, u, w, midx)
        assert Rs.problem.small_lds_stats() == dict(eligible=True, lds=B, dense=0)
        assert np.array_equal(a["status"], b["status"])
        assert np.all(a["status"][hot] == INFEASIBLE) and np.all(a["status"][~hot] == OPTIMAL)
        assert np.all(np.isnan(a["v"][hot])) and np.all(np.isfinite(a["v"][~hot]))
        assert np.array_equal(a["delta"][~hot], b["delta"][~hot])
    finally:
        Rs.close(); Rd.close()


# ---- real branch-and-bound -----------------------------------------------------------------------------------------------------------------------------------
def mpc_case(name):
    """models, prices and one scenario per instance of an MPC shape (numpy only)"""
    n_h, n_models, N, B, tie, seed = MPC_SHAPES[name]
    mats, atoms, xs, oms = [], [], [], []
    for k in range(n_models):
        rng = np.random.default_rng(seed + k)
        m, d, params = syn.make_agent(n_h, rng, tie=tie)
        x0, om = syn.make_scenarios(n_h, N, B, rng, tie=tie)
        mats.append(m); atoms.append(syn.make_cost(n_h, N, params, tie=tie)); xs.append(x0); oms.append(om)
    midx = (np.arange(B) % n_models).astype(np.int32)
    at = np.arange(B)
    return dict(mats=mats, atoms=atoms, d=d, N=N, B=B, midx=midx, x0=np.stack(xs)[midx, at], om=np.stack(oms)[midx, at], n_h=n_h, tie=tie)


def mpc_variant(c, variant):
    """fixed_bin and per-instance lin_v of a variant (None where it has none)"""
    sf = cn.standard_form(c["mats"][0], c["atoms"][0], c["N"] - 1, c["N"], nu_l=c["d"]["nu_l"])
    bins = np.flatnonzero(sf["is_bin"])
    fixed = lin_v = None
    if variant == "fixed":
        fixed = np.full((c["B"], len(bins)), 255, np.uint8)
        fixed[1::2, 0], fixed[1::2, 1] = 0, 1
    if variant == "lin_v":
        rng = np.random.default_rng(8300 + c["B"] + c["N"])
        q0 = np.abs(np.ravel(cn.lin_cost(sf["cost"], c["x0"][0], c["om"][0])))
        lin_v = rng.uniform(0.0, 1.0, (c["B"], len(q0))) * np.maximum(q0.max(), 1e-3) * 0.5
    return bins, fixed, lin_v


def mpc_reference(c, s, bins, fixed, lin_v):
    """scipy.optimize.milp on the original rows of instance s: (feasible, objective with its constant)"""
    from scipy.optimize import milp, LinearConstraint, Bounds
    k = c["midx"][s]
    sf = cn.standard_form(c["mats"][k], c["atoms"][k], c["N"] - 1, c["N"], nu_l=c["d"]["nu_l"])
    x0, om = c["x0"][s], c["om"][s]
    q, r, h = np.ravel(cn.lin_cost(sf["cost"], x0, om)), cn.cost_const(sf["cost"]["const_terms"], x0, om), cn.rhs(sf["evo"], x0, om)
    lb, ub = np.array(sf["lb"], float), np.array(sf["ub"], float)
    if lin_v is not None:
        q = q + lin_v[s]
    if fixed is not None:
        for kb in np.flatnonzero(fixed[s] != 255):
            lb[bins[kb]] = ub[bins[kb]] = float(fixed[s, kb])
    ref = milp(q, constraints=LinearConstraint(sf["G"], -np.inf, np.ravel(h)), integrality=sf["is_bin"].astype(int), bounds=Bounds(lb, ub), options=dict(mip_rel_gap=0.0))
    assert ref.status in (0, 2), ref.message
    return ref.status == 0, (ref.fun + float(r)) if ref.status == 0 else np.inf


class _Mpc(object):
    """a flagged and an unflagged handle over the same models and cost"""

    def __init__(self, name, quadratic=False, **opts):
        c = mpc_case(name)
        self.__dict__.update(c)
        self.c = c
        if quadratic:
            self.atoms = [dict(a, Q_x=1e-3 * np.eye(self.n_h)) for a in self.atoms]
        self.model = gpu.GpuModel(self.mats, self.d)
        cost = host.stack_costs([host.cost_from_atoms(a, self.d, self.N - 1, self.N) for a in self.atoms])
        o = dict(gap_rel=0.0, gap_abs=1e-9, max_nodes=20000)
        o.update(opts)
        self.flag = gpu.GpuProblem(self.model, self.N - 1, self.N, cost, flags=SMALL, **o)
        self.plain = gpu.GpuProblem(self.model, self.N - 1, self.N, cost, **o)

    def close(self):
        self.flag.close(); self.plain.close(); self.model.close()


_CACHE = {}


@pytest.fixture(scope="module")
def mpc():
    def get(name):
        if name not in _CACHE:
            _CACHE[name] = _Mpc(name)
        return _CACHE[name]
    yield get
    for c in _CACHE.values():
        c.close()
    _CACHE.clear()


def _solve(p, c, fixed=None, lin_v=None, order=None):
    sel = np.arange(c.B) if order is None else np.asarray(order)
    return p.solve(c.x0[sel], c.om[sel], c.midx[sel], None if fixed is None else np.ascontiguousarray(fixed[sel]),
                   inst_cost=None if lin_v is None else dict(lin_v=np.ascontiguousarray(lin_v[sel])))


def _same_answers(a, b, what):
    assert np.array_equal(a["status"], b["status"]), what
    ok = a["status"] == OPTIMAL
    assert np.all(np.abs(a["obj"][ok] - b["obj"][ok]) <= _tol(b["obj"][ok])), what
    assert np.all(np.isinf(a["obj"][~ok])), what


@pytest.mark.parametrize("variant", ["plain", "fixed", "lin_v"])
@pytest.mark.parametrize("name", list(MPC_SHAPES))
def test_branch_and_bound_against_highs_and_the_dense_path(mpc, name, variant):
    c = mpc(name)
    bins, fixed, lin_v = mpc_variant(c.c, variant)
    got = _solve(c.flag, c, fixed, lin_v)
    st = c.flag.small_lds_stats()
    q = c.flag.evaluate()
    dense = _solve(c.plain, c, fixed, lin_v)
    print("%s %s: small path %s, nodes %s, pivots %s" % (name, variant, st, got["nodes"].tolist(), got["pivots"].tolist()))
    assert st["eligible"] and st["lds"] + st["dense"] == c.B and st["lds"] > 0, st
    assert c.plain.small_lds_stats() == dict(eligible=False, lds=0, dense=0)
    _same_answers(got, dense, "dense path")
    for s in range(c.B):
        feasible, opt = mpc_reference(c.c, s, bins, fixed, lin_v)
        assert got["status"][s] == (OPTIMAL if feasible else INFEASIBLE), (s, got["status"][s])
        if feasible:
            assert abs(got["obj"][s] - opt) <= _tol(opt), (s, got["obj"][s], opt)
    ok = got["status"] == OPTIMAL
    assert np.all(q["int_vio"][ok] == 0.0)
    assert np.all(q["constr_vio"][ok] <= _tol(np.abs(got["v"][ok]).max(axis=1)))
    vb = got["v"][:, bins]
    assert np.all((vb == 0.0) | (vb == 1.0))
    if fixed is not None:
        fx = fixed != 255
        assert np.array_equal(vb[ok][fx[ok]], fixed[ok][fx[ok]].astype(float))
    if variant == "plain":
        assert st["dense"] == 0, st
        assert got["nodes"].max() > 1                                        # the root is node 1: at least one instance branched


@pytest.mark.parametrize("name", list(MPC_SHAPES))
def test_declined_instances_are_solved_by_the_dense_kernel(mpc, name):
    c = mpc(name)
    ref = _solve(c.flag, c)
    assert c.flag.small_lds_stats()["dense"] == 0
    c.flag.set_opts(reserved=_lib.MLD_DBG_SMALL_PIVOT_CAP)
    try:
        got = _solve(c.flag, c)
        st = c.flag.small_lds_stats()
    finally:
        c.flag.set_opts(reserved=0)
    print(name, st)
    assert st["dense"] > 0 and st["lds"] + st["dense"] == c.B, st
    _same_answers(got, ref, "pivot cap")
    assert np.all(got["status"] >= 0)
    again = _solve(c.flag, c)                                                # the bit cleared: the handle is as before
    for k in RESULT:
        assert np.array_equal(again[k], ref[k]), k


@pytest.mark.parametrize("name", list(MPC_SHAPES))
def test_an_instance_has_the_same_bits_wherever_it_runs(mpc, name):
    c = mpc(name)
    ref = _solve(c.flag, c)
    rev = _solve(c.flag, c, order=np.arange(c.B)[::-1])
    big_order = np.r_[np.arange(c.B)[::2], np.tile(np.arange(c.B), 6), np.arange(c.B)[1::2]]      # 7 B instances: more than one workgroup
    big = _solve(c.flag, c, order=big_order)
    assert c.flag.small_lds_stats() == dict(eligible=True, lds=len(big_order), dense=0)
    for k in RESULT:
        assert np.array_equal(rev[k], ref[k][::-1]), k
        assert np.array_equal(big[k], ref[k][big_order]), k


# ---- the path rule -------------------------------------------------------------------------------------------------------------------------------------------
def _dense_and_identical(c, prepare=None, what=""):
    outs = []
    for p in (c.flag, c.plain):
        p.upload(c.x0, c.om, c.midx)
        if prepare:
            prepare(p)
        p.solve_resident()
        outs.append(p.download())
    st = c.flag.small_lds_stats()
    assert st["lds"] == 0 and st["dense"] == 0, (what, st)
    for k in RESULT:
        assert np.array_equal(outs[0][k], outs[1][k]), (what, k)
    return st


def test_path_rule_ineligible_shape():
    n_h, N, B = 7, 25, 2
    rng = np.random.default_rng(8401)
    mats, d, params = syn.make_agent(n_h, rng, tie=True)
    x0, om = syn.make_scenarios(n_h, N, B, rng, tie=True)
    model = gpu.GpuModel([mats], d)
    cost = host.cost_from_atoms(syn.make_cost(n_h, N, params), d, N - 1, N)
    outs = []
    try:
        for flags in (SMALL, 0):
            p = gpu.GpuProblem(model, N - 1, N, cost, gap_rel=1e-2, max_nodes=50, flags=flags)
            try:
                outs.append(p.solve(x0, om))
                st = p.small_lds_stats()
                assert st == dict(eligible=False, lds=0, dense=0), st
            finally:
                p.close()
    finally:
        model.close()
    for k in RESULT:
        assert np.array_equal(outs[0][k], outs[1][k]), k


def test_path_rule_quadratic_cost():
    c = _Mpc("a3n2", quadratic=True, max_nodes=400)
    try:
        st = _dense_and_identical(c, what="quadratic")
        assert st["eligible"]
    finally:
        c.close()


def test_path_rule_cutoffs_time_limit_and_handoff(mpc):
    c = mpc("a3n2")
    assert c.flag.small_lds_stats()["eligible"]
    _dense_and_identical(c, lambda p: p.set_cutoffs(np.full(c.B, np.inf)), "cutoffs")
    for p in (c.flag, c.plain):
        p.set_opts(time_limit=30.0)
    try:
        _dense_and_identical(c, what="time limit")
    finally:
        for p in (c.flag, c.plain):
            p.set_opts(time_limit=0.0)
    for p in (c.flag, c.plain):
        p.set_handoff(True)
    try:
        _dense_and_identical(c, what="hand-off")
    finally:
        for p in (c.flag, c.plain):
            p.set_handoff(False)
    # ... and with all of it cleared the flagged handle is back on the small path
    _solve(c.flag, c)
    assert c.flag.small_lds_stats() == dict(eligible=True, lds=c.B, dense=0)
