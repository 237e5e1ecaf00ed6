"""Per-instance linear cost of a resident batch (mld_upload_instance_cost / mld_download_instance_cost): the reference rebuilds its objective
from the current tariff before every solve() call (micro_grid_control_simulation.py:194-198,229), so N calls replaced by one batch may carry N
price vectors.  Checked: the pull-back kernels (k_inst_pullback fp64 / fp32, k_inst_pullback_valu) against fp64 numpy; one model with B costs
against B replicated models with one cost each (bitwise for weights on v); HiGHS on the original rows; the paths around the solver (streams,
staged inputs, advance, in-kernel hand-off, MIQP, the LDS-resident LP and its overflow re-solve); the lifetime of the uploaded cost."""
import datetime

import numpy as np
import pytest

import _paths
import condense_np as cn
import orc
import tighten_np
from pyhybridcontrol_amd import gpu, host, synthetic as syn, _lib

pytestmark = pytest.mark.gpu

PATHS = (("mfma64", dict()), ("valu", dict(reserved=128)), ("mfma32", dict(flags=_lib.MLD_F32)))
# name -> (N, dims); the first five are COST_SHAPES of test_gpu_kernel_paths.py, "k380" has N nx + N ny = 380 > 256 (two chunks of the inner dimension)
SHAPES = {
    "below16": (5, dict(nx=3, nu=1, ndelta=1, nz=1, nomega=3, ny=3, nc=4)),
    "straddle64": (13, dict(nx=5, nu=3, ndelta=1, nz=1, nomega=5, ny=1, nc=4)),
    "nx17": (4, dict(nx=17, nu=14, ndelta=1, nz=1, nomega=16, ny=4, nc=4)),
    "nw0": (9, dict(nx=7, nu=5, ndelta=1, nz=1, nomega=0, ny=2, nc=3)),
    "nx0": (6, dict(nx=0, nu=4, ndelta=1, nomega=4, ny=3, nc=4)),
    "k380": (20, dict(nx=17, nu=2, ndelta=1, nz=1, nomega=2, ny=2, nc=3)),
}


def _ref_pullback(evo, lin_v, lin_x, lin_y, x0, om):
    """q = lin_v + Gamma_v' lin_x + L_v' lin_y and the constant lin_x'(Phi_x x0 + Gamma_w w + Gamma_5) + lin_y'(L_x x0 + L_w w + L_5), per instance"""
    B = x0.shape[0]
    q, c = np.zeros((B, evo["Gamma_v"].shape[1])), np.zeros(B)
    if lin_v is not None:
        q += lin_v
    for lin, Mv, Mx, Mw, M5 in ((lin_x, "Gamma_v", "Phi_x", "Gamma_omega", "Gamma_5"), (lin_y, "L_v", "L_x", "L_omega", "L_5")):
        if lin is None:
            continue
        q += lin @ evo[Mv]
        e = x0 @ evo[Mx].T + om @ evo[Mw].T + evo[M5][:, 0]
        c += np.einsum("bi,bi->b", lin, e)
    return q, c


def _check_pullback(got, ref_q, ref_c, fp32, gemm):
    for name, g, r in (("q", got["q"], ref_q), ("const", got["const"], ref_c)):
        scale = float(np.abs(r).max())
        err = float(np.abs(g - r).max())
        print("%s: max|ref| %.3e err %.3e" % (name, scale, err))
        if not gemm:
            assert np.array_equal(g, r), name            # weights on v alone: kept as uploaded, no constant
            continue
        assert scale > 0, name
        assert err <= (1e-5 if fp32 else 1e-11) * scale, (name, err / scale)
        if fp32 and name == "q":
            assert err > 1e-13 * scale                   # the fp32 kernel really ran


def _pullback_case(mats_list, d, N, evos, path, seed, tv=False):
    rng = np.random.default_rng(seed)
    kw = dict(PATHS)[path]
    n, NX, NY, nx, nW = N * d["nv"], N * d["nx"], N * d["ny"], d["nx"], N * d["nomega"]
    m = gpu.GpuModel(mats_list, d, time_varying=tv)
    p = gpu.GpuProblem(m, N - 1, N, None, **kw)
    try:
        midx = rng.permutation(np.r_[np.zeros(170), np.full(130, 2)]).astype(np.int32)      # model 1 unused; partial groups of 42 and 2
        x0, om = rng.standard_normal((300, nx)), rng.standard_normal((300, nW))
        p.upload(x0, om, midx)
        lv, lx, ly = rng.standard_normal((300, n)), (rng.standard_normal((300, NX)) if NX else None), rng.standard_normal((300, NY))
        if not NX:
            with pytest.raises(ValueError):
                p.upload_instance_cost(lin_x=np.zeros((300, 0)))
        for which in ("v", "x", "y", "all"):
            a = dict(lin_v=lv if which in ("v", "all") else None, lin_x=lx if which in ("x", "all") else None, lin_y=ly if which in ("y", "all") else None)
            if all(v is None for v in a.values()):
                continue
            p.upload_instance_cost(**a)
            got = p.instance_cost()
            rq, rc = np.zeros((300, n)), np.zeros(300)
            for k in (0, 2):
                s = midx == k
                rq[s], rc[s] = _ref_pullback(evos[k], *(None if v is None else v[s] for v in (a["lin_v"], a["lin_x"], a["lin_y"])), x0[s], om[s])
            print(path, which, end=" ")
            _check_pullback(got, rq, rc, path == "mfma32", which != "v")
        # one model, model_idx = None: two full groups and one of 44
        p.upload(x0, om)
        p.upload_instance_cost(lin_v=lv, lin_x=lx, lin_y=ly)
        rq, rc = _ref_pullback(evos[0], lv, lx, ly, x0, om)
        _check_pullback(p.instance_cost(), rq, rc, path == "mfma32", True)
    finally:
        p.close(); m.close()


@pytest.mark.parametrize("path", [p for p, _ in PATHS])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_pullback_paths_against_fp64_numpy(shape, path):
    """k_inst_pullback<false> (default), k_inst_pullback_valu (reserved bit 7), k_inst_pullback<true> (MLD_F32) through mld_download_instance_cost:
    300 instances over three interleaved models with one unused, each of lin_v / lin_x / lin_y alone and all together"""
    N, dims = SHAPES[shape]
    d = _paths.make_dims(**dims)
    seed = 5000 + 10 * list(SHAPES).index(shape)
    mats = [_paths.random_mld(seed * 100000 + i, **dims)[0] for i in range(3)]
    _pullback_case(mats, d, N, [cn.condense(a, N) for a in mats], path, seed)


def test_valu_switch_selects_another_kernel():
    """reserved bit 7 must really select k_inst_pullback_valu: the two fp64 kernels sum in different orders (two MFMA accumulators over k blocks of
    four against one sequential sum), so on the same inputs their results agree to rounding and are NOT bit-identical"""
    N, dims = SHAPES["straddle64"]
    d = _paths.make_dims(**dims)
    mats = [_paths.random_mld(777, **dims)[0]]
    rng = np.random.default_rng(778)
    x0, om = rng.standard_normal((200, d["nx"])), rng.standard_normal((200, N * d["nomega"]))
    lx, ly = rng.standard_normal((200, N * d["nx"])), rng.standard_normal((200, N * d["ny"]))
    got = {}
    for path in ("mfma64", "valu"):
        m = gpu.GpuModel(mats, d)
        p = gpu.GpuProblem(m, N - 1, N, None, **dict(PATHS)[path])
        try:
            p.upload(x0, om); p.upload_instance_cost(lin_x=lx, lin_y=ly)
            got[path] = p.instance_cost()["q"]
        finally:
            p.close(); m.close()
    diff = np.abs(got["mfma64"] - got["valu"]).max()
    print("max |mfma64 - valu| = %.3e over %d entries, %d differ" % (diff, got["valu"].size, (got["mfma64"] != got["valu"]).sum()))
    assert diff <= 1e-11 * np.abs(got["valu"]).max()
    assert not np.array_equal(got["mfma64"], got["valu"])


@pytest.mark.parametrize("path", [p for p, _ in PATHS])
def test_pullback_time_varying(path):
    """a time-varying handle (three horizons of independent step models, maps from k_tv_chain + k_tv_rows): model_idx indexes horizons"""
    N, dims = 8, dict(nx=4, nu=3, ndelta=1, nmu=1, nomega=2, ny=2, nc=4)
    horizons = [_paths.random_horizon(90 + i, N, **dims)[0] for i in range(3)]
    _pullback_case(horizons, _paths.make_dims(**dims), N, [cn.condense_tv(h) for h in horizons], path, 5900, tv=True)


# ------------------------------------------------------------------------------------------------------------------ solver
def _cfg2(batch):
    wl = syn.make_workload("cfg2", batch=batch)
    ag = wl["agents"][0]
    return wl, ag, ag["dims"]


def _scaled_tariffs(wl, ag, B, seed, with_xy=False, qx=1e-6):
    """per instance the workload's atoms with q_z scaled by a seeded factor in [0.5, 2] (optionally q_y = 0.1 q_z u, q_x = qx u)"""
    rng = np.random.default_rng(seed)
    d, N = ag["dims"], wl["N_tilde"]
    out = []
    for _ in range(B):
        a = dict(ag["atoms"])
        a["q_z"] = a["q_z"] * rng.uniform(0.5, 2.0)
        if with_xy:
            a["q_y"] = 0.1 * a["q_z"] * rng.uniform(0, 1, size=a["q_z"].shape)
            a["q_x"] = qx * rng.uniform(0, 1, size=(N * d["nx"], 1))
        out.append(a)
    return out


def _split(atoms):
    """(common part for the model, scenario part per instance)"""
    return {"q_mu": atoms["q_mu"]}, {k: v for k, v in atoms.items() if k != "q_mu"}


def _shared(wl, ag, atoms_list, model=None, **opts):
    """problem A: ONE model whose cost is the q_mu atoms; the rest of every instance's atoms as the per-instance cost"""
    d = ag["dims"]
    m = model or gpu.GpuModel([ag["mats"]], d)
    p = gpu.GpuProblem(m, wl["N_p"], wl["N_tilde"], host.cost_from_atoms(_split(atoms_list[0])[0], d, wl["N_p"], wl["N_tilde"]), **opts)
    ic = host.instance_costs([_split(a)[1] for a in atoms_list], d, wl["N_p"], wl["N_tilde"])
    return m, p, {k: v for k, v in ic.items() if v is not None}


def _replicated(wl, ag, atoms_list, **opts):
    """problem B: the model replicated once per instance, model b carrying instance b's full atoms; model_idx = arange(B)"""
    d = ag["dims"]
    B = len(atoms_list)
    m = gpu.GpuModel([ag["mats"]] * B, d)
    cost = host.stack_costs([host.cost_from_atoms(a, d, wl["N_p"], wl["N_tilde"]) for a in atoms_list])
    return m, gpu.GpuProblem(m, wl["N_p"], wl["N_tilde"], cost, **opts), np.arange(B, dtype=np.int32)


def _same_bits(a, b, keys=("obj", "v", "status", "nodes", "pivots")):
    for k in keys:
        assert np.array_equal(a[k], b[k]), (k, a[k], b[k])


def _close_proven(a, b, min_cmp):
    both = (a["status"] == 0) & (b["status"] == 0)
    rel = np.abs(a["obj"][both] - b["obj"][both]) / np.maximum(1.0, np.abs(b["obj"][both]))
    print("proven on both sides %d of %d, worst relative difference %.2e" % (both.sum(), both.size, rel.max() if both.any() else 0.0))
    assert both.sum() >= min_cmp and np.all(rel <= 1e-6)


def test_one_model_with_b_costs_equals_b_models_with_one_cost_each():
    B = 16
    wl, ag, d = _cfg2(B)
    kw = dict(max_nodes=20000, gap_rel=1e-6)
    atoms = _scaled_tariffs(wl, ag, B, 21)
    mA, pA, ic = _shared(wl, ag, atoms, **kw)
    mB, pB, midx = _replicated(wl, ag, atoms, **kw)
    assert set(ic) == {"lin_v"}
    a = pA.solve(ag["x0"], ag["omega"], inst_cost=ic)
    b = pB.solve(ag["x0"], ag["omega"], midx)
    _same_bits(a, b)
    assert len(set(a["obj"].tolist())) > 1
    pA.close(); pB.close(); mB.close()
    # weights on x and y per instance: the batched GEMM against k_pullback of the replicated models
    atoms = _scaled_tariffs(wl, ag, B, 22, with_xy=True)
    _, pA, ic = _shared(wl, ag, atoms, model=mA, **kw)
    mB, pB, midx = _replicated(wl, ag, atoms, **kw)
    assert set(ic) == {"lin_v", "lin_x", "lin_y"}
    a = pA.solve(ag["x0"], ag["omega"], inst_cost=ic)
    b = pB.solve(ag["x0"], ag["omega"], midx)
    _close_proven(a, b, B - 4)
    pA.close(); pB.close(); mA.close(); mB.close()


@pytest.mark.parametrize("variant", ["qz", "qz_qx_qy", "qz_qx6_qy"])
def test_against_highs_on_the_original_rows(variant):
    """cfg2, 16 instances, each with its own tariff (start hour and scale seeded); reference scipy.optimize.milp on the un-tightened rows.
    At most 2 of the 16 may be left unproven.  Variants: q_z only; q_z with q_y = 0.1 q_z u and q_x = -1e-9 u (a weight the atom parser takes
    for zero, so only lin_y reaches the solver); and the same draws with q_x = +1e-6 u, so that a branch-and-bound solve with lin_x, lin_y and
    lin_v together is held to an independent MILP solver."""
    from scipy.optimize import milp, LinearConstraint, Bounds
    B = 16
    wl, ag, d = _cfg2(B)
    N, N_p = wl["N_tilde"], wl["N_p"]
    rng = np.random.default_rng(11)
    atoms = []
    for s in range(B):
        hour = int(rng.integers(0, 24))
        factor = rng.uniform(0.5, 2.0)
        a = syn.make_cost(wl["n_h"], N, ag["params"], tie=True, t0=datetime.datetime(2018, 12, 10, hour, 0))
        a["q_z"] = a["q_z"] * factor
        if variant != "qz":
            a["q_y"] = 0.1 * a["q_z"] * rng.uniform(0, 1, size=a["q_z"].shape)
            a["q_x"] = (-1e-9 if variant == "qz_qx_qy" else 1e-6) * rng.uniform(0, 1, size=(N * d["nx"], 1))
        atoms.append(a)
    m = gpu.GpuModel([ag["mats"]], d)
    p = gpu.GpuProblem(m, N_p, N, None, max_nodes=20000, gap_rel=1e-6)
    ic = {k: v for k, v in host.instance_costs(atoms, d, N_p, N).items() if v is not None}
    # (q_x = -1e-9 u is below the atom parser's zero threshold -- np.isclose(w, 0), as in the reference's objective_atoms.py -- and is dropped on
    #  both sides: that variant exercises lin_y, the third one all three)
    assert set(ic) == {"qz": {"lin_v"}, "qz_qx_qy": {"lin_v", "lin_y"}, "qz_qx6_qy": {"lin_v", "lin_x", "lin_y"}}[variant]
    out = p.solve(ag["x0"], ag["omega"], inst_cost=ic)
    p.close(); m.close()
    unproven = 0
    for s in range(B):
        sf = cn.standard_form(ag["mats"], atoms[s], N_p, N, nu_l=d["nu_l"])
        x0, om = ag["x0"][s], ag["omega"][s]
        q, r, h = cn.lin_cost(sf["cost"], x0, om), cn.cost_const(sf["cost"]["const_terms"], x0, om), cn.rhs(sf["evo"], x0, om)
        ref = milp(q, constraints=LinearConstraint(sf["G"], -np.inf, h), integrality=sf["is_bin"].astype(int), bounds=Bounds(sf["lb"], sf["ub"]),
                   options=dict(mip_rel_gap=1e-9))
        assert ref.status == 0, (s, ref.message)
        opt = ref.fun + r
        tol = 1e-6 * max(1.0, abs(opt))
        st = int(out["status"][s])
        print("instance %d: status %d obj %.12g bound %.12g HiGHS %.12g nodes %d" % (s, st, out["obj"][s], out["lower_bound"][s], opt, out["nodes"][s]))
        assert st in (0, 2), (s, st)
        if np.isfinite(out["obj"][s]):
            v = out["v"][s]
            bins = sf["is_bin"].astype(bool)
            assert np.all((v[bins] == 0) | (v[bins] == 1)), s
            assert np.all((sf["G"] @ v - h) / np.maximum(1.0, np.abs(sf["G"]).max(axis=1)) <= 1e-6), s
        if st == 0:
            assert abs(out["obj"][s] - opt) <= tol, (s, out["obj"][s], opt)
        else:
            unproven += 1
            assert out["obj"][s] >= opt - tol and out["lower_bound"][s] <= opt + tol, (s, out["obj"][s], out["lower_bound"][s], opt)
    print("unproven: %d of %d" % (unproven, B))
    assert unproven <= 2, unproven


def test_eight_tariffs_on_one_instance():
    """the model, x0 and omega of instance 0 eight times under eight tariffs as per-instance lin_v: every objective is the single-instance solve of a
    problem whose MODEL cost is that tariff, bit for bit, and the objectives differ"""
    wl, ag, d = _cfg2(8)
    N, N_p = wl["N_tilde"], wl["N_p"]
    costs = [host.cost_from_atoms(syn.make_cost(wl["n_h"], N, ag["params"], tie=True, t0=datetime.datetime(2018, 12, 10, h, 0)), d, N_p, N)
             for h in range(0, 24, 3)]
    m = gpu.GpuModel([ag["mats"]], d)
    p = gpu.GpuProblem(m, N_p, N, None, max_nodes=20000)
    x0, om = np.repeat(ag["x0"][:1], 8, axis=0), np.repeat(ag["omega"][:1], 8, axis=0)
    out = p.solve(x0, om, inst_cost=dict(lin_v=np.stack([c["lin_v"] for c in costs])))
    print("objectives:", out["obj"])
    assert np.all(out["status"] == 0)
    for s, c in enumerate(costs):
        p.set_cost(c)
        one = p.solve(x0[:1], om[:1])
        assert one["obj"][0] == out["obj"][s] and np.array_equal(one["v"][0], out["v"][s]), (s, one["obj"][0], out["obj"][s])
    assert len(set(out["obj"].tolist())) > 1
    p.close(); m.close()


def test_two_handles_on_two_streams():
    B = 16
    wl, ag, d = _cfg2(2 * B)
    kw = dict(max_nodes=2000, gap_rel=1e-4)
    atoms = _scaled_tariffs(wl, ag, B, 31)
    mA, p1, ic = _shared(wl, ag, atoms, **kw)
    _, p2, _ = _shared(wl, ag, atoms, model=mA, **kw)
    mB, pB, midx = _replicated(wl, ag, atoms, **kw)
    halves = [(ag["x0"][:B], ag["omega"][:B]), (ag["x0"][B:], ag["omega"][B:])]
    for p, (x, w) in zip((p1, p2), halves):
        p.use_stream(); p.upload(x, w); p.upload_instance_cost(**ic)
    p1.launch(); p2.launch()
    with pytest.raises(gpu.MldGpuError):
        p1.upload_instance_cost(**ic)               # between launch and finish: refused
    got = []
    for p in (p1, p2):
        p.finish(); got.append(p.download())
    for g, (x, w) in zip(got, halves):
        _same_bits(g, pB.solve(x, w, midx))
    for q in (p1, p2, pB):
        q.close()
    mA.close(); mB.close()


def test_staged_inputs_and_the_constant_term():
    """stage + select of a second input set: the weights stay, the constant term follows the selected inputs (q_x makes it non-zero)"""
    B = 16
    wl, ag, d = _cfg2(2 * B)
    N, N_p = wl["N_tilde"], wl["N_p"]
    kw = dict(max_nodes=2000, gap_rel=1e-6)
    atoms = _scaled_tariffs(wl, ag, B, 41, with_xy=True, qx=1e-6)
    mA, pA, ic = _shared(wl, ag, atoms, **kw)
    mB, pB, midx = _replicated(wl, ag, atoms, **kw)
    X, W = np.stack([ag["x0"][:B], ag["x0"][B:]]), np.stack([ag["omega"][:B], ag["omega"][B:]])
    pA.upload(X[0], W[0]); pA.upload_instance_cost(**ic); pA.stage(X, W)
    pB.upload(X[0], W[0], midx); pB.stage(X, W)
    evo = cn.condense(ag["mats"], N)
    for k in (1, 0):
        pA.select(k); pB.select(k)
        got = pA.instance_cost()
        rq, rc = _ref_pullback(evo, ic["lin_v"], ic["lin_x"], ic["lin_y"], X[k], W[k])
        assert np.abs(rc).max() > 1e-4
        assert np.abs(got["const"] - rc).max() <= 1e-11 * np.abs(rc).max() and np.abs(got["q"] - rq).max() <= 1e-11 * np.abs(rq).max()
        pA.solve_resident(); pB.solve_resident()
        _close_proven(pA.download(), pB.download(), B - 4)
    pA.close(); pB.close(); mA.close(); mB.close()


def test_advance_keeps_the_weights():
    B = 16
    wl, ag, d = _cfg2(B)
    kw = dict(max_nodes=2000, gap_rel=1e-4)
    atoms = _scaled_tariffs(wl, ag, B, 51)
    mA, pA, ic = _shared(wl, ag, atoms, **kw)
    mB, pB, midx = _replicated(wl, ag, atoms, **kw)
    a = pA.solve(ag["x0"], ag["omega"], inst_cost=ic)
    b = pB.solve(ag["x0"], ag["omega"], midx)
    _same_bits(a, b)
    assert pA.advance() == pB.advance()
    pA.solve_resident(); pB.solve_resident()
    _same_bits(pA.download(), pB.download())
    xa, wa = pA.inputs(); xb, wb = pB.inputs()
    assert np.array_equal(xa, xb) and np.array_equal(wa, wb) and not np.array_equal(xa, ag["x0"])
    pA.close(); pB.close(); mA.close(); mB.close()


def test_handoff_items_use_their_source_instances_cost():
    B = 16
    wl, ag, d = _cfg2(B)
    kw = dict(gap_rel=0.0, max_nodes=100000, cut_rounds=1)
    ho = dict(first_nodes=3, sub_nodes=12, max_gen=8, max_children=64, max_tree=100000, room_factor=64.0)
    atoms = _scaled_tariffs(wl, ag, B, 61)
    mA, pA, ic = _shared(wl, ag, atoms, **kw)
    mB, pB, midx = _replicated(wl, ag, atoms, **kw)
    a = pA.solve_handoff_device(ag["x0"], ag["omega"], inst_cost=ic, **ho)
    b = pB.solve_handoff_device(ag["x0"], ag["omega"], midx, **ho)
    print("hand-off:", a["handoff"], b["handoff"])
    assert pA.handoff_stats()["items"] > 0 and a["handoff"] == b["handoff"]
    _same_bits(a, b)
    pA.close(); pB.close(); mA.close(); mB.close()


def test_miqp_with_a_per_instance_linear_cost():
    """quadratic model cost (Q_x, q_mu) + per-instance tariff against the C oracle's MIQP on the same instance (tolerances of test_gpu_miqp.py)"""
    nb = 8
    wl = syn.make_workload("cfg3", batch=nb, quadratic=True)
    ag = wl["agents"][0]
    d, N, N_p = ag["dims"], wl["N_tilde"], wl["N_p"]
    atoms = _scaled_tariffs(wl, ag, nb, 71)
    common = {k: v for k, v in ag["atoms"].items() if k != "q_z"}
    m = gpu.GpuModel([ag["mats"]], d)
    p = gpu.GpuProblem(m, N_p, N, host.cost_from_atoms(common, d, N_p, N), gap_rel=1e-6, max_nodes=20000, max_pivots=400000)
    ic = host.instance_costs([{"q_z": a["q_z"]} for a in atoms], d, N_p, N)
    out = p.solve(ag["x0"], ag["omega"], inst_cost=dict(lin_v=ic["lin_v"]))
    p.close(); m.close()
    tm = tighten_np.tighten(ag["mats"], d, nu_l=d["nu_l"])
    proven = 0
    for s in range(nb):
        sft = cn.standard_form(tm, atoms[s], N_p, N, nu_l=d["nu_l"])
        x0, om = ag["x0"][s], ag["omega"][s]
        q, r = cn.lin_cost(sft["cost"], x0, om), cn.cost_const(sft["cost"]["const_terms"], x0, om)
        ref = orc.solve_miqp(sft["cost"]["P"], q, sft["G"], cn.rhs(sft["evo"], x0, om), sft["lb"], sft["ub"], sft["is_bin"], max_nodes=20000, presolve=0, gap_rel=1e-6)
        assert ref["status"] == "optimal", (s, ref["status"])
        tot = ref["obj"] + r
        st = int(out["status"][s])
        print("instance %d: status %d obj %.12g oracle %.12g" % (s, st, out["obj"][s], tot))
        assert st in (0, 2), (s, st)
        v = out["v"][s]
        val = 0.5 * v @ sft["cost"]["P"] @ v + q @ v + r
        assert abs(val - out["obj"][s]) <= 1e-6 * max(1.0, abs(tot)), (s, val, out["obj"][s])       # the reported objective is the point's, under ITS tariff
        assert out["lower_bound"][s] <= tot + 1e-6 * max(1.0, abs(tot)), s
        if st == 0:
            proven += 1
            assert abs(out["obj"][s] - tot) <= 2e-6 * max(1.0, abs(tot)), (s, out["obj"][s], tot)
        else:
            assert out["obj"][s] >= tot - 1e-6 * max(1.0, abs(tot)), s
    assert proven >= int(0.9 * nb), proven


def _fixed_pattern(ag, wl, p, d, rng, nb):
    """random heater schedules with the grid binary consistent with the sign of the tie flow (as test_gpu_loop does)"""
    bins = np.where(p.is_bin)[0]
    nv = d["nu"] + d["ndelta"] + d["nz"] + d["nmu"]
    isdelta = (bins % nv) == d["nu"]
    fixed = np.zeros((nb, p.n_bin), dtype=np.uint8)
    for s in range(nb):
        om = ag["omega"][s].reshape(wl["N_tilde"], -1)
        u = (rng.random((wl["N_tilde"], d["nu"])) < 0.2).astype(np.uint8)
        y = u @ ag["params"]["P_h_Nom"] + om[:, -1]
        fixed[s, ~isdelta] = u.ravel()
        fixed[s, isdelta] = (y >= 0).astype(np.uint8)
    return fixed


@pytest.mark.parametrize("reserved", [0, 256, 512])
def test_all_binaries_fixed_against_linprog(reserved):
    """relaxation-only batch with a per-instance cost: k_lp_lds (default), the dense kernel (MLD_DBG_NO_LP_LDS) and k_lp_lds with a working basis of
    24 (MLD_DBG_LP_LDS_K24: most instances overflow and are re-solved by the dense kernel) against scipy's HiGHS LP on the original rows"""
    from scipy.optimize import linprog
    B = 16
    wl, ag, d = _cfg2(B)
    N, N_p = wl["N_tilde"], wl["N_p"]
    atoms = _scaled_tariffs(wl, ag, B, 81, with_xy=True, qx=1e-6)
    m, p, ic = _shared(wl, ag, atoms, reserved=reserved)
    fixed = _fixed_pattern(ag, wl, p, d, np.random.Generator(np.random.PCG64(9)), B)
    out = p.solve(ag["x0"], ag["omega"], fixed_bin=fixed, inst_cost=ic)
    rows = p.telemetry()["rows_updated"]      # dictionary rows touched by rank-1 updates: counted by the dense kernel only, zeroed by the LDS path
    print("reserved %d: statuses %s pivots %s instances solved by the dense kernel %d of %d" % (reserved, out["status"], out["pivots"], (rows > 0).sum(), B))
    p.close(); m.close()
    if reserved == 0:
        assert np.all(rows == 0) and np.all(out["nodes"] == 1)       # k_lp_lds solved every instance
    elif reserved == 256:
        assert np.all(rows > 0)                                      # the dense kernel solved every instance
    else:
        assert (rows > 0).sum() >= 1                                 # working basis capped at 24: the overflow re-solve was taken
    n_opt = 0
    for s in range(B):
        sf = cn.standard_form(ag["mats"], atoms[s], N_p, N, nu_l=d["nu_l"])
        x0, om = ag["x0"][s], ag["omega"][s]
        bins = sf["is_bin"].astype(bool)
        lb, ub = sf["lb"].copy(), sf["ub"].copy()
        lb[bins] = ub[bins] = fixed[s]
        q, r = cn.lin_cost(sf["cost"], x0, om), cn.cost_const(sf["cost"]["const_terms"], x0, om)
        ref = linprog(q, A_ub=sf["G"], b_ub=cn.rhs(sf["evo"], x0, om), bounds=np.c_[lb, ub], method="highs")
        if ref.status == 0:
            n_opt += 1
            assert out["status"][s] == 0, (s, out["status"][s])
            assert abs(out["obj"][s] - (ref.fun + r)) <= 1e-6 * max(1.0, abs(ref.fun + r)), (s, out["obj"][s], ref.fun + r)
        else:
            assert out["status"][s] != 0, (s, ref.status, out["status"][s])
    print("LPs HiGHS solved to optimality: %d of %d" % (n_opt, B))
    assert n_opt == B          # (every fixing of this seed is feasible: all instances are compared)


def test_lifetime_of_the_uploaded_cost():
    B = 16
    wl, ag, d = _cfg2(B)
    atoms = _scaled_tariffs(wl, ag, B, 91)
    m, p, ic = _shared(wl, ag, atoms, max_nodes=2000, gap_rel=1e-4)
    with pytest.raises(gpu.MldGpuError):
        gpu.check(_lib.load().mld_upload_instance_cost(p._h, None, None, None))        # before any batch
    plain = p.solve(ag["x0"], ag["omega"])
    with_cost = p.solve(ag["x0"], ag["omega"], inst_cost=ic)
    assert not np.array_equal(plain["obj"], with_cost["obj"])
    _same_bits(p.solve(ag["x0"], ag["omega"]), plain)                                   # a new upload() clears
    p.upload(ag["x0"], ag["omega"]); p.upload_instance_cost(**ic); p.upload_instance_cost()
    assert not np.any(p.instance_cost()["q"])
    p.solve_resident(); _same_bits(p.download(), plain)                                 # everything None clears
    p.upload(ag["x0"], ag["omega"]); p.upload_instance_cost(**ic)
    with pytest.raises(ValueError):
        p.upload_instance_cost(lin_v=ic["lin_v"][:, :-1])                               # wrong shape: refused, nothing changed
    p.solve_resident(); _same_bits(p.download(), with_cost)
    p.close(); m.close()
