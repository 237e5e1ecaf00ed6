"""Predicted state and output trajectories of a resident batch on device (mld_predict_batch, GpuProblem.trajectories): the variables the reference
builds after every solve(), gen_state_output_vars (controllers/components/variables.py:246-286).  Checked: the three kernel paths (k_trajectory fp64 /
fp32, k_trajectory_valu) against fp64 numpy on condense_np maps with caller-supplied plans; a solved cfg3 batch against numpy, the step-0 output
formula and MpcController.predicted_trajectory(); the adjoint identity with the per-instance cost's pull-back; inputs that move (select, advance);
NaN rows for exactly the instances without a plan; the in-kernel hand-off; the states of the handle in which the call is refused.

Tolerances are those of tests/test_gpu_instance_cost.py::_check_pullback for the same GEMM paths: max abs error <= 1e-11 max|ref| in fp64 (MFMA and
VALU), <= 1e-5 max|ref| and > 1e-13 max|ref| under MLD_F32."""
import ctypes as C

import numpy as np
import pytest

import _paths
import condense_np as cn
from pyhybridcontrol_amd import gpu, host, synthetic as syn, _lib
from _traj_shapes import SHAPES, TV_SHAPE
from test_gpu_instance_cost import PATHS, SHAPES as COST_SHAPES

pytestmark = pytest.mark.gpu

# tests/_traj_shapes.py: the six shapes of the pull-back test, "ny0" and "odd3"
assert {k: SHAPES[k] for k in COST_SHAPES} == COST_SHAPES and len(SHAPES) == len(COST_SHAPES) + 2


def _ref(evo, v, x0, om):
    """x_tilde, y_tilde per instance (rows), fp64 numpy on the oracle's condensed maps"""
    x = v @ evo["Gamma_v"].T + x0 @ evo["Phi_x"].T + om @ evo["Gamma_omega"].T + evo["Gamma_5"][:, 0]
    y = v @ evo["L_v"].T + x0 @ evo["L_x"].T + om @ evo["L_omega"].T + evo["L_5"][:, 0]
    return x, y


def _check(got, ref, fp32, what="", only="xy"):
    """got / ref: (x, y); a family of width 0 only has its shape checked"""
    for name, g, r in zip(("x", "y"), got, ref):
        if name not in only:
            continue
        assert g.shape == r.shape, (what, name, g.shape, r.shape)
        if r.size == 0:
            continue
        scale, err = float(np.abs(r).max()), float(np.abs(g - r).max())
        print("%s %s: max|ref| %.3e err %.3e" % (what, name, scale, err))
        assert scale > 0 and np.all(np.isfinite(g)), (what, name)
        assert err <= (1e-5 if fp32 else 1e-11) * scale, (what, name, err / scale)
        if fp32:
            assert err > 1e-13 * scale, (what, name)          # the fp32 kernel really ran


def _raw(p, v, want_x, want_y):
    """the C entry itself (as tests/test_gpu_edges.py calls the ABI): x_out only / y_out only"""
    d, N = p.model.dims, p.N_tilde
    x = np.full((p.batch, N * d["nx"]), -7.0) if want_x else None
    y = np.full((p.batch, N * d["ny"]), -7.0) if want_y else None
    v = np.ascontiguousarray(v, dtype=np.float64)
    rc = _lib.load().mld_predict_batch(p._h, _lib.dptr(v), _lib.dptr(x), _lib.dptr(y))
    assert rc == 0, _lib.load().mld_last_error()
    return x, y


def _paths_case(mats_list, d, N, evos, path, seed, tv=False):
    rng = np.random.default_rng(seed)
    kw = dict(PATHS)[path]
    f32 = path == "mfma32"
    n, NX, NY, nx, nW = N * d["nv"], N * d["nx"], N * d["ny"], d["nx"], N * d["nomega"]
    m = gpu.GpuModel(mats_list, d, time_varying=tv)
    p = gpu.GpuProblem(m, N - 1, N, None, **kw)
    try:
        midx = rng.permutation(np.r_[np.zeros(170), np.full(130, 2)]).astype(np.int32)      # model 1 unused; partial groups of 42 and 2
        x0, om, v = rng.standard_normal((300, nx)), rng.standard_normal((300, nW)), rng.standard_normal((300, n))
        p.upload(x0, om, midx)
        rx, ry = np.zeros((300, NX)), np.zeros((300, NY))
        for k in (0, 2):
            s = midx == k
            rx[s], ry[s] = _ref(evos[k], v[s], x0[s], om[s])
        got = p.trajectories(v)                                  # no solve involved: the caller's plans
        assert set(got) == {"x", "y"}
        _check((got["x"], got["y"]), (rx, ry), f32, path + " both")
        if NX:
            gx, _ = _raw(p, v, True, False)
            _check((gx, None), (rx, None), f32, path + " x_out only", only="x")
        else:
            assert _lib.load().mld_predict_batch(p._h, _lib.dptr(v), _lib.dptr(np.zeros(1)), None) == -1 and b"nx = 0" in _lib.load().mld_last_error()
        if NY:
            _, gy = _raw(p, v, False, True)
            _check((None, gy), (None, ry), f32, path + " y_out only", only="y")
        else:
            assert _lib.load().mld_predict_batch(p._h, _lib.dptr(v), None, _lib.dptr(np.zeros(1))) == -1 and b"ny = 0" in _lib.load().mld_last_error()
        # a (n,) plan is broadcast
        one = p.trajectories(v[7])
        b1 = _ref(evos[0], np.tile(v[7], (300, 1))[midx == 0], x0[midx == 0], om[midx == 0])
        _check((one["x"][midx == 0], one["y"][midx == 0]), b1, f32, path + " broadcast")
        # one model, model_idx = None: two full groups and one of 44
        p.upload(x0, om)
        got = p.trajectories(v)
        _check((got["x"], got["y"]), _ref(evos[0], v, x0, om), f32, path + " one model")
    finally:
        p.close(); m.close()


@pytest.mark.parametrize("path", [p for p, _ in PATHS])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_kernel_paths_against_fp64_numpy(shape, path):
    """k_trajectory<false> (default), k_trajectory_valu (reserved bit 7), k_trajectory<true> (MLD_F32): 300 instances over three interleaved models
    with one unused, then one model without model_idx; both families, x_out only and y_out only"""
    N, dims = SHAPES[shape]
    d = _paths.make_dims(**dims)
    seed = 7000 + 10 * list(SHAPES).index(shape)
    mats = [_paths.random_mld(seed * 100000 + i, **dims)[0] for i in range(3)]
    _paths_case(mats, d, N, [cn.condense(a, N) for a in mats], path, seed)


@pytest.mark.parametrize("path", [p for p, _ in PATHS])
def test_kernel_paths_time_varying(path):
    """a time-varying handle (three horizons of independent step models): model_idx indexes horizons"""
    N, dims = TV_SHAPE
    horizons = [_paths.random_horizon(90 + i, N, **dims)[0] for i in range(3)]
    _paths_case(horizons, _paths.make_dims(**dims), N, [cn.condense_tv(h) for h in horizons], path, 7900, tv=True)


def test_valu_switch_selects_another_kernel():
    """reserved bit 7 must really select k_trajectory_valu: the two fp64 kernels sum in different orders (two MFMA accumulators over groups of four,
    chunk by chunk, against 64 strided partial sums and a shuffle tree), so on the same inputs they agree to rounding and are NOT bit-identical"""
    N, dims = SHAPES["straddle64"]
    d = _paths.make_dims(**dims)
    mats = [_paths.random_mld(777, **dims)[0]]
    rng = np.random.default_rng(779)
    x0, om, v = rng.standard_normal((200, d["nx"])), rng.standard_normal((200, N * d["nomega"])), rng.standard_normal((200, N * d["nv"]))
    got = {}
    for path in ("mfma64", "valu"):
        m = gpu.GpuModel(mats, d)
        p = gpu.GpuProblem(m, N - 1, N, None, **dict(PATHS)[path])
        try:
            p.upload(x0, om)
            t = p.trajectories(v)
            got[path] = np.hstack([t["x"], t["y"]])
        finally:
            p.close(); m.close()
    diff = np.abs(got["mfma64"] - got["valu"]).max()
    print("max |mfma64 - valu| = %.3e over %d entries, %d differ" % (diff, got["valu"].size, (got["mfma64"] != got["valu"]).sum()))
    assert diff <= 1e-11 * np.abs(got["valu"]).max()
    assert not np.array_equal(got["mfma64"], got["valu"])


# ------------------------------------------------------------------------------------------------------------------ solved batches
def _problem(name, batch, **opts):
    wl = syn.make_workload(name, batch=batch)
    ag = wl["agents"][0]
    d = ag["dims"]
    m = gpu.GpuModel([ag["mats"]], d)
    p = gpu.GpuProblem(m, wl["N_p"], wl["N_tilde"], host.cost_from_atoms(ag["atoms"], d, wl["N_p"], wl["N_tilde"]), **opts)
    return wl, ag, d, m, p


def _close_rows(got, ref, rows, what):
    """fp64 bound on the given rows of (x, y)"""
    for name, g, r in zip(("x", "y"), got, ref):
        scale, err = float(np.abs(r[rows]).max()), float(np.abs(g[rows] - r[rows]).max())
        print("%s %s: max|ref| %.3e err %.3e over %d rows" % (what, name, scale, err, np.count_nonzero(rows) if np.asarray(rows).dtype == bool else len(rows)))
        assert scale > 0 and err <= 1e-11 * scale, (what, name, err / scale)


def test_solved_batch_cfg3():
    """trajectories() of a solved cfg3 batch: numpy on the downloaded v; step 0 of y is C x + D1 u + D2 delta + D3 z + D4 omega + d5 (variables_k);
    one instance against MpcController.predicted_trajectory(); solve(..., trajectories=True) returns the same arrays"""
    import pyhybridcontrol_amd as phc
    B = 32
    wl, ag, d, m, p = _problem("cfg3", B, gap_rel=1e-4, max_nodes=2000)
    N, nx, ny, nv, nw = wl["N_tilde"], d["nx"], d["ny"], d["nu"] + d["ndelta"] + d["nz"] + d["nmu"], d["nomega"]
    x0, om = ag["x0"][:B], ag["omega"][:B]
    out = p.solve(x0, om, trajectories=True)
    assert set(out) >= {"v", "obj", "status", "x", "y", "stats"}
    plain = p.solve(x0, om)
    assert "x" not in plain and "y" not in plain and np.array_equal(plain["v"], out["v"])
    usable = np.isin(out["status"], (0, 2)) & np.isfinite(out["obj"])
    print("usable plans: %d of %d" % (usable.sum(), B))
    assert usable.sum() >= B - 2
    t = p.trajectories()
    assert t["x"].shape == (B, N * nx) and t["y"].shape == (B, N * ny)
    assert np.array_equal(t["x"], out["x"], equal_nan=True) and np.array_equal(t["y"], out["y"], equal_nan=True)
    evo = cn.condense(ag["mats"], N)
    ref = _ref(evo, out["v"], x0, om)
    _close_rows((t["x"], t["y"]), ref, usable, "cfg3 solved")
    assert np.all(np.isnan(t["x"][~usable])) and np.all(np.isnan(t["y"][~usable]))
    # step 0: the state is x_k itself, the output the MLD output equation
    def mat(name, cols):
        a = ag["mats"].get(name)
        return np.zeros((ny, cols)) if a is None or np.size(a) == 0 else np.asarray(a, np.float64).reshape(ny, cols)
    v0 = out["v"][:, :nv]
    o1, o2, o3 = d["nu"], d["nu"] + d["ndelta"], d["nu"] + d["ndelta"] + d["nz"]
    y0 = x0 @ mat("C", nx).T + v0[:, :o1] @ mat("D1", d["nu"]).T + v0[:, o1:o2] @ mat("D2", d["ndelta"]).T + v0[:, o2:o3] @ mat("D3", d["nz"]).T \
        + om[:, :nw] @ mat("D4", nw).T + mat("d5", 1).T
    ys = float(np.abs(ref[1][usable]).max())
    assert np.abs(t["y"][usable, :ny] - y0[usable]).max() <= 1e-11 * ys
    assert np.abs(t["x"][usable, :nx] - x0[usable]).max() <= 1e-11 * float(np.abs(ref[0][usable]).max())
    # the single-instance host route: a controller on the same agent; its plan evaluated by the batch kernel under instance 0's inputs
    ctrl = phc.MpcController(phc.MldModel(nu_l=d["nu_l"], ts=900, **{k: v for k, v in ag["mats"].items()}), N_p=wl["N_p"])
    ctrl.set_std_obj_atoms(**ag["atoms"])
    ctrl.build()
    ctrl.solve(0, x_k=x0[0], omega_tilde_k=om[0], MIPGap=1e-4, NodeLimit=2000)
    cx, cy = ctrl.predicted_trajectory()
    vc = np.asarray(ctrl.v_N_tilde, np.float64).ravel()
    assert vc.shape == (p.n,)
    tc = p.trajectories(vc)
    assert np.abs(tc["x"][0] - cx.ravel()).max() <= 1e-11 * np.abs(cx).max() and np.abs(tc["y"][0] - cy.ravel()).max() <= 1e-11 * np.abs(cy).max()
    p.close(); m.close()


@pytest.mark.parametrize("shape", ["straddle64", "k380", "odd3"])
def test_adjoint_identity_with_the_instance_cost(shape):
    """k_inst_pullback computes q = Gamma_v' lin_x + L_v' lin_y and the constant; k_trajectory the forward product: for any v
    lin_x . x_tilde + lin_y . y_tilde = q . v + const.  The two kernels were written independently and must agree to 1e-11 of the sum of |terms|."""
    N, dims = SHAPES[shape]
    d = _paths.make_dims(**dims)
    rng = np.random.default_rng(8100 + len(shape))
    mats = [_paths.random_mld(8200 + i, **dims)[0] for i in range(3)]
    m = gpu.GpuModel(mats, d)
    p = gpu.GpuProblem(m, N - 1, N, None)
    try:
        B = 200
        midx = rng.integers(0, 3, B).astype(np.int32)
        x0, om, v = rng.standard_normal((B, d["nx"])), rng.standard_normal((B, N * d["nomega"])), rng.standard_normal((B, N * d["nv"]))
        lx, ly = rng.standard_normal((B, N * d["nx"])), rng.standard_normal((B, N * d["ny"]))
        p.upload(x0, om, midx)
        p.upload_instance_cost(lin_x=lx, lin_y=ly)
        ic = p.instance_cost()
        t = p.trajectories(v)
        lhs = np.einsum("bi,bi->b", lx, t["x"]) + np.einsum("bi,bi->b", ly, t["y"])
        rhs = np.einsum("bi,bi->b", ic["q"], v) + ic["const"]
        terms = np.abs(lx * t["x"]).sum(1) + np.abs(ly * t["y"]).sum(1) + np.abs(ic["q"] * v).sum(1) + np.abs(ic["const"])
        rel = np.abs(lhs - rhs) / terms
        print("%s: worst |lhs - rhs| / sum|terms| = %.3e" % (shape, rel.max()))
        assert np.all(terms > 0) and rel.max() <= 1e-11
    finally:
        p.close(); m.close()


def _half_without_a_plan(p, ag, B):
    """solve once to the optimum, then give every second instance a cutoff just below its own optimum ("nothing better exists": INFEASIBLE,
    objective +inf, tests/test_gpu_handoff.py:41) and the others +inf; returns (masked instances, the second solve's download)"""
    ref = p.solve(ag["x0"][:B], ag["omega"][:B])
    assert np.all(ref["status"] == 0)
    p.upload(ag["x0"][:B], ag["omega"][:B])
    cut = np.full(B, np.inf)
    masked = np.arange(B) % 2 == 1
    cut[masked] = (ref["obj"] - 1e-6 * np.maximum(1.0, np.abs(ref["obj"])))[masked]
    p.set_cutoffs(cut)
    p.solve_resident()
    out = p.download()
    assert np.all(out["status"][masked] == 1) and np.all(out["status"][~masked] == 0)
    return masked, out


def test_inputs_that_move():
    """select(k): the result with a given v follows set k.  advance(): v=None is refused and the handle stays usable; for a time-invariant model the
    new x0 of every advanced instance is step 1 of the previous x_tilde (1e-11 max|x|: k_advance and k_trajectory sum in different orders); skipped
    instances keep their state"""
    B = 16
    wl, ag, d, m, p = _problem("cfg2", 2 * B, gap_rel=0.0, max_nodes=100000)
    N, nx = wl["N_tilde"], d["nx"]
    evo = cn.condense(ag["mats"], N)
    rng = np.random.default_rng(8300)
    v = rng.standard_normal((B, p.n))
    X, W = np.stack([ag["x0"][:B], ag["x0"][B:]]), np.stack([ag["omega"][:B], ag["omega"][B:]])
    p.upload(X[0], W[0]); p.stage(X, W)
    for k in (1, 0, 1):
        p.select(k)
        t = p.trajectories(v)
        _check((t["x"], t["y"]), _ref(evo, v, X[k], W[k]), False, "set %d" % k)
        with pytest.raises(gpu.MldGpuError, match="not been solved"):
            p.trajectories()                                   # a selection leaves no plan of the current inputs
    assert not np.array_equal(_ref(evo, v, X[0], W[0])[0], _ref(evo, v, X[1], W[1])[0])
    masked, out = _half_without_a_plan(p, ag, B)
    t = p.trajectories()
    x_old, w_old = p.inputs()
    assert p.advance() == masked.sum()
    with pytest.raises(gpu.MldGpuError, match="moved the inputs on"):
        p.trajectories()
    x_new, w_new = p.inputs()
    xs = float(np.nanmax(np.abs(t["x"])))
    err = np.abs(x_new[~masked] - t["x"][~masked, nx:2 * nx]).max()
    print("advance: max|x| %.3e, worst |x0_new - x_tilde[step 1]| %.3e over %d instances" % (xs, err, (~masked).sum()))
    assert err <= 1e-11 * xs
    assert np.array_equal(x_new[masked], x_old[masked]) and np.array_equal(w_new[masked], w_old[masked])
    assert not np.array_equal(x_new[~masked], x_old[~masked])
    t2 = p.trajectories(v)                                     # the caller's plans under the advanced inputs: valid without a solve
    _check((t2["x"], t2["y"]), _ref(evo, v, x_new, w_new), False, "after advance")
    p.solve_resident()
    t3, o3 = p.trajectories(), p.download()
    ok = np.isin(o3["status"], (0, 2)) & np.isfinite(o3["obj"])
    assert ok.sum() >= B // 2
    _close_rows((t3["x"], t3["y"]), _ref(evo, o3["v"], x_new, w_new), ok, "next step")
    p.close(); m.close()


@pytest.mark.parametrize("path", ["mfma64", "valu"])
def test_instances_without_a_plan_get_nan_rows(path):
    """half of the batch ends INFEASIBLE under a cutoff below its own optimum: exactly those rows are NaN in every element, they are exactly the
    instances advance() skips, and every other row matches numpy"""
    B = 16
    wl, ag, d, m, p = _problem("cfg2", B, gap_rel=0.0, max_nodes=100000, **dict(PATHS)[path])
    evo = cn.condense(ag["mats"], wl["N_tilde"])
    masked, out = _half_without_a_plan(p, ag, B)
    t = p.trajectories()
    for name in ("x", "y"):
        nan_rows = np.isnan(t[name]).any(axis=1)
        assert np.array_equal(nan_rows, masked), (name, np.flatnonzero(nan_rows))           # the set of NaN rows IS the set given a cutoff
        assert np.all(np.isnan(t[name][masked])) and np.all(np.isfinite(t[name][~masked]))  # every element of a masked row, none of the others
    _close_rows((t["x"], t["y"]), _ref(evo, out["v"], ag["x0"][:B], ag["omega"][:B]), ~masked, "unmasked rows")
    tv = p.trajectories(out["v"])                              # the same plans passed in: no masking
    assert np.all(np.isfinite(tv["x"])) and np.all(np.isfinite(tv["y"]))
    assert np.array_equal(tv["x"][~masked], t["x"][~masked]) and np.array_equal(tv["y"][~masked], t["y"][~masked])
    assert p.advance() == masked.sum() == B // 2
    p.close(); m.close()


def test_in_kernel_handoff():
    """with the hand-off on the result arrays hold the instances, then the items: trajectories() has `batch` rows, read after the device merge"""
    B = 48
    wl, ag, d, m, p = _problem("cfg2", B, gap_rel=0.0, max_nodes=100000, cut_rounds=1)
    evo = cn.condense(ag["mats"], wl["N_tilde"])
    x0, om = ag["x0"][:B], ag["omega"][:B]
    ho = dict(sub_nodes=12, max_gen=8, max_children=64, max_tree=100000, room_factor=64.0)
    p.set_opts(max_nodes=3)
    p.set_handoff(True, **ho)
    p.upload(x0, om)
    p.solve_resident()
    assert p.handoff_stats()["items"] >= 3
    t, out = p.trajectories(), p.download()
    assert t["x"].shape[0] == B and t["y"].shape[0] == B and np.all(out["status"] == 0)
    _close_rows((t["x"], t["y"]), _ref(evo, out["v"], x0, om), np.ones(B, bool), "hand-off on")
    p.set_handoff(False)
    p.set_opts(max_nodes=100000)
    # the convenience call reads the trajectories before it drops the resident batch
    o2 = p.solve_handoff_device(x0, om, first_nodes=3, trajectories=True, **ho)
    assert o2["handoff"]["items"] >= 3 and o2["x"].shape == t["x"].shape
    _close_rows((o2["x"], o2["y"]), _ref(evo, o2["v"], x0, om), np.ones(B, bool), "solve_handoff_device")
    assert "x" not in p.solve_handoff_device(x0, om, first_nodes=3, **ho)
    p.close(); m.close()


def test_handle_states():
    B = 16
    wl, ag, d, m, p = _problem("cfg2", B, gap_rel=1e-4, max_nodes=2000)
    evo = cn.condense(ag["mats"], wl["N_tilde"])
    lib = _lib.load()
    x0, om = ag["x0"][:B], ag["omega"][:B]
    v = np.random.default_rng(8400).standard_normal((B, p.n))
    xb, yb = np.zeros((B, wl["N_tilde"] * d["nx"])), np.zeros((B, wl["N_tilde"] * d["ny"]))
    # before any upload
    assert lib.mld_predict_batch(p._h, _lib.dptr(v), _lib.dptr(xb), _lib.dptr(yb)) == -1 and b"no batch resident" in lib.mld_last_error()
    assert lib.mld_predict_batch(p._h, None, _lib.dptr(xb), _lib.dptr(yb)) == -1
    # uploaded, not solved: the resident solution is refused, a caller's plan is fine
    p.upload(x0, om)
    with pytest.raises(gpu.MldGpuError, match="not been solved"):
        p.trajectories()
    t = p.trajectories(v)
    _check((t["x"], t["y"]), _ref(evo, v, x0, om), False, "before any solve")
    # between launch and finish: refused either way, nothing written; fine after finish()
    p.launch()
    xb[:] = -3.0
    with pytest.raises(gpu.MldGpuError, match="not been finished"):
        p.trajectories(v)
    with pytest.raises(gpu.MldGpuError, match="not been finished"):
        p.trajectories()
    assert lib.mld_predict_batch(p._h, _lib.dptr(v), _lib.dptr(xb), None) == -1 and np.all(xb == -3.0)
    p.finish()
    out, t = p.download(), p.trajectories()
    ok = np.isin(out["status"], (0, 2)) & np.isfinite(out["obj"])
    assert ok.sum() >= B - 2
    _close_rows((t["x"], t["y"]), _ref(evo, out["v"], x0, om), ok, "after finish")
    # nothing asked for: accepted, nothing done
    assert lib.mld_predict_batch(p._h, _lib.dptr(v), None, None) == 0
    p.close(); m.close()
