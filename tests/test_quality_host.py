"""Host side of the solution quality (mld_evaluate_batch, GpuProblem.evaluate): the entry point is declared, listed and exported; the shape checks
(made before any C call); the absence of a CPU fallback; the causal structure of the condensed constraint maps that k_evaluate's skip relies on --
every block the kernel leaves out is exactly zero; and the numpy reference of tests/_quality_ref.py against facts: solved oracle instances and a
plan with a known violation.  No GPU needed."""
import os
import re
import types

import numpy as np
import pytest

import _paths
import _quality_ref as qr
import _tv
import condense_np as cn
import orc
from pyhybridcontrol_amd import gpu, synthetic as syn, _lib
from _traj_shapes import SHAPES, TV_SHAPE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the two shapes tests/test_gpu_quality.py adds to those of tests/_traj_shapes.py
EXTRA_SHAPES = {
    "n300": (25, dict(nx=3, nu=10, ndelta=1, nz=1, nomega=2, ny=2, nc=3)),                # n = 300: two chunks of H_v alone; m0 = 75: a partial last block
    "bounds": (6, dict(nx=3, nu=3, ndelta=2, nz=1, nmu=4, nomega=2, ny=1, nc=4)),         # (with nu_l = 2: binaries inside u, bounded mu)
}
ALL_SHAPES = dict(SHAPES, **EXTRA_SHAPES)


def test_evaluate_batch_is_declared_listed_and_exported():
    with open(os.path.join(ROOT, "include", "mldgpu.h")) as f:
        header = f.read()
    ws = r"\s*"
    args = [r"mld_problem_t\s*\*", r"const\s+double\s*\*\s*v", r"int\s+n_cols", r"const\s+double\s*\*\s*omega_cols", r"const\s+int32_t\s*\*\s*col_rows",
            r"const\s+double\s*\*\s*x_cols", r"double\s*\*\s*obj_out", r"double\s*\*\s*constr_vio_out", r"int32_t\s*\*\s*constr_row_out",
            r"double\s*\*\s*int_vio_out", r"double\s*\*\s*bound_vio_out"]
    assert re.search(r"\bint\s+mld_evaluate_batch\s*\(" + ws + (ws + "," + ws).join(args) + ws + r"\)\s*;", header)
    assert "controller_base.py:509" in header and "controller_base.py:411-456" in header       # declared with the reference lines it replaces
    assert "MLD_F32" in header[header.index("Solution quality of the resident batch"):header.index("int mld_evaluate_batch")]   # fp64 whatever the handle
    assert "mld_evaluate_batch" in _lib.EXPORTS
    fn = _lib.load().mld_evaluate_batch
    assert fn.argtypes is not None and len(fn.argtypes) == 11
    assert _lib.version().startswith("mldgpu 0.6 ") and "solution quality" in _lib.version()


def _shell(batch, nx=3, nw=2, nv=11, N=5):
    """a GpuProblem without a handle: what the shape checks read"""
    p = gpu.GpuProblem.__new__(gpu.GpuProblem)
    p.model = types.SimpleNamespace(dims=dict(nx=nx, ny=1, nomega=nw), nv=nv)
    p.N_tilde, p.n, p.nW, p.batch, p._h = N, N * nv, N * nw, batch, None
    return p


def test_shape_errors_raise_before_any_c_call():
    p = _shell(4)
    n_cols, oc, cr, xc = p._column_arrays(np.ones((4, 3, 10)), [20, 10, 0], np.ones((4, 3, 3)))
    assert n_cols == 3 and oc.shape == (4, 3, 10) and cr.dtype == np.int32 and xc.shape == (4, 3, 3)
    assert p._column_arrays() == (0, None, None, None)
    for bad in (np.ones(54), np.ones((3, 55)), np.ones((4, 55, 1))):
        with pytest.raises(ValueError, match="v has shape"):
            p.evaluate(v=bad)                        # (_h is None: a C call would have raised MldGpuError instead)
    for bad in (np.ones((4, 3, 9)), np.ones((3, 3, 10)), np.ones((4, 30)), np.ones((4, 0, 10))):
        with pytest.raises(ValueError, match=r"omega_cols has shape \(%s\)" % ", ".join(map(str, bad.shape))):
            p.evaluate(v=np.ones(55), omega_cols=bad)
    for bad in (np.ones((4, 2, 3)), np.ones((4, 3, 4)), np.ones((4, 9))):
        with pytest.raises(ValueError, match=r"x_cols has shape \(%s\)" % ", ".join(map(str, bad.shape))):
            p.evaluate(v=np.ones(55), omega_cols=np.ones((4, 3, 10)), x_cols=bad)
    for bad in ([1, 2], [[1, 2, 3]], [1.0, 2.0, 3.0]):
        with pytest.raises(ValueError, match="col_rows has shape"):
            p.evaluate(v=np.ones(55), omega_cols=np.ones((4, 3, 10)), col_rows=bad)
    with pytest.raises(ValueError, match="col_rows given without columns"):
        p.evaluate(v=np.ones(55), col_rows=[1])
    with pytest.raises(ValueError, match="x_cols given without omega_cols"):
        p.evaluate(v=np.ones(55), x_cols=np.ones((4, 3, 3)))
    with pytest.raises(ValueError, match="no state"):
        _shell(4, nx=0).evaluate(v=np.ones(55), omega_cols=np.ones((4, 3, 10)), x_cols=np.ones((4, 3, 0)))


def test_no_cpu_fallback_for_the_quality():
    expect = "no HIP device" if _lib.device_count() <= 0 else "no batch resident"
    with pytest.raises(gpu.MldGpuError, match=expect):
        _shell(4).evaluate(v=np.ones(55))
    with pytest.raises(gpu.MldGpuError, match=expect):
        _shell(4).evaluate()
    with pytest.raises(gpu.MldGpuError, match=expect):
        _shell(4).evaluate(v=np.ones(55), omega_cols=np.ones((4, 2, 10)))


def _assert_causal(evo, N, d, what):
    """block (i, j) of H_v and H_omega is exactly zero for j > i: the rows of step i see the inputs of the steps up to i.  That is what k_evaluate skips."""
    for name, cols in (("H_v", d["nv"]), ("H_omega", d["nomega"])):
        M = np.asarray(evo[name])
        assert M.shape == (N * d["nc"], N * cols), (what, name, M.shape)
        if M.size == 0:
            continue
        B = M.reshape(N, d["nc"], N, cols)
        seen = 0
        for i in range(N):
            for j in range(i + 1, N):
                assert not np.any(B[i, :, j, :]), (what, name, i, j)          # exactly 0.0: not a tolerance
                seen += 1
        assert seen == N * (N - 1) // 2
        assert np.any(M), (what, name)                                        # (the map is not simply empty)
        assert all(np.any(B[i, :, i, :]) for i in range(N)), (what, name)     # and the diagonal blocks, which are NOT skipped, are there


@pytest.mark.parametrize("shape", list(ALL_SHAPES))
def test_causal_zero_blocks_of_the_constraint_maps(shape):
    N, dims = ALL_SHAPES[shape]
    d = _paths.make_dims(**dims)
    for i in range(3):
        _assert_causal(cn.condense(_paths.random_mld(4321 + i, **dims)[0], N), N, d, shape)


def test_causal_zero_blocks_of_time_varying_horizons():
    N, dims = TV_SHAPE
    _assert_causal(cn.condense_tv(_paths.random_horizon(90, N, **dims)[0]), N, _paths.make_dims(**dims), "random horizon")
    wl = syn.make_workload("cfg2", batch=1)
    ag = wl["agents"][0]
    N = wl["N_tilde"]
    d = dict(ag["dims"])
    d["nv"] = d["nu"] + d["ndelta"] + d["nz"] + d["nmu"]
    _assert_causal(cn.condense_tv(_tv.step_models(ag["mats"], N, seed=3)), N, d, "_tv.step_models")
    _assert_causal(cn.condense(ag["mats"], N), N, d, "cfg2")


# ---- the reference against facts ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [3, 11])
def test_reference_on_a_solved_oracle_instance(seed):
    """a point the oracle proves optimal: integral, feasible for the rows to 1e-6 of the row's largest coefficient, and its objective is the oracle's"""
    N = 4
    mats, dims, atoms, rng = _paths.fuzz_mld(seed)
    sf = cn.standard_form(mats, atoms, N, N, nu_l=dims["nu_l"], nmu_l=dims["nmu_l"])
    d = sf["dims"]
    x0, om = 0.5 * rng.standard_normal(d["nx"]), 0.5 * rng.standard_normal(N * d["nomega"])
    q, h, r = cn.lin_cost(sf["cost"], x0, om), cn.rhs(sf["evo"], x0, om), cn.cost_const(sf["cost"]["const_terms"], x0, om)
    sol = orc.solve_milp(q, sf["G"], h, sf["lb"], sf["ub"], sf["is_bin"], presolve=0)
    assert sol["status"] == "optimal"
    ref = dict(evo=sf["evo"], is_bin=sf["is_bin"], lb=sf["lb"], ub=sf["ub"])
    out = qr.quality(ref, sol["x"], x0, om, cost=sf["cost"])
    assert out["int_vio"][0] == 0.0
    row = int(out["constr_row"][0])
    assert out["constr_vio"][0] == out["R"][0, 0, row] == out["R"][0, 0].max()
    assert out["constr_vio"][0] <= 1e-6 * max(1.0, np.abs(sf["G"][row]).max())
    assert out["bound_vio"][0] <= 1e-9
    assert abs(out["obj"][0] - (sol["obj"] + r)) <= 1e-9 * max(1.0, abs(sol["obj"] + r))
    assert out["S"][0] > 0 and out["obj_scale"][0] >= abs(out["obj"][0])
    # the same columns passed explicitly, one restricted to its first rows, one to none
    m0 = sf["G"].shape[0]
    oc = np.tile(om, (1, 3, 1))
    cols = qr.quality(ref, sol["x"], x0, om, omega_cols=oc, col_rows=[m0, m0 // 2, 0], cost=sf["cost"])
    assert cols["constr_vio"].shape == (1, 3) and cols["constr_vio"][0, 0] == out["constr_vio"][0]
    assert cols["constr_vio"][0, 1] == out["R"][0, 0, :m0 // 2].max() and cols["constr_row"][0, 1] < m0 // 2
    assert cols["constr_vio"][0, 2] == -np.inf and cols["constr_row"][0, 2] == -1


def test_reference_reports_known_violations_exactly():
    N, dims = EXTRA_SHAPES["bounds"]
    d = _paths.make_dims(**dims)
    d["nu_l"] = 2
    ref = qr.model_ref(_paths.random_mld(5, **dims)[0], d, N)
    nv, omu = d["nv"], d["nu"] + d["ndelta"] + d["nz"]
    assert ref["is_bin"].sum() == N * 4 and np.isfinite(ref["lb"]).sum() == N * (4 + 4)
    v = np.zeros(N * nv)
    v[ref["is_bin"]] = np.tile([1.0, 0.0, 1.0, 1.0], N)
    v[2 * nv + 0] = -123.0                                   # a free input: no bound, not integer
    assert np.array_equal(qr.point_quality(ref["is_bin"], ref["lb"], ref["ub"], v), (np.zeros(1), np.zeros(1)))
    v[3 * nv + d["nu"] - 1] = 0.25                           # a binary inside u
    v[4 * nv + omu + 1] = -0.5                               # a mu below its bound
    iv, bv = qr.point_quality(ref["is_bin"], ref["lb"], ref["ub"], v)
    assert iv[0] == 0.25 and bv[0] == 0.5
    v[nv + d["nu"]] = 1.75                                   # a delta above 1: 0.75 over the bound, 0.25 from the nearest integer
    iv, bv = qr.point_quality(ref["is_bin"], ref["lb"], ref["ub"], v)
    assert iv[0] == 0.25 and bv[0] == 0.75
    # no binaries, nothing bounded
    d0 = _paths.make_dims(nx=2, nu=2, nz=1, nomega=1, ny=1, nc=2)
    r0 = qr.model_ref(_paths.random_mld(6, nx=2, nu=2, nz=1, nomega=1, ny=1, nc=2)[0], d0, 3)
    assert np.array_equal(qr.point_quality(r0["is_bin"], r0["lb"], r0["ub"], -7.3 * np.ones(9)), (np.zeros(1), np.zeros(1)))


def test_reference_objective_is_the_cost_at_the_point():
    """objective() restates 1/2 v'Pv + q'v + r: against a direct evaluation of the atoms on the trajectories the maps give"""
    N, dims = SHAPES["straddle64"]
    d = _paths.make_dims(**dims)
    evo = cn.condense(_paths.random_mld(77, **dims)[0], N)
    c = _paths.random_cost(78, d, N)
    rng = np.random.default_rng(79)
    B = 3
    v, x0, om = rng.standard_normal((B, N * d["nv"])), rng.standard_normal((B, d["nx"])), rng.standard_normal((B, N * d["nomega"]))
    inst = dict(lin_v=rng.standard_normal((B, N * d["nv"])), lin_x=rng.standard_normal((B, N * d["nx"])), lin_y=rng.standard_normal((B, N * d["ny"])))
    obj, scale = qr.objective(evo, qr.cost_of(evo, **c), v, x0, om, inst)
    x = v @ evo["Gamma_v"].T + x0 @ evo["Phi_x"].T + om @ evo["Gamma_omega"].T + evo["Gamma_5"][:, 0]
    y = v @ evo["L_v"].T + x0 @ evo["L_x"].T + om @ evo["L_omega"].T + evo["L_5"][:, 0]
    for b in range(B):
        direct = sum((c["lin_" + k] + inst["lin_" + k][b]) @ t[b] + t[b] @ c["quad_" + k] @ t[b] for k, t in (("v", v), ("x", x), ("y", y)))
        assert abs(obj[b] - direct) <= 1e-12 * scale[b] and scale[b] >= abs(direct)
