"""Solution quality of a resident batch on device (mld_evaluate_batch, GpuProblem.evaluate): ObjVal / ConstrVio / IntVio / BoundVio of the reference's
backend (controllers/controller_base.py:509) for resident or caller-supplied plans, on the ORIGINAL rows, as posed or under validation columns
(the layout of controller_base.py:411-456).  Checked against the fp64 numpy reference of tests/_quality_ref.py: the kernel paths (k_evaluate,
k_evaluate_valu, and k_evaluate on a handle created with MLD_F32 -- the arithmetic is fp64 whatever the handle) with random plans; time-varying
horizons; quadratic and per-instance costs; solved batches; constraint blocks; instances without a plan; the in-kernel hand-off; handle states.

Tolerances: constr_vio within 1e-11 S of the reference, S the row scale max_i (|H_v||v| + |H_x||x| + |H_omega||omega| + |H_5|)_i; obj within 1e-11 of
the sum of the absolute terms of the objective (the project's standing fp64 GEMM tolerance, tests/test_gpu_instance_cost.py::_check_pullback, about
60 x the gamma_K bound of a 1 400-term fp64 dot); int_vio and bound_vio bit for bit; constr_row not by index -- the reference residual at the returned
row must be within the same tolerance of the reference maximum, and the row must lie inside the column's col_rows."""
import ctypes as C
import functools

import numpy as np
import pytest

import _paths
import _quality_ref as qr
import condense_np as cn
from pyhybridcontrol_amd import gpu, host, synthetic as syn, _lib
from _traj_shapes import SHAPES, TV_SHAPE
from test_gpu_instance_cost import PATHS
from test_gpu_trajectories import _half_without_a_plan, _problem
from test_gpu_blocks import _draw_profiles

pytestmark = pytest.mark.gpu

TOL = 1e-11
ALL_SHAPES = dict(SHAPES)
ALL_SHAPES["n300"] = (25, dict(nx=3, nu=10, ndelta=1, nz=1, nomega=2, ny=2, nc=3))          # n = 300: two chunks of H_v alone; m0 = 75: partial last block
ALL_SHAPES["bounds"] = (6, dict(nx=3, nu=3, ndelta=2, nz=1, nmu=4, nomega=2, ny=1, nc=4))   # with nu_l = 2: binaries inside u; bounded mu
assert len(ALL_SHAPES) == 10
B0 = 300


def _dims(shape, dims):
    d = _paths.make_dims(**dims)
    if shape == "bounds":
        d["nu_l"] = 2
    return d


# ---- comparison ------------------------------------------------------------------------------------------------------------------------------
def _check_constr(vio, row, R, S, rows, what):
    """vio / row (B, C) from the device; R (B, C, m0) reference residuals, S (B, C) row scales, rows (C) leading rows of every column"""
    vio, row = np.asarray(vio).reshape(S.shape), np.asarray(row).reshape(S.shape)
    worst = 0.0
    for c, r in enumerate(rows):
        if r == 0:
            assert np.all(np.isneginf(vio[:, c])) and np.all(row[:, c] == -1), (what, c)
            continue
        ref = R[:, c, :r].max(axis=1)
        assert np.all(S[:, c] > 0) and np.all(np.isfinite(vio[:, c])), (what, c)
        err = np.abs(vio[:, c] - ref) / S[:, c]
        worst = max(worst, float(err.max()))
        assert err.max() <= TOL, (what, "constr_vio", c, err.max())
        assert np.all((row[:, c] >= 0) & (row[:, c] < r)), (what, "constr_row outside col_rows", c)
        at = R[np.arange(R.shape[0]), c, row[:, c]]
        assert np.all(np.abs(at - ref) <= TOL * S[:, c]), (what, "constr_row", c)
    return worst


def _check(got, ref, what, sel=None):
    """got: evaluate()'s dict; ref: qr.quality's; sel: the instances to compare (default all)"""
    B = ref["obj"].shape[0]
    sel = np.ones(B, bool) if sel is None else sel
    assert set(got) == {"obj", "constr_vio", "constr_row", "int_vio", "bound_vio"}
    assert got["constr_vio"].shape == ref["constr_vio"].shape == got["constr_row"].shape and got["constr_row"].dtype == np.int32
    S = ref["S"].reshape(B, -1)
    worst = _check_constr(got["constr_vio"].reshape(B, -1)[sel], got["constr_row"].reshape(B, -1)[sel], ref["R"][sel], S[sel], ref["rows"], what)
    oerr = np.abs(got["obj"] - ref["obj"])[sel] / np.maximum(ref["obj_scale"][sel], np.finfo(float).tiny)
    print("%s: constr_vio worst err / S %.2e, obj worst err / scale %.2e" % (what, worst, oerr.max()))
    assert np.all(np.abs(got["obj"] - ref["obj"])[sel] <= TOL * ref["obj_scale"][sel]), (what, "obj", oerr.max())
    assert np.array_equal(got["int_vio"][sel], ref["int_vio"][sel]), (what, "int_vio")
    assert np.array_equal(got["bound_vio"][sel], ref["bound_vio"][sel]), (what, "bound_vio")
    assert np.all(got["bound_vio"][sel] >= 0) and np.all(got["int_vio"][sel] >= 0)


def _by_model(refs, midx, v, x0, om, **kw):
    """qr.quality per model of an interleaved batch, put back in batch order"""
    out = None
    for k in np.unique(midx):
        s = midx == k
        sub = {a: (b[s] if isinstance(b, np.ndarray) and b.shape[:1] == s.shape and a != "col_rows" else b) for a, b in kw.items()}
        if sub.get("inst"):
            sub["inst"] = {a: b[s] for a, b in sub["inst"].items()}
        if isinstance(sub.get("cost"), list):
            sub["cost"] = sub["cost"][k]
        q = qr.quality(refs[k], v[s], x0[s], om[s], **sub)
        if out is None:
            out = {a: (np.zeros((len(midx),) + b.shape[1:], b.dtype) if a != "rows" else b) for a, b in q.items()}
        for a, b in q.items():
            if a != "rows":
                out[a][s] = b
    return out


_IP = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32)) if a is not None else None


def _raw_alone(p, v, ref, what, n_cols=0, oc=None, cr=None, xc=None):
    """the C entry itself, every output requested alone"""
    lib, B = _lib.load(), p.batch
    shp = (B, n_cols) if n_cols else (B,)
    for k in range(5):
        bufs = [np.full(B, -7.0), np.full(shp, -7.0), np.full(shp, -7, np.int32), np.full(B, -7.0), np.full(B, -7.0)]
        args = [None] * 5
        args[k] = _IP(bufs[k]) if k == 2 else _lib.dptr(bufs[k])
        rc = lib.mld_evaluate_batch(p._h, _lib.dptr(v), n_cols, _lib.dptr(oc), _IP(cr), _lib.dptr(xc), *args)
        assert rc == 0, lib.mld_last_error()
        S, R = ref["S"].reshape(B, -1), ref["R"]
        if k == 0:
            assert np.all(np.abs(bufs[0] - ref["obj"]) <= TOL * ref["obj_scale"]), (what, "obj alone")
        elif k == 1:
            fin = np.isfinite(ref["constr_vio"])
            assert np.all(np.abs(bufs[1][fin] - ref["constr_vio"][fin]) <= TOL * ref["S"][fin]) and np.all(np.isneginf(bufs[1][~fin])), (what, "constr_vio alone")
        elif k == 2:
            rows = bufs[2].reshape(B, -1)
            for c, r in enumerate(ref["rows"]):
                if r == 0:
                    assert np.all(rows[:, c] == -1)
                    continue
                assert np.all((rows[:, c] >= 0) & (rows[:, c] < r)), (what, "constr_row alone")
                assert np.all(np.abs(R[np.arange(B), c, rows[:, c]] - R[:, c, :r].max(axis=1)) <= TOL * S[:, c]), (what, "constr_row alone")
        elif k == 3:
            assert np.array_equal(bufs[3], ref["int_vio"]), (what, "int_vio alone")
        else:
            assert np.array_equal(bufs[4], ref["bound_vio"]), (what, "bound_vio alone")
    assert lib.mld_evaluate_batch(p._h, _lib.dptr(v), n_cols, _lib.dptr(oc), _IP(cr), _lib.dptr(xc), None, None, None, None, None) == 0      # nothing asked for


@functools.lru_cache(maxsize=None)
def _case(shape, tv=False):
    """models, inputs and every numpy reference of one shape: computed once, shared by the three paths, never changed"""
    N, dims = TV_SHAPE if tv else ALL_SHAPES[shape]
    d = _dims(shape, dims)
    seed = 9000 + 10 * (len(ALL_SHAPES) if tv else list(ALL_SHAPES).index(shape))
    if tv:
        mats = [_paths.random_horizon(190 + i, N, **dims)[0] for i in range(3)]
    else:
        mats = [_paths.random_mld(seed * 100000 + i, **dims)[0] for i in range(3)]
    refs = [qr.model_ref(a, d, N) for a in mats]
    rng = np.random.default_rng(seed)
    n, nx, nW, m0 = N * d["nv"], d["nx"], N * d["nomega"], N * d["nc"]
    midx = rng.permutation(np.r_[np.zeros(170), np.full(130, 2)]).astype(np.int32)      # model 1 unused; partial groups of 42 and 2
    x0, om, v = rng.standard_normal((B0, nx)), rng.standard_normal((B0, nW)), rng.standard_normal((B0, n))
    v[::7] = np.rint(v[::7])                                                              # (some plans integral: int_vio exactly 0 there)
    oc, xc = rng.standard_normal((B0, 3, nW)), rng.standard_normal((B0, 3, nx))
    cr = np.array([m0, m0 // 2, 0], np.int32)
    c = dict(N=N, d=d, mats=mats, refs=refs, midx=midx, x0=x0, om=om, v=v, oc=oc, xc=xc, cr=cr)
    c["posed"] = _by_model(refs, midx, v, x0, om)
    c["cols"] = _by_model(refs, midx, v, x0, om, omega_cols=oc, col_rows=cr)
    c["xcols"] = _by_model(refs, midx, v, x0, om, omega_cols=oc, col_rows=cr, x_cols=xc) if nx else None
    c["one"] = qr.quality(refs[0], v, x0, om)
    c["one_cols"] = qr.quality(refs[0], v, x0, om, omega_cols=oc, col_rows=cr)
    for k in ("midx", "x0", "om", "v", "oc", "xc", "cr"):
        c[k].setflags(write=False)
    return c


def _paths_case(c, path, tv=False):
    kw = dict(PATHS)[path]
    N, d = c["N"], c["d"]
    m = gpu.GpuModel(c["mats"], d, time_varying=tv)
    p = gpu.GpuProblem(m, N - 1, N, None, **kw)
    try:
        p.upload(c["x0"], c["om"], c["midx"])
        _check(p.evaluate(c["v"]), c["posed"], path + " as posed")                       # no solve involved: the caller's plans
        got = p.evaluate(c["v"], omega_cols=c["oc"], col_rows=c["cr"])
        assert got["constr_vio"].shape == (B0, 3)
        assert np.all(np.isneginf(got["constr_vio"][:, 2])) and np.all(got["constr_row"][:, 2] == -1)      # the zero-row column
        _check(got, c["cols"], path + " 3 columns")
        if d["nx"]:
            _check(p.evaluate(c["v"], omega_cols=c["oc"], col_rows=c["cr"], x_cols=c["xc"]), c["xcols"], path + " x_cols")
        else:
            rc = _lib.load().mld_evaluate_batch(p._h, _lib.dptr(c["v"]), 3, _lib.dptr(c["oc"]), None, _lib.dptr(np.zeros(1)), _lib.dptr(np.zeros(B0)), None, None, None, None)
            assert rc == -1 and b"nx = 0" in _lib.load().mld_last_error()
        _raw_alone(p, c["v"], c["posed"], path + " raw as posed")
        _raw_alone(p, c["v"], c["cols"], path + " raw columns", 3, c["oc"] if c["oc"].size else None, c["cr"])
        # a (n,) plan is broadcast
        one = p.evaluate(c["v"][7])
        s = c["midx"] == 0
        _check({k: a[s] for k, a in one.items()}, qr.quality(c["refs"][0], np.tile(c["v"][7], (int(s.sum()), 1)), c["x0"][s], c["om"][s]), path + " broadcast")
        # one model, model_idx = None: two full groups and one of 44
        p.upload(c["x0"], c["om"])
        _check(p.evaluate(c["v"]), c["one"], path + " one model")
        _check(p.evaluate(c["v"], omega_cols=c["oc"], col_rows=c["cr"]), c["one_cols"], path + " one model, columns")
    finally:
        p.close(); m.close()


@pytest.mark.parametrize("path", [p for p, _ in PATHS])
@pytest.mark.parametrize("shape", list(ALL_SHAPES))
def test_kernel_paths_against_fp64_numpy(shape, path):
    """k_evaluate (default), k_evaluate_valu (reserved bit 7) and k_evaluate on an MLD_F32 handle -- all three fp64: 300 instances over three interleaved
    models with one unused, then one model without model_idx; as posed, 3 validation columns (the last with no rows), x_cols, every output alone"""
    _paths_case(_case(shape), path)


@pytest.mark.parametrize("path", [p for p, _ in PATHS])
def test_kernel_paths_time_varying(path):
    """a time-varying handle (three horizons of independent step models) against cn.condense_tv: model_idx indexes horizons"""
    _paths_case(_case("tv", tv=True), path, tv=True)


def test_valu_switch_selects_another_kernel():
    """reserved bit 7 must really select k_evaluate_valu: the two kernels sum in different orders (two MFMA accumulators over groups of four, chunk by
    chunk, against 64 strided partial sums and a shuffle tree), so on the same inputs they agree to rounding and are NOT bit-identical"""
    c = _case("straddle64")
    N, d = c["N"], c["d"]
    got = {}
    for path in ("mfma64", "valu"):
        m = gpu.GpuModel(c["mats"], d)
        p = gpu.GpuProblem(m, N - 1, N, None, **dict(PATHS)[path])
        try:
            p.upload(c["x0"], c["om"], c["midx"])
            got[path] = p.evaluate(c["v"], omega_cols=c["oc"])["constr_vio"]
        finally:
            p.close(); m.close()
    diff = np.abs(got["mfma64"] - got["valu"])
    print("max |mfma64 - valu| = %.3e over %d entries, %d differ" % (diff.max(), diff.size, (diff > 0).sum()))
    assert np.all(diff <= 2 * TOL * _by_model(c["refs"], c["midx"], c["v"], c["x0"], c["om"], omega_cols=c["oc"])["S"])
    assert not np.array_equal(got["mfma64"], got["valu"])


def test_bad_arguments_are_refused_and_change_nothing():
    c = _case("below16")
    N, d = c["N"], c["d"]
    m = gpu.GpuModel(c["mats"], d)
    p = gpu.GpuProblem(m, N - 1, N, None)
    lib = _lib.load()
    try:
        p.upload(c["x0"], c["om"], c["midx"])
        obj = np.full(B0, -3.0)
        v, oc = c["v"], c["oc"]
        m0 = N * d["nc"]
        for args, msg in (((-1, None, None, None), b"n_cols"), ((2, None, None, None), b"omega_cols"),
                          ((3, _lib.dptr(oc), _IP(np.array([0, m0 + 1, 1], np.int32)), None), b"col_rows[1]"),
                          ((3, _lib.dptr(oc), _IP(np.array([-1, 0, 1], np.int32)), None), b"col_rows[0]")):
            assert lib.mld_evaluate_batch(p._h, _lib.dptr(v), *args, _lib.dptr(obj), None, None, None, None) == -1
            assert msg in lib.mld_last_error() and np.all(obj == -3.0)
        _check(p.evaluate(v), c["posed"], "after the refusals")
    finally:
        p.close(); m.close()


# ---- costs ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["mfma64", "valu"])
@pytest.mark.parametrize("shape", ["straddle64", "odd3"])
def test_quadratic_model_cost(shape, path):
    """a quadratic model cost (non-symmetric weights on v, x and y, one per model): obj = 1/2 v'Pv + (q0 + Qx x0 + Qw omega)'v + the atoms' value at v = 0;
    on the second shape together with a resident per-instance cost"""
    c = _case(shape)
    N, d = c["N"], c["d"]
    costs = [_paths.random_cost(9500 + i, d, N) for i in range(3)]
    stacked = {k: np.stack([cc[k] for cc in costs]) for k in costs[0] if costs[0][k] is not None}
    rcost = [qr.cost_of(r["evo"], **cc) for r, cc in zip(c["refs"], costs)]
    rng = np.random.default_rng(9600)
    inst = dict(lin_v=rng.standard_normal((B0, N * d["nv"])), lin_x=rng.standard_normal((B0, N * d["nx"]))) if shape == "odd3" else None
    m = gpu.GpuModel(c["mats"], d)
    p = gpu.GpuProblem(m, N - 1, N, stacked, **dict(PATHS)[path])
    try:
        p.upload(c["x0"], c["om"], c["midx"])
        if inst:
            p.upload_instance_cost(**inst)
        ref = _by_model(c["refs"], c["midx"], c["v"], c["x0"], c["om"], cost=rcost, inst=inst)
        assert np.all(np.abs(ref["obj"] - c["posed"]["obj"]) > 1e-3)                   # (the cost is really there)
        _check(p.evaluate(c["v"]), ref, "%s quadratic cost%s" % (path, " + instance cost" if inst else ""))
        p.set_cost(None)                                                                # the cost of the LAST mld_problem_set_cost
        _check(p.evaluate(c["v"]), _by_model(c["refs"], c["midx"], c["v"], c["x0"], c["om"], inst=inst), path + " cost removed")
    finally:
        p.close(); m.close()


@pytest.mark.parametrize("path", ["mfma64", "valu"])
@pytest.mark.parametrize("shape", ["k380", "nx17"])
def test_resident_instance_cost(shape, path):
    """a resident per-instance cost with lin_x / lin_y (pulled back by k_inst_pullback) over a linear model cost: q_b and the constant at the current inputs"""
    c = _case(shape)
    N, d = c["N"], c["d"]
    rng = np.random.default_rng(9700)
    lin = {k: rng.standard_normal((3, ln)) for k, ln in (("lin_v", N * d["nv"]), ("lin_x", N * d["nx"]), ("lin_y", N * d["ny"]))}
    rcost = [qr.cost_of(r["evo"], **{k: a[i] for k, a in lin.items()}) for i, r in enumerate(c["refs"])]
    inst = dict(lin_v=rng.standard_normal((B0, N * d["nv"])), lin_x=rng.standard_normal((B0, N * d["nx"])), lin_y=rng.standard_normal((B0, N * d["ny"])))
    m = gpu.GpuModel(c["mats"], d)
    p = gpu.GpuProblem(m, N - 1, N, lin, **dict(PATHS)[path])
    try:
        p.upload(c["x0"], c["om"], c["midx"])
        _check(p.evaluate(c["v"]), _by_model(c["refs"], c["midx"], c["v"], c["x0"], c["om"], cost=rcost), path + " model cost only")
        p.upload_instance_cost(**inst)
        _check(p.evaluate(c["v"]), _by_model(c["refs"], c["midx"], c["v"], c["x0"], c["om"], cost=rcost, inst=inst), path + " with instance cost")
        p.upload_instance_cost(lin_v=inst["lin_v"])                                     # weights on v only: no constant maps resident
        _check(p.evaluate(c["v"]), _by_model(c["refs"], c["midx"], c["v"], c["x0"], c["om"], cost=rcost, inst=dict(lin_v=inst["lin_v"])), path + " lin_v only")
    finally:
        p.close(); m.close()


# ---- solved batches -----------------------------------------------------------------------------------------------------------------------
def _solved_ref(ag, wl, B):
    d = ag["dims"]
    sf = cn.standard_form(ag["mats"], ag["atoms"], wl["N_p"], wl["N_tilde"], nu_l=d["nu_l"], nmu_l=d.get("nmu_l", 0))
    return sf, dict(evo=sf["evo"], is_bin=sf["is_bin"], lb=sf["lb"], ub=sf["ub"])


def _check_solved(q, out, sf, what, sel):
    """the quality of plans the solver calls usable: the objective it reported, integral, inside the bounds, feasible for the ORIGINAL rows"""
    assert np.all(np.abs(q["obj"] - out["obj"])[sel] <= 1e-6 * np.maximum(1.0, np.abs(out["obj"][sel]))), what
    assert np.all(q["int_vio"][sel] == 0.0), what
    assert np.all(q["bound_vio"][sel] <= 1e-9), what
    rown = np.maximum(1.0, np.abs(sf["G"]).max(axis=1))
    assert np.all(q["constr_row"][sel] >= 0) and np.all(q["constr_vio"][sel] <= 1e-6 * rown[q["constr_row"][sel]]), what


@pytest.mark.parametrize("name,nb", [("cfg1", 6), ("cfg2", 6)])
def test_solved_batch(name, nb):
    """the instances of tests/test_gpu_solve.py::test_solve_matches_oracle: solve(..., quality=True) is an independent certificate of every OPTIMAL"""
    wl = syn.make_workload(name, batch=nb)
    ag = wl["agents"][0]
    d = ag["dims"]
    m = gpu.GpuModel([ag["mats"]], d)
    p = gpu.GpuProblem(m, wl["N_p"], wl["N_tilde"], host.cost_from_atoms(ag["atoms"], d, wl["N_p"], wl["N_tilde"]), max_nodes=20000)
    try:
        out = p.solve(ag["x0"], ag["omega"], quality=True)
        assert np.all(out["status"] == 0)
        q = out["quality"]
        sf, ref = _solved_ref(ag, wl, nb)
        _check_solved(q, out, sf, name, np.ones(nb, bool))
        _check(q, qr.quality(ref, out["v"], ag["x0"], ag["omega"], cost=sf["cost"]), name + " solved")
        again = p.evaluate()
        assert all(np.array_equal(again[k], q[k]) for k in q)
        assert "quality" not in p.solve(ag["x0"], ag["omega"])
        # the downloaded plans passed back in are the same plans
        same = p.evaluate(out["v"])
        assert all(np.array_equal(same[k], q[k]) for k in q)
    finally:
        p.close(); m.close()


# ---- constraint blocks ---------------------------------------------------------------------------------------------------------------------
def _posed_ref(ref, v, x0, om, cols, cr, xc, std):
    """the problem as posed with constraint blocks: the maximum over the standard column (when on) and the blocks' columns, each over its rows -- the
    residual against the row-wise minimum right-hand side over the rows that exist"""
    B, m0 = v.shape[0], ref["evo"]["H_v"].shape[0]
    oc = np.concatenate([om[:, None, :], cols], axis=1) if std else cols
    rows = np.r_[m0, cr] if std else np.asarray(cr)
    xx = None
    if xc is not None:
        xx = np.concatenate([x0[:, None, :], xc], axis=1) if std else xc
    q = qr.quality(ref, v, x0, om, omega_cols=oc, col_rows=rows, x_cols=xx)
    mask = np.arange(m0)[None, :] < rows[:, None]                                       # (C, m0): the rows column c covers
    Rm = np.where(mask[None], q["R"], -np.inf).max(axis=1)                               # (B, m0): H_v v - min_c h_c over the covering columns
    Sm = q["S"].max(axis=1)
    return q, Rm, Sm


def _check_posed(got, Rm, Sm, what):
    ref = Rm.max(axis=1)
    assert np.all(np.abs(got["constr_vio"] - ref) <= TOL * Sm), (what, (np.abs(got["constr_vio"] - ref) / Sm).max())
    row = got["constr_row"]
    assert np.all(row >= 0) and np.all(np.abs(Rm[np.arange(len(row)), row] - ref) <= TOL * Sm), what


@pytest.mark.parametrize("path", ["mfma64", "valu"])
def test_constraint_blocks_as_posed(path):
    """random rows, 300 instances over three models: blocks with a reduced col_rows, with x_cols, and without the standard block"""
    c = _case("straddle64")
    N, d = c["N"], c["d"]
    m0 = N * d["nc"]
    rng = np.random.default_rng(9800)
    cols, xc = rng.standard_normal((B0, 2, N * d["nomega"])), rng.standard_normal((B0, 2, d["nx"]))
    cr = np.array([m0 - 5, m0 // 3], np.int32)
    m = gpu.GpuModel(c["mats"], d)
    p = gpu.GpuProblem(m, N - 1, N, None, **dict(PATHS)[path])
    try:
        for std in (True, False):
            for use_x in (False, True):
                p.set_std_block(std)
                p.upload(c["x0"], c["om"], c["midx"])
                p.upload_constraint_blocks(cols, cr, xc if use_x else None)
                got = p.evaluate(c["v"])
                what = "%s std %d x_cols %d" % (path, std, use_x)
                for k in (0, 2):
                    s = c["midx"] == k
                    q, Rm, Sm = _posed_ref(c["refs"][k], c["v"][s], c["x0"][s], c["om"][s], cols[s], cr, xc[s] if use_x else None, std)
                    _check_posed({a: b[s] for a, b in got.items()}, Rm, Sm, what)
                    if not std:
                        assert np.all(got["constr_row"][s] < cr.max())                  # rows no block covers do not exist
                # the same columns passed as validation columns: per column, and their maximum is the as-posed value
                oc = np.concatenate([c["om"][:, None, :], cols], axis=1) if std else cols
                rows = np.r_[m0, cr].astype(np.int32) if std else cr
                xx = (np.concatenate([c["x0"][:, None, :], xc], axis=1) if std else xc) if use_x else None
                per = p.evaluate(c["v"], omega_cols=oc, col_rows=rows, x_cols=xx)
                S = np.concatenate([_posed_ref(c["refs"][k], c["v"], c["x0"], c["om"], cols, cr, xc if use_x else None, std)[2][:, None] for k in (0, 2)], axis=1)
                Sb = np.where(c["midx"] == 0, S[:, 0], S[:, 1])
                assert np.all(np.abs(per["constr_vio"].max(axis=1) - got["constr_vio"]) <= TOL * Sb), what
                again = p.evaluate(c["v"])                                              # the resident blocks were neither used nor changed
                assert all(np.array_equal(again[k], got[k]) for k in got), what
        # no standard block and no blocks: no row exists
        p.set_std_block(False)
        p.upload(c["x0"], c["om"], c["midx"])
        none = p.evaluate(c["v"])
        assert np.all(np.isneginf(none["constr_vio"])) and np.all(none["constr_row"] == -1)
        assert np.array_equal(none["int_vio"], c["posed"]["int_vio"]) and np.all(np.isfinite(none["obj"]))
        p.set_std_block(True)
    finally:
        p.close(); m.close()


def test_validation_columns_leave_the_problem_alone():
    """cfg2 with constraint blocks (the columns of tests/test_gpu_blocks.py): evaluating validation columns between upload and solve changes neither
    the inputs nor the solve's results, bit for bit; the solved plans are feasible for every block"""
    B, S = 4, 3
    wl, ag, d, m, p = _problem("cfg2", B, max_nodes=20000)
    N, nc = wl["N_tilde"], d["nc"]
    rng = np.random.default_rng(5)
    cols = np.stack([_draw_profiles(dict(ag, omega=ag["omega"][b:b + 1]), wl, rng, S) for b in range(B)])
    cr = np.array([N * nc, 8 * nc, 3 * nc], np.int32)
    x0, om = ag["x0"][:B], ag["omega"][:B]
    try:
        base = p.solve(x0, om, omega_cols=cols, col_rows=cr)
        p.upload(x0, om)
        p.upload_constraint_blocks(cols, cr)
        fresh = np.stack([_draw_profiles(dict(ag, omega=ag["omega"][b:b + 1]), wl, rng, 5) for b in range(B)])
        v = rng.standard_normal((B, p.n))
        i0 = p.inputs()
        val = p.evaluate(v, omega_cols=fresh, col_rows=[N * nc, N * nc, 8 * nc, 1, 0])
        assert val["constr_vio"].shape == (B, 5) and np.all(np.isneginf(val["constr_vio"][:, 4]))
        i1 = p.inputs()
        assert np.array_equal(i0[0], i1[0]) and np.array_equal(i0[1], i1[1])
        p.solve_resident()
        out = p.download()
        for k in ("v", "obj", "status", "lower_bound", "nodes", "pivots"):
            assert np.array_equal(out[k], base[k]), k
        ok = np.isin(out["status"], (0, 2)) & np.isfinite(out["obj"])
        assert ok.sum() >= 2
        sf, ref = _solved_ref(ag, wl, B)
        q = p.evaluate()
        _check_solved(q, out, sf, "cfg2 with blocks", ok)
        _, Rm, Sm = _posed_ref(ref, out["v"], x0, om, cols, cr, None, True)
        _check_posed({a: b[ok] for a, b in q.items()}, Rm[ok], Sm[ok], "cfg2 with blocks, solved")
        # a-posteriori validation of the solved plans on fresh columns: counted, nothing else
        fv = p.evaluate(omega_cols=fresh)
        print("violated fresh columns per instance (> 1e-6):", (fv["constr_vio"] > 1e-6).sum(axis=1))
        _check({k: a[ok] for k, a in fv.items()}, {k: (a[ok] if k != "rows" else a) for k, a in qr.quality(ref, out["v"], x0, om, omega_cols=fresh, cost=sf["cost"]).items()}, "fresh columns")
    finally:
        p.close(); m.close()


# ---- instances without a plan, the hand-off, handle states -----------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["mfma64", "valu"])
def test_instances_without_a_plan(path):
    """half of the batch ends INFEASIBLE under a cutoff just below its own optimum: exactly those instances are NaN / -1 with v=None; with v given nothing is masked"""
    B = 16
    wl, ag, d, m, p = _problem("cfg2", B, gap_rel=0.0, max_nodes=100000, **dict(PATHS)[path])
    try:
        masked, out = _half_without_a_plan(p, ag, B)
        sf, ref = _solved_ref(ag, wl, B)
        om3 = np.repeat(ag["omega"][:B, None, :], 3, axis=1)
        for kw in (dict(), dict(omega_cols=om3, col_rows=[p.m, 7, 0])):
            q = p.evaluate(**kw)
            for k in ("obj", "int_vio", "bound_vio"):
                assert np.array_equal(np.isnan(q[k]), masked), k
            cv, crow = q["constr_vio"].reshape(B, -1), q["constr_row"].reshape(B, -1)
            assert np.all(np.isnan(cv[masked])) and np.all(crow[masked] == -1) and not np.any(np.isnan(cv[~masked]))
            r = qr.quality(ref, out["v"], ag["x0"][:B], ag["omega"][:B], cost=sf["cost"], **kw)
            _check(q, r, path + " unmasked", sel=~masked)
            given = p.evaluate(out["v"], **kw)                                          # the same plans passed in: no masking
            assert all(np.all(np.isfinite(given[k]) | np.isneginf(given[k])) for k in ("obj", "int_vio", "bound_vio", "constr_vio"))
            _check(given, r, path + " v given")
            assert all(np.array_equal(given[k].reshape(B, -1)[~masked], q[k].reshape(B, -1)[~masked]) for k in q)
        _check_solved(p.evaluate(), out, sf, path, ~masked)
    finally:
        p.close(); m.close()


def test_in_kernel_handoff():
    """solve_handoff_device(..., quality=True) on the fixture of tests/test_gpu_handoff.py: the quality of the MERGED plans, read before the batch is dropped"""
    B = 48
    wl, ag, d, m, p = _problem("cfg2", B, gap_rel=0.0, max_nodes=100000, cut_rounds=1)
    try:
        x0, om = ag["x0"][:B], ag["omega"][:B]
        ho = dict(sub_nodes=12, max_gen=8, max_children=64, max_tree=100000, room_factor=64.0)
        out = p.solve_handoff_device(x0, om, first_nodes=3, quality=True, **ho)
        assert out["handoff"]["items"] >= 3 and np.all(out["status"] == 0)
        sf, ref = _solved_ref(ag, wl, B)
        q = out["quality"]
        assert q["obj"].shape == (B,) and q["constr_vio"].shape == (B,)
        _check_solved(q, out, sf, "hand-off", np.ones(B, bool))
        _check(q, qr.quality(ref, out["v"], x0, om, cost=sf["cost"]), "hand-off merged plans")
        assert "quality" not in p.solve_handoff_device(x0, om, first_nodes=3, **ho)
    finally:
        p.close(); m.close()


def test_handle_states():
    B = 16
    wl, ag, d, m, p = _problem("cfg2", B, gap_rel=1e-4, max_nodes=2000)
    lib = _lib.load()
    try:
        x0, om = ag["x0"][:B], ag["omega"][:B]
        sf, ref = _solved_ref(ag, wl, B)
        v = np.random.default_rng(9900).standard_normal((B, p.n))
        want = qr.quality(ref, v, x0, om, cost=sf["cost"])
        first = p.solve(x0, om)

        def same_solve():
            p.solve_resident()
            out = p.download()
            assert all(np.array_equal(out[k], first[k]) for k in ("v", "obj", "status", "nodes", "pivots"))

        obj = np.full(B, -3.0)
        # before any upload
        p2 = gpu.GpuProblem(m, wl["N_p"], wl["N_tilde"], None)
        assert lib.mld_evaluate_batch(p2._h, _lib.dptr(v), 0, None, None, None, _lib.dptr(obj), None, None, None, None) == -1 and b"no batch resident" in lib.mld_last_error()
        assert lib.mld_evaluate_batch(p2._h, None, 0, None, None, None, _lib.dptr(obj), None, None, None, None) == -1 and np.all(obj == -3.0)
        p2.close()
        # uploaded, not solved: the resident solution is refused, a caller's plan is fine
        p.upload(x0, om)
        with pytest.raises(gpu.MldGpuError, match="not been solved"):
            p.evaluate()
        _check(p.evaluate(v), want, "before any solve")
        same_solve()
        # after a selection
        p.stage(np.stack([x0, x0]), np.stack([om, om]))
        p.select(1)
        with pytest.raises(gpu.MldGpuError, match="not been solved"):
            p.evaluate()
        _check(p.evaluate(v), want, "after select")
        same_solve()
        # after advance
        q0 = p.evaluate()
        assert np.all(np.isfinite(q0["obj"][first["status"] == 0]))
        p.advance()
        with pytest.raises(gpu.MldGpuError, match="moved the inputs on"):
            p.evaluate()
        xn, wn = p.inputs()
        _check(p.evaluate(v), qr.quality(ref, v, xn, wn, cost=sf["cost"]), "after advance")
        p.upload(x0, om)
        same_solve()
        # between launch and finish: refused either way, nothing written
        p.launch()
        with pytest.raises(gpu.MldGpuError, match="not been finished"):
            p.evaluate(v)
        with pytest.raises(gpu.MldGpuError, match="not been finished"):
            p.evaluate()
        assert lib.mld_evaluate_batch(p._h, _lib.dptr(v), 0, None, None, None, _lib.dptr(obj), None, None, None, None) == -1 and np.all(obj == -3.0)
        p.finish()
        out = p.download()
        assert all(np.array_equal(out[k], first[k]) for k in ("v", "obj", "status", "nodes", "pivots"))
        ok = np.isin(out["status"], (0, 2)) & np.isfinite(out["obj"])
        assert ok.sum() >= B - 2
        _check_solved(p.evaluate(), out, sf, "after finish", ok)
        same_solve()
    finally:
        p.close(); m.close()
