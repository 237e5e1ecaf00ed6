"""Plant step and simulation log of a resident batch on device (mld_sim_step_batch / GpuProblem.sim_step, kernel k_sim_step): the reference's
ControllerBase.sim_step_k -> MldModel.lsim_k(x_k, v_k=, omega_k) -> MldSimLog (controllers/controller_base.py:229-253, models/mld_model.py:647-699,
controller_base.py:58-146).  Checked: the kernel against simlog.lsim_k_batch on every shape and batch (LDS staging and the global-memory path); the same
bits as advance(); three logged steps of a closed loop; the realised disturbance out of the profile library; instances without a plan; the caller's v0
before any solve; the in-kernel hand-off; every refusal.

Bound on x_k1, y and the residuals: simlog.sum_bound(dims) = (K + ny) 2^-52 times the row's sum of |terms|, K = nx + nv + nomega + 1 (two fp64 sums of
K terms in any order differ by at most that; a constraint row adds the ny terms of G y)."""
import ctypes as C

import numpy as np
import pytest

import _paths
from _traj_shapes import SHAPES, TV_SHAPE
from pyhybridcontrol_amd import gpu, host, profiles, simlog, synthetic as syn, _lib

pytestmark = pytest.mark.gpu

# more than 64 rows in a family (nc = 70: lanes take a second row) and a long inner dimension (nx + nv + nomega = 97 > 64: the staging loops run twice)
BIG = (3, dict(nx=17, nu=60, ndelta=1, nz=1, nmu=2, nomega=16, ny=4, nc=70))
STEP_SHAPES = dict({k: SHAPES[k] for k in ("below16", "nx17", "nw0", "nx0", "ny0")}, big=BIG)
BATCHES = (1, 3, 65, 257)
NO_LDS = 1 << 23      # MLD_DBG_SIM_NO_LDS


def _draw(rng, mats, d, midx, B):
    """inputs whose every residual is 1e-9 away from the threshold and whose row maximum is unique by 1e-9: failing instances are redrawn"""
    nx, nv, nw = d["nx"], d["nv"], d["nomega"]
    x, v, w = rng.standard_normal((B, nx)), rng.standard_normal((B, nv)), rng.standard_normal((B, nw))
    for _ in range(100):
        ref = simlog.lsim_k_batch(mats, d, midx, x, v, w)
        if not d["nc"]:
            return x, v, w, ref
        r = np.sort(ref["resid"], axis=1)
        bad = np.abs(ref["resid"] - 1e-6).min(axis=1) < 1e-9
        if d["nc"] > 1:
            bad |= r[:, -1] - r[:, -2] < 1e-9
        if not bad.any():
            return x, v, w, ref
        n = int(bad.sum())
        x[bad], v[bad], w[bad] = rng.standard_normal((n, nx)), rng.standard_normal((n, nv)), rng.standard_normal((n, nw))
    raise AssertionError("no draw with every residual away from the threshold")


def _check_step(got, ref, d, what, drawn=True):
    """drawn: the inputs come from _draw, so truth values and the maximal row are exact.  A solved plan rests ON its active rows (several residuals
    equal up to rounding, the soft rows at their slack), so there a truth value is compared only where the residual is 1e-9 away from the threshold and
    the reported row must attain the reference's maximum within the bound"""
    bound = simlog.sum_bound(d)
    for name, terms in (("x_k1", ref["terms_x"]), ("y", ref["terms_y"])):
        assert got[name].shape == ref[name].shape, (what, name)
        err = np.abs(got[name] - ref[name])
        if err.size:
            print("%s %s: worst err / (bound x sum|terms|) = %.3f" % (what, name, float((err / np.maximum(bound * terms, 1e-300)).max())))
        assert np.all(err <= bound * terms), (what, name)
    assert got["cons"].shape == ref["cons"].shape and got["cons"].dtype == bool, what
    if not d["nc"]:
        assert np.all(got["cons_vio"] == -np.inf) and np.all(got["cons_row"] == -1), what
        return
    rows = got["cons_row"]
    assert rows.dtype == np.int32 and np.all((rows >= 0) & (rows < d["nc"])), what
    at = np.arange(rows.size)
    if drawn:
        assert np.array_equal(got["cons"], ref["cons"]), what
        assert np.array_equal(rows, ref["cons_row"]), what
    else:
        clear = np.abs(ref["resid"] - 1e-6) >= 1e-9
        assert np.array_equal(got["cons"][clear], ref["cons"][clear]), what
        assert np.all(ref["resid"][at, rows] >= ref["cons_vio"] - 2 * bound * ref["terms_r"].max(axis=1)), what
    assert np.all(np.abs(got["cons_vio"] - ref["resid"][at, rows]) <= bound * ref["terms_r"][at, rows]), what


def _raw_step(p, v0, flags, want):
    """the C entry itself with a chosen subset of outputs; returns the arrays asked for"""
    d, B = p.model.dims, p.batch
    bufs = dict(x_k1=np.full((B, d["nx"]), -7.0), y=np.full((B, d["ny"]), -7.0), cons=np.full((B, d["nc"]), 9, np.uint8), cons_vio=np.full(B, -7.0),
                cons_row=np.full(B, -7, np.int32))
    ptr = dict(x_k1=_lib.dptr, y=_lib.dptr, cons=lambda a: a.ctypes.data_as(C.POINTER(C.c_uint8)), cons_vio=_lib.dptr,
               cons_row=lambda a: a.ctypes.data_as(C.POINTER(C.c_int32)))
    args = [ptr[k](bufs[k]) if k in want else None for k in ("x_k1", "y", "cons", "cons_vio", "cons_row")]
    v0 = np.ascontiguousarray(v0, dtype=np.float64)
    rc = _lib.load().mld_sim_step_batch(p._h, _lib.dptr(v0), None, 0, flags, *args, None)
    assert rc == 0, _lib.load().mld_last_error()
    return {k: bufs[k] for k in want}


@pytest.mark.parametrize("shape", list(STEP_SHAPES))
def test_kernel_against_numpy(shape):
    """the caller's v0 on every shape and batch: two interleaved models with model_idx, then one model without; all outputs, x_k1 only, cons only, all
    NULL; the global-memory path (MLD_DBG_SIM_NO_LDS) gives the same bits as the LDS staging"""
    N, dims = STEP_SHAPES[shape]
    d = _paths.make_dims(**dims)
    seed = 9100 + 10 * list(STEP_SHAPES).index(shape)
    mats = [_paths.random_mld(seed * 1000 + i, **dims)[0] for i in range(2)]
    rng = np.random.default_rng(seed)
    m = gpu.GpuModel(mats, d)
    p = gpu.GpuProblem(m, N - 1, N, None)
    try:
        for B in BATCHES:
            for midx in (rng.integers(0, 2, B).astype(np.int32), None):
                if midx is not None and B > 1:
                    midx[:2] = (0, 1)
                used = mats if midx is not None else mats[:1]
                x, v, w, ref = _draw(rng, used, d, midx, B)
                om = np.concatenate([w, rng.standard_normal((B, (N - 1) * d["nomega"]))], axis=1)      # step 0 of the forecast is omega_k
                p.upload(x, om, midx)
                what = "%s B=%d %s" % (shape, B, "two models" if midx is not None else "one model")
                got = p.sim_step(v0=v, advance=False, log=False, outputs=True)
                assert got["n_skipped"] == 0
                _check_step(got, ref, d, what)
                p.set_opts(reserved=NO_LDS)
                glob = p.sim_step(v0=v, advance=False, log=False, outputs=True)
                p.set_opts(reserved=0)
                for k in ("x_k1", "y", "cons", "cons_vio", "cons_row"):
                    assert np.array_equal(glob[k], got[k]), (what, k, "global-memory path")
                only = _raw_step(p, v, 0, ("x_k1",))
                assert np.array_equal(only["x_k1"], got["x_k1"]), what
                only = _raw_step(p, v, 0, ("cons",))
                assert np.array_equal(only["cons"].astype(bool), got["cons"]), what
                x_in, om_in = p.inputs()
                assert np.array_equal(x_in, x) and np.array_equal(om_in, om), what          # a what-if writes nothing
                assert _raw_step(p, v, 0, ()) == {}                                         # all NULL, no flag: nothing to do
                assert _raw_step(p, v, _lib.MLD_SIM_ADVANCE, ()) == {}                      # all NULL with ADVANCE: the step is taken
                x_in, om_in = p.inputs()
                assert np.array_equal(x_in, got["x_k1"]), what
                assert np.array_equal(om_in.reshape(B, N, d["nomega"]), np.roll(om.reshape(B, N, d["nomega"]), -1, axis=1)), what
    finally:
        p.close(); m.close()


# ------------------------------------------------------------------------------------------------------------------ solved batches
def _cfg2_two_agents():
    wl = syn.make_workload("cfg2", batch=6, n_agents=2)
    d = wl["agents"][0]["dims"]
    N = wl["N_tilde"]
    m = gpu.GpuModel([a["mats"] for a in wl["agents"]], d)
    cost = host.stack_costs([host.cost_from_atoms(a["atoms"], d, wl["N_p"], N) for a in wl["agents"]])
    x0 = np.concatenate([a["x0"] for a in wl["agents"]])
    om = np.concatenate([a["omega"] for a in wl["agents"]])
    midx = np.repeat(np.arange(2), 6).astype(np.int32)
    return wl, d, N, m, cost, x0, om, midx


def _new_problem(wl, m, cost, **kw):
    return gpu.GpuProblem(m, wl["N_p"], wl["N_tilde"], cost, **dict(dict(gap_rel=1e-2, max_nodes=400), **kw))


def test_same_bits_as_advance():
    wl, d, N, m, cost, x0, om, midx = _cfg2_two_agents()
    pa, pb = _new_problem(wl, m, cost), _new_problem(wl, m, cost)
    try:
        oa, ob = pa.solve(x0, om, midx), pb.solve(x0, om, midx)
        assert np.array_equal(oa["v"], ob["v"])
        assert pa.advance() == 0
        # the C entry with nothing to report: no output, no skip count (the call that does not wait for the stream)
        assert _lib.load().mld_sim_step_batch(pb._h, None, None, 0, _lib.MLD_SIM_ADVANCE, None, None, None, None, None, None) == 0, _lib.load().mld_last_error()
        (xa, wa), (xb, wb) = pa.inputs(), pb.inputs()
        assert np.array_equal(xa, xb) and np.array_equal(wa, wb)
        assert not np.array_equal(xa, x0)
        pa.warm_start_from_previous(1); pb.warm_start_from_previous(1)
        pa.solve_resident(); pb.solve_resident()
        ra, rb = pa.download(), pb.download()
        for k in ("v", "obj", "status", "lower_bound", "nodes", "pivots"):
            assert np.array_equal(ra[k], rb[k]), k
        assert pb.sim_step(advance=True) == 0
        with pytest.raises(gpu.MldGpuError, match="already been applied"):
            pb.sim_step(advance=True)
    finally:
        pa.close(); pb.close(); m.close()


def test_three_logged_steps():
    wl, d, N, m, cost, x0, om, midx = _cfg2_two_agents()
    p = _new_problem(wl, m, cost)
    nv, nw, B = m.nv, d["nomega"], 12
    try:
        p.upload(x0, om, midx)
        assert p.sim_log_count() == (0, 0)
        p.sim_log_begin(3)
        assert p.sim_log_count() == (0, 3)
        xs, ws, outs = [], [], []
        for k in range(3):
            p.solve_resident()
            outs.append(p.download())
            x_in, w_in = p.inputs()
            xs.append(x_in); ws.append(w_in)
            assert p.sim_step() == 0                            # log defaults to "a log has begun", advance to True
            assert p.sim_log_count() == (k + 1, 3)
            p.warm_start_from_previous(1)
        log = p.sim_log()
        assert log["x"].shape == (3, B, d["nx"]) and log["cons"].shape == (3, B, d["nc"]) and log["cons"].dtype == bool
        for k in range(3):
            assert np.array_equal(log["x"][k], xs[k]) and np.array_equal(log["v"][k], outs[k]["v"][:, :nv])
            assert np.array_equal(log["omega"][k], ws[k][:, :nw])
            for name in ("obj", "lower_bound", "status", "nodes"):
                assert np.array_equal(log[name][k], outs[k][name]), (k, name)
            ref = simlog.lsim_k_batch([a["mats"] for a in wl["agents"]], d, midx, xs[k], outs[k]["v"][:, :nv], ws[k][:, :nw])
            _check_step({n: log[n][k] for n in ("x_k1", "y", "cons", "cons_vio", "cons_row")}, ref, _dims_nv(d), "logged step %d" % k, drawn=False)
        assert np.array_equal(log["x_k1"][0], log["x"][1]) and np.array_equal(log["x_k1"][1], log["x"][2])
        assert np.array_equal(log["x_k1"][2], p.inputs()[0])
        part = p.sim_log(1, 2)
        for name in log:
            assert np.array_equal(part[name], log[name][1:3]), name
        # a fourth record does not fit: refused, nothing changes
        p.solve_resident()
        before = p.inputs()
        with pytest.raises(gpu.MldGpuError, match="log is full"):
            p.sim_step(log=True)
        after = p.inputs()
        assert p.sim_log_count() == (3, 3) and np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
        again = p.sim_log()
        for name in log:
            assert np.array_equal(again[name], log[name], equal_nan=True), name
        assert p.sim_step(log=False) == 0                       # ... and the step itself is still there to take
        frame = simlog.to_mld_sim_log(log, 5, d).get_concat_log()
        assert frame.shape[0] == 3 and np.array_equal(frame["x"].to_numpy(), log["x"][:, 5])
        p.upload(x0, om, midx)                                  # a new batch discards the log
        assert p.sim_log_count() == (0, 0)
    finally:
        p.close(); m.close()


def _dims_nv(d):
    return dict(d, nv=d["nu"] + d["ndelta"] + d["nz"] + d["nmu"])


@pytest.mark.parametrize("widths", ["one", "ones", "uneven"])
def test_realised_disturbance(widths):
    wl, d, N, m, cost, x0, om, midx = _cfg2_two_agents()
    nw, nv, B, step = d["nomega"], m.nv, 12, 2
    gw = dict(one=(nw,), ones=(1,) * nw, uneven=(1, nw - 1))[widths]
    G, T = len(gw), N + step + B + 4
    rng = np.random.default_rng(9500 + G)
    # per group one forecast series and one REALISED series (T, width), the forecast cut out of the workload's own disturbances
    goff = np.concatenate([[0], np.cumsum(gw)[:-1]])
    base_series = np.tile(om[0].reshape(N, nw), (T // N + 1, 1))[:T]
    fc = [base_series[:, goff[g]:goff[g] + gw[g]] for g in range(G)]
    act = [s * (1.0 + 0.2 * rng.standard_normal(s.shape)) for s in fc]
    lib, base = profiles.pack(fc + act)
    t_b = np.arange(B) % 5
    fstart = np.stack([base[g] + t_b * gw[g] for g in range(G)], axis=1)
    astart = np.stack([base[G + g] + t_b * gw[g] for g in range(G)], axis=1)
    # the exact last valid offset of the last group at `step`, and offset 0 (instance 0 reads the library's first series as its realised one)
    astart[0, 0] = 0
    last = lib.size - (step + 1) * gw[-1]
    astart[B - 1, G - 1] = last
    mats = [a["mats"] for a in wl["agents"]]
    p = _new_problem(wl, m, cost)
    try:
        p.upload(x0, om, midx)
        p.upload_profiles(lib, gw)
        p.forecast_from_profiles(fstart, step)
        p.solve_resident()
        out = p.download()
        assert np.all(np.isin(out["status"], (0, 2)))
        x_in, w_in = p.inputs()
        v0 = out["v"][:, :nv]

        def element(start, s):
            return profiles.windows(lib, start, s, 1, gw)

        w_act = element(astart, step)
        assert not np.array_equal(w_act, w_in[:, :nw])
        ref = simlog.lsim_k_batch(mats, d, midx, x_in, v0, w_act)
        t_before = p.trajectories()
        # a what-if under the realised value: nothing moves, the solved state stays
        got = p.sim_step(act_start=astart, step=step, advance=False, outputs=True)
        _check_step(got, ref, _dims_nv(d), "what-if " + widths, drawn=False)
        assert got["n_skipped"] == 0
        x_same, w_same = p.inputs()
        assert np.array_equal(x_same, x_in) and np.array_equal(w_same, w_in)
        t_after = p.trajectories()
        assert np.array_equal(t_before["x"], t_after["x"]) and np.array_equal(t_before["y"], t_after["y"])
        p.set_opts(reserved=NO_LDS)
        glob = p.sim_step(act_start=astart, step=step, advance=False, outputs=True)
        p.set_opts(reserved=0)
        for k in ("x_k1", "y", "cons", "cons_vio", "cons_row"):
            assert np.array_equal(glob[k], got[k], equal_nan=True), (k, "global-memory path")
        # the resident starts under the next step: the last group's largest start no longer fits, and is named
        with pytest.raises(gpu.MldGpuError, match="largest resident actual start of group %d" % (G - 1)):
            p.sim_step(step=step + 1, actual=True, advance=False)
        bad = astart.copy()
        bad[B - 1, G - 1] = last + 1
        with pytest.raises(gpu.MldGpuError, match="instance %d, group %d" % (B - 1, G - 1)):
            p.sim_step(act_start=bad, step=step, advance=False)
        # starts that leave room for one more step; act_start=None then reads the next element
        astart[B - 1, G - 1] = lib.size - (step + 2) * gw[-1]
        w_act = element(astart, step)
        ref = simlog.lsim_k_batch(mats, d, midx, x_in, v0, w_act)
        got = p.sim_step(act_start=astart, step=step, advance=False, outputs=True)
        _check_step(got, ref, _dims_nv(d), "new starts " + widths, drawn=False)
        nxt = p.sim_step(step=step + 1, actual=True, advance=False, outputs=True)
        _check_step(nxt, simlog.lsim_k_batch(mats, d, midx, x_in, v0, element(astart, step + 1)), _dims_nv(d), "next element " + widths, drawn=False)
        assert not np.array_equal(nxt["x_k1"], got["x_k1"])
        # the step itself
        done = p.sim_step(step=step, actual=True, advance=True, outputs=True)
        for k in ("x_k1", "y", "cons", "cons_vio", "cons_row"):
            assert np.array_equal(done[k], got[k]), k
        x_new, w_new = p.inputs()
        assert np.array_equal(x_new, done["x_k1"])
        assert np.array_equal(w_new.reshape(B, N, nw), np.roll(w_in.reshape(B, N, nw), -1, axis=1))
        p.forecast_from_profiles(None, step + 1)               # as after advance(): the resident forecast starts slide on
        assert np.array_equal(p.inputs()[1], profiles.windows(lib, fstart, step + 1, N, gw))
        p.warm_start_from_previous(1)
        p.solve_resident()
        # a new library invalidates the resident actual starts
        p.upload_profiles(lib, gw)
        with pytest.raises(gpu.MldGpuError, match="no actual starts"):
            p.sim_step(step=0, actual=True, advance=False)
    finally:
        p.close(); m.close()


def test_instances_without_a_plan():
    from test_gpu_trajectories import _half_without_a_plan, _problem
    B = 16
    wl, ag, d, m, p = _problem("cfg2", 2 * B, gap_rel=0.0, max_nodes=100000)
    N, nv, nw = wl["N_tilde"], m.nv, d["nomega"]
    try:
        masked, out = _half_without_a_plan(p, ag, B)
        x_old, w_old = p.inputs()
        p.sim_log_begin(1)
        got = p.sim_step(outputs=True)
        assert got["n_skipped"] == masked.sum() == B // 2
        x_new, w_new = p.inputs()
        assert np.array_equal(x_new[masked], x_old[masked]) and np.array_equal(w_new[masked], w_old[masked])
        ref = simlog.lsim_k_batch([ag["mats"]], d, None, x_old, np.where(masked[:, None], 0.0, out["v"][:, :nv]), w_old[:, :nw])
        live = ~masked
        _check_step({k: got[k][live] for k in ("x_k1", "y", "cons", "cons_vio", "cons_row")}, {k: v[live] for k, v in ref.items()}, _dims_nv(d), "live half", drawn=False)
        assert np.array_equal(x_new[live], got["x_k1"][live])
        assert np.array_equal(w_new[live].reshape(-1, N, nw), np.roll(w_old[live].reshape(-1, N, nw), -1, axis=1))
        log = p.sim_log()
        for name in ("v", "y", "x_k1"):
            assert np.all(np.isnan(log[name][0][masked])) and np.all(np.isnan(got[name][masked]) if name != "v" else True), name
            assert np.all(np.isfinite(log[name][0][live])), name
        assert np.all(np.isnan(log["cons_vio"][0][masked])) and np.all(np.isnan(got["cons_vio"][masked]))
        assert not log["cons"][0][masked].any() and not got["cons"][masked].any()
        assert np.all(log["cons_row"][0][masked] == -1) and np.all(got["cons_row"][masked] == -1)
        assert np.array_equal(log["x"][0], x_old) and np.array_equal(log["omega"][0], w_old[:, :nw])
        for name in ("obj", "lower_bound", "status", "nodes"):
            assert np.array_equal(log[name][0], out[name]), name
        assert np.array_equal(log["v"][0][live], out["v"][live, :nv]) and np.array_equal(log["x_k1"][0][live], got["x_k1"][live])
    finally:
        p.close(); m.close()


def test_callers_v0_before_any_solve():
    """a rule-based baseline stepped through the resident batch: no solve needed; with ADVANCE the handle is a freshly selected batch afterwards"""
    wl, d, N, m, cost, x0, om, midx = _cfg2_two_agents()
    p = _new_problem(wl, m, cost)
    nv, nw, B = m.nv, d["nomega"], 12
    try:
        p.upload(x0, om, midx)
        p.sim_log_begin(2)
        v0 = np.zeros((B, nv))
        v0[:, 0] = 1.0                                          # "first heater on"
        ref = simlog.lsim_k_batch([a["mats"] for a in wl["agents"]], d, midx, x0, v0, om[:, :nw])
        got = p.sim_step(v0=v0[0], outputs=True)                # a (nv,) slice is broadcast
        _check_step(got, ref, _dims_nv(d), "caller's v0", drawn=False)
        assert got["n_skipped"] == 0 and np.array_equal(p.inputs()[0], got["x_k1"])
        log = p.sim_log()
        assert np.array_equal(log["v"][0], v0) and np.all(np.isnan(log["obj"][0])) and np.all(np.isnan(log["lower_bound"][0]))
        assert np.all(log["status"][0] == -1) and np.all(log["nodes"][0] == 0)
        with pytest.raises(gpu.MldGpuError, match="not been solved"):
            p.trajectories()
        with pytest.raises(gpu.MldGpuError, match="not been solved"):
            p.sim_step()
        with pytest.raises(gpu.MldGpuError):
            p.warm_start_from_previous(1)
        p.solve_resident()
        direct = _new_problem(wl, m, cost)
        want = direct.solve(got["x_k1"], np.roll(om.reshape(B, N, nw), -1, axis=1).reshape(B, -1), midx)
        direct.close()
        mine = p.download()
        assert np.array_equal(mine["obj"], want["obj"]) and np.array_equal(mine["status"], want["status"])
        # after a solve the caller's inputs still step (and un-solve) the batch
        assert p.sim_step(v0=v0) == 0
        with pytest.raises(gpu.MldGpuError, match="not been solved"):
            p.trajectories()
        assert p.sim_log_count() == (2, 2)
    finally:
        p.close(); m.close()


def test_handoff_on():
    from test_gpu_trajectories import _problem
    B = 48
    wl, ag, d, m, p = _problem("cfg2", B, gap_rel=0.0, max_nodes=100000, cut_rounds=1)
    nv, nw = m.nv, d["nomega"]
    try:
        x0, om = ag["x0"][:B], ag["omega"][:B]
        p.set_opts(max_nodes=3)
        p.set_handoff(True, sub_nodes=12, max_gen=8, max_children=64, max_tree=100000, room_factor=64.0)
        p.upload(x0, om)
        p.solve_resident()
        assert p.handoff_stats()["items"] >= 3
        out = p.download()
        assert np.all(out["status"] == 0)
        p.sim_log_begin(1)
        got = p.sim_step(outputs=True)
        assert got["n_skipped"] == 0
        log = p.sim_log()
        assert log["v"].shape == (1, B, nv) and np.array_equal(log["v"][0], out["v"][:, :nv])            # the merged plans
        for name in ("obj", "lower_bound", "status", "nodes"):
            assert np.array_equal(log[name][0], out[name]), name
        _check_step(got, simlog.lsim_k_batch([ag["mats"]], d, None, x0, out["v"][:, :nv], om[:, :nw]), _dims_nv(d), "hand-off on", drawn=False)
    finally:
        p.close(); m.close()


def test_refusals_change_nothing():
    wl, d, N, m, cost, x0, om, midx = _cfg2_two_agents()
    nv, nw, B = m.nv, d["nomega"], 12
    p = _new_problem(wl, m, cost)
    v0 = np.zeros((B, nv))
    lib = _lib.load()
    try:
        # no batch resident
        for call in (lambda: p.sim_log_begin(2), lambda: p.sim_step(v0=np.zeros(nv), log=False), lambda: p.sim_log(0, 0)):
            with pytest.raises(gpu.MldGpuError, match="no batch resident"):
                call()
        first = p.solve(x0, om, midx)
        p.sim_log_begin(2)
        assert p.sim_step(advance=False, log=True) == 0
        state = (p.inputs(), p.sim_log_count(), p.sim_log())

        def refused(match, **kw):
            with pytest.raises(gpu.MldGpuError, match=match):
                p.sim_step(**kw)

        refused("step = -1", step=-1, advance=False)
        refused("no profile library", actual=True, advance=False)
        refused("no profile library", act_start=np.zeros((B, 1), np.int64), advance=False)
        assert lib.mld_sim_step_batch(p._h, None, None, 0, 8, None, None, None, None, None, None) == -1 and b"unknown flag" in lib.mld_last_error()
        assert lib.mld_sim_step_batch(p._h, None, None, 0, -1, None, None, None, None, None, None) == -1
        st = np.zeros((B, 1), np.int64)
        assert lib.mld_sim_step_batch(p._h, None, st.ctypes.data_as(C.POINTER(C.c_int64)), 0, 1, None, None, None, None, None, None) == -1
        assert b"without MLD_SIM_ACTUAL" in lib.mld_last_error()
        with pytest.raises(gpu.MldGpuError, match=r"records \[1, 3\)"):
            p.sim_log(1, 2)
        with pytest.raises(gpu.MldGpuError, match="records"):
            p.sim_log(-1, 1)
        with pytest.raises(gpu.MldGpuError, match="capacity = -1"):
            p.sim_log_begin(-1)
        # with a library: a missing start, a start past the end (named by instance and group)
        series = np.arange(40.0 * nw).reshape(40, nw)
        flat, _ = profiles.pack([series])
        # (upload_profiles does not touch the batch or the log)
        p.upload_profiles(flat)
        refused("no actual starts", actual=True, advance=False)
        bad = np.zeros((B, 1), np.int64)
        bad[7, 0] = flat.size - nw + 1
        refused("instance 7, group 0", act_start=bad, advance=False)
        bad[7, 0] = -1
        refused("instance 7, group 0", act_start=bad, advance=False)
        refused("no actual starts", actual=True, advance=False)                 # a refused call left no starts behind
        # a launched solve not finished
        p.launch()
        for call in (lambda: p.sim_step(v0=v0, log=False), lambda: p.sim_log_begin(1), lambda: p.sim_log()):
            with pytest.raises(gpu.MldGpuError, match="has not been finished"):
                call()
        p.finish()
        # a full log
        assert p.sim_step(advance=False, log=True) == 0
        state = (state[0], p.sim_log_count(), p.sim_log())
        assert state[1] == (2, 2)
        refused("log is full", log=True, advance=False)
        refused("log is full", v0=v0, log=True)
        p.sim_log_begin(0)
        refused("no log has been begun", log=True, advance=False)
        p.sim_log_begin(2)
        assert p.sim_log_count() == (0, 2)
        # nothing a later solve reads has moved
        x_in, w_in = p.inputs()
        assert np.array_equal(x_in, state[0][0]) and np.array_equal(w_in, state[0][1]) and np.array_equal(x_in, x0)
        p.solve_resident()
        again = p.download()
        for k in ("v", "obj", "status"):
            assert np.array_equal(again[k], first[k]), k
    finally:
        p.close(); m.close()
    # nomega == 0: MLD_SIM_ACTUAL has nothing to fill; a time-varying handle is refused as advance() refuses it
    Nn, dims = STEP_SHAPES["nw0"]
    dd = _paths.make_dims(**dims)
    mm = gpu.GpuModel([_paths.random_mld(9901, **dims)[0]], dd)
    pp = gpu.GpuProblem(mm, Nn - 1, Nn, None)
    try:
        pp.upload(np.zeros((2, dd["nx"])), np.zeros((2, 0)))
        with pytest.raises(gpu.MldGpuError, match="nomega = 0"):
            pp.sim_step(v0=np.zeros(dd["nv"]), actual=True, advance=False)
    finally:
        pp.close(); mm.close()
    Nt, tdims = TV_SHAPE
    td = _paths.make_dims(**tdims)
    tm = gpu.GpuModel([_paths.random_horizon(91, Nt, **tdims)[0]], td, time_varying=True)
    tp = gpu.GpuProblem(tm, Nt - 1, Nt, None)
    try:
        x, w = np.ones((3, td["nx"])), np.ones((3, Nt * td["nomega"]))
        tp.upload(x, w)
        with pytest.raises(gpu.MldGpuError, match="time-varying"):
            tp.sim_step(v0=np.zeros(td["nv"]), log=False)
        x_in, w_in = tp.inputs()
        assert np.array_equal(x_in, x) and np.array_equal(w_in, w)
    finally:
        tp.close(); tm.close()
