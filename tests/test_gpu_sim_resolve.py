"""Plant step of a resident batch with the auxiliaries re-derived on device (mld_sim_step_resolve / GpuProblem.sim_step(resolve=...), kernels k_aux_inputs
and k_aux_merge): the reference's ControllerBase.sim_step_k -> MldModel.lsim_k(x_k, u_k=, omega_k) -> _compute_aux (controllers/controller_base.py:229-253,
models/mld_model.py:683-686, 701-766).  Checked: the device route against the host route over the same resolver handle, bit for bit; the closed form of
tests/_aux_ref.py under realised loads that differ from the forecast -- where the planned auxiliaries are inconsistent --; masking of instances whose
auxiliary problem is infeasible or whose plan is unusable; advance and log; a second upload with other model indices; a model without auxiliaries; every
refusal.

Shapes: make_agent(3, tie=True) x 3 models at N_tilde = 3 with batch 10 (not a multiple of the four waves of a k_sim_step workgroup, model_idx interleaved)
and batch 1; make_agent(7, tie=True) x 2 models at N_tilde = 2 with batch 9; each with the LDS staging of k_sim_step and without (MLD_DBG_SIM_NO_LDS)."""
import ctypes as C

import numpy as np
import pytest

import _aux_ref
from test_gpu_sim_step import _check_step, _dims_nv
from pyhybridcontrol_amd import gpu, host, profiles, simlog, synthetic as syn, _lib
from pyhybridcontrol_amd.aux_resolve import BatchAuxResolver

pytestmark = pytest.mark.gpu

NO_LDS = 1 << 23      # MLD_DBG_SIM_NO_LDS
SHAPES = dict(a10=(3, 3, 3, 10), a1=(3, 3, 3, 1), b9=(7, 2, 2, 9))      # n_h, models, N_tilde, batch
OUT = ("x_k1", "y", "cons", "cons_vio", "cons_row")
INFEASIBLE = 1


class _Ctx(object):
    """models, a problem over them, the resolver, and one scenario per instance; model_idx interleaved"""

    def __init__(self, n_h, n_models, N, B, hard=False, tie=True, seed=7700):
        self.N, self.B = N, B
        self.mats, self.atoms, xs, oms = [], [], [], []
        for k in range(n_models):
            rng = np.random.default_rng(seed + 10 * n_h + k)
            mats, d, params = syn.make_agent(n_h, rng, tie=tie)
            atoms = syn.make_cost(n_h, N, params, tie=tie)
            if hard:
                mats, d = _aux_ref.hard_variant(mats, d)
                atoms = {k_: v for k_, v in atoms.items() if k_ != "q_mu"}
            x0, om = syn.make_scenarios(n_h, N, B, rng, tie=tie)
            self.mats.append(mats); self.atoms.append(atoms); xs.append(x0); oms.append(om)
        self.d = d
        self.midx = (np.arange(B) % n_models).astype(np.int32)
        at = np.arange(B)
        self.x0, self.om = np.stack(xs)[self.midx, at], np.stack(oms)[self.midx, at]
        self.nu, self.nw, self.nx = d["nu"], d["nomega"], d["nx"]
        self.model = gpu.GpuModel(self.mats, d)
        cost = host.stack_costs([host.cost_from_atoms(a, d, N - 1, N) for a in self.atoms])
        self.p = gpu.GpuProblem(self.model, N - 1, N, cost, gap_rel=1e-2, max_nodes=400)
        self.R = BatchAuxResolver(self.mats, d)
        self.nv = self.model.nv

    def close(self):
        self.R.close(); self.p.close(); self.model.close()

    def closed_form(self, x, u, w):
        """tests/_aux_ref.py per instance's model"""
        out = None
        for k, mats in enumerate(self.mats):
            cf = _aux_ref.closed_form(mats, self.d, x, u, w)
            if out is None:
                out = {n: np.zeros_like(a) for n, a in cf.items()}
            for n in cf:
                out[n][self.midx == k] = cf[n][self.midx == k]
        return out

    def realised(self, rng, step):
        """a library of one realised series per instance and group (groups of widths 1 and nomega - 1, as tests/test_gpu_sim_step.py packs them): the forecast
        with its load channel moved by N(0, 800); returns (lib, group widths, act_start, the realised omega_k of `step`)"""
        gw = (1, self.nw - 1)
        T = self.N + step + 2
        series = []
        for b in range(self.B):
            s = np.tile(self.om[b].reshape(self.N, self.nw), (T // self.N + 1, 1))[:T].copy()
            s[:, self.nx] += rng.normal(0.0, 800.0, T)
            series += [s[:, :1], s[:, 1:]]
        lib, base = profiles.pack(series)
        astart = base.reshape(self.B, 2)
        return lib, gw, astart, profiles.windows(lib, astart, step, 1, gw)


_CACHE = {}


@pytest.fixture(scope="module")
def ctx():
    def get(name, **kw):
        key = (name,) + tuple(sorted(kw.items()))
        if key not in _CACHE:
            _CACHE[key] = _Ctx(*SHAPES[name], **kw)
        return _CACHE[key]
    yield get
    for c in _CACHE.values():
        c.close()
    _CACHE.clear()


def _equal(a, b, names, what):
    for k in names:
        assert np.array_equal(a[k], b[k], equal_nan=True), (what, k)


def _host_route(c, x, u, w, midx, **kw):
    """the parent's route over the SAME resolver handle: BatchAuxResolver.resolve fed from the host, then sim_step(v0=[u; delta; z; mu])"""
    h = c.R.resolve(x, u, w, midx)
    v0 = np.hstack([u, h["v"]])
    out = c.p.sim_step(v0=v0, advance=False, log=False, outputs=True, **kw)
    return dict(out, v0=v0, aux_status=h["status"])


@pytest.mark.parametrize("no_lds", [False, True])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_device_route_equals_host_route_bit_for_bit(ctx, shape, no_lds):
    c = ctx(shape)
    p = c.p
    p.set_opts(reserved=NO_LDS if no_lds else 0)
    try:
        p.upload(c.x0, c.om, c.midx)
        p.solve_resident()
        plan = p.download()
        assert np.all(np.isin(plan["status"], (0, 2)) & np.isfinite(plan["obj"]))
        x_in, w_in = p.inputs()
        got = p.sim_step(resolve=c.R, outputs=True, advance=False, log=False)
        assert got["n_skipped"] == 0 and np.all(got["aux_status"] == 0) and got["aux_status"].dtype == np.int32
        u, w = plan["v"][:, :c.nu], w_in[:, :c.nw]
        ref = _host_route(c, x_in, u, w, c.midx)
        _equal(got, ref, OUT + ("v0", "aux_status"), shape)
        assert np.array_equal(got["v0"][:, :c.nu], u) and np.all(np.isin(got["v0"][:, c.nu], (0.0, 1.0)))
        _check_step(got, simlog.lsim_k_batch(c.mats, c.d, c.midx, x_in, got["v0"], w), _dims_nv(c.d), shape, drawn=False)
        # the host route has laid the resolver's batch out itself in between: the device route notices and lays it out again
        again = p.sim_step(resolve=c.R, outputs=True, advance=False, log=False)
        _equal(again, got, OUT + ("v0", "aux_status"), shape + " again")
        # a what-if moved nothing
        x_same, w_same = p.inputs()
        assert np.array_equal(x_same, x_in) and np.array_equal(w_same, w_in)
    finally:
        p.set_opts(reserved=0)


def _closed_form_checks(c, got, x, u, w, what):
    """delta exactly; sum(mu) to the project's 1e-6 max(1, sum(mu)); the reference's own residual statement <= 1e-6 max(1, max|x|) for the device's point"""
    cf = c.closed_form(x, u, w)
    assert np.all(np.abs(cf["y"]) >= 1e-3), what
    nu, d = c.nu, c.d
    dl, z, mu = got["v0"][:, nu:nu + 1], got["v0"][:, nu + 1:nu + 2], got["v0"][:, nu + 2:]
    assert np.array_equal(got["v0"][:, :nu], u) and np.array_equal(dl, cf["delta"]), what
    tot = cf["mu"].sum(axis=1)
    err_mu = np.abs(mu.sum(axis=1) - tot) / np.maximum(1.0, tot)
    res = np.array([_aux_ref.residual(c.mats[c.midx[b]], d, x[b], u[b], w[b], dl[b], z[b], mu[b]).max() / max(1.0, np.abs(x[b]).max()) for b in range(c.B)])
    print("%s: worst |sum(mu) - closed| / max(1, sum) %.3g, worst residual / max(1, max|x|) %.3g, worst |z - z_closed| / max(1, |y|) %.3g"
          % (what, err_mu.max(), res.max(), (np.abs(z[:, 0] - cf["z"][:, 0]) / np.maximum(1.0, np.abs(cf["y"]))).max()))
    assert np.all(err_mu <= 1e-6), what
    assert np.all(res <= 1e-6), what
    assert np.all(got["aux_status"] == 0) and got["n_skipped"] == 0, what
    return cf


@pytest.mark.parametrize("no_lds", [False, True])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_closed_form_under_realised_loads(ctx, shape, no_lds):
    """the case the feature exists for: the plan's inputs applied under a realised load that is not the forecast's.  The resolved step is consistent (every
    cons true) and equals the closed form; the step with the PLANNED slice is inconsistent wherever the grid power that occurred is not the planned one."""
    c = ctx(shape)
    p = c.p
    step = 1
    rng = np.random.default_rng(dict(a10=7811, a1=7813, b9=7812)[shape])
    lib, gw, astart, w_act = c.realised(rng, step)
    p.set_opts(reserved=NO_LDS if no_lds else 0)
    try:
        p.upload(c.x0, c.om, c.midx)
        p.upload_profiles(lib, gw)
        p.solve_resident()
        plan = p.download()
        v_plan = plan["v"][:, :c.nv]
        u = np.ascontiguousarray(v_plan[:, :c.nu])
        got = p.sim_step(resolve=c.R, u0=u, act_start=astart, step=step, advance=False, log=False, outputs=True)
        cf = _closed_form_checks(c, got, c.x0, u, w_act, shape + " inside the bounds")
        assert got["cons"].all(), shape                                      # tanks inside their bounds, auxiliaries that follow the model
        _check_step(got, simlog.lsim_k_batch(c.mats, c.d, c.midx, c.x0, got["v0"], w_act), _dims_nv(c.d), shape, drawn=False)
        # the planned slice under the same realised load.  z = delta y is the grid power: where the one that occurred is not the planned one, a row says so.
        # (An instance that planned delta = 0 and whose realised y is still negative has z = 0 either way: it is consistent, whatever |y| is.)
        old = p.sim_step(v0=v_plan, step=step, actual=True, advance=False, log=False, outputs=True)
        z_plan, d_plan = v_plan[:, c.nu + 1], v_plan[:, c.nu]
        moved = np.abs(cf["y"] - z_plan) > 1e-3
        moved &= ~((d_plan < 0.5) & (cf["y"] < 0))
        assert np.array_equal(moved, np.abs(cf["z"][:, 0] - z_plan) > 1e-3)
        assert moved.any() or c.B == 1, shape                                # (ten and nine instances have such; the single one need not)
        assert np.all(~old["cons"][moved].all(axis=1)), shape
        # tanks outside their soft bounds: the least total slack
        x_out, u_out, _ = _aux_ref.draw_triples(dict(dims=c.d, omega=c.om), c.B, rng)
        x_out[0, 0], x_out[-1, -1] = 47.0, 80.5                              # at least one tank below T_min and one above either T_max
        p.upload(x_out, c.om, c.midx)
        got = p.sim_step(resolve=c.R, u0=u_out, act_start=astart, step=step, advance=False, log=False, outputs=True)
        cf = _closed_form_checks(c, got, x_out, u_out, w_act, shape + " outside the bounds")
        assert cf["mu"][0, 1] == 3.0 and cf["mu"][-1, -2] >= 0.5
        soft = 2 * c.nx
        assert got["cons"][:, soft:].all() and np.array_equal(got["cons"][:, :soft], cf["mu"] == 0), shape      # (cons zeroes the Psi mu term, mld_model.py:692-694)
    finally:
        p.set_opts(reserved=0)


def test_masking_infeasible_auxiliaries_and_unusable_plans(ctx):
    # the hard 3-tank model: E x <= T_max has no slack, a tank at 90 degrees leaves the auxiliary problem infeasible
    c = ctx("a10", hard=True)
    p, B, N = c.p, c.B, c.N
    assert c.d["nmu"] == 0 and c.R.nv2 == 2
    hot = np.zeros(B, bool)
    hot[[1, 4, 7]] = True
    x = c.x0.copy()
    x[hot, 0] = 90.0
    u = np.zeros((B, c.nu))
    p.upload(x, c.om, c.midx)
    got = p.sim_step(resolve=c.R, u0=u, advance=True, log=False, outputs=True)
    assert got["n_skipped"] == 3
    assert np.all(got["aux_status"][hot] == INFEASIBLE) and np.all(got["aux_status"][~hot] == 0)
    for k in ("x_k1", "y", "v0", "cons_vio"):
        assert np.all(np.isnan(got[k][hot])) and np.all(np.isfinite(got[k][~hot])), k
    assert np.all(got["cons_row"][hot] == -1) and not got["cons"][hot].any()
    x_new, w_new = p.inputs()
    assert np.array_equal(x_new[hot], x[hot]) and np.array_equal(w_new[hot], c.om[hot])
    assert np.array_equal(x_new[~hot], got["x_k1"][~hot])
    assert np.array_equal(w_new[~hot].reshape(-1, N, c.nw), np.roll(c.om[~hot].reshape(-1, N, c.nw), -1, axis=1))
    ref = simlog.lsim_k_batch(c.mats, c.d, c.midx, x, np.where(hot[:, None], 0.0, got["v0"]), c.om[:, :c.nw])
    _check_step({k: got[k][~hot] for k in OUT}, {k: v[~hot] for k, v in ref.items()}, _dims_nv(c.d), "feasible instances", drawn=False)
    # u0 = None: an instance without a usable plan is not attempted (a cutoff just below its optimum: INFEASIBLE, as tests/test_gpu_trajectories.py does)
    s = ctx("a10")
    q = s.p
    first = q.solve(s.x0, s.om, s.midx)
    assert np.all(first["status"] == 0)
    q.upload(s.x0, s.om, s.midx)
    masked = np.arange(B) % 2 == 1
    cut = np.full(B, np.inf)
    cut[masked] = (first["obj"] - 1e-6 * np.maximum(1.0, np.abs(first["obj"])))[masked]
    q.set_cutoffs(cut)
    q.solve_resident()
    out = q.download()
    assert np.all(out["status"][masked] == 1) and np.all(out["status"][~masked] == 0)
    q.sim_log_begin(1)
    got = q.sim_step(resolve=s.R, outputs=True)
    assert got["n_skipped"] == masked.sum()
    assert np.all(got["aux_status"][masked] == -1) and np.all(got["aux_status"][~masked] == 0)
    assert np.all(np.isnan(got["v0"][masked])) and np.all(np.isnan(got["x_k1"][masked])) and np.all(np.isfinite(got["x_k1"][~masked]))
    x_new, w_new = q.inputs()
    assert np.array_equal(x_new[masked], s.x0[masked]) and np.array_equal(w_new[masked], s.om[masked]) and np.array_equal(x_new[~masked], got["x_k1"][~masked])
    log = q.sim_log()
    assert np.all(np.isnan(log["v"][0][masked])) and np.array_equal(log["v"][0][~masked], got["v0"][~masked])
    for name in ("obj", "lower_bound", "status", "nodes"):                  # the record's solve fields stay the plan's
        assert np.array_equal(log[name][0], out[name]), name
    assert np.array_equal(q.sim_log_aux()[0], got["aux_status"])


def test_advance_and_log(ctx):
    c = ctx("a10")
    p, B, N, nw = c.p, c.B, c.N, c.nw
    T = N + 6
    series = [np.tile(c.om[b].reshape(N, nw), (T // N + 1, 1))[:T] for b in range(B)]
    lib, base = profiles.pack(series)
    fstart = base.reshape(B, 1)
    p.upload(c.x0, c.om, c.midx)
    p.upload_profiles(lib)
    p.forecast_from_profiles(fstart, 0)
    p.sim_log_begin(4)
    outs, xs = [], []
    for k in range(3):
        p.solve_resident()
        xs.append(p.inputs()[0])
        outs.append(p.sim_step(resolve=c.R, outputs=True))             # advance and log default to True / "a log has begun"
        assert outs[k]["n_skipped"] == 0 and p.sim_log_count() == (k + 1, 4)
        p.warm_start_from_previous(1)                                   # accepted, as after advance()
        p.forecast_from_profiles(None, k + 1)
        assert np.array_equal(p.inputs()[0], outs[k]["x_k1"])
        with pytest.raises(gpu.MldGpuError, match="already been applied"):
            p.sim_step(resolve=c.R)
    log = p.sim_log()
    for k in range(3):
        assert np.array_equal(log["v"][k], outs[k]["v0"]) and np.array_equal(log["x"][k], xs[k]) and np.array_equal(log["x_k1"][k], outs[k]["x_k1"])
        assert np.array_equal(log["y"][k], outs[k]["y"]) and np.array_equal(log["cons"][k], outs[k]["cons"])
    assert np.array_equal(log["x_k1"][0], log["x"][1]) and np.array_equal(log["x_k1"][1], log["x"][2])
    aux = p.sim_log_aux()
    assert aux.shape == (3, B) and aux.dtype == np.int32 and np.all(aux == 0)
    p.solve_resident()
    assert p.sim_step() == 0                                            # a plain step appended to the same log: "not resolved"
    aux = p.sim_log_aux()
    assert aux.shape == (4, B) and np.all(aux[:3] == 0) and np.all(aux[3] == -2)
    assert np.array_equal(p.sim_log_aux(3, 1), aux[3:])
    with pytest.raises(gpu.MldGpuError, match=r"records \[3, 5\)"):
        p.sim_log_aux(3, 2)
    p.sim_log_begin(2)                                                  # a new log: the aux array is gone with the old one
    p.solve_resident()
    assert p.sim_step() == 0
    assert np.all(p.sim_log_aux() == -2)
    p.solve_resident()
    p.sim_step(resolve=c.R)
    assert np.array_equal(p.sim_log_aux(), np.repeat([[-2], [0]], B, axis=1))
    # the caller's u0 with ADVANCE: the handle ends as after select() -- no plan
    p.sim_log_begin(0)
    p.solve_resident()
    p.sim_step(resolve=c.R, u0=np.zeros(c.nu))
    with pytest.raises(gpu.MldGpuError, match="not been solved"):
        p.sim_step(resolve=c.R)


def test_second_upload_with_other_model_indices(ctx):
    c = ctx("a10")
    p = c.p
    p.upload(c.x0, c.om, c.midx)
    p.solve_resident()
    first = p.sim_step(resolve=c.R, outputs=True, advance=False, log=False)
    midx2 = ((c.midx + 1) % len(c.mats)).astype(np.int32)
    p.upload(c.x0, c.om, midx2)                                        # the same size: only the upload counter tells the resolver's batch is stale
    p.solve_resident()
    plan = p.download()
    got = p.sim_step(resolve=c.R, outputs=True, advance=False, log=False)
    assert got["n_skipped"] == 0
    u, w = plan["v"][:, :c.nu], c.om[:, :c.nw]
    h = c.R.resolve(c.x0, u, w, midx2)
    ref = dict(p.sim_step(v0=np.hstack([u, h["v"]]), advance=False, log=False, outputs=True), v0=np.hstack([u, h["v"]]))
    _equal(got, ref, OUT + ("v0",), "second upload")
    # every heater on: y = sum(P_h) + load tells the models apart, so stale indices would show
    rated = np.array([float(np.sum(m["D1"])) for m in c.mats])
    assert np.any(rated[c.midx] != rated[midx2])
    ones = np.ones((c.B, c.nu))
    on = p.sim_step(resolve=c.R, u0=ones, outputs=True, advance=False, log=False)
    new, stale = c.R.resolve(c.x0, ones, w, midx2), c.R.resolve(c.x0, ones, w, c.midx)
    assert np.array_equal(on["v0"][:, c.nu:], new["v"]) and not np.array_equal(new["v"], stale["v"])
    assert first["n_skipped"] == 0


def test_model_without_auxiliaries(ctx):
    c = ctx("a10", hard=True, tie=False)
    p, B = c.p, c.B
    assert c.nv == c.nu and c.R.nv2 == 0 and c.R.problem is None
    rng = np.random.default_rng(7860)
    u = (rng.uniform(size=(B, c.nu)) < 0.4).astype(float)
    p.upload(c.x0, c.om, c.midx)
    got = p.sim_step(resolve=c.R, u0=u, advance=False, log=False, outputs=True)
    ref = p.sim_step(v0=u, advance=False, log=False, outputs=True)
    _equal(got, ref, OUT, "nv2 == 0")
    assert np.array_equal(got["v0"], u) and np.all(got["aux_status"] == 0) and got["n_skipped"] == 0
    other = ctx("a10")
    lib = _lib.load()
    assert lib.mld_sim_step_resolve(p._h, other.R.problem._h, _lib.dptr(u), None, 0, 0, None, None, None, None, None, None, None, None) == -1
    assert b"aux must be NULL" in lib.mld_last_error()


def test_refusals_change_nothing(ctx):
    c, big = ctx("a10"), ctx("b9")
    p, R, B = c.p, c.R, c.B
    lib = _lib.load()
    p.upload(c.x0, c.om, c.midx)
    p.upload_profiles(np.zeros(0))                                      # (the problem is shared with the tests above: no library from here on)
    p.solve_resident()
    p.sim_log_begin(2)
    assert p.sim_step(resolve=R, advance=False, log=True) == 0
    # the resolver's batch: four instances of the host route, so that a layout for this batch would show
    four = R.resolve(c.x0[:4], np.zeros((4, c.nu)), c.om[:4, :c.nw], c.midx[:4])
    state = (p.inputs(), p.sim_log_count(), p.sim_log(), p.sim_log_aux())

    def unchanged(what):
        x_in, w_in = p.inputs()
        assert np.array_equal(x_in, state[0][0]) and np.array_equal(w_in, state[0][1]) and p.sim_log_count() == state[1], what
        st = R.problem.solve_resident()
        assert st["n_optimal"] + st["n_infeasible"] + st["n_node_limit"] + st["n_numerical"] == 4, what      # the resolver still holds ITS batch
        assert np.array_equal(R.problem.download()["v"], four["v"]), what

    def refused(match, **kw):
        with pytest.raises(gpu.MldGpuError, match=match):
            p.sim_step(resolve=kw.pop("resolve", R), **kw)
        unchanged(match)

    def raw(aux, flags=0, u0=None, start=None):
        rc = lib.mld_sim_step_resolve(p._h, aux, _lib.dptr(u0), start.ctypes.data_as(C.POINTER(C.c_int64)) if start is not None else None, 0, flags,
                                      None, None, None, None, None, None, None, None)
        msg = lib.mld_last_error()
        unchanged(msg)
        return rc, msg

    # everything mld_sim_step_batch refuses
    refused("step = -1", step=-1, advance=False)
    refused("no profile library", actual=True, advance=False)
    refused("no profile library", act_start=np.zeros((B, 1), np.int64), advance=False)
    rc, msg = raw(R.problem._h, flags=8)
    assert rc == -1 and b"unknown flag" in msg
    rc, msg = raw(R.problem._h, flags=1, start=np.zeros((B, 1), np.int64))
    assert rc == -1 and b"without MLD_SIM_ACTUAL" in msg
    assert lib.mld_sim_step_batch(p._h, None, None, 0, 8, None, None, None, None, None, None) == -1 and b"unknown flag" in lib.mld_last_error()
    # the resolver handle
    rc, msg = raw(p._h)
    assert rc == -1 and b"the stepped problem itself" in msg
    rc, msg = raw(None)
    assert rc == -1 and b"aux == NULL" in msg
    refused("not the fold", resolve=big.R, advance=False)
    two = gpu.GpuProblem(R._model, 1, 2, None)
    tv_model = gpu.GpuModel([[m] for m in R.mats2], R.dims2, time_varying=True)
    tv = gpu.GpuProblem(tv_model, 0, 1, None)
    try:
        rc, msg = raw(two._h)
        assert rc == -1 and b"N_tilde = 2" in msg
        rc, msg = raw(tv._h)
        assert rc == -1 and b"time-varying" in msg
    finally:
        two.close(); tv.close(); tv_model.close()
    # the caller's u0
    bad = np.zeros((B, c.nu))
    bad[6, 2] = np.nan
    refused("u0 of instance 6, input 2 is not finite", u0=bad, advance=False)
    bad[6, 2] = np.inf
    refused("not finite", u0=bad)
    # a full log
    assert p.sim_step(resolve=R, advance=False, log=True) == 0
    four = R.resolve(c.x0[:4], np.zeros((4, c.nu)), c.om[:4, :c.nw], c.midx[:4])      # (the step laid the resolver's batch out as this one)
    state = (state[0], p.sim_log_count(), p.sim_log(), p.sim_log_aux())
    assert state[1] == (2, 2)
    refused("log is full", log=True, advance=False)
    refused("log is full", u0=np.zeros(c.nu), log=True)
    again = p.sim_log()
    for name in again:
        assert np.array_equal(again[name], state[2][name], equal_nan=True), name
    assert np.array_equal(p.sim_log_aux(), state[3])
    # launched solves, on either handle
    R.problem.launch()
    with pytest.raises(gpu.MldGpuError, match="aux has a launched solve"):
        p.sim_step(resolve=R, advance=False, log=False)
    R.problem.finish()
    unchanged("aux in flight")
    p.launch()
    with pytest.raises(gpu.MldGpuError, match="has not been finished"):
        p.sim_step(resolve=R, advance=False, log=False)
    p.finish()
    unchanged("problem in flight")
    # no plan: after the caller's inputs have advanced the batch, u0 = None has nothing to take
    p.sim_log_begin(0)
    state = (state[0], (0, 0), None, None)
    refused("no log has been begun", log=True, advance=False)
    p.sim_step(resolve=R, u0=np.zeros(c.nu), advance=True)
    state = (p.inputs(), p.sim_log_count(), None, None)
    four = R.resolve(c.x0[:4], np.zeros((4, c.nu)), c.om[:4, :c.nw], c.midx[:4])
    refused("not been solved", advance=False)
    # the hand-off on the resolver (switching it drops the resolver's batch, so this comes last)
    R.problem.set_handoff(True)
    try:
        with pytest.raises(gpu.MldGpuError, match="hand-off on"):
            p.sim_step(resolve=R, u0=np.zeros(c.nu), advance=False)
    finally:
        R.problem.set_handoff(False)
    x_in, w_in = p.inputs()
    assert np.array_equal(x_in, state[0][0]) and np.array_equal(w_in, state[0][1])
    assert p.sim_step(resolve=R, u0=np.zeros(c.nu), advance=False) == 0      # ... and the handles still work
