"""Open-loop rollout of a resident batch under realised disturbances (mld_rollout_batch / GpuProblem.rollout, kernel k_rollout): the reference's MldModel.lsim,
lsim_k in a loop (models/mld_model.py:543-642, 647-699) with _compute_aux (:701-766) at every step, batch x S trajectories in one launch.  The yardstick is
the stepwise route the library already has -- K advancing sim_step(resolve=R) calls per realisation over the same flagged resolver --; every returned step
is checked against the model in numpy and the closed form of tests/_aux_ref.py; then start against omega_seq, determinism and position independence, the
reductions, every ending, the host completion of declined trajectories, the untouched handle and every refusal.  Last, what the one definition of the
plant step's sums (csrc/plant_step.inc) must keep: the rollout's plant rows equal k_sim_step's bit for bit given the same v_k, also without auxiliaries at
nc = 70 (lanes take a second row), and the largest residual's NaN and tie rules in both kernels.

Shapes (tests/test_gpu_sim_resolve.py): a10 -- n_h 3, three models interleaved, N_tilde 3, batch 10; a1 -- batch 1 (three of the four waves of the only
workgroup find no work); b9 -- n_h 7, batch 9.  S = 3 realisations, so batch x S is no multiple of the four waves of a workgroup for a10 and b9."""
import ctypes as C

import numpy as np
import pytest

import _paths
import _rollout_ref
from test_gpu_sim_resolve import NO_LDS, SHAPES
from test_gpu_small_lds_step import _SmallCtx
from pyhybridcontrol_amd import gpu, simlog, _lib
from pyhybridcontrol_amd.aux_resolve import BatchAuxResolver

pytestmark = pytest.mark.gpu

S, STEP = 3, 1
TRAJ = ("x", "v", "y", "cons_vio", "cons_row")
SUMM = ("cost", "mu_total", "worst_vio", "worst_step", "steps_done", "end_status")
_CACHE = {}


@pytest.fixture(scope="module")
def ctx():
    def get(name, **kw):
        key = (name,) + tuple(sorted(kw.items()))
        if key not in _CACHE:
            _CACHE[key] = _SmallCtx(*SHAPES[name], **kw)
        return _CACHE[key]
    yield get
    for c in _CACHE.values():
        c.close()
    _CACHE.clear()


def _scenario(c, K, seed):
    """(lib, group widths, start (B, S, 2), omega_seq (B, S, K, nomega), u_seq (B, K, nu)) of a context"""
    rng = np.random.default_rng(seed)
    lib, gw, start, om_seq = _rollout_ref.realised_library(c.om, c.N, c.nw, c.nx, S, K, STEP, rng)
    u_seq = (rng.uniform(size=(c.B, K, c.nu)) < 0.4).astype(float)
    return lib, gw, start, om_seq, u_seq


def _same(a, b, names, what):
    for k in names:
        assert np.array_equal(a[k], b[k], equal_nan=True), (what, k)


def _stepwise(c, u_ref, start, K):
    """the yardstick: per realisation, x0 uploaded and K advancing sim_step(resolve=R) calls; the arrays of a rollout"""
    p, B = c.p, c.B
    ref = dict(x=np.zeros((B, S, K + 1, c.nx)), v=np.zeros((B, S, K, c.nv)), y=np.zeros((B, S, K, c.d["ny"])), cons_vio=np.zeros((B, S, K)),
               cons_row=np.zeros((B, S, K), np.int32), aux_status=np.zeros((B, S, K), np.int32))
    for cc in range(S):
        p.upload(c.x0, c.om, c.midx)
        ref["x"][:, cc, 0] = c.x0
        for k in range(K):
            o = p.sim_step(resolve=c.R, u0=np.ascontiguousarray(u_ref[:, k]), act_start=np.ascontiguousarray(start[:, cc]), step=STEP + k, advance=True, outputs=True)
            c.in_lds()
            assert o["n_skipped"] == 0
            ref["x"][:, cc, k + 1], ref["v"][:, cc, k], ref["y"][:, cc, k] = o["x_k1"], o["v0"], o["y"]
            ref["cons_vio"][:, cc, k], ref["cons_row"][:, cc, k], ref["aux_status"][:, cc, k] = o["cons_vio"], o["cons_row"], o["aux_status"]
    return ref


def _against_stepwise(c, got, ref, K, what):
    """binaries, steps_done, end_status and cons_row equal; x, y, z, mu and cons_vio within 1e-6 max(1, |reference|) (the project's tolerance for this comparison,
    tests/test_gpu_sim_resolve.py::_closed_form_checks: only the summation order of the right-hand side differs between the two routes)"""
    nu = c.nu
    worst = 0.0
    for name, a, b in (("x", got["x"], ref["x"]), ("y", got["y"], ref["y"]), ("z, mu", got["v"][..., nu + 1:], ref["v"][..., nu + 1:]),
                       ("cons_vio", got["cons_vio"], ref["cons_vio"])):
        dev = np.abs(a - b) / np.maximum(1.0, np.abs(b))
        if dev.size:
            print("%s %s: worst |rollout - stepwise| / max(1, |stepwise|) = %.3g" % (what, name, dev.max()))
            worst = max(worst, float(dev.max()))
    print("%s: worst deviation from the stepwise route %.3g" % (what, worst))
    assert np.all(ref["aux_status"] == 0), what
    assert np.all(got["steps_done"] == K) and np.all(got["end_status"] == 0), what
    assert np.array_equal(got["v"][..., :nu + 1], ref["v"][..., :nu + 1]), what                   # u and the binaries
    assert np.array_equal(got["cons_row"], ref["cons_row"]), what
    assert worst <= 1e-6, what


@pytest.mark.parametrize("mode", ["one", "plan", "long"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_against_the_stepwise_route(ctx, shape, mode):
    """K = 1; K = N_tilde with the resident plan's inputs (u_seq=None); K = N_tilde + 2 with the caller's u_seq.
    Measured on the device (MI355X), worst deviation over all shapes and modes: see DESIGN.md section 6."""
    c = ctx(shape)
    p = c.p
    K = dict(one=1, plan=c.N, long=c.N + 2)[mode]
    lib, gw, start, om_seq, u_seq = _scenario(c, K, 9100 + 10 * list(SHAPES).index(shape) + K)
    try:
        p.upload(c.x0, c.om, c.midx)
        p.upload_profiles(lib, gw)
        if mode == "plan":
            p.solve_resident()
            plan = p.download()
            assert np.all(np.isin(plan["status"], (0, 2)) & np.isfinite(plan["obj"]))
            u_ref = np.ascontiguousarray(plan["v"].reshape(c.B, c.N, c.nv)[:, :K, :c.nu])
        else:
            u_ref = u_seq
        # the guard: no instance sits on a switching surface at any step of any trajectory, and none is left out
        assert np.all(np.abs(_rollout_ref.closed_y(c.mats, c.d, c.midx, u_ref, om_seq)) >= 1e-3)
        got = p.rollout(c.R, u_seq=None if mode == "plan" else u_seq, start=start, step=STEP, trajectories=True)
        assert got["x"].shape == (c.B, S, K + 1, c.nx) and got["end_status"].dtype == np.int32
        assert got["stats"] == dict(trajectories=c.B * S, complete=c.B * S, infeasible=0, declined=0, not_attempted=0, finished_on_host=0)
        ref = _stepwise(c, u_ref, start, K)
        _against_stepwise(c, got, ref, K, "%s %s" % (shape, mode))
    finally:
        p.upload_profiles(np.zeros(0))


def _check_every_step(c, got, u_ref, om_seq, K, what):
    """simlog.lsim_k_batch on the returned (x_k, v_k, omega_k) reproduces x_{k+1}, y, cons_vio and cons_row the way _check_step(..., drawn=False) of
    tests/test_gpu_sim_step.py compares them; the closed form gives delta exactly and sum(mu) to 1e-6"""
    B, nu, d = c.B, c.nu, c.d
    T = B * S
    midx = np.repeat(c.midx, S)
    bound = simlog.sum_bound(d)
    flat = {k: got[k].reshape((T,) + got[k].shape[2:]) for k in TRAJ}
    om, u = om_seq.reshape(T, K, c.nw), np.repeat(u_ref, S, axis=0)
    fn = _rollout_ref.closed_form_resolver(c.mats, d)
    at = np.arange(T)
    for k in range(K):
        x, v = flat["x"][:, k], flat["v"][:, k]
        ref = simlog.lsim_k_batch(c.mats, d, midx, x, v, om[:, k])
        assert np.all(np.abs(flat["x"][:, k + 1] - ref["x_k1"]) <= bound * ref["terms_x"]), (what, k)
        assert np.all(np.abs(flat["y"][:, k] - ref["y"]) <= bound * ref["terms_y"]), (what, k)
        rows = flat["cons_row"][:, k]
        assert rows.dtype == np.int32 and np.all((rows >= 0) & (rows < d["nc"])), (what, k)
        assert np.all(ref["resid"][at, rows] >= ref["cons_vio"] - 2 * bound * ref["terms_r"].max(axis=1)), (what, k)
        assert np.all(np.abs(flat["cons_vio"][:, k] - ref["resid"][at, rows]) <= bound * ref["terms_r"][at, rows]), (what, k)
        cf = fn(x, u[:, k], om[:, k], midx)["v"]
        assert np.array_equal(v[:, :nu], u[:, k]) and np.array_equal(v[:, nu], cf[:, 0]), (what, k)
        tot = cf[:, 2:].sum(axis=1)
        assert np.all(np.abs(v[:, nu + 2:].sum(axis=1) - tot) <= 1e-6 * np.maximum(1.0, tot)), (what, k)


@pytest.mark.parametrize("shape", list(SHAPES))
def test_each_step_is_the_models_and_start_equals_omega_seq(ctx, shape):
    c = ctx(shape)
    p = c.p
    K = c.N + 2
    lib, gw, start, om_seq, u_seq = _scenario(c, K, 9200 + list(SHAPES).index(shape))
    x0 = c.x0.copy()
    x0[0, 0], x0[-1, -1] = 47.0, 80.5                                      # slack on both sides somewhere
    assert np.all(np.abs(_rollout_ref.closed_y(c.mats, c.d, c.midx, u_seq, om_seq)) >= 1e-3)
    try:
        p.upload(x0, c.om, c.midx)
        p.upload_profiles(lib, gw)
        by_index = p.rollout(c.R, u_seq=u_seq, start=start, step=STEP, trajectories=True)
        assert by_index["stats"]["complete"] == c.B * S
        assert (by_index["v"][..., c.nu + 2:] > 0).any()
        _check_every_step(c, by_index, u_seq, om_seq, K, shape)
        uploaded = p.rollout(c.R, u_seq=u_seq, omega_seq=om_seq, trajectories=True)
        _same(by_index, uploaded, TRAJ + SUMM, shape)                      # the same windows by index (groups of widths 1 and nomega - 1, step = 1) and uploaded
        assert by_index["stats"] == uploaded["stats"]
    finally:
        p.upload_profiles(np.zeros(0))


@pytest.mark.parametrize("shape", list(SHAPES))
def test_determinism_and_position_independence(ctx, shape):
    c = ctx(shape)
    p = c.p
    K = c.N + 1
    _, _, _, om_seq, u_seq = _scenario(c, K, 9300 + list(SHAPES).index(shape))
    p.upload(c.x0, c.om, c.midx)
    one = p.rollout(c.R, u_seq=u_seq, omega_seq=om_seq, trajectories=True)
    two = p.rollout(c.R, u_seq=u_seq, omega_seq=om_seq, trajectories=True)
    _same(one, two, TRAJ + SUMM, shape + " twice")
    p.upload(c.x0[::-1], c.om[::-1], np.ascontiguousarray(c.midx[::-1]))
    rev = p.rollout(c.R, u_seq=u_seq[::-1], omega_seq=om_seq[::-1], trajectories=True)
    _same({k: v[::-1] for k, v in rev.items() if k != "stats"}, one, TRAJ + SUMM, shape + " reversed")
    summaries_only = p.rollout(c.R, u_seq=u_seq[::-1], omega_seq=om_seq[::-1])
    assert sorted(summaries_only) == sorted(SUMM + ("stats",))
    _same(summaries_only, rev, SUMM, shape + " summaries only")


@pytest.mark.parametrize("rows", ["model", "instance"])
def test_reductions(ctx, rows):
    c = ctx("a10")
    p, B = c.p, c.B
    K = c.N + 2
    _, _, _, om_seq, u_seq = _scenario(c, K, 9400)
    rng = np.random.default_rng(9401)
    cw = rng.uniform(0.5, 2.0, size=(len(c.mats) if rows == "model" else B, K, c.nv))
    x0 = c.x0.copy()
    x0[:, 0] = 47.0                                                         # every trajectory carries slack: mu_total > 0
    p.upload(x0, c.om, c.midx)
    got = p.rollout(c.R, u_seq=u_seq, omega_seq=om_seq, cost_w=cw, trajectories=True)
    assert np.all(got["end_status"] == 0)
    w = cw[c.midx] if rows == "model" else cw
    cost = np.einsum("bkj,bskj->bs", w, got["v"])
    mu = got["v"][..., c.nu + 2:].sum(axis=(2, 3))
    assert np.all(mu > 0)
    assert np.all(np.abs(got["cost"] - cost) <= 1e-12 * np.abs(cost)) and np.all(np.abs(got["mu_total"] - mu) <= 1e-12 * np.abs(mu))
    vio = got["cons_vio"]
    assert np.array_equal(got["worst_vio"], vio.max(axis=2)) and np.array_equal(got["worst_step"], vio.argmax(axis=2))      # (argmax: the earliest step of equals)
    print("trajectories whose worst violation is attained at more than one step: %d of %d" % (int(((vio == vio.max(axis=2, keepdims=True)).sum(axis=2) > 1).sum()), B * S))
    none = p.rollout(c.R, u_seq=u_seq, omega_seq=om_seq)
    assert np.all(none["cost"] == 0.0) and np.array_equal(none["mu_total"], got["mu_total"])


def test_endings(ctx):
    # the hard 3-tank model: no slack on the tank rows, a tank above T_max leaves the auxiliary problem without a feasible point
    c = ctx("a10", hard=True)
    p, B, K = c.p, c.B, 4
    assert c.d["nmu"] == 0 and c.R.nv2 == 2
    _, _, _, om_seq, _ = _scenario(c, K, 9500)
    fn = _rollout_ref.closed_form_resolver(c.mats, c.d)
    hot, heat = np.arange(B) % 3 == 1, np.arange(B) % 3 == 2
    x0 = c.x0.copy()
    x0[hot, 0] = 90.0
    u_seq = np.zeros((B, K, c.nu))
    u_seq[heat, 1, 0] = 1.0                                                 # tank 0 heated during step 1: found below, the start from which it is above T_max at step 2
    for b in np.where(heat)[0]:
        for t0 in np.arange(80.0, 55.0, -0.25):
            x0[b, 0] = t0
            r = simlog.rollout_np(c.mats, c.d, c.midx[b:b + 1], x0[b:b + 1], u_seq[b:b + 1], om_seq[b:b + 1], fn)
            if np.all(r["end_status"] == 1) and np.all(r["steps_done"] == 2):
                break
    ref = simlog.rollout_np(c.mats, c.d, c.midx, x0, u_seq, om_seq, fn)
    assert np.all(ref["end_status"][hot] == 1) and np.all(ref["steps_done"][hot] == 0)
    assert np.all(ref["end_status"][heat] == 1) and np.all(ref["steps_done"][heat] == 2)
    assert np.all(ref["end_status"][~hot & ~heat] == 0) and np.all(ref["steps_done"][~hot & ~heat] == K)
    assert np.all(np.abs(_rollout_ref.closed_y(c.mats, c.d, c.midx, u_seq, om_seq)) >= 1e-3)
    p.upload(x0, c.om, c.midx)
    got = p.rollout(c.R, u_seq=u_seq, omega_seq=om_seq, trajectories=True)
    assert np.array_equal(got["end_status"], ref["end_status"]) and np.array_equal(got["steps_done"], ref["steps_done"])
    n1 = int((hot | heat).sum()) * S
    assert got["stats"] == dict(trajectories=B * S, complete=B * S - n1, infeasible=n1, declined=0, not_attempted=0, finished_on_host=0)
    for b in range(B):
        for cc in range(S):
            sd, dead = got["steps_done"][b, cc], got["end_status"][b, cc] == 1
            assert np.all(np.isfinite(got["x"][b, cc, :sd + 1])) and np.all(np.isnan(got["x"][b, cc, sd + 1:]))
            for k in ("v", "y", "cons_vio"):
                assert np.all(np.isfinite(got[k][b, cc, :sd])) and np.all(np.isnan(got[k][b, cc, sd:])), k
            assert np.all(got["cons_row"][b, cc, :sd] >= 0) and np.all(got["cons_row"][b, cc, sd:] == -1)
            assert dead == bool(np.isnan(got["cost"][b, cc]) and np.isnan(got["mu_total"][b, cc]) and np.isnan(got["worst_vio"][b, cc]) and got["worst_step"][b, cc] == -1)
    live = got["end_status"] == 0
    assert np.allclose(got["x"][live], ref["x"][live], rtol=1e-9, atol=0) and np.array_equal(got["v"][live][..., c.nu], ref["v"][live][..., c.nu])
    # unusable plans with u_seq=None (a cutoff just below the optimum, as tests/test_gpu_sim_resolve.py makes them): not attempted
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
    assert np.all(q.download()["status"][masked] == 1)
    _, _, _, om3, _ = _scenario(s, s.N, 9501)
    got = q.rollout(s.R, omega_seq=om3, trajectories=True)
    assert np.all(got["end_status"][masked] == -1) and np.all(got["end_status"][~masked] == 0) and np.all(got["steps_done"][masked] == 0)
    for k in TRAJ[:-1] + SUMM[:3]:
        assert np.all(np.isnan(got[k][masked])) and np.all(np.isfinite(got[k][~masked])), k
    assert np.all(got["cons_row"][masked] == -1) and np.all(got["worst_step"][masked] == -1)
    st = got["stats"]
    assert st["not_attempted"] == masked.sum() * S and st["complete"] == (~masked).sum() * S and st["infeasible"] == st["declined"] == 0
    # the model without auxiliaries: a plain lsim
    e = ctx("a10", hard=True, tie=False)
    assert e.nv == e.nu and e.R.nv2 == 0 and e.R.problem is None
    _, _, _, om_e, u_e = _scenario(e, K, 9502)
    e.p.upload(e.x0, e.om, e.midx)
    got = e.p.rollout(e.R, u_seq=u_e, omega_seq=om_e, trajectories=True)
    assert got["stats"]["complete"] == B * S and np.all(got["mu_total"] == 0.0)
    bound = simlog.sum_bound(e.d)
    midx = np.repeat(e.midx, S)
    for k in range(K):
        x, v = got["x"][:, :, k].reshape(B * S, -1), got["v"][:, :, k].reshape(B * S, -1)
        assert np.array_equal(v, np.repeat(u_e[:, k], S, axis=0))
        r = simlog.lsim_k_batch(e.mats, e.d, midx, x, v, om_e[:, :, k].reshape(B * S, -1))
        assert np.all(np.abs(got["x"][:, :, k + 1].reshape(B * S, -1) - r["x_k1"]) <= bound * r["terms_x"])
        assert np.all(np.abs(got["cons_vio"][:, :, k].reshape(-1) - r["cons_vio"]) <= bound * r["terms_r"].max(axis=1))


def _raw(p, R, K, u_seq, om_seq):
    """the C call itself, summaries only"""
    B = p.batch
    es, sd, stats = np.zeros((B, S), np.int32), np.zeros((B, S), np.int32), np.zeros(4, np.int64)
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    rc = _lib.load().mld_rollout_batch(p._h, R.problem._h, K, S, _lib.dptr(u_seq), _lib.dptr(om_seq), None, 0, None, 0, None, None, None, None, None, None, None,
                                       None, None, ip(sd), ip(es), stats.ctypes.data_as(C.POINTER(C.c_int64)))
    return rc, es, sd, stats


def test_host_completion(ctx):
    c = ctx("a10")
    p, B = c.p, c.B
    K = c.N
    _, _, _, om_seq, u_seq = _scenario(c, K, 9600)
    x0 = c.x0.copy()
    x0[0, 0] = 47.0
    p.upload(x0, c.om, c.midx)
    want = p.rollout(c.R, u_seq=u_seq, omega_seq=om_seq, trajectories=True)
    assert want["stats"]["declined"] == 0
    c.R.problem.set_opts(reserved=_lib.MLD_DBG_SMALL_PIVOT_CAP)
    try:
        rc, es, sd, stats = _raw(p, c.R, K, u_seq, om_seq)
        assert rc == 0 and np.all(es == 2) and np.all(sd == 0) and list(stats) == [B * S, 0, 0, B * S]
        got = p.rollout(c.R, u_seq=u_seq, omega_seq=om_seq, trajectories=True)
        assert got["stats"] == dict(trajectories=B * S, complete=B * S, infeasible=0, declined=B * S, not_attempted=0, finished_on_host=B * S)
        _against_stepwise(c, got, dict(want, aux_status=np.zeros(1, np.int32)), K, "finished on the host")
        for k in ("mu_total", "worst_vio"):
            assert np.all(np.abs(got[k] - want[k]) <= 1e-6 * np.maximum(1.0, np.abs(want[k]))), k
        lean = p.rollout(c.R, u_seq=u_seq, omega_seq=om_seq)
        assert sorted(lean) == sorted(SUMM + ("stats",)) and lean["stats"]["finished_on_host"] == B * S
        _same(lean, got, SUMM, "summaries only")
    finally:
        c.R.problem.set_opts(reserved=0)


def test_the_handle_is_untouched(ctx):
    c = ctx("a10")
    p, B = c.p, c.B
    K = c.N
    lib, gw, start, om_seq, u_seq = _scenario(c, K, 9700)
    try:
        p.upload(c.x0, c.om, c.midx)
        p.upload_profiles(lib, gw)
        p.sim_log_begin(2)
        p.solve_resident()
        astart = np.ascontiguousarray(start[:, 0])
        before_step = p.sim_step(act_start=astart, step=STEP, advance=False, log=False, outputs=True)      # (makes the actual starts resident)
        before = (p.inputs(), p.download(), p.sim_log_count())
        for kw in (dict(start=start, step=STEP), dict(omega_seq=om_seq, u_seq=u_seq), dict(start=start, step=STEP, trajectories=True)):
            p.rollout(c.R, **kw)
            x_in, w_in = p.inputs()
            assert np.array_equal(x_in, before[0][0]) and np.array_equal(w_in, before[0][1]) and p.sim_log_count() == before[2]
            after = p.download()
            for k in after:
                assert np.array_equal(after[k], before[1][k], equal_nan=True), k
        after_step = p.sim_step(actual=True, step=STEP, advance=False, log=False, outputs=True)               # act_start=None: the resident starts
        for k in before_step:
            assert np.array_equal(before_step[k], after_step[k], equal_nan=True), k
        p.solve_resident()
        again = p.download()
        for k in ("v", "obj", "status", "lower_bound", "nodes", "pivots"):
            assert np.array_equal(again[k], before[1][k], equal_nan=True), k
    finally:
        p.sim_log_begin(0)
        p.upload_profiles(np.zeros(0))


def test_refusals_change_nothing(ctx):
    c, big = ctx("a10"), ctx("b9")
    p, B = c.p, c.B
    K = c.N
    lib, gw, start, om_seq, u_seq = _scenario(c, K, 9800)
    plain = BatchAuxResolver(c.mats, c.d)                                   # not flagged: the dense path's resolver
    tv_model = gpu.GpuModel([[m] * c.N for m in c.mats], c.d, time_varying=True)
    tv = gpu.GpuProblem(tv_model, c.N - 1, c.N, None)
    try:
        p.upload(c.x0, c.om, c.midx)
        p.upload_profiles(lib, gw)
        p.solve_resident()
        state = (p.inputs(), p.download())
        good = p.rollout(c.R, start=start, step=STEP)

        def refused(match, resolve=c.R, exc=gpu.MldGpuError, **kw):
            with pytest.raises(exc, match=match):
                p.rollout(resolve, **kw)
            x_in, w_in = p.inputs()
            assert np.array_equal(x_in, state[0][0]) and np.array_equal(w_in, state[0][1]), match
            now = p.download()
            for k in now:
                assert np.array_equal(now[k], state[1][k], equal_nan=True), (match, k)

        refused("not on the small-problem path.*mld_sim_step_resolve", resolve=plain, start=start, step=STEP)
        refused("not the fold", resolve=big.R, start=start, step=STEP)
        refused("N_tilde = %d" % c.N, K=c.N + 1, omega_seq=np.zeros((B, S, c.N + 1, c.nw)))
        refused("exactly one of omega_seq and start", exc=ValueError, omega_seq=om_seq, start=start)
        refused("exactly one of omega_seq and start", exc=ValueError)
        lp = lambda a: a.ctypes.data_as(C.POINTER(C.c_int64))
        for om, st, word in ((om_seq, start, b"both are"), (None, None, b"neither is")):
            rc = _lib.load().mld_rollout_batch(p._h, c.R.problem._h, K, S, None, _lib.dptr(om), lp(st) if st is not None else None, STEP, None, 0,
                                               None, None, None, None, None, None, None, None, None, None, None, None)
            assert rc == -1 and b"exactly one of omega_seq and start" in _lib.load().mld_last_error() and word in _lib.load().mld_last_error()
        out = start.copy()
        out[B - 1, S - 1, 1] = lib.size - (STEP + K) * (c.nw - 1) + 1      # one double past the last valid start
        refused("leaves the library", start=out, step=STEP)
        out[B - 1, S - 1, 1] = -1
        refused("leaves the library", start=out, step=STEP)
        bad = u_seq.copy()
        bad[6, 1, 2] = np.nan
        refused("u_seq of instance 6, step 1, input 2 is not finite", u_seq=bad, start=start, step=STEP)
        bad[6, 1, 2] = np.inf
        refused("not finite", u_seq=bad, omega_seq=om_seq)
        tv.upload(c.x0, c.om, c.midx)
        with pytest.raises(gpu.MldGpuError, match="time-varying"):
            tv.rollout(c.R, u_seq=u_seq, omega_seq=om_seq)
        again = p.rollout(c.R, start=start, step=STEP)                       # ... and one good call afterwards still works
        _same(again, good, SUMM, "after the refusals")
        assert again["stats"] == good["stats"] and again["stats"]["complete"] == B * S
    finally:
        plain.close(); tv.close(); tv_model.close()
        p.upload_profiles(np.zeros(0))


# ---- the plant step's arithmetic is ONE definition (csrc/plant_step.inc): the rollout's rows against k_sim_step's, bit for bit ----------------------------
def _by_sim_step(p, got, om_seq, forecast, midx):
    """per realisation and step the what-if sim_step(v0 = the rollout's v_k) on the rollout's own x_k, with omega_k as the forecast's step 0:
    dict(x_k1, y, cons_vio, cons_row) shaped (B, S, K, ...) like the rollout's arrays"""
    K, nw = got["v"].shape[2], om_seq.shape[-1]
    ref = dict(x_k1=np.zeros_like(got["x"][:, :, 1:]), y=np.zeros_like(got["y"]), cons_vio=np.zeros_like(got["cons_vio"]), cons_row=np.zeros_like(got["cons_row"]))
    for cc in range(got["v"].shape[1]):
        for k in range(K):
            om = forecast.copy()
            om[:, :nw] = om_seq[:, cc, k]
            p.upload(np.ascontiguousarray(got["x"][:, cc, k]), om, midx)
            o = p.sim_step(v0=np.ascontiguousarray(got["v"][:, cc, k]), advance=False, log=False, outputs=True)
            assert o["n_skipped"] == 0
            for name in ref:
                ref[name][:, cc, k] = o[name]
    return ref


def _same_plant_rows(got, ref, what):
    assert np.array_equal(got["x"][:, :, 1:], ref["x_k1"]), (what, "x_k1")
    for name in ("y", "cons_vio", "cons_row"):
        assert np.array_equal(got[name], ref[name], equal_nan=name == "cons_vio"), (what, name)


@pytest.mark.parametrize("shape", ["a10", "b9"])
def test_plant_rows_equal_sim_step_bit_for_bit(ctx, shape):
    """given the same v_k the two kernels run the same sums (the 1e-6 of the stepwise comparison belongs to the right-hand side's order alone)"""
    c = ctx(shape)
    p, K = c.p, 3
    _, _, _, om_seq, u_seq = _scenario(c, K, 9900 + list(SHAPES).index(shape))
    p.upload(c.x0, c.om, c.midx)
    got = p.rollout(c.R, u_seq=u_seq, omega_seq=om_seq, trajectories=True)
    assert got["stats"]["complete"] == c.B * S and got["x"].shape == (c.B, S, K + 1, c.nx)
    _same_plant_rows(got, _by_sim_step(p, got, om_seq, c.om, c.midx), shape)


# no auxiliaries, a row family above the wave (nc = 70: lanes take a second constraint row) and nx + nv + nomega = 97 staged values (tests/test_gpu_sim_step.py: BIG)
PLAIN = dict(nx=17, nu=40, nomega=40, ny=4, nc=70)
PLAIN_N = 2
J0 = 7      # the disturbance channel that is exactly 0 in test_merge_rules_*


class _Plain(object):
    def __init__(self, mats):
        self.d = _paths.make_dims(**PLAIN)
        self.model = gpu.GpuModel(mats, self.d)
        self.p = gpu.GpuProblem(self.model, PLAIN_N - 1, PLAIN_N, None)

    def close(self):
        self.p.close(); self.model.close()


def _plain_inputs(seed, B, n_real, K, zero_channel=None):
    rng = np.random.default_rng(seed)
    x0, forecast = rng.standard_normal((B, PLAIN["nx"])), rng.standard_normal((B, PLAIN_N, PLAIN["nomega"]))
    u_seq, om_seq = rng.standard_normal((B, K, PLAIN["nu"])), rng.standard_normal((B, n_real, K, PLAIN["nomega"]))
    if zero_channel is not None:
        forecast[..., zero_channel] = 0.0
        om_seq[..., zero_channel] = 0.0
    return x0, forecast.reshape(B, -1), u_seq, om_seq, (np.arange(B) % 2).astype(np.int32)


def test_no_auxiliaries_rows_beyond_the_wave():
    """aux=None at nc = 70: bit for bit the what-if sim_step(v0=u_k) per realisation and step, and simlog.rollout_np within the bound of
    tests/test_gpu_sim_step.py::test_kernel_against_numpy -- simlog.sum_bound(dims) times the row's sum of |terms| -- carried along the chain: the state the
    step starts from may differ by the previous step's bound e, which adds |A| e, |C| e and (|E| + |G| |C|) e to the rows (first order, as the bound itself)"""
    d = _paths.make_dims(**PLAIN)
    nx, nu, nw, ny = d["nx"], d["nu"], d["nomega"], d["ny"]
    assert 8 * ((2 * nx + nw + nu + 0 + nu + ny + 1) & ~1) <= 16 * 1024      # ro_stage_doubles(nx, nu, nw, 0, nv, ny) against SM_WAVE_BUDGET
    mats = [_paths.random_mld(9910 + i, rho=0.9, **PLAIN)[0] for i in range(2)]
    B, n_real, K = 5, 3, 2
    T = B * n_real
    x0, forecast, u_seq, om_seq, midx = _plain_inputs(9912, B, n_real, K)
    c = _Plain(mats)
    try:
        c.p.upload(x0, forecast, midx)
        got = c.p.rollout(None, u_seq=u_seq, omega_seq=om_seq, trajectories=True)
        assert got["stats"] == dict(trajectories=T, complete=T, infeasible=0, declined=0, not_attempted=0, finished_on_host=0)
        assert np.array_equal(got["v"], np.broadcast_to(u_seq[:, None], got["v"].shape)) and np.all(got["mu_total"] == 0.0) and np.all(got["steps_done"] == K)
        _same_plant_rows(got, _by_sim_step(c.p, got, om_seq, forecast, midx), "plain")
    finally:
        c.close()
    ref = simlog.rollout_np(mats, d, midx, x0, u_seq, om_seq, None)
    bound = simlog.sum_bound(d)
    mT = np.repeat(midx, n_real)
    absm = {name: np.stack([np.abs(m[name]) for m in mats])[mT] for name in ("A", "C", "E", "G")}
    through = lambda name, e: np.einsum("tij,tj->ti", absm[name], e)
    flat = lambda a: a.reshape((T,) + a.shape[2:])
    e_x = np.zeros((T, nx))
    for k in range(K):
        st = simlog.lsim_k_batch(mats, d, mT, flat(ref["x"])[:, k], np.repeat(u_seq[:, k], n_real, axis=0), flat(om_seq)[:, k])
        tol_x, tol_y = bound * st["terms_x"] + through("A", e_x), bound * st["terms_y"] + through("C", e_x)
        tol_r = (bound * st["terms_r"] + through("E", e_x) + through("G", through("C", e_x))).max(axis=1)
        err_x, err_y = np.abs(flat(got["x"])[:, k + 1] - flat(ref["x"])[:, k + 1]), np.abs(flat(got["y"])[:, k] - flat(ref["y"])[:, k])
        err_r = np.abs(flat(got["cons_vio"])[:, k] - flat(ref["cons_vio"])[:, k])
        print("step %d: worst err / tolerance  x %.3f  y %.3f  cons_vio %.3f" % (k, (err_x / tol_x).max(), (err_y / tol_y).max(), (err_r / tol_r).max()))
        assert np.all(err_x <= tol_x) and np.all(err_y <= tol_y) and np.all(err_r <= tol_r), k
        r = np.sort(st["resid"], axis=1)
        clear = r[:, -1] - r[:, -2] > 2 * tol_r                                # the largest residual leads by more than both routes' rounding
        assert clear.any() and np.array_equal(flat(got["cons_row"])[clear, k], flat(ref["cons_row"])[clear, k]), k
        e_x = tol_x


def _edited(seed, edit):
    mats = {k: np.array(v, copy=True) for k, v in _paths.random_mld(seed, rho=0.9, **PLAIN)[0].items()}
    edit(mats)
    return mats


def _merge_rules(mats, rows, nan):
    """sim_step with the LDS staging and without, and the rollout, on two interleaved models whose largest residual sits at rows[model]; nan: it is a NaN"""
    d = _paths.make_dims(**PLAIN)
    B, n_real, K = 4, 2, 2
    x0, forecast, u_seq, om_seq, midx = _plain_inputs(9930, B, n_real, K, zero_channel=J0)
    om_seq[:, 0, 0] = forecast[:, :d["nomega"]]                                # trajectory (b, 0) starts with the step sim_step takes
    want = np.array(rows, np.int32)[midx]
    with np.errstate(invalid="ignore"):
        st = simlog.lsim_k_batch(mats, d, midx, x0, u_seq[:, 0], forecast[:, :d["nomega"]])
    at = np.arange(B)
    if nan:      # the construction: the wanted row is the only NaN, and a finite residual larger than every other sits at row 2
        assert np.all(np.isnan(st["resid"][at, want])) and np.all(np.isnan(st["resid"]).sum(axis=1) == 1) and np.all(np.nanargmax(st["resid"], axis=1) == 2)
    else:        # the construction: the maximum is attained twice, first at the wanted row
        assert np.array_equal(st["cons_row"], want) and np.all((st["resid"] == st["cons_vio"][:, None]).sum(axis=1) == 2)
    c = _Plain(mats)
    try:
        p = c.p
        p.upload(x0, forecast, midx)
        steps = []
        for reserved in (0, NO_LDS):
            p.set_opts(reserved=reserved)
            steps.append(p.sim_step(v0=u_seq[:, 0], advance=False, log=False, outputs=True))
        p.set_opts(reserved=0)
        got = p.rollout(None, u_seq=u_seq, omega_seq=om_seq, trajectories=True)
    finally:
        c.close()
    for o, what in zip(steps, ("LDS", "global memory")):
        assert np.array_equal(o["cons_row"], want), what
        if nan:
            assert np.all(np.isnan(o["cons_vio"])) and not o["cons"][at, want].any(), what
        else:
            assert np.all(np.abs(o["cons_vio"] - st["cons_vio"]) <= simlog.sum_bound(d) * st["terms_r"][at, want]), what
            assert np.array_equal(o["cons_vio"], steps[0]["cons_vio"]), what
    assert np.all(got["end_status"] == 0)
    assert np.array_equal(got["cons_row"], np.broadcast_to(want[:, None, None], got["cons_row"].shape))
    if nan:
        assert np.all(np.isnan(got["cons_vio"])) and np.all(np.isnan(got["worst_vio"])) and np.all(got["worst_step"] == 0)      # (the earliest step of equals)
        assert np.all(np.isfinite(got["x"])) and np.all(np.isfinite(got["y"]))
    else:
        assert np.array_equal(got["cons_vio"][:, 0, 0], steps[0]["cons_vio"])
        assert np.array_equal(got["worst_vio"], got["cons_vio"].max(axis=2)) and np.array_equal(got["worst_step"], got["cons_vio"].argmax(axis=2))


def _tie(lo, hi):
    def edit(m):
        for name in ("E", "F1", "F4", "G", "f5"):
            m[name][hi] = m[name][lo]
        m["f5"][lo] = m["f5"][hi] = -1.0e3      # residual about +1e3: above every other row
    return edit


def _nan(row):
    def edit(m):
        m["F4"][row, J0] = np.inf              # against omega[J0] = 0: the residual of `row` is a NaN
        m["f5"][2] = -1.0e3
    return edit


def test_merge_rules_ties_go_to_the_lower_row():
    """equal residuals: rows 3 and 67 are two passes of ONE lane (the first of equals stays), rows 9 and 40 sit in two lanes (the merge prefers the lower row)"""
    _merge_rules([_edited(9920, _tie(3, 67)), _edited(9921, _tie(9, 40))], (3, 9), nan=False)


def test_merge_rules_a_nan_wins():
    """a NaN residual beats the finite larger one at row 2: row 66 is lane 2's own second pass, row 50 another lane's"""
    _merge_rules([_edited(9922, _nan(66)), _edited(9923, _nan(50))], (66, 50), nan=True)
