"""Closed-loop rollout of a rule-based feedback policy on the device (mld_rollout_policy / GpuProblem.rollout(policy=True), kernel k_rollout_policy): the
reference's `thermo` baseline (examples/residential_mg_with_pv_and_dewhs/theromstat_control.py:38-64) stepped K times under S realisations, batch x S
trajectories in one launch.  The yardstick is the stepwise route the library already has -- per realisation K advancing
sim_step(resolve=R, u0=apply_np(x_k, u_prev)) calls with the rule applied on the host --; every returned step is checked against the model in numpy;
then the rule's ties, mixed modes, a non-unit selector, u_prev against the resident state, determinism and position independence, an infeasible
ending, the host completion of declined trajectories, the untouched handle, every refusal, and the open-loop rollout beside a resident policy.

The guard (a condition, not a tolerance): the two device routes may differ by rounding in x (the project's bound for that comparison is 1e-6), so on the
numpy reference every selector value of every trajectory and step stays at least 1e-4 away from both thresholds.  It excludes no instance.

Shapes (tests/test_gpu_sim_resolve.py): a10 -- n_h 3, three models interleaved, batch 10; a1 -- batch 1; b9 -- n_h 7, batch 9.  S = 3."""
import ctypes as C

import numpy as np
import pytest

import _rollout_ref
from test_gpu_sim_resolve import SHAPES
from test_gpu_small_lds_step import _SmallCtx
from test_gpu_rollout import _against_stepwise, _scenario, _stepwise
from pyhybridcontrol_amd import gpu, policy, simlog, _lib
from pyhybridcontrol_amd.aux_resolve import BatchAuxResolver

pytestmark = pytest.mark.gpu

S, STEP = 3, 1
TRAJ = ("x", "v", "y", "cons_vio", "cons_row")
SUMM = ("cost", "mu_total", "worst_vio", "worst_step", "steps_done", "end_status", "switches")
GUARD = 1e-4
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


def thermostat(c, on_at=57.5, off_at=60.5, **kw):
    """the reference's thermostat over a context's models: channel j on tank j, thresholds on the half-integer grid (the states start on integers)"""
    return policy.ThresholdPolicy(np.broadcast_to(np.eye(c.nx), (len(c.mats), c.nu, c.nx)), on_at, off_at, **kw)


def reference(c, P, x0, u_seq, om_seq, u_prev=None):
    """simlog.rollout_np(policy=P) with the closed form as resolver, after the guards: every selector value of every trajectory and step at least 1e-4
    away from both thresholds, and (as tests/test_gpu_rollout.py) no instance on the switching surface of delta.  Prints the margin."""
    B, K = u_seq.shape[:2]
    ref = simlog.rollout_np(c.mats, c.d, c.midx, x0, u_seq, om_seq, _rollout_ref.closed_form_resolver(c.mats, c.d), policy=P, u_prev=u_prev)
    midx = np.repeat(c.midx, S)
    live = np.arange(K)[None, None, :] < ref["steps_done"][:, :, None]
    s = np.stack([policy.selector_values(P, midx, ref["x"][:, :, k].reshape(B * S, -1)) for k in range(K)], axis=1).reshape(B, S, K, c.nu)
    ruled = np.broadcast_to((P.mode[c.midx] == 1)[:, None, None, :], s.shape) & live[..., None]
    margin = np.minimum(np.abs(s - P.on_at[c.midx][:, None, None, :]), np.abs(s - P.off_at[c.midx][:, None, None, :]))[ruled]
    print("selector margin to the thresholds: %.3g over %d values" % (margin.min(), margin.size))
    assert margin.min() >= GUARD
    D1 = np.stack([np.asarray(m["D1"], float).reshape(-1) for m in c.mats])[c.midx]
    y = np.einsum("bskj,bj->bsk", ref["v"][..., :c.nu], D1) + om_seq[..., c.nx]
    assert np.all(np.abs(y[live]) >= 1e-3)
    return ref


def _same(a, b, names, what):
    for k in names:
        assert np.array_equal(a[k], b[k], equal_nan=True), (what, k)


def _against_reference(c, got, ref, what):
    """the discrete results equal -- endings, u and the binaries, cons_row, switches --, the continuous ones within 1e-6 max(1, |reference|)"""
    nu = c.nu
    for k in ("end_status", "steps_done", "switches"):
        assert np.array_equal(got[k], ref[k]), (what, k)
    assert np.array_equal(got["v"][..., :nu + 1], ref["v"][..., :nu + 1], equal_nan=True), what
    worst = 0.0
    for name, a, b in (("x", got["x"], ref["x"]), ("y", got["y"], ref["y"]), ("z, mu", got["v"][..., nu + 1:], ref["v"][..., nu + 1:]), ("cons_vio", got["cons_vio"], ref["cons_vio"])):
        assert np.array_equal(np.isnan(a), np.isnan(b)), (what, name)
        dev = np.abs(a - b) / np.maximum(1.0, np.abs(b))
        if np.isfinite(dev).any():
            worst = max(worst, float(np.nanmax(dev)))
    print("%s: worst deviation from rollout_np %.3g" % (what, worst))
    assert worst <= 1e-6, what


def _stepwise_policy(c, P, u_pass, start, K, u_prev0=None):
    """the yardstick: per realisation x0 uploaded, then K times (download x, apply_np, advancing sim_step(resolve=R, u0=u)); the arrays of a rollout"""
    p, B = c.p, c.B
    ref = dict(x=np.zeros((B, S, K + 1, c.nx)), v=np.zeros((B, S, K, c.nv)), y=np.zeros((B, S, K, c.d["ny"])), cons_vio=np.zeros((B, S, K)),
               cons_row=np.zeros((B, S, K), np.int32), aux_status=np.zeros((B, S, K), np.int32), switches=np.zeros((B, S), np.int32))
    for cc in range(S):
        p.upload(c.x0, c.om, c.midx)
        ref["x"][:, cc, 0] = c.x0
        up = P.initial_state(c.midx) if u_prev0 is None else u_prev0
        us = []
        for k in range(K):
            x = p.inputs()[0]
            u = policy.apply_np(P, c.midx, x, up if k == 0 else us[-1], u_pass[:, k])
            o = p.sim_step(resolve=c.R, u0=u, act_start=np.ascontiguousarray(start[:, cc]), step=STEP + k, advance=True, outputs=True, log=False)
            c.in_lds()
            assert o["n_skipped"] == 0
            ref["x"][:, cc, k + 1], ref["v"][:, cc, k], ref["y"][:, cc, k] = o["x_k1"], o["v0"], o["y"]
            ref["cons_vio"][:, cc, k], ref["cons_row"][:, cc, k], ref["aux_status"][:, cc, k] = o["cons_vio"], o["cons_row"], o["aux_status"]
            us.append(u)
        ref["switches"][:, cc] = policy.switches_np(P, c.midx, np.stack(us, axis=1), up)
    return ref


@pytest.mark.parametrize("mode", ["one", "long"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_against_the_stepwise_route(ctx, shape, mode):
    """K = 1 and K = N_tilde + 2, every channel ruled and no plan resident (u_seq=None attempts every instance).
    Measured on the device (MI355X), worst deviation over all shapes and modes: see DESIGN.md section 6."""
    c = ctx(shape)
    p = c.p
    K = dict(one=1, long=c.N + 2)[mode]
    lib, gw, start, om_seq, u_seq = _scenario(c, K, 9100 + 10 * list(SHAPES).index(shape) + K)
    P = thermostat(c)
    num = reference(c, P, c.x0, u_seq, om_seq)
    try:
        p.upload(c.x0, c.om, c.midx)
        p.upload_profiles(lib, gw)
        p.upload_policy(P)
        got = p.rollout(c.R, K=K, start=start, step=STEP, trajectories=True, policy=True)
        assert got["x"].shape == (c.B, S, K + 1, c.nx) and got["switches"].dtype == np.int32 and got["switches"].shape == (c.B, S)
        assert got["stats"] == dict(trajectories=c.B * S, complete=c.B * S, infeasible=0, declined=0, not_attempted=0, finished_on_host=0)
        ref = _stepwise_policy(c, P, u_seq, start, K)
        _against_stepwise(c, got, ref, K, "%s %s" % (shape, mode))                 # u and the binaries, cons_row, endings equal; x, y, z, mu, cons_vio 1e-6
        assert np.array_equal(got["switches"], ref["switches"]) and np.array_equal(got["switches"], num["switches"])
        if mode == "long":
            u = got["v"][..., :c.nu]
            first = np.concatenate([np.broadcast_to(P.initial_state(c.midx)[:, None, None, :], u[:, :, :1].shape), u[:, :, :-1]], axis=2)
            assert ((u == 1) & (first == 0)).any() and ((u == 0) & (first == 1)).any()      # a channel switches on and one off
    finally:
        p.upload_policy(None)
        p.upload_profiles(np.zeros(0))


@pytest.mark.parametrize("shape", list(SHAPES))
def test_each_step_is_the_models_and_the_rules(ctx, shape):
    """on the returned (x_k, v_k, omega_k): simlog.lsim_k_batch reproduces x_{k+1}, y, cons_vio and cons_row as tests/test_gpu_rollout.py compares them, and
    apply_np on the device's own x_k and u_{k-1} gives the device's u_k exactly (unit selectors: s is x_j itself)"""
    c = ctx(shape)
    p, B, nu, d = c.p, c.B, c.nu, c.d
    K = c.N + 2
    _, _, _, om_seq, u_seq = _scenario(c, K, 9200 + list(SHAPES).index(shape))
    P = thermostat(c, 59.5, 62.5)
    rng = np.random.default_rng(9210)
    u_prev = (rng.uniform(size=(B, nu)) < 0.5).astype(float)
    num = reference(c, P, c.x0, u_seq, om_seq, u_prev)
    try:
        p.upload(c.x0, c.om, c.midx)
        p.upload_policy(P)
        got = p.rollout(c.R, K=K, omega_seq=om_seq, trajectories=True, policy=True, u_prev=u_prev)
        _against_reference(c, got, num, shape)
    finally:
        p.upload_policy(None)
    T = B * S
    midx = np.repeat(c.midx, S)
    bound = simlog.sum_bound(d)
    flat = {k: got[k].reshape((T,) + got[k].shape[2:]) for k in TRAJ}
    om, at = om_seq.reshape(T, K, c.nw), np.arange(T)
    up = np.repeat(u_prev, S, axis=0)
    for k in range(K):
        x, v = flat["x"][:, k], flat["v"][:, k]
        assert np.array_equal(v[:, :nu], policy.apply_np(P, midx, x, up)), (shape, k)
        up = v[:, :nu]
        ref = simlog.lsim_k_batch(c.mats, d, midx, x, v, om[:, k])
        assert np.all(np.abs(flat["x"][:, k + 1] - ref["x_k1"]) <= bound * ref["terms_x"]), (shape, k)
        assert np.all(np.abs(flat["y"][:, k] - ref["y"]) <= bound * ref["terms_y"]), (shape, k)
        rows = flat["cons_row"][:, k]
        assert np.all((rows >= 0) & (rows < d["nc"])), (shape, k)
        assert np.all(ref["resid"][at, rows] >= ref["cons_vio"] - 2 * bound * ref["terms_r"].max(axis=1)), (shape, k)
        assert np.all(np.abs(flat["cons_vio"][:, k] - ref["resid"][at, rows]) <= bound * ref["terms_r"][at, rows]), (shape, k)


def test_ties_are_exact(ctx):
    """thresholds ON the integer grid: x0[b, j] exactly on_at, exactly off_at, strictly between, with u_prev on and off.  The step-0 u is the rule's:
    on at on_at whatever was, off at off_at whatever was, in between what was; and on_at == off_at == x: on."""
    c = ctx("a10")
    p, B, nu = c.p, c.B, c.nu
    _, _, _, om_seq, _ = _scenario(c, 1, 9300)
    P = thermostat(c, 58.0, 61.0)
    x0, u_prev, want = np.zeros((B, c.nx)), np.zeros((B, nu)), np.zeros((B, nu))
    cases = [(58.0, 0.0, 1.0), (58.0, 1.0, 1.0), (61.0, 1.0, 0.0), (61.0, 0.0, 0.0), (59.5, 1.0, 1.0), (59.5, 0.0, 0.0), (58.0 + 2.0 ** -40, 0.0, 0.0), (61.0 - 2.0 ** -40, 1.0, 1.0)]
    for b in range(B):
        for j in range(nu):
            x0[b, j], u_prev[b, j], want[b, j] = cases[(3 * b + j) % len(cases)]
    try:
        p.upload(x0, c.om, c.midx)
        p.upload_policy(P)
        got = p.rollout(c.R, K=1, omega_seq=om_seq, trajectories=True, policy=True, u_prev=u_prev)
        assert np.all(got["end_status"] == 0)
        assert np.array_equal(got["v"][:, :, 0, :nu], np.broadcast_to(want[:, None], (B, S, nu)))
        assert np.array_equal(got["switches"], np.broadcast_to((want != u_prev).sum(axis=1)[:, None], (B, S)))
        p.upload_policy(thermostat(c, 59.0, 59.0))
        xe = np.full((B, c.nx), 59.0)
        xe[:, 1:] += np.array([-1.0, 1.0])[None, :c.nx - 1]
        p.upload(xe, c.om, c.midx)
        got = p.rollout(c.R, K=1, omega_seq=om_seq, trajectories=True, policy=True, u_prev=np.zeros((B, nu)))
        assert np.array_equal(got["v"][:, :, 0, :3], np.broadcast_to(np.array([1.0, 1.0, 0.0]), (B, S, 3)))      # at, below, above the one threshold
    finally:
        p.upload_policy(None)


def test_mixed_modes(ctx):
    """channel 0 passed through: its values come from u_seq, then (u_seq=None) from the resident plan; the other channels are ruled"""
    c = ctx("a10")
    p, B, nu = c.p, c.B, c.nu
    K = c.N
    _, _, _, om_seq, u_seq = _scenario(c, K, 9400)
    P = thermostat(c, mode=[0] + [1] * (nu - 1))
    num = reference(c, P, c.x0, u_seq, om_seq)
    try:
        p.upload(c.x0, c.om, c.midx)
        p.upload_policy(P)
        got = p.rollout(c.R, u_seq=u_seq, omega_seq=om_seq, trajectories=True, policy=True)
        assert np.array_equal(got["v"][..., 0], np.broadcast_to(u_seq[:, None, :, 0], (B, S, K)))
        _against_reference(c, got, num, "from u_seq")
        with pytest.raises(gpu.MldGpuError, match="has not been solved"):
            p.rollout(c.R, omega_seq=om_seq, policy=True)                          # a passed-through channel needs the plan
        p.solve_resident()
        plan = p.download()
        assert np.all(np.isin(plan["status"], (0, 2)) & np.isfinite(plan["obj"]))
        u_plan = np.ascontiguousarray(plan["v"].reshape(B, c.N, c.nv)[:, :K, :nu])
        num = reference(c, P, c.x0, u_plan, om_seq)
        got = p.rollout(c.R, omega_seq=om_seq, trajectories=True, policy=True)
        assert np.array_equal(got["v"][..., 0], np.broadcast_to(u_plan[:, None, :, 0], (B, S, K)))
        _against_reference(c, got, num, "from the plan")
        with pytest.raises(gpu.MldGpuError, match="N_tilde = %d" % c.N):
            p.rollout(c.R, K=c.N + 1, omega_seq=np.zeros((B, S, c.N + 1, c.nw)), policy=True)
    finally:
        p.upload_policy(None)


@pytest.mark.parametrize("shape", ["a10", "b9"])
def test_a_selector_over_two_tanks(ctx, shape):
    """channel j switches on the mean of tanks j and j + 1 (cyclic): s is a sum of two products, inside the guard"""
    c = ctx(shape)
    p, nx = c.p, c.nx
    K = c.N + 2
    _, _, _, om_seq, u_seq = _scenario(c, K, 9500 + list(SHAPES).index(shape))
    sel = 0.5 * (np.eye(nx) + np.roll(np.eye(nx), 1, axis=1))
    P = policy.ThresholdPolicy(np.broadcast_to(sel, (len(c.mats), nx, nx)), 58.25 + 1.0 / 64, 60.75 + 1.0 / 64)
    num = reference(c, P, c.x0, u_seq, om_seq)
    assert num["switches"].max() > 0
    try:
        p.upload(c.x0, c.om, c.midx)
        p.upload_policy(P)
        got = p.rollout(c.R, K=K, omega_seq=om_seq, trajectories=True, policy=True)
        _against_reference(c, got, num, shape)
    finally:
        p.upload_policy(None)


def test_u_prev_against_the_resident_state(ctx):
    c = ctx("a10")
    p, B, nu = c.p, c.B, c.nu
    K = c.N + 1
    _, _, _, om_seq, _ = _scenario(c, K, 9600)
    P = thermostat(c)
    on = np.ones((B, nu))
    try:
        p.upload(c.x0, c.om, c.midx)
        p.upload_policy(P)
        assert np.array_equal(p.policy_state(), np.zeros((B, nu)))                    # after upload(): every ruled channel at u_off
        reset = p.rollout(c.R, K=K, omega_seq=om_seq, trajectories=True, policy=True)
        given = p.rollout(c.R, K=K, omega_seq=om_seq, trajectories=True, policy=True, u_prev=on)
        assert np.array_equal(p.policy_state(), np.zeros((B, nu)))                    # u_prev= is the call's own
        assert not np.array_equal(given["v"][:, :, 0, :nu], reset["v"][:, :, 0, :nu])      # tanks inside the band hold what they had
        assert np.array_equal(p.policy_state(u_prev=on), on)
        resident = p.rollout(c.R, K=K, omega_seq=om_seq, trajectories=True, policy=True)
        _same(resident, given, TRAJ + SUMM, "resident against given")
        assert np.array_equal(p.policy_state(), on)
        zeros = p.rollout(c.R, K=K, omega_seq=om_seq, trajectories=True, policy=True, u_prev=np.zeros(nu))
        _same(zeros, reset, TRAJ + SUMM, "given zeros against the reset state")
        assert np.array_equal(p.policy_state(reset=True), np.zeros((B, nu)))
    finally:
        p.upload_policy(None)


@pytest.mark.parametrize("shape", list(SHAPES))
def test_determinism_and_position_independence(ctx, shape):
    c = ctx(shape)
    p = c.p
    K = c.N + 1
    _, _, _, om_seq, _ = _scenario(c, K, 9700 + list(SHAPES).index(shape))
    rng = np.random.default_rng(9710)
    u_prev = (rng.uniform(size=(c.B, c.nu)) < 0.5).astype(float)
    try:
        p.upload(c.x0, c.om, c.midx)
        p.upload_policy(thermostat(c))
        one = p.rollout(c.R, K=K, omega_seq=om_seq, trajectories=True, policy=True, u_prev=u_prev)
        two = p.rollout(c.R, K=K, omega_seq=om_seq, trajectories=True, policy=True, u_prev=u_prev)
        _same(one, two, TRAJ + SUMM, shape + " twice")
        p.upload(c.x0[::-1], c.om[::-1], np.ascontiguousarray(c.midx[::-1]))
        rev = p.rollout(c.R, K=K, omega_seq=om_seq[::-1], trajectories=True, policy=True, u_prev=u_prev[::-1])
        _same({k: v[::-1] for k, v in rev.items() if k != "stats"}, one, TRAJ + SUMM, shape + " reversed")
        lean = p.rollout(c.R, K=K, omega_seq=om_seq[::-1], policy=True, u_prev=u_prev[::-1])
        assert sorted(lean) == sorted(SUMM + ("stats",))
        _same(lean, rev, SUMM, shape + " summaries only")
    finally:
        p.upload_policy(None)


def test_an_infeasible_ending(ctx):
    """the hard 3-tank model: a tank above T_max leaves the auxiliary problem of step 0 without a feasible point -- switches -1, NaN from that step on"""
    c = ctx("a10", hard=True)
    p, B, K = c.p, c.B, 3
    assert c.d["nmu"] == 0
    _, _, _, om_seq, u_seq = _scenario(c, K, 9800)
    hot = np.arange(B) % 3 == 1
    x0 = c.x0.copy()
    x0[hot, 0] = 90.0
    P = thermostat(c)
    num = reference(c, P, x0, u_seq, om_seq)
    dead = num["end_status"][:, 0] == 1                                              # (the realisations differ in the load only: a tank's fate is the instance's)
    assert np.all(num["end_status"][hot] == 1) and np.all(num["steps_done"][hot] == 0) and (~dead).sum() >= 3
    assert np.all((num["end_status"] == 1) == dead[:, None]) and (num["steps_done"][dead & ~hot] > 0).all()      # a heated tank may pass T_max later on
    hot = dead
    try:
        p.upload(x0, c.om, c.midx)
        p.upload_policy(P)
        got = p.rollout(c.R, K=K, omega_seq=om_seq, trajectories=True, policy=True)
    finally:
        p.upload_policy(None)
    n1 = int(hot.sum()) * S
    assert got["stats"] == dict(trajectories=B * S, complete=B * S - n1, infeasible=n1, declined=0, not_attempted=0, finished_on_host=0)
    assert np.all(got["switches"][hot] == -1) and np.all(got["switches"][~hot] >= 0)
    _against_reference(c, got, num, "hard")                                         # (endings and steps_done equal)
    for b in range(B):
        for cc in range(S):
            sd = got["steps_done"][b, cc]
            assert np.all(np.isfinite(got["x"][b, cc, :sd + 1])) and np.all(np.isnan(got["x"][b, cc, sd + 1:]))
            for k in ("v", "y", "cons_vio"):
                assert np.all(np.isfinite(got[k][b, cc, :sd])) and np.all(np.isnan(got[k][b, cc, sd:])), k
            assert np.all(got["cons_row"][b, cc, :sd] >= 0) and np.all(got["cons_row"][b, cc, sd:] == -1)
    for k in ("cost", "mu_total", "worst_vio"):
        assert np.all(np.isnan(got[k][hot])) and np.all(np.isfinite(got[k][~hot])), k
    assert np.all(got["worst_step"][hot] == -1)


def test_host_completion(ctx):
    """MLD_DBG_SMALL_PIVOT_CAP: every trajectory ends 2 at step 0 on the device and is finished on the host, with the rule applied there"""
    c = ctx("a10")
    p, B = c.p, c.B
    K = c.N + 1
    _, _, _, om_seq, u_seq = _scenario(c, K, 9900)
    P = thermostat(c)
    rng = np.random.default_rng(9910)
    u_prev = (rng.uniform(size=(B, c.nu)) < 0.5).astype(float)
    num = reference(c, P, c.x0, u_seq, om_seq, u_prev)
    try:
        p.upload(c.x0, c.om, c.midx)
        p.upload_policy(P)
        want = p.rollout(c.R, K=K, omega_seq=om_seq, trajectories=True, policy=True, u_prev=u_prev)
        assert want["stats"]["declined"] == 0
        c.R.problem.set_opts(reserved=_lib.MLD_DBG_SMALL_PIVOT_CAP)
        try:
            es, sw, stats = np.zeros((B, S), np.int32), np.zeros((B, S), np.int32), np.zeros(4, np.int64)
            ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
            rc = _lib.load().mld_rollout_policy(p._h, c.R.problem._h, K, S, None, _lib.dptr(u_prev), _lib.dptr(om_seq), None, 0, None, 0, None, None, None, None, None,
                                                None, None, None, None, None, ip(es), ip(sw), stats.ctypes.data_as(C.POINTER(C.c_int64)))
            assert rc == 0 and np.all(es == 2) and np.all(sw == -1) and list(stats) == [B * S, 0, 0, B * S]
            got = p.rollout(c.R, K=K, omega_seq=om_seq, trajectories=True, policy=True, u_prev=u_prev)
            assert got["stats"] == dict(trajectories=B * S, complete=B * S, infeasible=0, declined=B * S, not_attempted=0, finished_on_host=B * S)
            _against_reference(c, got, num, "finished on the host")
            _against_reference(c, got, want, "host against device")
            lean = p.rollout(c.R, K=K, omega_seq=om_seq, policy=True, u_prev=u_prev)
            assert sorted(lean) == sorted(SUMM + ("stats",)) and lean["stats"]["finished_on_host"] == B * S
            _same(lean, got, SUMM, "summaries only")
        finally:
            c.R.problem.set_opts(reserved=0)
    finally:
        p.upload_policy(None)


def test_the_handle_is_untouched(ctx):
    c = ctx("a10")
    p, B = c.p, c.B
    K = c.N
    lib, gw, start, om_seq, u_seq = _scenario(c, K, 9950)
    on = np.ones((B, c.nu))
    try:
        p.upload(c.x0, c.om, c.midx)
        p.upload_profiles(lib, gw)
        p.upload_policy(thermostat(c, mode=[1] * (c.nu - 1) + [0]))
        p.policy_state(u_prev=on)
        p.sim_log_begin(2)
        p.solve_resident()
        before = (p.inputs(), p.download(), p.sim_log_count())
        for kw in (dict(start=start, step=STEP), dict(omega_seq=om_seq, u_seq=u_seq, u_prev=np.zeros((B, c.nu))), dict(start=start, step=STEP, trajectories=True)):
            p.rollout(c.R, policy=True, **kw)
            x_in, w_in = p.inputs()
            assert np.array_equal(x_in, before[0][0]) and np.array_equal(w_in, before[0][1]) and p.sim_log_count() == before[2]
            after = p.download()
            for k in after:
                assert np.array_equal(after[k], before[1][k], equal_nan=True), k
            assert np.array_equal(p.policy_state(), on)
        p.solve_resident()
        again = p.download()
        for k in ("v", "obj", "status", "lower_bound", "nodes", "pivots"):
            assert np.array_equal(again[k], before[1][k], equal_nan=True), k
    finally:
        p.sim_log_begin(0)
        p.upload_policy(None)
        p.upload_profiles(np.zeros(0))


def test_refusals_change_nothing(ctx):
    c, big = ctx("a10"), ctx("b9")
    p, B, nu = c.p, c.B, c.nu
    K = c.N
    lib, gw, start, om_seq, u_seq = _scenario(c, K, 9960)
    plain = BatchAuxResolver(c.mats, c.d)                                   # not flagged: the dense path's resolver
    P = thermostat(c)
    lib_ = _lib.load()
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    try:
        p.upload(c.x0, c.om, c.midx)
        p.upload_profiles(lib, gw)
        p.solve_resident()
        state = (p.inputs(), p.download())
        with pytest.raises(gpu.MldGpuError, match="no policy uploaded"):
            p.rollout(c.R, start=start, step=STEP, policy=True)
        for call in (p.policy_state, lambda: p.policy_state(reset=True), lambda: p.policy_state(u_prev=np.zeros((B, nu)))):
            with pytest.raises(gpu.MldGpuError, match="no policy uploaded"):
                call()
        # the tables are validated on the host like the constructor's; a refused upload leaves the resident policy
        p.upload_policy(P)
        good = p.rollout(c.R, start=start, step=STEP, policy=True)
        col = lambda v: np.full((len(c.mats), nu), float(v))
        mode = np.ones((len(c.mats), nu), np.int32)
        for sel, on_at, off_at, u_on, u_off, md, word in (
                (np.where(np.arange(P.sel.size).reshape(P.sel.shape) == 4, np.nan, P.sel), col(58), col(61), col(1), col(0), mode, b"sel of model 0, channel 1, state 1 is not finite"),
                (P.sel, col(np.inf), col(61), col(1), col(0), mode, b"on_at of model 0, channel 0 is not finite"),
                (P.sel, col(58), col(np.nan), col(1), col(0), mode, b"off_at of model 0, channel 0 is not finite"),
                (P.sel, col(58), col(61), col(-np.inf), col(0), mode, b"u_on of model 0, channel 0 is not finite"),
                (P.sel, col(58), col(61), col(1), col(np.nan), mode, b"u_off of model 0, channel 0 is not finite"),
                (P.sel, col(62), col(61), col(1), col(0), mode, b"on_at > off_at for model 0, channel 0"),
                (P.sel, col(58), col(61), col(1), col(0), mode * 2, b"mode of model 0, channel 0 is 2"),
                (P.sel, None, col(61), col(1), col(0), mode, b"is NULL")):
            sel = np.ascontiguousarray(sel)
            assert lib_.mld_upload_policy(p._h, _lib.dptr(sel), _lib.dptr(on_at), _lib.dptr(off_at), _lib.dptr(u_on), _lib.dptr(u_off), ip(np.ascontiguousarray(md))) == -1
            assert word in lib_.mld_last_error(), word
        with pytest.raises(ValueError, match="the policy is shaped"):
            p.upload_policy(thermostat(big))

        def refused(match, resolve=c.R, exc=gpu.MldGpuError, **kw):
            with pytest.raises(exc, match=match):
                p.rollout(resolve, policy=True, **kw)
            x_in, w_in = p.inputs()
            assert np.array_equal(x_in, state[0][0]) and np.array_equal(w_in, state[0][1]), match
            now = p.download()
            for k in now:
                assert np.array_equal(now[k], state[1][k], equal_nan=True), (match, k)
            assert np.array_equal(p.policy_state(), np.zeros((B, nu))), match

        bad = np.zeros((B, nu))
        bad[6, 2] = np.nan
        refused("u_prev of instance 6, input 2 is not finite", start=start, step=STEP, u_prev=bad)
        bad[6, 2] = np.inf
        refused("not finite", omega_seq=om_seq, u_prev=bad)
        with pytest.raises(gpu.MldGpuError, match="u_prev of instance 6, input 2 is not finite"):
            p.policy_state(u_prev=bad)
        with pytest.raises(ValueError, match="u_prev given without policy"):
            p.rollout(c.R, start=start, step=STEP, u_prev=np.zeros((B, nu)))
        # everything mld_rollout_batch refuses
        refused("not on the small-problem path.*mld_sim_step_resolve", resolve=plain, start=start, step=STEP)
        refused("not the fold", resolve=big.R, start=start, step=STEP)
        refused("exactly one of omega_seq and start", exc=ValueError, omega_seq=om_seq, start=start)
        refused("exactly one of omega_seq and start", exc=ValueError)
        refused("K = 0", K=0, omega_seq=np.zeros((B, S, 0, c.nw)))
        out = start.copy()
        out[B - 1, S - 1, 1] = lib.size - (STEP + K) * (c.nw - 1) + 1      # one double past the last valid start
        refused("leaves the library", start=out, step=STEP)
        nan_u = u_seq.copy()
        nan_u[6, 1, 2] = np.nan                                            # a ruled channel of u_seq is ignored but must be finite
        refused("u_seq of instance 6, step 1, input 2 is not finite", u_seq=nan_u, start=start, step=STEP)
        nan_w = om_seq.copy()
        nan_w[0, 0, 0, 0] = np.nan
        refused("omega_seq of trajectory 0, step 0, channel 0 is not finite", omega_seq=nan_w)
        refused("cost_w has shape", exc=ValueError, start=start, step=STEP, cost_w=np.zeros((B + 1, K, c.nv)))
        again = p.rollout(c.R, start=start, step=STEP, policy=True)             # ... and one good call afterwards still works
        _same(again, good, SUMM, "after the refusals")
        assert again["stats"] == good["stats"] and again["stats"]["complete"] == B * S
        p.upload_policy(None)
        with pytest.raises(gpu.MldGpuError, match="no policy uploaded"):
            p.rollout(c.R, start=start, step=STEP, policy=True)
    finally:
        plain.close()
        p.upload_policy(None)
        p.upload_profiles(np.zeros(0))


@pytest.mark.parametrize("shape", ["a10", "b9"])
def test_open_loop_rollout_beside_a_resident_policy(ctx, shape):
    """rollout() without `policy` takes the path it always took, whatever is resident: against tests/test_gpu_rollout.py's own stepwise yardstick, and
    bit for bit the same with and without a policy on the handle"""
    c = ctx(shape)
    p = c.p
    K = c.N + 2
    lib, gw, start, om_seq, u_seq = _scenario(c, K, 9100 + 10 * list(SHAPES).index(shape) + K)
    assert np.all(np.abs(_rollout_ref.closed_y(c.mats, c.d, c.midx, u_seq, om_seq)) >= 1e-3)
    try:
        p.upload(c.x0, c.om, c.midx)
        p.upload_profiles(lib, gw)
        without = p.rollout(c.R, u_seq=u_seq, start=start, step=STEP, trajectories=True)
        p.upload_policy(thermostat(c))
        got = p.rollout(c.R, u_seq=u_seq, start=start, step=STEP, trajectories=True)
        assert "switches" not in got
        _same(got, without, TRAJ + SUMM[:-1], shape)
        assert got["stats"] == without["stats"]
        ref = _stepwise(c, u_seq, start, K)
        _against_stepwise(c, got, ref, K, shape)
    finally:
        p.upload_policy(None)
        p.upload_profiles(np.zeros(0))
