"""MIP start from a baseline rollout on the device (mld_warm_start_from_rollout / GpuProblem.warm_start_from_rollout, kernels k_rollout[_policy] and
k_warm_from_rollout): the start for the instances warm_start_from_previous leaves without one -- the reference's warm_start=True (controllers/
controller_base.py:493,509-512) fed from the thermostat baseline its campaign quotes every MPC variant against.  Checked: the bytes against the host route
(the device's own rollout under the resident forecast, simlog.start_from_rollout_np) and the binaries against simlog.rollout_np; the solve takes the device
start exactly as it takes the uploaded bytes; with it no instance ends worse than the baseline; the keep rule behind warm_start_from_previous; the endings;
the untouched handle, determinism, position independence and every refusal.

The guards are those of tests/test_gpu_policy_rollout.py (conditions on the numpy reference, not tolerances): every selector value at least 1e-4 away from
both thresholds, |y| at least 1e-3 (no instance on the switching surface of delta).  They exclude no instance.

Shapes (tests/test_gpu_sim_resolve.py): a10 -- n_h 3, three models interleaved, N_tilde 3, batch 10; a1 -- batch 1; b9 -- n_h 7, N_tilde 2, batch 9.  The policy
is the thermostat at 57.5 / 60.5."""
import ctypes as C

import numpy as np
import pytest

import _rollout_ref
from test_gpu_sim_resolve import SHAPES
from test_gpu_small_lds_step import _SmallCtx
from test_gpu_policy_rollout import GUARD, thermostat
from pyhybridcontrol_amd import gpu, policy, simlog, _lib
from pyhybridcontrol_amd.aux_resolve import BatchAuxResolver

pytestmark = pytest.mark.gpu

_CACHE = {}
CUT = -1e30
RESULT = ("v", "obj", "status", "lower_bound", "nodes", "pivots")


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


def _bins(p):
    return np.flatnonzero(p.is_bin)


def _host_route(c, forecast, old=None, **kw):
    """the route the library had: the device's own rollout under the forecast with trajectories downloaded, the byte rule on the host"""
    ro = c.p.rollout(c.R, omega_seq=forecast.reshape(c.B, 1, c.N, c.nw), trajectories=True, **kw)
    assert ro["stats"]["finished_on_host"] == 0
    start, source = simlog.start_from_rollout_np(ro["v"], ro["end_status"], _bins(c.p), old=old)
    return ro, start, source


def _reference(c, x0, forecast, P=None, u_seq=None, u_prev=None):
    """simlog.rollout_np with the closed form as resolver under the forecast, after the guards of tests/test_gpu_policy_rollout.py; prints the margins"""
    B, K = c.B, c.N
    om_seq = forecast.reshape(B, 1, K, c.nw)
    u = np.zeros((B, K, c.nu)) if u_seq is None else u_seq
    ref = simlog.rollout_np(c.mats, c.d, c.midx, x0, u, om_seq, _rollout_ref.closed_form_resolver(c.mats, c.d), policy=P, u_prev=u_prev)
    live = np.arange(K)[None, None, :] < ref["steps_done"][:, :, None]
    if P is not None:
        s = np.stack([policy.selector_values(P, c.midx, ref["x"][:, 0, k]) for k in range(K)], axis=1).reshape(B, 1, K, c.nu)
        margin = np.minimum(np.abs(s - P.on_at[c.midx][:, None, None, :]), np.abs(s - P.off_at[c.midx][:, None, None, :]))[np.broadcast_to(live[..., None], s.shape)]
        print("selector margin to the thresholds: %.3g over %d values" % (margin.min(), margin.size))
        assert margin.min() >= GUARD
    D1 = np.stack([np.asarray(m["D1"], float).reshape(-1) for m in c.mats])[c.midx]
    y = np.einsum("bskj,bj->bsk", np.where(live[..., None], ref["v"][..., :c.nu], 0.0), D1) + om_seq[..., c.nx]
    print("|y| at least %.3g" % np.abs(y[live]).min())
    assert np.all(np.abs(y[live]) >= 1e-3)
    return ref


@pytest.mark.parametrize("shape", list(SHAPES))
def test_bytes_equal_the_host_route(ctx, shape):
    """policy=True and policy=False (a random 0/1 u_seq): every byte equals the host route's, source 1 everywhere, and the binaries equal rollout_np's"""
    c = ctx(shape)
    p, B, N, nb = c.p, c.B, c.N, c.p.n_bin
    P = thermostat(c)
    rng = np.random.default_rng(9100 + list(SHAPES).index(shape))
    u_seq = (rng.uniform(size=(B, N, c.nu)) < 0.4).astype(float)
    try:
        p.upload(c.x0, c.om, c.midx)
        p.upload_policy(P)
        assert p.debug_warm_start() is None and nb > 0
        forecast = p.inputs()[1]
        for what, kw, num in (("policy", dict(policy=True), _reference(c, c.x0, forecast, P=P)), ("u_seq", dict(u_seq=u_seq), _reference(c, c.x0, forecast, u_seq=u_seq))):
            got = p.warm_start_from_rollout(c.R, **kw)
            start = p.debug_warm_start()
            ro, want, source = _host_route(c, forecast, **kw)
            assert start is not None and start.shape == (B, nb) and np.array_equal(start, want), (shape, what)
            assert got["source"].dtype == np.int32 and np.array_equal(got["source"], source) and np.all(got["source"] == 1), (shape, what)
            assert got["stats"] == dict(trajectories=B, written=B, kept=0, none=0), (shape, what)
            assert np.all(num["end_status"] == 0), (shape, what)
            ref_start, _ = simlog.start_from_rollout_np(num["v"], num["end_status"], _bins(p))
            assert np.array_equal(start, ref_start), (shape, what)
            assert np.array_equal(start, np.rint(ro["v"].reshape(B, -1)[:, _bins(p)]).astype(np.uint8)), (shape, what)      # the binaries ARE 0 / 1
    finally:
        p.upload_policy(None)


@pytest.mark.parametrize("shape", list(SHAPES))
def test_the_solve_takes_the_device_start_as_it_takes_the_uploaded_bytes(ctx, shape):
    c = ctx(shape)
    p = c.p
    try:
        p.upload(c.x0, c.om, c.midx)
        p.upload_policy(thermostat(c))
        p.warm_start_from_rollout(c.R, policy=True)
        start = p.debug_warm_start()
        p.solve_resident()
        a = p.download()
        p.upload(c.x0, c.om, c.midx)
        assert p.debug_warm_start() is None
        p.set_warm_start(start)
        p.solve_resident()
        b = p.download()
        for k in RESULT:
            assert np.array_equal(a[k], b[k], equal_nan=True), (shape, k)
    finally:
        p.upload_policy(None)


@pytest.mark.parametrize("shape", list(SHAPES))
def test_never_worse_than_the_baseline(ctx, shape):
    """the baseline plan is feasible for the MPC's rows without slack (asserted first, for every instance); evaluated first, as any start is on a
    problem with a linear cost (the eager rule of mld_set_warm_start), it bounds every instance's objective: obj <= A + 1e-6 max(1, |A|), the project's
    objective contract.
    Measured on the device (MI355X): the baseline's worst residual on the original rows is 9.2e-10 (a10), 9.1e-10 (a1), 9.2e-10 (b9), no integrality or
    bound violation; every instance ends OPTIMAL; the worst obj - A is 0 (a10, b9: an instance whose optimum within the gap IS the baseline) and -1.94 (a1)."""
    c = ctx(shape)
    p, B = c.p, c.B
    try:
        p.upload(c.x0, c.om, c.midx)
        p.upload_policy(thermostat(c))
        forecast = p.inputs()[1]
        ro, _, _ = _host_route(c, forecast, policy=True)
        base = p.evaluate(ro["v"].reshape(B, -1))
        print("%s baseline: constr_vio %.3g int_vio %.3g bound_vio %.3g" % (shape, base["constr_vio"].max(), base["int_vio"].max(), base["bound_vio"].max()))
        assert np.all(base["constr_vio"] <= 1e-9) and np.all(base["int_vio"] == 0) and np.all(base["bound_vio"] == 0)
        assert np.all(p.warm_start_from_rollout(c.R, policy=True)["source"] == 1)
        p.solve_resident()
        out = p.download()
        A = base["obj"]
        print("%s worst obj - baseline: %.3g; statuses %s" % (shape, (out["obj"] - A).max(), np.bincount(out["status"], minlength=3).tolist()))
        assert np.all(np.isin(out["status"], (0, 2))), out["status"]
        assert np.all(out["obj"] <= A + 1e-6 * np.maximum(1.0, np.abs(A))), (out["obj"] - A)
    finally:
        p.upload_policy(None)


@pytest.mark.parametrize("shape", ["a10", "b9"])
def test_keep_behind_warm_start_from_previous(ctx, shape):
    """some instances cut off (an unbeatable cutoff, as tests/test_gpu_fallback_step.py), a solve, an advancing fallback step, warm_start_from_previous(1):
    their rows are 255.  keep=True fills exactly those from the rollout and leaves the others byte for byte; without keep every row is the rollout's"""
    c = ctx(shape)
    p, B = c.p, c.B
    chosen = [1, 4, B - 1]
    try:
        p.upload(c.x0, c.om, c.midx)
        p.upload_policy(thermostat(c))
        cut = np.full(B, np.inf)
        cut[chosen] = CUT
        p.set_cutoffs(cut)
        p.solve_resident()
        plan = p.download()
        usable = np.isin(plan["status"], (0, 2)) & np.isfinite(plan["obj"])
        assert np.array_equal(np.flatnonzero(~usable), np.array(chosen))
        step = p.sim_step(resolve=c.R, fallback=("policy",), outputs=True)
        assert step["n_skipped"] == 0 and np.array_equal(step["u_source"], np.where(usable, 0, 2))
        p.warm_start_from_previous(1)
        prev = p.debug_warm_start()
        assert np.all(prev[~usable] == 255) and np.all(prev[usable] <= 1)
        forecast = p.inputs()[1]
        _, want_keep, src_keep = _host_route(c, forecast, old=prev, policy=True)
        _, want_all, src_all = _host_route(c, forecast, policy=True)
        assert np.all(src_all == 1)
        got = p.warm_start_from_rollout(c.R, policy=True, keep=True)
        start = p.debug_warm_start()
        assert np.array_equal(got["source"], np.where(usable, 0, 1)) and np.array_equal(got["source"], src_keep)
        assert got["stats"] == dict(trajectories=B, written=len(chosen), kept=B - len(chosen), none=0)
        assert np.array_equal(start[usable], prev[usable]) and np.array_equal(start[~usable], want_all[~usable]) and np.array_equal(start, want_keep)
        again = p.warm_start_from_rollout(c.R, policy=True, keep=True)      # every row has a start now: all kept
        assert np.all(again["source"] == 0) and np.array_equal(p.debug_warm_start(), start)
        got = p.warm_start_from_rollout(c.R, policy=True)
        assert np.all(got["source"] == 1) and np.array_equal(p.debug_warm_start(), want_all)
        # keep with no start resident: the same as without keep
        p.upload(c.x0, c.om, c.midx)
        assert p.debug_warm_start() is None
        fresh = p.warm_start_from_rollout(c.R, policy=True, keep=True)
        kept_none = p.debug_warm_start()
        plain = p.warm_start_from_rollout(c.R, policy=True)
        assert np.all(fresh["source"] == 1) and fresh["stats"] == plain["stats"] and np.array_equal(kept_none, p.debug_warm_start())
    finally:
        p.upload_policy(None)


def test_an_infeasible_ending(ctx):
    """the hard 3-tank model: a tank above T_max leaves an auxiliary problem without a feasible point -- that row is 255, its source -1, the others are the
    rollout's"""
    c = ctx("a10", hard=True)
    p, B = c.p, c.B
    assert c.d["nmu"] == 0
    hot = np.arange(B) % 3 == 1
    x0 = c.x0.copy()
    x0[hot, 0] = 90.0
    P = thermostat(c)
    try:
        p.upload(x0, c.om, c.midx)
        p.upload_policy(P)
        forecast = p.inputs()[1]
        num = _reference(c, x0, forecast, P=P)
        dead = num["end_status"][:, 0] == 1
        assert np.all(dead[hot]) and (~dead).sum() >= 3
        got = p.warm_start_from_rollout(c.R, policy=True)
        start = p.debug_warm_start()
        _, want, source = _host_route(c, forecast, policy=True)
        assert np.array_equal(got["source"], np.where(dead, -1, 1)) and np.array_equal(got["source"], source)
        assert got["stats"] == dict(trajectories=B, written=int((~dead).sum()), kept=0, none=int(dead.sum()))
        assert np.all(start[dead] == 255) and np.all(start[~dead] <= 1) and np.array_equal(start, want)
        ref_start, _ = simlog.start_from_rollout_np(num["v"], num["end_status"], _bins(p))
        assert np.array_equal(start, ref_start)
    finally:
        p.upload_policy(None)


def test_a_declined_rollout_is_no_start(ctx):
    """MLD_DBG_SMALL_PIVOT_CAP on the resolver: every trajectory ends declined (this entry has no host completion): source -2, every row 255, a start is
    set all the same, and the solve equals the solve without a start bit for bit"""
    c = ctx("a10")
    p, B = c.p, c.B
    try:
        p.upload(c.x0, c.om, c.midx)
        p.upload_policy(thermostat(c))
        c.R.problem.set_opts(reserved=_lib.MLD_DBG_SMALL_PIVOT_CAP)
        try:
            got = p.warm_start_from_rollout(c.R, policy=True)
        finally:
            c.R.problem.set_opts(reserved=0)
        start = p.debug_warm_start()
        assert np.all(got["source"] == -2) and got["stats"] == dict(trajectories=B, written=0, kept=0, none=B)
        assert start is not None and np.all(start == 255)
        p.solve_resident()
        a = p.download()
        p.upload(c.x0, c.om, c.midx)
        assert p.debug_warm_start() is None
        p.solve_resident()
        b = p.download()
        for k in RESULT:
            assert np.array_equal(a[k], b[k], equal_nan=True), k
    finally:
        p.upload_policy(None)


def _snapshot(p):
    blocks = p.constraint_blocks()
    return dict(inputs=p.inputs(), plan=p.download(), policy=p.policy_state(), memory=p.plan_memory_state(), blocks=blocks, log=p.sim_log_count())


def _unchanged(p, before, what):
    now = _snapshot(p)
    for a, b in zip(now["inputs"], before["inputs"]):
        assert np.array_equal(a, b), what
    for k in now["plan"]:
        assert np.array_equal(now["plan"][k], before["plan"][k], equal_nan=True), (what, k)
    assert np.array_equal(now["policy"], before["policy"]), what
    for k in ("u", "age"):
        assert np.array_equal(now["memory"][k], before["memory"][k]), (what, k)
    assert np.array_equal(now["blocks"]["omega_cols"], before["blocks"]["omega_cols"]) and np.array_equal(now["blocks"]["col_rows"], before["blocks"]["col_rows"]), what
    assert now["log"] == before["log"], what


def test_the_handle_is_untouched(ctx):
    c = ctx("a10")
    p, B, nu = c.p, c.B, c.nu
    on = np.ones((B, nu))
    rng = np.random.default_rng(9400)
    u_seq = (rng.uniform(size=(B, c.N, nu)) < 0.4).astype(float)
    try:
        p.upload(c.x0, c.om, c.midx)
        p.upload_policy(thermostat(c))
        p.policy_state(u_prev=on)
        p.plan_memory()
        p.sim_log_begin(2)
        p.upload_constraint_blocks(np.ascontiguousarray(np.stack([c.om * 1.01, c.om * 0.99], axis=1)))
        p.solve_resident()
        before = _snapshot(p)
        assert before["blocks"]["omega_cols"].shape[1] == 2
        starts = []
        for kw in (dict(policy=True), dict(policy=True), dict(policy=True, u_prev=np.zeros(nu)), dict(u_seq=u_seq), dict(policy=True, keep=True)):
            got = p.warm_start_from_rollout(c.R, **kw)
            _unchanged(p, before, kw)
            starts.append(p.debug_warm_start())
            assert got["stats"]["trajectories"] == B
        assert np.array_equal(starts[0], starts[1])                             # a second call gives the same bytes
        assert not np.array_equal(starts[0], starts[2])                         # u_prev= is the call's own: tanks inside the band hold what they had
        assert np.array_equal(starts[4], starts[3])                             # keep: every row had a start
        p.solve_resident()                                                      # the solve reads the start; nothing else has moved
        _unchanged(p, dict(before, plan=p.download()), "after the solve")
    finally:
        p.sim_log_begin(0)
        p.plan_memory(False)
        p.upload_policy(None)


@pytest.mark.parametrize("shape", ["a10", "b9"])
def test_position_independence(ctx, shape):
    c = ctx(shape)
    p = c.p
    try:
        p.upload(c.x0, c.om, c.midx)
        p.upload_policy(thermostat(c))
        one = p.warm_start_from_rollout(c.R, policy=True)
        fwd = p.debug_warm_start()
        p.upload(c.x0[::-1], c.om[::-1], np.ascontiguousarray(c.midx[::-1]))
        two = p.warm_start_from_rollout(c.R, policy=True)
        assert np.array_equal(p.debug_warm_start()[::-1], fwd) and np.array_equal(two["source"][::-1], one["source"])
    finally:
        p.upload_policy(None)


def test_refusals_leave_the_resident_start(ctx):
    c, big = ctx("a10"), ctx("b9")
    p, B, nu = c.p, c.B, c.nu
    rng = np.random.default_rng(9500)
    u_seq = (rng.uniform(size=(B, c.N, nu)) < 0.4).astype(float)
    plain = BatchAuxResolver(c.mats, c.d)                                       # not flagged: the dense path's resolver
    tv_model = gpu.GpuModel([[m] * c.N for m in c.mats], c.d, time_varying=True)
    tv = gpu.GpuProblem(tv_model, c.N - 1, c.N, None)
    lib = _lib.load()
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    lp = lambda a: a.ctypes.data_as(C.POINTER(C.c_int64))
    try:
        p.upload(c.x0, c.om, c.midx)
        mark = (np.arange(B * p.n_bin).reshape(B, p.n_bin) % 2).astype(np.uint8)
        mark[3] = 255
        p.set_warm_start(mark)

        def refused(match, resolve=c.R, exc=gpu.MldGpuError, **kw):
            with pytest.raises(exc, match=match):
                p.warm_start_from_rollout(resolve, **kw)
            assert np.array_equal(p.debug_warm_start(), mark), match

        def refused_c(match, policy_, u, up, flags):
            src, stats = np.full(B, 7, np.int32), np.full(4, 7, np.int64)
            rc = lib.mld_warm_start_from_rollout(p._h, c.R.problem._h, policy_, _lib.dptr(u), _lib.dptr(up), flags, ip(src), lp(stats))
            assert rc == -1 and match in lib.mld_last_error(), (match, lib.mld_last_error())
            assert np.all(src == 7) and np.all(stats == 7) and np.array_equal(p.debug_warm_start(), mark), match

        refused("no policy uploaded", policy=True)
        p.upload_policy(thermostat(c))
        with pytest.raises(ValueError, match="the policy is shaped"):
            p.upload_policy(thermostat(big))
        # the entry's own
        refused("policy = 0 needs u_seq")
        refused("u_prev given without policy", exc=ValueError, u_seq=u_seq, u_prev=np.zeros((B, nu)))
        refused_c(b"u_prev given with policy = 0", 0, u_seq, np.zeros((B, nu)), 0)
        refused_c(b"unknown flag bits 0x2", 1, None, None, 3)
        refused_c(b"policy = 2", 2, None, None, 0)
        # everything the rollouts refuse
        refused("not on the small-problem path.*mld_sim_step_resolve", resolve=plain, policy=True)
        refused("not the fold", resolve=big.R, policy=True)
        refused("aux == NULL", resolve=None, policy=True)
        bad = u_seq.copy()
        bad[6, 1, 2] = np.nan
        refused("u_seq of instance 6, step 1, input 2 is not finite", u_seq=bad)
        refused("u_seq of instance 6, step 1, input 2 is not finite", u_seq=bad, policy=True)      # a ruled channel of u_seq is ignored but must be finite
        refused("u_seq has shape", exc=ValueError, u_seq=np.zeros((B, c.N + 1, nu)))
        up = np.zeros((B, nu))
        up[6, 2] = np.inf
        refused("u_prev of instance 6, input 2 is not finite", policy=True, u_prev=up)
        p.upload_policy(thermostat(c, mode=[0] + [1] * (nu - 1)))
        refused("has not been solved", policy=True)                             # a passed-through channel needs the plan
        p.upload_policy(thermostat(c))
        p.launch()
        try:
            with pytest.raises(gpu.MldGpuError, match="has not been finished"):
                p.warm_start_from_rollout(c.R, policy=True)
        finally:
            p.finish()
        assert np.array_equal(p.debug_warm_start(), mark)
        tv.upload(c.x0, c.om, c.midx)
        with pytest.raises(gpu.MldGpuError, match="time-varying"):
            tv.warm_start_from_rollout(c.R, u_seq=u_seq)
        assert tv.debug_warm_start() is None
        good = p.warm_start_from_rollout(c.R, policy=True)                      # ... and one good call afterwards still works
        assert np.all(good["source"] == 1) and not np.array_equal(p.debug_warm_start(), mark)
    finally:
        plain.close(); tv.close(); tv_model.close()
        p.upload_policy(None)
