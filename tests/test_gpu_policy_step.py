"""One resolving plant step under a rule-based feedback policy (mld_sim_step_policy / GpuProblem.sim_step(resolve=R, policy=True), kernels k_policy_inputs
and k_policy_commit): the device writes u from the current x0, the resident u_prev and the policy tables; the rest is mld_sim_step_resolve's own phases.
The yardstick is the route the library had before: download x, policy.apply_np on the host, sim_step(resolve=R, u0=u) on a second handle over the same
models -- both routes feed the same u to the same kernels, so everything is equal bit for bit.  Then the resident policy state: what-if, skipped
instances, upload(), the round trip; mixed modes; a model without auxiliaries; the refusals."""
import numpy as np
import pytest

from test_gpu_sim_resolve import INFEASIBLE, OUT, SHAPES
from test_gpu_small_lds_step import _SmallCtx
from pyhybridcontrol_amd import gpu, policy, profiles

pytestmark = pytest.mark.gpu

_CACHE = {}
STEP_OUT = OUT + ("v0", "aux_status", "n_skipped")


@pytest.fixture(scope="module")
def ctx():
    def get(name, **kw):
        key = (name,) + tuple(sorted(kw.items()))
        if key not in _CACHE:
            _CACHE[key] = _SmallCtx(*SHAPES[name], **{k: v for k, v in kw.items() if k != "twin"})
        return _CACHE[key]
    yield get
    for c in _CACHE.values():
        c.close()
    _CACHE.clear()


def thermostat(c, on_at=57.5, off_at=60.5, **kw):
    return policy.ThresholdPolicy(np.broadcast_to(np.eye(c.nx), (len(c.mats), c.nu, c.nx)), on_at, off_at, **kw)


def _equal(a, b, names, what):
    for k in names:
        assert np.array_equal(a[k], b[k], equal_nan=True), (what, k)


@pytest.mark.parametrize("shape", list(SHAPES))
def test_four_logged_steps_equal_the_host_loop_bit_for_bit(ctx, shape):
    c, t = ctx(shape), ctx(shape, twin=True)                                # the same models twice (the seeds are the shape's): one handle per route
    p, q, B, N, nw = c.p, t.p, c.B, c.N, c.nw
    P = thermostat(c)
    T = N + 8
    series = [np.tile(c.om[b].reshape(N, nw), (T // N + 1, 1))[:T] * (1.0 + 0.01 * b) for b in range(B)]
    lib, base = profiles.pack(series)
    start = np.asarray(base, np.int64).reshape(B, 1)
    try:
        for h in (p, q):
            h.upload(c.x0, c.om, c.midx)
            h.upload_profiles(lib)
            h.sim_log_begin(4)
        p.upload_policy(P)
        up = P.initial_state(c.midx)
        assert np.array_equal(p.policy_state(), up)
        switched_on = switched_off = False
        for k in range(4):
            got = p.sim_step(resolve=c.R, policy=True, act_start=start, step=k, advance=True, outputs=True)
            c.in_lds()
            x = q.inputs()[0]
            u = policy.apply_np(P, c.midx, x, up)
            ref = q.sim_step(resolve=t.R, u0=u, act_start=start, step=k, advance=True, outputs=True)
            _equal(got, ref, STEP_OUT, "%s step %d" % (shape, k))
            assert got["n_skipped"] == 0 and np.array_equal(got["v0"][:, :c.nu], u)
            assert np.array_equal(p.policy_state(), u), k                   # the resident u_prev is the u applied
            assert np.array_equal(p.inputs()[0], q.inputs()[0]) and p.sim_log_count() == q.sim_log_count() == (k + 1, 4)
            switched_on, switched_off = switched_on or bool(((u == 1) & (up == 0)).any()), switched_off or bool(((u == 0) & (up == 1)).any())
            up = u
        assert switched_on and (switched_off or B == 1)
        la, lb = p.sim_log(), q.sim_log()
        for k in la:
            assert np.array_equal(la[k], lb[k], equal_nan=True), k          # the record is what the resolving step writes (status -1 / NaN: the caller's u)
        assert np.array_equal(p.sim_log_aux(), q.sim_log_aux()) and np.all(p.sim_log_aux() == 0)
    finally:
        for h in (p, q):
            h.sim_log_begin(0)
            h.upload_profiles(np.zeros(0))
        p.upload_policy(None)


def test_the_policy_state(ctx):
    """advance=False leaves it; an advancing step moves it; policy_state() round-trips; upload() resets it; a new policy resets it"""
    c = ctx("a10")
    p, B, nu = c.p, c.B, c.nu
    P = thermostat(c)
    rng = np.random.default_rng(9020)
    mine = (rng.uniform(size=(B, nu)) < 0.5).astype(float)
    try:
        p.upload(c.x0, c.om, c.midx)
        p.upload_policy(P)
        assert np.array_equal(p.policy_state(u_prev=mine), mine) and np.array_equal(p.policy_state(), mine)
        want = policy.apply_np(P, c.midx, c.x0, mine)
        assert not np.array_equal(want, mine) and not np.array_equal(want, policy.apply_np(P, c.midx, c.x0, np.zeros((B, nu))))      # the state matters, and moves
        x_before = p.inputs()[0]
        whatif = p.sim_step(resolve=c.R, policy=True, advance=False, log=False, outputs=True)
        assert np.array_equal(whatif["v0"][:, :nu], want) and np.array_equal(p.policy_state(), mine) and np.array_equal(p.inputs()[0], x_before)
        again = p.sim_step(resolve=c.R, policy=True, advance=False, log=False, outputs=True)
        _equal(again, whatif, STEP_OUT, "what-if twice")
        took = p.sim_step(resolve=c.R, policy=True, advance=True, log=False, outputs=True)
        _equal(took, whatif, STEP_OUT, "the step against its what-if")
        assert np.array_equal(p.policy_state(), want) and np.array_equal(p.inputs()[0], took["x_k1"])
        assert p.sim_step(resolve=c.R, policy=True, advance=True, log=False) == 0                     # without outputs: the skip count
        p.upload(c.x0, c.om, c.midx)
        assert np.array_equal(p.policy_state(), np.zeros((B, nu)))                                    # upload() resets: every ruled channel at u_off
        p.policy_state(u_prev=mine)
        p.upload_policy(policy.ThresholdPolicy(P.sel, 57.5, 60.5, u_on=2.0, u_off=-1.0, mode=[1] * (nu - 1) + [0]))
        reset = np.full((B, nu), -1.0)
        reset[:, -1] = 0.0
        assert np.array_equal(p.policy_state(), reset)                                                # a new policy: its own u_off, 0 on the passed-through channel
        assert np.array_equal(p.policy_state(u_prev=np.ones(nu)), np.ones((B, nu))) and np.array_equal(p.policy_state(reset=True), reset)
    finally:
        p.upload_policy(None)


def test_skipped_instances_keep_their_state(ctx):
    """the hard 3-tank model: a tank above T_max leaves the auxiliary problem without a feasible point -- the instance is skipped, not advanced, and its
    resident u_prev stays"""
    c = ctx("a10", hard=True)
    p, B, nu = c.p, c.B, c.nu
    P = thermostat(c)
    hot = np.zeros(B, bool)
    hot[[1, 4, 7]] = True
    x = c.x0.copy()
    x[hot, 0] = 90.0
    mine = np.tile(np.array([1.0, 0.0, 1.0])[:nu], (B, 1))
    try:
        p.upload(x, c.om, c.midx)
        p.upload_policy(P)
        p.policy_state(u_prev=mine)
        want = policy.apply_np(P, c.midx, x, mine)
        assert not np.array_equal(want[hot], mine[hot])
        got = p.sim_step(resolve=c.R, policy=True, advance=True, log=False, outputs=True)
        assert got["n_skipped"] == 3 and np.all(got["aux_status"][hot] == INFEASIBLE) and np.all(got["aux_status"][~hot] == 0)
        assert np.all(np.isnan(got["v0"][hot])) and np.array_equal(got["v0"][~hot][:, :nu], want[~hot])
        state = p.policy_state()
        assert np.array_equal(state[hot], mine[hot]) and np.array_equal(state[~hot], want[~hot])
        assert np.array_equal(p.inputs()[0][hot], x[hot]) and np.array_equal(p.inputs()[0][~hot], got["x_k1"][~hot])
    finally:
        p.upload_policy(None)


def test_mixed_modes_and_the_resident_plan(ctx):
    """channel 0 passed through: from u0, then (u0=None) from the resident plan, as sim_step(resolve=R) takes it; the handle ends `advanced`"""
    c, t = ctx("a10"), ctx("a10", twin=True)
    p, q, B, nu = c.p, t.p, c.B, c.nu
    P = thermostat(c, mode=[0] + [1] * (nu - 1))
    rng = np.random.default_rng(9030)
    u0 = (rng.uniform(size=(B, nu)) < 0.5).astype(float)
    try:
        for h in (p, q):
            h.upload(c.x0, c.om, c.midx)
        p.upload_policy(P)
        with pytest.raises(gpu.MldGpuError, match="has not been solved"):
            p.sim_step(resolve=c.R, policy=True, advance=False, log=False)      # a passed-through channel needs u0 or a plan
        want = policy.apply_np(P, c.midx, c.x0, P.initial_state(c.midx), u0)
        assert np.array_equal(want[:, 0], u0[:, 0])
        got = p.sim_step(resolve=c.R, policy=True, u0=u0, advance=False, log=False, outputs=True)
        ref = q.sim_step(resolve=t.R, u0=want, advance=False, log=False, outputs=True)
        _equal(got, ref, STEP_OUT, "from u0")
        for h in (p, q):
            h.solve_resident()
        plan = p.download()
        assert np.all(np.isin(plan["status"], (0, 2)) & np.isfinite(plan["obj"])) and np.array_equal(plan["v"], q.download()["v"])
        want = policy.apply_np(P, c.midx, c.x0, P.initial_state(c.midx), plan["v"][:, :nu])
        got = p.sim_step(resolve=c.R, policy=True, advance=True, log=False, outputs=True)
        ref = q.sim_step(resolve=t.R, u0=want, advance=True, log=False, outputs=True)
        _equal(got, ref, STEP_OUT, "from the plan")
        assert np.array_equal(p.policy_state(), want)
        with pytest.raises(gpu.MldGpuError, match="already been applied"):
            p.sim_step(resolve=c.R, policy=True, advance=False, log=False)      # the plan belongs to inputs that are gone, as after sim_step(resolve=R)
    finally:
        p.upload_policy(None)


def test_a_model_without_auxiliaries(ctx):
    """aux == NULL: the step is sim_step(v0 = u) with the rule's u"""
    e = ctx("a10", hard=True, tie=False)
    p, B = e.p, e.B
    assert e.nv == e.nu and e.R.problem is None
    P = thermostat(e)
    try:
        p.upload(e.x0, e.om, e.midx)
        p.upload_policy(P)
        want = policy.apply_np(P, e.midx, e.x0, np.zeros((B, e.nu)))
        assert (want == 1).any() and (want == 0).any()
        plain = p.sim_step(v0=want, advance=False, log=False, outputs=True)
        got = p.sim_step(resolve=e.R, policy=True, advance=True, log=False, outputs=True)
        _equal(got, plain, OUT, "no auxiliaries")
        assert np.array_equal(got["v0"], want) and np.all(got["aux_status"] == 0) and got["n_skipped"] == 0
        assert np.array_equal(p.policy_state(), want) and np.array_equal(p.inputs()[0], got["x_k1"])
    finally:
        p.upload_policy(None)


def test_refusals(ctx):
    c = ctx("a10")
    p, B, nu = c.p, c.B, c.nu
    p.upload(c.x0, c.om, c.midx)
    x_in = p.inputs()[0]
    with pytest.raises(gpu.MldGpuError, match="no policy uploaded"):
        p.sim_step(resolve=c.R, policy=True, advance=True, log=False)
    with pytest.raises(ValueError, match="policy=True goes with resolve"):
        p.sim_step(policy=True)
    try:
        p.upload_policy(thermostat(c))
        bad = np.zeros((B, nu))
        bad[3, 1] = np.nan
        with pytest.raises(gpu.MldGpuError, match="u0 of instance 3, input 1 is not finite"):
            p.sim_step(resolve=c.R, policy=True, u0=bad, advance=True, log=False)      # ignored on a ruled channel, but finite
        with pytest.raises(gpu.MldGpuError, match="MLD_SIM_LOG, but no log"):
            p.sim_step(resolve=c.R, policy=True, advance=True, log=True)
        with pytest.raises(gpu.MldGpuError, match="aux == NULL"):
            p.sim_step(resolve=type("NoAux", (), dict(problem=None))(), policy=True, advance=True, log=False)
        assert np.array_equal(p.inputs()[0], x_in) and np.array_equal(p.policy_state(), np.zeros((B, nu)))
    finally:
        p.upload_policy(None)
