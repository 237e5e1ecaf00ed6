"""The resolving plant step with fallback inputs (mld_sim_step_fallback / GpuProblem.sim_step(resolve=R, fallback=...), kernels k_fallback_inputs and
k_fallback_commit): an instance whose solve left no usable plan takes its u from the plan memory's row for the current time, then from the resident
policy's rule, instead of being frozen.  The yardstick is the route the library had before, on a second handle over the same models: download() the
plans, fallback.choose_np / commit_np with the memory held in numpy, sim_step(resolve=R, u0=u) -- both routes feed the same u to the same kernels, so
everything is equal bit for bit.

The lever that makes an instance plan-less without making its plant infeasible is set_cutoffs with an unbeatable value (-1e30): the header documents that
such a search ends INFEASIBLE with objective +inf.  An advance clears cutoffs, so they are set before every solve.  Every test asserts on the downloaded
plan that exactly the chosen instances are unusable, and that every resolver status is 0 (or -1 where nothing was attempted).

Shapes: those of tests/test_gpu_sim_resolve.py.  a10 and a1 have N_tilde = 3, the smallest horizon with two memory rows; b9 has N_tilde = 2, where one row
is all a memory can give (age 2 is already exhausted), so the chain is run on it with the sources that horizon yields and, as "b9n3", on the same models at
N_tilde = 3 with the sources of the other shapes."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_sim_resolve import OUT, SHAPES
from test_gpu_small_lds_step import _SmallCtx
from test_gpu_policy_step import STEP_OUT, thermostat
from pyhybridcontrol_amd import _lib, fallback, gpu, policy, profiles

pytestmark = pytest.mark.gpu

_CACHE = {}
FB_SHAPES = dict(SHAPES, b9n3=SHAPES["b9"][:2] + (3,) + SHAPES["b9"][3:])
BOTH = ("memory", "policy")
CUT = -1e30
GUARD = 1e-4
LOG_PLANT = ("x", "v", "y", "omega", "x_k1", "cons", "cons_vio", "cons_row")
LOG_SOLVE = ("obj", "lower_bound", "status", "nodes")


@pytest.fixture(scope="module")
def ctx():
    def get(name, **kw):
        key = (name,) + tuple(sorted(kw.items()))
        if key not in _CACHE:
            _CACHE[key] = _SmallCtx(*FB_SHAPES[name], **{k: v for k, v in kw.items() if k != "twin"})
        return _CACHE[key]
    yield get
    for c in _CACHE.values():
        c.close()
    _CACHE.clear()


def _equal(a, b, names, what):
    for k in names:
        assert np.array_equal(a[k], b[k], equal_nan=True), (what, k)


def _solve_cut(handles, B, chosen):
    """the solve of one step on every handle with the chosen instances cut off; the guards on the downloaded plan; returns (plan, usable)"""
    cut = np.full(B, np.inf)
    cut[chosen] = CUT
    plans = []
    for h in handles:
        h.set_cutoffs(cut)
        h.solve_resident()
        plans.append(h.download())
    plan = plans[0]
    usable = np.isin(plan["status"], (0, 2)) & np.isfinite(plan["obj"])
    want = np.ones(B, bool)
    want[chosen] = False
    assert np.array_equal(usable, want), (plan["status"], plan["obj"])          # the chosen instances are unusable, all others usable
    for other in plans[1:]:
        assert np.array_equal(other["v"][usable], plan["v"][usable]) and np.array_equal(other["status"], plan["status"])
    return plan, usable


def _plan_u(c, plan):
    return np.ascontiguousarray(plan["v"].reshape(c.B, c.N, c.nv)[:, :, :c.nu])


def _library(c, T):
    """forecast series (the scenario's, periodic) and realised series (each instance's scaled by its own factor) in one library, one group"""
    B, N, nw = c.B, c.N, c.nw
    fc = [np.tile(c.om[b].reshape(N, nw), (T // N + 1, 1))[:T] for b in range(B)]
    act = [s * (1.0 + 0.01 * (b + 1)) for b, s in enumerate(fc)]
    lib, base = profiles.pack(fc + act)
    base = np.asarray(base, np.int64)
    return lib, base[:B].reshape(B, 1), base[B:].reshape(B, 1)


@pytest.mark.parametrize("shape", list(SHAPES))
def test_no_source_allowed_is_the_resolving_step_bit_for_bit(ctx, shape):
    c, t = ctx(shape), ctx(shape, twin=True)
    p, q, B = c.p, t.p, c.B
    chosen = [min(1, B - 1)]
    try:
        for h in (p, q):
            h.upload(c.x0, c.om, c.midx)
            h.sim_log_begin(1)
        plan, usable = _solve_cut((p, q), B, chosen)
        got = p.sim_step(resolve=c.R, fallback=(), outputs=True)
        ref = q.sim_step(resolve=t.R, outputs=True)
        _equal(got, ref, STEP_OUT, shape)
        assert got["n_skipped"] == 1 and np.all(got["aux_status"][usable] == 0) and np.all(got["aux_status"][~usable] == -1)
        assert got["u_source"].dtype == np.int32 and np.array_equal(got["u_source"], np.where(usable, 0, -1))
        for a, b in zip(p.inputs(), q.inputs()):
            assert np.array_equal(a, b)
        assert np.array_equal(p.inputs()[0][~usable], c.x0[~usable])
        la, lb = p.sim_log(), q.sim_log()
        _equal(la, lb, list(la), shape + " log")
        assert np.array_equal(p.sim_log_aux(), q.sim_log_aux())
        assert np.array_equal(p.sim_log_source()[0], got["u_source"]) and np.all(q.sim_log_source() == -2)
        with pytest.raises(gpu.MldGpuError, match="already been applied"):
            p.sim_step(resolve=c.R, fallback=())                                # the handle ends `advanced`, as after sim_step(resolve=R)
    finally:
        for h in (p, q):
            h.sim_log_begin(0)


# which instances are cut off at which step, and the sources that follow from it, worked out by hand from the rule: at N_tilde = 3 the memory serves two
# steps (rows 1 and 2) before the policy takes over; at N_tilde = 2 its only row is age 1, so instance 1's second step without a plan already falls
# through to the policy
CHAIN_CUT = {0: (0,), 1: (1, 2, 3), 2: (2,)}
CHAIN_SOURCES = {3: {0: [2, 0, 0, 0, 0], 1: [0, 1, 1, 2, 0], 2: [0, 0, 1, 0, 0]},
                 2: {0: [2, 0, 0, 0, 0], 1: [0, 1, 2, 2, 0], 2: [0, 0, 1, 0, 0]}}


@pytest.mark.parametrize("shape", list(FB_SHAPES))
def test_the_chain_equals_the_host_loop_bit_for_bit(ctx, shape):
    c, t = ctx(shape), ctx(shape, twin=True)
    p, q, B, N, nu = c.p, t.p, c.B, c.N, c.nu
    K = 5
    P = thermostat(c)
    lib, fstart, astart = _library(c, N + K + 3)
    want_src = np.zeros((K, B), np.int32)
    for b, row in CHAIN_SOURCES[N].items():
        if b < B:
            want_src[:, b] = row
    try:
        for h in (p, q):
            h.upload(c.x0, c.om, c.midx)
            h.upload_profiles(lib)
            h.forecast_from_profiles(fstart, 0)
            h.sim_log_begin(K)
        p.upload_policy(P)
        p.plan_memory()
        mem, age, up = np.zeros((B, N, nu)), np.full(B, -1, np.int32), P.initial_state(c.midx)
        state = p.plan_memory_state()
        assert np.array_equal(state["age"], age) and state["age"].dtype == np.int32 and np.array_equal(state["u"], mem)
        plans = []
        for k in range(K):
            chosen = [b for b, steps in CHAIN_CUT.items() if k in steps and b < B]
            plan, usable = _solve_cut((p, q), B, chosen)
            plans.append(plan)
            got = p.sim_step(resolve=c.R, fallback=BOTH, act_start=astart, step=k, advance=True, outputs=True)
            c.in_lds()
            x = q.inputs()[0]
            s = policy.selector_values(P, c.midx, x)
            assert np.all(np.abs(s - P.on_at[c.midx]) >= GUARD) and np.all(np.abs(s - P.off_at[c.midx]) >= GUARD), k
            u, src = fallback.choose_np(usable, plan["v"][:, :nu], mem, age, BOTH, P=P, midx=c.midx, x=x, u_prev=up)
            ref = q.sim_step(resolve=t.R, u0=u, act_start=astart, step=k, advance=True, outputs=True)
            what = "%s step %d" % (shape, k)
            _equal(got, ref, STEP_OUT, what)
            assert np.array_equal(got["u_source"], src) and np.array_equal(src, want_src[k]), what
            assert got["n_skipped"] == 0 and np.all(got["aux_status"] == 0) and np.array_equal(got["v0"][:, :nu], u), what
            mem, age = fallback.commit_np(src, _plan_u(c, plan), mem, age, N)
            up = u                                                              # every instance advanced
            state = p.plan_memory_state()
            assert np.array_equal(state["u"], mem) and np.array_equal(state["age"], age), what
            assert np.array_equal(p.policy_state(), up), what
            for a, b in zip(p.inputs(), q.inputs()):
                assert np.array_equal(a, b), what
            assert p.sim_log_count() == q.sim_log_count() == (k + 1, K)
            for h in (p, q):
                h.forecast_from_profiles(None, k + 1)
            for a, b in zip(p.inputs(), q.inputs()):
                assert np.array_equal(a, b), what
        la, lb = p.sim_log(), q.sim_log()
        _equal(la, lb, LOG_PLANT, shape + " log")
        for k in range(K):                                                      # the plan's, as they are (the u0 route records NaN / -1 there)
            for name in LOG_SOLVE:
                assert np.array_equal(la[name][k], plans[k][name], equal_nan=True), (shape, k, name)
        assert np.array_equal(p.sim_log_source(), want_src) and np.array_equal(p.sim_log_source(1, 2), want_src[1:3])
        assert np.array_equal(p.sim_log_aux(), q.sim_log_aux()) and np.all(q.sim_log_source() == -2)
    finally:
        for h in (p, q):
            h.sim_log_begin(0)
            h.upload_profiles(np.zeros(0))
        p.upload_policy(None)
        p.plan_memory(False)


def test_no_source_left(ctx):
    """memory only: instance 0 is cut off at step 0 (nothing remembered), instance 1 three times running from step 1 -- rows 1 and 2, then exhausted"""
    c = ctx("a10")
    p, B, N, nu = c.p, c.B, c.N, c.nu
    K = 4
    cuts = {0: (0,), 1: (1, 2, 3)}
    want_src = np.zeros((K, B), np.int32)
    want_src[:, 0], want_src[:, 1] = [-1, 0, 0, 0], [0, 1, 1, -1]
    try:
        p.upload(c.x0, c.om, c.midx)
        p.sim_log_begin(K)
        p.plan_memory()
        plan_1 = None
        for k in range(K):
            chosen = [b for b, steps in cuts.items() if k in steps]
            plan, usable = _solve_cut((p,), B, chosen)
            if k == 0:
                plan_1 = _plan_u(c, plan)[1]
            x_in, w_in = p.inputs()
            got = p.sim_step(resolve=c.R, fallback=("memory",), outputs=True)
            assert np.array_equal(got["u_source"], want_src[k]), k
            none = want_src[k] == -1
            assert none.sum() == (1 if k in (0, 3) else 0) and got["n_skipped"] == none.sum(), k      # skipped and counted
            assert np.all(got["aux_status"][none] == -1) and np.all(got["aux_status"][~none] == 0), k
            for name in ("x_k1", "y", "v0", "cons_vio"):
                assert np.all(np.isnan(got[name][none])) and np.all(np.isfinite(got[name][~none])), (k, name)
            assert np.all(got["cons_row"][none] == -1) and not got["cons"][none].any(), k
            x_new, w_new = p.inputs()
            assert np.array_equal(x_new[none], x_in[none]) and np.array_equal(w_new[none], w_in[none]), k      # its plant keeps its state
            assert np.array_equal(x_new[~none], got["x_k1"][~none]), k
            if k in (1, 2):
                assert np.array_equal(got["v0"][1, :nu], plan_1[k]), k          # the row the remembered plan made for this step
            age = p.plan_memory_state()["age"]
            assert age[0] == (-1 if k == 0 else 1) and age[1] == min(k + 1, N) and np.all(age[2:] == 1), (k, age)
        assert p.plan_memory_state()["age"][1] == N                             # capped
        log = p.sim_log()
        assert np.all(np.isnan(log["v"][0, 0])) and np.all(np.isnan(log["x_k1"][3, 1])) and log["cons_row"][3, 1] == -1 and not log["cons"][3, 1].any()
        assert np.array_equal(p.sim_log_source(), want_src) and np.array_equal(p.sim_log_aux(), np.where(want_src == -1, -1, 0))
    finally:
        p.sim_log_begin(0)
        p.plan_memory(False)


def test_state_rules(ctx):
    c = ctx("a10")
    p, B, N, nu = c.p, c.B, c.N, c.nu
    P = thermostat(c)
    lib, fstart, _ = _library(c, N + 4)
    rng = np.random.default_rng(9210)
    seed_u, seed_age = rng.normal(size=(B, N, nu)), (np.arange(B) % (N + 1)).astype(np.int32)
    seed_age[seed_age == 0] = -1
    mine = (rng.uniform(size=(B, nu)) < 0.5).astype(float)

    def seeded():
        st = p.plan_memory_state(u=seed_u, age=seed_age)
        assert np.array_equal(st["u"], seed_u) and np.array_equal(st["age"], seed_age)
        again = p.plan_memory_state()                                           # the round trip
        assert np.array_equal(again["u"], seed_u) and np.array_equal(again["age"], seed_age)

    def emptied(what):
        assert np.all(p.plan_memory_state()["age"] == -1), what

    try:
        p.upload(c.x0, c.om, c.midx)
        p.upload_profiles(lib)
        p.forecast_from_profiles(fstart, 0)
        p.upload_policy(P)
        p.policy_state(u_prev=mine)
        p.plan_memory()
        p.sim_log_begin(2)
        plan, _ = _solve_cut((p,), B, [2])
        seeded()                                                                # a solve in between does not empty it either (below)
        x_in, w_in = p.inputs()
        whatif = p.sim_step(resolve=c.R, fallback=BOTH, advance=False, log=False, outputs=True)
        assert whatif["u_source"][2] == (1 if 1 <= seed_age[2] <= N - 1 else 2) and np.all(np.delete(whatif["u_source"], 2) == 0)
        st = p.plan_memory_state()
        assert np.array_equal(st["u"], seed_u) and np.array_equal(st["age"], seed_age)          # advance=False: nothing is written
        assert np.array_equal(p.policy_state(), mine) and p.sim_log_count() == (0, 2)
        assert np.array_equal(p.inputs()[0], x_in) and np.array_equal(p.inputs()[1], w_in)
        took = p.sim_step(resolve=c.R, fallback=BOTH, advance=True, log=False, outputs=True)
        _equal(took, whatif, STEP_OUT + ("u_source",), "the step against its what-if")
        mem, age = fallback.commit_np(took["u_source"], _plan_u(c, plan), seed_u, seed_age, N)
        st = p.plan_memory_state()
        assert np.array_equal(st["u"], mem) and np.array_equal(st["age"], age) and not np.array_equal(age, seed_age)
        assert np.array_equal(p.policy_state(), took["v0"][:, :nu])
        p.forecast_from_profiles(None, 1)                                       # completes the step: the memory stays
        p.solve_resident()
        st = p.plan_memory_state()
        assert np.array_equal(st["u"], mem) and np.array_equal(st["age"], age)
        # an advance through any other entry point, and new inputs, empty it
        p.advance()
        emptied("advance()")
        p.solve_resident()
        seeded()
        p.sim_step(resolve=c.R, log=False)
        emptied("sim_step(resolve=R)")
        p.stage(c.x0[None], c.om[None])
        seeded()
        p.select(0)
        emptied("select()")
        seeded()
        p.upload(c.x0, c.om, c.midx)
        emptied("upload()")
        seeded()                                                                # ... and it is still enabled
        # disabled: freed, and a step that names it is refused
        p.plan_memory(False)
        p.solve_resident()
        with pytest.raises(gpu.MldGpuError, match="no plan memory is enabled"):
            p.sim_step(resolve=c.R, fallback=("memory",), log=False)
        with pytest.raises(gpu.MldGpuError, match="no plan memory enabled"):
            p.plan_memory_state()
        assert p.sim_step(resolve=c.R, fallback=("policy",), advance=False, log=False) == 0
    finally:
        p.sim_log_begin(0)
        p.upload_profiles(np.zeros(0))
        p.upload_policy(None)
        p.plan_memory(False)


def test_a_model_without_auxiliaries(ctx):
    """aux == NULL: the step is sim_step(v0 = u) for the chosen u -- instance 1 from the memory, instance 4 from the policy"""
    e = ctx("a10", hard=True, tie=False)
    p, B, N, nu = e.p, e.B, e.N, e.nu
    assert e.nv == nu and e.R.problem is None
    P = thermostat(e)
    rng = np.random.default_rng(9220)
    mem = (rng.uniform(size=(B, N, nu)) < 0.5).astype(float)
    age = np.full(B, -1, np.int32)
    age[1] = 2
    try:
        p.upload(e.x0, e.om, e.midx)
        p.upload_policy(P)
        p.plan_memory()
        plan, usable = _solve_cut((p,), B, [1, 4])
        p.plan_memory_state(u=mem, age=age)
        up = P.initial_state(e.midx)
        u, src = fallback.choose_np(usable, plan["v"][:, :nu], mem, age, BOTH, P=P, midx=e.midx, x=e.x0, u_prev=up)
        assert src[1] == 1 and src[4] == 2 and np.array_equal(u[1], mem[1, 2])
        plain = p.sim_step(v0=u, advance=False, log=False, outputs=True)
        got = p.sim_step(resolve=e.R, fallback=BOTH, advance=True, log=False, outputs=True)
        _equal(got, plain, OUT, "no auxiliaries")
        assert np.array_equal(got["v0"], u) and np.array_equal(got["u_source"], src) and np.all(got["aux_status"] == 0) and got["n_skipped"] == 0
        mem2, age2 = fallback.commit_np(src, _plan_u(e, plan), mem, age, N)
        st = p.plan_memory_state()
        assert np.array_equal(st["u"], mem2) and np.array_equal(st["age"], age2) and age2[1] == N and age2[4] == -1
        assert np.array_equal(p.policy_state(), u) and np.array_equal(p.inputs()[0], got["x_k1"])
    finally:
        p.upload_policy(None)
        p.plan_memory(False)


def test_refusals_change_nothing(ctx):
    c = ctx("a10")
    p, R, B, N, nu = c.p, c.R, c.B, c.N, c.nu
    lib = _lib.load()
    P = thermostat(c)
    rng = np.random.default_rng(9230)
    seed_u, seed_age = rng.normal(size=(B, N, nu)), np.full(B, 1, np.int32)
    mine = (rng.uniform(size=(B, nu)) < 0.5).astype(float)
    state = {}

    def unchanged(what):
        x_in, w_in = p.inputs()
        assert np.array_equal(x_in, state["x"]) and np.array_equal(w_in, state["w"]) and p.sim_log_count() == state["count"], what
        if state.get("mem"):
            st = p.plan_memory_state()
            assert np.array_equal(st["u"], seed_u) and np.array_equal(st["age"], seed_age), what
        if state.get("pol"):
            assert np.array_equal(p.policy_state(), mine), what

    def snapshot(**kw):
        state.update(kw)
        state["x"], state["w"] = p.inputs()
        state["count"] = p.sim_log_count()

    def refused(match, **kw):
        with pytest.raises(gpu.MldGpuError, match=match):
            p.sim_step(resolve=kw.pop("resolve", R), fallback=kw.pop("fallback", ()), **kw)
        unchanged(match)

    def raw(h, aux, fb=0, flags=0):
        rc = lib.mld_sim_step_fallback(h, aux, fb, None, 0, flags, None, None, None, None, None, None, None, None, None)
        return rc, lib.mld_last_error()

    with pytest.raises(ValueError, match="fallback goes with resolve"):
        p.sim_step(fallback=BOTH)
    with pytest.raises(ValueError, match="fallback goes with resolve"):
        p.sim_step(resolve=R, fallback=BOTH, u0=np.zeros(nu))
    with pytest.raises(ValueError, match="not one of"):
        p.sim_step(resolve=R, fallback=("plan",))
    try:
        p.upload(c.x0, c.om, c.midx)
        p.sim_log_begin(2)
        snapshot()
        with pytest.raises(ValueError, match=r"u has shape"):
            p.plan_memory_state(u=np.zeros((B, N)))                             # shape checks come before any C call (no memory is enabled yet)
        with pytest.raises(ValueError, match=r"age has shape"):
            p.plan_memory_state(age=np.zeros(B))
        refused("has not been solved", advance=False)                           # an unsolved batch
        p.solve_resident()
        # the fallback's own refusals
        refused("unknown fallback bits", fallback=4, advance=False)
        refused("no plan memory is enabled", fallback=("memory",))
        refused("MLD_FB_POLICY, but no policy uploaded", fallback=BOTH[1:])
        p.upload_policy(thermostat(c, mode=[0] + [1] * (nu - 1)))
        refused("passes a channel through", fallback=("policy",))
        p.upload_policy(P)
        p.policy_state(u_prev=mine)
        p.plan_memory()
        p.plan_memory_state(u=seed_u, age=seed_age)
        snapshot(mem=True, pol=True)
        bad = seed_age.copy()
        bad[3] = N + 1
        with pytest.raises(gpu.MldGpuError, match="age of instance 3 is %d" % (N + 1)):
            p.plan_memory_state(age=bad)
        bad[3] = 0
        with pytest.raises(gpu.MldGpuError, match="age of instance 3 is 0"):
            p.plan_memory_state(age=bad)
        nan_u = seed_u.copy()
        nan_u[2, 1, 0] = np.nan
        with pytest.raises(gpu.MldGpuError, match="u of instance 2, step 1, input 0 is not finite"):
            p.plan_memory_state(u=nan_u)
        unchanged("plan_memory_state")
        # everything mld_sim_step_resolve(u0 = NULL) refuses
        refused("step = -1", fallback=BOTH, step=-1)
        refused("no profile library", fallback=BOTH, actual=True)
        rc, msg = raw(p._h, R.problem._h, fb=3, flags=8)
        assert rc == -1 and b"unknown flag" in msg
        rc, msg = raw(p._h, p._h, fb=3)
        assert rc == -1 and b"the stepped problem itself" in msg
        rc, msg = raw(p._h, None, fb=3)
        assert rc == -1 and b"aux == NULL" in msg
        unchanged("raw")
        refused("not the fold", resolve=ctx("b9").R, fallback=BOTH)
        assert p.sim_step(resolve=R, fallback=BOTH, advance=False, log=False) == 0          # lays the resolver's batch out; changes nothing
        unchanged("a what-if")
        rc, msg = raw(R.problem._h, None)                                       # the resolver's own problem: the folded models have no input
        assert rc == -1 and b"no input (nu = 0)" in msg
        R.problem.launch()
        with pytest.raises(gpu.MldGpuError, match="aux has a launched solve"):
            p.sim_step(resolve=R, fallback=BOTH)
        R.problem.finish()
        unchanged("aux in flight")
        p.launch()
        with pytest.raises(gpu.MldGpuError, match="has not been finished"):
            p.sim_step(resolve=R, fallback=BOTH)
        p.finish()
        unchanged("problem in flight")
        tv_model = gpu.GpuModel([[m] for m in c.mats], c.d, time_varying=True)
        tv = gpu.GpuProblem(tv_model, 0, 1, None)
        try:
            tv.upload(c.x0, c.om[:, :c.nw], c.midx)
            rc, msg = raw(tv._h, R.problem._h)
            assert rc == -1 and b"time-varying" in msg
        finally:
            tv.close(); tv_model.close()
        # a full log
        assert p.sim_step(resolve=R, fallback=BOTH, advance=False, log=True) == 0 and p.sim_step(resolve=R, fallback=BOTH, advance=False, log=True) == 0
        snapshot()
        assert state["count"] == (2, 2)
        refused("log is full", fallback=BOTH, log=True)
        # an advanced batch
        assert p.sim_step(resolve=R, fallback=BOTH, log=False) == 0
        seed_age[:] = 1                                                         # every plan was usable: remembered, age 1
        seed_u[:] = _plan_u(c, p.download())
        mine[:] = p.policy_state()
        snapshot()
        refused("already been applied", fallback=BOTH, log=False)
    finally:
        p.sim_log_begin(0)
        p.upload_policy(None)
        p.plan_memory(False)
