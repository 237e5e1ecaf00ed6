"""The resolving plant step that applies a kept selection (mld_keep_selection / mld_set_selection / mld_download_selection / mld_sim_step_selected /
mld_download_sim_log_pick; GpuProblem.select_plan(..., keep=True), select_plan_policies(..., keep=True), selection(), set_selection(),
sim_step(resolve=R, selected=True), sim_log_pick(); kernels k_selected_inputs and k_selected_commit).  The yardstick is the route the library had before, on
a second handle over the same models, built the way tests/test_gpu_fallback_step.py builds its reference: selection() downloaded,
fallback.choose_selected_np / commit_selected_np with the memory held in numpy, sim_step(resolve=R, u0=u) -- both routes feed the same u to the same
kernels, so everything is equal bit for bit.

Shapes: make_agent(3) x 3 models interleaved by model_idx at N_tilde = 3, the resolver on the small-LDS path, S = 2 realisations, batch 37 and 67 -- with
nu = 3 neither batch nu (111, 201) nor batch N nu (333, 603) is a multiple of the 256 threads of a workgroup, and an instance's elements straddle a
workgroup boundary -- and P = 3 candidates: the plan first, one sequence, the thermostat.

The levers: set_cutoffs with an unbeatable value (tests/test_gpu_fallback_step.py) leaves chosen instances without a plan, so candidate 0 is not attempted
for them; a bound on the worst realisation's cost, the median over the instances of their best candidate's, leaves about half of the instances without an
admissible candidate (choice -1); plan_memory_state seeds the ages."""
import numpy as np
import pytest

import _rollout_ref
from test_gpu_small_lds_step import _SmallCtx
from test_gpu_policy_step import STEP_OUT, thermostat
from test_gpu_fallback_step import _library, _solve_cut, _plan_u, BOTH, GUARD
from pyhybridcontrol_amd import _lib, fallback, gpu, policy, synthetic as syn
from pyhybridcontrol_amd.aux_resolve import BatchAuxResolver
from pyhybridcontrol_amd.simlog import PlanSelector, RiskTable

pytestmark = pytest.mark.gpu

N, S = 3, 2
BATCHES = (37, 67)
_CACHE = {}
SEL_KEYS = ("choice", "policy", "u")


@pytest.fixture(scope="module")
def ctx():
    def get(B, twin=False):
        if (B, twin) not in _CACHE:
            _CACHE[(B, twin)] = _SmallCtx(3, 3, N, B)
        return _CACHE[(B, twin)]
    yield get
    for c in _CACHE.values():
        c.close()
    _CACHE.clear()


def _equal(a, b, names, what):
    for k in names:
        assert np.array_equal(a[k], b[k], equal_nan=True), (what, k)


def _scenario(c, K, seed):
    """(omega_seq (B, S, K, nomega), one random binary sequence per instance (B, 1, K, nu), cost_w (K, nv) of either sign, so that no kind of candidate is
    the cheapest for every instance)"""
    rng = np.random.default_rng(seed)
    _, _, _, om_seq = _rollout_ref.realised_library(c.om, c.N, c.nw, c.nx, S, K, 1, rng)
    cand = (rng.uniform(size=(c.B, 1, K, c.nu)) < 0.4).astype(float)
    return np.ascontiguousarray(om_seq), cand, rng.uniform(-1.0, 1.0, size=(K, c.nv))


def _risk():
    return RiskTable(None, (0.5,)).add("cost", "cost", level=0.0).add("vio", "worst_vio", level=1e-6)


def _selector(bound=None):
    sel = PlanSelector(_risk()).minimise("cost", "mean")
    return sel if bound is None else sel.subject_to("cost", "max", bound)


def _bound(p, c, P, K, om_seq, cand, cw):
    """the median over the instances of their best candidate's worst-realisation cost: about half of them keep an admissible candidate.  P: the thermostat,
    or None for the plan and the sequence alone (select_plan_policies() without policies is select_plan())"""
    probe = p.select_plan_policies(c.R, _selector(), policies=[P] if P is not None else None, candidates=cand, plan_first=True, K=K, omega_seq=om_seq, cost_w=cw, per_candidate=True)
    worst = np.where(probe["admissible"], probe["risk"]["max"][:, :, 0], np.inf)
    return float(np.median(worst.min(axis=1)))


def _select(p, c, P, sel, K, om_seq, cand, cw, **kw):
    out = p.select_plan_policies(c.R, sel, policies=[P] if P is not None else None, candidates=cand, plan_first=True, K=K, omega_seq=om_seq, cost_w=cw, **kw)
    out.setdefault("policy", np.full(p.batch, -1, np.int32))                    # (select_plan() has no policy to report)
    return out


def _clean(*problems):
    for p in problems:
        p.set_cutoffs(np.full(p.batch, np.inf))
        p.sim_log_begin(0)
        p.upload_profiles(np.zeros(0))
        p.upload_policy(None)
        p.plan_memory(False)
        _lib.check(_lib.load().mld_keep_selection(p._h, 0))
        p._sel_keep = False


def _guard(P, midx, x, what):
    s = policy.selector_values(P, midx, x)
    assert np.all(np.abs(s - P.on_at[midx]) >= GUARD) and np.all(np.abs(s - P.off_at[midx]) >= GUARD), what


def _begin(c, handles, P, K_log, T):
    lib, fstart, astart = _library(c, T)
    for h in handles:
        h.upload(c.x0, c.om, c.midx)
        h.upload_profiles(lib)
        h.forecast_from_profiles(fstart, 0)
        h.sim_log_begin(K_log)
    handles[0].upload_policy(P)
    handles[0].plan_memory()
    return astart


@pytest.mark.parametrize("B", BATCHES)
def test_the_chain_equals_the_host_route_bit_for_bit(ctx, B):
    """five chained, logged, advancing steps; at every step some instances are without a plan and some without an admissible candidate.  Even steps choose
    among the plan, a random sequence and the thermostat.  Odd steps choose between the plan and a sequence alone (select_plan's own route), and the sequence
    of every even instance with a plan IS its plan's inputs: the two tie in every bit, the smaller p wins, so the plan is applied wherever it is admissible"""
    c, t = ctx(B), ctx(B, twin=True)
    p, q, nu = c.p, t.p, c.nu
    K = 5
    P = thermostat(c)
    om_seq, _, cw = _scenario(c, N, 9400 + B)
    srcs, picks = [], []
    try:
        astart = _begin(c, (p, q), P, K, N + K + 3)
        mem, age, up = np.zeros((B, N, nu)), np.full(B, -1, np.int32), P.initial_state(c.midx)
        for k in range(K):
            what = "B %d step %d" % (B, k)
            plan, usable = _solve_cut((p,), B, [b for b in range(B) if (b + k) % 5 == 0])
            cand = _scenario(c, N, 9410 + 10 * B + k)[1]
            pol = P if k % 2 == 0 else None
            if pol is None:
                twin = usable & (np.arange(B) % 2 == 0)
                cand[twin, 0] = _plan_u(c, plan)[twin]
            bound = _bound(p, c, pol, N, om_seq, cand, cw)
            out = _select(p, c, pol, _selector(bound), N, om_seq, cand, cw, keep=True)
            if pol is None:                                                     # the tie goes to the plan; how many twins are admissible is the data's
                assert np.all(out["choice"][twin] <= 0), what                   # business: that the plan IS applied somewhere is asserted on the whole chain
            sel = p.selection()
            assert sel["valid"] and sel["K"] == N and sel["choice"].dtype == sel["policy"].dtype == np.int32, what
            _equal(sel, out, SEL_KEYS, what + " selection()")
            got = p.sim_step(resolve=c.R, selected=True, fallback=BOTH, act_start=astart, step=k, advance=True, outputs=True)
            c.in_lds()
            x = q.inputs()[0]
            _guard(P, c.midx, x, what)
            u, src, pick = fallback.choose_selected_np(sel["choice"], sel["u"], mem, age, BOTH, P=P, midx=c.midx, x=x, u_prev=up)
            ref = q.sim_step(resolve=t.R, u0=u, act_start=astart, step=k, advance=True, outputs=True)
            _equal(got, ref, STEP_OUT, what)
            assert np.array_equal(got["u_source"], src) and np.array_equal(got["pick"], pick) and got["pick"].dtype == got["u_source"].dtype == np.int32, what
            assert got["n_skipped"] == 0 and np.all(got["aux_status"] == 0) and np.array_equal(got["v0"][:, :nu], u), what
            mem, age = fallback.commit_selected_np(src, sel["policy"], sel["u"], mem, age, N)
            up = u                                                              # every instance advanced
            state = p.plan_memory_state()
            assert np.array_equal(state["u"], mem) and np.array_equal(state["age"], age), what
            assert np.array_equal(p.policy_state(), up), what
            assert not p.selection()["valid"], what                             # consumed
            for a, b in zip(p.inputs(), q.inputs()):
                assert np.array_equal(a, b), what
            assert p.sim_log_count() == q.sim_log_count() == (k + 1, K)
            for h in (p, q):
                h.forecast_from_profiles(None, k + 1)
            for a, b in zip(p.inputs(), q.inputs()):
                assert np.array_equal(a, b), what
            srcs.append(src); picks.append(pick)
        la, lb = p.sim_log(), q.sim_log()
        _equal(la, lb, list(la), "B %d log" % B)
        srcs, picks = np.array(srcs), np.array(picks)
        assert np.array_equal(p.sim_log_source(), srcs) and np.array_equal(p.sim_log_source(1, 2), srcs[1:3])
        assert np.array_equal(p.sim_log_pick(), picks) and np.array_equal(p.sim_log_pick(1, 2), picks[1:3])
        assert np.array_equal(p.sim_log_aux(), q.sim_log_aux()) and np.all(q.sim_log_source() == -2) and np.all(q.sim_log_pick() == -2)
        for s in (3, 1, 2):                                                     # the chain cannot pass on the selected source alone
            assert (srcs == s).sum() >= K, (s, (srcs == s).sum())
        assert set(np.unique(picks)) == {-1, 0, 1, 2}                           # the plan, the sequence and the thermostat were all applied somewhere
    finally:
        _clean(p, q)


def _one_step_setup(c, p, P, K=N, seed=9500, cut=True, ages=True, keep=True):
    """a solved batch with every fifth plan cut off, the memory seeded with ages -1, 1, N - 1, N in turn, a selection with a binding bound kept"""
    B, nu = c.B, c.nu
    rng = np.random.default_rng(seed)
    om_seq, cand, cw = _scenario(c, K, seed + B)
    plan, usable = _solve_cut((p,), B, [b for b in range(B) if b % 5 == 0] if cut else [])
    mem_u = rng.normal(size=(B, N, nu))
    mem_age = np.array([-1, 1, N - 1, N], np.int32)[np.arange(B) % 4]
    if ages:
        p.plan_memory_state(u=mem_u, age=mem_age)
    mine = (rng.uniform(size=(B, nu)) < 0.5).astype(float)
    p.policy_state(u_prev=mine)
    bound = _bound(p, c, P, K, om_seq, cand, cw)
    out = _select(p, c, P, _selector(bound), K, om_seq, cand, cw, keep=keep)
    return dict(plan=plan, usable=usable, mem_u=mem_u, mem_age=mem_age, up=mine, out=out, om_seq=om_seq, cand=cand, cw=cw, bound=bound)


@pytest.mark.parametrize("B", BATCHES)
def test_every_source_occurs(ctx, B):
    c = ctx(B)
    p, nu = c.p, c.nu
    P = thermostat(c)
    try:
        _begin(c, (p,), P, 2, N + 4)
        s = _one_step_setup(c, p, P)
        sel = p.selection()
        x = p.inputs()[0]
        _guard(P, c.midx, x, B)
        assert np.any((sel["choice"] == -1) & s["usable"])                      # a usable plan that the filter turned down: it must not be applied
        # memory and policy: nobody is left out
        u, src, pick = fallback.choose_selected_np(sel["choice"], sel["u"], s["mem_u"], s["mem_age"], BOTH, P=P, midx=c.midx, x=x, u_prev=s["up"])
        got = p.sim_step(resolve=c.R, selected=True, fallback=BOTH, advance=False, log=False, outputs=True)
        assert np.array_equal(got["u_source"], src) and np.array_equal(got["pick"], pick) and np.array_equal(got["v0"][:, :nu], u)
        share = {k: int((src == k).sum()) for k in (3, 1, 2, -1)}
        assert share[3] >= B // 8 and share[1] >= B // 8 and share[2] >= B // 8 and share[-1] == 0 and sum(share.values()) == B, share
        held = (s["mem_age"] >= 1) & (s["mem_age"] <= N - 1)
        assert np.array_equal(src == 1, (sel["choice"] < 0) & held) and np.array_equal(src == 2, (sel["choice"] < 0) & ~held)
        none = sel["choice"] < 0
        assert np.array_equal(u[src == 1], s["mem_u"][src == 1, s["mem_age"][src == 1]]) and np.array_equal(u[~none], sel["u"][~none, 0])
        # ... and never the plan's input where the filter turned a usable plan down (unless a source happens to agree with it)
        plan_u0 = s["plan"]["v"][:, :nu]
        turned = none & s["usable"] & np.any(plan_u0 != u, axis=1)
        assert turned.any() and np.array_equal(got["v0"][turned, :nu], u[turned])
        # memory only: the instances the policy served are not attempted
        u1, src1, pick1 = fallback.choose_selected_np(sel["choice"], sel["u"], s["mem_u"], s["mem_age"], ("memory",))
        got1 = p.sim_step(resolve=c.R, selected=True, fallback=("memory",), advance=False, log=False, outputs=True)
        left = src1 == -1
        assert np.array_equal(got1["u_source"], src1) and np.array_equal(left, src == 2) and left.sum() >= B // 8 and got1["n_skipped"] == left.sum()
        assert np.all(got1["aux_status"][left] == -1) and np.all(got1["aux_status"][~left] == 0) and np.all(got1["pick"][left] == -1)
        for name in ("x_k1", "y", "v0", "cons_vio"):
            assert np.all(np.isnan(got1[name][left])) and np.array_equal(got1[name][~left], got[name][~left]), name
        # no fallback argument: a choice or nothing
        got0 = p.sim_step(resolve=c.R, selected=True, advance=False, log=False, outputs=True)
        assert np.array_equal(got0["u_source"], np.where(none, -1, 3)) and got0["n_skipped"] == none.sum() and np.array_equal(got0["pick"], sel["choice"])
        assert p.selection()["valid"]
    finally:
        _clean(p)


@pytest.mark.parametrize("B", BATCHES[:1])
def test_the_gaps_the_step_closes(ctx, B):
    """after a selected advancing step the plan memory is still valid and holds the chosen sequence at age 1, u_prev is the applied input, the log says 3 and
    which candidate; the same campaign through sim_step(resolve=R, u0=...) empties the memory, leaves u_prev and logs -2"""
    c, t = ctx(B), ctx(B, twin=True)
    p, q, nu = c.p, t.p, c.nu
    P = thermostat(c)
    try:
        _begin(c, (p, q), P, 1, N + 4)
        q.upload_policy(P)
        q.plan_memory()
        s = _one_step_setup(c, p, P)
        r = _one_step_setup(t, q, P, keep=False)
        _equal(s["out"], r["out"], SEL_KEYS + ("u0", "score", "n_admissible", "admissible"), "the two handles select alike")
        sel = p.selection()
        got = p.sim_step(resolve=c.R, selected=True, fallback=BOTH, outputs=True)
        st = p.plan_memory_state()
        seq = (sel["choice"] >= 0) & (sel["policy"] < 0)
        assert seq.sum() >= B // 8 and (sel["policy"] >= 0).any()
        assert np.all(st["age"][seq] == 1) and np.array_equal(st["u"][seq], sel["u"][seq])          # remembered, and still there: the memory survived
        older = np.where(s["mem_age"] >= 1, np.minimum(s["mem_age"] + 1, N), s["mem_age"])
        assert np.array_equal(st["age"][~seq], older[~seq]) and np.array_equal(st["u"][~seq], s["mem_u"][~seq])
        assert got["n_skipped"] == 0 and np.array_equal(p.policy_state(), got["v0"][:, :nu]) and not np.array_equal(p.policy_state(), s["up"])
        assert np.array_equal(p.sim_log_source()[0], np.where(sel["choice"] >= 0, 3, got["u_source"])) and np.all(p.sim_log_source()[0][sel["choice"] >= 0] == 3)
        assert np.array_equal(p.sim_log_pick()[0], sel["choice"]) and np.array_equal(got["pick"], sel["choice"])
        p.forecast_from_profiles(None, 1)                                       # completes the step: the memory stays
        p.solve_resident()
        assert np.array_equal(p.plan_memory_state()["age"], st["age"])
        # the route the README had: u0 down and up again, the NaN rows patched on the host
        u0 = np.where(np.isnan(r["out"]["u0"]), 0.0, r["out"]["u0"])
        q.sim_step(resolve=t.R, u0=u0)
        assert np.all(q.plan_memory_state()["age"] == -1)                       # emptied
        assert np.array_equal(q.policy_state(), r["up"])                        # stale
        assert np.all(q.sim_log_source() == -2) and np.all(q.sim_log_pick() == -2)
    finally:
        _clean(p, q)


def test_short_sequences_are_not_remembered(ctx):
    """K = 2 < N_tilde: nothing is remembered, the ages move on"""
    c = ctx(BATCHES[0])
    p, B = c.p, c.B
    P = thermostat(c)
    try:
        _begin(c, (p,), P, 0, N + 4)
        s = _one_step_setup(c, p, P, K=2, seed=9600)
        sel = p.selection()
        assert sel["K"] == 2 and sel["u"].shape == (B, 2, c.nu) and ((sel["choice"] >= 0) & (sel["policy"] < 0)).sum() >= B // 8
        got = p.sim_step(resolve=c.R, selected=True, fallback=BOTH, log=False, outputs=True)
        mem, age = fallback.commit_selected_np(got["u_source"], sel["policy"], sel["u"], s["mem_u"], s["mem_age"], N)
        st = p.plan_memory_state()
        assert np.array_equal(st["u"], s["mem_u"]) and np.array_equal(st["u"], mem) and np.array_equal(st["age"], age)
        assert np.array_equal(age, np.where(s["mem_age"] >= 1, np.minimum(s["mem_age"] + 1, N), -1)) and not np.any(age == 1)
        assert np.array_equal(got["v0"][sel["choice"] >= 0, :c.nu], sel["u"][sel["choice"] >= 0, 0])
    finally:
        _clean(p)


def test_a_what_if_changes_nothing(ctx):
    c = ctx(BATCHES[0])
    p = c.p
    P = thermostat(c)
    try:
        _begin(c, (p,), P, 2, N + 4)
        s = _one_step_setup(c, p, P, seed=9700)
        x_in, w_in = p.inputs()
        sel = p.selection()
        first = p.sim_step(resolve=c.R, selected=True, fallback=BOTH, advance=False, log=False, outputs=True)
        st = p.plan_memory_state()
        assert np.array_equal(st["u"], s["mem_u"]) and np.array_equal(st["age"], s["mem_age"]) and np.array_equal(p.policy_state(), s["up"])
        assert p.sim_log_count() == (0, 2) and np.array_equal(p.inputs()[0], x_in) and np.array_equal(p.inputs()[1], w_in)
        again = p.selection()
        assert again["valid"] and again["K"] == sel["K"]
        _equal(again, sel, SEL_KEYS, "the selection")
        second = p.sim_step(resolve=c.R, selected=True, fallback=BOTH, advance=False, log=False, outputs=True)
        _equal(second, first, STEP_OUT + ("u_source", "pick"), "the second what-if")
        took = p.sim_step(resolve=c.R, selected=True, fallback=BOTH, advance=True, log=False, outputs=True)
        _equal(took, first, STEP_OUT + ("u_source", "pick"), "the step against its what-if")
        assert not p.selection()["valid"] and np.array_equal(p.inputs()[0], took["x_k1"])
    finally:
        _clean(p)


OUT_KEYS = ("choice", "score", "n_admissible", "admissible", "u", "u0")


@pytest.mark.parametrize("B", BATCHES)
def test_keep_leaves_the_select_call_as_it_was(ctx, B):
    """keep=True against keep=False bit for bit, and selection() against what the call returned: select_plan, select_plan_policies, complete="device", and a
    host completion forced by MLD_DBG_SMALL_PIVOT_CAP on the resolver"""
    c = ctx(B)
    p = c.p
    P = thermostat(c)
    om_seq, cand, cw = _scenario(c, N, 9800 + B)
    try:
        _begin(c, (p,), P, 0, N + 4)
        _solve_cut((p,), B, [b for b in range(B) if b % 5 == 0])
        bound = _bound(p, c, P, N, om_seq, cand, cw)
        sel = _selector(bound)
        plain = dict(candidates=cand, plan_first=True, K=N, omega_seq=om_seq, cost_w=cw, per_candidate=True, per_trajectory=True)
        for what, fn, kw in (("select_plan", p.select_plan, plain), ("select_plan_policies", p.select_plan_policies, dict(plain, policies=[P])),
                             ("select_plan device", p.select_plan, dict(plain, complete="device")),
                             ("select_plan_policies device", p.select_plan_policies, dict(plain, policies=[P], complete="device"))):
            off = fn(c.R, sel, **kw)
            with pytest.raises(gpu.MldGpuError, match="no kept selection"):
                p.selection()                                                   # keep=False: nothing is allocated
            on = fn(c.R, sel, keep=True, **kw)
            _equal(on, off, OUT_KEYS + ("cost", "end_status") + (("policy",) if "policies" in kw else ()), what)
            for k in off["risk"]:
                if k not in ("names", "levels"):
                    assert np.array_equal(on["risk"][k], off["risk"][k], equal_nan=True), (what, k)
            assert on["stats"] == off["stats"], what
            kept = p.selection()
            assert kept["valid"] and kept["K"] == N, what
            _equal(kept, dict(on, policy=on.get("policy", np.full(B, -1, np.int32))), SEL_KEYS, what + " selection()")
            assert (kept["choice"] >= 0).any() and (kept["choice"] < 0).any(), what
            if "policies" in kw:
                assert (kept["policy"] >= 0).any() and np.all(np.isnan(kept["u"][kept["policy"] >= 0, 1:])), what
        # the host completion: the LDS solver declines, select_plan finishes the instances on the host, and the device holds what it returned
        plain = dict(plain, plan_first=False, candidates=np.concatenate([cand, _scenario(c, N, 9850 + B)[1]], axis=1))
        c.R.problem.set_opts(reserved=_lib.MLD_DBG_SMALL_PIVOT_CAP)
        try:
            off = p.select_plan(c.R, sel, **plain)
            on = p.select_plan(c.R, sel, keep=True, **plain)
        finally:
            c.R.problem.set_opts(reserved=0)
        assert on["stats"]["finished_on_host"] > 0 and on["stats"] == off["stats"]
        _equal(on, off, OUT_KEYS + ("cost", "end_status"), "host completion")
        kept = p.selection()
        assert kept["valid"] and (kept["choice"] >= 0).any()
        _equal(kept, dict(on, policy=np.full(B, -1, np.int32)), SEL_KEYS, "host completion selection()")
    finally:
        _clean(p)


def test_set_selection_round_trip_steps_like_a_kept_one(ctx):
    c, t = ctx(BATCHES[0]), ctx(BATCHES[0], twin=True)
    p, q, B = c.p, t.p, c.B
    P = thermostat(c)
    try:
        _begin(c, (p, q), P, 1, N + 4)
        q.upload_policy(P)
        q.plan_memory()
        s = _one_step_setup(c, p, P, seed=9900)
        sel = p.selection()
        q.plan_memory_state(u=s["mem_u"], age=s["mem_age"])
        q.policy_state(u_prev=s["up"])
        q.set_selection(sel["choice"], sel["u"], policy=sel["policy"])           # NaN rows of "no choice" and behind a policy pick included
        back = q.selection()
        assert back["valid"] and back["K"] == N
        _equal(back, sel, SEL_KEYS, "round trip")
        got = p.sim_step(resolve=c.R, selected=True, fallback=BOTH, outputs=True)
        ref = q.sim_step(resolve=t.R, selected=True, fallback=BOTH, outputs=True)
        _equal(got, ref, STEP_OUT + ("u_source", "pick"), "a caller's selection")
        a, b = p.plan_memory_state(), q.plan_memory_state()
        assert np.array_equal(a["u"], b["u"]) and np.array_equal(a["age"], b["age"]) and np.array_equal(p.policy_state(), q.policy_state())
        assert np.array_equal(p.sim_log_pick(), q.sim_log_pick()) and np.array_equal(p.sim_log_source(), q.sim_log_source())
        # policy=None: every pick a sequence
        q.set_selection(np.zeros(B, np.int64), np.ones((B, 1, c.nu)))
        back = q.selection()
        assert back["K"] == 1 and np.all(back["policy"] == -1) and np.all(back["choice"] == 0) and back["valid"]
    finally:
        _clean(p, q)


def test_validity(ctx):
    c = ctx(BATCHES[0])
    p, B = c.p, c.B
    P = thermostat(c)
    stale = "the kept selection is stale"
    try:
        _begin(c, (p,), P, 0, N + 4)
        s = _one_step_setup(c, p, P, seed=10000)
        sel = p.selection()

        def again():
            p.set_selection(sel["choice"], sel["u"], policy=sel["policy"])
            assert p.selection()["valid"]

        def ended(match):
            assert not p.selection()["valid"]
            with pytest.raises(gpu.MldGpuError, match=match):
                p.sim_step(resolve=c.R, selected=True, fallback=BOTH, log=False)

        # what keeps it: a new forecast, a solve, a new cost
        p.forecast_from_profiles(None, 0)
        assert p.selection()["valid"]
        p.solve_resident()
        assert p.selection()["valid"]
        p.upload_instance_cost(lin_v=np.zeros((B, p.n)))
        assert p.selection()["valid"]
        p.upload_instance_cost()
        assert p.sim_step(resolve=c.R, selected=True, fallback=BOTH, advance=False, log=False) == 0
        # a failing select call leaves the previous one
        om4, cand4, cw4 = _scenario(c, N + 1, 10010)
        with pytest.raises(gpu.MldGpuError, match="N_tilde"):                   # the plan is shorter than the rollout
            _select(p, c, P, _selector(s["bound"]), N + 1, om4, cand4, cw4, keep=True)
        kept = p.selection()
        assert kept["valid"]
        _equal(kept, sel, SEL_KEYS, "after a failing select call")
        # what ends it
        p.advance()
        ended(stale + ".*the inputs moved")
        p.solve_resident(); again()
        p.sim_step(resolve=c.R, log=False)
        ended(stale + ".*the inputs moved")
        p.solve_resident(); again()
        p.sim_step(log=False)
        ended(stale + ".*the inputs moved")
        p.solve_resident(); again()
        p.sim_step(resolve=c.R, fallback=BOTH, log=False)
        ended(stale + ".*the inputs moved")
        again()
        p.sim_step(resolve=c.R, selected=True, fallback=BOTH, log=False)
        ended(stale + ".*the inputs moved")
        again()
        p.sim_step(resolve=c.R, policy=True, log=False)
        ended(stale + ".*the inputs moved")
        p.stage(c.x0[None], c.om[None])
        again()
        p.select(0)
        ended(stale + ".*the inputs moved")
        again()
        p.upload(c.x0, c.om, c.midx)
        assert not p.selection()["valid"] and p.selection()["choice"] is None
        with pytest.raises(gpu.MldGpuError, match=stale + ".*a batch has been uploaded"):
            p.sim_step(resolve=c.R, selected=True, log=False)
        again()                                                                 # ... and a new one can be set for the new batch
    finally:
        _clean(p)


def test_refusals_change_nothing(ctx):
    c = ctx(BATCHES[0])
    p, R, B, nu = c.p, c.R, c.B, c.nu
    P = thermostat(c)
    state = {}

    def snapshot():
        state["x"], state["w"] = p.inputs()
        state["count"] = p.sim_log_count()
        state["mem"], state["up"] = p.plan_memory_state(), p.policy_state()
        state["sel"] = p.selection()

    def unchanged(what):
        x, w = p.inputs()
        assert np.array_equal(x, state["x"]) and np.array_equal(w, state["w"]) and p.sim_log_count() == state["count"], what
        st = p.plan_memory_state()
        assert np.array_equal(st["u"], state["mem"]["u"]) and np.array_equal(st["age"], state["mem"]["age"]) and np.array_equal(p.policy_state(), state["up"]), what
        now = p.selection()
        assert now["valid"] == state["sel"]["valid"], what
        _equal(now, state["sel"], SEL_KEYS, what)

    def refused(match, **kw):
        with pytest.raises(gpu.MldGpuError, match=match):
            p.sim_step(resolve=kw.pop("resolve", R), selected=True, **kw)
        unchanged(match)

    for bad in (dict(), dict(resolve=R, u0=np.zeros(nu)), dict(resolve=R, policy=True), dict(resolve=R, v0=np.zeros(c.nv))):
        with pytest.raises(ValueError, match="selected=True goes with resolve alone"):
            p.sim_step(selected=True, **bad)
    try:
        p.upload(c.x0, c.om, c.midx)
        p.sim_log_begin(1)
        with pytest.raises(gpu.MldGpuError, match="mld_sim_step_selected: no kept selection"):
            p.sim_step(resolve=R, selected=True)
        with pytest.raises(gpu.MldGpuError, match="no kept selection"):
            p.selection()
        choice, u = np.zeros(B, np.int32), np.ones((B, N, nu))
        # mld_set_selection's refusals, the instance named
        with pytest.raises(ValueError, match="choice has shape"):
            p.set_selection(choice[:-1], u)
        with pytest.raises(ValueError, match="u has shape"):
            p.set_selection(choice, u[:, :, :-1])
        with pytest.raises(ValueError, match="policy has shape"):
            p.set_selection(choice, u, policy=np.zeros(B))
        with pytest.raises(gpu.MldGpuError, match="K = 0"):
            p.set_selection(choice, u[:, :0])
        for arr, i, val, match in ((choice, 5, -2, "choice of instance 5 is -2"),):
            bad = arr.copy(); bad[i] = val
            with pytest.raises(gpu.MldGpuError, match=match):
                p.set_selection(bad, u)
        pol = np.full(B, -1, np.int32); pol[7] = -2
        with pytest.raises(gpu.MldGpuError, match="policy of instance 7 is -2"):
            p.set_selection(choice, u, policy=pol)
        none = choice.copy(); none[4] = -1
        pol = np.full(B, -1, np.int32); pol[4] = 0
        with pytest.raises(gpu.MldGpuError, match="policy of instance 4 is 0, but its choice is -1"):
            p.set_selection(none, u, policy=pol)
        nan0 = u.copy(); nan0[3, 0, 1] = np.nan
        with pytest.raises(gpu.MldGpuError, match="u of instance 3, step 0, input 1 is not finite"):
            p.set_selection(choice, nan0, policy=np.zeros(B, np.int32))         # row 0 is read for a policy pick too
        nan2 = u.copy(); nan2[6, 2, 0] = np.nan
        with pytest.raises(gpu.MldGpuError, match="u of instance 6, step 2, input 0 is not finite"):
            p.set_selection(choice, nan2)
        p.set_selection(choice, nan2, policy=np.zeros(B, np.int32))             # ... behind a policy pick's row 0 it is not
        none = choice.copy(); none[6] = -1
        p.set_selection(none, nan2)                                             # ... and nothing of an instance without a choice
        # the step's refusals
        p.upload_policy(P)
        p.plan_memory()
        p.plan_memory_state(u=np.zeros((B, N, nu)), age=np.full(B, 1, np.int32))
        snapshot()
        refused("unknown fallback bits", fallback=4, advance=False)
        p.solve_resident()
        with pytest.raises(gpu.MldGpuError, match="mld_sim_step_fallback: unknown fallback bits"):
            p.sim_step(resolve=R, fallback=4, advance=False)                    # mld_sim_step_fallback still refuses the bit
        snapshot()
        refused("step = -1", fallback=BOTH, step=-1)
        refused("no profile library", fallback=BOTH, actual=True)
        mats7, d7, _ = syn.make_agent(7, np.random.default_rng(10200), tie=True)
        other = BatchAuxResolver([mats7] * 3, d7, small_lds=True)                # a resolver over other models
        try:
            refused("not the fold", resolve=other, fallback=BOTH)
        finally:
            other.close()
        p.plan_memory(False)
        state["mem"] = None
        with pytest.raises(gpu.MldGpuError, match="MLD_FB_MEMORY, but no plan memory is enabled"):
            p.sim_step(resolve=R, selected=True, fallback=("memory",))
        p.plan_memory()
        p.upload_policy(thermostat(c, mode=[0] + [1] * (nu - 1)))
        with pytest.raises(gpu.MldGpuError, match="passes a channel through"):
            p.sim_step(resolve=R, selected=True, fallback=("policy",))
        p.upload_policy(None)
        with pytest.raises(gpu.MldGpuError, match="MLD_FB_POLICY, but no policy uploaded"):
            p.sim_step(resolve=R, selected=True, fallback=("policy",))
        assert p.selection()["valid"]
        last = p.sim_step(resolve=R, selected=True, advance=False, log=True, outputs=True)
        assert np.array_equal(last["u_source"], np.where(none < 0, -1, 3)) and last["aux_status"][6] == -1 and last["n_skipped"] >= 1      # no choice, no source
        with pytest.raises(gpu.MldGpuError, match="log is full"):
            p.sim_step(resolve=R, selected=True, log=True)
        assert p.selection()["valid"] and np.array_equal(p.sim_log_pick()[0], none) and p.sim_log_source()[0, 6] == -1
    finally:
        _clean(p)


@pytest.mark.parametrize("B", BATCHES[:1])
def test_a_handle_that_never_keeps_is_as_before(ctx, B):
    """one full select plus fallback step on a handle that never set keep, against the same on one that keeps (and never applies the selection): the select
    call's results, the step's outputs, the memory, the policy state and the log are the same bits, and nothing was allocated on the first"""
    c, t = ctx(B), ctx(B, twin=True)
    p, q = c.p, t.p
    P = thermostat(c)
    try:
        _begin(c, (p, q), P, 1, N + 4)
        q.upload_policy(P)
        q.plan_memory()
        s = _one_step_setup(c, p, P, seed=10100, keep=False)
        r = _one_step_setup(t, q, P, seed=10100, keep=True)
        _equal(s["out"], r["out"], OUT_KEYS + ("policy",), "select")
        assert s["out"]["stats"] == r["out"]["stats"]
        with pytest.raises(gpu.MldGpuError, match="no kept selection"):
            p.selection()
        got = p.sim_step(resolve=c.R, fallback=BOTH, outputs=True)
        ref = q.sim_step(resolve=t.R, fallback=BOTH, outputs=True)
        _equal(got, ref, STEP_OUT + ("u_source",), "fallback step")
        assert set(np.unique(got["u_source"])) == {0, 1, 2} and "pick" not in got
        a, b = p.plan_memory_state(), q.plan_memory_state()
        assert np.array_equal(a["u"], b["u"]) and np.array_equal(a["age"], b["age"]) and np.array_equal(p.policy_state(), q.policy_state())
        la, lb = p.sim_log(), q.sim_log()
        _equal(la, lb, list(la), "log")
        assert np.array_equal(p.sim_log_source(), q.sim_log_source()) and np.all(p.sim_log_pick() == -2) and np.all(q.sim_log_pick() == -2)
        with pytest.raises(gpu.MldGpuError, match="already been applied"):
            p.sim_step(resolve=c.R, fallback=BOTH, log=False)                   # the handle ends `advanced`, as ever
    finally:
        _clean(p, q)
