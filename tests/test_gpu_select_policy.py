"""Plan selection with closed-loop rule policies among the candidates (mld_rollout_select_policy / GpuProblem.select_plan_policies(policies=...); kernels
k_rollout_cand_policy / k_rollout_cand_policy_kpi, k_rollout_risk, k_plan_select, k_select_inputs): the plan, n_own open-loop sequences and T thermostats per
instance rolled out under the same S realisations in one launch.  Every comparison is bit for bit, NaN equal to NaN: a policy candidate against
upload_policy(P_t) followed by rollout(policy=True, u_prev=..., kpis=..., risk=...) on the same handle -- the two routes share ro_run<true> and the same
inputs, so there is no guard and no tolerance --, a sequence or plan candidate against rollout(u_seq=...) / rollout(K=K) with switches 0, the choice against
simlog.select_plan_np on the per-candidate risk of the same call, the chosen step 0 against policy.apply_np.

Shapes (tests/test_gpu_sim_resolve.py): a10 -- n_h 3, three models interleaved, batch 10; a1 -- batch 1; b9 -- n_h 7, batch 9.  K = 3, STEP = 1."""
import ctypes as C

import numpy as np
import pytest

import _rollout_ref
from test_gpu_sim_resolve import SHAPES
from test_gpu_small_lds_step import _SmallCtx
from test_gpu_log_summary import _kpis
from test_gpu_rollout_kpi import N_CHAN, _tariff
from test_gpu_policy_rollout import thermostat
from test_gpu_plan_select import _scenario, _table, _constraints, _clean, _plan_u, LEVELS
from pyhybridcontrol_amd import policy, simlog, _lib
from pyhybridcontrol_amd._lib import MldGpuError
from pyhybridcontrol_amd.simlog import PlanSelector, RiskTable

pytestmark = pytest.mark.gpu

K, STEP = 3, 1
SUMM = ("cost", "mu_total", "worst_vio", "worst_step", "steps_done", "end_status")
RISK = simlog.RISK_COL_KEYS + simlog.RISK_LEVEL_KEYS + simlog.RISK_COUNTS
PICK = ("choice", "score", "n_admissible", "admissible", "u", "u0", "policy")
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


def _same(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, (what, a.dtype, b.dtype, a.shape, b.shape)
    ok = ((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))) if a.dtype.kind == "f" else a == b
    assert np.all(ok), (what, int((~ok).sum()), a[~ok][:4], b[~ok][:4])


def _bands(c, T):
    """T thermostats over a context's models, thresholds on the half-integer grid, every band another one"""
    return [thermostat(c, 54.5 + (t % 8), 55.5 + (t % 8) + (t // 8)) for t in range(T)]


def _with_switches(kpis):
    """tests/test_gpu_plan_select.py's columns and, behind them, the switch count"""
    return _table(kpis).add("sw", "switches", level=0.0)


def _u_prev(c, seed):
    return (np.random.default_rng(seed).uniform(size=(c.B, c.nu)) < 0.5).astype(float)


def _policy_u0(c, pols, up, x0=None):
    """the rules' step-0 inputs (B, T, nu): policy.apply_np on the uploaded x0 and u_prev"""
    return np.stack([policy.apply_np(P, c.midx, c.x0 if x0 is None else x0, up) for P in pols], axis=1)


def _check_pick(c, got, sel, mc, seqs, pols, up, what, x0=None):
    """the choice, the policy index and the chosen inputs against the numpy rule on the call's own risk, and the chosen input's convention on its own"""
    T = len(pols)
    seqs = np.zeros((c.B, 0, K, c.nu)) if seqs is None else seqs      # (the policies alone: the empty array carries K)
    want = simlog.select_plan_np(got["risk"], sel, mc, candidates=seqs, policy_u0=_policy_u0(c, pols, up, x0))
    for k in PICK:
        _same(got[k], want[k], what + (k,))
    P = got["admissible"].shape[1]
    for b in range(c.B):
        ch = got["choice"][b]
        if ch < 0:
            assert got["policy"][b] == -1 and np.all(np.isnan(got["u"][b])) and np.all(np.isnan(got["u0"][b])), what + (b,)
        elif ch >= P - T:
            t = ch - (P - T)
            assert got["policy"][b] == t, what + (b,)
            u0 = policy.apply_np(pols[t], c.midx[b:b + 1], (c.x0 if x0 is None else x0)[b:b + 1], up[b:b + 1])[0]
            assert np.array_equal(got["u0"][b], u0) and np.array_equal(got["u"][b, 0], u0) and np.all(np.isnan(got["u"][b, 1:])), what + (b,)
        else:
            assert got["policy"][b] == -1 and np.array_equal(got["u"][b], seqs[b, ch]) and np.array_equal(got["u0"][b], seqs[b, ch, 0]), what + (b,)


def _sw_risk(kpis, es):
    """the switches column of a plan or sequence candidate: rollout_risk_np on switches = 0 (-1 where the trajectory did not end 0)"""
    r = RiskTable(kpis, LEVELS).add("sw", "switches", level=0.0)
    return simlog.rollout_risk_np(dict(end_status=es, switches=np.where(es == 0, 0, -1).astype(np.int32)), r, policy=True)


def _against_open_loop(got, p, ref, kpis, what):
    """candidate p of `got` is `ref`, a rollout(u_seq=... / K=K, kpis=..., risk=<the table without the switch column>)"""
    for k in SUMM:
        _same(got[k][:, p], ref[k], what + (p, k))
    _same(got["switches"][:, p], np.where(ref["end_status"] == 0, 0, -1).astype(np.int32), what + (p, "switches"))
    if kpis is not None:
        for k in simlog.KPI_ROLLOUT_KEYS:
            _same(got["kpi"][k][:, p], ref["kpi"][k], what + (p, "kpi", k))
    sw = _sw_risk(kpis, ref["end_status"])
    for k in simlog.RISK_COL_KEYS + simlog.RISK_LEVEL_KEYS:
        _same(got["risk"][k][:, p, :-1], ref["risk"][k], what + (p, "risk", k))
        _same(got["risk"][k][:, p, -1:], sw[k], what + (p, "risk of switches = 0", k))
    for k in simlog.RISK_COUNTS:
        _same(got["risk"][k][:, p], ref["risk"][k], what + (p, "risk", k))


def _against_closed_loop(got, p, ref, kpis, what):
    """candidate p of `got` is `ref`, a rollout(policy=True, u_prev=..., kpis=..., risk=<the whole table>) of the same policy uploaded"""
    for k in SUMM + ("switches",):
        _same(got[k][:, p], ref[k], what + (p, k))
    if kpis is not None:
        for k in simlog.KPI_ROLLOUT_KEYS:
            _same(got["kpi"][k][:, p], ref["kpi"][k], what + (p, "kpi", k))
    for k in RISK:
        _same(got["risk"][k][:, p], ref["risk"][k], what + (p, "risk", k))


@pytest.mark.parametrize("case", [(0, 1, 1), (1, 1, 1), (2, 2, 3), (62, 2, 2), (0, 64, 2), (1, 2, 64)])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_per_candidate_against_the_existing_entries(ctx, shape, case):
    """without KPIs, with them, and with priced ones whose price start differs per instance; plan_first off and on.  The references are taken on the handle
    first, the policy is removed, then select_plan runs."""
    n_own, T, S = case
    c = ctx(shape)
    p = c.p
    pols = _bands(c, T)
    up = _u_prev(c, 9801)
    try:
        p.upload(c.x0, c.om, c.midx)
        p.solve_resident()
        plib, pstart = _tariff(c.B, K, 9805)
        om_seq, cand, cw = _scenario(c, max(n_own, 1), S, 9810 + 10 * n_own + S)
        cand = np.ascontiguousarray(cand[:, :n_own])
        for with_kpis in (False, True, "priced"):
            kpis = _kpis(c, 9800, priced=with_kpis == "priced") if with_kpis else None
            p.upload_prices(plib, N_CHAN) if with_kpis == "priced" else p.upload_prices(np.zeros(0))
            risk, open_risk = _with_switches(kpis), _table(kpis)
            sel = PlanSelector(risk).minimise("cost", "mean")
            kw = dict(omega_seq=om_seq, step=STEP, cost_w=cw, kpis=kpis, price_start=pstart if with_kpis == "priced" else None)
            ref_seq = [p.rollout(c.R, u_seq=np.ascontiguousarray(cand[:, i]), risk=open_risk, **kw) for i in range(n_own)]
            ref_plan = p.rollout(c.R, K=K, risk=open_risk, **kw) if K <= c.N else None
            ref_pol = []
            for P_t in pols:
                p.upload_policy(P_t)
                ref_pol.append(p.rollout(c.R, K=K, policy=True, u_prev=up, risk=risk, **kw))
            p.upload_policy(None)
            for plan_first in (False, True):
                what = (shape, case, with_kpis, plan_first)
                args = dict(candidates=cand if n_own else None, plan_first=plan_first, K=K, policies=pols, u_prev=up, per_candidate=True, per_trajectory=True)
                no, nt = n_own, T
                if plan_first and 1 + n_own + T > simlog.SELECT_P_MAX:      # one candidate too many: refused, and the case goes on with one fewer
                    with pytest.raises(ValueError, match="1 .. 64"):
                        p.select_plan_policies(c.R, sel, **dict(kw, **args))
                    no, nt = (n_own - 1, T) if n_own else (0, T - 1)
                    args.update(candidates=np.ascontiguousarray(cand[:, :no]) if no else None, policies=pols[:nt])
                if plan_first and K > c.N:      # the plan is shorter than the rollout: refused as rollout(u_seq=None) refuses it
                    with pytest.raises(MldGpuError, match="N_tilde"):
                        p.select_plan_policies(c.R, sel, **dict(kw, **args))
                    continue
                pf = 1 if plan_first else 0
                P = pf + no + nt
                got = p.select_plan_policies(c.R, sel, **dict(kw, **args))
                assert got["stats"]["finished_on_host"] == 0 and got["stats"]["trajectories"] == c.B * P * S and got["switches"].shape == (c.B, P, S), what
                assert np.all(got["end_status"] == 0), what      # the comparison cannot pass on NaN alone
                if plan_first:
                    _against_open_loop(got, 0, ref_plan, kpis, what)
                for i in range(no):
                    _against_open_loop(got, pf + i, ref_seq[i], kpis, what)
                for t in range(nt):
                    _against_closed_loop(got, pf + no + t, ref_pol[t], kpis, what)
                assert np.all(got["switches"][:, :pf + no] == 0) and np.all(got["switches"][:, pf + no:] >= 0), what
                seqs = np.concatenate(([_plan_u(c)[:, None]] if plan_first else []) + [cand[:, :no]], axis=1)
                _check_pick(c, got, sel, S, seqs, pols[:nt], up, what)
                if with_kpis == "priced" and c.B > 1:
                    q = kpis.names.index("priced")
                    assert len(set(pstart.tolist())) > 1 and np.any(got["kpi"]["sum"][:, :, :, q] != 0.0), what
        assert any(np.any(r["switches"] > 0) for r in ref_pol)      # the rules do switch
    finally:
        _clean(p)


def test_closed_loop_equals_open_loop_where_they_must(ctx):
    """S = 1: the thermostat's realised u as a sequence candidate beside the thermostat -- every per-trajectory figure and KPI identical in every bit except
    switches, the choice the sequence (the smaller p) on the exact tie; two identical tables: the first wins"""
    c = ctx("a10")
    p = c.p
    P_t = thermostat(c)
    up = _u_prev(c, 9820)
    kpis = _kpis(c, 9821, priced=False)
    risk = _with_switches(kpis)
    om_seq, _, cw = _scenario(c, 1, 1, 9822)
    kw = dict(omega_seq=om_seq, step=STEP, cost_w=cw, kpis=kpis)
    try:
        p.upload(c.x0, c.om, c.midx)
        p.upload_policy(P_t)
        ref = p.rollout(c.R, K=K, policy=True, u_prev=up, trajectories=True, **kw)
        p.upload_policy(None)
        assert np.all(ref["end_status"] == 0) and np.any(ref["switches"] > 0)
        realised = np.ascontiguousarray(ref["v"][:, 0, :, :c.nu])[:, None]
        for obj in ("cost", "mu", "y_sum"):
            sel = PlanSelector(risk).minimise(obj, "mean")
            got = p.select_plan_policies(c.R, sel, candidates=realised, policies=[P_t], u_prev=up, per_candidate=True, per_trajectory=True, **kw)
            assert np.all(got["end_status"] == 0)
            for k in SUMM:
                _same(got[k][:, 0], got[k][:, 1], (obj, k))
                _same(got[k][:, 1], ref[k], (obj, k, "the rollout"))
            for k in simlog.KPI_ROLLOUT_KEYS:
                _same(got["kpi"][k][:, 0], got["kpi"][k][:, 1], (obj, "kpi", k))
            for k in simlog.RISK_COL_KEYS + simlog.RISK_LEVEL_KEYS:
                _same(got["risk"][k][:, 0, :-1], got["risk"][k][:, 1, :-1], (obj, "risk", k))
            assert np.all(got["switches"][:, 0] == 0) and np.array_equal(got["switches"][:, 1], ref["switches"])
            assert np.all(got["choice"] == 0) and np.all(got["policy"] == -1) and np.all(got["n_admissible"] == 2), obj
            _same(got["u"], realised[:, 0], (obj, "u"))
        sel = PlanSelector(risk).minimise("cost", "mean")
        two = p.select_plan_policies(c.R, sel, policies=[P_t, thermostat(c)], u_prev=up, K=K, per_candidate=True, **kw)
        for k in RISK:
            _same(two["risk"][k][:, 0], two["risk"][k][:, 1], ("twins", k))
        assert np.all(two["choice"] == 0) and np.all(two["policy"] == 0) and np.all(two["n_admissible"] == 2)
        _check_pick(c, two, sel, 1, None, [P_t, P_t], up, ("twins",))
    finally:
        _clean(p)


def test_the_choice_against_the_rule(ctx):
    """every kind of statistic as the objective, with 0, 1 and 8 constraints whose bounds are medians of the call's own statistics, a constraint on the
    switches column, and the policies permuted"""
    c = ctx("a10")
    p, S = c.p, 5
    kpis = _kpis(c, 9830, priced=False)
    risk = _with_switches(kpis)
    om_seq, cand, cw = _scenario(c, 2, S, 9831)
    pols = [thermostat(c, 57.5, 60.5), thermostat(c, 59.5, 60.5), thermostat(c, 55.5, 63.5)]
    up = _u_prev(c, 9832)
    kw = dict(candidates=cand, policies=pols, u_prev=up, omega_seq=om_seq, step=STEP, cost_w=cw, kpis=kpis, per_candidate=True)
    seen = dict(none=0, seq=0, pol=0)
    try:
        p.upload(c.x0, c.om, c.midx)
        base = p.select_plan_policies(c.R, PlanSelector(risk).minimise("cost", "mean"), **kw)["risk"]
        assert np.all(base["n_complete"] == S)
        for j, kind in enumerate(simlog.SELECT_KINDS):
            for n_cons in (0, 1, 8):
                lvl = dict(level=LEVELS[j % 3]) if j >= 4 else {}
                sel = _constraints(PlanSelector(risk).minimise(risk.names[j % len(risk)], kind, **lvl), risk, base, n_cons)
                for mc in (S, 1):
                    got = p.select_plan_policies(c.R, sel, min_complete=mc, **kw)
                    for k in RISK:
                        _same(got["risk"][k], base[k], (kind, n_cons, mc, "risk", k))
                    _check_pick(c, got, sel, mc, cand, pols, up, (kind, n_cons, mc))
                    seen["none"] += int((got["choice"] < 0).sum()); seen["seq"] += int(((got["choice"] >= 0) & (got["policy"] < 0)).sum()); seen["pol"] += int((got["policy"] >= 0).sum())
        # a constraint on the switch count: the sequences (0 switches) always pass it, a policy only where it switches rarely
        sw = base["mean"][:, :, -1]
        assert np.all(sw[:, :2] == 0.0) and np.any(sw[:, 2:] > 0.0)
        bound = float(np.median(sw[:, 2:]))
        sel = PlanSelector(risk).minimise("mu", "mean").subject_to("sw", "mean", bound)
        got = p.select_plan_policies(c.R, sel, **kw)
        assert np.array_equal(got["admissible"], sw <= bound) and got["admissible"][:, :2].all() and not got["admissible"][:, 2:].all() and got["admissible"][:, 2:].any()
        _check_pick(c, got, sel, S, cand, pols, up, ("switches bound",))
        tight = PlanSelector(risk).minimise("mu", "mean").subject_to("sw", "mean", float(np.median(sw[:, 2:].min(axis=1))))
        only = p.select_plan_policies(c.R, tight, **dict(kw, candidates=None, K=K))      # the policies alone: the bound decides, also that nobody is chosen
        assert np.array_equal(only["admissible"], sw[:, 2:] <= tight.constraints[0][3]) and np.array_equal(only["choice"] < 0, ~only["admissible"].any(axis=1))
        _check_pick(c, only, tight, S, None, pols, up, ("switches bound, policies alone",))
        # the policies permuted: the risk is permuted with them, and the choice wherever the least value is attained once
        perm = np.array([2, 0, 1])
        s2 = PlanSelector(risk).minimise("cost", "mean")
        a, b = p.select_plan_policies(c.R, s2, **kw), p.select_plan_policies(c.R, s2, **dict(kw, policies=[pols[i] for i in perm]))
        at = np.concatenate([[0, 1], 2 + perm])
        for k in RISK:
            _same(b["risk"][k], a["risk"][k][:, at], ("permuted", k))
        v = a["risk"]["mean"][:, :, 0]
        once = (v == v.min(axis=1, keepdims=True)).sum(axis=1) == 1
        assert once.any() and np.array_equal(at[b["choice"][once]], a["choice"][once])
        _check_pick(c, b, s2, S, cand, [pols[i] for i in perm], up, ("permuted",))
        print("choices over all calls:", seen)
        assert seen["none"] > 0 and seen["seq"] > 0 and seen["pol"] > 0, "the inputs no longer exercise the rule: %s" % (seen,)
    finally:
        _clean(p)


def test_the_filter_filters(ctx):
    """the safety filter: an "all off" sequence is cheapest, but for the instances whose tanks start cold it violates mu_total max <= bound, and the thermostat
    wins there; for the others it is admissible and wins.  The inputs are chosen on the CPU (simlog.rollout_np with the closed form as resolver) so that both
    outcomes occur -- a condition on the inputs, not a tolerance.  Two bands, narrow and wide, differ in their mean switch count."""
    c = ctx("a10")
    p, S = c.p, 3
    om_seq, _, _ = _scenario(c, 1, S, 9850)
    x0 = c.x0.copy()
    x0[::2] -= 5.0                                                          # every other instance starts five degrees colder
    off = np.zeros((c.B, 1, K, c.nu))
    wide, narrow = thermostat(c, 57.5, 60.5), thermostat(c, 59.5, 60.5)
    up = np.zeros((c.B, c.nu))
    fn = _rollout_ref.closed_form_resolver(c.mats, c.d)
    num_off = simlog.rollout_np(c.mats, c.d, c.midx, x0, off[:, 0], om_seq, fn)
    num = [simlog.rollout_np(c.mats, c.d, c.midx, x0, off[:, 0], om_seq, fn, policy=P, u_prev=up) for P in (wide, narrow)]
    assert all(np.all(r["end_status"] == 0) for r in [num_off] + num)
    mu_off, mu_th = num_off["mu_total"].max(axis=1), np.maximum(num[0]["mu_total"].max(axis=1), num[1]["mu_total"].max(axis=1))
    cold = mu_off > 0.0
    assert cold.any() and (~cold).any()
    bound = 0.5 * float(mu_off[cold].min())
    assert np.all(mu_th[cold] <= 0.5 * bound) and np.all(mu_off[cold] >= 2.0 * bound) and np.all(mu_off[~cold] == 0.0)      # far from the bound on both sides
    heats = np.array([np.any(r["v"][..., :c.nu] == 1.0, axis=(1, 2, 3)) for r in num])
    assert np.all(heats[:, cold])                                           # a thermostat that heats costs more than "all off"
    assert num[0]["switches"].mean() != num[1]["switches"].mean()
    cw = np.zeros((K, c.nv))
    cw[:, :c.nu] = 1.0                                                      # the cost: the steps heated
    risk = RiskTable(None, LEVELS).add("cost", "cost").add("mu", "mu_total").add("sw", "switches")
    sel = PlanSelector(risk).minimise("cost", "mean").subject_to("mu", "max", bound)
    try:
        p.upload(x0, c.om, c.midx)
        got = p.select_plan_policies(c.R, sel, candidates=off, policies=[wide, narrow], u_prev=up, omega_seq=om_seq, step=STEP, cost_w=cw, per_candidate=True, per_trajectory=True)
        assert np.all(got["end_status"] == 0)
        assert np.array_equal(got["admissible"][:, 0], ~cold) and got["admissible"][:, 1:].all()
        assert np.all(got["choice"][~cold] == 0) and np.all(got["policy"][~cold] == -1) and np.all(got["u"][~cold] == 0.0)      # the sequence is admissible and wins
        assert np.all(got["choice"][cold] >= 1) and np.all(got["policy"][cold] >= 0)                                            # filtered: a thermostat wins
        assert cold.sum() >= 1 and (~cold).sum() >= 1
        sw = got["risk"]["mean"][:, :, 2]
        assert np.all(sw[:, 0] == 0.0) and sw[:, 1].mean() != sw[:, 2].mean()
        _check_pick(c, got, sel, S, off, [wide, narrow], up, ("filter",), x0=x0)
    finally:
        _clean(p)


def test_endings(ctx):
    S = 3
    # an infeasible ending (tests/test_gpu_policy_rollout.py::test_an_infeasible_ending): a tank above T_max leaves the auxiliary problem without a feasible point
    h = ctx("a10", hard=True)
    p, B = h.p, h.B
    assert h.d["nmu"] == 0
    om_seq, cand, cw = _scenario(h, 1, S, 9860)
    x0 = h.x0.copy()
    hot = np.arange(B) % 3 == 1
    x0[hot, 0] = 90.0
    P_t = thermostat(h)
    up = np.zeros((B, h.nu))
    risk = RiskTable(None, LEVELS).add("cost", "cost").add("sw", "switches", level=0.0)
    sel = PlanSelector(risk).minimise("cost", "mean")
    kw = dict(omega_seq=om_seq, step=STEP, cost_w=cw)
    try:
        p.upload(x0, h.om, h.midx)
        p.upload_policy(P_t)
        ref = p.rollout(h.R, K=K, policy=True, u_prev=up, risk=risk, **kw)
        p.upload_policy(None)
        dead = ref["end_status"][:, 0] == 1
        assert np.all(dead[hot]) and (~dead).sum() >= 3 and np.all((ref["end_status"] == 1) == dead[:, None])
        for mc in (S, 1):
            got = p.select_plan_policies(h.R, sel, candidates=cand, policies=[P_t], u_prev=up, min_complete=mc, per_candidate=True, per_trajectory=True, **kw)
            _against_closed_loop(got, 1, ref, None, ("infeasible", mc))
            assert np.all(got["switches"][dead, 1] == -1) and np.all(got["switches"][~dead, 1] >= 0) and np.all(got["end_status"][dead, 1] == 1)
            assert np.all(got["switches"][:, 0] == np.where(got["end_status"][:, 0] == 0, 0, -1))
            assert np.all(got["risk"]["n_infeasible"][dead, 1] == S) and not got["admissible"][dead, 1].any() and got["admissible"][~dead, 1].all()
            assert got["stats"]["infeasible"] == int((got["end_status"] == 1).sum()) and got["stats"]["finished_on_host"] == 0
            _check_pick(h, got, sel, mc, cand, [P_t], up, ("infeasible", mc), x0=x0)
    finally:
        _clean(p)

    # a plan candidate without a usable plan beside policy candidates (the cutoff of tests/test_gpu_plan_select.py::test_endings): -1 for that candidate only
    s = ctx("a10")
    p, B = s.p, s.B
    om_seq, cand, cw = _scenario(s, 1, S, 9861)
    pols = [thermostat(s), thermostat(s, 59.5, 60.5)]
    up = _u_prev(s, 9862)
    risk = RiskTable(None, LEVELS).add("cost", "cost").add("mu", "mu_total").add("sw", "switches", level=0.0)
    sel = PlanSelector(risk).minimise("mu", "mean")
    try:
        first = p.solve(s.x0, s.om, s.midx)
        assert np.all(first["status"] == 0)
        p.upload(s.x0, s.om, s.midx)
        masked = np.arange(B) % 2 == 1
        cut = np.full(B, np.inf)
        cut[masked] = (first["obj"] - 1e-6 * np.maximum(1.0, np.abs(first["obj"])))[masked]
        p.set_cutoffs(cut)
        p.solve_resident()
        assert np.all(p.download()["status"][masked] == 1)
        got = p.select_plan_policies(s.R, sel, candidates=cand, plan_first=True, K=K, policies=pols, u_prev=up, omega_seq=om_seq, step=STEP, cost_w=cw,
                            per_candidate=True, per_trajectory=True)
        assert np.all(got["end_status"][masked, 0] == -1) and np.all(got["switches"][masked, 0] == -1) and np.all(got["risk"]["n_not_attempted"][masked, 0] == S)
        assert np.all(got["end_status"][:, 1:] == 0) and np.all(got["end_status"][~masked] == 0) and np.all(got["risk"]["n_not_attempted"][:, 1:] == 0)
        assert not got["admissible"][masked, 0].any() and got["admissible"][:, 1:].all() and np.all(got["choice"][masked] >= 1)
        assert got["stats"]["not_attempted"] == int(masked.sum()) * S
        _check_pick(s, got, sel, S, np.concatenate([_plan_u(s)[:, None], cand], axis=1), pols, up, ("no plan",))
        # the resolver's pivot budget capped: every trajectory ends 2, nothing is finished on the host, nothing is chosen, nothing raised
        p.set_cutoffs(np.full(B, np.inf))
        s.R.problem.set_opts(reserved=_lib.MLD_DBG_SMALL_PIVOT_CAP)
        try:
            got = p.select_plan_policies(s.R, sel, candidates=cand, policies=pols, u_prev=up, omega_seq=om_seq, step=STEP, cost_w=cw, per_candidate=True, per_trajectory=True)
        finally:
            s.R.problem.set_opts(reserved=0)
        assert np.all(got["end_status"] == 2) and np.all(got["switches"] == -1) and np.all(got["risk"]["n_declined"] == S) and np.all(got["risk"]["n_complete"] == 0)
        assert np.all(got["choice"] == -1) and np.all(got["policy"] == -1) and not got["admissible"].any() and np.all(np.isnan(got["u"])) and np.all(np.isnan(got["u0"]))
        assert got["stats"] == dict(trajectories=B * 3 * S, complete=0, infeasible=0, declined=B * 3 * S, not_attempted=0, finished_on_host=0)
    finally:
        p.set_cutoffs(np.full(B, np.inf))
        _clean(p)


def test_u_prev_against_the_resident_state(ctx):
    c = ctx("a10")
    p, S = c.p, 2
    om_seq, cand, cw = _scenario(c, 1, S, 9870)
    P_t = thermostat(c)
    on = np.ones((c.B, c.nu))
    risk = RiskTable(None, LEVELS).add("cost", "cost").add("sw", "switches")
    sel = PlanSelector(risk).minimise("cost", "mean")
    kw = dict(candidates=cand, policies=[P_t], omega_seq=om_seq, step=STEP, cost_w=cw, per_candidate=True, per_trajectory=True)
    try:
        p.upload(c.x0, c.om, c.midx)
        with pytest.raises(MldGpuError, match="u_prev is NULL, but no policy is resident"):
            p.select_plan_policies(c.R, sel, **kw)
        p.upload_policy(thermostat(c, 50.5, 51.5))                          # ANOTHER policy is resident: of it the call reads the state only
        assert np.array_equal(p.policy_state(), np.zeros((c.B, c.nu)))
        reset = p.select_plan_policies(c.R, sel, **kw)
        zeros = p.select_plan_policies(c.R, sel, u_prev=np.zeros(c.nu), **kw)
        given = p.select_plan_policies(c.R, sel, u_prev=on, **kw)
        assert np.array_equal(p.policy_state(), np.zeros((c.B, c.nu)))      # u_prev= is the call's own
        assert np.array_equal(p.policy_state(u_prev=on), on)
        resident = p.select_plan_policies(c.R, sel, **kw)
        for k in PICK + SUMM + ("switches",):
            _same(resident[k], given[k], ("resident against given", k))
            _same(zeros[k], reset[k], ("given zeros against the reset state", k))
        assert not np.array_equal(given["switches"][:, 1], reset["switches"][:, 1])      # tanks inside the band hold what they had
        assert np.array_equal(p.policy_state(), on)
    finally:
        _clean(p)


def test_the_handle_is_untouched(ctx):
    c = ctx("a10")
    p, S = c.p, 3
    rng = np.random.default_rng(9880)
    lib, gw, start, om_seq = _rollout_ref.realised_library(c.om, c.N, c.nw, c.nx, S, K, STEP, rng)
    om_seq = np.ascontiguousarray(om_seq)
    cand = (rng.uniform(size=(c.B, 2, K, c.nu)) < 0.4).astype(float)
    kpis = _kpis(c, 9881, priced=False)
    risk = _with_switches(kpis)
    sel = PlanSelector(risk).minimise("cost", "cvar_hi", level=0.5).subject_to("sw", "max", 1e9)
    resident, on = thermostat(c, 58.5, 61.5), np.ones((c.B, c.nu))
    pols = [thermostat(c), thermostat(c, 59.5, 60.5)]
    try:
        def prepared():
            p.upload(c.x0, c.om, c.midx)
            p.upload_profiles(lib, gw)
            p.upload_policy(resident)
            p.policy_state(u_prev=on)
            p.sim_log_begin(2)
            p.solve_resident()
            p.warm_start_from_previous()

        prepared()
        astart = np.ascontiguousarray(start[:, 0])
        before_step = p.sim_step(act_start=astart, step=STEP, advance=False, log=False, outputs=True)      # (makes the actual starts resident)
        before_roll = p.rollout(c.R, K=K, omega_seq=om_seq, policy=True)                                     # the resident policy and its state, by what they do
        before = (p.inputs(), p.download(), p.sim_log_count(), p.debug_warm_start())
        outs = []
        for kw in (dict(start=start), dict(omega_seq=om_seq)):
            for plan_first in (False, True):
                for up in (None, np.zeros((c.B, c.nu))):
                    got = p.select_plan_policies(c.R, sel, candidates=cand, plan_first=plan_first, K=K, step=STEP, kpis=kpis, policies=pols, u_prev=up, per_candidate=True, **kw)
                    outs.append(got)
                    assert np.all(got["risk"]["n_complete"] == S) and np.all(got["choice"] >= 0)
                    x_in, w_in = p.inputs()
                    assert np.array_equal(x_in, before[0][0]) and np.array_equal(w_in, before[0][1]) and p.sim_log_count() == before[2]
                    after = p.download()
                    for k in after:
                        assert np.array_equal(after[k], before[1][k], equal_nan=True), k
                    assert np.array_equal(p.debug_warm_start(), before[3]) and np.array_equal(p.policy_state(), on)
        for k in PICK:      # the windows gathered from the resident library are the disturbance uploaded
            for i in range(4):
                _same(outs[i][k], outs[4 + i][k], ("start against omega_seq", i, k))
        after_roll = p.rollout(c.R, K=K, omega_seq=om_seq, policy=True)
        for k in SUMM + ("switches",):
            _same(after_roll[k], before_roll[k], ("the resident policy", k))
        after_step = p.sim_step(actual=True, step=STEP, advance=False, log=False, outputs=True)               # act_start=None: the resident starts
        for k in before_step:
            assert np.array_equal(before_step[k], after_step[k], equal_nan=True), k
        p.solve_resident()
        with_call = p.download()
        prepared()
        p.solve_resident()
        without = p.download()
        for k in without:
            assert np.array_equal(with_call[k], without[k], equal_nan=True), k
        # the chosen step 0 is what the resolving step takes
        stepped = p.sim_step(resolve=c.R, u0=outs[0]["u0"], advance=False, log=False, outputs=True)
        assert stepped["n_skipped"] == 0 and np.array_equal(stepped["v0"][:, :c.nu], outs[0]["u0"])
    finally:
        p.set_warm_start(None)
        _clean(p)


def _raw(p, R, S, cand, om_seq, risk, pols, up, P=None, plan_first=0, T=None, obj=(0, 0, 0), min_complete=None, null_cand=False, null_pol=(), tab=None, entry="mld_rollout_select_policy"):
    """the entry itself, outputs prefilled with 7: (rc, message, dict of outputs).  tab: (name, table, model, channel[, state], value) overwrites one table
    entry; null_pol: which of the six pol_* arrays are passed as NULL"""
    B, nu = p.batch, cand.shape[3]
    dp = _lib.dptr
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32)) if a is not None else None
    arr = risk.arrays()
    Tn = len(pols) if T is None else T
    Pn = cand.shape[1] + plan_first + len(pols) if P is None else P
    Pb = max(Pn, 1)
    names = ("sel", "on_at", "off_at", "u_on", "u_off", "mode")
    ptr = [None] * 6
    if pols:
        tabs = {k: np.ascontiguousarray(np.stack([getattr(q, k) for q in pols])) for k in names[:5]}
        tabs["mode"] = np.ascontiguousarray(np.stack([q.mode for q in pols]), dtype=np.int32)
        if tab is not None:
            tabs[tab[0]][tuple(tab[1:-1])] = tab[-1]
        ptr = [None if i in null_pol else (ip(tabs[k]) if k == "mode" else dp(tabs[k])) for i, k in enumerate(names)]
    Gn, Ln = len(risk), max(len(risk.levels), 1)
    o = dict(choice=np.full(B, 7, np.int32), score=np.full(B, 7.0), n_admissible=np.full(B, 7, np.int32), admissible=np.full((B, Pb), 7, np.uint8),
             u=np.full((B, K, nu), 7.0), u0=np.full((B, nu), 7.0), mean=np.full((B, Pb, Gn), 7.0), counts=np.full((B, Pb, 4), 7, np.int32),
             end_status=np.full((B, Pb, S), 7, np.int32), switches=np.full((B, Pb, S), 7, np.int32), stats=np.zeros(4, np.int64))
    lib = _lib.load()
    head = (p._h, R.problem._h, K, S, Pn, plan_first, None if null_cand else dp(cand), dp(om_seq), None, STEP, None, 0, 0,
            None, None, None, None, None, None, None, 1e-6, None,
            Gn, ip(arr["col_src"]), ip(arr["col_q"]), dp(arr["level"]), len(risk.levels), dp(arr["alpha"]),
            obj[0], obj[1], obj[2], 0, None, None, None, None, S if min_complete is None else min_complete,
            ip(o["choice"]), dp(o["score"]), ip(o["n_admissible"]), o["admissible"].ctypes.data_as(C.POINTER(C.c_uint8)), dp(o["u"]), dp(o["u0"]),
            dp(o["mean"]), None, None, None, None, None, None, None, None, None, ip(o["counts"]),
            None, None, None, None, None, ip(o["end_status"]), o["stats"].ctypes.data_as(C.POINTER(C.c_int64)),
            None, None, None, None, None, None, None, None)
    if entry == "mld_rollout_select":
        rc = lib.mld_rollout_select(*head)
    else:
        rc = lib.mld_rollout_select_policy(*(head + (Tn,) + tuple(ptr) + (dp(up), ip(o["switches"]))))
    return rc, lib.mld_last_error(), o


def test_refusals_change_nothing(ctx):
    c, big = ctx("a10"), ctx("b9")
    p, B, S = c.p, c.B, 3
    om_seq, cand, _ = _scenario(c, 2, S, 9890)
    risk = RiskTable(None, (0.5, 1.0)).add("cost", "cost").add("sw", "switches", level=0.0)
    pols = [thermostat(c), thermostat(c, 59.5, 60.5)]
    up, on = np.zeros((B, c.nu)), np.ones((B, c.nu))
    resident = thermostat(c, 58.5, 61.5)
    try:
        p.upload(c.x0, c.om, c.midx)
        p.upload_policy(resident)
        p.policy_state(u_prev=on)
        good_roll = p.rollout(c.R, K=K, omega_seq=om_seq, policy=True)
        state = (p.inputs(), p.download())

        def untouched(word):
            x_in, w_in = p.inputs()
            assert np.array_equal(x_in, state[0][0]) and np.array_equal(w_in, state[0][1]), word
            now = p.download()
            for k in now:
                assert np.array_equal(now[k], state[1][k], equal_nan=True), (word, k)
            assert np.array_equal(p.policy_state(), on), word

        def refused(word, S_=S, om=om_seq, cd=cand, table=risk, pl=pols, u_prev=up, R=c.R, **kw):
            rc, msg, o = _raw(p, R, S_, cd, om, table, pl, u_prev, **kw)
            assert rc == -1 and b"mld_rollout_select_policy" in msg and word in msg, (word, rc, msg)
            for k, a in o.items():                                           # nothing was written
                assert np.all(a == (0 if k == "stats" else 7)), (word, k)
            untouched(word)

        rc, msg, o = _raw(p, c.R, S, cand, om_seq, risk, pols, up, obj=(1, 0, 0))
        assert rc == 0 and np.all(o["choice"] >= 0) and np.all(o["counts"][:, :, 0] == S) and np.all(o["switches"][:, :2] == 0) and np.all(o["u0"] != 7.0), msg      # the helper's good call
        untouched(b"good")
        # the policies
        refused(b"T = -1", T=-1)
        refused(b"T = 5 policy candidates, but P = 4", T=5)
        refused(b"T = 4 policy candidates, but P = 4 candidates in all, the resident plan among them", T=4, plan_first=1, P=4)
        wide = np.ascontiguousarray(np.resize(cand, (B, 63, K, c.nu)))
        refused(b"P = 65", cd=wide)
        rc, msg, o = _raw(p, c.R, S, np.ascontiguousarray(wide[:, :62]), om_seq, risk, pols, up)
        assert rc == 0 and np.all(o["n_admissible"] == 64), msg              # ... and P = 64 counting the policies is the last one accepted
        refused(b"P = 0", P=0, T=0)
        refused(b"pol_sel of table 1, model 0, channel 1, state 1 is not finite", tab=("sel", 1, 0, 1, 1, np.nan))
        refused(b"pol_on_at of table 0, model 2, channel 0 is not finite", tab=("on_at", 0, 2, 0, np.inf))
        refused(b"pol_off_at of table 1, model 1, channel 2 is not finite", tab=("off_at", 1, 1, 2, np.nan))
        refused(b"pol_u_on of table 0, model 0, channel 0 is not finite", tab=("u_on", 0, 0, 0, -np.inf))
        refused(b"pol_u_off of table 1, model 2, channel 1 is not finite", tab=("u_off", 1, 2, 1, np.nan))
        refused(b"pol_on_at > pol_off_at for table 1, model 0, channel 0", tab=("on_at", 1, 0, 0, 99.0))
        refused(b"pol_mode of table 0, model 1, channel 2 is 2", tab=("mode", 0, 1, 2, 2))
        refused(b"pol_mode of table 1, model 2, channel 0 is 0 (passed through): a policy candidate rules every channel", tab=("mode", 1, 2, 0, 0))
        for i in range(6):
            refused(b"is NULL with T = 2", null_pol=(i,))
        bad = up.copy()
        bad[6, 2] = np.nan
        refused(b"u_prev of instance 6, input 2 is not finite", u_prev=bad)
        bad[6, 2] = np.inf
        refused(b"u_prev of instance 6, input 2 is not finite", u_prev=bad)
        # everything mld_rollout_select refuses, by the same code
        refused(b"u_cand is NULL", null_cand=True)
        bad_c = cand.copy()
        bad_c[1, 1, 2, 0] = np.nan
        refused(b"u_cand of instance 1, candidate 1, step 2, input 0 is not finite", cd=bad_c)
        refused(b"has not been solved", plan_first=1)
        refused(b"obj_col = 2", obj=(2, 0, 0))
        refused(b"obj_kind = 7", obj=(0, 7, 0))
        refused(b"obj_level = 2", obj=(0, 4, 2))
        refused(b"min_complete = 0", min_complete=0)
        refused(b"min_complete = 4", min_complete=S + 1)
        om65 = np.ascontiguousarray(np.repeat(om_seq[:, :1], 65, axis=1))
        refused(b"S = 65", S_=65, om=om65)
        refused(b"reads the KPIs, but n_kpi = 0", table=RiskTable(_kpis(c, 9891, priced=False)).add("n", "n_vio"))
        refused(b"not the fold", R=big.R)
        refused(b"exactly one of omega_seq and start", om=None)
        # without policies the switch count has no source, in the new entry as in the old one
        rc, msg, _ = _raw(p, c.R, S, cand, om_seq, risk, [], None, T=0, P=2)
        assert rc == -1 and b"col_src[1] = 3 (switches)" in msg, msg
        # T == 0 is mld_rollout_select's call
        plain = RiskTable(None, (0.5, 1.0)).add("cost", "cost").add("mu", "mu_total", level=0.0)
        rc, msg, new = _raw(p, c.R, S, cand, om_seq, plain, [], None, T=0, P=2, obj=(1, 5, 1))
        rc2, msg2, old = _raw(p, c.R, S, cand, om_seq, plain, [], None, P=2, obj=(1, 5, 1), entry="mld_rollout_select")
        assert rc == 0 and rc2 == 0, (msg, msg2)
        for k in new:
            if k != "switches":
                _same(new[k], old[k], ("T == 0", k))
        assert np.all(new["switches"] == 7)
        # u_prev NULL: the resident state; with no resident policy refused
        rc, msg, res = _raw(p, c.R, S, cand, om_seq, risk, pols, None)
        rc2, msg2, giv = _raw(p, c.R, S, cand, om_seq, risk, pols, on)
        assert rc == 0 and rc2 == 0, (msg, msg2)
        for k in res:
            _same(res[k], giv[k], ("resident u_prev", k))
        untouched(b"after the good calls")
        _same(p.rollout(c.R, K=K, omega_seq=om_seq, policy=True)["switches"], good_roll["switches"], "the resident policy")
        p.upload_policy(None)
        rc, msg, o = _raw(p, c.R, S, cand, om_seq, risk, pols, None)
        assert rc == -1 and b"u_prev is NULL, but no policy is resident" in msg and np.all(o["choice"] == 7), msg
        # the wrapper's own refusals, and one good call afterwards
        sel = PlanSelector(risk).minimise("cost", "mean")
        with pytest.raises(ValueError, match="passes channel 0 of model 0 through"):
            p.select_plan_policies(c.R, sel, candidates=cand, policies=[thermostat(c, mode=[0] + [1] * (c.nu - 1))], u_prev=up, omega_seq=om_seq)
        with pytest.raises(ValueError, match="policies\\[1\\]: a policy.ThresholdPolicy"):
            p.select_plan_policies(c.R, sel, candidates=cand, policies=[pols[0], "thermo"], u_prev=up, omega_seq=om_seq)
        with pytest.raises(ValueError, match="policies\\[0\\] is shaped"):
            p.select_plan_policies(c.R, sel, candidates=cand, policies=[thermostat(big)], u_prev=up, omega_seq=om_seq)
        with pytest.raises(ValueError, match="u_prev given without policies"):
            p.select_plan_policies(c.R, PlanSelector(plain).minimise("cost", "mean"), candidates=cand, u_prev=up, omega_seq=om_seq)
        with pytest.raises(ValueError, match="u_prev has shape"):
            p.select_plan_policies(c.R, sel, candidates=cand, policies=pols, u_prev=np.zeros((B + 1, c.nu)), omega_seq=om_seq)
        again = p.select_plan_policies(c.R, sel, candidates=cand, policies=pols, u_prev=up, omega_seq=om_seq, step=STEP)
        assert np.all(again["choice"] >= 0) and np.all(np.isfinite(again["u0"]))
    finally:
        _clean(p)


def test_without_policies_the_old_entry(ctx):
    """policies=None and policies=[] run today's code path: the same results, host completion included"""
    c = ctx("a10")
    p, S = c.p, 3
    kpis = _kpis(c, 9895, priced=False)
    risk = _table(kpis)
    sel = PlanSelector(risk).minimise("cost", "mean").subject_to("mu", "max", 1e9)
    om_seq, cand, cw = _scenario(c, 3, S, 9896)
    kw = dict(candidates=cand, omega_seq=om_seq, step=STEP, cost_w=cw, kpis=kpis, per_candidate=True, per_trajectory=True)
    try:
        p.upload(c.x0, c.om, c.midx)
        for cap in (0, _lib.MLD_DBG_SMALL_PIVOT_CAP):
            c.R.problem.set_opts(reserved=cap)
            try:
                ref, none, empty = p.select_plan(c.R, sel, **kw), p.select_plan_policies(c.R, sel, policies=None, **kw), p.select_plan_policies(c.R, sel, policies=[], **kw)
            finally:
                c.R.problem.set_opts(reserved=0)
            assert (ref["stats"]["finished_on_host"] > 0) == bool(cap) and "policy" not in ref and "switches" not in ref
            for got in (none, empty):
                assert sorted(got) == sorted(ref) and got["stats"] == ref["stats"]
                for k in PICK[:-1] + SUMM:
                    _same(got[k], ref[k], (cap, k))
                for k in RISK:
                    _same(got["risk"][k], ref["risk"][k], (cap, "risk", k))
                for k in simlog.KPI_ROLLOUT_KEYS:
                    _same(got["kpi"][k], ref["kpi"][k], (cap, "kpi", k))
    finally:
        _clean(p)
