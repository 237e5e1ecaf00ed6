"""Plan selection on the device (mld_rollout_select / GpuProblem.select_plan; kernels k_rollout_cand / k_rollout_cand_kpi, k_rollout_risk, k_plan_select): P
candidate input sequences per instance rolled out under the same S realisations in one launch, each candidate's risk reduced on the device, and the
admissible candidate of least objective statistic chosen.  Two yardsticks, both bit for bit: per candidate the EXISTING entry, rollout(u_seq=cand[:, p],
kpis=..., risk=...) on the same handle; for the choice simlog.select_plan_np on the per-candidate risk of the same call.  Then ties and order, every ending,
the host-completion route, plan certification, the untouched handle and every refusal.

Shapes (tests/test_gpu_sim_resolve.py): a10 -- n_h 3, three models interleaved, batch 10; a1 -- batch 1; b9 -- n_h 7, batch 9.  K = 3, STEP = 1."""
import ctypes as C

import numpy as np
import pytest

import _rollout_ref
from test_gpu_sim_resolve import SHAPES
from test_gpu_small_lds_step import _SmallCtx
from test_gpu_log_summary import _kpis
from test_gpu_rollout_kpi import N_CHAN, _tariff
from pyhybridcontrol_amd import simlog, _lib
from pyhybridcontrol_amd._lib import MldGpuError
from pyhybridcontrol_amd.simlog import PlanSelector, RiskTable

pytestmark = pytest.mark.gpu

K, STEP = 3, 1
SUMM = ("cost", "mu_total", "worst_vio", "worst_step", "steps_done", "end_status")
RISK = simlog.RISK_COL_KEYS + simlog.RISK_LEVEL_KEYS + simlog.RISK_COUNTS
PICK = ("choice", "score", "n_admissible", "admissible", "u", "u0")
LEVELS = (0.5, 1.0, 0.25)
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


def _scenario(c, P, S, seed):
    """(omega_seq (B, S, K, nomega), candidates (B, P, K, nu) random binary, cost_w (K, nv)): test_gpu_rollout_risk._scenario's, P sequences per instance"""
    rng = np.random.default_rng(seed)
    _, _, _, om_seq = _rollout_ref.realised_library(c.om, c.N, c.nw, c.nx, S, K, STEP, rng)
    cand = (rng.uniform(size=(c.B, P, K, c.nu)) < 0.4).astype(float)
    return np.ascontiguousarray(om_seq), cand, rng.uniform(0.5, 2.0, size=(K, c.nv))


def _table(kpis):
    """the risk columns: the summaries, and with a KPI table the counts and a few KPI statistics"""
    r = RiskTable(kpis, LEVELS).add("cost", "cost", level=0.0).add("mu", "mu_total", level=0.0).add("vio", "worst_vio", level=1e-6)
    if kpis is not None:
        r.add("n_vio", "n_vio", level=0.0).add("chg_u0", "kpi_n_changes", kpi="u_0", level=0.0).add("y_sum", "kpi_sum", kpi="y_only").add("all_max", "kpi_max", kpi="all_five")
        r.add("om_min", "kpi_min", kpi="omega_only").add("x_above", "kpi_n_above", kpi="x_only", level=0.0)
        if "priced" in kpis.names:
            r.add("priced_sum", "kpi_sum", kpi="priced").add("priced_max", "kpi_max", kpi="priced")
    return r


def _same(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, (what, a.dtype, b.dtype, a.shape, b.shape)
    ok = ((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))) if a.dtype.kind == "f" else a == b
    assert np.all(ok), (what, int((~ok).sum()), a[~ok][:4], b[~ok][:4])


def _stack(per, keys):
    """the results of P rollout() calls with a candidate axis behind the batch's"""
    return {k: np.stack([r[k] for r in per], axis=1) for k in keys}


def _per_candidate(c, cand, plan_first, **kw):
    """the existing entry, once per candidate: rollout(u_seq=None) for the plan, rollout(u_seq=cand[:, p]) for the others"""
    out = [c.p.rollout(c.R, K=K, **kw)] if plan_first else []
    return out + [c.p.rollout(c.R, u_seq=np.ascontiguousarray(cand[:, p]), **kw) for p in range(cand.shape[1])]


def _check_pick(got, risk, sel, mc, cand_all, what):
    """choice, score, n_admissible, admissible, u, u0 against the numpy rule on `risk`, and the choice's two properties on their own"""
    want = simlog.select_plan_np(risk, sel, mc, candidates=cand_all)
    for k in PICK:
        _same(got[k], want[k], what + (k,))
    val = simlog._select_value(risk, *sel.arrays()["obj"])
    for b in range(val.shape[0]):
        adm = np.flatnonzero(got["admissible"][b])
        if got["choice"][b] < 0:
            assert adm.size == 0 and np.isnan(got["score"][b]) and np.all(np.isnan(got["u"][b])) and np.all(np.isnan(got["u0"][b])), what + (b,)
        else:
            assert got["admissible"][b, got["choice"][b]] and np.all(got["score"][b] <= val[b, adm]), what + (b,)
            assert np.array_equal(got["u"][b], cand_all[b, got["choice"][b]]) and np.array_equal(got["u0"][b], got["u"][b, 0]), what + (b,)


def _clean(*problems):
    for p in problems:
        p.upload_policy(None)
        p.sim_log_begin(0)
        p.upload_profiles(np.zeros(0))
        p.upload_prices(np.zeros(0))


def _plan_u(c):
    return np.ascontiguousarray(c.p.download()["v"].reshape(c.B, c.N, c.nv)[:, :K, :c.nu])


@pytest.mark.parametrize("PS", [(1, 1), (2, 3), (5, 5), (64, 2), (3, 64)])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_per_candidate_against_the_existing_entry(ctx, shape, PS):
    """the summaries, KPI arrays and risk arrays of candidate p are those of rollout(u_seq=cand[:, p], kpis=..., risk=...); with plan_first candidate 0 is
    rollout(u_seq=None)'s.  Without KPIs, with them, and with priced ones whose price start differs from instance to instance (the candidate kernel reads it at b,
    every output at t).  No tolerance."""
    P, S = PS
    c = ctx(shape)
    p = c.p
    try:
        p.upload(c.x0, c.om, c.midx)
        p.solve_resident()
        plib, pstart = _tariff(c.B, K, 9705)
        for with_kpis in (False, True, "priced"):
            kpis = _kpis(c, 9700, priced=with_kpis == "priced") if with_kpis else None
            p.upload_prices(plib, N_CHAN) if with_kpis == "priced" else p.upload_prices(np.zeros(0))
            risk = _table(kpis)
            sel = PlanSelector(risk).minimise("cost", "mean")
            for plan_first in (False, True):
                n_own = P - 1 if plan_first else P
                om_seq, cand, cw = _scenario(c, max(n_own, 1), S, 9710 + 10 * P + S)
                cand = cand[:, :n_own]
                kw = dict(omega_seq=om_seq, step=STEP, cost_w=cw, kpis=kpis, price_start=pstart if with_kpis == "priced" else None)
                what = (shape, P, S, with_kpis, plan_first)
                if plan_first and K > c.N:      # the plan is shorter than the rollout: refused as rollout(u_seq=None) refuses it
                    with pytest.raises(MldGpuError, match="N_tilde"):
                        p.select_plan(c.R, sel, candidates=cand if n_own else None, plan_first=True, K=K, **kw)
                    continue
                got = p.select_plan(c.R, sel, candidates=cand if n_own else None, plan_first=plan_first, K=K, per_candidate=True, per_trajectory=True, **kw)
                ref = _per_candidate(c, cand, plan_first, risk=risk, **kw)
                assert len(ref) == P and got["stats"]["finished_on_host"] == 0 and got["stats"]["trajectories"] == c.B * P * S, what
                assert np.all(got["end_status"] == 0), what      # the comparison cannot pass on NaN alone
                for k in SUMM:
                    assert got[k].shape == (c.B, P, S), (what, k)
                    _same(got[k], _stack(ref, (k,))[k], what + (k,))
                if with_kpis:
                    for k in simlog.KPI_ROLLOUT_KEYS:
                        _same(got["kpi"][k], np.stack([r["kpi"][k] for r in ref], axis=1), what + ("kpi", k))
                    if with_kpis == "priced" and c.B > 1:      # the tariffs differ between instances, and the priced figures with them
                        q = kpis.names.index("priced")
                        assert len(set(pstart.tolist())) > 1 and np.all(np.isfinite(got["kpi"]["sum"][:, :, :, q])) and np.any(got["kpi"]["sum"][:, :, :, q] != 0.0), what
                assert got["risk"]["names"] == risk.names and got["risk"]["levels"] == list(LEVELS)
                for k in RISK:
                    _same(got["risk"][k], np.stack([r["risk"][k] for r in ref], axis=1), what + ("risk", k))
                assert got["risk"]["mean"].shape == (c.B, P, len(risk)) and got["risk"]["quantile"].shape == (c.B, P, len(risk), len(LEVELS))
                assert np.all(got["risk"]["n_complete"] == S) and np.all(got["admissible"]) and np.all(got["n_admissible"] == P)
                if P > 1 and n_own > 1:
                    assert np.any(got["risk"]["mean"][:, 0] != got["risk"]["mean"][:, -1])      # the candidates differ
                cand_all = np.concatenate([_plan_u(c)[:, None], cand], axis=1) if plan_first else cand
                _check_pick(got, got["risk"], sel, S, cand_all, what)
                lean = p.select_plan(c.R, sel, candidates=cand if n_own else None, plan_first=plan_first, K=K, **kw)      # nothing per candidate asked for
                assert sorted(lean) == sorted(PICK + ("stats",)) and lean["stats"] == got["stats"]
                for k in PICK:
                    _same(lean[k], got[k], what + ("lean", k))
    finally:
        _clean(p)


def _constraints(sel, risk, ref_risk, n_cons):
    """n_cons constraints over the table's columns and every kind; each bound the median over (b, p) of its statistic in ref_risk"""
    G = len(risk)
    for k in range(n_cons):
        col, kind = (2 * k + 1) % G, simlog.SELECT_KINDS[k % 7]
        lvl = k % len(LEVELS) if k % 7 >= 4 else None
        bound = float(np.median(simlog._select_value(ref_risk, col, k % 7, 0 if lvl is None else lvl)))
        assert np.isfinite(bound)
        sel.subject_to(col, kind, bound, level=lvl)
    return sel


def test_the_choice_against_the_rule(ctx):
    """every kind of statistic as the objective, with 0, 1 and 8 constraints whose bounds are medians of the per-candidate rollout() calls' statistics"""
    c = ctx("a10")
    p, P, S = c.p, 5, 5
    kpis = _kpis(c, 9720, priced=False)
    risk = _table(kpis)
    om_seq, cand, cw = _scenario(c, P, S, 9721)
    kw = dict(omega_seq=om_seq, step=STEP, cost_w=cw, kpis=kpis)
    seen = dict(none=0, first=0, later=0)
    try:
        p.upload(c.x0, c.om, c.midx)
        ref = _per_candidate(c, cand, False, risk=risk, **kw)
        ref_risk = {k: np.stack([r["risk"][k] for r in ref], axis=1) for k in RISK}
        for j, kind in enumerate(simlog.SELECT_KINDS):
            for n_cons in (0, 1, 8):
                lvl = dict(level=LEVELS[j % 3]) if j >= 4 else {}
                sel = _constraints(PlanSelector(risk).minimise(risk.names[j % len(risk)], kind, **lvl), risk, ref_risk, n_cons)
                for mc in (S, 1):
                    got = p.select_plan(c.R, sel, candidates=cand, min_complete=mc, per_candidate=True, **kw)
                    what = (kind, n_cons, mc)
                    for k in RISK:
                        _same(got["risk"][k], ref_risk[k], what + ("risk", k))
                    _check_pick(got, got["risk"], sel, mc, cand, what)
                    seen["none"] += int((got["choice"] < 0).sum()); seen["first"] += int((got["choice"] == 0).sum()); seen["later"] += int((got["choice"] >= 1).sum())
        print("choices over all calls:", seen)
        assert seen["none"] > 0 and seen["first"] > 0 and seen["later"] > 0, "the inputs no longer exercise the rule: %s" % (seen,)
    finally:
        _clean(p)


def test_ties_and_order(ctx):
    """a column of integer counts as the objective: two identical candidates -- the smaller p wins; permuting the candidates permutes the choice wherever the
    least value is attained once"""
    c = ctx("a10")
    p, P, S = c.p, 6, 3
    kpis = _kpis(c, 9730, priced=False)
    risk = _table(kpis)
    sel = PlanSelector(risk).minimise("chg_u0", "mean")
    om_seq, cand, cw = _scenario(c, P, S, 9731)
    cand[:, 1] = cand[:, 0]
    cand[:, 4] = cand[:, 2]
    kw = dict(omega_seq=om_seq, step=STEP, cost_w=cw, kpis=kpis, per_candidate=True)
    try:
        p.upload(c.x0, c.om, c.midx)
        got = p.select_plan(c.R, sel, candidates=cand, **kw)
        val = got["risk"]["mean"][:, :, risk.names.index("chg_u0")]
        assert np.all(val == np.round(val)) and np.array_equal(val[:, 0], val[:, 1]) and np.array_equal(val[:, 2], val[:, 4])      # integer counts, the ties are there
        assert not np.any(np.isin(got["choice"], (1, 4))) and np.all(got["choice"] >= 0)
        assert np.array_equal(got["choice"], val.argmin(axis=1))      # (argmin: the first of equals)
        _check_pick(got, got["risk"], sel, S, cand, ("ties",))
        two = p.select_plan(c.R, sel, candidates=np.ascontiguousarray(cand[:, :2]), **kw)      # nothing but the tie
        assert np.all(two["choice"] == 0) and np.all(two["n_admissible"] == 2)
        perm = np.array([3, 5, 1, 0, 2, 4])
        swapped = p.select_plan(c.R, sel, candidates=np.ascontiguousarray(cand[:, perm]), **kw)
        for k in RISK:
            _same(swapped["risk"][k], got["risk"][k][:, perm], ("permuted", k))
        for obj in ("cost", "chg_u0"):
            s2 = PlanSelector(risk).minimise(obj, "mean")
            a, b = p.select_plan(c.R, s2, candidates=cand, **kw), p.select_plan(c.R, s2, candidates=np.ascontiguousarray(cand[:, perm]), **kw)
            v = a["risk"]["mean"][:, :, risk.names.index(obj)]
            once = (v == v.min(axis=1, keepdims=True)).sum(axis=1) == 1
            assert np.array_equal(perm[b["choice"][once]], a["choice"][once]), obj
            assert np.array_equal(b["choice"][~once], b["risk"]["mean"][:, :, risk.names.index(obj)].argmin(axis=1)[~once]), obj      # a tie: the smaller p of THIS order
            if obj == "cost":
                assert once.any()
            _same(b["score"], a["score"], ("permuted score", obj))
    finally:
        _clean(p)


def test_endings(ctx):
    S = 3
    # instances whose plan is cut off by an unbeatable cutoff (tests/test_gpu_fallback_step.py): with plan_first candidate 0 is not attempted and never chosen
    s = ctx("a10")
    p, B = s.p, s.B
    kpis = _kpis(s, 9740, priced=False)
    risk = _table(kpis)
    sel = PlanSelector(risk).minimise("mu", "mean")
    om_seq, cand, cw = _scenario(s, 2, S, 9741)
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
        for mc in (S, 1):
            got = p.select_plan(s.R, sel, candidates=cand, plan_first=True, K=K, omega_seq=om_seq, step=STEP, cost_w=cw, kpis=kpis, min_complete=mc,
                                per_candidate=True, per_trajectory=True)
            r = got["risk"]
            assert np.all(r["n_not_attempted"][masked, 0] == S) and np.all(r["n_complete"][masked, 0] == 0) and np.all(got["end_status"][masked, 0] == -1)
            assert np.all(r["n_not_attempted"][:, 1:] == 0) and np.all(r["n_complete"][~masked] == S) and np.all(r["n_complete"][:, 1:] == S)
            assert not got["admissible"][masked, 0].any() and np.all(got["choice"][masked] >= 1) and np.all(got["admissible"][~masked])
            assert got["stats"]["not_attempted"] == int(masked.sum()) * S
            ref = _per_candidate(s, cand, True, omega_seq=om_seq, step=STEP, cost_w=cw, kpis=kpis, risk=risk)
            for k in RISK:
                _same(r[k], np.stack([q["risk"][k] for q in ref], axis=1), ("no plan", k))
            _check_pick(got, r, sel, mc, np.concatenate([_plan_u(s)[:, None], cand], axis=1), ("no plan", mc))
    finally:
        p.set_cutoffs(np.full(B, np.inf))
        _clean(p)

    # a candidate with an infeasible auxiliary step (the search of tests/test_gpu_rollout_risk.py::test_endings): inadmissible at min_complete = S, admissible
    # at min_complete = 1 when a complete realisation exists
    h = ctx("a10", hard=True)
    p, B = h.p, h.B
    kpis = _kpis(h, 9742, priced=False)
    risk = _table(kpis)
    sel = PlanSelector(risk).minimise("mu", "mean")
    om_seq, cand, cw = _scenario(h, 3, S, 9743)
    cand[:, 0] = 0.0
    fn = _rollout_ref.closed_form_resolver(h.mats, h.d)
    found = None
    for f in (5.0, 3.0, 8.0, 2.0, 12.0, 20.0, 50.0):
        om_try = om_seq.copy()
        om_try[:, 1] *= f
        n_ref = np.stack([(simlog.rollout_np(h.mats, h.d, h.midx, h.x0, cand[:, q], om_try, fn)["end_status"] == 0).sum(axis=1) for q in range(3)], axis=1)
        if np.any((n_ref > 0) & (n_ref < S)):
            found = np.ascontiguousarray(om_try)
            break
    assert found is not None
    try:
        p.upload(h.x0, h.om, h.midx)
        kw = dict(candidates=cand, omega_seq=found, cost_w=cw, kpis=kpis, per_candidate=True, per_trajectory=True)
        strict, loose = p.select_plan(h.R, sel, min_complete=S, **kw), p.select_plan(h.R, sel, min_complete=1, **kw)
        n = strict["risk"]["n_complete"]
        part = (n > 0) & (n < S)
        print("mixed endings: n_complete =", n.tolist())
        assert part.any() and np.array_equal(n, (strict["end_status"] == 0).sum(axis=2)) and np.any(strict["end_status"] == 1)      # asserted, not skipped
        assert not strict["admissible"][part].any() and loose["admissible"][part].all()
        assert np.array_equal(strict["admissible"], n == S) and np.array_equal(loose["admissible"], n >= 1)
        ref = _per_candidate(h, cand, False, omega_seq=found, cost_w=cw, kpis=kpis, risk=risk)
        for k in RISK:
            _same(strict["risk"][k], np.stack([q["risk"][k] for q in ref], axis=1), ("infeasible", k))
            _same(loose["risk"][k], strict["risk"][k], ("infeasible, min_complete = 1", k))
        _check_pick(strict, strict["risk"], sel, S, cand, ("infeasible", S))
        _check_pick(loose, loose["risk"], sel, 1, cand, ("infeasible", 1))
    finally:
        _clean(p)


def test_declined_trajectories_take_the_host_route(ctx):
    """the resolver's pivot budget capped: every trajectory is declined on the device and finished on the host -- the same choice as the uncapped handle"""
    c = ctx("a10")
    p, P, S = c.p, 3, 3
    kpis = _kpis(c, 9750, priced=False)
    risk = _table(kpis)
    om_seq, cand, cw = _scenario(c, P, S, 9751)
    kw = dict(candidates=cand, omega_seq=om_seq, step=STEP, cost_w=cw, kpis=kpis, per_candidate=True, per_trajectory=True)
    try:
        p.upload(c.x0, c.om, c.midx)
        free = p.select_plan(c.R, PlanSelector(risk).minimise("cost", "mean"), **kw)
        worst = free["risk"]["max"][:, :, risk.names.index("cost")]
        sel = PlanSelector(risk).minimise("cost", "mean").subject_to("cost", "max", float(np.median(worst)))      # (30 values: the median lies between two of them)
        want = p.select_plan(c.R, sel, **kw)
        assert (want["choice"] < 0).any() and (want["choice"] >= 0).any()
        assert want["stats"]["declined"] == 0 and want["stats"]["finished_on_host"] == 0 and np.all(want["end_status"] == 0)
        c.R.problem.set_opts(reserved=_lib.MLD_DBG_SMALL_PIVOT_CAP)
        try:
            got = p.select_plan(c.R, sel, **kw)
            assert got["stats"]["declined"] == c.B * P * S and got["stats"]["finished_on_host"] > 0 and np.all(got["end_status"] == 0)
            assert np.all(got["risk"]["n_complete"] == S) and not got["risk"]["n_declined"].any()
            host = _per_candidate(c, cand, False, omega_seq=om_seq, step=STEP, cost_w=cw, kpis=kpis, risk=risk)
            for k in RISK:
                _same(got["risk"][k], np.stack([r["risk"][k] for r in host], axis=1), ("host route", k))
            _check_pick(got, got["risk"], sel, S, cand, ("host route",))
            lean = p.select_plan(c.R, sel, **dict(kw, per_candidate=False, per_trajectory=False))
            for k in PICK:
                _same(lean[k], got[k], ("host route, lean", k))
        finally:
            c.R.problem.set_opts(reserved=0)
        assert np.array_equal(got["choice"], want["choice"]) and np.array_equal(got["admissible"], want["admissible"])
        assert np.array_equal(got["u"], want["u"], equal_nan=True) and np.array_equal(got["u0"], want["u0"], equal_nan=True)
    finally:
        _clean(p)


def test_plan_certification(ctx):
    """P = 1 with plan_first: the risk is rollout(risk=...)'s, the choice 0 or -1 by the constraint"""
    c = ctx("a10")
    p, S = c.p, 5
    kpis = _kpis(c, 9760, priced=False)
    risk = _table(kpis)
    om_seq, _, cw = _scenario(c, 1, S, 9761)
    kw = dict(omega_seq=om_seq, step=STEP, cost_w=cw, kpis=kpis)
    try:
        p.upload(c.x0, c.om, c.midx)
        p.solve_resident()
        ref = p.rollout(c.R, K=K, risk=risk, **kw)
        j, l = risk.names.index("cost"), LEVELS.index(0.5)
        stat = ref["risk"]["cvar_hi"][:, j, l]
        bound = float(np.median(stat))
        sel = PlanSelector(risk).minimise("mu", "max").subject_to("cost", "cvar_hi", bound, level=0.5)
        got = p.select_plan(c.R, sel, plan_first=True, K=K, per_candidate=True, per_trajectory=True, **kw)
        for k in RISK:
            _same(got["risk"][k][:, 0], ref["risk"][k], ("certify", k))
        for k in SUMM:
            _same(got[k][:, 0], ref[k], ("certify", k))
        assert got["admissible"].shape == (c.B, 1)
        assert np.array_equal(got["choice"], np.where(stat <= bound, 0, -1)) and (got["choice"] == 0).any() and (got["choice"] == -1).any()
        _check_pick(got, got["risk"], sel, S, _plan_u(c)[:, None], ("certify",))
        with pytest.raises(ValueError, match="no candidate"):
            p.select_plan(c.R, sel, K=K, **kw)
    finally:
        _clean(p)


def test_the_handle_is_untouched(ctx):
    c = ctx("a10")
    p, P, S = c.p, 3, 3
    rng = np.random.default_rng(9770)
    lib, gw, start, om_seq = _rollout_ref.realised_library(c.om, c.N, c.nw, c.nx, S, K, STEP, rng)
    cand = (rng.uniform(size=(c.B, P, K, c.nu)) < 0.4).astype(float)
    kpis = _kpis(c, 9771, priced=False)
    risk = _table(kpis)
    sel = PlanSelector(risk).minimise("cost", "cvar_hi", level=0.5).subject_to("vio", "max", 1e9)
    try:
        def prepared():
            p.upload(c.x0, c.om, c.midx)
            p.upload_profiles(lib, gw)
            p.sim_log_begin(2)
            p.solve_resident()
            p.warm_start_from_previous()

        prepared()
        astart = np.ascontiguousarray(start[:, 0])
        before_step = p.sim_step(act_start=astart, step=STEP, advance=False, log=False, outputs=True)      # (makes the actual starts resident)
        before = (p.inputs(), p.download(), p.sim_log_count(), p.debug_warm_start())
        assert before[3] is not None
        outs = []
        for kw in (dict(start=start), dict(omega_seq=np.ascontiguousarray(om_seq))):
            for plan_first in (False, True):
                got = p.select_plan(c.R, sel, candidates=cand, plan_first=plan_first, K=K, step=STEP, kpis=kpis, per_candidate=True, **kw)
                outs.append(got)
                assert np.all(got["risk"]["n_complete"] == S) and np.all(got["choice"] >= 0)
                x_in, w_in = p.inputs()
                assert np.array_equal(x_in, before[0][0]) and np.array_equal(w_in, before[0][1]) and p.sim_log_count() == before[2]
                after = p.download()
                for k in after:
                    assert np.array_equal(after[k], before[1][k], equal_nan=True), k
                assert np.array_equal(p.debug_warm_start(), before[3])
        for k in PICK:      # the windows gathered from the resident library are the disturbance uploaded
            _same(outs[0][k], outs[2][k], ("start against omega_seq", k))
            _same(outs[1][k], outs[3][k], ("start against omega_seq, plan first", k))
        after_step = p.sim_step(actual=True, step=STEP, advance=False, log=False, outputs=True)               # act_start=None: the resident starts
        for k in before_step:
            assert np.array_equal(before_step[k], after_step[k], equal_nan=True), k
        # a following solve gives the bits it gives without the call
        p.solve_resident()
        with_call = p.download()
        prepared()
        p.solve_resident()
        without = p.download()
        for k in without:
            assert np.array_equal(with_call[k], without[k], equal_nan=True), k
        # the chosen step 0 is what the resolving step takes
        stepped = p.sim_step(resolve=c.R, u0=outs[1]["u0"], advance=False, log=False, outputs=True)
        assert stepped["n_skipped"] == 0 and np.array_equal(stepped["v0"][:, :c.nu], outs[1]["u0"])
    finally:
        p.set_warm_start(None)
        _clean(p)


def _raw(p, R, S, cand, om_seq, risk, P=None, plan_first=0, obj=(0, 0, 0), cons=(), n_cons=None, min_complete=None, null_cand=False, G=None, L=None,
         null_cons=(), no_traj=False):
    """mld_rollout_select itself, outputs prefilled with 7: (rc, message, dict of outputs).  cons: (col, kind, level index, bound) tuples; null_cons: which of
    cons_col, cons_kind, cons_level, cons_bound (0 .. 3) are passed as NULL; no_traj: no (batch, P, S) output is passed (for an S no array of a test can hold)"""
    B, nu = p.batch, cand.shape[3]
    dp = _lib.dptr
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32)) if a is not None else None
    arr = risk.arrays()
    Pn = cand.shape[1] + plan_first if P is None else P
    Pb = max(Pn, 1)
    cc = [np.ascontiguousarray(np.resize(np.asarray([t[i] for t in cons] or [0], np.int32), 8)) for i in range(3)]
    cb = np.ascontiguousarray(np.resize(np.asarray([t[3] for t in cons] or [0.0], np.float64), 8))
    Gn, Ln = len(risk), max(len(risk.levels), 1)
    o = dict(choice=np.full(B, 7, np.int32), score=np.full(B, 7.0), n_admissible=np.full(B, 7, np.int32), admissible=np.full((B, Pb), 7, np.uint8),
             u=np.full((B, K, nu), 7.0), u0=np.full((B, nu), 7.0), mean=np.full((B, Pb, Gn), 7.0), quantile=np.full((B, Pb, Gn, Ln), 7.0),
             counts=np.full((B, Pb, 4), 7, np.int32), end_status=np.full((B, Pb, 1 if no_traj else S), 7, np.int32), stats=np.zeros(4, np.int64))
    cptr = [None if i in null_cons else (ip(cc[i]) if i < 3 else dp(cb)) for i in range(4)]
    lib = _lib.load()
    rc = lib.mld_rollout_select(
        p._h, R.problem._h, K, S, Pn, plan_first, None if null_cand else dp(cand), dp(om_seq), None, STEP, None, 0, 0,
        None, None, None, None, None, None, None, 1e-6, None,
        Gn if G is None else G, ip(arr["col_src"]), ip(arr["col_q"]), dp(arr["level"]), len(risk.levels) if L is None else L, dp(arr["alpha"]),
        obj[0], obj[1], obj[2], len(cons) if n_cons is None else n_cons, cptr[0], cptr[1], cptr[2], cptr[3], S if min_complete is None else min_complete,
        ip(o["choice"]), dp(o["score"]), ip(o["n_admissible"]), o["admissible"].ctypes.data_as(C.POINTER(C.c_uint8)), dp(o["u"]), dp(o["u0"]),
        dp(o["mean"]), None, None, None, None, None, dp(o["quantile"]), None, None, None, ip(o["counts"]),
        None, None, None, None, None, None if no_traj else ip(o["end_status"]), o["stats"].ctypes.data_as(C.POINTER(C.c_int64)),
        None, None, None, None, None, None, None, None)
    return rc, lib.mld_last_error(), o


def test_refusals_change_nothing(ctx):
    c, big = ctx("a10"), ctx("b9")
    p, B, S = c.p, c.B, 3
    om_seq, cand, _ = _scenario(c, 2, S, 9780)
    risk = RiskTable(None, (0.5, 1.0)).add("cost", "cost").add("mu", "mu_total", level=0.0)
    flat = RiskTable(None, ()).add("mu", "mu_total")
    try:
        p.upload(c.x0, c.om, c.midx)
        state = (p.inputs(), p.download())

        def refused(word, S_=S, om=om_seq, cd=cand, table=risk, **kw):
            rc, msg, o = _raw(p, kw.pop("R", c.R), S_, cd, om, table, **kw)
            assert rc == -1 and b"mld_rollout_select" in msg and word in msg, (word, rc, msg)
            for k, a in o.items():                                           # nothing was written
                assert np.all(a == (0 if k == "stats" else 7)), (word, k)
            x_in, w_in = p.inputs()
            assert np.array_equal(x_in, state[0][0]) and np.array_equal(w_in, state[0][1]), word
            now = p.download()
            for k in now:
                assert np.array_equal(now[k], state[1][k], equal_nan=True), (word, k)

        rc, msg, o = _raw(p, c.R, S, cand, om_seq, risk, obj=(1, 5, 1), cons=((0, 4, 0, 1e9),))
        assert rc == 0 and np.all(o["choice"] >= 0) and np.all(o["counts"][:, :, 0] == S) and np.all(o["mean"] != 7.0) and np.all(o["u"] != 7.0), msg      # the helper's good call
        refused(b"P = 0", P=0)
        refused(b"P = -1", P=-1)
        wide = np.ascontiguousarray(np.resize(cand, (B, 65, K, c.nu)))
        refused(b"P = 65", cd=wide)
        rc, msg, o = _raw(p, c.R, S, np.ascontiguousarray(wide[:, :64]), om_seq, risk)
        assert rc == 0 and np.all(o["n_admissible"] == 64) and np.all(o["counts"][:, :, 0] == S), msg      # ... and P = 64 is the last one accepted
        refused(b"u_cand is NULL", null_cand=True)
        refused(b"u_cand is NULL", null_cand=True, plan_first=1, P=2)
        bad = cand.copy()
        bad[1, 1, 2, 0] = np.nan
        refused(b"u_cand of instance 1, candidate 1, step 2, input 0 is not finite", cd=bad)
        bad[1, 1, 2, 0] = np.inf
        refused(b"u_cand of instance 1, candidate 1, step 2, input 0 is not finite", cd=bad)
        refused(b"has not been solved", plan_first=1)                                    # the plan-state tests of by_plan
        refused(b"obj_col = 2", obj=(2, 0, 0))
        refused(b"obj_col = -1", obj=(-1, 0, 0))
        refused(b"obj_kind = 7", obj=(0, 7, 0))
        refused(b"obj_kind = -1", obj=(0, -1, 0))
        refused(b"obj_level = 2", obj=(0, 4, 2))
        refused(b"obj_level = -1", obj=(0, 6, -1))
        refused(b"obj_level = 0", obj=(0, 5, 0), table=flat)                             # a per-level kind with L = 0
        rc, msg, _ = _raw(p, c.R, S, cand, om_seq, risk, obj=(0, 3, 99))
        assert rc == 0, msg                                                              # the level index is read for the per-level kinds only
        refused(b"cons_col[1] = 2", cons=((0, 0, 0, 1.0), (2, 0, 0, 1.0)))
        refused(b"cons_kind[0] = 9", cons=((0, 9, 0, 1.0),))
        refused(b"cons_level[1] = 2", cons=((0, 0, 0, 1.0), (1, 6, 2, 1.0)))
        refused(b"cons_level[0] = 0", cons=((0, 4, 0, 1.0),), table=flat)
        refused(b"cons_bound[1] is NaN", cons=((0, 0, 0, 1.0), (1, 1, 0, np.nan)))
        refused(b"min_complete = 0", min_complete=0)
        refused(b"min_complete = 4", min_complete=S + 1)
        refused(b"n_cons = -1", n_cons=-1)
        refused(b"n_cons = 9", n_cons=9)
        rc, msg, _ = _raw(p, c.R, S, cand, om_seq, risk, cons=((0, 0, 0, 1e9),) * 8)
        assert rc == 0, msg                                                              # ... and eight are accepted
        for i in (0, 1, 3):                                                              # the constraint arrays: three are needed, the level indices are not
            refused(b"cons_col, cons_kind or cons_bound is NULL with n_cons = 1", cons=((0, 0, 0, 1e9),), null_cons=(i,))
        rc, msg, o = _raw(p, c.R, S, cand, om_seq, risk, obj=(1, 0, 0), cons=((0, 4, 1, 1e9), (1, 2, 0, 1e9)), null_cons=(2,))
        rc2, msg2, o2 = _raw(p, c.R, S, cand, om_seq, risk, obj=(1, 0, 0), cons=((0, 4, 0, 1e9), (1, 2, 0, 1e9)))
        assert rc == 0 and rc2 == 0, (msg, msg2)                                         # cons_level == NULL: level index 0 for every constraint
        for k in ("choice", "score", "n_admissible", "admissible", "u0"):
            _same(o[k], o2[k], ("cons_level NULL", k))
        refused(b"cons_level[0] = 0", cons=((0, 4, 0, 1.0),), table=flat, null_cons=(2,))   # ... which a table without levels does not have
        # batch x P x S beyond INT_MAX while batch x S is not: tested before S <= 64 and before omega_seq is read, so no array of that size exists
        big_S = (2 ** 31) // (B * 64) + 1
        assert B * big_S <= 2 ** 31 - 1 < B * 64 * big_S
        refused(b"batch x P x S = %d trajectories" % (B * 64 * big_S), S_=big_S, cd=np.ascontiguousarray(wide[:, :64]), no_traj=True)
        # everything mld_rollout_risk refuses for an open-loop call, by the same code
        om65 = np.ascontiguousarray(np.repeat(om_seq[:, :1], 65, axis=1))
        refused(b"S = 65", S_=65, om=om65)
        refused(b"G = 0", G=0)
        refused(b"L = 9", L=9)
        refused(b"col_src[0] = 3 (switches)", table=RiskTable().add("s", "switches"))
        refused(b"reads the KPIs, but n_kpi = 0", table=RiskTable(_kpis(c, 9781, priced=False)).add("n", "n_vio"))
        refused(b"not the fold", R=big.R)
        refused(b"exactly one of omega_seq and start", om=None)
        # the plan-state tests once more, after a solve and an applied step
        p.solve_resident()
        state = (p.inputs(), p.download())
        rc, msg, o = _raw(p, c.R, S, cand, om_seq, risk, plan_first=1)
        assert rc == 0 and o["admissible"].shape == (B, 3) and np.all(o["counts"][:, :, 0] == S), msg
        with pytest.raises(ValueError, match="1 .. 64"):
            p.select_plan(c.R, PlanSelector(risk).minimise("cost", "mean"), candidates=wide, omega_seq=om_seq)
        with pytest.raises(ValueError, match="min_complete"):
            p.select_plan(c.R, PlanSelector(risk).minimise("cost", "mean"), candidates=cand, omega_seq=om_seq, min_complete=0)
        again = p.select_plan(c.R, PlanSelector(risk).minimise("mu", "cvar_hi", level=1.0).subject_to("cost", "quantile", 1e9, level=0.5), candidates=cand,
                              omega_seq=om_seq, step=STEP)                               # ... and one good call afterwards still works
        assert np.all(again["choice"] >= 0) and np.all(np.isfinite(again["u0"]))
    finally:
        _clean(p)
