"""Rollout risk on the device (mld_rollout_risk / GpuProblem.rollout(risk=...), kernel k_rollout_risk): the statistics across the realisations of every
instance -- mean, extremes, exceedances, quantiles and tail means of a rollout's per-trajectory results over the realisations that ended 0 -- reduced behind
the rollout kernel.  The yardstick is simlog.rollout_risk_np on the per-trajectory outputs of the SAME call, expected bit for bit: the rule fixes the order
(sorted by (value, c)) and the summation tree.  Then the rollout beside it unchanged, every ending, declined trajectories finished on the host, the untouched
handle and every refusal.

Shapes (tests/test_gpu_rollout.py): a10 -- n_h 3, three models interleaved, batch 10; a1 -- batch 1; b9 -- n_h 7, batch 9.  STEP = 1."""
import ctypes as C

import numpy as np
import pytest

import _rollout_ref
from test_gpu_sim_resolve import SHAPES
from test_gpu_small_lds_step import _SmallCtx
from test_gpu_policy_rollout import thermostat
from test_gpu_log_summary import _kpis
from pyhybridcontrol_amd import simlog, _lib
from pyhybridcontrol_amd.simlog import RiskTable

pytestmark = pytest.mark.gpu

STEP = 1
SUMM = ("cost", "mu_total", "worst_vio", "worst_step", "steps_done", "end_status")
TRAJ = ("x", "v", "y", "cons_vio", "cons_row")
RISK = simlog.RISK_COL_KEYS + simlog.RISK_LEVEL_KEYS + simlog.RISK_COUNTS
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


def _scenario(c, K, S, seed):
    """(omega_seq (B, S, K, nomega), u_seq (B, K, nu)) of a context: tests/test_gpu_rollout.py's, with S of the caller's choice"""
    rng = np.random.default_rng(seed)
    _, _, _, om_seq = _rollout_ref.realised_library(c.om, c.N, c.nw, c.nx, S, K, STEP, rng)
    u_seq = (rng.uniform(size=(c.B, K, c.nu)) < 0.4).astype(float)
    return np.ascontiguousarray(om_seq), u_seq


def _levels(S):
    return (1.0 / S, 1.0, 1e-9, 0.5, 0.25, 0.75, 0.95, 0.05)


def _sixty_four(kpis, S, policy, nu):
    """G = 64 over all ten sources (switches with the policy only) and L = 8; the columns with ties first: every input channel's n_changes, switches"""
    r = RiskTable(kpis, _levels(S))
    for j in range(nu):
        r.add("chg_u%d" % j, "kpi_n_changes", kpi="u_%d" % j, level=0.0)
    if policy:
        r.add("switches", "switches", level=1.0)
    r.add("cost", "cost").add("mu", "mu_total", level=0.0).add("vio", "worst_vio", level=1e-6).add("n_vio", "n_vio", level=0.0)
    k = 0
    while len(r) < 64:
        src = ("kpi_sum", "kpi_min", "kpi_max", "kpi_n_above", "kpi_n_changes")[k % 5]
        name = kpis.names[(k // 5) % len(kpis)]
        r.add("%s:%s:%d" % (src, name, k), src, kpi=name, level=float(k % 7) - 3.0)
        k += 1
    return r


def _bits(got, want, what):
    """every risk array equal in every bit (NaN compares as NaN)"""
    assert got["names"] == want["names"] and got["levels"] == want["levels"], what
    for k in RISK:
        a, b = got[k], want[k]
        assert a.dtype == b.dtype and a.shape == b.shape, (what, k, a.dtype, b.dtype, a.shape, b.shape)
        same = ((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))) if a.dtype.kind == "f" else a == b
        assert np.all(same), (what, k, int((~same).sum()), a[~same][:4], b[~same][:4])


def _clean(*problems):
    for p in problems:
        p.upload_policy(None)
        p.sim_log_begin(0)
        p.upload_profiles(np.zeros(0))
        p.upload_prices(np.zeros(0))


@pytest.mark.parametrize("S", [1, 2, 3, 5, 64])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_bit_for_bit_against_the_numpy_rule(ctx, shape, S):
    """open loop and the thermostat's closed loop, K = 1 and K = N_tilde + 2, G = 64 with L = 8 (all ten sources, levels 1 / S, 1.0, 1e-9 among them) and
    G = 1 with L = 0.  No tolerance."""
    c = ctx(shape)
    p = c.p
    kpis = _kpis(c, 9900, priced=False)
    P = thermostat(c)
    x0 = c.x0.copy()
    x0[0, 0] = 47.0                                                          # slack somewhere: cons_vio above the tolerance, n_vio not all zero
    seen_tie = seen_spread = False
    try:
        p.upload(x0, c.om, c.midx)
        p.upload_policy(P)
        for K in (1, c.N + 2):
            om_seq, u_seq = _scenario(c, K, S, 9910 + 100 * S + K)
            for policy in (False, True):
                kw = dict(K=K, policy=True) if policy else dict(u_seq=u_seq)
                big = _sixty_four(kpis, S, policy, c.nu)
                one = RiskTable().add("sw", "switches") if policy else RiskTable(kpis).add("chg", "kpi_n_changes", kpi="u_0", level=0.0)
                for risk in (big, one):
                    got = p.rollout(c.R, omega_seq=om_seq, step=STEP, kpis=kpis, risk=risk, **kw)
                    what = (shape, S, K, policy, len(risk))
                    assert np.all(got["end_status"] == 0), what      # the comparison cannot pass on NaN alone
                    assert got["stats"]["finished_on_host"] == 0, what       # ... nor on figures the host put there
                    r = got["risk"]
                    assert r["mean"].shape == (c.B, len(risk)) and r["quantile"].shape == (c.B, len(risk), len(risk.levels)) and np.all(r["n_complete"] == S)
                    _bits(r, simlog.rollout_risk_np(got, risk, policy=policy), what)
                    assert np.all(np.isfinite(r["mean"])) and np.all((r["min_c"] >= 0) & (r["max_c"] < S))
                    if risk is big:
                        chg = got["kpi"]["n_changes"][:, :, kpis.names.index("u_0")]
                        if not policy:      # open loop: the realisations of an instance apply the same inputs -- the column ties, the smallest c wins
                            assert np.all(chg == chg[:, :1])
                            assert np.all(r["min_c"][:, 0] == 0) and np.all(r["max_c"][:, 0] == 0)
                            assert np.array_equal(r["quantile_c"][:, 0, :], np.broadcast_to(simlog.risk_rank_table(risk.levels, S)[:, S - 1], (c.B, 8)))
                            seen_tie = seen_tie or chg.max() > 0
                        j = [n.startswith("kpi_sum:omega_only") for n in big.names].index(True)      # the realised disturbance itself: it differs over c
                        seen_spread = seen_spread or bool(np.any(r["max"][:, j] > r["min"][:, j]))
                        assert np.array_equal(r["quantile"][:, :, 1], r["max"]) and np.array_equal(r["quantile"][:, :, 2], r["min"])      # alpha = 1, 1e-9
        assert seen_tie and (seen_spread or S == 1)
    finally:
        _clean(p)


def test_the_rollout_beside_it_is_unchanged(ctx):
    c = ctx("a10")
    p, S, K = c.p, 5, c.N + 2
    om_seq, u_seq = _scenario(c, K, S, 9920)
    kpis = _kpis(c, 9921, priced=False)
    P = thermostat(c)
    try:
        p.upload(c.x0, c.om, c.midx)
        p.upload_policy(P)
        for policy in (False, True):
            kw = dict(K=K, policy=True) if policy else dict(u_seq=u_seq)
            risk = _sixty_four(kpis, S, policy, c.nu)
            plain = p.rollout(c.R, omega_seq=om_seq, step=STEP, trajectories=True, kpis=kpis, **kw)
            bare = p.rollout(c.R, omega_seq=om_seq, step=STEP, **kw)
            assert sorted(plain) == sorted(SUMM + TRAJ + ("kpi", "stats") + (("switches",) if policy else ()))      # risk=None: the keys of today
            assert sorted(bare) == sorted(SUMM + ("stats",) + (("switches",) if policy else ()))
            full = p.rollout(c.R, omega_seq=om_seq, step=STEP, trajectories=True, kpis=kpis, risk=risk, **kw)
            assert sorted(full) == sorted(list(plain) + ["risk"])
            for k in SUMM + TRAJ + (("switches",) if policy else ()):
                assert np.array_equal(full[k].view(np.uint64 if full[k].dtype.kind == "f" else full[k].dtype),
                                      plain[k].view(np.uint64 if plain[k].dtype.kind == "f" else plain[k].dtype)), (policy, k)
            for k in simlog.KPI_ROLLOUT_KEYS:
                assert np.array_equal(full["kpi"][k], plain["kpi"][k], equal_nan=True) and full["kpi"][k].dtype == plain["kpi"][k].dtype, (policy, k)
            assert full["stats"] == plain["stats"]
            only = p.rollout(c.R, omega_seq=om_seq, step=STEP, kpis=kpis, risk=risk, per_trajectory=False, **kw)
            assert sorted(only) == ["risk", "stats"] and only["stats"] == plain["stats"]
            assert not any(isinstance(a, np.ndarray) and a.shape[:2] == (c.B, S) and a.ndim >= 2 and k not in RISK for k, a in only["risk"].items())
            _bits(only["risk"], full["risk"], ("per_trajectory=False", policy))
            # a table without KPI columns needs no KPI table: n_kpi = 0 in the C call
            lean = RiskTable(None, (0.5, 1.0)).add("cost", "cost").add("mu", "mu_total", level=0.0)
            a = p.rollout(c.R, omega_seq=om_seq, step=STEP, risk=lean, **kw)
            assert sorted(a) == sorted(list(bare) + ["risk"])
            _bits(a["risk"], simlog.rollout_risk_np(a, lean, policy=policy), ("no KPI table", policy))
            for k in SUMM:
                assert np.array_equal(a[k], bare[k], equal_nan=True), k
        with pytest.raises(ValueError, match="per_trajectory=False without risk"):
            p.rollout(c.R, omega_seq=om_seq, u_seq=u_seq, per_trajectory=False)
        with pytest.raises(ValueError, match="switches"):
            p.rollout(c.R, omega_seq=om_seq, u_seq=u_seq, risk=RiskTable().add("s", "switches"))
        with pytest.raises(ValueError, match="kpis is None"):
            p.rollout(c.R, omega_seq=om_seq, u_seq=u_seq, risk=RiskTable(kpis).add("s", "n_vio"))
    finally:
        _clean(p)


def _empty(r, at):
    ok = all(np.all(np.isnan(r[k][at])) for k in ("mean", "quantile", "cvar_hi", "cvar_lo"))
    ok = ok and np.all(r["min"][at] == np.inf) and np.all(r["max"][at] == -np.inf) and np.all(r["n_exceed"][at] == 0)
    return ok and all(np.all(r[k][at] == -1) for k in ("min_c", "max_c", "quantile_c"))


def _counts_agree(r, es):
    for key, e in zip(simlog.RISK_COUNTS, (0, 1, 2, -1)):
        assert np.array_equal(r[key], (es == e).sum(axis=1)), key


def test_endings(ctx):
    S = 3
    # infeasible auxiliaries (the fixture of tests/test_gpu_rollout_kpi.py::test_endings): instances without a complete realisation are empty
    h = ctx("a10", hard=True)
    p, B, K = h.p, h.B, 4
    om_seq, _ = _scenario(h, K, S, 9930)
    hot = np.arange(B) % 3 == 1
    x0 = h.x0.copy()
    x0[hot, 0] = 90.0
    u_seq = np.zeros((B, K, h.nu))
    kpis = _kpis(h, 9931, priced=False)
    risk = _sixty_four(kpis, S, False, h.nu)
    p.upload(x0, h.om, h.midx)
    got = p.rollout(h.R, u_seq=u_seq, omega_seq=om_seq, kpis=kpis, risk=risk)
    r = got["risk"]
    assert np.all(got["end_status"][hot] == 1) and np.all(r["n_complete"][hot] == 0) and np.all(r["n_infeasible"][hot] == S) and (r["n_complete"] == S).any()
    _counts_agree(r, got["end_status"])
    assert _empty(r, hot) and np.all(np.isfinite(r["mean"][r["n_complete"] > 0]))
    _bits(r, simlog.rollout_risk_np(got, risk), "beside infeasible instances")

    # mixed endings inside an instance: realisation 1's disturbance scaled until simlog.rollout_np ends some instance's realisations differently
    fn = _rollout_ref.closed_form_resolver(h.mats, h.d)
    found = None
    for f in (5.0, 3.0, 8.0, 2.0, 12.0, 20.0, 50.0):
        for u_try in (u_seq, _scenario(h, K, S, 9932)[1]):
            om_try = om_seq.copy()
            om_try[:, 1] *= f
            ref = simlog.rollout_np(h.mats, h.d, h.midx, h.x0, u_try, om_try, fn)
            n_ref = (ref["end_status"] == 0).sum(axis=1)
            if np.any((n_ref > 0) & (n_ref < S)):
                found = (om_try, u_try, n_ref)
                break
        if found:
            break
    assert found is not None
    om_mix, u_mix, n_ref = found
    p.upload(h.x0, h.om, h.midx)
    got = p.rollout(h.R, u_seq=u_mix, omega_seq=np.ascontiguousarray(om_mix), kpis=kpis, risk=risk)
    r = got["risk"]
    print("mixed endings: n_complete =", r["n_complete"].tolist(), "numpy rollout:", n_ref.tolist())
    part = (r["n_complete"] > 0) & (r["n_complete"] < S)
    assert part.any()                                                        # asserted, not skipped: some instance has 0 < n < S
    _counts_agree(r, got["end_status"])
    _bits(r, simlog.rollout_risk_np(got, risk), "mixed endings")
    j = risk.names.index("mu")
    for b in np.flatnonzero(part):                                           # the statistics over the complete realisations only
        done = np.flatnonzero(got["end_status"][b] == 0)
        mu = got["mu_total"][b, done]
        assert r["min"][b, j] == mu.min() and r["max"][b, j] == mu.max() and r["min_c"][b, j] in done and r["max_c"][b, j] in done
        assert np.all(np.isin(r["quantile_c"][b], done)) and np.all(np.isfinite(r["mean"][b])) and np.all(np.isfinite(r["cvar_hi"][b]))
    assert _empty(r, r["n_complete"] == 0)

    # instances without a usable plan with u_seq=None: not attempted
    s = ctx("a10")
    p = s.p
    K = s.N
    om_seq, _ = _scenario(s, K, S, 9933)
    kpis = _kpis(s, 9934, priced=False)
    risk = _sixty_four(kpis, S, False, s.nu)
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
        got = p.rollout(s.R, omega_seq=om_seq, step=STEP, kpis=kpis, risk=risk)
        r = got["risk"]
        assert np.all(r["n_not_attempted"][masked] == S) and np.all(r["n_complete"][masked] == 0) and np.all(r["n_complete"][~masked] == S)
        _counts_agree(r, got["end_status"])
        assert _empty(r, masked) and np.all(np.isfinite(r["mean"][~masked]))
        _bits(r, simlog.rollout_risk_np(got, risk), "beside instances without a plan")
    finally:
        p.set_cutoffs(np.full(B, np.inf))
        _clean(p)


def _raw(p, R, K, S, u_seq, om_seq, kpis=None, policy=0, cols=((0, 0),), level=None, alpha=(), G=None, L=None, n_kpi=None):
    """mld_rollout_risk itself, outputs prefilled with 7: (rc, message, dict of outputs).  cols: (src, q) pairs; G, L, n_kpi override the counts."""
    B = p.batch
    dp = _lib.dptr
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32)) if a is not None else None
    lp = lambda a: a.ctypes.data_as(C.POINTER(C.c_int64)) if a is not None else None
    Q, tabs, chan, thr = 0, [None] * 5, None, None
    if kpis is not None:
        arr = kpis.arrays()
        Q = len(kpis)
        tabs = [None if arr[k] is None else np.ascontiguousarray(arr[k], dtype=np.float64) for k in simlog.KPI_TABLES]
        chan = np.ascontiguousarray(arr["price_chan"], dtype=np.int32)
        thr = None if arr["thresh"] is None else np.ascontiguousarray(arr["thresh"], dtype=np.float64)
    Gn, Ln = max(len(cols), G or 0, 1), max(len(alpha), L or 0, 1)
    src, q = np.zeros(Gn, np.int32), np.zeros(Gn, np.int32)
    src[:len(cols)], q[:len(cols)] = [a for a, _ in cols], [b for _, b in cols]
    lev = None if level is None else np.ascontiguousarray(np.resize(np.asarray(level, np.float64), Gn))
    al = np.full(Ln, 0.5)
    al[:len(alpha)] = alpha
    o = dict(end_status=np.full((B, S), 7, np.int32), cost=np.full((B, S), 7.0), stats=np.zeros(4, np.int64), counts=np.full((B, 4), 7, np.int32))
    o.update({k: np.full((B, Gn), 7.0) for k in ("mean", "min", "max")}, **{k: np.full((B, Gn), 7, np.int32) for k in ("min_c", "max_c", "n_exceed")})
    o.update({k: np.full((B, Gn, Ln), 7.0) for k in ("quantile", "cvar_hi", "cvar_lo")}, quantile_c=np.full((B, Gn, Ln), 7, np.int32))
    lib = _lib.load()
    rc = lib.mld_rollout_risk(p._h, R.problem._h, policy, K, S, dp(u_seq), None, dp(om_seq), None, STEP, None, 0, Q if n_kpi is None else n_kpi,
                              *([dp(a) for a in tabs] + [ip(chan), dp(thr), 1e-6, None]),
                              None, None, None, None, None, dp(o["cost"]), None, None, None, None, ip(o["end_status"]), None, lp(o["stats"]),
                              None, None, None, None, None, None, None, None,
                              len(cols) if G is None else G, ip(src), ip(q), dp(lev), len(alpha) if L is None else L, dp(al),
                              dp(o["mean"]), dp(o["min"]), dp(o["max"]), ip(o["min_c"]), ip(o["max_c"]), ip(o["n_exceed"]),
                              dp(o["quantile"]), ip(o["quantile_c"]), dp(o["cvar_hi"]), dp(o["cvar_lo"]), ip(o["counts"]))
    return rc, lib.mld_last_error(), o


def test_declined_trajectories(ctx):
    """the resolver's pivot budget capped: the C call returns every trajectory declined and the empty statistics; rollout() finishes them on the host and
    its risk is the numpy rule's of the finished arrays"""
    c = ctx("a10")
    p, B, S, K = c.p, c.B, 3, c.N
    om_seq, u_seq = _scenario(c, K, S, 9940)
    kpis = _kpis(c, 9941, priced=False)
    risk = _sixty_four(kpis, S, False, c.nu)
    arr = risk.arrays()
    cols = list(zip(arr["col_src"].tolist(), arr["col_q"].tolist()))
    try:
        p.upload(c.x0, c.om, c.midx)
        want = p.rollout(c.R, u_seq=u_seq, omega_seq=om_seq, step=STEP, kpis=kpis, risk=risk)
        assert want["stats"]["declined"] == 0 and np.all(want["end_status"] == 0)
        c.R.problem.set_opts(reserved=_lib.MLD_DBG_SMALL_PIVOT_CAP)
        try:
            rc, msg, o = _raw(p, c.R, K, S, u_seq, om_seq, kpis=kpis, cols=cols, level=arr["level"], alpha=risk.levels)
            assert rc == 0, msg
            assert np.all(o["end_status"] == 2) and list(o["stats"]) == [B * S, 0, 0, B * S]
            assert np.array_equal(o["counts"], np.tile(np.array([0, 0, S, 0], np.int32), (B, 1)))
            assert _empty(o, np.ones(B, bool))
            host = None
            for kw in (dict(trajectories=True), dict(), dict(per_trajectory=False)):
                got = p.rollout(c.R, u_seq=u_seq, omega_seq=om_seq, step=STEP, kpis=kpis, risk=risk, **kw)
                assert got["stats"]["finished_on_host"] == B * S and got["stats"]["declined"] == B * S
                assert ("x" in got) == bool(kw.get("trajectories")) and ("end_status" in got) == kw.get("per_trajectory", True)
                if host is None:
                    assert np.all(got["end_status"] == 0)
                    host = simlog.rollout_risk_np(got, risk)
                _bits(got["risk"], host, "finished on the host %s" % (kw,))
                assert np.all(got["risk"]["n_complete"] == S) and not got["risk"]["n_declined"].any()
            # the host-finished figures are the device's up to the completion's own deviation in x, v (tests/test_gpu_rollout.py::test_host_completion: 1e-6)
            j = risk.names.index("mu")
            assert np.all(np.abs(host["mean"][:, j] - want["risk"]["mean"][:, j]) <= 1e-6 * K * np.maximum(1.0, np.abs(want["risk"]["mean"][:, j])))
        finally:
            c.R.problem.set_opts(reserved=0)
    finally:
        _clean(p)


def test_the_handle_is_untouched(ctx):
    c = ctx("a10")
    p, S, K = c.p, 3, c.N
    rng = np.random.default_rng(9950)
    lib, gw, start, om_seq = _rollout_ref.realised_library(c.om, c.N, c.nw, c.nx, S, K, STEP, rng)
    u_seq = (rng.uniform(size=(c.B, K, c.nu)) < 0.4).astype(float)
    kpis = _kpis(c, 9951, priced=False)
    P = thermostat(c)
    try:
        p.upload(c.x0, c.om, c.midx)
        p.upload_profiles(lib, gw)
        p.upload_policy(P)
        p.sim_log_begin(2)
        p.solve_resident()
        p.warm_start_from_previous()
        u_state = p.policy_state((rng.uniform(size=(c.B, c.nu)) < 0.5).astype(float))
        astart = np.ascontiguousarray(start[:, 0])
        before_step = p.sim_step(act_start=astart, step=STEP, advance=False, log=False, outputs=True)      # (makes the actual starts resident)
        before = (p.inputs(), p.download(), p.sim_log_count(), p.debug_warm_start())
        assert before[3] is not None
        for policy in (False, True):
            risk = _sixty_four(kpis, S, policy, c.nu)
            for kw in (dict(), dict(per_trajectory=False)):
                got = p.rollout(c.R, u_seq=u_seq, start=start, step=STEP, policy=policy, kpis=kpis, risk=risk, **kw)
                assert np.all(got["risk"]["n_complete"] == S)
                x_in, w_in = p.inputs()
                assert np.array_equal(x_in, before[0][0]) and np.array_equal(w_in, before[0][1]) and p.sim_log_count() == before[2]
                after = p.download()
                for k in after:
                    assert np.array_equal(after[k], before[1][k], equal_nan=True), k
                assert np.array_equal(p.debug_warm_start(), before[3]) and np.array_equal(p.policy_state(), u_state)
        after_step = p.sim_step(actual=True, step=STEP, advance=False, log=False, outputs=True)               # act_start=None: the resident starts
        for k in before_step:
            assert np.array_equal(before_step[k], after_step[k], equal_nan=True), k
    finally:
        p.set_warm_start(None)
        _clean(p)


def test_refusals_change_nothing(ctx):
    c, big = ctx("a10"), ctx("b9")
    p, B, S, K = c.p, c.B, 3, c.N
    om_seq, u_seq = _scenario(c, K, S, 9960)
    kpis = _kpis(c, 9961, priced=False)
    Q = len(kpis)
    try:
        p.upload(c.x0, c.om, c.midx)
        p.solve_resident()
        state = (p.inputs(), p.download())
        risk = _sixty_four(kpis, S, False, c.nu)
        good = p.rollout(c.R, u_seq=u_seq, omega_seq=om_seq, step=STEP, kpis=kpis, risk=risk)

        def refused(word, S_=S, om=om_seq, **kw):
            rc, msg, o = _raw(p, kw.pop("R", c.R), K, S_, u_seq, om, **kw)
            assert rc == -1 and b"mld_rollout_risk" in msg and word in msg, (word, rc, msg)
            for k, a in o.items():                                           # nothing was written
                assert np.all(a == (0 if k == "stats" else 7)), (word, k)
            x_in, w_in = p.inputs()
            assert np.array_equal(x_in, state[0][0]) and np.array_equal(w_in, state[0][1]), word
            now = p.download()
            for k in now:
                assert np.array_equal(now[k], state[1][k], equal_nan=True), (word, k)

        rc, msg, o = _raw(p, c.R, K, S, u_seq, om_seq, kpis=kpis, cols=((0, 0), (5, Q - 1), (9, 0)), alpha=(0.5, 1.0))
        assert rc == 0 and np.all(o["counts"][:, 0] == S) and np.all(o["mean"] != 7.0), msg      # the helper's good call is accepted
        om65 = np.ascontiguousarray(np.repeat(om_seq[:, :1], 65, axis=1))
        refused(b"S = 65", S_=65, om=om65)
        rc, msg, o = _raw(p, c.R, K, 64, u_seq, np.ascontiguousarray(om65[:, :64]))
        assert rc == 0 and np.all(o["counts"][:, 0] == 64), msg             # ... and S = 64 is the last one accepted
        refused(b"G = 0", G=0)
        refused(b"G = 65", G=65)
        refused(b"L = -1", L=-1)
        refused(b"L = 9", L=9)
        refused(b"col_src[1] = 10", kpis=kpis, cols=((0, 0), (10, 0)))
        refused(b"col_src[0] = -1", kpis=kpis, cols=((-1, 0),))
        refused(b"col_src[2] = 3 (switches)", kpis=kpis, cols=((0, 0), (1, 0), (3, 0)))
        for s in range(4, 10):
            refused(b"col_src[0] = %d reads the KPIs, but n_kpi = 0" % s, cols=((s, 0),))
        refused(b"col_q[1] = -1", kpis=kpis, cols=((0, 0), (5, -1)))
        refused(b"col_q[0] = %d" % Q, kpis=kpis, cols=((9, Q),))
        rc, msg, _ = _raw(p, c.R, K, S, u_seq, om_seq, kpis=kpis, cols=((4, Q + 5), (0, -3)))
        assert rc == 0, msg                                                  # col_q is read for the sources 5 .. 9 only
        refused(b"alpha[1] = 0", alpha=(0.5, 0.0))
        refused(b"alpha[0] = 1.5", alpha=(1.5,))
        refused(b"alpha[2] = nan", alpha=(0.5, 1.0, np.nan))
        refused(b"alpha[0] = -0.25", alpha=(-0.25,))
        refused(b"level[1] is NaN", cols=((0, 0), (1, 0)), level=(0.0, np.nan))
        # everything mld_rollout_kpi refuses, by the same code
        refused(b"n_kpi = 65", kpis=kpis, n_kpi=65)
        refused(b"n_kpi = -1", kpis=kpis, n_kpi=-1)
        refused(b"not the fold", R=big.R)
        refused(b"no policy uploaded", policy=1)
        refused(b"exactly one of omega_seq and start", om=None)
        with pytest.raises(ValueError, match="at most 64"):
            p.rollout(c.R, u_seq=u_seq, omega_seq=om65, risk=RiskTable().add("c", "cost"))
        again = p.rollout(c.R, u_seq=u_seq, omega_seq=om_seq, step=STEP, kpis=kpis, risk=risk)      # ... and one good call afterwards still works
        _bits(again["risk"], good["risk"], "after the refusals")
    finally:
        _clean(p)
