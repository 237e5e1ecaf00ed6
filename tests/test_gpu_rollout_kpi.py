"""Rollout KPIs on the device (mld_rollout_kpi / GpuProblem.rollout(kpis=...), kernels k_rollout_kpi and k_rollout_policy_kpi): the campaign's column
statistics (simlog.KpiTable, the rule of mld_sim_log_summary) of every rolled-out trajectory, reduced inside the rollout kernel and optionally priced from
the resident price library.  The yardstick is the route the library already has: per realisation, on a second handle, K logged advancing
sim_step(resolve=R, ...) calls with the stage cost armed at the same price starts, then sim_log_summary -- expected bit for bit, because the rollout equals
the stepwise route in x, v, y on these shapes and seeds (tests/test_gpu_rollout.py, tests/test_gpu_policy_rollout.py: the scenarios below are theirs) and the
KPI rule has one order of operations.  Then simlog.rollout_kpis_np on the same call's trajectories, the priced cost against the weighted cost, every
ending, the untouched handle, the old paths beside the new one, and every refusal.

Shapes (tests/test_gpu_rollout.py): a10 -- n_h 3, three models interleaved, batch 10; a1 -- batch 1; b9 -- n_h 7, batch 9.  S = 3, STEP = 1."""
import ctypes as C

import numpy as np
import pytest

import _rollout_ref
from test_gpu_sim_resolve import SHAPES
from test_gpu_small_lds_step import _SmallCtx
from test_gpu_rollout import _scenario
from test_gpu_policy_rollout import reference, thermostat
from test_gpu_log_summary import _kpis
from pyhybridcontrol_amd import gpu, policy, prices, simlog, _lib
from pyhybridcontrol_amd.simlog import KpiTable

pytestmark = pytest.mark.gpu

S, STEP = 3, 1
N_CHAN = 2
KEYS = simlog.KPI_ROLLOUT_KEYS
SUMM = ("cost", "mu_total", "worst_vio", "worst_step", "steps_done", "end_status")
TRAJ = ("x", "v", "y", "cons_vio", "cons_row")
_CACHE = {}


class _Two(object):
    """a context of tests/test_gpu_rollout.py and a second handle over the same models for the logged stepwise route"""

    def __init__(self, *a, **kw):
        self.c = _SmallCtx(*a, **kw)
        self.q = gpu.GpuProblem(self.c.model, self.c.N - 1, self.c.N, None)

    def close(self):
        self.q.close(); self.c.close()


@pytest.fixture(scope="module")
def ctx():
    def get(name, **kw):
        key = (name,) + tuple(sorted(kw.items()))
        if key not in _CACHE:
            _CACHE[key] = _Two(*SHAPES[name], **kw)
        return _CACHE[key]
    yield get
    for t in _CACHE.values():
        t.close()
    _CACHE.clear()


def _tariff(B, K, seed, n_chan=N_CHAN):
    """(price library, price starts (B,)): three tariffs, each long enough for STEP + K steps"""
    rng = np.random.default_rng(seed)
    return rng.uniform(0.5, 2.0, (STEP + K + 3) * n_chan), ((np.arange(B) % 3) * n_chan).astype(np.int64)


def _clean(*problems):
    for p in problems:
        p.upload_policy(None)
        p.sim_log_begin(0)
        p.upload_profiles(np.zeros(0))
        p.upload_prices(np.zeros(0))


def _bits(got, want, what):
    """every statistic equal in every bit (NaN patterns aside, which compare as NaN)"""
    for k in KEYS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k, got[k].dtype, want[k].dtype, got[k].shape, want[k].shape)
        if got[k].dtype.kind == "f":
            same = (got[k].view(np.uint64) == want[k].view(np.uint64)) | (np.isnan(got[k]) & np.isnan(want[k]))
        else:
            same = got[k] == want[k]
        assert np.all(same), (what, k, int((~same).sum()), got[k][~same][:4], want[k][~same][:4])


def _log_route(t, kpis, u_ref, start, K, plib, pstart, P=None, u_prev=None):
    """the yardstick: per realisation x0 uploaded on the second handle, a log of K records begun and its stage cost armed at the price starts, K logged
    advancing steps (the caller's inputs, or the resident policy's), then sim_log_summary; the statistics stacked (B, S, ...)"""
    c, q = t.c, t.q
    out = {k: [] for k in KEYS}
    q.upload_prices(plib, N_CHAN)
    q.set_stage_cost(w_v=np.ones(c.nv))                                     # any weights: the price record is what the priced KPIs read
    for cc in range(S):
        q.upload(c.x0, c.om, c.midx)
        if P is not None:
            q.policy_state(u_prev)
        q.sim_log_begin(K)
        q.sim_log_cost_begin(pstart)
        for k in range(K):
            kw = dict(policy=True) if P is not None else dict(u0=np.ascontiguousarray(u_ref[:, k]))
            o = q.sim_step(resolve=c.R, act_start=np.ascontiguousarray(start[:, cc]), step=STEP + k, advance=True, outputs=True, **kw)
            assert o["n_skipped"] == 0 and np.all(o["aux_status"] == 0)
        s = q.sim_log_summary(kpis)
        assert np.all(s["n_stepped"] == K)
        for k in KEYS:
            out[k].append(s[k])
    return {k: np.stack(out[k], axis=1) for k in KEYS}


@pytest.mark.parametrize("mode", ["one", "plan", "long"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_against_the_log_route_bit_for_bit(ctx, shape, mode):
    """K = 1; K = N_tilde with the resident plan's inputs (u_seq=None); K = N_tilde + 2 with the caller's u_seq.  No tolerance: the rollout's x, v, y equal the
    stepwise route's on these scenarios and the KPI rule has one order of operations."""
    t = ctx(shape)
    c, p, q = t.c, t.c.p, t.q
    K = dict(one=1, plan=c.N, long=c.N + 2)[mode]
    lib, gw, start, om_seq, u_seq = _scenario(c, K, 9100 + 10 * list(SHAPES).index(shape) + K)
    plib, pstart = _tariff(c.B, K, 9150 + K)
    kpis = _kpis(c, 9160)
    try:
        p.upload(c.x0, c.om, c.midx)
        p.upload_profiles(lib, gw); q.upload_profiles(lib, gw)
        p.upload_prices(plib, N_CHAN)
        if mode == "plan":
            p.solve_resident()
            plan = p.download()
            assert np.all(np.isin(plan["status"], (0, 2)) & np.isfinite(plan["obj"]))
            u_ref = np.ascontiguousarray(plan["v"].reshape(c.B, c.N, c.nv)[:, :K, :c.nu])
        else:
            u_ref = u_seq
        assert np.all(np.abs(_rollout_ref.closed_y(c.mats, c.d, c.midx, u_ref, om_seq)) >= 1e-3)      # (the guard of tests/test_gpu_rollout.py)
        got = p.rollout(c.R, u_seq=None if mode == "plan" else u_seq, start=start, step=STEP, kpis=kpis, price_start=pstart)
        assert np.all(got["end_status"] == 0) and got["stats"]["complete"] == c.B * S      # the comparison cannot pass on NaN alone
        kp = got["kpi"]
        assert kp["names"] == kpis.names and kp["sum"].shape == (c.B, S, len(kpis)) and kp["n_vio"].shape == (c.B, S) and kp["n_vio"].dtype == np.int32
        assert np.all(np.isfinite(kp["sum"])) and np.abs(kp["sum"]).max() > 0
        assert np.all((kp["min_step"] >= 0) & (kp["min_step"] < K) & (kp["max_step"] >= 0) & (kp["max_step"] < K))      # step indices k, not STEP + k
        ref = _log_route(t, kpis, u_ref, start, K, plib, pstart)
        _bits(kp, ref, "%s %s" % (shape, mode))
    finally:
        _clean(p, q)


@pytest.mark.parametrize("mode", ["one", "long"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_policy_against_the_log_route_bit_for_bit(ctx, shape, mode):
    """the closed loop of the thermostat against K logged sim_step(resolve=R, policy=True) calls, under the threshold guard of
    tests/test_gpu_policy_rollout.py.  u_prev is the rule's own step-0 input, so that no channel switches at step 0 and the switch count is the sum of the
    u_j KPIs' n_changes (which count from the second record on)."""
    t = ctx(shape)
    c, p, q = t.c, t.c.p, t.q
    K = dict(one=1, long=c.N + 2)[mode]
    lib, gw, start, om_seq, u_seq = _scenario(c, K, 9100 + 10 * list(SHAPES).index(shape) + K)
    plib, pstart = _tariff(c.B, K, 9250 + K)
    kpis = _kpis(c, 9260)
    P = thermostat(c)
    up0 = policy.apply_np(P, c.midx, c.x0, P.initial_state(c.midx), u_seq[:, 0])
    num = reference(c, P, c.x0, u_seq, om_seq, up0)
    try:
        p.upload(c.x0, c.om, c.midx)
        for h in (p, q):
            h.upload_profiles(lib, gw)
            h.upload_policy(P)
        p.upload_prices(plib, N_CHAN)
        got = p.rollout(c.R, K=K, start=start, step=STEP, policy=True, u_prev=up0, kpis=kpis, price_start=pstart)
        assert np.all(got["end_status"] == 0) and np.array_equal(got["switches"], num["switches"])
        kp = got["kpi"]
        ref = _log_route(t, kpis, None, start, K, plib, pstart, P=P, u_prev=up0)
        _bits(kp, ref, "%s %s" % (shape, mode))
        ruled = [kpis.names.index("u_%d" % j) for j in range(c.nu)]          # every channel is ruled
        assert np.array_equal(kp["n_changes"][:, :, ruled].sum(axis=2), got["switches"])
        if mode == "long":
            assert got["switches"].max() > 0
    finally:
        _clean(p, q)


def _sixty_four(c, seed, priced):
    """tests/test_gpu_log_summary.py::test_one_kpi_and_sixty_four's table: every subset of the five tables, then pairs"""
    rng = np.random.default_rng(seed)
    M, d = len(c.mats), c.d
    full = KpiTable(M, d)
    keys, widths = simlog.KPI_TABLES, (d["nx"], c.nv, d["ny"], d["nomega"], d["nx"])
    for q in range(64):
        use = [i for i in range(5) if (q + 1) >> i & 1] if q < 31 else [q % 5, (q + 2) % 5]
        full.add("k%d" % q, price_chan=q % 2 if priced and q % 3 == 0 else None, thresh=float(rng.normal()),
                 **{keys[i]: rng.standard_normal((M, widths[i])) for i in use})
    return full


@pytest.mark.parametrize("priced", [False, True])
@pytest.mark.parametrize("n_kpi", [1, 64])
@pytest.mark.parametrize("shape", ["a10", "b9"])
def test_against_the_numpy_rule(ctx, shape, n_kpi, priced):
    """simlog.rollout_kpis_np on the SAME call's trajectories: bit for bit, at one KPI and at MLD_KPI_MAX"""
    t = ctx(shape)
    c, p = t.c, t.c.p
    K = c.N + 2
    _, _, _, om_seq, u_seq = _scenario(c, K, 9300 + list(SHAPES).index(shape))
    plib, pstart = _tariff(c.B, K, 9350)
    if n_kpi == 1:
        kpis = KpiTable(len(c.mats), c.d).add("z", w_v=np.eye(c.nv)[c.d["nu"] + c.d["ndelta"]], price_chan=1 if priced else None, thresh=100.0)
    else:
        kpis = _sixty_four(c, 9360, priced)
    x0 = c.x0.copy()
    x0[0, 0] = 47.0                                                          # slack somewhere: cons_vio above the tolerance
    try:
        p.upload(x0, c.om, c.midx)
        if priced:
            p.upload_prices(plib, N_CHAN)
        got = p.rollout(c.R, u_seq=u_seq, omega_seq=om_seq, step=STEP, trajectories=True, kpis=kpis, price_start=pstart if priced else None)
        assert np.all(got["end_status"] == 0)
        price = prices.windows(plib, pstart, STEP, K, N_CHAN).reshape(c.B, K, N_CHAN) if priced else None
        ref = simlog.rollout_kpis_np(got, kpis, price=price, omega_seq=om_seq, model_idx=c.midx)
        _bits(got["kpi"], ref, (shape, n_kpi, priced))
        assert (got["kpi"]["n_vio"] > 0).any() and (got["kpi"]["n_vio"] == 0).any()
        tight = p.rollout(c.R, u_seq=u_seq, omega_seq=om_seq, step=STEP, kpis=kpis, price_start=pstart if priced else None, vio_tol=-1.0)
        assert np.all(tight["kpi"]["n_vio"] == (got["cons_vio"] > -1.0).sum(axis=2))
    finally:
        _clean(p)


def test_priced_cost_equals_weighted_cost(ctx):
    """w_v = e_z priced on channel 0 of a one-channel library is cost with cost_w[k] = price_k e_z.  Both round price_k z_k once and add over k ascending, but
    cost sums a step's products over the lanes (a butterfly) before it adds them to the running sum, and its products may be contracted into that lane sum:
    the two are equal only where these roundings coincide.  So the KPI is asserted bit for bit against the numpy rule, and against cost within
    K 2^-52 sum_k |price_k z_k| -- one rounding per product and per addition either way."""
    t = ctx("a10")
    c, p = t.c, t.c.p
    K = c.N + 2
    _, _, _, om_seq, u_seq = _scenario(c, K, 9400)
    plib, pstart = _tariff(c.B, K, 9450, n_chan=1)
    z = c.d["nu"] + c.d["ndelta"]
    kpis = KpiTable(len(c.mats), c.d).add("cost", w_v=np.eye(c.nv)[z], price_chan=0)
    price = prices.windows(plib, pstart, STEP, K, 1).reshape(c.B, K)
    cw = np.zeros((c.B, K, c.nv))
    cw[:, :, z] = price
    try:
        p.upload(c.x0, c.om, c.midx)
        p.upload_prices(plib, 1)
        got = p.rollout(c.R, u_seq=u_seq, omega_seq=om_seq, step=STEP, cost_w=cw, trajectories=True, kpis=kpis, price_start=pstart)
        assert np.all(got["end_status"] == 0) and np.abs(got["cost"]).max() > 0
        _bits(got["kpi"], simlog.rollout_kpis_np(got, kpis, price=price[:, :, None], model_idx=c.midx), "priced cost")
        terms = np.abs(price[:, None, :] * got["v"][..., z]).sum(axis=2)
        dev = np.abs(got["kpi"]["sum"][:, :, 0] - got["cost"])
        print("priced-cost KPI against cost: worst |difference| / bound = %.3g, equal in %d of %d" % ((dev / (K * 2.0 ** -52 * terms)).max(), int((dev == 0).sum()), dev.size))
        assert np.all(dev <= K * 2.0 ** -52 * terms)
    finally:
        _clean(p)


def _raw(p, R, kpis, K, u_seq=None, om_seq=None, pstart=None, policy=0, n_kpi=None, outs=True, vio_tol=1e-6, **over):
    """mld_rollout_kpi itself: (rc, message, dict of outputs); over: w_x .. w_xk1, price_chan, thresh replaced (None = NULL)"""
    arr = dict(kpis.arrays())
    arr.update(over)
    B, Q = p.batch, len(kpis)
    dp, ip = _lib.dptr, lambda a: a.ctypes.data_as(C.POINTER(C.c_int32)) if a is not None else None
    lp = lambda a: a.ctypes.data_as(C.POINTER(C.c_int64)) if a is not None else None
    keep = [None if arr[k] is None else np.ascontiguousarray(arr[k], dtype=np.float64) for k in simlog.KPI_TABLES]
    chan = None if arr["price_chan"] is None else np.ascontiguousarray(arr["price_chan"], dtype=np.int32)
    thr = None if arr["thresh"] is None else np.ascontiguousarray(arr["thresh"], dtype=np.float64)
    o = dict(end_status=np.full((B, S), -7, np.int32), stats=np.zeros(4, np.int64))
    if outs:
        o.update(sum=np.full((B, S, Q), -7.0), min=np.full((B, S, Q), -7.0), max=np.full((B, S, Q), -7.0), min_step=np.full((B, S, Q), -7, np.int32),
                 max_step=np.full((B, S, Q), -7, np.int32), n_above=np.full((B, S, Q), -7, np.int32), n_changes=np.full((B, S, Q), -7, np.int32),
                 n_vio=np.full((B, S), -7, np.int32))
    lib = _lib.load()
    rc = lib.mld_rollout_kpi(p._h, R.problem._h, policy, K, S, dp(u_seq), None, dp(om_seq), None, STEP, None, 0, Q if n_kpi is None else n_kpi,
                             *([dp(a) for a in keep] + [ip(chan), dp(thr), float(vio_tol), lp(pstart)]),
                             None, None, None, None, None, None, None, None, None, None, ip(o["end_status"]), None, lp(o["stats"]),
                             dp(o.get("sum")), dp(o.get("min")), dp(o.get("max")), ip(o.get("min_step")), ip(o.get("max_step")), ip(o.get("n_above")),
                             ip(o.get("n_changes")), ip(o.get("n_vio")))
    return rc, lib.mld_last_error(), o


def _blank(kp, at):
    return all(np.all(np.isnan(kp[k][at])) if kp[k].dtype.kind == "f" else np.all(kp[k][at] == -1) for k in KEYS)


def test_endings(ctx):
    # infeasible auxiliaries at a known step (the fixture of tests/test_gpu_rollout.py::test_endings): NaN / -1 for those trajectories only
    t = ctx("a10", hard=True)
    c, p = t.c, t.c.p
    B, K = c.B, 4
    _, _, _, om_seq, _ = _scenario(c, K, 9500)
    fn = _rollout_ref.closed_form_resolver(c.mats, c.d)
    hot, heat = np.arange(B) % 3 == 1, np.arange(B) % 3 == 2
    x0 = c.x0.copy()
    x0[hot, 0] = 90.0
    u_seq = np.zeros((B, K, c.nu))
    u_seq[heat, 1, 0] = 1.0
    for b in np.where(heat)[0]:
        for t0 in np.arange(80.0, 55.0, -0.25):
            x0[b, 0] = t0
            r = simlog.rollout_np(c.mats, c.d, c.midx[b:b + 1], x0[b:b + 1], u_seq[b:b + 1], om_seq[b:b + 1], fn)
            if np.all(r["end_status"] == 1) and np.all(r["steps_done"] == 2):
                break
    M, d = len(c.mats), c.d
    rng = np.random.default_rng(9510)
    hard = KpiTable(M, d).add("x", w_x=rng.standard_normal(d["nx"]), thresh=0.0).add("vy", w_v=rng.standard_normal(c.nv), w_y=np.ones(d["ny"]))
    hard.add("xk1", w_xk1=rng.standard_normal((M, d["nx"])))
    p.upload(x0, c.om, c.midx)
    got = p.rollout(c.R, u_seq=u_seq, omega_seq=om_seq, trajectories=True, kpis=hard)
    dead = np.broadcast_to((hot | heat)[:, None], (B, S))
    assert np.array_equal(got["end_status"] == 1, dead) and np.all(got["end_status"][~dead] == 0)
    assert np.all(got["steps_done"][heat] == 2) and np.all(got["steps_done"][hot] == 0)
    kp = got["kpi"]
    assert _blank(kp, dead) and np.all(np.isfinite(kp["sum"][~dead])) and np.all(kp["n_vio"][~dead] >= 0) and np.all(kp["min_step"][~dead] >= 0)
    _bits(kp, simlog.rollout_kpis_np(got, hard, model_idx=c.midx), "beside infeasible trajectories")

    # the resolver's pivot budget capped: every trajectory ends 2 in the C call with NaN / -1; rollout() completes them on the host and its KPIs are the numpy rule's
    s = ctx("a10")
    c, p = s.c, s.c.p
    K = c.N
    _, _, _, om_seq, u_seq = _scenario(c, K, 9600)
    plib, pstart = _tariff(B, K, 9650)
    kpis = _kpis(c, 9660)
    try:
        p.upload(c.x0, c.om, c.midx)
        p.upload_prices(plib, N_CHAN)
        want = p.rollout(c.R, u_seq=u_seq, omega_seq=om_seq, step=STEP, kpis=kpis, price_start=pstart)
        assert want["stats"]["declined"] == 0 and np.all(want["end_status"] == 0)
        c.R.problem.set_opts(reserved=_lib.MLD_DBG_SMALL_PIVOT_CAP)
        try:
            rc, msg, o = _raw(p, c.R, kpis, K, u_seq, om_seq, pstart)
            assert rc == 0, msg
            assert np.all(o["end_status"] == 2) and list(o["stats"]) == [B * S, 0, 0, B * S] and _blank(o, np.ones((B, S), bool))
            for full in (True, False):
                got = p.rollout(c.R, u_seq=u_seq, omega_seq=om_seq, step=STEP, trajectories=full, kpis=kpis, price_start=pstart)
                assert got["stats"]["finished_on_host"] == B * S and np.all(got["end_status"] == 0) and ("x" in got) == full
                if full:
                    price = prices.windows(plib, pstart, STEP, K, N_CHAN).reshape(B, K, N_CHAN)
                    host = simlog.rollout_kpis_np(got, kpis, price=price, omega_seq=om_seq, model_idx=c.midx)
                    _bits(got["kpi"], host, "finished on the host")
                else:
                    _bits(got["kpi"], host, "finished on the host, summaries only")
            # the host-finished figures are the device's up to the completion's own deviation in x, v (tests/test_gpu_rollout.py::test_host_completion: 1e-6)
            assert np.all(np.abs(host["sum"] - want["kpi"]["sum"]) <= 1e-6 * K * np.maximum(1.0, np.abs(want["kpi"]["sum"])))
        finally:
            c.R.problem.set_opts(reserved=0)

        # instances without a usable plan with u_seq=None: not attempted, NaN / -1
        first = p.solve(c.x0, c.om, c.midx)
        assert np.all(first["status"] == 0)
        p.upload(c.x0, c.om, c.midx)
        masked = np.arange(B) % 2 == 1
        cut = np.full(B, np.inf)
        cut[masked] = (first["obj"] - 1e-6 * np.maximum(1.0, np.abs(first["obj"])))[masked]
        p.set_cutoffs(cut)
        p.solve_resident()
        assert np.all(p.download()["status"][masked] == 1)
        got = p.rollout(c.R, omega_seq=om_seq, step=STEP, trajectories=True, kpis=kpis, price_start=pstart)
        assert np.all(got["end_status"][masked] == -1) and np.all(got["end_status"][~masked] == 0)
        m2 = np.broadcast_to(masked[:, None], (B, S))
        assert _blank(got["kpi"], m2) and np.all(np.isfinite(got["kpi"]["sum"][~m2]))
        price = prices.windows(plib, pstart, STEP, K, N_CHAN).reshape(B, K, N_CHAN)
        _bits(got["kpi"], simlog.rollout_kpis_np(got, kpis, price=price, omega_seq=om_seq, model_idx=c.midx), "beside instances without a plan")
    finally:
        p.set_cutoffs(np.full(B, np.inf))
        _clean(p)


def test_the_handle_is_untouched_and_the_old_paths_are(ctx):
    t = ctx("a10")
    c, p = t.c, t.c.p
    K = c.N
    lib, gw, start, om_seq, u_seq = _scenario(c, K, 9700)
    plib, pstart = _tariff(c.B, K, 9750)
    kpis = _kpis(c, 9760)
    P = thermostat(c)
    rng = np.random.default_rng(9770)
    cw = rng.uniform(0.5, 2.0, size=(c.B, K, c.nv))
    try:
        p.upload(c.x0, c.om, c.midx)
        p.upload_profiles(lib, gw)
        p.upload_prices(plib, N_CHAN)
        p.upload_policy(P)
        p.sim_log_begin(2)
        p.solve_resident()
        p.warm_start_from_previous()
        u_state = p.policy_state((rng.uniform(size=(c.B, c.nu)) < 0.5).astype(float))
        astart = np.ascontiguousarray(start[:, 0])
        before_step = p.sim_step(act_start=astart, step=STEP, advance=False, log=False, outputs=True)      # (makes the actual starts resident)
        before = (p.inputs(), p.download(), p.sim_log_count(), p.debug_warm_start())
        assert before[3] is not None
        old = {pol: p.rollout(c.R, u_seq=u_seq, start=start, step=STEP, cost_w=cw, trajectories=True, policy=pol) for pol in (False, True)}
        for pol in (False, True):
            new = p.rollout(c.R, u_seq=u_seq, start=start, step=STEP, cost_w=cw, trajectories=True, policy=pol, kpis=kpis, price_start=pstart)
            again = p.rollout(c.R, u_seq=u_seq, start=start, step=STEP, cost_w=cw, trajectories=True, policy=pol)
            for k in SUMM + TRAJ + (("switches",) if pol else ()):      # the old path beside the new one, and the new one's old outputs: the same bits
                assert np.array_equal(old[pol][k], again[k], equal_nan=True) and np.array_equal(old[pol][k], new[k], equal_nan=True), (pol, k)
            assert "kpi" not in again and old[pol]["stats"] == new["stats"] == again["stats"]
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
    t, big = ctx("a10"), ctx("b9")
    c, p = t.c, t.c.p
    B, K = c.B, c.N
    M, d = len(c.mats), c.d
    lib, gw, start, om_seq, u_seq = _scenario(c, K, 9800)
    plib, pstart = _tariff(B, K, 9850)
    kpis = _kpis(c, 9860)
    try:
        p.upload(c.x0, c.om, c.midx)
        p.upload_prices(plib, N_CHAN)
        p.solve_resident()
        state = (p.inputs(), p.download())
        good = p.rollout(c.R, u_seq=u_seq, omega_seq=om_seq, step=STEP, kpis=kpis, price_start=pstart)

        def unchanged(what):
            x_in, w_in = p.inputs()
            assert np.array_equal(x_in, state[0][0]) and np.array_equal(w_in, state[0][1]), what
            now = p.download()
            for k in now:
                assert np.array_equal(now[k], state[1][k], equal_nan=True), (what, k)

        def refused(word, ps=pstart, table=kpis, **kw):
            rc, msg, o = _raw(p, c.R, table, K, u_seq, om_seq, ps, **kw)
            assert rc == -1 and b"mld_rollout_kpi" in msg and word in msg, (word, rc, msg)
            assert np.all(o["sum"] == -7.0) and np.all(o["n_vio"] == -7) and np.all(o["end_status"] == -7), word      # nothing was written
            unchanged(word)

        refused(b"n_kpi = 0", n_kpi=0)
        refused(b"n_kpi = 65", n_kpi=65)
        refused(b"are all NULL", w_x=None, w_v=None, w_y=None, w_omega=None, w_xk1=None)
        bad = kpis.arrays()["w_v"].copy()
        bad[1, 2, 3] = np.inf
        refused(b"w_v of model 1, KPI 2, entry 3 is not finite", w_v=bad)
        thr = kpis.arrays()["thresh"].copy()
        thr[2, 1] = np.nan
        refused(b"thresh of model 2, KPI 1 is NaN", thresh=thr)
        refused(b"vio_tol is NaN", vio_tol=np.nan)
        chan = kpis.arrays()["price_chan"].copy()
        q_priced = int(np.flatnonzero(chan >= 0)[0])
        for val, word in ((-2, b"price_chan[0] = -2"), (N_CHAN, b"price_chan[0] = %d" % N_CHAN)):
            ch = chan.copy()
            ch[0] = val
            refused(word, price_chan=ch)
        refused(b"price_chan[%d] = %d, but price_start is NULL" % (q_priced, chan[q_priced]), ps=None)
        out = pstart.copy()
        out[B - 1] = plib.size - (STEP + K) * N_CHAN + 1                       # one double past the last valid start
        refused(b"price start %d of instance %d" % (out[B - 1], B - 1), ps=out)
        out[B - 1] = -1
        refused(b"leaves the price library", ps=out)
        out = pstart.copy()
        out[3], out[7] = -5, -6
        refused(b"price start -5 of instance 3", ps=out)                       # the first offender is named
        # a priced KPI without a price library
        p.upload_prices(np.zeros(0))
        refused(b"no price library is resident")
        with pytest.raises(ValueError, match="no price library|priced"):
            p.rollout(c.R, u_seq=u_seq, omega_seq=om_seq, kpis=kpis)
        p.upload_prices(plib, N_CHAN)
        # every refusal of the rollout applies by the same code
        rc, msg, _ = _raw(p, big.c.R, kpis, K, u_seq, om_seq, pstart)
        assert rc == -1 and b"mld_rollout_kpi" in msg and b"not the fold" in msg
        rc, msg, _ = _raw(p, c.R, kpis, K, u_seq, om_seq, pstart, policy=1)
        assert rc == -1 and b"no policy uploaded" in msg
        rc, msg, _ = _raw(p, c.R, kpis, K, u_seq, None, pstart)
        assert rc == -1 and b"exactly one of omega_seq and start" in msg
        unchanged("the rollout's own refusals")
        # the Python wrapper's checks, before any C call
        with pytest.raises(ValueError, match="price_start is None"):
            p.rollout(c.R, u_seq=u_seq, omega_seq=om_seq, kpis=kpis)
        with pytest.raises(ValueError, match="price_start given without kpis"):
            p.rollout(c.R, u_seq=u_seq, omega_seq=om_seq, price_start=pstart)
        with pytest.raises(ValueError, match="has %d models" % (M + 1)):
            p.rollout(c.R, u_seq=u_seq, omega_seq=om_seq, kpis=KpiTable(M + 1, d).add("x", w_x=np.ones(d["nx"])))
        with pytest.raises(ValueError, match="other dimensions"):
            p.rollout(c.R, u_seq=u_seq, omega_seq=om_seq, kpis=KpiTable(M, dict(d, nx=d["nx"] + 1)).add("x", w_x=np.ones(d["nx"] + 1)))
        with pytest.raises(ValueError, match="expected integers"):
            p.rollout(c.R, u_seq=u_seq, omega_seq=om_seq, kpis=kpis, price_start=pstart.astype(float))
        # the price-window edges are valid: s = 0 and s = lib_len - (step + K) n_chan
        edge = np.zeros(B, np.int64)
        edge[B - 1] = plib.size - (STEP + K) * N_CHAN
        at_edge = p.rollout(c.R, u_seq=u_seq, omega_seq=om_seq, step=STEP, trajectories=True, kpis=kpis, price_start=edge)
        price = prices.windows(plib, edge, STEP, K, N_CHAN).reshape(B, K, N_CHAN)
        _bits(at_edge["kpi"], simlog.rollout_kpis_np(at_edge, kpis, price=price, omega_seq=om_seq, model_idx=c.midx), "the window's edges")
        again = p.rollout(c.R, u_seq=u_seq, omega_seq=om_seq, step=STEP, kpis=kpis, price_start=pstart)   # ... and one good call afterwards still works
        _bits(again["kpi"], good["kpi"], "after the refusals")
        for k in SUMM:
            assert np.array_equal(again[k], good[k], equal_nan=True), k
    finally:
        _clean(p)


def test_refusals_of_a_model_without_outputs_and_of_the_staging():
    """w_y for a model without outputs; and a model whose staging fits a wave's share of LDS (2048 doubles) with one KPI's accumulators but not with 64:
    2 nx + nomega + nu + nv = 4 + 62 + 800 + 800 = 1666 doubles, + 6 n_kpi (a narrow model otherwise: one state pair, one constraint row)"""
    import _paths
    dims = dict(nx=2, nu=800, nomega=62, ny=0, nc=1)
    d = _paths.make_dims(**dims)
    mats = [_paths.random_mld(9910, rho=0.9, **dims)[0]]
    model = gpu.GpuModel(mats, d)
    p = gpu.GpuProblem(model, 1, 2, None)
    try:
        rng = np.random.default_rng(9911)
        B, K = 3, 2
        x0, om = rng.standard_normal((B, 2)), rng.standard_normal((B, 2 * 62))
        u_seq, om_seq = rng.standard_normal((B, K, 800)), rng.standard_normal((B, S, K, 62))
        p.upload(x0, om)
        one = KpiTable(1, d).add("x", w_x=np.ones(2)).add("u_sum", w_v=np.ones(800), w_omega=rng.standard_normal(62), thresh=0.0)
        got = p.rollout(None, u_seq=u_seq, omega_seq=om_seq, trajectories=True, kpis=one)
        assert np.all(got["end_status"] == 0)
        _bits(got["kpi"], simlog.rollout_kpis_np(got, one, omega_seq=om_seq), "no auxiliaries, a staging of 1678 doubles")
        lib = _lib.load()
        es = np.full((B, S), -7, np.int32)

        def raw(n_kpi, w_x, w_y):
            return lib.mld_rollout_kpi(p._h, None, 0, K, S, _lib.dptr(u_seq), None, _lib.dptr(om_seq), None, 0, None, 0, n_kpi, _lib.dptr(w_x), None, _lib.dptr(w_y),
                                       None, None, None, None, 1e-6, None, None, None, None, None, None, None, None, None, None, None,
                                       es.ctypes.data_as(C.POINTER(C.c_int32)), None, None, None, None, None, None, None, None, None, None)
        assert raw(1, np.ones(2), np.ones(1)) == -1 and b"w_y given but the model has none of that variable" in lib.mld_last_error()
        assert raw(64, np.ones((1, 64, 2)), None) == -1
        msg = lib.mld_last_error()
        assert b"mld_rollout_kpi: the staging of a trajectory (%d bytes" % (8 * (1666 + 6 * 64)) in msg and b"does not fit a wave's share of LDS" in msg
        assert np.all(es == -7)
        assert raw(1, np.ones(2), None) == 0 and np.all(es == 0)
        with pytest.raises(ValueError, match="w_y given but the model has none"):
            KpiTable(1, d).add("y", w_y=np.ones(1))
    finally:
        p.close(); model.close()
