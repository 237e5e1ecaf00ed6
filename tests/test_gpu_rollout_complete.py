"""Device completion of declined rollout trajectories (mld_set_rollout_completion / complete="device"; kernels k_ro_collect, k_rollout_redo[_kpi],
k_ro_fix_merge): a trajectory the LDS solver declines is re-run from step 0 on the device, its declined steps answered by the dense kernel on the resolver's
handle, before anything reads its result.  MLD_DBG_SMALL_PIVOT_CAP on the resolver makes the LDS solver decline on demand -- most steps, not all: a step two
pivots answer stays the LDS solver's, so what the rollout kernel declined is read from the C call itself (_first) before it is expected.  The yardsticks are the routes the
library already has: the stepwise route and the host completion within the project's 1e-6 max(1, |reference|) (tests/test_gpu_rollout.py::_against_stepwise: the
summation order of the right-hand side differs), and bit for bit a dense-kernel resolver fed from the host for every dense step, sim_step(v0=v_k) for every plant
row, and the numpy rules for KPIs, risk, choice and MIP start on the completed arrays.

Shapes (tests/test_gpu_sim_resolve.py): a10 -- n_h 3, three models interleaved, N_tilde 3, batch 10; b9 -- n_h 7, batch 9."""
import ctypes as C

import numpy as np
import pytest

import _rollout_ref
from test_gpu_sim_resolve import SHAPES
from test_gpu_small_lds_step import _SmallCtx
from test_gpu_log_summary import _kpis
from test_gpu_rollout import S, STEP, SUMM, TRAJ, _against_stepwise, _by_sim_step, _raw, _same_plant_rows, _scenario, _stepwise
from test_gpu_rollout_kpi import N_CHAN, _tariff
from test_gpu_policy_rollout import thermostat
from test_gpu_plan_select import _table
from pyhybridcontrol_amd import prices, simlog, _lib
from pyhybridcontrol_amd._lib import MldGpuError
from pyhybridcontrol_amd.aux_resolve import BatchAuxResolver
from pyhybridcontrol_amd.simlog import PlanSelector

pytestmark = pytest.mark.gpu

CAP = _lib.MLD_DBG_SMALL_PIVOT_CAP
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


class _capped(object):
    """the resolver's LDS pivot budget capped inside the block; the stepped handle's completion mode back at 0 behind it"""

    def __init__(self, c, mode=0):
        self.c, self.mode = c, mode

    def __enter__(self):
        self.c.R.problem.set_opts(reserved=CAP)
        if self.mode:
            self.c.p.set_rollout_completion(self.mode)

    def __exit__(self, *exc):
        self.c.R.problem.set_opts(reserved=0)
        self.c.p.set_rollout_completion(0)


def _bits(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, (what, a.dtype, b.dtype, a.shape, b.shape)
    ok = ((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))) if a.dtype.kind == "f" else a == b
    assert np.all(ok), (what, int((~ok).sum()), a[~ok][:4], b[~ok][:4])


def _dev_stats(n, nd, rounds, infeasible=0, not_attempted=0):
    """stats of a complete="device" call over n trajectories of which the rollout kernel declined nd"""
    return dict(trajectories=n, complete=n - infeasible - not_attempted, infeasible=infeasible, declined=nd, not_attempted=not_attempted, finished_on_host=0,
                finished_on_device=nd, completion_rounds=rounds)


def _first(c, K, u_seq, om_seq):
    """what the rollout kernel alone does under the caller's cap (the C call, mode 0): (declined mask (B, S), the step each declined at, their number)"""
    rc, es, sd, stats = _raw(c.p, c.R, K, u_seq, om_seq)
    assert rc == 0 and int((es == 2).sum()) == int(stats[3]) > 0 and int(stats[1] + stats[2] + stats[3]) == c.B * S
    return es == 2, sd, int(stats[3])


def _rounds_and_solves(cs, nd, sd, declined, K):
    """the completion's own counts: a round per dense phase, at least one dense solve per declined trajectory and at most one per step from its first decline on"""
    most = int((K - sd[declined]).sum())
    assert cs["finished_on_device"] == nd and cs["left_declined"] == 0 and nd <= cs["dense_solves"] <= most and 1 <= cs["rounds"] <= K, cs
    assert cs["rounds"] <= cs["dense_solves"] and (cs["dense_solves"] < most or cs["rounds"] == int((K - sd[declined]).max())), cs
    return cs["dense_solves"] == most      # every step from the first decline on was the dense kernel's


def _chain(c, got, u_seq, om_seq, dense, what):
    """bit for bit: every step the dense solver is known to have answered (dense (B, S, K) bool) against a dense-kernel resolver fed from the host with the
    state and inputs the trajectory had, every step's plant rows against sim_step(v0=v_k, advance=False)"""
    B, n_real, K = got["v"].shape[:3]
    T = B * n_real
    midx = np.repeat(c.midx, n_real)
    D = BatchAuxResolver(c.mats, c.d)      # (no MLD_SMALL_LDS: k_solve answers every row)
    try:
        assert dense[:, :, 0].any(), what
        for k in range(K):
            m = dense[:, :, k].reshape(T)
            if m.any():
                r = D.resolve(got["x"][:, :, k].reshape(T, -1), np.repeat(u_seq[:, k], n_real, axis=0), om_seq[:, :, k].reshape(T, -1), midx)
                assert np.all(r["status"][m] == 0), (what, k)
                _bits(got["v"][:, :, k, c.nu:].reshape(T, -1)[m], r["v"][m], (what, "the dense kernel fed from the host, step", k))
    finally:
        D.close()
    _same_plant_rows(got, _by_sim_step(c.p, got, om_seq, c.om, c.midx), what)


def _dense_mask(declined, sd, K, every):
    """(B, S, K): the step a declined trajectory first declined at, and with `every` each step behind it"""
    k = np.arange(K)[None, None, :]
    return declined[:, :, None] & ((k >= sd[:, :, None]) if every else (k == sd[:, :, None]))


@pytest.mark.parametrize("shape,K,seed", [("a10", 1, 9111), ("a10", 2, 9112), ("a10", 3, 9600), ("b9", 2, 9123)])
def test_every_step_dense(ctx, shape, K, seed):
    """1: every trajectory the rollout kernel declined ends 0, after at most K rounds -- exactly K where every step behind the first decline was dense;
    against the stepwise route under the same cap and against the host completion.  Seed 9600 at K = N_tilde draws the inputs of
    tests/test_gpu_rollout.py::test_host_completion."""
    c = ctx(shape)
    p, B = c.p, c.B
    lib, gw, start, om_seq, u_seq = _scenario(c, K, seed)
    assert np.all(np.abs(_rollout_ref.closed_y(c.mats, c.d, c.midx, u_seq, om_seq)) >= 1e-3)
    try:
        p.upload(c.x0, c.om, c.midx)
        p.upload_profiles(lib, gw)
        with _capped(c):
            declined, sd, nd = _first(c, K, u_seq, om_seq)
            print("%s K = %d: the rollout kernel declined %d of %d trajectories" % (shape, K, nd, B * S))
            got = p.rollout(c.R, u_seq=u_seq, start=start, step=STEP, trajectories=True, complete="device")
            cs = p.rollout_completion_stats()
            print("completion:", cs)
            assert got["stats"] == _dev_stats(B * S, nd, cs["rounds"]), got["stats"]
            _rounds_and_solves(cs, nd, sd, declined, K)
            assert np.all(got["end_status"] == 0) and np.all(got["steps_done"] == K)
            host = p.rollout(c.R, u_seq=u_seq, start=start, step=STEP, trajectories=True, complete="host")
            assert host["stats"] == dict(trajectories=B * S, complete=B * S, infeasible=0, declined=nd, not_attempted=0, finished_on_host=nd)
            _against_stepwise(c, got, dict(host, aux_status=np.zeros(1, np.int32)), K, "%s K = %d against the host completion" % (shape, K))
            c.in_lds = lambda n=None: None      # (the stepwise route under the cap is answered by the dense kernel: that is the point)
            try:
                ref = _stepwise(c, u_seq, start, K)
            finally:
                del c.in_lds
            _against_stepwise(c, got, ref, K, "%s K = %d against the stepwise route" % (shape, K))
    finally:
        p.upload_profiles(np.zeros(0))


@pytest.mark.parametrize("shape,K,n_real", [("a10", 3, 3), ("b9", 2, 1)])
def test_the_chain_bit_for_bit(ctx, shape, K, n_real):
    """2: every dense answer is the resolver's own for the state and inputs the trajectory had, every plant row k_sim_step's"""
    c = ctx(shape)
    p, B = c.p, c.B
    _, _, _, om_seq, u_seq = _scenario(c, K, 9200 + K)
    om_seq = np.ascontiguousarray(om_seq[:, :n_real])
    p.upload(c.x0, c.om, c.midx)
    with _capped(c):
        rc, es, sd, stats = _raw(p, c.R, K, u_seq, np.ascontiguousarray(np.repeat(om_seq, S // n_real, axis=1)))      # (the C helper rolls S realisations out)
        assert rc == 0
        declined, sd, nd = (es == 2)[:, :n_real], sd[:, :n_real], int((es == 2)[:, :n_real].sum())
        assert nd > 0
        got = p.rollout(c.R, u_seq=u_seq, omega_seq=om_seq, trajectories=True, complete="device")
        cs = p.rollout_completion_stats()
        print("%s K = %d: declined %d of %d, completion %s" % (shape, K, nd, B * n_real, cs))
        assert got["stats"] == _dev_stats(B * n_real, nd, cs["rounds"]), got["stats"]
        every = _rounds_and_solves(cs, nd, sd, declined, K)
        _chain(c, got, u_seq, om_seq, _dense_mask(declined, sd, K, every), (shape, K, n_real))


def test_one_dense_step_then_lds(ctx):
    """3: MLD_ROLLOUT_COMPLETE_DBG_FIRST_ONLY -- the cap holds for the rollout kernel and the first re-run only: one round, step 0 dense, the rest in LDS"""
    c = ctx("a10")
    p, B, K = c.p, c.B, c.N
    _, _, _, om_seq, u_seq = _scenario(c, K, 9300)
    x0 = c.x0.copy()
    x0[0, 0] = 47.0
    p.upload(x0, c.om, c.midx)
    want = p.rollout(c.R, u_seq=u_seq, omega_seq=om_seq, trajectories=True)
    assert want["stats"]["declined"] == 0 and np.all(want["end_status"] == 0)
    with _capped(c, _lib.MLD_ROLLOUT_COMPLETE_DBG_FIRST_ONLY):
        c.p.set_rollout_completion(0)
        declined, sd, nd = _first(c, K, u_seq, om_seq)
        c.p.set_rollout_completion(_lib.MLD_ROLLOUT_COMPLETE_DBG_FIRST_ONLY)
        got = p.rollout(c.R, u_seq=u_seq, omega_seq=om_seq, trajectories=True, complete="device")
        assert got["stats"] == _dev_stats(B * S, nd, 1), got["stats"]
        assert p.rollout_completion_stats() == dict(rounds=1, finished_on_device=nd, dense_solves=nd, left_declined=0)      # one dense step each, the rest in LDS
        _chain(c, got, u_seq, om_seq, _dense_mask(declined, sd, K, False), "first only")
    _against_stepwise(c, got, dict(want, aux_status=np.zeros(1, np.int32)), K, "one dense step against the uncapped call")


def test_compaction_and_chunks(ctx):
    """4: a third of the instances without a usable plan (u_seq=None), S = 3: the list is longer than the resolver's batch and is solved in chunks of its models'
    slots; the unattempted trajectories stay -1 and untouched; summaries only equals trajectories=True in every summary bit; the resolver is left as found"""
    c = ctx("a10")
    p, B, K = c.p, c.B, c.N
    first = p.solve(c.x0, c.om, c.midx)
    assert np.all(first["status"] == 0)
    p.upload(c.x0, c.om, c.midx)
    masked = np.arange(B) % 3 == 1
    cut = np.full(B, np.inf)
    cut[masked] = (first["obj"] - 1e-6 * np.maximum(1.0, np.abs(first["obj"])))[masked]
    _, _, _, om_seq, _ = _scenario(c, K, 9400)
    try:
        p.set_cutoffs(cut)
        p.solve_resident()
        assert np.all(p.download()["status"][masked] == 1) and np.all(p.download()["status"][~masked] == 0)
        p.sim_step(resolve=c.R, advance=False, log=False, outputs=True)      # the resolver's resident batch: this handle's size and models
        want = p.rollout(c.R, omega_seq=om_seq, trajectories=True)
        assert want["stats"]["declined"] == 0
        n_no = int(masked.sum()) * S
        r_in, r_out = c.R.problem.inputs(), c.R.problem.download()
        with _capped(c):
            rc, es, sd, stats = _raw(p, c.R, K, None, om_seq)
            nd = int(stats[3])
            print("declined %d of %d attempted trajectories; the resolver has %d slots" % (nd, B * S - n_no, B))
            assert rc == 0 and nd > c.R.problem.batch == B and not (es[masked] == 2).any()
            got = p.rollout(c.R, omega_seq=om_seq, trajectories=True, complete="device")
            cs = p.rollout_completion_stats()
            lean = p.rollout(c.R, omega_seq=om_seq, complete="device")
        _rounds_and_solves(cs, nd, sd, es == 2, K)
        assert got["stats"] == _dev_stats(B * S, nd, cs["rounds"], not_attempted=n_no), got["stats"]
        assert lean["stats"] == got["stats"] and sorted(lean) == sorted(SUMM + ("stats",))
        for k in SUMM:
            _bits(lean[k], got[k], ("summaries only", k))
        assert np.all(got["end_status"][masked] == -1) and np.all(got["steps_done"][masked] == 0) and np.all(got["end_status"][~masked] == 0)
        for k in TRAJ + SUMM:
            _bits(got[k][masked], want[k][masked], ("not attempted: untouched", k))
        _against_stepwise(c, {k: v[~masked] for k, v in got.items() if k != "stats"},
                          dict({k: v[~masked] for k, v in want.items() if k != "stats"}, aux_status=np.zeros(1, np.int32)), K, "completed in chunks against the uncapped call")
        assert c.R.problem.batch == B
        for a, b in zip(r_in + tuple(r_out[k] for k in sorted(r_out)), c.R.problem.inputs() + tuple(c.R.problem.download()[k] for k in sorted(r_out))):
            _bits(a, b, "the resolver's inputs and results are put back")
    finally:
        p.set_cutoffs(np.full(B, np.inf))


def test_endings(ctx):
    """5: the hard model with a tank outside its bounds -- the capped and completed call ends 1 at the step the uncapped call ends 1 at (step 0 and step K - 1),
    NaN / -1 in the same places"""
    c = ctx("a10", hard=True)
    p, B, K = c.p, c.B, 3
    assert c.d["nmu"] == 0 and c.R.nv2 == 2
    _, _, _, om_seq, _ = _scenario(c, K, 9500)
    fn = _rollout_ref.closed_form_resolver(c.mats, c.d)
    hot, heat = np.arange(B) % 3 == 1, np.arange(B) % 3 == 2
    x0 = c.x0.copy()
    x0[hot, 0] = 90.0
    u_seq = np.zeros((B, K, c.nu))
    u_seq[heat, 1, 0] = 1.0                                                 # tank 0 heated during step 1: above T_max at step 2 = K - 1
    for b in np.where(heat)[0]:
        for t0 in np.arange(80.0, 55.0, -0.25):
            x0[b, 0] = t0
            r = simlog.rollout_np(c.mats, c.d, c.midx[b:b + 1], x0[b:b + 1], u_seq[b:b + 1], om_seq[b:b + 1], fn)
            if np.all(r["end_status"] == 1) and np.all(r["steps_done"] == K - 1):
                break
    assert np.all(np.abs(_rollout_ref.closed_y(c.mats, c.d, c.midx, u_seq, om_seq)) >= 1e-3)
    p.upload(x0, c.om, c.midx)
    want = p.rollout(c.R, u_seq=u_seq, omega_seq=om_seq, trajectories=True)
    assert want["stats"]["declined"] == 0
    assert np.all(want["end_status"][hot] == 1) and np.all(want["steps_done"][hot] == 0)
    assert np.all(want["end_status"][heat] == 1) and np.all(want["steps_done"][heat] == K - 1)
    assert np.all(want["end_status"][~hot & ~heat] == 0)
    with _capped(c):
        rc, es, sd, stats = _raw(p, c.R, K, u_seq, om_seq)
        print("hard model: the rollout kernel declined %d of %d trajectories (%d of those that end 1 at step 0, %d of those that end 1 at step K - 1), first at steps %s"
              % (stats[3], B * S, (es[hot] == 2).sum(), (es[heat] == 2).sum(), sorted(set(sd[es == 2].tolist()))))
        assert rc == 0 and stats[3] > 0
        got = p.rollout(c.R, u_seq=u_seq, omega_seq=om_seq, trajectories=True, complete="device")
    n1 = int((hot | heat).sum()) * S
    st = got["stats"]
    assert st["complete"] == B * S - n1 and st["infeasible"] == n1 and st["declined"] == int(stats[3]) == st["finished_on_device"] and st["not_attempted"] == 0
    assert 1 <= st["completion_rounds"] <= K and st["finished_on_host"] == 0
    for k in ("end_status", "steps_done", "worst_step", "cons_row"):
        assert np.array_equal(got[k], want[k]), k
    for k in ("x", "v", "y", "cons_vio", "cost", "mu_total", "worst_vio"):
        assert np.array_equal(np.isnan(got[k]), np.isnan(want[k])), k
        dev = np.abs(got[k] - want[k])[~np.isnan(want[k])] / np.maximum(1.0, np.abs(want[k][~np.isnan(want[k])]))
        assert dev.size and dev.max() <= 1e-6, (k, dev.max())


def test_every_consumer(ctx):
    """6: rollout(policy=True), rollout(kpis=, risk=, per_trajectory=False), select_plan(plan_first=True), select_plan_policies, warm_start_from_rollout"""
    c = ctx("a10")
    p, B, K = c.p, c.B, c.N
    _, _, _, om_seq, u_seq = _scenario(c, K, 9600)
    rng = np.random.default_rng(9601)
    cand = (rng.uniform(size=(B, 2, K, c.nu)) < 0.4).astype(float)
    cw = rng.uniform(0.5, 2.0, size=(K, c.nv))
    up = (rng.uniform(size=(B, c.nu)) < 0.5).astype(float)
    kpis = _kpis(c, 9602, priced=True)
    risk = _table(kpis)
    sel = PlanSelector(risk).minimise("cost", "mean")
    plib, pstart = _tariff(B, K, 9603)
    pol = thermostat(c)
    try:
        p.upload(c.x0, c.om, c.midx)
        p.upload_policy(pol)
        p.upload_prices(plib, N_CHAN)
        p.solve_resident()
        plan_u = np.ascontiguousarray(p.download()["v"].reshape(B, c.N, c.nv)[:, :K, :c.nu])
        forecast = p.inputs()[1]
        with _capped(c):
            # the closed loop: the switches of the host-completed call
            host = p.rollout(c.R, K=K, policy=True, u_prev=up, omega_seq=om_seq, step=STEP, complete="host")
            dev = p.rollout(c.R, K=K, policy=True, u_prev=up, omega_seq=om_seq, step=STEP, complete="device")
            assert host["stats"]["finished_on_host"] == dev["stats"]["finished_on_device"] == dev["stats"]["declined"] > 0 and dev["stats"]["finished_on_host"] == 0
            assert np.all(dev["end_status"] == 0) and np.array_equal(dev["switches"], host["switches"]) and dev["switches"].max() > 0
            # KPIs and risk, nothing per trajectory downloaded: the numpy rules on the same call's trajectories, the priced KPI included
            kw = dict(u_seq=u_seq, omega_seq=om_seq, step=STEP, cost_w=cw, kpis=kpis, price_start=pstart, risk=risk)
            lean = p.rollout(c.R, per_trajectory=False, complete="device", **kw)
            st = lean["stats"]
            assert sorted(lean) == ["risk", "stats"] and st["declined"] > 0 and st == _dev_stats(B * S, st["declined"], st["completion_rounds"]) and 1 <= st["completion_rounds"] <= K
            full = p.rollout(c.R, trajectories=True, complete="device", **kw)
            assert np.all(full["end_status"] == 0) and full["stats"] == st
            price = prices.windows(plib, pstart, STEP, K, N_CHAN).reshape(B, K, N_CHAN)
            kp = simlog.rollout_kpis_np(full, kpis, price=price, omega_seq=om_seq, model_idx=c.midx)
            for k in simlog.KPI_ROLLOUT_KEYS:
                _bits(full["kpi"][k], kp[k], ("kpi", k))
            rk = simlog.rollout_risk_np(full, risk)
            for k in RISK:
                _bits(lean["risk"][k], rk[k], ("risk, nothing per trajectory", k))
                _bits(full["risk"][k], rk[k], ("risk", k))
            # plan selection: the numpy rule on the per-candidate risk
            got = p.select_plan(c.R, sel, candidates=cand, plan_first=True, K=K, omega_seq=om_seq, step=STEP, cost_w=cw, kpis=kpis, price_start=pstart,
                                per_candidate=True, complete="device")
            st = got["stats"]
            assert st["declined"] > 0 and st == _dev_stats(B * 3 * S, st["declined"], st["completion_rounds"]), st
            assert np.all(got["risk"]["n_complete"] == S) and got["admissible"].all()
            pick = simlog.select_plan_np(got["risk"], sel, S, candidates=np.concatenate([plan_u[:, None], cand], axis=1))
            for k in ("choice", "score", "n_admissible", "admissible", "u", "u0"):
                _bits(got[k], pick[k], ("select_plan", k))
            # policies among the candidates: none is lost to a decline
            lost = p.select_plan_policies(c.R, sel, candidates=cand, policies=[pol], u_prev=up, omega_seq=om_seq, step=STEP, cost_w=cw, kpis=kpis, price_start=pstart,
                                          per_candidate=True)
            assert not lost["admissible"].all() and lost["risk"]["n_declined"].sum() == lost["stats"]["declined"] > 0
            assert np.array_equal(lost["admissible"], lost["risk"]["n_declined"] == 0)      # inadmissible only because of a decline
            got = p.select_plan_policies(c.R, sel, candidates=cand, policies=[pol], u_prev=up, omega_seq=om_seq, step=STEP, cost_w=cw, kpis=kpis, price_start=pstart,
                                         per_candidate=True, complete="device")
            assert not got["risk"]["n_declined"].any() and np.all(got["risk"]["n_complete"] == S) and got["admissible"].all() and np.all(got["choice"] >= 0)
            assert got["stats"]["declined"] == lost["stats"]["declined"] == got["stats"]["finished_on_device"]
            # the MIP start: written where it was "declined"
            none = p.warm_start_from_rollout(c.R, policy=True, u_prev=up)
            nm = int((none["source"] == -2).sum())
            assert nm > 0 and np.all(np.isin(none["source"], (1, -2))) and sorted(none["stats"]) == ["kept", "none", "trajectories", "written"]
            dev = p.warm_start_from_rollout(c.R, policy=True, u_prev=up, complete="device")
            rounds = dev["stats"]["completion_rounds"]
            assert np.all(dev["source"] == 1) and dev["stats"] == dict(trajectories=B, written=B, kept=0, none=0, finished_on_device=nm, completion_rounds=rounds) and 1 <= rounds <= c.N
            start = p.debug_warm_start()
            ro = p.rollout(c.R, policy=True, u_prev=up, omega_seq=forecast.reshape(B, 1, c.N, c.nw), trajectories=True, complete="device")
            want, source = simlog.start_from_rollout_np(ro["v"], ro["end_status"], np.flatnonzero(p.is_bin))
            assert np.array_equal(start, want) and np.all(source == 1)
    finally:
        p.upload_policy(None)
        p.upload_prices(np.zeros(0))


def test_off_means_off(ctx):
    """7: complete=None on a handle whose setter has been used is a handle that never saw it -- with the cap (the host route) and without; complete="device"
    with nothing declined runs no round and returns the default call's bits"""
    c = ctx("a10")
    K = c.N
    _, _, _, om_seq, u_seq = _scenario(c, K, 9700)
    c.p.set_rollout_completion(_lib.MLD_ROLLOUT_COMPLETE_DEVICE)
    c.p.set_rollout_completion(0)
    fresh = _SmallCtx(*SHAPES["a10"])
    try:
        for cap in (0, CAP):
            out = []
            for s in (c, fresh):
                s.p.upload(s.x0, s.om, s.midx)
                s.R.problem.set_opts(reserved=cap)
                try:
                    out.append(s.p.rollout(s.R, u_seq=u_seq, omega_seq=om_seq, trajectories=True))
                finally:
                    s.R.problem.set_opts(reserved=0)
            n, nd = c.B * S, out[0]["stats"]["declined"]
            assert out[0]["stats"] == out[1]["stats"] == dict(trajectories=n, complete=n, infeasible=0, declined=nd, not_attempted=0, finished_on_host=nd) and (nd > 0) == bool(cap)
            assert sorted(out[0]) == sorted(out[1]) == sorted(TRAJ + SUMM + ("stats",))
            for k in TRAJ + SUMM:
                _bits(out[0][k], out[1][k], (cap, k))
        dev = c.p.rollout(c.R, u_seq=u_seq, omega_seq=om_seq, trajectories=True, complete="device")
        assert dev["stats"] == dict(out[0]["stats"], declined=0, finished_on_host=0, finished_on_device=0, completion_rounds=0)
        assert c.p.rollout_completion_stats() == dict(rounds=0, finished_on_device=0, dense_solves=0, left_declined=0)
        plain = c.p.rollout(c.R, u_seq=u_seq, omega_seq=om_seq, trajectories=True)
        for k in TRAJ + SUMM:
            _bits(dev[k], plain[k], ("nothing declined", k))
    finally:
        fresh.close()


def test_handles_left_as_found(ctx):
    """8: the stepped handle's inputs, plan, log count, policy state and MIP start; sim_step(resolve=R) before and after; the mode after an exception"""
    c = ctx("a10")
    p, B, K = c.p, c.B, c.N
    _, _, _, om_seq, u_seq = _scenario(c, K, 9800)
    rng = np.random.default_rng(9801)
    try:
        p.upload(c.x0, c.om, c.midx)
        p.upload_policy(thermostat(c))
        p.policy_state(u_prev=np.ones((B, c.nu)))
        p.sim_log_begin(2)
        p.solve_resident()
        p.set_warm_start(rng.integers(0, 2, (B, p.n_bin)).astype(np.uint8))
        step_before = p.sim_step(resolve=c.R, advance=False, log=False, outputs=True)
        before = (p.inputs(), p.download(), p.sim_log_count(), p.policy_state(), p.debug_warm_start())

        def unchanged(what):
            after = (p.inputs(), p.download(), p.sim_log_count(), p.policy_state(), p.debug_warm_start())
            for a, b in zip(before[0] + tuple(before[1][k] for k in sorted(before[1])) + before[3:], after[0] + tuple(after[1][k] for k in sorted(after[1])) + after[3:]):
                _bits(a, b, what)
            assert before[2] == after[2], what

        with _capped(c):
            for kw in (dict(u_seq=u_seq), dict(K=K), dict(K=K, policy=True), dict(u_seq=u_seq, trajectories=True)):
                got = p.rollout(c.R, omega_seq=om_seq, complete="device", **kw)
                assert got["stats"]["finished_on_device"] == got["stats"]["declined"] > 0 and got["stats"]["complete"] == B * S, kw
                unchanged(kw)
            with pytest.raises(ValueError, match="omega_seq has shape"):      # raised inside the call, behind the setter
                p.rollout(c.R, u_seq=u_seq, omega_seq=om_seq[:, :, :1], complete="device")
            rc, es, _, stats = _raw(p, c.R, K, u_seq, om_seq)
            assert rc == 0 and int((es == 2).sum()) == int(stats[3]) > 0      # the mode is back at 0: the C call completes nothing
            assert p.rollout_completion_stats() == dict(rounds=0, finished_on_device=0, dense_solves=0, left_declined=0)
        unchanged("after everything")
        step_after = p.sim_step(resolve=c.R, advance=False, log=False, outputs=True)
        for k in step_before:
            _bits(step_before[k], step_after[k], ("sim_step(resolve=R)", k))
    finally:
        p.upload_policy(None)
        p.sim_log_begin(0)


def test_refusals(ctx):
    """9: unknown mode bits, "host" where there is no host route, an unknown word, a NULL stats pointer: each names its argument and changes nothing"""
    c = ctx("a10")
    p, B, K = c.p, c.B, c.N
    lib = _lib.load()
    _, _, _, om_seq, u_seq = _scenario(c, K, 9900)
    p.upload(c.x0, c.om, c.midx)
    for mode in (4, 5, -1, 1 << 20):
        assert lib.mld_set_rollout_completion(p._h, mode) != 0 and b"mode" in lib.mld_last_error()
        with pytest.raises(MldGpuError, match="mode"):
            p.set_rollout_completion(mode)
    assert lib.mld_set_rollout_completion(None, 1) != 0 and b"p is NULL" in lib.mld_last_error()
    assert lib.mld_rollout_completion_stats(p._h, None) != 0 and b"out is NULL" in lib.mld_last_error()
    out = np.full(4, -7, np.int64)
    assert lib.mld_rollout_completion_stats(None, out.ctypes.data_as(C.POINTER(C.c_int64))) != 0 and np.all(out == -7)
    with _capped(c):      # the refused modes left 0 behind: nothing is completed
        rc, es, _, stats = _raw(p, c.R, K, u_seq, om_seq)
        assert rc == 0 and int((es == 2).sum()) == int(stats[3]) > 0
    sel = PlanSelector(simlog.RiskTable().add("cost", "cost")).minimise("cost", "mean")
    try:
        p.upload_policy(thermostat(c))
        with pytest.raises(ValueError, match="complete = 'host'.*select_plan_policies"):
            p.select_plan_policies(c.R, sel, policies=[thermostat(c)], omega_seq=om_seq, K=K, complete="host")
        with pytest.raises(ValueError, match="complete = 'host'.*warm_start_from_rollout"):
            p.warm_start_from_rollout(c.R, policy=True, complete="host")
        assert p.debug_warm_start() is None
        for entry, args in ((p.rollout, (c.R,)), (p.select_plan, (c.R, sel)), (p.select_plan_policies, (c.R, sel)), (p.warm_start_from_rollout, (c.R,))):
            with pytest.raises(ValueError, match="complete = 'gpu'"):
                entry(*args, complete="gpu")
    finally:
        p.upload_policy(None)
    good = p.rollout(c.R, u_seq=u_seq, omega_seq=om_seq)                     # ... and one good call afterwards still works
    assert good["stats"] == dict(trajectories=B * S, complete=B * S, infeasible=0, declined=0, not_attempted=0, finished_on_host=0)
