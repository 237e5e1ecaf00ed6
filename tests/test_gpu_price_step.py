"""Resident price profiles, the log side (mld_set_stage_cost / mld_sim_log_cost_begin / mld_download_sim_log_cost / mld_download_cost_total, kernel
k_stage_cost): every logged step also records the price of the step and the stage cost of the record's own v and y, and adds it to the instance's total.
The yardstick is prices.stage_cost_np on the DOWNLOADED log -- the formula in numpy, plain loops in the kernel's order -- bit for bit, and the same loop on
a second handle that never arms: every other field of the log, the inputs and the plan are bit-identical.

The closed loop is the one of tests/test_gpu_fallback_step.py (realised omega out of the profile library, instances made plan-less by an unbeatable
cutoff): once through sim_step(), sim_step(resolve=R) and sim_step(resolve=R, policy=True), where the cut-off instances are skipped, and once through
sim_step(resolve=R, fallback=("memory",)), where they are stepped from the plan memory."""
import numpy as np
import pytest

from test_gpu_fallback_step import FB_SHAPES, _library, _solve_cut
from test_gpu_small_lds_step import _SmallCtx
from test_gpu_policy_step import thermostat
from pyhybridcontrol_amd import gpu, prices

pytestmark = pytest.mark.gpu

_CACHE = {}
K = 5
SHAPE = "a10"


@pytest.fixture(scope="module")
def ctx():
    def get(twin=False):
        if twin not in _CACHE:
            _CACHE[twin] = _SmallCtx(*FB_SHAPES[SHAPE])
        return _CACHE[twin]
    yield get
    for c in _CACHE.values():
        c.close()
    _CACHE.clear()


def _price_setup(c, C, seed):
    """a price library of K + 3 rows of C channels, starts on the first three rows -- instance 4's at the largest value that is valid for step K - 1, so the
    last logged step reads the library's last elements --, and stage weights: channel 0 prices the grid import z, the others carry random weights"""
    rng = np.random.default_rng(seed)
    d = c.d
    lib = rng.uniform(0.5, 2.0, (K + 3) * C)
    start = ((np.arange(c.B) % 3) * C).astype(np.int64)
    start[4] = lib.size - K * C
    w_v = 0.1 * rng.standard_normal((len(c.mats), C, c.nv))
    w_v[:, 0, :] = 0.0
    w_v[:, 0, d["nu"] + d["ndelta"]] = 1.0
    w_y = 0.1 * rng.standard_normal((len(c.mats), C, d["ny"])) if d["ny"] else None
    return lib, start, w_v, w_y


def _begin(c, h, lib, fstart, plib, C, w_v, w_y):
    h.upload(c.x0, c.om, c.midx)
    h.upload_profiles(lib)
    h.forecast_from_profiles(fstart, 0)
    h.sim_log_begin(K)
    h.upload_prices(plib, C)
    h.set_stage_cost(w_v, w_y)


def _end(handles):
    for h in handles:
        h.sim_log_begin(0)
        h.upload_profiles(np.zeros(0))
        h.upload_prices(np.zeros(0))
        h.upload_policy(None)
        h.plan_memory(False)


def _check_costs(c, p, plib, pstart, C, w_v, w_y, want_skipped):
    """sim_log_cost() and cost_total() against prices.stage_cost_np on the downloaded log"""
    log, lc, tot = p.sim_log(), p.sim_log_cost(), p.cost_total()
    assert lc["cost"].shape == (K, c.B) and lc["price"].shape == (K, c.B, C) and tot["steps"].dtype == np.int32
    total, steps = np.zeros(c.B), np.zeros(c.B, np.int32)
    for k in range(K):
        skipped = np.isnan(log["x_k1"][k]).any(axis=1)
        assert np.array_equal(np.flatnonzero(skipped), np.asarray(want_skipped.get(k, ()), np.int64)), (k, skipped)
        cost, price = prices.stage_cost_np(plib, pstart, k, C, w_v, w_y, log["v"][k], log["y"][k], model_idx=c.midx, n_models=len(c.mats))
        assert np.array_equal(lc["price"][k], price), k                                       # recorded for the skipped instances too
        assert np.all(np.isnan(lc["cost"][k][skipped])) and np.all(np.isfinite(lc["cost"][k][~skipped])), k
        assert np.array_equal(lc["cost"][k][~skipped], cost[~skipped]), (k, np.abs(lc["cost"][k] - cost)[~skipped].max())
        total[~skipped] = total[~skipped] + cost[~skipped]
        steps[~skipped] += 1
    assert np.array_equal(tot["total"], total) and np.array_equal(tot["steps"], steps)
    assert np.abs(total).max() > 0
    part = p.sim_log_cost(1, 2)
    assert np.array_equal(part["cost"], lc["cost"][1:3], equal_nan=True) and np.array_equal(part["price"], lc["price"][1:3])
    return log


def _same_handles(p, q, la, what):
    lb = q.sim_log()
    for k in la:
        assert np.array_equal(la[k], lb[k], equal_nan=True), (what, k)
    assert np.array_equal(p.sim_log_aux(), q.sim_log_aux()) and np.array_equal(p.sim_log_source(), q.sim_log_source()), what
    for a, b in zip(p.inputs(), q.inputs()):
        assert np.array_equal(a, b), what
    pa, pb = p.download(), q.download()
    for k in pa:
        assert np.array_equal(pa[k], pb[k], equal_nan=True), (what, k)


def test_stage_cost_through_every_step_entry_point(ctx):
    """steps 0 and 4 through sim_step(), 1 and 2 through sim_step(resolve=R), 3 through sim_step(resolve=R, policy=True) (every channel ruled: nobody is
    skipped); instance 1 is cut off at steps 0 and 1, instance 2 at steps 2 and 3 and 4"""
    c, t = ctx(), ctx(twin=True)
    p, q, B, C = c.p, t.p, c.B, 3
    lib, fstart, astart = _library(c, c.N + K + 3)
    plib, pstart, w_v, w_y = _price_setup(c, C, 51)
    cuts = {0: (1,), 1: (1,), 2: (2,), 3: (2,), 4: (2,)}
    want_skipped = {0: (1,), 1: (1,), 2: (2,), 4: (2,)}
    try:
        for h in (p, q):
            _begin(c, h, lib, fstart, plib, C, w_v, w_y)
            h.upload_policy(thermostat(c))
        p.sim_log_cost_begin(pstart)
        first = p.sim_log_cost(0, 0)
        assert first["cost"].shape == (0, B) and not p.cost_total()["total"].any() and not p.cost_total()["steps"].any()
        for k in range(K):
            _solve_cut((p, q), B, list(cuts[k]))
            for h, r in ((p, c.R), (q, t.R)):
                kw = dict(act_start=astart, step=k, advance=True)
                if k in (1, 2):
                    kw.update(resolve=r)
                elif k == 3:
                    kw.update(resolve=r, policy=True)
                n_skipped = h.sim_step(**kw)
                assert n_skipped == len(want_skipped.get(k, ())), (k, n_skipped)
                h.forecast_from_profiles(None, k + 1)
        assert p.sim_log_count() == q.sim_log_count() == (K, K)
        la = _check_costs(c, p, plib, pstart, C, w_v, w_y, want_skipped)
        _same_handles(p, q, la, "armed against never armed")
        with pytest.raises(gpu.MldGpuError, match="no stage cost is armed"):
            q.sim_log_cost()
        with pytest.raises(gpu.MldGpuError, match="no stage cost is armed"):
            q.cost_total()
        with pytest.raises(gpu.MldGpuError, match=r"records \[3, 6\) asked for, 5 logged"):
            p.sim_log_cost(3, 3)
        # sim_log_begin disarms
        p.sim_log_begin(K)
        with pytest.raises(gpu.MldGpuError, match="no stage cost is armed"):
            p.sim_log_cost(0, 0)
    finally:
        _end((p, q))


def test_stage_cost_of_instances_stepped_from_the_plan_memory(ctx):
    """every step through sim_step(resolve=R, fallback=("memory",)); instance 1 is cut off at steps 1 and 2 and takes rows 1 and 2 of the plan it made at
    step 0 (N_tilde = 3): it is stepped, so its cost counts"""
    c, t = ctx(), ctx(twin=True)
    p, q, B, C = c.p, t.p, c.B, 1
    lib, fstart, astart = _library(c, c.N + K + 3)
    plib, pstart, w_v, _ = _price_setup(c, C, 52)
    w_y = None                                                                              # the stage cost is z times price, nothing else
    try:
        for h in (p, q):
            _begin(c, h, lib, fstart, plib, C, w_v, w_y)
            h.plan_memory()
        p.sim_log_cost_begin(pstart)
        for k in range(K):
            _solve_cut((p, q), B, [1] if k in (1, 2) else [])
            for h, r in ((p, c.R), (q, t.R)):
                out = h.sim_step(resolve=r, fallback=("memory",), act_start=astart, step=k, advance=True, outputs=True)
                assert out["n_skipped"] == 0 and out["u_source"][1] == (1 if k in (1, 2) else 0), k
                h.forecast_from_profiles(None, k + 1)
        la = _check_costs(c, p, plib, pstart, C, w_v, w_y, {})
        assert np.all(p.cost_total()["steps"] == K)
        # channel 0 prices z alone: the reference's sim_k.z * prices_k
        z = c.d["nu"] + c.d["ndelta"]
        assert np.array_equal(p.sim_log_cost()["cost"], plib[pstart[None, :] + np.arange(K)[:, None]] * la["v"][:, :, z])
        _same_handles(p, q, la, "armed against never armed, fallback")
    finally:
        _end((p, q))


def test_arming_and_step_refusals(ctx):
    c = ctx()
    p, B, C = c.p, c.B, 3
    lib, fstart, astart = _library(c, c.N + K + 3)
    plib, pstart, w_v, w_y = _price_setup(c, C, 53)
    try:
        p.upload(c.x0, c.om, c.midx)
        p.upload_profiles(lib)
        p.forecast_from_profiles(fstart, 0)
        p.upload_prices(plib, C)
        p.set_stage_cost(w_v, w_y)
        with pytest.raises(gpu.MldGpuError, match="no log has been begun"):
            p.sim_log_cost_begin(pstart)
        p.sim_log_begin(2)
        p.set_stage_cost(None, None)
        with pytest.raises(gpu.MldGpuError, match="no stage weights"):
            p.sim_log_cost_begin(pstart)
        p.set_stage_cost(w_v, w_y)
        bad = pstart.copy()
        bad[3] = plib.size - C + 1
        with pytest.raises(gpu.MldGpuError, match="price start %d of instance 3," % bad[3]):
            p.sim_log_cost_begin(bad)
        bad[3] = -C
        with pytest.raises(gpu.MldGpuError, match="price start -3 of instance 3,"):
            p.sim_log_cost_begin(bad)
        with pytest.raises(gpu.MldGpuError, match="no stage cost is armed"):
            p.cost_total()
        # a step whose `step` would read past the library: refused before anything is queued
        edge = pstart.copy()
        edge[6] = plib.size - C                                                             # valid at step 0 only
        p.sim_log_cost_begin(edge)
        p.solve_resident()
        x_before = p.inputs()[0]
        with pytest.raises(gpu.MldGpuError, match="step 1 moves the largest resident price start .* past the end of the price library"):
            p.sim_step(act_start=astart, step=1, advance=True)
        assert p.sim_log_count() == (0, 2) and np.array_equal(p.inputs()[0], x_before)
        assert p.sim_step(act_start=astart, step=0, advance=True) == 0                      # step 0 reads the library's last elements
        lc = p.sim_log_cost()
        assert np.array_equal(lc["price"][0, 6], plib[-C:]) and np.all(np.isfinite(lc["cost"]))
        # a new price library disarms; without a library arming is refused
        p.upload_prices(plib, C)
        with pytest.raises(gpu.MldGpuError, match="no stage cost is armed"):
            p.sim_log_cost()
        p.upload_prices(np.zeros(0))
        with pytest.raises(gpu.MldGpuError, match="no price library"):
            p.sim_log_cost_begin(pstart)
    finally:
        _end((p,))


def test_a_library_that_is_never_used_changes_nothing(ctx):
    """a solve and a logged resolving step on a handle with a price library, cost tables and stage weights uploaded, but no cost built and nothing armed,
    against a handle that has none of them"""
    c, t = ctx(), ctx(twin=True)
    p, q, B, C = c.p, t.p, c.B, 3
    plib, pstart, w_v, w_y = _price_setup(c, C, 54)
    try:
        p.upload_prices(plib, C)
        p.set_price_cost(a_v=w_v, sum_v=w_v)
        p.set_stage_cost(w_v, w_y)
        for h, r in ((p, c.R), (q, t.R)):
            h.upload(c.x0, c.om, c.midx)
            h.sim_log_begin(1)
            h.solve_resident()
            assert h.sim_step(resolve=r) == 0
        assert not p.instance_cost()["q"].any()
        la, lb = p.sim_log(), q.sim_log()
        for k in la:
            assert np.array_equal(la[k], lb[k], equal_nan=True), k
        for a, b in zip(p.inputs(), q.inputs()):
            assert np.array_equal(a, b)
        pa, pb = p.download(), q.download()
        for k in pa:
            assert np.array_equal(pa[k], pb[k], equal_nan=True), k
    finally:
        _end((p, q))
