"""Campaign KPIs on the device (mld_sim_log_summary / GpuProblem.sim_log_summary, kernel k_log_summary): column statistics of the resident log over time
-- the figures the reference quotes from grid_sim_dataframe (plot_multi_sim_campaign.py:69-131) -- against simlog.summary_np on the DOWNLOADED log.  The
rule has one order (every product and addition rounded on its own, i and k ascending), so every value is expected bit for bit.

The campaign is the closed loop of tests/test_gpu_fallback_step.py: make_agent(3) x 2 models at N_tilde = 3, five logged, advancing steps through
sim_step(resolve=R, fallback=("memory",)) under the realised omega, the stage cost armed with n_chan = 2, instances made plan-less by an unbeatable
cutoff.  A cut-off instance with nothing (left) in the plan memory is skipped: instance 0 is cut off at every step and is skipped in every record, instance
1 at steps 1, 2, 3 (the memory serves two of them), instances 5 and 9 at step 0.  Batch 70 is not a multiple of a wave nor of the four instances of a
workgroup; batch 1 is the other shape (there the one instance is cut off at step 0 only, so "skipped in every record" and "in none" cannot both be asked)."""
import ctypes as C

import numpy as np
import pytest

import _paths
from test_gpu_fallback_step import _library
from test_gpu_small_lds_step import _SmallCtx
from pyhybridcontrol_amd import _lib, gpu, simlog
from pyhybridcontrol_amd.simlog import KpiTable

pytestmark = pytest.mark.gpu

K = 5
CUT = -1e30
NO_PREFETCH = 1 << 18      # MLD_DBG_SUMMARY_NO_PREFETCH
CUTS = {70: {0: (0, 1, 2, 3, 4), 1: (1, 2, 3), 5: (0,), 9: (0,)}, 1: {0: (0,)}}
VALUES = ("sum", "min", "max", "min_step", "max_step", "n_above", "n_changes", "n_stepped", "vio_max", "vio_step", "n_vio", "nodes_total", "n_source")
_CACHE = {}


def _end(p):
    p.set_opts(reserved=0)
    p.sim_log_begin(0)
    p.upload_profiles(np.zeros(0))
    p.upload_prices(np.zeros(0))
    p.plan_memory(False)


def _stage_weights(c, n_chan, seed):
    """channel 0 prices the grid import z, the others carry random weights (as tests/test_gpu_price_step.py)"""
    rng = np.random.default_rng(seed)
    w_v = 0.1 * rng.standard_normal((len(c.mats), n_chan, c.nv))
    w_v[:, 0, :] = 0.0
    w_v[:, 0, c.d["nu"] + c.d["ndelta"]] = 1.0
    return w_v, 0.1 * rng.standard_normal((len(c.mats), n_chan, c.d["ny"]))


def _run(c, n_chan, steps, cuts, seed, capacity=None):
    """`steps` logged, advancing fallback steps on c.p with the stage cost armed; leaves the log resident"""
    p, B = c.p, c.B
    lib, fstart, astart = _library(c, c.N + K + 4)
    rng = np.random.default_rng(seed)
    plib = rng.uniform(0.5, 2.0, (K + 4) * n_chan)
    pstart = ((np.arange(B) % 3) * n_chan).astype(np.int64)
    w_v, w_y = _stage_weights(c, n_chan, seed + 1)
    p.upload(c.x0, c.om, c.midx)
    p.upload_profiles(lib)
    p.forecast_from_profiles(fstart, 0)
    p.sim_log_begin(capacity or steps)
    p.upload_prices(plib, n_chan)
    p.set_stage_cost(w_v, w_y)
    p.plan_memory()
    p.sim_log_cost_begin(pstart)
    for k in range(steps):
        _step(c, k, cuts, astart)
    return dict(astart=astart, w_v=w_v, w_y=w_y, n_chan=n_chan)


def _step(c, k, cuts, astart):
    cut = np.full(c.B, np.inf)
    cut[[b for b, at in cuts.items() if k in at]] = CUT
    c.p.set_cutoffs(cut)
    c.p.solve_resident()
    c.p.sim_step(resolve=c.R, fallback=("memory",), act_start=astart, step=k, advance=True)
    c.p.forecast_from_profiles(None, k + 1)


@pytest.fixture(scope="module", params=[70, 1])
def camp(request):
    """the campaign of one batch size, run once: the context, the downloaded log and what the summaries are compared with"""
    B = request.param
    c = _SmallCtx(3, 2, 3, B)
    try:
        run = _run(c, 2, K, CUTS[B], 9500 + B, capacity=K + 1)
        log, lc, src = c.p.sim_log(), c.p.sim_log_cost(), c.p.sim_log_source()
        assert c.p.sim_log_count() == (K, K + 1)
        skipped = np.isnan(log["x_k1"][:, :, 0])
        assert np.array_equal(skipped, np.isnan(log["x_k1"]).any(axis=2)) and np.all(skipped[src == -1])      # the marking
        if B > 1:
            assert skipped.all(axis=0).any() and (~skipped.any(axis=0)).any()   # one instance skipped in every record, one in none
            assert skipped.any(axis=1).all()                                    # every record holds a skipped instance
            assert (src == 1).any()                                             # ... and the memory served some
        assert skipped.any() and skipped.mean() < 0.5                           # the comparison cannot pass on empty values alone
        yield dict(run, c=c, log=log, price=lc["price"], src=src, skipped=skipped)
    finally:
        _end(c.p)
        c.close()


def _kpis(c, seed, priced=True):
    """every single-table KPI, one with all five tables, a priced one, the reference's columns"""
    rng = np.random.default_rng(seed)
    M, d = len(c.mats), c.d
    t = KpiTable(M, d)
    t.add("x_only", w_x=rng.standard_normal((M, d["nx"])), thresh=60.0)
    t.add("v_only", w_v=rng.standard_normal(c.nv))
    t.add("y_only", w_y=np.ones(d["ny"]), thresh=np.linspace(0.0, 1000.0, M))
    t.add("omega_only", w_omega=rng.standard_normal(d["nomega"]))
    t.add("xk1_only", w_xk1=rng.standard_normal((M, d["nx"])))
    t.add("all_five", w_x=rng.standard_normal(d["nx"]), w_v=rng.standard_normal((M, c.nv)), w_y=rng.standard_normal(d["ny"]),
          w_omega=rng.standard_normal(d["nomega"]), w_xk1=rng.standard_normal(d["nx"]), thresh=0.0)
    if priced:
        t.add("priced", w_v=rng.standard_normal(c.nv), w_y=rng.standard_normal(d["ny"]), price_chan=1)
    ref = KpiTable.microgrid(d, n_models=M, price_chan=0 if priced else None)
    for q, name in enumerate(ref.names):
        t.add(name, price_chan=None if ref._chan[q] < 0 else ref._chan[q], thresh=ref._thresh[q], **ref._rows[q])
    return t


def _compare(got, ref, what):
    assert got["names"] == ref["names"], what
    for name in VALUES:
        assert got[name].dtype == ref[name].dtype and got[name].shape == ref[name].shape, (what, name)
        assert np.array_equal(got[name], ref[name]), (what, name)
    assert np.array_equal(got["sum"].view(np.uint64), ref["sum"].view(np.uint64)), what      # the bit patterns


def _reference(camp, t, first=0, count=K, vio_tol=1e-6):
    sl = slice(first, first + count)
    log = {k: a[sl] for k, a in camp["log"].items()}
    return simlog.summary_np(log, t, camp["c"].midx, price=camp["price"][sl], source=camp["src"][sl], vio_tol=vio_tol, first=first)


def test_every_output_equals_the_numpy_restatement(camp):
    c = camp["c"]
    t = _kpis(c, 9510)
    got = c.p.sim_log_summary(t, 0, K)
    ref = _reference(camp, t)
    _compare(got, ref, "the whole range")
    assert np.array_equal(got["n_stepped"], (~camp["skipped"]).sum(axis=0)) and np.all(got["nodes_total"] == camp["log"]["nodes"].sum(axis=0))
    assert np.abs(got["sum"]).max() > 0 and (got["n_above"] > 0).any() and (got["n_changes"] > 0).any() and np.all(got["n_source"] >= 0)
    never = got["n_stepped"] == 0                                               # the empty values
    assert np.all(got["min"][never] == np.inf) and np.all(got["max"][never] == -np.inf) and np.all(got["min_step"][never] == -1)
    assert np.all(got["vio_max"][never] == -np.inf) and np.all(got["vio_step"][never] == -1) and np.all(got["sum"][never] == 0.0)
    # count=None: all from first; another tolerance
    _compare(c.p.sim_log_summary(t, vio_tol=-1.0), _reference(camp, t, vio_tol=-1.0), "count=None, vio_tol=-1")
    # the staging without the register prefetch: the same bits
    c.p.set_opts(reserved=NO_PREFETCH)
    try:
        _compare(c.p.sim_log_summary(t, 0, K), ref, "no prefetch")
        _compare(c.p.sim_log_summary(t, 1, 3), _reference(camp, t, 1, 3), "no prefetch, first=1, count=3")
    finally:
        c.p.set_opts(reserved=0)


@pytest.mark.parametrize("first,count", [(1, 3), (0, 1), (4, 1), (2, 0), (5, 0)])
def test_sub_ranges(camp, first, count):
    c = camp["c"]
    t = _kpis(c, 9520)
    got = c.p.sim_log_summary(t, first, count)
    _compare(got, _reference(camp, t, first, count), (first, count))
    if count == 0:
        assert not got["sum"].any() and np.all(got["min"] == np.inf) and np.all(got["max"] == -np.inf) and np.all(got["max_step"] == -1)
        assert not got["n_stepped"].any() and not got["nodes_total"].any() and not got["n_source"].any() and np.all(got["vio_step"] == -1)
    else:
        on = got["n_stepped"] > 0
        assert np.all(got["min_step"][on] >= first) and np.all(got["max_step"][on] < first + count)      # absolute record indices


def test_one_kpi_and_sixty_four(camp):
    c = camp["c"]
    M, d = len(c.mats), c.d
    one = KpiTable(M, d).add("z", w_v=np.eye(c.nv)[d["nu"] + d["ndelta"]])
    _compare(c.p.sim_log_summary(one, 0, K), _reference(camp, one), "n_kpi = 1")
    rng = np.random.default_rng(9530)
    full = KpiTable(M, d)
    keys, widths = ("w_x", "w_v", "w_y", "w_omega", "w_xk1"), (d["nx"], c.nv, d["ny"], d["nomega"], d["nx"])
    for q in range(64):
        use = [i for i in range(5) if (q + 1) >> i & 1] if q < 31 else [q % 5, (q + 2) % 5]
        full.add("k%d" % q, price_chan=q % 2 if q % 3 == 0 else None, thresh=float(rng.normal()),
                 **{keys[i]: rng.standard_normal((M, widths[i])) for i in use})
    assert len(full) == 64
    _compare(c.p.sim_log_summary(full, 0, K), _reference(camp, full), "n_kpi = 64")
    _compare(c.p.sim_log_summary(full, 1, 3), _reference(camp, full, 1, 3), "n_kpi = 64, first=1, count=3")
    with pytest.raises(ValueError, match="at most 64"):
        full.add("k64", w_x=np.ones(d["nx"]))
    rc, msg = _raw(c.p, full, n_kpi=65)
    assert rc == -1 and b"n_kpi = 65" in msg
    rc, msg = _raw(c.p, full, n_kpi=0)
    assert rc == -1 and b"n_kpi = 0" in msg


def test_switch_count_of_an_input_channel(camp):
    c = camp["c"]
    t = KpiTable.microgrid(c.d, n_models=len(c.mats))
    got = c.p.sim_log_summary(t, 0, K)
    v, on = camp["log"]["v"], ~camp["skipped"]
    for j in range(c.nu):
        want = np.array([(np.diff(v[on[:, b], b, j]) != 0).sum() for b in range(c.B)])
        assert np.array_equal(got["n_changes"][:, t.names.index("u_%d" % j)], want), j
    z, y = v[:, :, c.d["nu"] + c.d["ndelta"]], camp["log"]["y"][:, :, 0]
    assert np.allclose(got["sum"][:, t.names.index("p_exp")], np.where(on, y - z, 0.0).sum(axis=0), rtol=1e-12, atol=1e-9)
    assert np.allclose(got["sum"][:, t.names.index("p_imp")], np.where(on, z, 0.0).sum(axis=0), rtol=1e-12, atol=1e-9)


def _raw(p, t, n_kpi=None, first=0, count=0, vio_tol=1e-6, **over):
    """mld_sim_log_summary itself, every output NULL: (rc, message); over: w_x .. w_xk1, price_chan, thresh replaced (None = NULL)"""
    arr = dict(t.arrays(), **over)
    dp = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float64).ctypes.data_as(C.POINTER(C.c_double))
    keep = [None if arr[k] is None else np.ascontiguousarray(arr[k], dtype=np.float64) for k in simlog.KPI_TABLES + ("thresh",)]
    pc = None if arr["price_chan"] is None else np.ascontiguousarray(arr["price_chan"], dtype=np.int32)
    lib = _lib.load()
    rc = lib.mld_sim_log_summary(p._h, first, count, len(t) if n_kpi is None else n_kpi, *([dp(a) for a in keep[:5]] +
                                 [None if pc is None else pc.ctypes.data_as(C.POINTER(C.c_int32)), dp(keep[5]), vio_tol] + [None] * 13))
    return rc, lib.mld_last_error()


def test_the_call_changes_nothing_and_the_log_goes_on(camp):
    """LAST of the tests on the campaign: it appends record 5"""
    c = camp["c"]
    p = c.p
    t = _kpis(c, 9540)
    before = (p.sim_log(), p.sim_log_count(), p.cost_total(), p.inputs(), p.sim_log_cost(), p.sim_log_source(), p.plan_memory_state())
    p.sim_log_summary(t, 0, K)
    p.sim_log_summary(t, 1, 3)
    after = (p.sim_log(), p.sim_log_count(), p.cost_total(), p.inputs(), p.sim_log_cost(), p.sim_log_source(), p.plan_memory_state())
    assert before[1] == after[1] == (K, K + 1)
    for a, b in ((before[0], after[0]), (before[2], after[2]), (before[4], after[4]), (before[6], after[6])):
        for k in a:
            assert np.array_equal(a[k], b[k], equal_nan=True), k
    assert all(np.array_equal(a, b) for a, b in zip(before[3], after[3])) and np.array_equal(before[5], after[5])
    _step(c, K, {}, camp["astart"])                                             # one more logging step appends record 5
    assert p.sim_log_count() == (K + 1, K + 1)
    log = p.sim_log()
    for k in before[0]:
        assert np.array_equal(log[k][:K], before[0][k], equal_nan=True), k
    grown = dict(camp, log=log, price=p.sim_log_cost()["price"], src=p.sim_log_source())
    _compare(p.sim_log_summary(t), _reference(grown, t, 0, K + 1), "six records")
    _compare(p.sim_log_summary(t, 0, K), _reference(camp, t), "the first five again")


def test_cost_kpi_reproduces_cost_total():
    """n_chan = 1: the stage weights as a KPI with price_chan = 0 -- sum is cost_total()'s total, n_stepped its steps"""
    c = _SmallCtx(3, 2, 3, 70)
    try:
        run = _run(c, 1, 3, {0: (0, 1, 2), 1: (1, 2), 7: (0,)}, 9550)
        tot = c.p.cost_total()
        assert 0 < tot["steps"].sum() < 3 * c.B and np.abs(tot["total"]).max() > 0 and tot["steps"][0] == 0
        t = KpiTable(len(c.mats), c.d).add("cost", w_v=run["w_v"][:, 0, :], w_y=run["w_y"][:, 0, :], price_chan=0)
        got = c.p.sim_log_summary(t)
        assert np.array_equal(got["sum"][:, 0], tot["total"]) and np.array_equal(got["n_stepped"], tot["steps"])
        # the helper's cost column: z times price, the reference's sim_k.z * prices_k -- channel 0 of these weights prices z alone, y not at all
        ref = KpiTable.microgrid(c.d, n_models=len(c.mats), price_chan=0)
        lc, skipped = c.p.sim_log_cost(), np.isnan(c.p.sim_log()["x_k1"][:, :, 0])
        z = c.p.sim_log()["v"][:, :, c.d["nu"] + c.d["ndelta"]]
        want = np.zeros(c.B)
        for k in range(3):
            want = np.where(skipped[k], want, want + lc["price"][k, :, 0] * z[k])
        assert np.array_equal(c.p.sim_log_summary(ref)["sum"][:, ref.names.index("cost")], want)
    finally:
        _end(c.p)
        c.close()


def test_refusals_leave_the_handle_untouched():
    c = _SmallCtx(3, 2, 3, 1)
    p, d, M = c.p, c.d, 2
    t = KpiTable(M, d).add("z", w_v=np.eye(c.nv)[d["nu"] + d["ndelta"]]).add("y", w_y=np.ones(d["ny"]), thresh=1.0)
    priced = KpiTable(M, d).add("cost", w_v=np.ones(c.nv), price_chan=0)
    state = {}

    def snapshot():
        state.update(log=p.sim_log(), count=p.sim_log_count(), inputs=p.inputs())

    def refused(match, table=t, **kw):
        with pytest.raises(gpu.MldGpuError, match=match):
            p.sim_log_summary(table, **kw)
        unchanged(match)

    def unchanged(what):
        assert p.sim_log_count() == state["count"], what
        log = p.sim_log()
        for k in log:
            assert np.array_equal(log[k], state["log"][k], equal_nan=True), (what, k)
        assert all(np.array_equal(a, b) for a, b in zip(p.inputs(), state["inputs"])), what

    def raw(match, **kw):
        rc, msg = _raw(p, kw.pop("table", t), **kw)
        assert rc == -1 and match in msg, (match, msg)
        unchanged(match)

    try:
        p.upload(c.x0, c.om, c.midx)
        snapshot()
        refused("no log has been begun")
        p.sim_log_begin(3)
        p.solve_resident()
        p.sim_step(advance=True)
        snapshot()
        assert state["count"] == (1, 3)
        # the Python layer, before any C call
        with pytest.raises(ValueError, match="models"):
            p.sim_log_summary(KpiTable(3, d).add("a", w_x=np.ones(d["nx"])))
        with pytest.raises(ValueError, match="other dimensions"):
            p.sim_log_summary(KpiTable(M, dict(d, nx=d["nx"] + 1)).add("a", w_y=np.ones(d["ny"])))
        # the range
        refused(r"records \[0, 2\) asked for, 1 logged", count=2)
        refused(r"records \[2, 2\) asked for, 1 logged", first=2, count=0)
        raw(b"first, count", first=-1, count=1)
        raw(b"first, count", first=0, count=-1)
        # the tables
        raw(b"n_kpi = 65", n_kpi=65)
        raw(b"all NULL", w_v=None, w_y=None)
        bad = t.arrays()["w_v"].copy()
        bad[1, 0, 2] = np.nan
        raw(b"w_v of model 1, KPI 0, entry 2 is not finite", w_v=bad)
        bad = t.arrays()["w_y"].copy()
        bad[0, 1, 0] = np.inf
        raw(b"w_y of model 0, KPI 1, entry 0 is not finite", w_y=bad)
        raw(b"thresh of model 1, KPI 0 is NaN", thresh=np.array([[0.0, 0.0], [np.nan, 0.0]]))
        refused("vio_tol is NaN", vio_tol=np.nan)
        # prices
        refused(r"price_chan\[0\] = 0, but no stage cost is armed", table=priced)
        raw(b"price_chan[1] = -2", price_chan=np.array([-1, -2], np.int32))
        p.upload_prices(np.linspace(1.0, 2.0, 12), 2)
        p.set_stage_cost(np.ones(c.nv), None)
        p.sim_log_cost_begin(0)
        raw(b"price_chan[1] = 2, but the price library has n_chan = 2", price_chan=np.array([1, 2], np.int32))
        raw(b"price_chan[0] = -3", price_chan=np.array([-3, 0], np.int32))
        # record 0 was logged before the arming: its price is NaN, and so is the priced sum -- the call itself is valid
        out = p.sim_log_summary(priced)
        assert np.isnan(out["sum"][0, 0]) and out["n_stepped"][0] == 1
        # a launched solve that has not been finished
        p.set_cutoffs(None)
        p.launch()
        with pytest.raises(gpu.MldGpuError, match="has not been finished"):
            p.sim_log_summary(t)
        p.finish()
        # after all of it the call still answers
        out = p.sim_log_summary(t)
        assert out["n_stepped"][0] == 1 and out["sum"][0, 0] == state["log"]["v"][0, 0, d["nu"] + d["ndelta"]]
    finally:
        _end(p)
        c.close()


def test_a_table_of_a_variable_the_model_has_none_of():
    """w_y with ny == 0 and w_omega with nomega == 0: a model of states and inputs only"""
    dims = dict(nx=2, nu=1, nc=2)
    d = _paths.make_dims(**dims)
    model = gpu.GpuModel([_paths.random_mld(9560, rho=0.9, **dims)[0]], d)
    p = gpu.GpuProblem(model, 1, 2, None)
    try:
        p.upload(np.ones((3, 2)), np.zeros((3, 0)))
        p.sim_log_begin(1)
        assert p.sim_step(v0=np.zeros((3, 1)), advance=True) == 0
        t = KpiTable(1, d).add("x0", w_x=np.array([1.0, 0.0])).add("next", w_xk1=np.array([0.0, 1.0]))
        one = np.ones((1, 2, 1))
        rc, msg = _raw(p, t, w_y=one)
        assert rc == -1 and b"w_y given but the model has none of that variable" in msg
        rc, msg = _raw(p, t, w_omega=one)
        assert rc == -1 and b"w_omega given but the model has none of that variable" in msg
        got = p.sim_log_summary(t)
        log = p.sim_log()
        ref = simlog.summary_np(log, t, None)
        _compare(got, ref, "nx = 2, no y, no omega")
        assert np.all(got["n_source"] == -1) and np.all(got["n_stepped"] == 1) and np.all(got["sum"][:, 0] == 1.0)
        assert np.array_equal(got["sum"][:, 1], log["x_k1"][0, :, 1])
    finally:
        p.sim_log_begin(0)
        p.close()
        model.close()
