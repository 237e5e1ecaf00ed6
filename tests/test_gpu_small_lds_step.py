"""mld_sim_step_resolve over a resolver on the small-problem path (BatchAuxResolver(..., small_lds=True): k_small_milp instead of k_solve in phase 2 of the
step): the checks of tests/test_gpu_sim_resolve.py that touch the resolver -- device route against host route over the same flagged handle, bit for bit;
the closed form under realised loads; advance and log over three steps; masking of infeasible auxiliaries -- with its shapes and helpers, and the
resolver's small_lds_stats() read after every step: every instance answered in LDS."""
import numpy as np
import pytest

import _aux_ref
from test_gpu_sim_resolve import INFEASIBLE, OUT, SHAPES, _Ctx, _closed_form_checks, _equal, _host_route
from test_gpu_sim_step import _check_step, _dims_nv
from pyhybridcontrol_amd import profiles, simlog
from pyhybridcontrol_amd.aux_resolve import BatchAuxResolver

pytestmark = pytest.mark.gpu


class _SmallCtx(_Ctx):
    """the context of tests/test_gpu_sim_resolve.py with the resolver on the small-problem path"""

    def __init__(self, *a, **kw):
        _Ctx.__init__(self, *a, **kw)
        self.R.close()
        self.R = BatchAuxResolver(self.mats, self.d, small_lds=True)

    def in_lds(self, n=None):
        st = self.R.problem.small_lds_stats()
        assert st == dict(eligible=True, lds=self.B if n is None else n, dense=0), st


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


@pytest.mark.parametrize("shape", list(SHAPES))
def test_device_route_equals_host_route_bit_for_bit(ctx, shape):
    c = ctx(shape)
    p = c.p
    p.upload(c.x0, c.om, c.midx)
    p.solve_resident()
    plan = p.download()
    assert np.all(np.isin(plan["status"], (0, 2)) & np.isfinite(plan["obj"]))
    x_in, w_in = p.inputs()
    got = p.sim_step(resolve=c.R, outputs=True, advance=False, log=False)
    c.in_lds()
    assert got["n_skipped"] == 0 and np.all(got["aux_status"] == 0)
    u, w = plan["v"][:, :c.nu], w_in[:, :c.nw]
    ref = _host_route(c, x_in, u, w, c.midx)
    c.in_lds()
    _equal(got, ref, OUT + ("v0", "aux_status"), shape)
    assert np.array_equal(got["v0"][:, :c.nu], u) and np.all(np.isin(got["v0"][:, c.nu], (0.0, 1.0)))
    _check_step(got, simlog.lsim_k_batch(c.mats, c.d, c.midx, x_in, got["v0"], w), _dims_nv(c.d), shape, drawn=False)
    again = p.sim_step(resolve=c.R, outputs=True, advance=False, log=False)
    _equal(again, got, OUT + ("v0", "aux_status"), shape + " again")


@pytest.mark.parametrize("shape", list(SHAPES))
def test_closed_form_under_realised_loads(ctx, shape):
    c = ctx(shape)
    p = c.p
    step = 1
    rng = np.random.default_rng(dict(a10=7811, a1=7813, b9=7812)[shape])
    lib, gw, astart, w_act = c.realised(rng, step)
    try:
        p.upload(c.x0, c.om, c.midx)
        p.upload_profiles(lib, gw)
        p.solve_resident()
        u = np.ascontiguousarray(p.download()["v"][:, :c.nu])
        got = p.sim_step(resolve=c.R, u0=u, act_start=astart, step=step, advance=False, log=False, outputs=True)
        c.in_lds()
        _closed_form_checks(c, got, c.x0, u, w_act, shape + " inside the bounds")
        assert got["cons"].all(), shape
        _check_step(got, simlog.lsim_k_batch(c.mats, c.d, c.midx, c.x0, got["v0"], w_act), _dims_nv(c.d), shape, drawn=False)
        x_out, u_out, _ = _aux_ref.draw_triples(dict(dims=c.d, omega=c.om), c.B, rng)
        x_out[0, 0], x_out[-1, -1] = 47.0, 80.5
        p.upload(x_out, c.om, c.midx)
        got = p.sim_step(resolve=c.R, u0=u_out, act_start=astart, step=step, advance=False, log=False, outputs=True)
        c.in_lds()
        cf = _closed_form_checks(c, got, x_out, u_out, w_act, shape + " outside the bounds")
        soft = 2 * c.nx
        assert got["cons"][:, soft:].all() and np.array_equal(got["cons"][:, :soft], cf["mu"] == 0), shape
    finally:
        p.upload_profiles(np.zeros(0))


def test_advance_and_log_for_three_steps(ctx):
    c = ctx("a10")
    p, B, N, nw = c.p, c.B, c.N, c.nw
    T = N + 6
    series = [np.tile(c.om[b].reshape(N, nw), (T // N + 1, 1))[:T] for b in range(B)]
    lib, base = profiles.pack(series)
    try:
        p.upload(c.x0, c.om, c.midx)
        p.upload_profiles(lib)
        p.forecast_from_profiles(base.reshape(B, 1), 0)
        p.sim_log_begin(3)
        outs, xs = [], []
        for k in range(3):
            p.solve_resident()
            xs.append(p.inputs()[0])
            outs.append(p.sim_step(resolve=c.R, outputs=True))
            c.in_lds()
            assert outs[k]["n_skipped"] == 0 and p.sim_log_count() == (k + 1, 3)
            p.warm_start_from_previous(1)
            p.forecast_from_profiles(None, k + 1)
            assert np.array_equal(p.inputs()[0], outs[k]["x_k1"])
        log = p.sim_log()
        for k in range(3):
            assert np.array_equal(log["v"][k], outs[k]["v0"]) and np.array_equal(log["x"][k], xs[k]) and np.array_equal(log["x_k1"][k], outs[k]["x_k1"])
        aux = p.sim_log_aux()
        assert aux.shape == (3, B) and np.all(aux == 0)
    finally:
        p.sim_log_begin(0)
        p.upload_profiles(np.zeros(0))


def test_masking_of_infeasible_auxiliaries(ctx):
    c = ctx("a10", hard=True)
    p, B, N = c.p, c.B, c.N
    assert c.d["nmu"] == 0 and c.R.nv2 == 2
    hot = np.zeros(B, bool)
    hot[[1, 4, 7]] = True
    x = c.x0.copy()
    x[hot, 0] = 90.0
    u = np.zeros((B, c.nu))
    p.upload(x, c.om, c.midx)
    got = p.sim_step(resolve=c.R, u0=u, advance=True, log=False, outputs=True)
    c.in_lds()
    assert got["n_skipped"] == 3
    assert np.all(got["aux_status"][hot] == INFEASIBLE) and np.all(got["aux_status"][~hot] == 0)
    for k in ("x_k1", "y", "v0", "cons_vio"):
        assert np.all(np.isnan(got[k][hot])) and np.all(np.isfinite(got[k][~hot])), k
    assert np.all(got["cons_row"][hot] == -1) and not got["cons"][hot].any()
    x_new, w_new = p.inputs()
    assert np.array_equal(x_new[hot], x[hot]) and np.array_equal(w_new[hot], c.om[hot])
    assert np.array_equal(x_new[~hot], got["x_k1"][~hot])
    ref = simlog.lsim_k_batch(c.mats, c.d, c.midx, x, np.where(hot[:, None], 0.0, got["v0"]), c.om[:, :c.nw])
    _check_step({k: got[k][~hot] for k in OUT}, {k: v[~hot] for k, v in ref.items()}, _dims_nv(c.d), "feasible instances", drawn=False)
