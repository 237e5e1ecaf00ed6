"""Resident price profiles, the cost side (mld_upload_prices / mld_set_price_cost / mld_instance_cost_from_prices, kernel k_price_cost): the weights a
caller would have built from a price window and uploaded are built on the device from start offsets.  The yardsticks are prices.cost_np -- the formula in
numpy, plain loops in the kernel's order -- bit for bit, and the upload route (upload_instance_cost with the numpy-built weights) on the same or on a second
handle, bit for bit: cost, constant, solve.  Shapes: below16 and nx0 of tests/test_gpu_instance_cost.py (nx0: weights on y without a state), 300 instances
over three models with one unused and a permuted model_idx, so 300 * n is no multiple of 256 and the GEMM's groups are partial; n_chan 1 and 3; step 0
and 2; instance 7's window ends on the library's last element."""
import numpy as np
import pytest

import _paths
from test_gpu_instance_cost import PATHS, SHAPES, _cfg2
from pyhybridcontrol_amd import gpu, prices, synthetic as syn

pytestmark = pytest.mark.gpu

B300 = 300
ROWS = 40                                   # rows (time steps) of the price library of the 300-instance cases
LAST = 7                                    # the instance whose window ends on the library's last element


class _Case(object):
    """three random models of a shape, a problem on one GEMM path, 300 resident instances"""

    def __init__(self, shape, path, tv=False):
        self.N, dims = SHAPES[shape] if not tv else (8, dict(nx=4, nu=3, ndelta=1, nmu=1, nomega=2, ny=2, nc=4))
        self.d = d = _paths.make_dims(**dims)
        seed = 6100 + 10 * (list(SHAPES).index(shape) if not tv else 9)
        self.rng = rng = np.random.default_rng(seed)
        if tv:
            mats = [_paths.random_horizon(90 + i, self.N, **dims)[0] for i in range(3)]
        else:
            mats = [_paths.random_mld(seed * 100000 + i, **dims)[0] for i in range(3)]
        self.m = gpu.GpuModel(mats, d, time_varying=tv)
        self.p = gpu.GpuProblem(self.m, self.N - 1, self.N, None, **dict(PATHS)[path])
        self.midx = rng.permutation(np.r_[np.zeros(170), np.full(130, 2)]).astype(np.int32)      # model 1 unused; partial groups
        self.x0, self.om = rng.standard_normal((B300, d["nx"])), rng.standard_normal((B300, self.N * d["nomega"]))
        self.p.upload(self.x0, self.om, self.midx)

    def library(self, C):
        return self.rng.uniform(0.5, 2.0, ROWS * C)

    def starts(self, C, step, lib):
        """row-aligned random starts, instance LAST at the largest valid value for this step"""
        last = lib.size - (step + self.N) * C
        st = self.rng.integers(0, last // C + 1, B300).astype(np.int64) * C
        st[LAST] = last
        return st

    def tables(self, C, with_y):
        d = self.d
        t = dict(a_v=self.rng.standard_normal((3, C, d["nv"])), sum_v=self.rng.standard_normal((3, C, d["nv"])))
        if with_y:
            t["a_y"] = self.rng.standard_normal((3, C, d["ny"]))
        return t

    def close(self):
        self.p.close(); self.m.close()


_CACHE = {}


@pytest.fixture(scope="module")
def case():
    def get(shape, path, tv=False):
        key = (shape, path, tv)
        if key not in _CACHE:
            _CACHE[key] = _Case(shape, path, tv)
        return _CACHE[key]
    yield get
    for c in _CACHE.values():
        c.close()
    _CACHE.clear()


def _same_cost(a, b, what):
    assert np.array_equal(a["q"], b["q"]), (what, "q", np.abs(a["q"] - b["q"]).max())
    assert np.array_equal(a["const"], b["const"]), (what, "const")


def _refused(p, match, call):
    """the call is refused with `match` in the message and leaves the resident cost as it was"""
    before = p.instance_cost()
    with pytest.raises(gpu.MldGpuError, match=match):
        call()
    _same_cost(p.instance_cost(), before, match)


# ------------------------------------------------------------------------------------------------------------------ 1. the built cost
@pytest.mark.parametrize("path", [p for p, _ in PATHS])
@pytest.mark.parametrize("shape", ["below16", "nx0"])
def test_built_cost_equals_numpy_and_the_upload_route_bit_for_bit(case, shape, path):
    c = case(shape, path)
    p, N = c.p, c.N
    for C in (1, 3):
        lib = c.library(C)
        p.upload_prices(lib, C)
        for step in (0, 2):
            st = c.starts(C, step, lib)
            assert st[LAST] + (step + N) * C == lib.size
            # weights on v only: no GEMM, the cost IS the numpy weights
            t = c.tables(C, False)
            p.set_price_cost(**t)
            p.instance_cost_from_prices(st, step)
            lv, ly = prices.cost_np(lib, st, step, N, C, model_idx=c.midx, n_models=3, **t)
            got = p.instance_cost()
            assert ly is None and np.array_equal(got["q"], lv), (shape, path, C, step, np.abs(got["q"] - lv).max())
            assert not got["const"].any() and np.abs(lv).max() > 0.1
            assert np.array_equal(lv[LAST].reshape(N, -1)[N - 1], prices.cost_np(lib[-N * C:], np.zeros(1, np.int64), 0, N, C, model_idx=c.midx[[LAST]], n_models=3, **t)[0].reshape(N, -1)[N - 1])
            # with weights on y: the cost the SAME handle holds after the upload of the numpy-built weights
            t = c.tables(C, True)
            p.set_price_cost(**t)
            p.instance_cost_from_prices(st, step)
            got = p.instance_cost()
            lv, ly = prices.cost_np(lib, st, step, N, C, model_idx=c.midx, n_models=3, **t)
            p.upload_instance_cost(lin_v=lv, lin_y=ly)
            ref = p.instance_cost()
            _same_cost(got, ref, (shape, path, C, step))
            assert np.abs(ref["const"]).max() > 0 and not np.array_equal(ref["q"], lv)      # the pull-back really ran
    p.upload_prices(np.zeros(0))


# ------------------------------------------------------------------------------------------------------------------ 2. / 3. the solve, sliding
def _tariff_setup(B, seed):
    """cfg2 (one model: z is the grid import, mu the soft-constraint slacks): a library of four tariff series, the reference's q_z = prices_tilde as a_v on
    the z column and q_mu = sum(prices_tilde) * P_h_Nom * (10, 1) as sum_v on the mu columns (synthetic.make_cost)"""
    wl, ag, d = _cfg2(B)
    N, n_h = wl["N_tilde"], wl["n_h"]
    rng = np.random.default_rng(seed)
    T = N + 12
    series = [syn.price_vector(T) * f for f in (1.0, 0.6, 1.7, 1.2)]
    lib = np.concatenate(series)
    start = (rng.integers(0, 4, B) * T + rng.integers(0, 8, B)).astype(np.int64)
    nv = d["nu"] + d["ndelta"] + d["nz"] + d["nmu"]
    z, mu = d["nu"] + d["ndelta"], d["nu"] + d["ndelta"] + d["nz"]
    a_v, sum_v = np.zeros(nv), np.zeros(nv)
    a_v[z] = 1.0
    P_h = ag["params"]["P_h_Nom"]
    sum_v[mu:mu + 2 * n_h:2], sum_v[mu + 1:mu + 2 * n_h:2] = 10.0 * P_h, 1.0 * P_h
    return wl, ag, d, lib, start, dict(a_v=a_v, sum_v=sum_v)


SOLVE_KEYS = ("obj", "lower_bound", "status", "nodes", "pivots", "v")


def test_solve_with_the_built_cost_equals_solve_with_the_uploaded_weights():
    B = 24
    wl, ag, d, lib, start, t = _tariff_setup(B, 31)
    N = wl["N_tilde"]
    m = gpu.GpuModel([ag["mats"]], d)
    kw = dict(max_nodes=2000, gap_rel=1e-4)
    p, q = gpu.GpuProblem(m, wl["N_p"], N, None, **kw), gpu.GpuProblem(m, wl["N_p"], N, None, **kw)
    try:
        p.upload_prices(lib)
        p.set_price_cost(**t)
        with pytest.raises(gpu.MldGpuError, match="upload a batch first"):             # no batch resident (the C entry itself: nothing to shape starts by)
            gpu.check(gpu._lib.load().mld_instance_cost_from_prices(p._h, None, 0))
        step = 1
        lv, _ = prices.cost_np(lib, start, step, N, 1, **t)
        # q_z = prices_tilde and q_mu = sum(prices_tilde) * c, as the reference builds them
        z = d["nu"] + d["ndelta"]
        assert np.array_equal(lv.reshape(B, N, -1)[3, :, z], lib[start[3] + step:start[3] + step + N])
        # explicit route
        p.upload(ag["x0"], ag["omega"])
        p.instance_cost_from_prices(start, step)
        built = p.instance_cost()
        p.launch()                                                                    # a launched solve owns the buffers: refused, nothing changed
        with pytest.raises(gpu.MldGpuError, match="a launched solve has not been finished"):
            p.instance_cost_from_prices(start, step + 1)
        p.finish()
        _same_cost(p.instance_cost(), built, "refused while a solve is in flight")
        a = p.download()
        b = q.solve(ag["x0"], ag["omega"], inst_cost=dict(lin_v=lv))
        for k in SOLVE_KEYS:
            assert np.array_equal(a[k], b[k], equal_nan=True), k
        assert (a["status"] == 0).sum() >= B // 2 and len(set(a["obj"].tolist())) > 4, a["status"]
        # one-call form
        a2 = p.solve(ag["x0"], ag["omega"], price_start=start, price_step=step)
        for k in SOLVE_KEYS:
            assert np.array_equal(a2[k], b[k], equal_nan=True), k
        with pytest.raises(ValueError, match="price_start and inst_cost both given"):
            p.solve(ag["x0"], ag["omega"], inst_cost=dict(lin_v=lv), price_start=start)
        # ---- 3. sliding: the resident starts under the next step, between the advance and the next solve -----------------------------------------------------
        lv1, _ = prices.cost_np(lib, start, step + 1, N, 1, **t)
        for h in (p, q):
            h.advance()
            h.warm_start_from_previous(1)
        ws = p.debug_warm_start()
        assert ws is not None and np.array_equal(ws, q.debug_warm_start())
        p.instance_cost_from_prices(None, step + 1)
        q.upload_instance_cost(lin_v=lv1)
        slid = p.instance_cost()
        assert np.array_equal(slid["q"], lv1) and not np.array_equal(lv1, lv)
        # the state the upload route leaves: the plan readable, the MIP start kept, the batch solved and advanced
        for k in SOLVE_KEYS:
            assert np.array_equal(p.download()[k], q.download()[k], equal_nan=True), k
        assert np.array_equal(p.debug_warm_start(), ws) and np.array_equal(q.debug_warm_start(), ws)
        for h in (p, q):
            with pytest.raises(gpu.MldGpuError, match="already been applied"):
                h.advance()
        p.instance_cost_from_prices(start, step + 1)                                  # the explicit starts: the same cost
        _same_cost(p.instance_cost(), slid, "explicit starts")
        a3, b3 = p.solve_resident(), q.solve_resident()
        for k in SOLVE_KEYS:
            assert np.array_equal(p.download()[k], q.download()[k], equal_nan=True), k
        assert a3["nodes"] == b3["nodes"]
    finally:
        p.close(); q.close(); m.close()


# ------------------------------------------------------------------------------------------------------------------ 4. refusals
def test_refusals_leave_the_resident_cost_as_it_was(case):
    c = case("below16", "mfma64")
    p, N, C = c.p, c.N, 3
    lib = c.library(C)
    t = c.tables(C, True)
    p.upload(c.x0, c.om, c.midx)
    p.upload_prices(lib, C)
    p.set_price_cost(**t)
    st = c.starts(C, 2, lib)
    p.instance_cost_from_prices(st, 2)
    assert np.abs(p.instance_cost()["q"]).max() > 0
    bad = st.copy()
    bad[5] = lib.size - (2 + N) * C + 1                                              # one element too far for step 2 (valid for step 1)
    _refused(p, r"price start %d of instance 5,.*leaves the price library of %d doubles" % (bad[5], lib.size), lambda: p.instance_cost_from_prices(bad, 2))
    p.instance_cost_from_prices(bad, 1)
    p.instance_cost_from_prices(st, 2)
    bad = st.copy()
    bad[9] = -1
    _refused(p, "price start -1 of instance 9,", lambda: p.instance_cost_from_prices(bad, 2))
    _refused(p, "step 3 moves the largest resident price start", lambda: p.instance_cost_from_prices(None, 3))      # instance LAST's window would leave
    _refused(p, "step = -1", lambda: p.instance_cost_from_prices(st, -1))
    with pytest.raises(ValueError, match="price_start and inst_cost both given"):
        p.solve(c.x0, c.om, c.midx, inst_cost=dict(lin_v=np.zeros(p.n)), price_start=st)
    # no tables
    p.set_price_cost()
    _refused(p, "no price tables", lambda: p.instance_cost_from_prices(st, 2))
    p.set_price_cost(**t)
    # None after an upload of another batch size (the upload drops the cost: zeros before and after)
    p.upload(c.x0[:200], c.om[:200], c.midx[:200])
    assert not p.instance_cost()["q"].any()
    _refused(p, "no price starts of this batch are resident", lambda: p.instance_cost_from_prices(None, 0))
    p.upload(c.x0, c.om, c.midx)
    p.instance_cost_from_prices(None, 2)                                             # the starts belong to a batch size and outlive an upload of the same size
    # None without resident starts: a new library invalidates them
    p.upload_prices(lib, C)
    _refused(p, "no price starts of this batch are resident", lambda: p.instance_cost_from_prices(None, 0))
    # no library
    p.upload_prices(np.zeros(0))
    _refused(p, "no price library", lambda: p.instance_cost_from_prices(st, 2))
    with pytest.raises(gpu.MldGpuError, match="no price library"):
        gpu.check(gpu._lib.load().mld_set_price_cost(p._h, gpu._lib.dptr(np.zeros((3, C, c.d["nv"]))), None, None))
    # non-finite entries and a_y without outputs
    p.upload_prices(lib, C)
    nan = t["a_v"].copy()
    nan[2, 1, 0] = np.nan
    with pytest.raises(gpu.MldGpuError, match="a_v of model 2, channel 1, column 0 is not finite"):
        p.set_price_cost(a_v=nan)
    p.upload_prices(np.zeros(0))


def test_time_varying_handle_is_refused(case):
    c = case("tv", "mfma64", tv=True)
    p, N = c.p, c.N
    lib = c.library(1)
    p.upload_prices(lib)
    p.set_price_cost(**c.tables(1, True))
    p.upload_instance_cost(lin_v=c.rng.standard_normal((B300, p.n)))
    _refused(p, "time-varying", lambda: p.instance_cost_from_prices(c.starts(1, 0, lib), 0))
    p.upload_prices(np.zeros(0))


# ------------------------------------------------------------------------------------------------------------------ 5. lifetime
def test_lifetime_of_library_tables_starts_and_cost(case):
    c = case("nx0", "mfma64")
    p, N, C = c.p, c.N, 1
    lib = c.library(C)
    t = c.tables(C, True)
    p.upload(c.x0, c.om, c.midx)
    p.upload_prices(lib, C)
    p.set_price_cost(**t)
    st = c.starts(C, 0, lib)
    p.instance_cost_from_prices(st, 0)
    built = p.instance_cost()
    # upload() drops the cost but neither the library nor the tables (nor, at the same batch size, the starts)
    p.upload(c.x0, c.om, c.midx)
    assert not p.instance_cost()["q"].any() and not p.instance_cost()["const"].any()
    p.instance_cost_from_prices(None, 0)
    _same_cost(p.instance_cost(), built, "after upload()")
    # it survives select() and the one route replaces the other
    p.stage(c.x0[None], c.om[None]); p.select(0)
    _same_cost(p.instance_cost(), built, "after select()")
    lv = c.rng.standard_normal((B300, p.n))
    p.upload_instance_cost(lin_v=lv)
    assert np.array_equal(p.instance_cost()["q"], lv)
    p.instance_cost_from_prices(st, 0)
    _same_cost(p.instance_cost(), built, "the price route replaces an uploaded cost")
    # a new library keeps the tables (same n_chan) and invalidates the starts; another n_chan drops the tables
    lib2 = c.library(C)
    p.upload_prices(lib2, C)
    _refused(p, "no price starts of this batch are resident", lambda: p.instance_cost_from_prices(None, 0))
    p.instance_cost_from_prices(st, 0)
    lv2, ly2 = prices.cost_np(lib2, st, 0, N, C, model_idx=c.midx, n_models=3, **t)
    p.upload_instance_cost(lin_v=lv2, lin_y=ly2)
    ref = p.instance_cost()
    p.instance_cost_from_prices(None, 0)
    _same_cost(p.instance_cost(), ref, "new library, same tables")
    p.upload_prices(c.library(2), 2)
    _refused(p, "no price tables", lambda: p.instance_cost_from_prices(st, 0))
    p.upload_prices(np.zeros(0))
