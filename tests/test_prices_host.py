"""CPU tests of resident price profiles (pyhybridcontrol_amd/prices.py, the argument checks of GpuProblem's price methods): the index arithmetic against the
reference's own slices, the two formulas against what the reference builds from a window, and every ValueError before any C call.  No GPU needed."""
import types

import numpy as np
import pytest

from pyhybridcontrol_amd import _lib, gpu, prices


@pytest.mark.parametrize("m", [1, 3])
def test_windows_equal_the_references_slice(m):
    """get_price_tilde_k: price_profile.values[start:start + N_tilde].flatten(order='C') (micro_grid_agents.py:583-585)"""
    rng = np.random.default_rng(40 + m)
    n, N = 37, 6
    values = rng.standard_normal((n, m))
    lib = values.ravel()
    rows = np.array([0, 5, n - N, 11])                                             # one window ends on the series' last row
    got = prices.windows(lib, rows * m, 0, N, m)
    for b, r in enumerate(rows):
        assert np.array_equal(got[b], values[r:r + N].flatten(order="C"))
    got = prices.windows(lib, rows[:2] * m, 3, N, m)                               # `step` slides the window by whole rows
    for b, r in enumerate(rows[:2]):
        assert np.array_equal(got[b], values[r + 3:r + 3 + N].flatten(order="C"))
    with pytest.raises(IndexError):
        prices.windows(lib, np.array([(n - N) * m + 1]), 0, N, m)
    with pytest.raises(IndexError):
        prices.windows(lib, np.array([-1]), 0, N, m)
    with pytest.raises(ValueError, match="integers"):
        prices.windows(lib, np.array([0.0]), 0, N, m)


def test_window_start_is_the_references_arithmetic():
    """micro_grid_agents.py:583: start = int(pd.Timedelta(forecast_lag) / price_profile.index.freq) + k -- a lag of 100 minutes on a 15 minute grid
    is 6.67 intervals, which int() truncates to 6"""
    lag_s, ts = 100 * 60, 15 * 60
    for k in (0, 1, 17):
        ref = int(lag_s / ts) + k
        assert ref == 6 + k
        assert int(prices.window_start(lag_s / ts, k)) == ref
        assert int(prices.window_start(lag_s / ts, k, n_chan=3, base=1000)) == 1000 + 3 * ref
    assert np.array_equal(prices.window_start(0, np.arange(4)), np.arange(4))


def test_cost_np_with_a_v_on_one_column_is_q_z():
    """sim_mpc: q_z = prices_tilde (micro_grid_control_simulation.py:194): a_v = 1 on the z column, n_chan = 1"""
    rng = np.random.default_rng(7)
    N, nv, z = 5, 4, 2
    lib = rng.uniform(0.5, 2.0, 30)
    start = np.array([0, 3, 25])
    a_v = np.zeros(nv)
    a_v[z] = 1.0
    lin_v, lin_y = prices.cost_np(lib, start, 0, N, 1, a_v=a_v)
    assert lin_y is None
    lin_v = lin_v.reshape(3, N, nv)
    for b, s in enumerate(start):
        assert np.array_equal(lin_v[b, :, z], lib[s:s + N])
    assert not lin_v[:, :, [0, 1, 3]].any()


def test_cost_np_with_sum_v_is_the_sum_of_the_window():
    """q_mu = sum(price_vec) * P_h_Nom * mult (:196-198), n_chan = 1.  S is summed left to right, np.sum in another order: either lies within
    (N - 1) u sum|p| of the exact sum to first order (the classical bound of recursive summation in any order, Higham, Accuracy and Stability, section
    4.2), u = 2^-53, and the product with c adds one rounding to each side: the two differ by at most 2 N u = N 2^-52, relative to sum|p| |c|"""
    rng = np.random.default_rng(8)
    N, nv, C = 25, 3, 1
    lib = rng.uniform(0.5, 2.0, 200)
    start = np.array([0, 4, 200 - N * C])
    c = rng.uniform(1.0, 3.0, (C, nv))
    lin_v, _ = prices.cost_np(lib, start, 0, N, C, sum_v=c)
    lin_v = lin_v.reshape(3, N, nv)
    for b, s in enumerate(start):
        p = lib[s:s + N * C].reshape(N, C)
        ref = np.sum(p, axis=0) @ c                                               # sum over channels of sum(price_vec) * c
        bound = N * 2.0 ** -52 * (np.abs(p).sum(axis=0) @ np.abs(c))
        for k in range(N):
            assert np.all(np.abs(lin_v[b, k] - ref) <= bound)
        assert np.array_equal(lin_v[b, 0], lin_v[b, N - 1])                        # the sum term is the same at every step


def test_stage_cost_np_is_z_times_price():
    """sim_step_k: cost = sim_k.z * prices_k (micro_grid_agents.py:753): w_v = 1 on the z column, n_chan = 1"""
    rng = np.random.default_rng(9)
    B, nv, ny, z = 4, 5, 2, 3
    lib = rng.uniform(0.5, 2.0, 20)
    start = np.array([0, 2, 7, 19 - 3])
    v, y = rng.standard_normal((B, nv)), rng.standard_normal((B, ny))
    w_v = np.zeros(nv)
    w_v[z] = 1.0
    cost, price = prices.stage_cost_np(lib, start, 3, 1, w_v, None, v, y)
    assert np.array_equal(price[:, 0], lib[start + 3])
    assert np.array_equal(cost, lib[start + 3] * v[:, z])
    # per-model tables and an output weight: model 1's weights reach model 1's instances only
    w_y = np.zeros((2, 1, ny))
    w_y[1, 0, 0] = 2.0
    cost2, _ = prices.stage_cost_np(lib, start, 3, 1, np.broadcast_to(w_v, (2, 1, nv)), w_y, v, y, model_idx=np.array([0, 1, 0, 1]))
    assert np.array_equal(cost2[[0, 2]], cost[[0, 2]])
    assert np.array_equal(cost2[[1, 3]], lib[start[[1, 3]] + 3] * (v[[1, 3], z] + 2.0 * y[[1, 3], 0]))


def _shell(batch, nv=4, ny=2, n_models=3, n_chan=2, N=5):
    """a GpuProblem without a handle: what the shape checks read (a C call on it would raise MldGpuError, not ValueError)"""
    p = gpu.GpuProblem.__new__(gpu.GpuProblem)
    p.model = types.SimpleNamespace(dims=dict(nx=2, ny=ny, nomega=1), nv=nv, n_models=n_models)
    p.N_tilde, p.n, p.nW, p.batch, p._h = N, N * nv, N, batch, None
    p._pr_chan = n_chan
    return p


def test_python_layer_raises_before_the_library_is_loaded(monkeypatch):
    def no_load():
        raise AssertionError("a C call was made")
    monkeypatch.setattr(_lib, "load", no_load)
    p = _shell(6)
    # tables: (n_models, n_chan, width), (n_chan, width), (width,)
    for good in (np.zeros((3, 2, 4)), np.zeros((2, 4)), np.zeros(4)):
        assert p._price_tables(a_v=good)[0].shape == (3, 2, 4)
    assert p._price_tables(a_y=np.arange(2.0))[0].shape == (3, 2, 2) and p._price_tables(a_v=None) == [None]
    with pytest.raises(ValueError, match="a_v has shape"):
        p.set_price_cost(a_v=np.zeros((2, 2, 4)))
    with pytest.raises(ValueError, match="sum_v has shape"):
        p.set_price_cost(sum_v=np.zeros(5))
    with pytest.raises(ValueError, match="a_y has shape"):
        p.set_price_cost(a_y=np.zeros((3, 2, 4)))
    with pytest.raises(ValueError, match="w_v has shape"):
        p.set_stage_cost(w_v=np.zeros((4, 2)))
    with pytest.raises(ValueError, match="none of that variable"):
        _shell(6, ny=0).set_stage_cost(w_y=np.zeros(1))
    q = _shell(6)
    q._pr_chan = 0
    with pytest.raises(ValueError, match="no price library"):
        q.set_price_cost(a_v=np.zeros(4))
    # starts: (batch,), (1,) or a scalar, integers
    assert np.array_equal(p._price_start(7), np.full(6, 7)) and np.array_equal(p._price_start(np.array([7])), np.full(6, 7))
    assert p._price_start(np.arange(6)).dtype == np.int64
    with pytest.raises(ValueError, match="expected integers"):
        p.instance_cost_from_prices(np.zeros(6))
    with pytest.raises(ValueError, match="start has shape"):
        p.instance_cost_from_prices(np.zeros(5, np.int64))
    with pytest.raises(ValueError, match="start has shape"):
        p.sim_log_cost_begin(np.zeros((6, 1), np.int64))
    with pytest.raises(ValueError, match="needs start"):
        p.sim_log_cost_begin(None)
    with pytest.raises(ValueError, match="flat array"):
        p.upload_prices(np.zeros((3, 2)))
    with pytest.raises(ValueError, match="n_chan"):
        p.upload_prices(np.zeros(6), n_chan=0)
    # solve(): the per-instance cost comes from one side
    with pytest.raises(ValueError, match="price_start and inst_cost both given"):
        p.solve(np.zeros((6, 2)), np.zeros((6, 5)), inst_cost=dict(lin_v=np.zeros(20)), price_start=0)


def test_abi_declares_the_price_entry_points():
    names = ("mld_upload_prices", "mld_set_price_cost", "mld_instance_cost_from_prices", "mld_set_stage_cost", "mld_sim_log_cost_begin",
             "mld_download_sim_log_cost", "mld_download_cost_total")
    for n in names:
        assert n in _lib.EXPORTS
