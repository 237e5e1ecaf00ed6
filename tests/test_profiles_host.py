"""Host side of the resident disturbance profiles (mld_upload_profiles, mld_forecast_from_profiles, mld_constraint_blocks_from_profiles,
mld_evaluate_batch_profiles, mld_download_constraint_blocks): the entry points are declared, listed and loadable; the numpy helpers of
pyhybridcontrol_amd.profiles against the window rule written as a double loop and against the reference's own slicing expressions (written out in
numpy here); every shape / dtype error of the Python layer raised before the library is loaded.  No GPU needed."""
import os
import re
import types

import numpy as np
import pytest

from pyhybridcontrol_amd import gpu, profiles, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WS = r"\s*"
P = r"mld_problem_t\s*\*"
EVAL_OUT = [r"double\s*\*\s*obj_out", r"double\s*\*\s*constr_vio_out", r"int32_t\s*\*\s*constr_row_out", r"double\s*\*\s*int_vio_out", r"double\s*\*\s*bound_vio_out"]
PROTOTYPES = {
    "mld_upload_profiles": [P, r"int64_t\s+lib_len", r"const\s+double\s*\*\s*lib", r"int\s+n_groups", r"const\s+int32_t\s*\*\s*group_width"],
    "mld_forecast_from_profiles": [P, r"const\s+int64_t\s*\*\s*start", r"int\s+step"],
    "mld_constraint_blocks_from_profiles": [P, r"int\s+n_cols", r"const\s+int64_t\s*\*\s*start", r"int\s+step", r"const\s+int32_t\s*\*\s*col_rows",
                                            r"const\s+double\s*\*\s*x_cols"],
    "mld_evaluate_batch_profiles": [P, r"const\s+double\s*\*\s*v", r"int\s+n_cols", r"const\s+int64_t\s*\*\s*start", r"int\s+step",
                                    r"const\s+int32_t\s*\*\s*col_rows", r"const\s+double\s*\*\s*x_cols"] + EVAL_OUT,
    "mld_download_constraint_blocks": [P, r"int32_t\s*\*\s*n_cols_out", r"double\s*\*\s*omega_cols", r"int32_t\s*\*\s*col_rows", r"double\s*\*\s*x_cols"],
}


def test_entry_points_are_declared_listed_and_loadable():
    with open(os.path.join(ROOT, "include", "mldgpu.h")) as f:
        header = f.read()
    lib = _lib.load()
    for name, args in PROTOTYPES.items():
        assert re.search(r"\bint\s+" + name + r"\s*\(" + WS + (WS + "," + WS).join(args) + WS + r"\)\s*;", header), name
        assert name in _lib.EXPORTS, name
        fn = getattr(lib, name)
        assert fn.argtypes is not None and len(fn.argtypes) == len(args), name
    # declared with the reference lines they replace, and the version says so
    assert "micro_grid_agents.py:236-298" in header and ":206-232" in header and "micro_grid_control_simulation.py:200-227" in header
    assert "resident disturbance profiles" in _lib.version()


# ---- the window rule ------------------------------------------------------------------------------------------------------------------------
def _windows_loop(lib, start, step, N, gw):
    """the rule of include/mldgpu.h, literally"""
    nomega = sum(gw)
    start = np.asarray(start).reshape(-1, len(gw))
    out = np.zeros((start.shape[0], N * nomega))
    for r in range(start.shape[0]):
        goff = 0
        for g, w in enumerate(gw):
            for k in range(N):
                for j in range(goff, goff + w):
                    out[r, k * nomega + j] = lib[start[r, g] + (step + k) * w + (j - goff)]
            goff += w
    return out


@pytest.mark.parametrize("gw", [(1,), (3,), (1, 2), (2, 1, 5)])
def test_windows_is_the_window_rule(gw):
    rng = np.random.default_rng(100 + sum(gw))
    N, L = 7, 500
    lib = rng.standard_normal(L)
    for step in (0, 1, 7):
        hi = [L - (step + N) * w for w in gw]                     # the last valid start of every group
        start = np.stack([rng.integers(0, h + 1, size=(4, 3)) for h in hi], axis=-1)
        start[0, 0] = 0
        start[1, 1] = hi                                          # exactly the last valid offset
        start[2, :] = start[2, 0]                                 # the same start for several rows
        got = profiles.windows(lib, start, step, N, gw)
        assert got.shape == (4, 3, N * sum(gw))
        assert np.array_equal(got.reshape(12, -1), _windows_loop(lib, start, step, N, gw))
        assert np.array_equal(profiles.windows(lib, start[1, 1], step, N, gw), got[1, 1])          # a single start vector
        with pytest.raises(IndexError):
            profiles.windows(lib, start[1, 1] + np.eye(len(gw), dtype=np.int64)[-1], step, N, gw)  # one element past the end
        with pytest.raises(IndexError):
            profiles.windows(lib, -np.ones(len(gw), dtype=np.int64), step, N, gw)                   # numpy would wrap a negative index
    with pytest.raises(ValueError, match="expected integers"):
        profiles.windows(lib, np.zeros(len(gw)), 0, N, gw)
    with pytest.raises(ValueError, match="one offset per group"):
        profiles.windows(lib, np.zeros(len(gw) + 1, dtype=np.int64), 0, N, gw)


def test_pack_and_window_start_reproduce_the_profile_slices():
    """get_omega_tilde_k_hat: profile.values[k:k + N].flatten(order='C'); _act: the same from forecast_lag + k (micro_grid_agents.py:236-298)"""
    rng = np.random.default_rng(7)
    series = [rng.standard_normal((40, 3)), rng.standard_normal(25), rng.standard_normal((33, 2))]
    lib, base = profiles.pack(series)
    assert lib.shape == (40 * 3 + 25 + 33 * 2,) and base.tolist() == [0, 120, 145] and base.dtype == np.int64
    N = 6
    for i, (values, w) in enumerate(zip(series, (3, 1, 2))):
        values = values.reshape(-1, w)
        for k in (0, 5, values.shape[0] - N):                     # the last window that fits
            for lag in (0, 3):
                if k + lag + N > values.shape[0]:
                    continue
                ref = values[lag + k:lag + k + N].flatten(order="C")
                s = profiles.window_start(base[i], k, w, lag=lag)
                assert np.array_equal(profiles.windows(lib, [s], 0, N, (w,)), ref)
                assert np.array_equal(profiles.windows(lib, [profiles.window_start(base[i], 0, w, lag=lag)], k, N, (w,)), ref)   # the step slides it
    assert profiles.window_start(base, 2, 1).tolist() == [2, 122, 147]          # vectorised over bases
    assert profiles.pack([])[0].size == 0


class _FixedDays:
    """stands in for the generator: returns the requested day columns, and records the bound it was asked for"""

    def __init__(self, days):
        self.days = days

    def integers(self, low, high, size):
        self.low, self.high = low, high
        return np.broadcast_to(np.asarray(self.days if self.days is not None else high - 1), np.shape(np.zeros(size))).copy()


def test_scenario_starts_reproduce_the_scenario_slices():
    """get_omega_tilde_scenario (micro_grid_agents.py:206-232) on the matrix set_omega_scenarios builds (:176): the (n, nomega) series stacked and
    reshaped to (intervals_per_day * nomega, n_days) in column-major order"""
    rng = np.random.default_rng(11)
    ipd, n_days, m, N = 8, 9, 3, 5
    series = rng.standard_normal((ipd * n_days, m))
    other = rng.standard_normal(17)
    lib, base = profiles.pack([other, series])                   # the series does not start the library
    scenarios = np.asfortranarray(series.reshape(-1).reshape(ipd * m, -1, order="F"))          # omega_scenarios_profile.stack().values.reshape(ipd * m, -1, order='F')
    assert scenarios.shape == (ipd * m, n_days) and np.array_equal(scenarios.ravel(order="F"), series.ravel())
    for k in (0, 3, ipd + 2, 5 * ipd + 7):
        row = (k % ipd) * m
        limit = scenarios.size - row - (N * m) - 1
        valid_columns = int(np.unravel_index(limit, scenarios.shape, order="F")[1]) - 1
        assert valid_columns >= 1
        for num in (1, 4):
            assert not (limit <= 0 or limit < N * m * num)
            for days in (np.arange(num) % valid_columns, None):   # None: every draw is the last valid day, valid_columns - 1
                gen = _FixedDays(days)
                got = profiles.scenario_starts(base[1], k, ipd, n_days, m, N, num, gen)
                assert (gen.low, gen.high) == (0, valid_columns) and got.shape == (num,) and got.dtype == np.int64
                for c, column_sel in enumerate(days if days is not None else [valid_columns - 1] * num):
                    flat_index = scenarios.shape[0] * column_sel + row
                    ref = scenarios.ravel(order="F")[flat_index:flat_index + (N * m)]
                    assert ref.shape == (N * m,)
                    assert np.array_equal(profiles.windows(lib, [got[c]], 0, N, (m,)), ref)
    # a (batch, n_cols) draw from a real generator stays below the bound and inside the series
    got = profiles.scenario_starts(base[1], 3, ipd, n_days, m, N, (3, 4), np.random.default_rng(1))
    assert got.shape == (3, 4) and np.all((got - base[1] - 3 * m) % (ipd * m) == 0) and np.all((got - base[1]) // (ipd * m) < (scenarios.size - 3 * m - N * m - 1) // (ipd * m) - 1)
    profiles.windows(lib, got[..., None], 0, N, (m,))
    # the reference's error, under the reference's condition: too few days for the number of draws, or none at all
    with pytest.raises(ValueError, match="Insufficient number of scenarios"):
        profiles.scenario_starts(0, 0, ipd, n_days, m, N, 15, np.random.default_rng(1))          # limit = 200 < 5 * 3 * 15
    with pytest.raises(ValueError, match="Insufficient number of scenarios"):
        profiles.scenario_starts(0, 0, ipd, 1, m, 8, 1, np.random.default_rng(1))                # limit = 24 - 24 - 1 <= 0
    profiles.scenario_starts(0, 0, ipd, n_days, m, N, 13, np.random.default_rng(1))              # 195 <= 200: accepted


# ---- the Python layer refuses before the library is loaded ---------------------------------------------------------------------------------------
def _shell(batch, nx=3, nw=3, nv=11, N=5, width=(1, 2)):
    """a GpuProblem without a handle: what the shape checks read (a C call on it would raise MldGpuError, not ValueError)"""
    p = gpu.GpuProblem.__new__(gpu.GpuProblem)
    p.model = types.SimpleNamespace(dims=dict(nx=nx, ny=1, nomega=nw), nv=nv)
    p.N_tilde, p.n, p.nW, p.batch, p._h = N, N * nv, N * nw, batch, None
    p._pf_width = list(width) if width else None
    return p


def test_python_layer_raises_before_the_library_is_loaded(monkeypatch):
    def no_load():
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(_lib, "load", no_load)
    p = _shell(4)
    # start shapes: forecast (batch, n_groups) / (n_groups,), columns (batch, n_cols, n_groups) / (n_cols, n_groups)
    assert p._start_array(np.zeros((4, 2), np.int32), 0).dtype == np.int64
    assert p._start_array([5, 6], 0).tolist() == [[5, 6]] * 4
    assert p._start_array(np.zeros((3, 2), np.int64), 1).shape == (4, 3, 2)
    for bad in (np.zeros((4, 3), int), np.zeros((3, 2), int), np.zeros(3, int), np.zeros((4, 1, 2), int), np.zeros((), int)):
        with pytest.raises(ValueError, match="start has shape"):
            p.forecast_from_profiles(bad)
    for bad in (np.zeros((4, 3, 3), int), np.zeros((5, 3, 2), int), np.zeros(2, int), np.zeros((4, 0, 2), int), np.zeros((4, 2, 3, 2), int)):
        with pytest.raises(ValueError, match="start has shape"):
            p.constraint_blocks_from_profiles(bad)
        with pytest.raises(ValueError, match="start has shape"):
            p.evaluate_profiles(bad, v=np.ones(55))
    # float starts are an error, not a silent cast
    for call in (lambda a: p.forecast_from_profiles(a), lambda a: p.constraint_blocks_from_profiles(a[:, None, :]),
                 lambda a: p.evaluate_profiles(a[:, None, :], v=np.ones(55))):
        with pytest.raises(ValueError, match="start has dtype float64"):
            call(np.zeros((4, 2)))
    with pytest.raises(ValueError, match="needs start"):
        p.evaluate_profiles(None, v=np.ones(55))
    with pytest.raises(ValueError, match="v has shape"):
        p.evaluate_profiles(np.zeros((4, 3, 2), int), v=np.ones(54))
    # col_rows / x_cols as for uploaded columns
    with pytest.raises(ValueError, match="col_rows has shape"):
        p.constraint_blocks_from_profiles(np.zeros((4, 3, 2), int), col_rows=[1, 2])
    with pytest.raises(ValueError, match="col_rows has shape"):
        p.evaluate_profiles(np.zeros((4, 3, 2), int), v=np.ones(55), col_rows=[1.0, 2.0, 3.0])
    with pytest.raises(ValueError, match=r"x_cols has shape \(4, 2, 3\)"):
        p.constraint_blocks_from_profiles(np.zeros((4, 3, 2), int), x_cols=np.ones((4, 2, 3)))
    with pytest.raises(ValueError, match="no state"):
        _shell(4, nx=0).evaluate_profiles(np.zeros((4, 3, 2), int), v=np.ones(55), x_cols=np.ones((4, 3, 0)))
    # col_start together with omega_cols
    for fn in (p.solve, p.solve_handoff_device):
        with pytest.raises(ValueError, match="col_start and omega_cols both given"):
            fn(np.zeros((4, 3)), np.zeros((4, 15)), omega_cols=np.zeros((4, 1, 15)), col_start=np.zeros((4, 1, 2), int))
    # group widths that do not partition the channels
    for bad in ((1, 1), (2, 2), (3, 0), (4, -1), (1.0, 2.0), ((1, 2),), ()):
        with pytest.raises(ValueError, match="sum to nomega = 3"):
            p.upload_profiles(np.zeros(10), group_width=bad)
    with pytest.raises(ValueError, match="flat array"):
        p.upload_profiles(np.zeros((5, 3)), group_width=(1, 2))


def test_no_cpu_fallback_for_the_profiles():
    expect = "no HIP device" if _lib.device_count() <= 0 else "null problem|no batch resident|upload the batch first"
    p = _shell(4)
    with pytest.raises(gpu.MldGpuError, match=expect):
        p.upload_profiles(np.zeros(30), group_width=(1, 2))
    with pytest.raises(gpu.MldGpuError, match=expect):
        p.forecast_from_profiles(np.zeros((4, 2), int))
    with pytest.raises(gpu.MldGpuError, match=expect):
        p.constraint_blocks_from_profiles(np.zeros((4, 3, 2), int))
    with pytest.raises(gpu.MldGpuError, match=expect):
        p.evaluate_profiles(np.zeros((4, 3, 2), int), v=np.ones(55))
