"""Index arithmetic of resident disturbance profiles (GpuProblem.upload_profiles and its consumers): plain numpy, no device.

The reference cuts every disturbance window out of a time series it holds once -- `profile.values[start:start + N_tilde].flatten()`
(get_omega_tilde_k_hat / _act, examples/residential_mg_with_pv_and_dewhs/modelling/micro_grid_agents.py:236-298) and
`scenarios.ravel(order='F')[flat_index:flat_index + N_tilde * nomega]` (get_omega_tilde_scenario, :206-232) -- so a window is an offset into a
flat array.  These helpers restate that arithmetic for a library that holds many series back to back:

    lib, base = pack([pv_series, load_series, ...])          # each (n, width) row-major, as a device's profile
    start = window_start(base[i], k, width)                  # the forecast window of step k
    start = scenario_starts(base[i], k, 96, n_days, width, N_tilde, size=20, rng=rng)
    omega = windows(lib, start, step, N_tilde, group_width)  # what the device gathers: the reference of the tests
"""
import numpy as np


def pack(series_list):
    """flat library and the base offset of every series: series (n, width) -- or (n,) for width 1 -- are laid end to end, row-major"""
    flat = [np.ascontiguousarray(s, dtype=np.float64).ravel() for s in series_list]
    base = np.zeros(len(flat), dtype=np.int64)
    if flat:
        base[1:] = np.cumsum([f.size for f in flat])[:-1]
    return (np.concatenate(flat) if flat else np.zeros(0)), base


def window_start(base, k, width, lag=0):
    """start of the profile window of step k in a series at `base` with `width` channels: the flat offset of profile.values[lag + k] --
    get_omega_tilde_k_hat (lag = 0) and get_omega_tilde_k_act (lag = forecast_lag in sampling intervals)"""
    return np.asarray(base, dtype=np.int64) + (np.asarray(k, dtype=np.int64) + int(lag)) * int(width)


def scenario_starts(base, k, intervals_per_day, n_days, width, N_tilde, size, rng):
    """`size` scenario-window starts at step k, the rule of get_omega_tilde_scenario: a series of n_days whole days at `base` is the reference's
    (intervals_per_day * width, n_days) matrix in column-major order; every window starts in the row of the time of day,
    (k % intervals_per_day) * width, of a random day column below the reference's `valid_columns` bound, so that it ends inside the series.
    rng: a numpy Generator (the reference draws from numpy's global state)."""
    rows = int(intervals_per_day) * int(width)
    total = rows * int(n_days)
    row = (int(k) % int(intervals_per_day)) * int(width)
    n_draw = int(np.prod(size))
    limit = total - row - int(N_tilde) * int(width) - 1
    if limit <= 0 or limit < int(N_tilde) * int(width) * n_draw:
        raise ValueError("Insufficient number of scenarios to draw from.")
    valid_columns = limit // rows - 1                      # column of flat index `limit` in column-major order, less one
    day = rng.integers(low=0, high=valid_columns, size=size)
    return np.asarray(base, dtype=np.int64) + rows * day.astype(np.int64) + row


def windows(lib, start, step, N_tilde, group_width):
    """the window rule: start (..., n_groups) integer offsets into the flat `lib`, one per channel group; returns (..., N_tilde * nomega) with
        out[..., k * nomega + j] = lib[start[..., g] + (step + k) * width_g + (j - goff_g)]           j a channel of group g, goff_g its first channel
    IndexError when a window leaves the library (the device refuses the same starts)."""
    lib = np.asarray(lib, dtype=np.float64).ravel()
    start = np.asarray(start)
    if not np.issubdtype(start.dtype, np.integer):
        raise ValueError("start has dtype %s, expected integers" % start.dtype)
    gw = [int(w) for w in np.atleast_1d(group_width)]
    if start.ndim < 1 or start.shape[-1] != len(gw):
        raise ValueError("start has shape %s, expected (..., %d): one offset per group" % (start.shape, len(gw)))
    nomega, N = sum(gw), int(N_tilde)
    out = np.empty(start.shape[:-1] + (N, nomega))
    goff = 0
    for g, w in enumerate(gw):
        idx = start[..., g, None, None].astype(np.int64) + (int(step) + np.arange(N, dtype=np.int64))[:, None] * w + np.arange(w, dtype=np.int64)[None, :]
        if idx.size and (start[..., g].min() < 0 or idx.max() >= lib.size):       # (a start is valid iff s >= 0 and the window ends inside)
            raise IndexError("a window of group %d leaves the library of %d doubles" % (g, lib.size))
        out[..., goff:goff + w] = lib[idx]
        goff += w
    return out.reshape(start.shape[:-1] + (N * nomega,))
