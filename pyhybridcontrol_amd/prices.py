"""Index arithmetic and the two formulas of resident price profiles (GpuProblem.upload_prices and its consumers): plain numpy, no device.

The reference cuts every price window out of a series it holds once -- `price_profile.values[start:start + N_tilde].flatten(order='C')` with
`start = int(forecast_lag / freq) + k` (GridAgentMpc.get_price_tilde_k, examples/residential_mg_with_pv_and_dewhs/modelling/micro_grid_agents.py:581-585)
-- turns the window into the objective before every solve (q_z = prices_tilde, q_mu = sum(prices_tilde) * P_h_Nom * mult,
micro_grid_control_simulation.py:186-198) and prices the realised import of every step (cost = sim_k.z * prices_k, micro_grid_agents.py:746-755).

    start = window_start(forecast_lag_steps, k)                   # the row of the series the window of step k begins at
    p     = windows(lib, start, step, N_tilde, n_chan)            # what the device reads: (..., N_tilde * n_chan)
    lin_v, lin_y = cost_np(lib, start, step, N_tilde, n_chan, a_v, sum_v, a_y, model_idx)
    cost, price  = stage_cost_np(lib, start, step, n_chan, w_v, w_y, v, y, model_idx)

The sums of cost_np and stage_cost_np are plain loops in the order the kernels (csrc/prices.inc) take them, one rounding per product and per addition:
numpy's own reductions (np.sum, @, einsum) sum in another order and are not used.
"""
import numpy as np


def window_start(forecast_lag_steps, k, n_chan=1, base=0):
    """flat offset of the price window of step k: the reference's row `int(forecast_lag / freq) + k` (forecast_lag_steps = forecast_lag / freq, truncated
    as its int() does) of a series of n_chan channels that begins at `base` of the library"""
    return np.asarray(base, dtype=np.int64) + (int(forecast_lag_steps) + np.asarray(k, dtype=np.int64)) * int(n_chan)


def windows(lib, start, step, N, n_chan=1):
    """the window rule: start (...) integer offsets into the flat `lib`; returns (..., N * n_chan) with
        out[..., k * n_chan + c] = lib[start + (step + k) * n_chan + c]
    -- `values[row:row + N].flatten(order='C')` of a (time, n_chan) series.  IndexError when a window leaves the library (the device refuses the same starts)."""
    lib = np.asarray(lib, dtype=np.float64).ravel()
    start = np.asarray(start)
    if not np.issubdtype(start.dtype, np.integer):
        raise ValueError("start has dtype %s, expected integers" % start.dtype)
    N, C = int(N), int(n_chan)
    idx = start[..., None].astype(np.int64) + int(step) * C + np.arange(N * C, dtype=np.int64)
    if idx.size and (start.min() < 0 or idx.max() >= lib.size):
        raise IndexError("a price window leaves the library of %d doubles" % lib.size)
    return lib[idx]


def _tables(t, M, C, W, name):
    """(M, C, W) float64 from (M, C, W), (C, W) or (W,); None = zeros"""
    if t is None:
        return np.zeros((M, C, W))
    t = np.asarray(t, dtype=np.float64)
    if t.shape not in ((M, C, W), (C, W), (W,)):
        raise ValueError("%s has shape %s, expected (%d, %d, %d), (%d, %d) or (%d,)" % (name, t.shape, M, C, W, C, W, W))
    return np.ascontiguousarray(np.broadcast_to(t, (M, C, W)))


def cost_np(lib, start, step, N, n_chan, a_v=None, sum_v=None, a_y=None, model_idx=None, n_models=None):
    """the weights mld_instance_cost_from_prices builds, for start (batch,): (lin_v (batch, N * nv), lin_y (batch, N * ny) or None without a_y)
        S[c]               = p[0,c] + p[1,c] + ... + p[N-1,c]
        lin_v[b, k*nv + j] = sum_c ( a_v[m,c,j] * p[k,c] )  +  sum_c ( sum_v[m,c,j] * S[c] )
        lin_y[b, k*ny + j] = sum_c ( a_y[m,c,j] * p[k,c] )
    m = model_idx[b] (0 without).  Tables (n_models, n_chan, width), (n_chan, width) or (width,); the width of a_v / sum_v is nv (one of them is needed)."""
    start = np.atleast_1d(np.asarray(start))
    B, N, C = start.shape[0], int(N), int(n_chan)
    midx = np.zeros(B, np.int64) if model_idx is None else np.asarray(model_idx, np.int64)
    shapes = [np.shape(t) for t in (a_v, sum_v) if t is not None]
    if not shapes and a_y is None:
        raise ValueError("cost_np needs at least one table")
    M = int(n_models) if n_models is not None else max([int(midx.max()) + 1] + [np.shape(t)[0] for t in (a_v, sum_v, a_y) if t is not None and np.ndim(t) == 3])
    nv = shapes[0][-1] if shapes else 0
    av, sv = _tables(a_v, M, C, nv, "a_v"), _tables(sum_v, M, C, nv, "sum_v")
    p = windows(lib, start, step, N, C).reshape(B, N, C)
    S = p[:, 0, :].copy()
    for k in range(1, N):
        S = S + p[:, k, :]
    lin_v = np.zeros((B, N, nv))
    acs = np.zeros((B, nv))
    for c in range(C):
        acs = acs + sv[midx, c, :] * S[:, c, None]
    for k in range(N):
        acc = np.zeros((B, nv))
        for c in range(C):
            acc = acc + av[midx, c, :] * p[:, k, c, None]
        lin_v[:, k, :] = acc + acs
    lin_y = None
    if a_y is not None:
        ny = np.shape(a_y)[-1]
        ay = _tables(a_y, M, C, ny, "a_y")
        lin_y = np.zeros((B, N, ny))
        for k in range(N):
            acc = np.zeros((B, ny))
            for c in range(C):
                acc = acc + ay[midx, c, :] * p[:, k, c, None]
            lin_y[:, k, :] = acc
        lin_y = lin_y.reshape(B, N * ny)
    return lin_v.reshape(B, N * nv), lin_y


def stage_cost_np(lib, start, step, n_chan, w_v, w_y, v, y, model_idx=None, n_models=None):
    """price and stage cost of one logged step, for start (batch,), v (batch, nv), y (batch, ny): (cost (batch,), price (batch, n_chan))
        price[c] = lib[start + step * n_chan + c]
        cost     = sum_c price[c] * ( sum_j w_v[m,c,j] * v[j]  +  sum_j w_y[m,c,j] * y[j] )
    An instance whose record has NaN in v or y (it was skipped) gets cost NaN by the arithmetic itself only where a weight meets it: callers mask the
    skipped instances (the device writes NaN for them whatever the weights)."""
    start = np.atleast_1d(np.asarray(start))
    B, C = start.shape[0], int(n_chan)
    v, y = np.asarray(v, dtype=np.float64).reshape(B, -1), np.asarray(y, dtype=np.float64).reshape(B, -1)
    nv, ny = v.shape[1], y.shape[1]
    midx = np.zeros(B, np.int64) if model_idx is None else np.asarray(model_idx, np.int64)
    M = int(n_models) if n_models is not None else max([int(midx.max()) + 1] + [np.shape(t)[0] for t in (w_v, w_y) if t is not None and np.ndim(t) == 3])
    wv, wy = _tables(w_v, M, C, nv, "w_v"), _tables(w_y, M, C, ny, "w_y")
    price = windows(lib, start, step, 1, C).reshape(B, C)
    cost = np.zeros(B)
    for c in range(C):
        sv, sy = np.zeros(B), np.zeros(B)
        for j in range(nv):
            sv = sv + wv[midx, c, j] * v[:, j]
        for j in range(ny):
            sy = sy + wy[midx, c, j] * y[:, j]
        cost = cost + price[:, c] * (sv + sy)
    return cost, price
