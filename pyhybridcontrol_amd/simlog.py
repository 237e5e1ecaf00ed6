"""The plant step of a resident batch stated in numpy, and the bridge from its device log to the reference's MldSimLog.

`GpuProblem.sim_step` (mld_sim_step_batch, kernel k_sim_step) is the reference's ``MldModel.lsim_k(x_k, v_k=[u; delta; z; mu], omega_k)``
(models/mld_model.py:647-699; with ``v_k=`` given nothing is re-derived, :666-676) for every instance of a batch.  `lsim_k_batch` states the same
rule in numpy, term for term in the kernel's order, for tests and for callers without a device; `to_mld_sim_log` fills the package's `MldSimLog`
(controllers/controller_base.py:58-146) from the arrays `GpuProblem.sim_log()` returns, so that ``get_concat_log()`` gives the reference's frame.

The stage cost is not part of the step: in the reference it is the agent's business (``sim_k.z * prices_k``,
examples/residential_mg_with_pv_and_dewhs/modelling/micro_grid_agents.py:753) and stays a host product on the downloaded log.
"""
import numpy as np

CONS_TOL = 1e-6      # lsim_k's cons_tol default (models/mld_model.py:648)


def _mat(mats, name, rows, cols):
    m = mats.get(name)
    if m is None or np.size(m) == 0:
        return np.zeros((rows, cols))
    return np.asarray(m, dtype=np.float64).reshape(rows, cols)


def lsim_k_batch(mats_list, dims, model_idx, x, v0, omega):
    """lsim_k with the whole step-0 slice for a batch: mats_list models (dicts of the 20 system matrices, missing = zeros), model_idx (batch,) or None
    = all model 0, x (batch, nx), v0 (batch, nv) = [u; delta; z; mu], omega (batch, nomega).

        x_k1 = b5 + A x + [B1 B2 B3] (u, delta, z) + B4 omega                          models/mld_model.py:690
        y    = d5 + C x + [D1 D2 D3] (u, delta, z) + D4 omega                          :691
        r    = E x + [F1 F2 F3] (u, delta, z) + F4 omega + G y - f5                    :692-694 (Psi @ (mu * 0) adds nothing)
        cons = r <= 1e-6 ;  cons_vio = max_i r_i ;  cons_row = the lowest row that attains it (-inf, -1 without rows)

    Returns dict(x_k1, y, resid, cons, cons_vio, cons_row, terms_x, terms_y, terms_r); terms_* hold the row-wise sum of the absolute values of
    every term of the sums (the scale a rounding bound is proportional to; terms_r counts the terms of y inside G y)."""
    nx, nu, nd, nz, nmu, nw, ny, nc = (int(dims.get(k, 0)) for k in ("nx", "nu", "ndelta", "nz", "nmu", "nomega", "ny", "nc"))
    nf = nu + nd + nz
    B = int(np.shape(x)[0]) if np.ndim(x) == 2 else int(np.shape(v0)[0] if np.ndim(v0) == 2 else 1)      # (a family may be empty: the leading axis counts)
    x = np.asarray(x, dtype=np.float64).reshape(B, nx)
    v0 = np.asarray(v0, dtype=np.float64).reshape(B, nf + nmu)
    omega = np.asarray(omega, dtype=np.float64).reshape(B, nw)
    midx = np.zeros(B, dtype=np.int64) if model_idx is None else np.asarray(model_idx, dtype=np.int64).reshape(B)
    out = dict(x_k1=np.zeros((B, nx)), y=np.zeros((B, ny)), resid=np.zeros((B, nc)), terms_x=np.zeros((B, nx)), terms_y=np.zeros((B, ny)),
               terms_r=np.zeros((B, nc)))
    for k, mats in enumerate(mats_list):
        sel = np.where(midx == k)[0]
        if not sel.size:
            continue
        A, B4, b5 = _mat(mats, "A", nx, nx), _mat(mats, "B4", nx, nw), _mat(mats, "b5", nx, 1)[:, 0]
        Cm, D4, d5 = _mat(mats, "C", ny, nx), _mat(mats, "D4", ny, nw), _mat(mats, "d5", ny, 1)[:, 0]
        E, F4, f5, G = _mat(mats, "E", nc, nx), _mat(mats, "F4", nc, nw), _mat(mats, "f5", nc, 1)[:, 0], _mat(mats, "G", nc, ny)
        Bv = np.hstack([_mat(mats, "B1", nx, nu), _mat(mats, "B2", nx, nd), _mat(mats, "B3", nx, nz)])
        Dv = np.hstack([_mat(mats, "D1", ny, nu), _mat(mats, "D2", ny, nd), _mat(mats, "D3", ny, nz)])
        Fv = np.hstack([_mat(mats, "F1", nc, nu), _mat(mats, "F2", nc, nd), _mat(mats, "F3", nc, nz)])
        xs, vs, ws = x[sel], v0[sel, :nf], omega[sel]
        ax, av, aw = np.abs(xs), np.abs(vs), np.abs(ws)
        out["x_k1"][sel] = b5 + xs @ A.T + vs @ Bv.T + ws @ B4.T
        out["terms_x"][sel] = np.abs(b5) + ax @ np.abs(A).T + av @ np.abs(Bv).T + aw @ np.abs(B4).T
        y = d5 + xs @ Cm.T + vs @ Dv.T + ws @ D4.T
        ty = np.abs(d5) + ax @ np.abs(Cm).T + av @ np.abs(Dv).T + aw @ np.abs(D4).T
        out["y"][sel], out["terms_y"][sel] = y, ty
        out["resid"][sel] = xs @ E.T + vs @ Fv.T + ws @ F4.T + y @ G.T - f5
        out["terms_r"][sel] = ax @ np.abs(E).T + av @ np.abs(Fv).T + aw @ np.abs(F4).T + ty @ np.abs(G).T + np.abs(f5)
    r = out["resid"]
    out["cons"] = r <= CONS_TOL
    if nc:
        out["cons_vio"], out["cons_row"] = r.max(axis=1), r.argmax(axis=1).astype(np.int32)      # (argmax: the first = lowest row of equals)
    else:
        out["cons_vio"], out["cons_row"] = np.full(B, -np.inf), np.full(B, -1, dtype=np.int32)
    return out


def sum_bound(dims):
    """relative bound, times the row's sum of |terms|, of the difference between two fp64 evaluations of one row of lsim_k in any order: a sum of
    K = nx + nv + nomega + 1 terms carries at most K roundings of relative size 2^-53 each way (products included, to first order), two evaluations
    differ by at most twice that; a constraint row adds the ny terms of G y, whose y carries its own error: (K + ny) * 2^-52."""
    K = sum(int(dims.get(k, 0)) for k in ("nx", "nu", "ndelta", "nz", "nmu", "nomega")) + 1
    return (K + int(dims.get("ny", 0))) * 2.0 ** -52


def to_mld_sim_log(log, instance, dims, k0=0):
    """the reference's MldSimLog (controllers/controller_base.py:58-146) of one instance of a device log: `log` as GpuProblem.sim_log() returns it,
    entries named as lsim_k names them (x, u, delta, z, mu, v, y, omega, cons, x_k1; models/mld_model.py:696-699), step k0 + row.  get_concat_log()
    of the result is the reference's frame: one row per step, column levels (var_names, var_index)."""
    from .controllers import MldSimLog
    nu, nd, nz = (int(dims.get(k, 0)) for k in ("nu", "ndelta", "nz"))
    o1, o2, o3 = nu, nu + nd, nu + nd + nz
    out = MldSimLog()
    b = int(instance)
    for r in range(np.shape(log["v"])[0]):
        v = np.asarray(log["v"][r, b], dtype=np.float64)
        out.set_sim_k(k0 + r, dict(x_k1=log["x_k1"][r, b], x=log["x"][r, b], u=v[:o1], delta=v[o1:o2], z=v[o2:o3], mu=v[o3:], v=v, y=log["y"][r, b],
                                   omega=log["omega"][r, b], cons=np.asarray(log["cons"][r, b], dtype=bool)))
    return out
