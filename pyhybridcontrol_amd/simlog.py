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


# ---- campaign KPIs: column statistics of the log over time (GpuProblem.sim_log_summary, kernel k_log_summary) ------------------------------------------
KPI_MAX = 64                                                # MLD_KPI_MAX: one lane of a wave owns one KPI
KPI_TABLES = ("w_x", "w_v", "w_y", "w_omega", "w_xk1")      # the order of the functional's terms
_KPI_FIELDS = ("x", "v", "y", "omega", "x_k1")


class KpiTable(object):
    """The KPIs of one summary: each a linear functional of a record, f = w_x . x + w_v . v + w_y . y + w_omega . omega + w_xk1 . x_k1 (the given tables
    only), optionally times the record's price of channel price_chan, with a threshold for n_above.  n_models per-model rows, dims as the model's."""

    def __init__(self, n_models, dims):
        self.n_models = int(n_models)
        if self.n_models < 1:
            raise ValueError("n_models = %r, expected at least one model" % (n_models,))
        nv = sum(int(dims.get(k, 0)) for k in ("nu", "ndelta", "nz", "nmu"))
        self.widths = dict(w_x=int(dims.get("nx", 0)), w_v=nv, w_y=int(dims.get("ny", 0)), w_omega=int(dims.get("nomega", 0)), w_xk1=int(dims.get("nx", 0)))
        self.names, self._rows, self._chan, self._thresh = [], [], [], []

    def __len__(self):
        return len(self.names)

    def add(self, name, w_x=None, w_v=None, w_y=None, w_omega=None, w_xk1=None, price_chan=None, thresh=None):
        """one KPI: a vector (width,) broadcasts over the models, a (n_models, width) array gives one row per model; thresh a scalar or (n_models,).
        ValueError on a duplicate name, a 65th KPI, no table at all, a table of a variable the model has none of, a shape that fits neither, a non-finite
        weight, a NaN threshold, price_chan < 0."""
        given = dict(w_x=w_x, w_v=w_v, w_y=w_y, w_omega=w_omega, w_xk1=w_xk1)
        if name in self.names:
            raise ValueError("a KPI named %r has been added already" % (name,))
        if len(self.names) >= KPI_MAX:
            raise ValueError("a summary holds at most %d KPIs" % KPI_MAX)
        if all(t is None for t in given.values()):
            raise ValueError("KPI %r: no table given (w_x, w_v, w_y, w_omega, w_xk1)" % (name,))
        row = {}
        for key, t in given.items():
            if t is None:
                continue
            W, M = self.widths[key], self.n_models
            t = np.asarray(t, dtype=np.float64)
            if W == 0:
                raise ValueError("KPI %r: %s given but the model has none of that variable" % (name, key))
            if t.shape not in ((W,), (M, W)):
                raise ValueError("KPI %r: %s has shape %s, expected (%d,) or (%d, %d)" % (name, key, t.shape, W, M, W))
            if not np.all(np.isfinite(t)):
                raise ValueError("KPI %r: %s has a non-finite entry" % (name, key))
            row[key] = np.array(np.broadcast_to(t, (M, W)))
        if price_chan is not None and int(price_chan) < 0:
            raise ValueError("KPI %r: price_chan = %r, expected a channel >= 0 or None" % (name, price_chan))
        th = None
        if thresh is not None:
            th = np.asarray(thresh, dtype=np.float64)
            if th.shape not in ((), (self.n_models,)) or np.any(np.isnan(th)):
                raise ValueError("KPI %r: thresh %r, expected a scalar or (%d,) without NaN" % (name, thresh, self.n_models))
            th = np.array(np.broadcast_to(th, (self.n_models,)))
        self.names.append(name)
        self._rows.append(row)
        self._chan.append(-1 if price_chan is None else int(price_chan))
        self._thresh.append(th)
        return self

    def arrays(self):
        """the arguments of mld_sim_log_summary: dict(w_x .. w_xk1 (n_models, n_kpi, width) or None where NO KPI gave that table -- a KPI that did not
        give a table another one gave has zeros there --, price_chan (n_kpi,) int32 with -1 = not priced, thresh (n_models, n_kpi) or None)"""
        Q, M = len(self.names), self.n_models
        if Q < 1:
            raise ValueError("the table holds no KPI")
        out = {}
        for key in KPI_TABLES:
            if not any(key in r for r in self._rows):
                out[key] = None
                continue
            t = np.zeros((M, Q, self.widths[key]))
            for q, r in enumerate(self._rows):
                if key in r:
                    t[:, q, :] = r[key]
            out[key] = t
        out["price_chan"] = np.asarray(self._chan, dtype=np.int32)
        out["thresh"] = None
        if any(t is not None for t in self._thresh):
            out["thresh"] = np.stack([np.full(M, np.inf) if t is None else t for t in self._thresh], axis=1)
        return out

    @classmethod
    def microgrid(cls, dims, n_models=1, price_chan=None):
        """the reference's columns for the synthetic.make_agent(tie=True) models, v = [u; delta; z; mu], y = the grid power: p_imp = z, p_exp = y - z
        (micro_grid_agents.py:750-753), cost = z * price of channel price_chan (:753; left out with price_chan=None), mu_over / mu_under = the comfort
        violations over and under (mu[0::2], mu[1::2]; n_above counts the records where they are positive), and one selector per input channel u_0 ..
        whose n_changes is that channel's switch count"""
        nu, nd, nz, nmu, ny = (int(dims.get(k, 0)) for k in ("nu", "ndelta", "nz", "nmu", "ny"))
        if nz < 1 or ny < 1:
            raise ValueError("KpiTable.microgrid needs a model with a grid tie (nz >= 1, ny >= 1), got nz = %d, ny = %d" % (nz, ny))
        nv, z, mu0 = nu + nd + nz + nmu, nu + nd, nu + nd + nz

        def unit(n, at, val=1.0):
            e = np.zeros(n)
            e[at] = val
            return e
        t = cls(n_models, dims)
        t.add("p_imp", w_v=unit(nv, z))
        t.add("p_exp", w_v=unit(nv, z, -1.0), w_y=unit(ny, 0))
        if price_chan is not None:
            t.add("cost", w_v=unit(nv, z), price_chan=price_chan)
        t.add("mu_over", w_v=unit(nv, np.arange(mu0, nv, 2)), thresh=0.0)
        t.add("mu_under", w_v=unit(nv, np.arange(mu0 + 1, nv, 2)), thresh=0.0)
        for j in range(nu):
            t.add("u_%d" % j, w_v=unit(nv, j))
        return t


def summary_np(log, kpis, model_idx, price=None, source=None, vio_tol=1e-6, first=0):
    """GpuProblem.sim_log_summary stated in numpy, in the kernel's order: log as GpuProblem.sim_log(first, count) returns it, kpis a KpiTable, model_idx
    (batch,) or None, price (count, batch, n_chan) = sim_log_cost()["price"] (needed by a priced KPI), source (count, batch) = sim_log_source() or None
    (the log has no source array: n_source is -1), first: the absolute index of the log's row 0.

    The rule: a record k counts for instance b -- is STEPPED -- iff x_k1[k, b, 0] is not NaN.  s_t = sum_i w_t[m, q, i] * field_t[i] with i ascending
    from 0.0; f = the s_t of the given tables, x, v, y, omega, x_k1, added left to right beginning with the first; f = price[k, b, c] * f where
    price_chan[q] = c >= 0.  The loops over k and i are explicit (numpy only spans (b, q), element by element), so every product and every addition is
    rounded on its own in the stated order."""
    arr = kpis.arrays()
    x_k1 = np.asarray(log["x_k1"], dtype=np.float64)
    K, B = x_k1.shape[0], x_k1.shape[1]
    Q = len(kpis)
    midx = np.zeros(B, dtype=np.int64) if model_idx is None else np.asarray(model_idx, dtype=np.int64).reshape(B)
    chan = arr["price_chan"]
    if np.any(chan >= 0) and price is None:
        raise ValueError("a KPI is priced (price_chan >= 0): summary_np needs price (sim_log_cost()['price'])")
    thr = np.full((B, Q), np.inf) if arr["thresh"] is None else arr["thresh"][midx]
    out = dict(names=list(kpis.names), sum=np.zeros((B, Q)), min=np.full((B, Q), np.inf), max=np.full((B, Q), -np.inf),
               min_step=np.full((B, Q), -1, np.int32), max_step=np.full((B, Q), -1, np.int32), n_above=np.zeros((B, Q), np.int32),
               n_changes=np.zeros((B, Q), np.int32), n_stepped=np.zeros(B, np.int32), vio_max=np.full(B, -np.inf), vio_step=np.full(B, -1, np.int32),
               n_vio=np.zeros(B, np.int32), nodes_total=np.zeros(B, np.int64), n_source=np.full((B, 3), -1 if source is None else 0, np.int32))
    prev, have_prev = np.zeros((B, Q)), np.zeros((B, 1), bool)
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(K):
            step = int(first) + k
            f, started = np.zeros((B, Q)), False
            for key, name in zip(KPI_TABLES, _KPI_FIELDS):
                if arr[key] is None:
                    continue
                w, fld = arr[key][midx], np.asarray(log[name][k], dtype=np.float64)      # (B, Q, width), (B, width)
                s = np.zeros((B, Q))
                for i in range(w.shape[2]):
                    t = w[:, :, i] * fld[:, i:i + 1]
                    s = s + t
                f = f + s if started else s
                started = True
            for q in np.flatnonzero(chan >= 0):
                f[:, q] = np.asarray(price[k], dtype=np.float64)[:, chan[q]] * f[:, q]
            stepped = ~np.isnan(x_k1[k, :, 0])
            on = stepped[:, None]
            out["sum"] = np.where(on, out["sum"] + f, out["sum"])
            lo, hi = on & (f < out["min"]), on & (f > out["max"])
            out["min"], out["min_step"] = np.where(lo, f, out["min"]), np.where(lo, step, out["min_step"]).astype(np.int32)
            out["max"], out["max_step"] = np.where(hi, f, out["max"]), np.where(hi, step, out["max_step"]).astype(np.int32)
            out["n_above"] += on & (f > thr)
            out["n_changes"] += on & have_prev & (f != prev)
            prev, have_prev = np.where(on, f, prev), have_prev | on
            vio = np.asarray(log["cons_vio"][k], dtype=np.float64)
            out["n_stepped"] += stepped
            worse = stepped & (vio > out["vio_max"])
            out["vio_max"], out["vio_step"] = np.where(worse, vio, out["vio_max"]), np.where(worse, step, out["vio_step"]).astype(np.int32)
            out["n_vio"] += stepped & (vio > vio_tol)
            out["nodes_total"] += np.asarray(log["nodes"][k], dtype=np.int64)
            if source is not None:
                for s in range(3):
                    out["n_source"][:, s] += np.asarray(source[k]) == s
    return out


# ---- open-loop rollout: the reference's MldModel.lsim, lsim_k in a loop (models/mld_model.py:543-642, 647-699) with _compute_aux (:701-766) per step ----
def _worst(vio):
    """(worst_vio, worst_step) of cons_vio rows (T, K): the largest value, a NaN wins, the earliest step of equals"""
    vio = np.asarray(vio, dtype=np.float64)
    nan = np.isnan(vio)
    step = np.where(nan.any(axis=1), nan.argmax(axis=1), np.where(nan, -np.inf, vio).argmax(axis=1)).astype(np.int32)
    return vio[np.arange(vio.shape[0]), step], step


def lsim_k_reference_order(mats_list, dims, model_idx, x, v0, omega):
    """lsim_k_batch with every sum in the REFERENCE's order of operations, instance by instance as the reference calls it (models/mld_model.py:690-694):
    A x + B1 u + B2 delta + B3 z + B4 omega + b5, the same for y, and E x + F1 u + F2 delta + F3 z + F4 omega + G y + Psi (mu * 0) - f5.  The kernels'
    order (lsim_k_batch) differs from it by rounding only.  Returns dict(x_k1, y, resid, cons, cons_vio, cons_row)."""
    nx, nu, nd, nz, nmu, nw, ny, nc = (int(dims.get(k, 0)) for k in ("nx", "nu", "ndelta", "nz", "nmu", "nomega", "ny", "nc"))
    B = int(np.shape(x)[0])
    o1, o2, o3 = nu, nu + nd, nu + nd + nz
    midx = np.zeros(B, dtype=np.int64) if model_idx is None else np.asarray(model_idx, dtype=np.int64).reshape(B)
    out = dict(x_k1=np.zeros((B, nx)), y=np.zeros((B, ny)), resid=np.zeros((B, nc)))
    for b in range(B):
        m = mats_list[midx[b]]
        g = lambda name, r, c: _mat(m, name, r, c)
        xk, wk = np.asarray(x[b], np.float64).reshape(nx, 1), np.asarray(omega[b], np.float64).reshape(nw, 1)
        vk = np.asarray(v0[b], np.float64).reshape(-1, 1)
        u, dl, z, mu = vk[:o1], vk[o1:o2], vk[o2:o3], vk[o3:]
        out["x_k1"][b] = (g("A", nx, nx) @ xk + g("B1", nx, nu) @ u + g("B2", nx, nd) @ dl + g("B3", nx, nz) @ z + g("B4", nx, nw) @ wk + g("b5", nx, 1))[:, 0]
        y = g("C", ny, nx) @ xk + g("D1", ny, nu) @ u + g("D2", ny, nd) @ dl + g("D3", ny, nz) @ z + g("D4", ny, nw) @ wk + g("d5", ny, 1)
        out["y"][b] = y[:, 0]
        out["resid"][b] = (g("E", nc, nx) @ xk + g("F1", nc, nu) @ u + g("F2", nc, nd) @ dl + g("F3", nc, nz) @ z + g("F4", nc, nw) @ wk + g("G", nc, ny) @ y
                           + g("Psi", nc, nmu) @ (mu * 0) - g("f5", nc, 1))[:, 0]
    r = out["resid"]
    out["cons"] = r <= CONS_TOL
    if nc:
        out["cons_vio"], out["cons_row"] = r.max(axis=1), r.argmax(axis=1).astype(np.int32)
    else:
        out["cons_vio"], out["cons_row"] = np.full(B, -np.inf), np.full(B, -1, dtype=np.int32)
    return out


def rollout_continue(mats_list, dims, model_idx, u_seq, omega_seq, out, todo, resolve_fn, cost_w=None, step_fn=lsim_k_batch, policy=None, u_prev=None):
    """continue the flat trajectories `todo` (indices) of `out` in place, each from its step out["steps_done"][t] and the state out["x"][t, steps_done]:
    model_idx (T,), u_seq (T, K, nu), omega_seq (T, K, nomega), cost_w (T, K, nv) or None; out: x (T, K + 1, nx), v (T, K, nv), y, cons_vio, cons_row (T, K),
    steps_done, end_status, cost, mu_total, worst_vio, worst_step (T,).  Per step, in the reference's order: resolve_fn(x, u, omega, model_idx) ->
    dict(v = [delta | z | mu] rows (NaN where there is no feasible point), status) as aux_resolve.BatchAuxResolver.resolve returns it, then step_fn
    (lsim_k_batch, or lsim_k_reference_order) with v_k = [u_k; delta; z; mu].  A trajectory whose auxiliary problem has no feasible point ends 1 at that step (NaN / -1 from there on, summaries
    NaN / -1), the others end 0 with their summaries reduced from the finished trajectory.
    policy: a policy.ThresholdPolicy -- the ruled channels of u_k come from policy.apply_np on the trajectory's own x_k and u_{k-1} (out["v"][t, k - 1, :nu],
    u_prev (T, nu) before step 0), u_seq supplies the passed-through channels only; out["switches"] (T,), if present, is filled like the other summaries."""
    nu, nv2 = int(dims.get("nu", 0)), sum(int(dims.get(k, 0)) for k in ("ndelta", "nz", "nmu"))
    nf = nu + int(dims.get("ndelta", 0)) + int(dims.get("nz", 0))
    todo = np.asarray(todo, dtype=np.int64)
    midx = np.asarray(model_idx, dtype=np.int64)
    K = out["v"].shape[1]
    out["end_status"][todo] = 0
    for k in range(K):
        act = todo[(out["steps_done"][todo] == k) & (out["end_status"][todo] == 0)]
        if not act.size:
            continue
        x, uk, wk = out["x"][act, k], u_seq[act, k], omega_seq[act, k]
        if policy is not None:
            from .policy import apply_np
            uk = apply_np(policy, midx[act], x, out["v"][act, k - 1, :nu] if k else np.asarray(u_prev, dtype=np.float64)[act], uk)
        if nv2:
            r = resolve_fn(x, uk, wk, midx[act])
            aux = np.asarray(r["v"], dtype=np.float64).reshape(act.size, nv2)
            ok = np.isin(np.asarray(r["status"]), (0, 2)) & np.all(np.isfinite(aux), axis=1)
        else:
            aux, ok = np.zeros((act.size, 0)), np.ones(act.size, bool)
        bad, good = act[~ok], act[ok]
        out["end_status"][bad] = 1
        out["x"][bad, k + 1:] = np.nan; out["v"][bad, k:] = np.nan; out["y"][bad, k:] = np.nan; out["cons_vio"][bad, k:] = np.nan; out["cons_row"][bad, k:] = -1
        if good.size:
            v = np.hstack([uk[ok], aux[ok]])
            st = step_fn(mats_list, dims, midx[good], x[ok], v, wk[ok])
            out["x"][good, k + 1], out["v"][good, k], out["y"][good, k] = st["x_k1"], v, st["y"]
            out["cons_vio"][good, k], out["cons_row"][good, k] = st["cons_vio"], st["cons_row"]
            out["steps_done"][good] = k + 1
    done = todo[out["end_status"][todo] == 0]
    dead = todo[out["end_status"][todo] != 0]
    out["cost"][dead] = out["mu_total"][dead] = out["worst_vio"][dead] = np.nan
    out["worst_step"][dead] = -1
    if policy is not None and "switches" in out:
        from .policy import switches_np
        out["switches"][dead] = -1
        if done.size:
            out["switches"][done] = switches_np(policy, midx[done], out["v"][done][:, :, :nu], np.asarray(u_prev, dtype=np.float64)[done])
    if done.size:
        v = out["v"][done]
        out["cost"][done] = np.einsum("tkj,tkj->t", cost_w[done], v) if cost_w is not None else 0.0
        out["mu_total"][done] = v[:, :, nf:].sum(axis=(1, 2))
        out["worst_vio"][done], out["worst_step"][done] = _worst(out["cons_vio"][done])
    return out


def rollout_np(mats_list, dims, model_idx, x0, u_seq, omega_seq, resolve_fn, cost_w=None, policy=None, u_prev=None):
    """GpuProblem.rollout stated in numpy: x0 (B, nx), u_seq (B, K, nu), omega_seq (B, S, K, nomega), model_idx (B,) or None, cost_w (B, K, nv) or None ->
    dict(x (B, S, K + 1, nx), v (B, S, K, nv), y, cons_vio, cons_row (B, S, K), cost, mu_total, worst_vio, worst_step, steps_done, end_status (B, S)).
    resolve_fn as rollout_continue takes it.  The chain is the reference's, in its order of operations (lsim_k_reference_order).
    policy: GpuProblem.rollout(policy=True) instead -- u_seq supplies the passed-through channels, u_prev (B, nu) the inputs before step 0 (None: the
    policy's reset state), and the result carries switches (B, S)."""
    nx, nw, ny = (int(dims.get(k, 0)) for k in ("nx", "nomega", "ny"))
    nv = sum(int(dims.get(k, 0)) for k in ("nu", "ndelta", "nz", "nmu"))
    u_seq = np.asarray(u_seq, dtype=np.float64)
    B, K = u_seq.shape[0], u_seq.shape[1]
    omega_seq = np.asarray(omega_seq, dtype=np.float64).reshape(B, -1, K, nw)
    S = omega_seq.shape[1]
    T = B * S
    midx = np.zeros(B, dtype=np.int64) if model_idx is None else np.asarray(model_idx, dtype=np.int64)
    out = dict(x=np.full((T, K + 1, nx), np.nan), v=np.full((T, K, nv), np.nan), y=np.full((T, K, ny), np.nan), cons_vio=np.full((T, K), np.nan),
               cons_row=np.full((T, K), -1, np.int32), cost=np.zeros(T), mu_total=np.zeros(T), worst_vio=np.zeros(T), worst_step=np.zeros(T, np.int32),
               steps_done=np.zeros(T, np.int32), end_status=np.zeros(T, np.int32))
    up = None
    if policy is not None:
        out["switches"] = np.zeros(T, np.int32)
        up = np.repeat(policy.initial_state(midx) if u_prev is None else np.asarray(u_prev, dtype=np.float64).reshape(B, -1), S, axis=0)
    out["x"][:, 0] = np.repeat(np.asarray(x0, dtype=np.float64).reshape(B, nx), S, axis=0)
    rollout_continue(mats_list, dims, np.repeat(midx, S), np.repeat(u_seq, S, axis=0), omega_seq.reshape(T, K, nw), out, np.arange(T), resolve_fn,
                     None if cost_w is None else np.repeat(np.asarray(cost_w, dtype=np.float64).reshape(B, K, nv), S, axis=0), step_fn=lsim_k_reference_order,
                     policy=policy, u_prev=up)
    return {k: a.reshape((B, S) + a.shape[1:]) for k, a in out.items()}


KPI_ROLLOUT_KEYS = ("sum", "min", "max", "min_step", "max_step", "n_above", "n_changes", "n_vio")      # what a rollout's "kpi" holds beside names


def rollout_kpis_np(traj, kpis, price=None, vio_tol=1e-6, omega_seq=None, model_idx=None):
    """GpuProblem.rollout(kpis=...)'s "kpi" stated in numpy (mld_rollout_kpi, kernels k_rollout_kpi / k_rollout_policy_kpi): traj the output of
    rollout(trajectories=True) or rollout_np -- x (B, S, K + 1, nx), v (B, S, K, nv), y, cons_vio (B, S, K), end_status (B, S) --, kpis a KpiTable,
    price (B, K, n_chan) the instances' price windows, prices.windows(lib, price_start, step, K, n_chan).reshape(B, K, n_chan) (needed by a priced KPI; the S
    realisations of an instance share it), omega_seq (B, S, K, nomega) the realised disturbance (needed by a KPI with w_omega), model_idx (B,) or None.

    The record of trajectory (b, c) at step k is x = x[b, c, k], v, y, omega = omega_seq[b, c, k], x_k1 = x[b, c, k + 1], and the statistics are summary_np's
    of the log these records make, begun at 0: the arithmetic is summary_np's own, not restated.  A trajectory that did not end 0 gets NaN / -1.
    Returns dict(names, sum, min, max (B, S, n_kpi), min_step, max_step, n_above, n_changes (B, S, n_kpi) int32, n_vio (B, S) int32)."""
    x = np.asarray(traj["x"], dtype=np.float64)
    v = np.asarray(traj["v"], dtype=np.float64)
    B, S, K = v.shape[0], v.shape[1], v.shape[2]
    T = B * S
    arr = kpis.arrays()
    if arr["w_omega"] is not None and omega_seq is None:
        raise ValueError("a KPI reads omega (w_omega): rollout_kpis_np needs omega_seq (B, S, K, nomega)")
    if np.any(arr["price_chan"] >= 0) and price is None:
        raise ValueError("a KPI is priced (price_chan >= 0): rollout_kpis_np needs price (B, K, n_chan)")
    steps = lambda a: np.ascontiguousarray(np.moveaxis(np.asarray(a).reshape((T, K) + np.shape(a)[3:]), 1, 0))      # (B, S, K, ...) -> (K, T, ...)
    log = dict(x=steps(x[:, :, :K]), v=steps(v), y=steps(np.asarray(traj["y"], dtype=np.float64)), x_k1=steps(x[:, :, 1:]),
               cons_vio=steps(np.asarray(traj["cons_vio"], dtype=np.float64)), nodes=np.zeros((K, T), np.int32))
    if omega_seq is not None:
        log["omega"] = steps(np.asarray(omega_seq, dtype=np.float64).reshape(B, S, K, -1))
    midx = None if model_idx is None else np.repeat(np.asarray(model_idx, dtype=np.int64).reshape(B), S)
    pr = None
    if price is not None:
        pr = np.ascontiguousarray(np.moveaxis(np.repeat(np.asarray(price, dtype=np.float64).reshape(B, K, -1), S, axis=0), 1, 0))      # (K, T, n_chan)
    full = summary_np(log, kpis, midx, price=pr, vio_tol=vio_tol)
    dead = np.asarray(traj["end_status"]).reshape(T) != 0
    out = dict(names=list(kpis.names))
    for key in KPI_ROLLOUT_KEYS:
        a = np.array(full[key])
        a[dead] = np.nan if a.dtype.kind == "f" else -1
        out[key] = a.reshape((B, S) + a.shape[1:])
    return out


# ---- rollout risk: statistics across the realisations of a rollout (GpuProblem.rollout(risk=...), mld_rollout_risk, kernel k_rollout_risk) ----------------
RISK_COLS_MAX, RISK_LEVELS_MAX, RISK_S_MAX = 64, 8, 64      # MLD_RISK_COLS_MAX, MLD_RISK_LEVELS_MAX, MLD_RISK_S_MAX
RISK_SOURCES = ("cost", "mu_total", "worst_vio", "switches", "n_vio", "kpi_sum", "kpi_min", "kpi_max", "kpi_n_above", "kpi_n_changes")      # src = the index
RISK_COUNTS = ("n_complete", "n_infeasible", "n_declined", "n_not_attempted")      # the endings 0, 1, 2, -1
RISK_COL_KEYS = ("mean", "min", "min_c", "max", "max_c", "n_exceed")               # (batch, G)
RISK_LEVEL_KEYS = ("quantile", "quantile_c", "cvar_hi", "cvar_lo")                 # (batch, G, L)
_RISK_KPI_KEYS = {5: "sum", 6: "min", 7: "max", 8: "n_above", 9: "n_changes"}


class RiskTable(object):
    """The columns of one risk reduction: each a per-trajectory result of the rollout -- cost, mu_total, worst_vio, switches (policy only), n_vio, or a KPI's
    sum / min / max / n_above / n_changes -- reduced over the complete realisations of every instance.  kpis: the simlog.KpiTable of the same rollout (needed by
    n_vio and the kpi_* sources), levels: the alpha in (0, 1] of the quantiles and tail means, at most 8."""

    def __init__(self, kpis=None, levels=()):
        self.kpis = kpis
        self.levels = [float(a) for a in levels]
        if len(self.levels) > RISK_LEVELS_MAX:
            raise ValueError("a risk table holds at most %d levels" % RISK_LEVELS_MAX)
        for a in self.levels:
            if not (0.0 < a <= 1.0):
                raise ValueError("level %r, expected alpha in (0, 1]" % (a,))
        self.names, self._src, self._q, self._level = [], [], [], []

    def __len__(self):
        return len(self.names)

    def add(self, name, source, kpi=None, level=None):
        """one column: source one of RISK_SOURCES, kpi the KPI's name for the kpi_* sources, level the threshold of n_exceed (None = +inf).  ValueError on a
        duplicate name, a 65th column, an unknown source or KPI, a kpi_* source or n_vio without a KPI table, kpi given for another source, a NaN level."""
        if name in self.names:
            raise ValueError("a column named %r has been added already" % (name,))
        if len(self.names) >= RISK_COLS_MAX:
            raise ValueError("a risk table holds at most %d columns" % RISK_COLS_MAX)
        if source not in RISK_SOURCES:
            raise ValueError("column %r: source %r, expected one of %s" % (name, source, ", ".join(RISK_SOURCES)))
        src, q = RISK_SOURCES.index(source), 0
        if src >= 4 and (self.kpis is None or len(self.kpis) < 1):
            raise ValueError("column %r: source %r needs the rollout's KPI table (RiskTable(kpis=...))" % (name, source))
        if src >= 5:
            if kpi not in self.kpis.names:
                raise ValueError("column %r: kpi %r is not a KPI of the table (%s)" % (name, kpi, ", ".join(map(str, self.kpis.names))))
            q = self.kpis.names.index(kpi)
        elif kpi is not None:
            raise ValueError("column %r: kpi given, but source %r is not a KPI's" % (name, source))
        if level is not None and np.isnan(float(level)):
            raise ValueError("column %r: level is NaN" % (name,))
        self.names.append(name)
        self._src.append(src)
        self._q.append(q)
        self._level.append(np.inf if level is None else float(level))
        return self

    def arrays(self):
        """the arguments of mld_rollout_risk: dict(col_src, col_q (G,) int32, level (G,) or None where no column gave one, alpha (L,))"""
        if not self.names:
            raise ValueError("the table holds no column")
        level = np.asarray(self._level, dtype=np.float64)
        return dict(col_src=np.asarray(self._src, dtype=np.int32), col_q=np.asarray(self._q, dtype=np.int32),
                    level=None if np.all(np.isposinf(level)) else level, alpha=np.asarray(self.levels, dtype=np.float64))


def risk_rank_table(alpha, S):
    """the rank table the host uploads: idx (L, S) int32 with idx[l, n - 1] = the smallest i >= 0 with float(i + 1) >= alpha[l] * float(n), the index
    ceil(alpha n) - 1, for n = 1 .. S"""
    alpha = np.asarray(alpha, dtype=np.float64).reshape(-1)
    idx = np.zeros((alpha.size, int(S)), np.int32)
    for l, a in enumerate(alpha):
        for n in range(1, int(S) + 1):
            an = np.float64(a) * np.float64(n)
            i = 0
            while i + 1 < n and not (np.float64(i + 1) >= an):
                i += 1
            idx[l, n - 1] = i
    return idx


def _tree64(leaves):
    """T over the last axis (64 leaves): neighbours added pairwise, six times; every addition is one rounded numpy addition"""
    t = np.asarray(leaves, dtype=np.float64)
    while t.shape[-1] > 1:
        t = t.reshape(t.shape[:-1] + (t.shape[-1] // 2, 2))
        t = t[..., 0] + t[..., 1]
    return t[..., 0]


def rollout_risk_np(out, risk, policy=False):
    """GpuProblem.rollout(risk=...)'s "risk" stated in numpy (mld_rollout_risk, kernel k_rollout_risk; the rule: include/mldgpu.h): out the dict rollout()
    returns -- cost, mu_total, worst_vio, end_status (B, S), switches with policy=True, kpi where a column reads one --, risk a RiskTable.  Over the COMPLETE
    realisations of an instance (end_status == 0), sorted ascending by (value, c) with NaN last: mean, min / min_c, max / max_c, n_exceed (B, G); per level
    quantile, quantile_c, cvar_hi, cvar_lo (B, G, L); the counts of the four endings (B,).  The sums are the balanced tree over 64 leaves.
    Returns dict(names, levels, <those arrays>)."""
    arr = risk.arrays()
    es = np.asarray(out["end_status"])
    B, S = es.shape
    if S > RISK_S_MAX:
        raise ValueError("S = %d realisations (at most %d)" % (S, RISK_S_MAX))
    G, L = len(risk), len(risk.levels)
    g = np.zeros((B, G, S))
    for j, (src, q) in enumerate(zip(arr["col_src"], arr["col_q"])):
        if src == 3 and (not policy or "switches" not in out):
            raise ValueError("column %r reads switches: the rollout has to be a policy's (policy=True)" % (risk.names[j],))
        if src >= 4 and "kpi" not in out:
            raise ValueError("column %r reads the KPIs: out has no 'kpi'" % (risk.names[j],))
        if src < 4:
            col = out[RISK_SOURCES[src]]
        elif src == 4:
            col = out["kpi"]["n_vio"]
        else:
            col = np.asarray(out["kpi"][_RISK_KPI_KEYS[int(src)]])[:, :, q]
        g[:, j, :] = np.asarray(col, dtype=np.float64)
    complete = np.broadcast_to((es == 0)[:, None, :], (B, G, S))
    level = np.full(G, np.inf) if arr["level"] is None else arr["level"]
    n = (es == 0).sum(axis=1).astype(np.int32)
    res = dict(names=list(risk.names), levels=list(risk.levels))
    for key, e in zip(RISK_COUNTS, (0, 1, 2, -1)):
        res[key] = (es == e).sum(axis=1).astype(np.int32)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        nan = np.isnan(g) & complete
        c = np.broadcast_to(np.arange(S), (B, G, S))
        order = np.lexsort((c, np.where(nan | ~complete, 0.0, g), nan, ~complete), axis=-1)      # (absent, isnan, g, c): the last key is the first
        pad = lambda a: np.concatenate([a, np.zeros((B, G, 64 - S))], axis=-1)
        srt, r = pad(np.take_along_axis(np.where(complete, g, 0.0), order, axis=-1)), np.arange(64)
        nn = n[:, None].astype(np.float64)
        res["mean"] = np.where(n[:, None] > 0, _tree64(pad(np.where(complete, g, 0.0))) / nn, np.nan)
        m = (complete & ~nan).sum(axis=-1)      # the numbers: sorted[0 .. m)
        some = m > 0
        top = np.take_along_axis(srt, np.maximum(m - 1, 0)[..., None], axis=-1)[..., 0]
        first_top = ((srt == top[..., None]) & (r < m[..., None])).argmax(axis=-1)
        res["min"] = np.where(some, srt[..., 0], np.inf)
        res["min_c"] = np.where(some, order[..., 0], -1).astype(np.int32)
        res["max"] = np.where(some, np.take_along_axis(srt, first_top[..., None], axis=-1)[..., 0], -np.inf)      # (the value at that c: zeros tie, signs may differ)
        res["max_c"] = np.where(some, np.take_along_axis(order, np.minimum(first_top, S - 1)[..., None], axis=-1)[..., 0], -1).astype(np.int32)
        res["n_exceed"] = (complete & (g > level[None, :, None])).sum(axis=-1).astype(np.int32)
        idx = risk_rank_table(arr["alpha"], S)
        res["quantile"], res["cvar_hi"], res["cvar_lo"] = np.full((B, G, L), np.nan), np.full((B, G, L), np.nan), np.full((B, G, L), np.nan)
        res["quantile_c"] = np.full((B, G, L), -1, np.int32)
        live = n > 0
        for l in range(L):
            i = idx[l][np.maximum(n, 1) - 1].astype(np.int64)      # (B,)
            ii = np.broadcast_to(i[:, None, None], (B, G, 1))
            hi = _tree64(np.where((r >= ii) & (r < n[:, None, None]), srt, 0.0)) / (n - i)[:, None].astype(np.float64)
            lo = _tree64(np.where(r <= ii, srt, 0.0)) / (i + 1)[:, None].astype(np.float64)
            at = np.minimum(ii, S - 1)
            res["quantile"][live, :, l] = np.take_along_axis(srt, ii, axis=-1)[..., 0][live]
            res["quantile_c"][live, :, l] = np.take_along_axis(order, at, axis=-1)[..., 0][live]
            res["cvar_hi"][live, :, l], res["cvar_lo"][live, :, l] = hi[live], lo[live]
    return res


# ---- plan selection: the admissible candidate of least objective statistic (GpuProblem.select_plan, mld_rollout_select, kernel k_plan_select) -------------
SELECT_P_MAX, SELECT_CONS_MAX = 64, 8      # MLD_SELECT_P_MAX, MLD_SELECT_CONS_MAX
SELECT_KINDS = ("mean", "min", "max", "n_exceed", "quantile", "cvar_hi", "cvar_lo")      # kind = the index; the last three are per level
SELECT_KEYS = ("choice", "score", "n_admissible", "admissible")


class PlanSelector(object):
    """The rule one selection applies to the risk of every candidate: PlanSelector(risk).minimise(column, kind, level=None).subject_to(column, kind, bound,
    level=None)...  risk: the simlog.RiskTable of the call; column: the name of one of its columns (or its index); kind: one of SELECT_KINDS; level: for
    quantile, cvar_hi and cvar_lo the alpha of one of the table's levels (a float) or its index (an int), None for the other kinds.  A candidate is
    admissible iff it has at least min_complete complete realisations, every constraint's value <= bound holds (a NaN fails) and its objective is not NaN;
    the choice is the admissible candidate of least objective, the smaller p on a tie (include/mldgpu.h: THE RULE)."""

    def __init__(self, risk):
        if not isinstance(risk, RiskTable) or len(risk) < 1:
            raise ValueError("PlanSelector(risk): a simlog.RiskTable with at least one column")
        self.risk = risk
        self.objective = None
        self.constraints = []      # (col, kind, lvl, bound)

    def _stat(self, column, kind, level):
        if isinstance(column, (int, np.integer)) and not isinstance(column, bool):
            col = int(column)
            if not 0 <= col < len(self.risk):
                raise ValueError("column %d, but the risk table has %d columns" % (col, len(self.risk)))
        elif column in self.risk.names:
            col = self.risk.names.index(column)
        else:
            raise ValueError("column %r is not a column of the risk table (%s)" % (column, ", ".join(map(str, self.risk.names))))
        if kind not in SELECT_KINDS:
            raise ValueError("kind %r, expected one of %s" % (kind, ", ".join(SELECT_KINDS)))
        k = SELECT_KINDS.index(kind)
        if k < 4:
            if level is not None:
                raise ValueError("level given, but kind %r is not per level" % (kind,))
            return col, k, 0
        L = len(self.risk.levels)
        if level is None:
            raise ValueError("kind %r is per level: level= one of the risk table's levels %s" % (kind, self.risk.levels))
        if isinstance(level, (int, np.integer)) and not isinstance(level, bool):
            lvl = int(level)
            if not 0 <= lvl < L:
                raise ValueError("level index %d, but the risk table has %d levels" % (lvl, L))
        elif float(level) in self.risk.levels:
            lvl = self.risk.levels.index(float(level))
        else:
            raise ValueError("level %r is not a level of the risk table (%s)" % (level, self.risk.levels))
        return col, k, lvl

    def minimise(self, column, kind, level=None):
        """the objective statistic (once)"""
        if self.objective is not None:
            raise ValueError("the objective has been set already")
        self.objective = self._stat(column, kind, level)
        return self

    def subject_to(self, column, kind, bound, level=None):
        """one constraint value <= bound, at most SELECT_CONS_MAX; a NaN bound is a ValueError"""
        if len(self.constraints) >= SELECT_CONS_MAX:
            raise ValueError("a selector holds at most %d constraints" % SELECT_CONS_MAX)
        bound = float(bound)
        if np.isnan(bound):
            raise ValueError("the bound is NaN")
        self.constraints.append(self._stat(column, kind, level) + (bound,))
        return self

    def arrays(self):
        """the arguments of mld_rollout_select: dict(obj (col, kind, level index), n_cons, cons_col, cons_kind, cons_level (n_cons,) int32, cons_bound)"""
        if self.objective is None:
            raise ValueError("the selector has no objective (minimise(...))")
        c = self.constraints
        return dict(obj=self.objective, n_cons=len(c), cons_col=np.asarray([a[0] for a in c], dtype=np.int32), cons_kind=np.asarray([a[1] for a in c], dtype=np.int32),
                    cons_level=np.asarray([a[2] for a in c], dtype=np.int32), cons_bound=np.asarray([a[3] for a in c], dtype=np.float64))


def _select_value(risk, col, kind, lvl):
    """the statistic (col, kind, lvl) of every candidate: (B, P) float64"""
    a = np.asarray(risk[SELECT_KINDS[kind]])
    return np.asarray(a[:, :, col, lvl] if kind >= 4 else a[:, :, col], dtype=np.float64)


def select_plan_np(risk_per_candidate, selector, min_complete, candidates=None, policy_u0=None):
    """GpuProblem.select_plan's choice stated in numpy (mld_rollout_select, kernel k_plan_select; the rule: include/mldgpu.h): risk_per_candidate the
    per-candidate risk -- mean, min, max, n_exceed (B, P, G), quantile, cvar_hi, cvar_lo (B, P, G, L), n_complete (B, P) --, selector a PlanSelector,
    min_complete the least number of complete realisations.  Returns dict(choice (B,) int32, -1 = none; score (B,), NaN without a choice; n_admissible (B,)
    int32; admissible (B, P) bool); with candidates (B, P, K, nu) also u (B, K, nu) and u0 (B, nu), the chosen sequence and its step 0, NaN without a choice.
    policy_u0 (B, T, nu) (select_plan_policies(policies=...), mld_rollout_select_policy): the last T of the P candidates are closed-loop policies and policy_u0 their
    step-0 inputs, policy.apply_np(P_t, model_idx, x0, u_prev); candidates is then (B, P - T, K, nu), the plan and the sequences ((B, 0, K, nu) where P == T: the empty array carries K; None there means K = 1).  The result
    gains policy (B,) int32, the index of the chosen policy or -1; where the choice is a policy u0 is its policy_u0 row, u[:, 0] that row and u[:, 1:] NaN."""
    arr = selector.arrays()
    val = _select_value(risk_per_candidate, *arr["obj"])
    B, P = val.shape
    with np.errstate(invalid="ignore"):
        adm = (np.asarray(risk_per_candidate["n_complete"]).reshape(B, P) >= int(min_complete)) & ~np.isnan(val)
        for k in range(arr["n_cons"]):
            adm &= _select_value(risk_per_candidate, int(arr["cons_col"][k]), int(arr["cons_kind"][k]), int(arr["cons_level"][k])) <= arr["cons_bound"][k]
    rows = np.arange(B)
    first = np.where(adm, val, np.inf).argmin(axis=1)      # argmin: the first of equals, -0.0 == +0.0
    first = np.where(adm[rows, first], first, adm.argmax(axis=1))      # (every admissible value is +inf: an inadmissible +inf came first -- the first admissible)
    choice = np.where(adm.any(axis=1), first, -1).astype(np.int32)
    some = choice >= 0
    score = np.where(some, val[rows, np.maximum(choice, 0)], np.nan)
    out = dict(choice=choice, score=score, n_admissible=adm.sum(axis=1).astype(np.int32), admissible=adm)
    if policy_u0 is not None:
        pu0 = np.asarray(policy_u0, dtype=np.float64)
        T, nu = pu0.shape[1:]
        n_seq = P - T
        if pu0.shape[0] != B or T > P or (n_seq > 0 and candidates is None):
            raise ValueError("policy_u0 has shape %s for %d instances and %d candidates, %d of them sequences%s" % (pu0.shape, B, P, n_seq, "" if candidates is not None else " (candidates is None)"))
        cand = np.zeros((B, 0, 1, nu)) if candidates is None else np.asarray(candidates, dtype=np.float64)
        if cand.shape[0] != B or cand.shape[1] != n_seq or cand.shape[3] != nu:
            raise ValueError("candidates has shape %s, expected (%d, %d, K, %d): the plan and the sequences in front of the %d policies" % (cand.shape, B, n_seq, nu, T))
        K = cand.shape[2]
        pol = np.where(choice >= n_seq, choice - n_seq, -1).astype(np.int32)
        u = np.full((B, K, nu), np.nan)
        seq = some & (pol < 0)
        u[seq] = cand[rows[seq], choice[seq]]
        u[pol >= 0, 0] = pu0[rows[pol >= 0], pol[pol >= 0]]
        out.update(u=u, u0=np.ascontiguousarray(u[:, 0, :]), policy=pol)
    elif candidates is not None:
        cand = np.asarray(candidates, dtype=np.float64)
        u = np.where(some[:, None, None], cand[rows, np.maximum(choice, 0)], np.nan)
        out.update(u=u, u0=np.ascontiguousarray(u[:, 0, :]))
    return out


def start_from_rollout_np(v, end_status, bins, old=None):
    """GpuProblem.warm_start_from_rollout's byte rule stated in numpy (kernel k_warm_from_rollout): v (B, N_tilde, nv) or (B, 1, N_tilde, nv) of a rollout with
    S = 1, end_status (B,) or (B, 1), bins (n_bin,) the binaries' indices step * nv + pos (np.flatnonzero(GpuProblem.is_bin)), old (B, n_bin) the resident
    start for keep=True, or None.  Row b: kept where old[b, 0] != 255; else v[b].ravel()[bins] > 0.5 (a NaN rounds to 0) where the trajectory ended 0, and
    255 everywhere for any other ending.  Returns (start (B, n_bin) uint8, source (B,) int32: 1 written, 0 kept, -1 / -2 / -3 for the endings 1 / 2 / -1)."""
    end = np.asarray(end_status).reshape(-1).astype(np.int64)
    B = end.size
    flat = np.asarray(v, dtype=np.float64).reshape(B, -1)
    bins = np.asarray(bins, dtype=np.int64).reshape(-1)
    start = np.where(end[:, None] == 0, flat[:, bins] > 0.5, 255).astype(np.uint8)
    source = np.select([end == 0, end == 1, end == 2], [1, -1, -2], -3).astype(np.int32)
    if old is not None:
        old = np.asarray(old, dtype=np.uint8).reshape(B, bins.size)
        kept = old[:, 0] != 255 if bins.size else np.zeros(B, bool)
        start[kept], source[kept] = old[kept], 0
    return start, source
