"""fp64 numpy reference of the solution quality of a batch (mld_evaluate_batch, GpuProblem.evaluate), restated from the oracle's pieces: the
condensed maps of condense_np (H_v, H_x, H_omega, H_5), the variable kinds and bounds of cn.standard_form (is_bin / lb / ub), and the cost of
cn.lin_cost / cn.cost_const / _paths.ref_cost.  No GPU; checked against facts by tests/test_quality_host.py.

Next to every value it returns the scale its rounding error is proportional to -- the sum of the absolute values of the terms that were added
up -- so that a test can bound |device - reference| by (a multiple of the unit roundoff) x scale, whatever cancels in the value itself."""
import numpy as np

import _paths
import condense_np as cn


def model_ref(mats, d, N):
    """what the reference needs of one model (a dict of matrices, or a list of N step models): evo, is_bin, lb, ub"""
    sf = cn.standard_form(mats, {}, max(1, N - 1), N, nu_l=d.get("nu_l", 0), nmu_l=d.get("nmu_l", 0))
    return dict(evo=sf["evo"], is_bin=sf["is_bin"], lb=sf["lb"], ub=sf["ub"])


def point_quality(is_bin, lb, ub, v):
    """int_vio (B): max over the binaries |v_j - rint(v_j)|, 0 without binaries; bound_vio (B): the largest violation of lb <= v <= ub, >= 0.
    Elementwise fp64 and an exact maximum: a device result must equal these bit for bit."""
    v = np.atleast_2d(np.asarray(v, np.float64))
    B = v.shape[0]
    iv = np.abs(v[:, is_bin] - np.rint(v[:, is_bin])).max(axis=1) if is_bin.any() else np.zeros(B)
    viol = np.maximum(lb[None, :] - v, v - ub[None, :])           # -inf where a side is free
    bv = np.maximum(0.0, viol.max(axis=1)) if v.shape[1] else np.zeros(B)
    return iv, bv


def residuals(evo, v, X, W):
    """r = H_v v - (H_x x + H_omega omega + H_5) per instance and row (B, m0), and per row the sum of the absolute terms"""
    Hv, Hx, Hw, H5 = evo["H_v"], evo["H_x"], evo["H_omega"], evo["H_5"][:, 0]
    r = v @ Hv.T - (X @ Hx.T + W @ Hw.T + H5)
    s = np.abs(v) @ np.abs(Hv).T + np.abs(X) @ np.abs(Hx).T + np.abs(W) @ np.abs(Hw).T + np.abs(H5)
    return r, s


def constraint_quality(evo, v, x0, om, omega_cols=None, col_rows=None, x_cols=None):
    """per validation column: constr_vio (B, C) = max over the column's leading col_rows[c] rows of r, -inf for a column without rows; constr_row
    (B, C) the first row that attains it, -1 without rows; S (B, C) the row scale max_i (|H_v||v| + |H_x||x| + |H_omega||omega| + |H_5|)_i over the
    same rows; R (B, C, m0) every residual.  omega_cols None: one column, the instance's own (x0, omega), all rows."""
    B, m0 = v.shape[0], evo["H_v"].shape[0]
    if omega_cols is None and x_cols is None:
        cols = [(x0, om, m0)]
    else:
        C = (omega_cols if omega_cols is not None else x_cols).shape[1]
        cols = [(x_cols[:, c] if x_cols is not None else x0, omega_cols[:, c] if omega_cols is not None else om,
                 m0 if col_rows is None else int(col_rows[c])) for c in range(C)]
    vio, row = np.full((B, len(cols)), -np.inf), np.full((B, len(cols)), -1, np.int64)
    S, R = np.zeros((B, len(cols))), np.zeros((B, len(cols), m0))
    for c, (X, W, rows) in enumerate(cols):
        r, s = residuals(evo, v, X, W)
        R[:, c] = r
        if rows > 0:
            vio[:, c], row[:, c], S[:, c] = r[:, :rows].max(axis=1), r[:, :rows].argmax(axis=1), s[:, :rows].max(axis=1)
    return dict(constr_vio=vio, constr_row=row, S=S, R=R, rows=np.array([c[2] for c in cols]))


def as_posed(cq):
    """the maximum over the columns of constraint_quality (the problem as posed: standard block and constraint blocks): vio (B), row (B), S (B)"""
    if cq["constr_vio"].shape[1] == 0:
        B = cq["constr_vio"].shape[0]
        return np.full(B, -np.inf), np.full(B, -1, np.int64), np.zeros(B)
    c = cq["constr_vio"].argmax(axis=1)
    b = np.arange(c.size)
    return cq["constr_vio"][b, c], cq["constr_row"][b, c], cq["S"].max(axis=1)


def cost_of(evo, **c):
    """_paths.ref_cost's P, q0, Qx, Qw of lin_* / quad_* weights plus the pieces of the constant in the form of cn.assemble_cost's const_terms"""
    cost = _paths.ref_cost(evo, **c)
    terms = []
    for k, (Mx, Mw, m5) in (("x", ("Phi_x", "Gamma_omega", "Gamma_5")), ("y", ("L_x", "L_omega", "L_5"))):
        if evo[Mx].shape[0] == 0:
            continue
        if c.get("lin_" + k) is not None:
            terms.append(("lin", np.asarray(c["lin_" + k], np.float64).reshape(-1), evo[Mx], evo[Mw], evo[m5]))
        if c.get("quad_" + k) is not None:
            terms.append(("quad", np.asarray(c["quad_" + k], np.float64), evo[Mx], evo[Mw], evo[m5]))
    cost["const_terms"] = terms
    return cost


def const_value(const_terms, x0, om):
    """cn.cost_const for a batch: the constant r(x0, omega) (B) -- the objective at v = 0 -- and the sum of its absolute terms"""
    B = x0.shape[0]
    r, a = np.zeros(B), np.zeros(B)
    for kind, w, Mx, Mw, m0 in const_terms:
        e = x0 @ Mx.T + om @ Mw.T + m0[:, 0]
        ea = np.abs(x0) @ np.abs(Mx).T + np.abs(om) @ np.abs(Mw).T + np.abs(m0[:, 0])
        if kind == "lin":
            w = np.asarray(w, np.float64).reshape(-1)
            r += e @ w
            a += ea @ np.abs(w)
        else:
            r += np.einsum("bi,ij,bj->b", e, w, e)
            a += np.einsum("bi,ij,bj->b", ea, np.abs(w), ea)
    return r, a


def objective(evo, cost, v, x0, om, inst=None):
    """obj (B) = 1/2 v'Pv + (q0 + Qx x0 + Qw omega + q_b)'v + constant and the sum of the absolute terms.  cost: dict(P, q0, Qx, Qw, const_terms) or
    None; inst: dict(lin_v, lin_x, lin_y) of (B, len) per-instance weights (mld_upload_instance_cost) or None"""
    B, n = v.shape
    obj, scale = np.zeros(B), np.zeros(B)
    q, qa = np.zeros((B, n)), np.zeros((B, n))
    if cost is not None:
        q += cost["q0"] + x0 @ cost["Qx"].T + om @ cost["Qw"].T                 # cn.lin_cost, batched
        qa += np.abs(cost["q0"]) + np.abs(x0) @ np.abs(cost["Qx"]).T + np.abs(om) @ np.abs(cost["Qw"]).T
        obj += 0.5 * np.einsum("bi,ij,bj->b", v, cost["P"], v)
        scale += 0.5 * np.einsum("bi,ij,bj->b", np.abs(v), np.abs(cost["P"]), np.abs(v))
        r, a = const_value(cost["const_terms"], x0, om)
        obj += r; scale += a
    if inst:
        for lin, Mv, Mx, Mw, m5 in ((inst.get("lin_x"), "Gamma_v", "Phi_x", "Gamma_omega", "Gamma_5"), (inst.get("lin_y"), "L_v", "L_x", "L_omega", "L_5")):
            if lin is None:
                continue
            q += lin @ evo[Mv]
            qa += np.abs(lin) @ np.abs(evo[Mv])
            e = x0 @ evo[Mx].T + om @ evo[Mw].T + evo[m5][:, 0]
            ea = np.abs(x0) @ np.abs(evo[Mx]).T + np.abs(om) @ np.abs(evo[Mw]).T + np.abs(evo[m5][:, 0])
            obj += np.einsum("bi,bi->b", lin, e); scale += np.einsum("bi,bi->b", np.abs(lin), ea)
        if inst.get("lin_v") is not None:
            q += inst["lin_v"]; qa += np.abs(inst["lin_v"])
    obj += np.einsum("bi,bi->b", q, v)
    scale += np.einsum("bi,bi->b", qa, np.abs(v))
    return obj, scale


def quality(ref, v, x0, om, omega_cols=None, col_rows=None, x_cols=None, cost=None, inst=None):
    """the five outputs of evaluate() for the model_ref `ref`, plus S (the row scale per (instance, column)), obj_scale and R"""
    v, x0, om = np.atleast_2d(v), np.atleast_2d(x0), np.atleast_2d(om)
    cq = constraint_quality(ref["evo"], v, x0, om, omega_cols, col_rows, x_cols)
    iv, bv = point_quality(ref["is_bin"], ref["lb"], ref["ub"], v)
    obj, oscale = objective(ref["evo"], cost, v, x0, om, inst)
    out = dict(obj=obj, obj_scale=oscale, int_vio=iv, bound_vio=bv, S=cq["S"], R=cq["R"], rows=cq["rows"])
    if omega_cols is None and x_cols is None:
        out["constr_vio"], out["constr_row"], out["S"] = cq["constr_vio"][:, 0], cq["constr_row"][:, 0], cq["S"][:, 0]
    else:
        out["constr_vio"], out["constr_row"] = cq["constr_vio"], cq["constr_row"]
    return out
