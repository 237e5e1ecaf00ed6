"""Rule-based feedback policies u_k = f(x_k, u_{k-1}) for the plant step and the rollout of a resident batch.

The reference's simulation campaign compares its MPC variants against `thermo`, DewhTheromstatController
(examples/residential_mg_with_pv_and_dewhs/controllers/theromstat_control.py:38-64): a hysteresis rule per tank, stepped through sim_step_k like
every other controller.  `ThresholdPolicy` is that rule per model and input channel, in a form the device can apply where the state lives
(GpuProblem.upload_policy, rollout(policy=True), sim_step(resolve=R, policy=True)); `apply_np` is its numpy statement.

A channel j of model m is either passed through (mode 0: its value comes from the caller's inputs or the resident plan, as without a policy) or ruled
(mode 1).  With s = sum_i sel[m, j, i] x[i] (fp64, i ascending):

    s <= on_at            u = u_on                (:53)
    s >= off_at           u = u_off               (:55)
    u_prev[j] == u_on     u = u_on                (:57: exact equality, the reference's `== 1`)
    otherwise             u = u_off

in this order: a NaN s falls through to the last two lines, and with on_at == off_at the first line wins.
"""
import numpy as np


class ThresholdPolicy(object):
    """sel (n_models, nu, nx) selector rows; on_at, off_at, u_on, u_off (n_models, nu) (scalars and (nu,) rows are broadcast); mode (n_models, nu)
    int32, 0 = passed through, 1 = ruled (None: every channel ruled).  ValueError unless the shapes match, every value is finite, on_at <= off_at and
    mode is 0 or 1."""

    def __init__(self, sel, on_at, off_at, u_on=1.0, u_off=0.0, mode=None):
        sel = np.array(sel, dtype=np.float64)
        if sel.ndim != 3:
            raise ValueError("sel has shape %s, expected (n_models, nu, nx)" % (sel.shape,))
        M, nu, nx = sel.shape
        cols = {}
        for name, a in (("on_at", on_at), ("off_at", off_at), ("u_on", u_on), ("u_off", u_off)):
            a = np.asarray(a, dtype=np.float64)
            if a.ndim > 2 or (a.ndim == 2 and a.shape != (M, nu)) or (a.ndim == 1 and a.shape != (nu,)):
                raise ValueError("%s has shape %s, expected (%d, %d), (%d,) or a scalar" % (name, a.shape, M, nu, nu))
            cols[name] = np.array(np.broadcast_to(a, (M, nu)), dtype=np.float64)
        if mode is None:
            mode = np.ones((M, nu), np.int32)
        mode_in = np.asarray(mode)
        if mode_in.ndim > 2 or (mode_in.ndim == 2 and mode_in.shape != (M, nu)) or (mode_in.ndim == 1 and mode_in.shape != (nu,)):
            raise ValueError("mode has shape %s, expected (%d, %d), (%d,) or a scalar" % (mode_in.shape, M, nu, nu))
        mode_in = np.broadcast_to(mode_in, (M, nu))
        if not np.all((mode_in == 0) | (mode_in == 1)):
            raise ValueError("mode holds values other than 0 (passed through) and 1 (ruled)")
        for name, a in (("sel", sel),) + tuple(cols.items()):
            if not np.all(np.isfinite(a)):
                raise ValueError("%s is not finite" % name)
        if np.any(cols["on_at"] > cols["off_at"]):
            m, j = np.argwhere(cols["on_at"] > cols["off_at"])[0]
            raise ValueError("on_at > off_at for model %d, channel %d (%g > %g): the band between the thresholds would be empty" % (m, j, cols["on_at"][m, j], cols["off_at"][m, j]))
        self.sel = np.ascontiguousarray(sel)
        self.on_at, self.off_at, self.u_on, self.u_off = (np.ascontiguousarray(cols[k]) for k in ("on_at", "off_at", "u_on", "u_off"))
        self.mode = np.ascontiguousarray(mode_in, dtype=np.int32)
        self.n_models, self.nu, self.nx = M, nu, nx

    @classmethod
    def thermostat(cls, T_on, T_off, n_models, nx=None):
        """the reference's thermostat: channel j switches on state j (unit selectors, nu == nx); T_on / T_off scalars, (nx,) or (n_models, nx) -- on at or
        below T_on, off at or above T_off, inputs 1 / 0.  nx is taken from the thresholds unless given."""
        if nx is None:
            nx = max(np.shape(np.atleast_1d(T_on))[-1], np.shape(np.atleast_1d(T_off))[-1])
        sel = np.broadcast_to(np.eye(int(nx)), (int(n_models), int(nx), int(nx)))
        return cls(sel, T_on, T_off, 1.0, 0.0)

    @property
    def all_ruled(self):
        return bool(np.all(self.mode == 1))

    def initial_state(self, model_idx, batch=None):
        """u_prev before the first step, (batch, nu): a ruled channel holds its model's u_off (the reference's first step has no previous record, so
        `u_k_neg1 == 1` is false), a passed-through one 0"""
        midx = np.zeros(int(batch), np.int64) if model_idx is None else np.asarray(model_idx, np.int64)
        return np.where(self.mode[midx] == 1, self.u_off[midx], 0.0)


def apply_np(P, model_idx, x, u_prev, u_pass=None):
    """the rule in numpy: x (B, nx), u_prev (B, nu), model_idx (B,) or None = model 0, u_pass (B, nu) the values of the passed-through channels
    (None: zeros).  Returns u (B, nu)."""
    x = np.asarray(x, dtype=np.float64).reshape(-1, P.nx)
    B = x.shape[0]
    midx = np.zeros(B, np.int64) if model_idx is None else np.asarray(model_idx, np.int64).reshape(B)
    u_prev = np.broadcast_to(np.asarray(u_prev, dtype=np.float64), (B, P.nu))
    u_pass = np.zeros((B, P.nu)) if u_pass is None else np.broadcast_to(np.asarray(u_pass, dtype=np.float64), (B, P.nu))
    sel = P.sel[midx]
    s = np.zeros((B, P.nu))
    for i in range(P.nx):                                   # i ascending, as the kernels sum
        s = s + sel[:, :, i] * x[:, None, i]
    on, off, u_on, u_off = P.on_at[midx], P.off_at[midx], P.u_on[midx], P.u_off[midx]
    with np.errstate(invalid="ignore"):
        u = np.where(s <= on, u_on, np.where(s >= off, u_off, np.where(u_prev == u_on, u_on, u_off)))
    return np.where(P.mode[midx] == 1, u, u_pass)


def selector_values(P, model_idx, x):
    """s = sel x per instance and channel, (B, nu): what the thresholds are compared with (tests guard their distance to both thresholds)"""
    x = np.asarray(x, dtype=np.float64).reshape(-1, P.nx)
    midx = np.zeros(x.shape[0], np.int64) if model_idx is None else np.asarray(model_idx, np.int64)
    return np.einsum("bji,bi->bj", P.sel[midx], x)


def switches_np(P, model_idx, u, u_prev):
    """the number of (step, ruled channel) pairs with u_k[j] != u_{k-1}[j]: u (B, K, nu), u_prev (B, nu) the input before step 0.  Returns (B,) int32."""
    u = np.asarray(u, dtype=np.float64)
    B = u.shape[0]
    midx = np.zeros(B, np.int64) if model_idx is None else np.asarray(model_idx, np.int64)
    before = np.concatenate([np.asarray(u_prev, dtype=np.float64).reshape(B, 1, P.nu), u[:, :-1]], axis=1)
    return ((u != before) & (P.mode[midx] == 1)[:, None, :]).sum(axis=(1, 2)).astype(np.int32)
