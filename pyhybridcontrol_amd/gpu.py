"""Thin object wrappers over the C ABI handles of libmldgpu (mld_model_t / mld_problem_t)."""
import ctypes as C
import functools
import os

import numpy as np

from . import _lib
from . import fallback as _fallback
from ._lib import MAT_NAMES, EVO_NAMES, MldGpuError, check

_MAT_SHAPES = dict(A=("nx", "nx"), B1=("nx", "nu"), B2=("nx", "ndelta"), B3=("nx", "nz"), B4=("nx", "nomega"),
                   b5=("nx", 1), C=("ny", "nx"), D1=("ny", "nu"), D2=("ny", "ndelta"), D3=("ny", "nz"),
                   D4=("ny", "nomega"), d5=("ny", 1), E=("nc", "nx"), F1=("nc", "nu"), F2=("nc", "ndelta"),
                   F3=("nc", "nz"), F4=("nc", "nomega"), f5=("nc", 1), G=("nc", "ny"), Psi=("nc", "nmu"))


def mat_shape(name, dims):
    r, c = _MAT_SHAPES[name]
    return (dims[r] if isinstance(r, str) else r, dims[c] if isinstance(c, str) else c)


def evo_shapes(dims, N):
    nx, ny, nc, nw = dims["nx"], dims["ny"], dims["nc"], dims["nomega"]
    nv = dims["nu"] + dims["ndelta"] + dims["nz"] + dims["nmu"]
    return dict(Phi_x=(N * nx, nx), Gamma_v=(N * nx, N * nv), Gamma_omega=(N * nx, N * nw), Gamma_5=(N * nx, 1),
                L_x=(N * ny, nx), L_v=(N * ny, N * nv), L_omega=(N * ny, N * nw), L_5=(N * ny, 1),
                H_x=(N * nc, nx), H_v=(N * nc, N * nv), H_omega=(N * nc, N * nw), H_5=(N * nc, 1))


class GpuModel(object):
    """n_models same-shaped numeric MLD systems resident in HBM (mld_model_create)."""

    def __init__(self, mats_list, dims, time_varying=False):
        """mats_list: list of dicts name -> 2-D array (missing / empty = zeros); dims: dict with
        nx,nu,ndelta,nz,nmu,nomega,ny,nc,nu_l,nmu_l.
        time_varying: mats_list is a list of horizons, each a list of N_tilde step models (mld_model_create_tv)."""
        if isinstance(mats_list, dict):
            mats_list = [mats_list]
        self.dims = {k: int(dims.get(k, 0)) for k in ("nx", "nu", "ndelta", "nz", "nmu", "nomega", "ny", "nc", "nu_l", "nmu_l")}
        self.tv_N = 0
        n_sets = len(mats_list)
        if time_varying:
            self.tv_N = len(mats_list[0])
            if self.tv_N < 1 or any(len(h) != self.tv_N for h in mats_list):
                raise ValueError("every horizon needs the same number (>= 1) of step models")
            mats_list = [m for h in mats_list for m in h]
        self.n_models = len(mats_list)
        self.nv = self.dims["nu"] + self.dims["ndelta"] + self.dims["nz"] + self.dims["nmu"]
        self._keep = []
        ptrs = (C.POINTER(C.c_double) * 20)()
        for k, name in enumerate(MAT_NAMES):
            shp = mat_shape(name, self.dims)
            if shp[0] * shp[1] == 0:
                ptrs[k] = None
                continue
            stack = np.zeros((self.n_models,) + shp)
            any_given = False
            for i, mats in enumerate(mats_list):
                a = mats.get(name)
                if a is None or np.size(a) == 0:
                    continue
                a = np.asarray(a, dtype=np.float64)
                if a.shape != shp:
                    a = a.reshape(shp)
                stack[i] = a
                any_given = True
            if any_given:
                self._keep.append(stack)
                ptrs[k] = _lib.dptr(stack)
            else:
                ptrs[k] = None
        d = _lib.Dims(**self.dims)
        self._h = C.c_void_p()
        if self.tv_N:
            check(_lib.load().mld_model_create_tv(C.byref(self._h), C.byref(d), n_sets, self.tv_N, ptrs))
        else:
            check(_lib.load().mld_model_create(C.byref(self._h), C.byref(d), self.n_models, ptrs))
        self.n_models = n_sets
        self._keep = []

    def close(self):
        if getattr(self, "_h", None):
            _lib.load().mld_model_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def condense_device(self, N_tilde, f32=False):
        """run K1+K2 into device-resident buffers (fp32 materialisation with f32=True); returns kernel milliseconds (HIP events)"""
        ms = C.c_double()
        fn = _lib.load().mld_condense_device_f32 if f32 else _lib.load().mld_condense_device
        check(fn(self._h, int(N_tilde), 0, C.byref(ms)))
        return ms.value

    def condense(self, N_tilde, names=EVO_NAMES, dtype=np.float64):
        """materialised evolution matrices, dict name -> (n_models, rows, cols) arrays; dtype np.float32 = mld_condense_f32"""
        shapes = evo_shapes(self.dims, int(N_tilde))
        f32 = np.dtype(dtype) == np.float32
        out, ptrs = {}, []
        for nm in EVO_NAMES:
            if nm in names:
                out[nm] = np.zeros((self.n_models,) + shapes[nm], dtype=np.float32 if f32 else np.float64)
                ptrs.append(out[nm].ctypes.data_as(C.POINTER(C.c_float)) if f32 else _lib.dptr(out[nm]))
            else:
                ptrs.append(None)
        check((_lib.load().mld_condense_f32 if f32 else _lib.load().mld_condense)(self._h, int(N_tilde), 0, *ptrs))
        return out


def expand_open_nodes(fix, depth, var, val, flag, pos):
    """The open nodes a stopped depth-first search leaves behind, from its stack (mld_download_open_nodes): `fix` are the fixings the search
    itself ran under (uint8 per binary, 255 = free), level k of the stack branched on decision-vector entry var[k] (pos maps it to its binary
    position), currently at val[k]; flag[k] = 1 when both children of that level are accounted for.  Returned: one fixing array per open node --
    for every level whose sibling has not been visited {levels above at their values, this level flipped}, and last the current path itself.
    The nodes are pairwise disjoint and together cover exactly what the search had not closed (tests/test_host.py)."""
    res, path = [], np.array(fix, dtype=np.uint8, copy=True)
    for k in range(int(depth)):
        kp = int(pos[int(var[k])])
        if not flag[k]:
            f = path.copy()
            f[kp] = 1 - int(val[k])
            res.append(f)
        path[kp] = int(val[k])
    res.append(path)
    return res


class _MergeIO(C.Structure):
    _fields_ = ([(k, C.c_int32) for k in ("batch", "cap", "n", "tail")] + [("gap_abs", C.c_double), ("gap_rel", C.c_double)] +
                [(k, C.POINTER(C.c_double)) for k in ("obj", "lbnd", "v")] +
                [(k, C.POINTER(C.c_int32)) for k in ("status", "nodes", "pivots", "cuts", "refac")] + [("rows", C.POINTER(C.c_int64))] +
                [("item_root", C.POINTER(C.c_int32)), ("item_label", C.POINTER(C.c_int64)), ("tree_dead", C.POINTER(C.c_int32))] +
                [("n_unfinished", C.c_int32), ("finished", C.c_int32)])


def debug_merge(batch, tail, obj, lbnd, status, nodes, pivots, cuts, refac, rows, v, item_root, item_label, tree_dead, gap_abs=1e-9, gap_rel=0.0):
    """diagnostics: the in-kernel hand-off's merge (k_merge_*, the function the solve path runs) on a queue of the caller's (internal entry
    mld_debug_merge).  Per-entry arrays of cap = len(obj) entries: `batch` roots, then the items up to `tail`; v (cap, n); item_root / item_label per
    entry (read in [batch, tail)); tree_dead per root.  Returns the roots' merged obj, lower_bound, status, nodes, pivots, cuts, refac, rows, v plus
    n_unfinished and given_up = (trees given up for their size, trees given up for a full queue).  The inputs are not modified."""
    f64 = lambda a: np.array(a, dtype=np.float64, order="C")
    i32 = lambda a: np.array(a, dtype=np.int32, order="C")
    i64 = lambda a: np.array(a, dtype=np.int64, order="C")
    a = dict(obj=f64(obj), lbnd=f64(lbnd), v=f64(v), status=i32(status), nodes=i32(nodes), pivots=i32(pivots), cuts=i32(cuts), refac=i32(refac),
             rows=i64(rows), item_root=i32(item_root), item_label=i64(item_label), tree_dead=i32(tree_dead))
    cap = a["obj"].shape[0]
    a["v"] = a["v"].reshape(cap, -1)
    for k in ("lbnd", "status", "nodes", "pivots", "cuts", "refac", "rows", "item_root", "item_label"):
        if a[k].shape != (cap,):
            raise ValueError("debug_merge: %s needs %d entries" % (k, cap))
    if a["tree_dead"].shape != (max(0, int(batch)),):
        raise ValueError("debug_merge: tree_dead needs one entry per root")
    io = _MergeIO(batch=int(batch), cap=cap, n=a["v"].shape[1], tail=int(tail), gap_abs=float(gap_abs), gap_rel=float(gap_rel))
    for k, _ in _MergeIO._fields_:
        if k in a:
            setattr(io, k, a[k].ctypes.data_as(dict(_MergeIO._fields_)[k]))
    lib = _lib.load()
    lib.mld_debug_merge.restype = C.c_int
    lib.mld_debug_merge.argtypes = [C.POINTER(_MergeIO)]
    check(lib.mld_debug_merge(C.byref(io)))
    b = int(batch)
    extra = int(io.finished) - int(tail)
    return dict(obj=a["obj"][:b], lower_bound=a["lbnd"][:b], status=a["status"][:b], nodes=a["nodes"][:b], pivots=a["pivots"][:b], cuts=a["cuts"][:b],
                refac=a["refac"][:b], rows=a["rows"][:b], v=a["v"][:b], n_unfinished=int(io.n_unfinished), given_up=(extra % 65536, extra // 65536))


def make_opts(**kw):
    o = _lib.Opts()
    check(_lib.load().mld_opts_default(C.byref(o)))
    alias = dict(MIPGap="gap_rel", NodeLimit="max_nodes", IterationLimit="max_pivots", TimeLimit="time_limit")
    for k, v in kw.items():
        k = alias.get(k, k)
        if not hasattr(o, k):
            raise TypeError("unknown solver option %r" % k)
        setattr(o, k, type(getattr(o, k))(v))
    return o


def _completes(host):
    """adds complete=None | "host" | "device" to an entry of the rollout family (host: the entry has a host completion, its default).  "device" sets
    MLD_ROLLOUT_COMPLETE_DEVICE on the handle for the call -- beside whatever set_rollout_completion() left there -- and puts the handle's mode back in a
    finally; the wrapped method, whose signature stays what it was, reads self._ro_dev and never enters its host completion."""
    def deco(fn):
        @functools.wraps(fn)
        def wrapper(self, *a, complete=None, **kw):
            if complete not in (None, "host", "device"):
                raise ValueError("complete = %r (None, 'host' or 'device')" % (complete,))
            if complete == "host" and not host:
                raise ValueError("complete = 'host': %s() has no host completion (None leaves declined trajectories as they end, 'device' finishes them on the device)" % fn.__name__)
            if complete != "device":
                return fn(self, *a, **kw)
            mode, was = getattr(self, "_ro_mode", 0), getattr(self, "_ro_dev", False)
            check(_lib.load().mld_set_rollout_completion(self._h, mode | _lib.MLD_ROLLOUT_COMPLETE_DEVICE))
            self._ro_dev = True
            try:
                out = fn(self, *a, **kw)
                resolve = a[0] if a else kw.get("resolve")
                if resolve is not None and resolve.problem is not None and self.rollout_completion_stats()["dense_solves"]:
                    resolve.problem.batch = self.batch      # (a completion leaves the resolver laid out as sim_step(resolve=) does)
                return out
            finally:
                self._ro_dev = was
                check(_lib.load().mld_set_rollout_completion(self._h, mode))
        return wrapper
    return deco


def _keeps(fn):
    """adds keep=False to a select entry: True switches mld_keep_selection on for the call, so that its choice stays on the device as the kept selection, and
    corrects the kept arrays where the method finished instances on the host; False switches it off (and frees what an earlier keep=True left).  The wrapped
    method's signature stays what it was.  A select entry that hands over to another one (select_plan_policies() without policies) is one call: the outer keep
    holds."""
    @functools.wraps(fn)
    def wrapper(self, *a, keep=False, **kw):
        if getattr(self, "_sel_in_call", False):
            return fn(self, *a, **kw)
        self._keep_selection(keep)
        self._sel_in_call = True
        try:
            out = fn(self, *a, **kw)
        finally:
            self._sel_in_call = False
        if keep and out["stats"].get("finished_on_host", 0) > 0:      # the device holds what the method returns
            self.set_selection(out["choice"], out["u"], out.get("policy"))
        return out
    return wrapper


class GpuProblem(object):
    """mld_problem_t: condensed constraint maps of a GpuModel + cost + solver workspace, on device."""

    _handoff = (False, 2.0)      # the library's in-kernel hand-off switch and room_factor, as set_handoff left them (its defaults)

    def __init__(self, model, N_p, N_tilde, cost=None, **opts):
        self.model = model
        self.N_p, self.N_tilde = int(N_p), int(N_tilde)
        d = model.dims
        self.n = self.N_tilde * model.nv
        self.m = self.N_tilde * d["nc"]
        self.nW = self.N_tilde * d["nomega"]
        step_bin = np.zeros(model.nv, dtype=bool)
        step_bin[d["nu"] - d["nu_l"]:d["nu"]] = True
        step_bin[d["nu"]:d["nu"] + d["ndelta"]] = True
        omu = d["nu"] + d["ndelta"] + d["nz"]
        step_bin[omu + d["nmu"] - d["nmu_l"]:omu + d["nmu"]] = True
        self.is_bin = np.tile(step_bin, self.N_tilde)
        self.n_bin = int(self.is_bin.sum())
        self.opts = make_opts(**opts)
        self._h = C.c_void_p()
        c, keep = self._cost_struct(cost)
        check(_lib.load().mld_problem_create(C.byref(self._h), model._h, self.N_p, self.N_tilde,
                                             C.byref(c) if c is not None else None, C.byref(self.opts)))
        check(_lib.load().mld_problem_get_opts(self._h, C.byref(self.opts)))      # the size-scaled defaults, resolved
        self.batch = 0

    def _cost_struct(self, cost):
        if not cost:
            return None, []
        M, d, N = self.model.n_models, self.model.dims, self.N_tilde
        lens = dict(lin_v=(self.n,), lin_x=(N * d["nx"],), lin_y=(N * d["ny"],), quad_v=(self.n, self.n),
                    quad_x=(N * d["nx"], N * d["nx"]), quad_y=(N * d["ny"], N * d["ny"]))
        c = _lib.Cost()
        keep = []
        for k, shp in lens.items():
            a = cost.get(k)
            if a is None or int(np.prod(shp)) == 0:
                setattr(c, k, None)
                continue
            a = np.ascontiguousarray(np.broadcast_to(np.asarray(a, np.float64).reshape((-1,) + shp), (M,) + shp))
            keep.append(a)
            setattr(c, k, _lib.dptr(a))
        self._keep_cost = keep
        return c, keep

    def set_cost(self, cost):
        c, keep = self._cost_struct(cost)
        check(_lib.load().mld_problem_set_cost(self._h, C.byref(c) if c is not None else None))

    def cost_assemble(self):
        M, n, nx, nW = self.model.n_models, self.n, self.model.dims["nx"], self.nW
        P, q0 = np.zeros((M, n, n)), np.zeros((M, n))
        Qx, Qw = np.zeros((M, n, nx)), np.zeros((M, n, nW))
        check(_lib.load().mld_cost_assemble(self._h, _lib.dptr(P), _lib.dptr(q0), _lib.dptr(Qx) if nx else None,
                                            _lib.dptr(Qw) if nW else None))
        return dict(P=P, q0=q0, Qx=Qx, Qw=Qw)

    def close(self):
        if getattr(self, "_h", None):
            _lib.load().mld_problem_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- batch ---------------------------------------------------------------------------------
    def upload(self, x0, omega, model_idx=None, fixed_bin=None):
        d = self.model.dims
        x0 = _lib.as_f64(x0).reshape(-1, d["nx"]) if d["nx"] else np.zeros((np.shape(omega)[0] if omega is not None else 1, 0))
        batch = x0.shape[0] if d["nx"] else int(np.asarray(omega).reshape(-1, max(self.nW, 1)).shape[0])
        omega = _lib.as_f64(omega).reshape(batch, self.nW) if self.nW else np.zeros((batch, 0))
        mi = np.ascontiguousarray(model_idx, dtype=np.int32) if model_idx is not None else None
        fb = np.ascontiguousarray(fixed_bin, dtype=np.uint8).reshape(batch, self.n_bin) if fixed_bin is not None else None
        check(_lib.load().mld_upload_batch(
            self._h, batch, mi.ctypes.data_as(C.POINTER(C.c_int32)) if mi is not None else None,
            _lib.dptr(x0) if d["nx"] else None, _lib.dptr(omega) if self.nW else None,
            fb.ctypes.data_as(C.POINTER(C.c_uint8)) if fb is not None else None))
        self.batch = batch
        self._model_idx = None if mi is None else mi.copy()      # (host copy: rollout() finishes declined trajectories with the instances' models)
        return batch

    def upload_constraint_blocks(self, omega_cols, col_rows=None, x_cols=None):
        """extra constraint blocks for the uploaded batch (mld_upload_constraint_blocks_x): omega_cols (batch, n_cols,
        N_tilde*nomega), col_rows (n_cols) leading rows each column constrains (None = all), x_cols (batch, n_cols, nx) the state
        each column was generated with (None = the instance's x0); None / empty clears"""
        if omega_cols is None or np.size(omega_cols) == 0:
            check(_lib.load().mld_upload_constraint_blocks(self._h, 0, None, None))
            return 0
        cols = _lib.as_f64(omega_cols).reshape(self.batch, -1, self.nW)
        n_cols = cols.shape[1]
        cr = None
        if col_rows is not None:
            cr = np.ascontiguousarray(col_rows, dtype=np.int32).reshape(n_cols)
        nx = self.model.dims["nx"]
        xc = _lib.as_f64(x_cols).reshape(self.batch, n_cols, nx) if (x_cols is not None and nx) else None
        check(_lib.load().mld_upload_constraint_blocks_x(self._h, n_cols, _lib.dptr(cols),
                                                         cr.ctypes.data_as(C.POINTER(C.c_int32)) if cr is not None else None,
                                                         _lib.dptr(xc) if xc is not None else None))
        return n_cols

    # -- resident disturbance profiles ----------------------------------------------------------------
    def upload_profiles(self, lib, group_width=None):
        """flat library of disturbance series resident in HBM (mld_upload_profiles), owned by the problem and independent of the batch.  group_width:
        positive widths that sum to nomega, one group of channels per fused device (None = one group of width nomega); a series of group g is stored
        row-major (time, width_g) -- profiles.pack lays series end to end.  A second call replaces the library and invalidates resident starts; an
        empty library frees it."""
        nomega = self.model.dims["nomega"]
        gw = None
        if group_width is not None:
            gw = np.asarray(group_width)
            if gw.ndim != 1 or gw.size < 1 or not np.issubdtype(gw.dtype, np.integer) or np.any(gw < 1) or int(gw.sum()) != nomega:
                raise ValueError("group_width %s: expected positive integer widths that sum to nomega = %d" % (np.asarray(group_width).tolist(), nomega))
            gw = np.ascontiguousarray(gw, dtype=np.int32)
        lib = np.ascontiguousarray(lib, dtype=np.float64)
        if lib.ndim != 1:
            raise ValueError("lib has shape %s, expected a flat array (profiles.pack)" % (lib.shape,))
        check(_lib.load().mld_upload_profiles(self._h, lib.size, _lib.dptr(lib) if lib.size else None, 0 if gw is None else gw.size,
                                              gw.ctypes.data_as(C.POINTER(C.c_int32)) if gw is not None else None))
        self._pf_width = None if not lib.size else ([nomega] if gw is None else [int(w) for w in gw])
        self._pf_lib = lib if lib.size else None      # (the host's array: rollout() cuts the windows of trajectories it finishes on the host out of it)
        self._pf_ccols = 0

    # -- rule-based feedback policy ------------------------------------------------------------------------
    def upload_policy(self, P):
        """a policy.ThresholdPolicy resident on the device (mld_upload_policy), owned by the problem and independent of the batch, like the profile
        library: rollout(policy=True) and sim_step(resolve=R, policy=True) apply it where the state lives.  None removes it.  A new policy resets the
        resident policy state."""
        if P is None:
            check(_lib.load().mld_upload_policy(self._h, None, None, None, None, None, None))
            self._policy = None
            return
        d = self.model.dims
        if (P.n_models, P.nu, P.nx) != (self.model.n_models, d["nu"], d["nx"]):
            raise ValueError("the policy is shaped (n_models %d, nu %d, nx %d), the problem (%d, %d, %d)" % (P.n_models, P.nu, P.nx, self.model.n_models, d["nu"], d["nx"]))
        check(_lib.load().mld_upload_policy(self._h, _lib.dptr(P.sel), _lib.dptr(P.on_at), _lib.dptr(P.off_at), _lib.dptr(P.u_on), _lib.dptr(P.u_off),
                                            P.mode.ctypes.data_as(C.POINTER(C.c_int32))))
        self._policy = P      # (host copy: rollout() applies the rule to the trajectories it finishes on the host)

    def policy_state(self, u_prev=None, reset=False):
        """the resident u_prev (batch, nu) of the policy: the input applied before the next step (mld_set_policy_state / mld_download_policy_state).
        u_prev given: set it ((nu,) is broadcast); reset=True: every ruled channel back to its model's u_off, the state after any upload().  Returns the
        state now resident."""
        B, nu = self.batch, self.model.dims["nu"]
        if u_prev is not None:
            u_prev = np.asarray(u_prev, dtype=np.float64)
            if u_prev.shape == (nu,):
                u_prev = np.broadcast_to(u_prev, (B, nu))
            if u_prev.shape != (B, nu):
                raise ValueError("u_prev has shape %s, expected (%d, %d) or (%d,)" % (u_prev.shape, B, nu, nu))
            check(_lib.load().mld_set_policy_state(self._h, _lib.dptr(np.ascontiguousarray(u_prev))))
        elif reset:
            check(_lib.load().mld_set_policy_state(self._h, None))
        out = np.zeros((B, nu))
        check(_lib.load().mld_download_policy_state(self._h, _lib.dptr(out)))
        return out

    # -- fallback inputs for instances without a usable plan ----------------------------------------------
    def plan_memory(self, enable=True):
        """the resident plan memory of the batch (mld_plan_memory): enable allocates it and empties it (every age -1), False frees it.  An advancing
        sim_step(resolve=R, fallback=...) remembers every usable plan's inputs in it and ages the others'; fallback=("memory", ...) lets an instance
        without a usable plan take the remembered row for the current time.  upload(), select(), advance() and an advancing step through any other
        entry empty it."""
        check(_lib.load().mld_plan_memory(self._h, 1 if enable else 0))

    def plan_memory_state(self, u=None, age=None):
        """the plan memory (mld_set_plan_memory / mld_download_plan_memory): u (batch, N_tilde, nu) the remembered plans' inputs, age (batch,) int32 the
        advancing steps since each was made (-1 nothing remembered, N_tilde exhausted).  u / age given: seed or restore them.  Returns dict(u, age)
        as now resident."""
        B, N, nu = self.batch, self.N_tilde, self.model.dims["nu"]
        if u is not None:
            u = np.asarray(u, dtype=np.float64)
            if u.shape != (B, N, nu):
                raise ValueError("u has shape %s, expected (%d, %d, %d)" % (u.shape, B, N, nu))
            u = np.ascontiguousarray(u)
        if age is not None:
            age = np.asarray(age)
            if age.shape != (B,) or not np.issubdtype(age.dtype, np.integer):
                raise ValueError("age has shape %s and dtype %s, expected (%d,) integers" % (age.shape, age.dtype, B))
            age = np.ascontiguousarray(age, dtype=np.int32)
        ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32)) if a is not None else None
        if u is not None or age is not None:
            check(_lib.load().mld_set_plan_memory(self._h, _lib.dptr(u), ip(age)))
        out = dict(u=np.zeros((B, N, nu)), age=np.zeros(B, np.int32))
        check(_lib.load().mld_download_plan_memory(self._h, _lib.dptr(out["u"]), ip(out["age"])))
        return out

    def _start_array(self, start, n_lead):
        """int64 starts with n_lead leading axes after the batch -- (batch, n_groups) or (batch, n_cols, n_groups); the same without the batch axis is
        broadcast over the batch; ValueError on a float dtype or a shape that fits neither, before any C call"""
        a = np.asarray(start)
        if not np.issubdtype(a.dtype, np.integer):
            raise ValueError("start has dtype %s, expected integers (offsets into the profile library)" % a.dtype)
        width = getattr(self, "_pf_width", None)
        G = len(width) if width else (a.shape[-1] if a.ndim else 0)
        want = "(%d, %s%d) or (%s%d)" % (self.batch, "n_cols, " * n_lead, G, "n_cols, " * n_lead, G)
        if a.ndim == 1 + n_lead:
            a = np.broadcast_to(a, (self.batch,) + a.shape)
        if a.ndim != 2 + n_lead or a.shape[0] != self.batch or a.shape[-1] != G or G < 1 or (n_lead and a.shape[1] < 1):
            raise ValueError("start has shape %s, expected %s" % (np.shape(start), want))
        return np.ascontiguousarray(a, dtype=np.int64)

    def _column_extras(self, n_cols, col_rows, x_cols):
        """col_rows (n_cols) int32 and x_cols (batch, n_cols, nx) of profile columns, checked as _column_arrays checks them"""
        nx, B = self.model.dims["nx"], self.batch
        if x_cols is not None:
            x_cols = np.asarray(x_cols, dtype=np.float64)
            if nx == 0:
                raise ValueError("x_cols has shape %s but the model has no state (nx = 0)" % (x_cols.shape,))
            if x_cols.shape != (B, n_cols, nx):
                raise ValueError("x_cols has shape %s, expected (%d, %d, %d)" % (x_cols.shape, B, n_cols, nx))
            x_cols = np.ascontiguousarray(x_cols)
        if col_rows is not None:
            cr = np.asarray(col_rows)
            if cr.shape != (n_cols,) or not np.issubdtype(cr.dtype, np.integer):
                raise ValueError("col_rows has shape %s and dtype %s, expected (%d,) integers" % (cr.shape, cr.dtype, n_cols))
            col_rows = np.ascontiguousarray(cr, dtype=np.int32)
        return col_rows, x_cols

    def forecast_from_profiles(self, start=None, step=0):
        """the forecast of every instance replaced by its window of the resident library (mld_forecast_from_profiles): start (batch, n_groups) or
        (n_groups,) integer offsets, window = profiles.windows(lib, start, step, N_tilde, group_width).  start=None re-uses the resident starts with
        another step.  After advance() only the forecast changes (plan and MIP start stay); otherwise the call counts as new inputs, like select()."""
        st = self._start_array(start, 0) if start is not None else None
        check(_lib.load().mld_forecast_from_profiles(self._h, st.ctypes.data_as(C.POINTER(C.c_int64)) if st is not None else None, int(step)))

    def constraint_blocks_from_profiles(self, start=None, step=0, col_rows=None, x_cols=None):
        """extra constraint blocks gathered from the resident library (mld_constraint_blocks_from_profiles): start (batch, n_cols, n_groups) or (n_cols,
        n_groups); col_rows / x_cols as upload_constraint_blocks.  start=None re-uses the resident column starts with another step.  Returns n_cols."""
        ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32)) if a is not None else None
        if start is not None:
            st = self._start_array(start, 1)
            n_cols = st.shape[1]
        else:
            st = None
            n_cols = getattr(self, "_pf_ccols", 0) or (len(col_rows) if col_rows is not None else 1)      # (without resident starts the library refuses)
        cr, xc = self._column_extras(n_cols, col_rows, x_cols)
        check(_lib.load().mld_constraint_blocks_from_profiles(self._h, n_cols, st.ctypes.data_as(C.POINTER(C.c_int64)) if st is not None else None, int(step),
                                                              ip(cr), _lib.dptr(xc)))
        self._pf_ccols = n_cols
        return n_cols

    def evaluate_profiles(self, start, step=0, v=None, col_rows=None, x_cols=None):
        """evaluate() under validation columns gathered from the resident library instead of uploaded (mld_evaluate_batch_profiles): start (batch, n_cols,
        n_groups) or (n_cols, n_groups); the dict of evaluate(omega_cols=...), constr_vio / constr_row (batch, n_cols).  The resident blocks and starts
        are neither used nor changed."""
        if start is None:
            raise ValueError("evaluate_profiles needs start (the resident column starts belong to the problem's blocks)")
        v = self._plan_array(v)
        st = self._start_array(start, 1)
        n_cols = st.shape[1]
        cr, xc = self._column_extras(n_cols, col_rows, x_cols)
        B = self.batch
        out = dict(obj=np.zeros(B), constr_vio=np.zeros((B, n_cols)), constr_row=np.zeros((B, n_cols), np.int32), int_vio=np.zeros(B), bound_vio=np.zeros(B))
        ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32)) if a is not None else None
        check(_lib.load().mld_evaluate_batch_profiles(self._h, _lib.dptr(v), n_cols, st.ctypes.data_as(C.POINTER(C.c_int64)), int(step), ip(cr), _lib.dptr(xc),
                                                      _lib.dptr(out["obj"]), _lib.dptr(out["constr_vio"]), ip(out["constr_row"]), _lib.dptr(out["int_vio"]),
                                                      _lib.dptr(out["bound_vio"])))
        return out

    def constraint_blocks(self):
        """the resident constraint blocks however they got there (mld_download_constraint_blocks): dict(omega_cols (batch, n_cols, N_tilde*nomega), col_rows
        (n_cols,) -- N_tilde*nc for blocks set without col_rows --, x_cols (batch, n_cols, nx) or None when every column uses the instance's x0)"""
        lib = _lib.load()
        n = C.c_int32(0)
        check(lib.mld_download_constraint_blocks(self._h, C.byref(n), None, None, None))
        n_cols, nx = int(n.value), self.model.dims["nx"]
        oc, cr = np.zeros((self.batch, n_cols, self.nW)), np.zeros(n_cols, np.int32)
        xc = None
        if n_cols:
            check(lib.mld_download_constraint_blocks(self._h, None, _lib.dptr(oc), cr.ctypes.data_as(C.POINTER(C.c_int32)), None))
            if nx:      # x_cols is refused (MLD_ERR_INVALID) exactly when the resident blocks have none
                xc = np.zeros((self.batch, n_cols, nx))
                rc = lib.mld_download_constraint_blocks(self._h, None, None, None, _lib.dptr(xc))
                if rc == -1:
                    xc = None
                else:
                    check(rc)
        return dict(omega_cols=oc, col_rows=cr, x_cols=xc)

    def _inst_cost_arrays(self, lin_v=None, lin_x=None, lin_y=None):
        """(batch, len) float64 arrays of a per-instance cost, a (len,) array broadcast; ValueError on a shape that fits neither"""
        d, N = self.model.dims, self.N_tilde
        out = []
        for name, a, ln in (("lin_v", lin_v, self.n), ("lin_x", lin_x, N * d["nx"]), ("lin_y", lin_y, N * d["ny"])):
            if a is None:
                out.append(None)
                continue
            a = np.asarray(a, dtype=np.float64)
            if a.ndim == 2 and a.shape[1] == 1 and a.shape[0] == ln and self.batch != ln:
                a = a[:, 0]                      # a column vector, as the reference writes its atoms
            if ln == 0:
                raise ValueError("%s given but the model has none of that variable" % name)
            if a.shape == (ln,):
                a = np.broadcast_to(a, (self.batch, ln))
            if a.shape != (self.batch, ln):
                raise ValueError("%s has shape %s, expected (%d, %d) or (%d,)" % (name, a.shape, self.batch, ln, ln))
            out.append(np.ascontiguousarray(a))
        return out

    def upload_instance_cost(self, lin_v=None, lin_x=None, lin_y=None):
        """per-instance LINEAR cost of the resident batch, added to the problem's cost (mld_upload_instance_cost): arrays (batch, len) with len =
        N_tilde * nv / nx / ny, a (len,) array is the same for every instance; everything None clears.  Valid until the next upload()."""
        lv, lx, ly = self._inst_cost_arrays(lin_v, lin_x, lin_y)
        check(_lib.load().mld_upload_instance_cost(self._h, _lib.dptr(lv), _lib.dptr(lx), _lib.dptr(ly)))

    def instance_cost(self):
        """read-back (mld_download_instance_cost): q (batch, n) the unscaled per-instance addition to the linear term pulled back to v, and const
        (batch) its constant term at the current x0 / omega"""
        q, c = np.zeros((self.batch, self.n)), np.zeros(self.batch)
        check(_lib.load().mld_download_instance_cost(self._h, _lib.dptr(q), _lib.dptr(c)))
        return dict(q=q, const=c)

    # -- resident price profiles -------------------------------------------------------------------------
    def upload_prices(self, lib, n_chan=1):
        """flat library of price series resident in HBM (mld_upload_prices), owned by the problem and independent of the batch, separate from the
        disturbance library.  A series is row-major (time, n_chan), as the reference's price_profile.values; profiles.pack lays series end to end.  A
        second call replaces the library, invalidates the resident price starts and disarms a stage cost; an empty library frees it."""
        lib = np.ascontiguousarray(lib, dtype=np.float64)
        if lib.ndim != 1:
            raise ValueError("lib has shape %s, expected a flat array (profiles.pack)" % (lib.shape,))
        if int(n_chan) < 1:
            raise ValueError("n_chan = %r, expected at least one price channel" % (n_chan,))
        check(_lib.load().mld_upload_prices(self._h, lib.size, _lib.dptr(lib) if lib.size else None, int(n_chan)))
        self._pr_chan = int(n_chan) if lib.size else 0
        self._pr_lib = lib if lib.size else None      # (rollout(kpis=...) prices the trajectories it finishes on the host from it)

    def _price_tables(self, **tables):
        """per-model tables (n_models, n_chan, width) of the price entry points; (n_chan, width) and (width,) broadcast over models and channels; None stays
        None.  ValueError on a shape that fits none, before any C call"""
        M, C = self.model.n_models, getattr(self, "_pr_chan", 0)
        if not C and any(t is not None for t in tables.values()):
            raise ValueError("no price library uploaded (upload_prices): its n_chan shapes the tables")
        widths = dict(a_v=self.model.nv, sum_v=self.model.nv, w_v=self.model.nv, a_y=self.model.dims["ny"], w_y=self.model.dims["ny"])
        out = []
        for name, t in tables.items():
            if t is None:
                out.append(None)
                continue
            W = widths[name]
            t = np.asarray(t, dtype=np.float64)
            if W == 0:
                raise ValueError("%s given but the model has none of that variable" % name)
            if t.shape not in ((M, C, W), (C, W), (W,)):
                raise ValueError("%s has shape %s, expected (%d, %d, %d), (%d, %d) or (%d,)" % (name, t.shape, M, C, W, C, W, W))
            out.append(np.ascontiguousarray(np.broadcast_to(t, (M, C, W))))
        return out

    def _price_start(self, start):
        """(batch,) int64 starts into the price library; a scalar or (1,) is broadcast over the batch; ValueError on a float dtype or another shape"""
        a = np.asarray(start)
        if not np.issubdtype(a.dtype, np.integer):
            raise ValueError("start has dtype %s, expected integers (offsets into the price library)" % a.dtype)
        if a.shape in ((), (1,)):
            a = np.broadcast_to(a.reshape(()), (self.batch,))
        if a.shape != (self.batch,):
            raise ValueError("start has shape %s, expected (%d,), (1,) or a scalar" % (np.shape(start), self.batch))
        return np.ascontiguousarray(a, dtype=np.int64)

    def set_price_cost(self, a_v=None, sum_v=None, a_y=None):
        """the tables that turn a price window into linear weights (mld_set_price_cost): a_v / sum_v (n_models, n_chan, nv), a_y (n_models, n_chan, ny);
        (n_chan, width) and (width,) broadcast; None = zeros, all None clears.  prices.cost_np states what they build."""
        av, sv, ay = self._price_tables(a_v=a_v, sum_v=sum_v, a_y=a_y)
        check(_lib.load().mld_set_price_cost(self._h, _lib.dptr(av), _lib.dptr(sv), _lib.dptr(ay)))

    def instance_cost_from_prices(self, start=None, step=0):
        """the per-instance linear cost of the resident batch built on the device from price windows (mld_instance_cost_from_prices): start (batch,)
        integer offsets into the price library (a scalar is broadcast), window = prices.windows(lib, start, step, N_tilde, n_chan).  start=None re-uses
        the resident starts with another step.  The result is the cost upload_instance_cost(*prices.cost_np(...)) leaves, bit for bit."""
        st = self._price_start(start) if start is not None else None
        check(_lib.load().mld_instance_cost_from_prices(self._h, st.ctypes.data_as(C.POINTER(C.c_int64)) if st is not None else None, int(step)))

    def set_stage_cost(self, w_v=None, w_y=None):
        """the weights of the stage cost (mld_set_stage_cost): w_v (n_models, n_chan, nv), w_y (n_models, n_chan, ny), broadcast as set_price_cost's;
        None = zeros, all None clears and disarms"""
        wv, wy = self._price_tables(w_v=w_v, w_y=w_y)
        check(_lib.load().mld_set_stage_cost(self._h, _lib.dptr(wv), _lib.dptr(wy)))

    def sim_log_cost_begin(self, start):
        """arms the stage cost for the log that has been begun (mld_sim_log_cost_begin): start (batch,) offsets of the realised prices; every logged step
        then records price[c] = lib[start + step * n_chan + c] and cost = prices.stage_cost_np(...) of its own v and y, and adds it to the instance's total"""
        if start is None:
            raise ValueError("sim_log_cost_begin needs start (the offsets of the realised prices, one per instance)")
        st = self._price_start(start)
        check(_lib.load().mld_sim_log_cost_begin(self._h, st.ctypes.data_as(C.POINTER(C.c_int64))))

    def sim_log_cost(self, first=0, count=None):
        """stage cost and price of records [first, first + count) (mld_download_sim_log_cost; count=None: all from first): dict(cost (count, batch),
        price (count, batch, n_chan)); cost is NaN for a skipped instance"""
        first = int(first)
        if count is None:
            count = self.sim_log_count()[0] - first
        K = int(count)
        if K < 0:
            raise ValueError("sim_log_cost: first = %d lies beyond the %d logged steps" % (first, K + first))
        out = dict(cost=np.zeros((K, self.batch)), price=np.zeros((K, self.batch, getattr(self, "_pr_chan", 0))))
        check(_lib.load().mld_download_sim_log_cost(self._h, first, K, _lib.dptr(out["cost"]), _lib.dptr(out["price"])))
        return out

    def cost_total(self):
        """the running stage cost per instance since the stage cost was armed (mld_download_cost_total): dict(total (batch,), steps (batch,) int32 the
        records that counted)"""
        out = dict(total=np.zeros(self.batch), steps=np.zeros(self.batch, np.int32))
        check(_lib.load().mld_download_cost_total(self._h, _lib.dptr(out["total"]), out["steps"].ctypes.data_as(C.POINTER(C.c_int32))))
        return out

    def _plan_array(self, v):
        """(batch, n) float64 array of caller-supplied plans, a (n,) array broadcast; ValueError on a shape that fits neither"""
        if v is None:
            return None
        v = np.asarray(v, dtype=np.float64)
        if v.shape == (self.n,):
            v = np.broadcast_to(v, (self.batch, self.n))
        if v.shape != (self.batch, self.n):
            raise ValueError("v has shape %s, expected (%d, %d) or (%d,)" % (v.shape, self.batch, self.n, self.n))
        return np.ascontiguousarray(v)

    def trajectories(self, v=None):
        """predicted trajectories of the resident batch on device (mld_predict_batch): dict(x=(batch, N_tilde*nx), y=(batch, N_tilde*ny)), step-major
        rows; a family the model lacks has width 0.  v=None: the last solve's plans (needs a finished solve of the current inputs; instances without
        a usable plan -- the ones advance() skips -- get NaN rows); v (batch, n) or (n,): these plans under the current x0 / omega, valid without a solve."""
        v = self._plan_array(v)
        d, N = self.model.dims, self.N_tilde
        x, y = np.zeros((self.batch, N * d["nx"])), np.zeros((self.batch, N * d["ny"]))
        check(_lib.load().mld_predict_batch(self._h, _lib.dptr(v), _lib.dptr(x) if x.shape[1] else None, _lib.dptr(y) if y.shape[1] else None))
        return dict(x=x, y=y)

    def _column_arrays(self, omega_cols=None, col_rows=None, x_cols=None):
        """validation columns in the layout of upload_constraint_blocks: (n_cols, omega_cols (batch, n_cols, N_tilde*nomega) or None, col_rows (n_cols) int32
        or None, x_cols (batch, n_cols, nx) or None); ValueError on a shape that does not fit, before any C call"""
        nx, nW, B = self.model.dims["nx"], self.nW, self.batch
        if omega_cols is None and x_cols is None:
            if col_rows is not None:
                raise ValueError("col_rows given without columns (omega_cols / x_cols)")
            return 0, None, None, None
        n_cols = None
        if omega_cols is not None:
            omega_cols = np.asarray(omega_cols, dtype=np.float64)
            if omega_cols.ndim != 3 or omega_cols.shape[0] != B or omega_cols.shape[2] != nW or omega_cols.shape[1] < 1:
                raise ValueError("omega_cols has shape %s, expected (%d, n_cols, %d)" % (omega_cols.shape, B, nW))
            n_cols = omega_cols.shape[1]
        elif nW:
            raise ValueError("x_cols given without omega_cols, but the model has a disturbance (expected omega_cols of shape (%d, n_cols, %d))" % (B, nW))
        if x_cols is not None:
            x_cols = np.asarray(x_cols, dtype=np.float64)
            if nx == 0:
                raise ValueError("x_cols has shape %s but the model has no state (nx = 0)" % (x_cols.shape,))
            if x_cols.ndim != 3 or x_cols.shape[0] != B or x_cols.shape[2] != nx or x_cols.shape[1] != (n_cols or x_cols.shape[1]) or x_cols.shape[1] < 1:
                raise ValueError("x_cols has shape %s, expected (%d, %s, %d)" % (x_cols.shape, B, n_cols if n_cols else "n_cols", nx))
            n_cols = x_cols.shape[1]
            x_cols = np.ascontiguousarray(x_cols)
        if col_rows is not None:
            cr = np.asarray(col_rows)
            if cr.shape != (n_cols,) or not np.issubdtype(cr.dtype, np.integer):
                raise ValueError("col_rows has shape %s and dtype %s, expected (%d,) integers" % (cr.shape, cr.dtype, n_cols))
            col_rows = np.ascontiguousarray(cr, dtype=np.int32)
        if omega_cols is not None:
            omega_cols = np.ascontiguousarray(omega_cols) if nW else None
        return n_cols, omega_cols, col_rows, x_cols

    def evaluate(self, v=None, omega_cols=None, col_rows=None, x_cols=None):
        """solution quality of the resident batch on device (mld_evaluate_batch), fp64 on the ORIGINAL rows: dict(obj, constr_vio, constr_row, int_vio,
        bound_vio).  v=None: the last solve's plans (needs a finished solve of the current inputs; instances without a usable plan get NaN / -1);
        v (batch, n) or (n,): these plans under the current x0 / omega.  Without columns the problem as posed (standard block and resident constraint
        blocks): constr_vio / constr_row (batch,) the largest residual H_v v - h and a row that attains it.  With omega_cols (batch, n_cols,
        N_tilde*nomega), col_rows (n_cols), x_cols (batch, n_cols, nx) -- the layout of upload_constraint_blocks -- the same per validation column,
        (batch, n_cols); the resident blocks are neither used nor changed."""
        v = self._plan_array(v)
        n_cols, oc, cr, xc = self._column_arrays(omega_cols, col_rows, x_cols)
        B = self.batch
        shp = (B, n_cols) if n_cols else (B,)
        out = dict(obj=np.zeros(B), constr_vio=np.zeros(shp), constr_row=np.zeros(shp, np.int32), int_vio=np.zeros(B), bound_vio=np.zeros(B))
        ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32)) if a is not None else None
        check(_lib.load().mld_evaluate_batch(self._h, _lib.dptr(v), int(n_cols), _lib.dptr(oc), ip(cr), _lib.dptr(xc), _lib.dptr(out["obj"]),
                                             _lib.dptr(out["constr_vio"]), ip(out["constr_row"]), _lib.dptr(out["int_vio"]), _lib.dptr(out["bound_vio"])))
        return out

    def set_opts(self, **opts):
        """limits / tolerances of the existing problem (mld_problem_set_opts): MIPGap, NodeLimit, IterationLimit, gap_abs, cut
        rounds, reserved -- no rebuild, like the per-call solver kwargs of the reference's solve()"""
        alias = dict(MIPGap="gap_rel", NodeLimit="max_nodes", IterationLimit="max_pivots", TimeLimit="time_limit")
        new = _lib.Opts.from_buffer_copy(self.opts)      # a refused call leaves the Python copy as it was, like the device options
        for k, v in opts.items():
            k = alias.get(k, k)
            if k in ("max_cuts", "n_slots", "presolve") or not hasattr(new, k):
                raise TypeError("option %r cannot be changed on an existing problem" % k)
            if k == "flags" and int(v) != int(self.opts.flags):
                raise TypeError("flags (MLD_F32, MLD_SMALL_LDS) are fixed when the problem is created")
            setattr(new, k, type(getattr(new, k))(v))
        check(_lib.load().mld_problem_set_opts(self._h, C.byref(new)))
        self.opts = new

    def advance(self):
        """receding horizon on device (mld_advance_batch2): x0 <- plant update with the step-0 slice of the last solution,
        disturbance forecast moved on by one step; the next solve_resident() is the next MPC step.  Returns the number of
        instances that were NOT advanced because their solve left no usable plan (they keep state and forecast)."""
        skipped = C.c_int32(0)
        check(_lib.load().mld_advance_batch2(self._h, C.byref(skipped)))
        return int(skipped.value)

    # -- plant step and simulation log ------------------------------------------------------------------
    def sim_log_begin(self, capacity):
        """a resident log of `capacity` steps of the resident batch (mld_sim_log_begin): resets the count, 0 frees; upload() discards the log"""
        check(_lib.load().mld_sim_log_begin(self._h, int(capacity)))

    def sim_log_count(self):
        """(steps logged, capacity) of the resident log; (0, 0) without one"""
        n, cap = C.c_int32(0), C.c_int32(0)
        check(_lib.load().mld_sim_log_count(self._h, C.byref(n), C.byref(cap)))
        return int(n.value), int(cap.value)

    def sim_step(self, v0=None, act_start=None, step=0, actual=None, advance=True, log=None, outputs=False, resolve=None, u0=None, policy=False, fallback=None, selected=False):
        """one plant step of the resident batch on device (mld_sim_step_batch): the reference's lsim_k(x_k, v_k=, omega_k) with the whole step-0 slice --
        of the last solve's plans (v0=None; instances without a usable plan are skipped and counted) or the caller's v0 (batch, nv) / (nv,) -- under the
        forecast's step 0 or, with actual, the element `step` of the realised series at act_start (batch, n_groups) / (n_groups,) of the resident profile
        library (None re-uses the resident actual starts).  actual defaults to `act_start is not None`, log to "a log has begun".  advance: x0 <- x_k1
        and the forecast rotated, as advance(); False is a what-if that changes nothing.  Returns the number of skipped instances, or with outputs=True
        dict(x_k1, y, cons (bool), cons_vio, cons_row, n_skipped).
        resolve: an aux_resolve.BatchAuxResolver over the same models -- the step of the reference's lsim_k(x_k, u_k=, omega_k) instead
        (mld_sim_step_resolve): only u is taken -- the plan's (u0=None) or the caller's u0 (batch, nu) / (nu,) -- and delta, z, mu are re-derived on the device
        under the omega_k used; v0 must be None.  An instance whose auxiliary problem has no feasible point is skipped like one without a plan.
        outputs=True additionally returns v0 (batch, nv), the resolved slices, and aux_status (batch), the resolver's status, -1 = not attempted.
        policy=True (with resolve): the ruled channels of u come from the resident policy (upload_policy), written on the device from the current x0 and
        the resident u_prev (mld_sim_step_policy, kernel k_policy_inputs); u0 / the plan supply the passed-through channels only, and no plan is needed
        when every channel is ruled.  An advancing step moves the resident u_prev of every advanced instance to the u applied.
        fallback (with resolve, without u0 / policy): any subset of ("memory", "policy") -- the plan's step (mld_sim_step_fallback, kernels
        k_fallback_inputs / k_fallback_commit) in which an instance WITHOUT a usable plan takes its u from the first source that applies: the plan memory's
        row for the current time (plan_memory()), then the resident policy's rule (upload_policy, every channel ruled); with neither it is skipped as
        before.  fallback=() allows no source: the step of sim_step(resolve=R).  outputs=True additionally returns u_source (batch) int32: 0 plan,
        1 memory, 2 policy, -1 none.  An advancing step remembers the usable plans in an enabled memory, ages the others, and moves a resident policy's
        u_prev of every advanced instance to the u applied.
        selected=True (with resolve, without u0 / policy): the kept selection as the FIRST source, in place of the plan (mld_sim_step_selected, kernels
        k_selected_inputs / k_selected_commit) -- what select_plan(..., keep=True) / select_plan_policies(..., keep=True) chose, or set_selection().  An
        instance with a choice takes its u[b, 0]; one without (choice -1) goes to the sources `fallback` names (none without the argument), never to the
        plan.  u_source: 3 selected, 1 memory, 2 policy, -1 none; outputs=True additionally returns pick (batch) int32, the candidate applied or -1.  An
        advancing step remembers a chosen plan or sequence of K == N_tilde steps in an enabled memory (age 1) and ages the others, keeps the memory valid,
        moves a resident policy's u_prev to the u applied, and consumes the selection; the log says 3 in sim_log_source() and the candidate in
        sim_log_pick().  No plan is needed; the handle ends as after sim_step(resolve=R, u0=...)."""
        d, B = self.model.dims, self.batch
        nv = self.model.nv
        if selected:
            if resolve is None or u0 is not None or policy or v0 is not None:
                raise ValueError("selected=True goes with resolve alone (no v0, no u0, no policy=True): the kept selection supplies u")
            if fallback is None:
                fallback = ()
        if policy and resolve is None:
            raise ValueError("policy=True goes with resolve (a BatchAuxResolver re-derives the auxiliaries of the rule's u)")
        fb = None
        if fallback is not None:
            if resolve is None or u0 is not None or policy:
                raise ValueError("fallback goes with resolve and the resident plan's u (no u0, no policy=True): it names where an instance without a usable plan takes its u from")
            fb = _fallback.fb_bits(fallback)
        if resolve is None and u0 is not None:
            raise ValueError("u0 given without resolve (the whole slice is v0; u0 goes with a BatchAuxResolver that re-derives the rest)")
        if resolve is not None:
            if v0 is not None:
                raise ValueError("resolve and v0 both given: the resolver re-derives the auxiliaries of u0 (or of the plan's u), a whole slice leaves it nothing")
            if u0 is not None:
                u0 = np.asarray(u0, dtype=np.float64)
                if u0.shape == (d["nu"],):
                    u0 = np.broadcast_to(u0, (B, d["nu"]))
                if u0.shape != (B, d["nu"]):
                    raise ValueError("u0 has shape %s, expected (%d, %d) or (%d,)" % (u0.shape, B, d["nu"], d["nu"]))
                u0 = np.ascontiguousarray(u0)
        if v0 is not None:
            v0 = np.asarray(v0, dtype=np.float64)
            if v0.shape == (nv,):
                v0 = np.broadcast_to(v0, (B, nv))
            if v0.shape != (B, nv):
                raise ValueError("v0 has shape %s, expected (%d, %d) or (%d,)" % (v0.shape, B, nv, nv))
            v0 = np.ascontiguousarray(v0)
        st = self._start_array(act_start, 0) if act_start is not None else None
        if actual is None:
            actual = act_start is not None
        if log is None:
            log = self.sim_log_count()[1] > 0
        flags = (_lib.MLD_SIM_ADVANCE if advance else 0) | (_lib.MLD_SIM_ACTUAL if actual else 0) | (_lib.MLD_SIM_LOG if log else 0)
        skipped = C.c_int32(0)
        ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32)) if a is not None else None
        out = None
        if outputs:
            out = dict(x_k1=np.zeros((B, d["nx"])), y=np.zeros((B, d["ny"])), cons=np.zeros((B, d["nc"]), np.uint8), cons_vio=np.zeros(B),
                       cons_row=np.zeros(B, np.int32))
        if resolve is not None:
            if outputs:
                out.update(v0=np.zeros((B, nv)), aux_status=np.zeros(B, np.int32))
            aux = resolve.problem._h if resolve.problem is not None else None
            if fb is not None:
                if outputs:
                    out["u_source"] = np.zeros(B, np.int32)
                    if selected:
                        out["pick"] = np.zeros(B, np.int32)
                check((_lib.load().mld_sim_step_selected if selected else _lib.load().mld_sim_step_fallback)(
                    self._h, aux, fb, st.ctypes.data_as(C.POINTER(C.c_int64)) if st is not None else None, int(step), flags,
                    _lib.dptr(out["x_k1"]) if out else None, _lib.dptr(out["y"]) if out else None,
                    out["cons"].ctypes.data_as(C.POINTER(C.c_uint8)) if out else None, _lib.dptr(out["cons_vio"]) if out else None,
                    ip(out["cons_row"]) if out else None, _lib.dptr(out["v0"]) if out else None, ip(out["aux_status"]) if out else None,
                    ip(out["u_source"]) if out else None, C.byref(skipped), *([ip(out["pick"]) if out else None] if selected else [])))
            else:
                check((_lib.load().mld_sim_step_policy if policy else _lib.load().mld_sim_step_resolve)(
                    self._h, aux, _lib.dptr(u0), st.ctypes.data_as(C.POINTER(C.c_int64)) if st is not None else None, int(step), flags,
                    _lib.dptr(out["x_k1"]) if out else None, _lib.dptr(out["y"]) if out else None,
                    out["cons"].ctypes.data_as(C.POINTER(C.c_uint8)) if out else None, _lib.dptr(out["cons_vio"]) if out else None,
                    ip(out["cons_row"]) if out else None, _lib.dptr(out["v0"]) if out else None, ip(out["aux_status"]) if out else None, C.byref(skipped)))
            if resolve.problem is not None:
                resolve.problem.batch = B      # the call lays the resolver's batch out as this one
            if not outputs:
                return int(skipped.value)
            out["cons"] = out["cons"].astype(bool)
            out["n_skipped"] = int(skipped.value)
            return out
        check(_lib.load().mld_sim_step_batch(
            self._h, _lib.dptr(v0), st.ctypes.data_as(C.POINTER(C.c_int64)) if st is not None else None, int(step), flags,
            _lib.dptr(out["x_k1"]) if out else None, _lib.dptr(out["y"]) if out else None,
            out["cons"].ctypes.data_as(C.POINTER(C.c_uint8)) if out else None, _lib.dptr(out["cons_vio"]) if out else None,
            ip(out["cons_row"]) if out else None, C.byref(skipped)))
        if not outputs:
            return int(skipped.value)
        out["cons"] = out["cons"].astype(bool)
        out["n_skipped"] = int(skipped.value)
        return out

    def set_rollout_completion(self, mode):
        """the sticky completion mode of this handle (mld_set_rollout_completion): 0 as ever, _lib.MLD_ROLLOUT_COMPLETE_DEVICE finishes the trajectories the
        LDS solver declines on the device in every later call of the rollout family -- what complete="device" sets for one call --,
        _lib.MLD_ROLLOUT_COMPLETE_DBG_FIRST_ONLY (tests) lets MLD_DBG_SMALL_PIVOT_CAP cap the rollout kernel and the first re-run only."""
        check(_lib.load().mld_set_rollout_completion(self._h, int(mode)))
        self._ro_mode = int(mode)

    def rollout_completion_stats(self):
        """what the last call of the rollout family did on the device (mld_rollout_completion_stats): dict(rounds, finished_on_device, dense_solves, left_declined)"""
        out = np.zeros(4, np.int64)
        check(_lib.load().mld_rollout_completion_stats(self._h, out.ctypes.data_as(C.POINTER(C.c_int64))))
        return dict(rounds=int(out[0]), finished_on_device=int(out[1]), dense_solves=int(out[2]), left_declined=int(out[3]))

    def _device_stats(self, stats):
        """stats of an entry after a call with complete="device": [1] and [2] count the final endings, [3] what the rollout kernel declined"""
        cs = self.rollout_completion_stats()
        return dict(trajectories=int(stats[0]), complete=int(stats[1]), infeasible=int(stats[2]), declined=int(stats[3]),
                    not_attempted=int(stats[0] - stats[1] - stats[2]) - cs["left_declined"], finished_on_host=0,
                    finished_on_device=cs["finished_on_device"], completion_rounds=cs["rounds"])

    def _u_seq_array(self, u_seq, K):
        """u_seq of rollout() / warm_start_from_rollout(): (batch, K, nu), or (K, nu) for every instance; K=None takes the array's"""
        B, nu = self.batch, self.model.dims["nu"]
        u_seq = np.asarray(u_seq, dtype=np.float64)
        if u_seq.ndim == 2:
            u_seq = np.broadcast_to(u_seq, (B,) + u_seq.shape)
        if u_seq.ndim != 3 or u_seq.shape[0] != B or u_seq.shape[2] != nu or (K is not None and u_seq.shape[1] != int(K)):
            raise ValueError("u_seq has shape %s, expected (%d, K, %d) or (K, %d)%s" % (u_seq.shape, B, nu, nu, "" if K is None else " with K = %d" % int(K)))
        return np.ascontiguousarray(u_seq)

    def _u_prev_array(self, u_prev, policy):
        """u_prev of the same two: (batch, nu), or (nu,) for every instance; only with a policy"""
        B, nu = self.batch, self.model.dims["nu"]
        if u_prev is None:
            return None
        if not policy:
            raise ValueError("u_prev given without policy=True (the open-loop rollout has no previous input)")
        u_prev = np.asarray(u_prev, dtype=np.float64)
        if u_prev.shape == (nu,):
            u_prev = np.broadcast_to(u_prev, (B, nu))
        if u_prev.shape != (B, nu):
            raise ValueError("u_prev has shape %s, expected (%d, %d) or (%d,)" % (u_prev.shape, B, nu, nu))
        return np.ascontiguousarray(u_prev)

    def _rollout_inputs(self, K, omega_seq, start, cost_w, kpis, price_start):
        """what rollout() and select_plan() share: the disturbance -- exactly one of omega_seq (batch, S, K, nomega) and start --, cost_w and the KPI table with its
        price starts, tested and made contiguous.  Returns (omega_seq, start array or None, S, cost_w, cost rows, KPI arrays, KPI tables, thresholds, price starts);
        the last four are None without a table."""
        from . import simlog
        d, B, nv = self.model.dims, self.batch, self.model.nv
        nx, nw, ny = d["nx"], d["nomega"], d["ny"]
        if (omega_seq is None) == (start is None) and nw:
            raise ValueError("exactly one of omega_seq and start must be given (%s)" % ("both are" if start is not None else "neither is"))
        st = None
        if omega_seq is not None:
            omega_seq = np.asarray(omega_seq, dtype=np.float64)
            if omega_seq.ndim != 4 or omega_seq.shape[0] != B or omega_seq.shape[1] < 1 or omega_seq.shape[2:] != (K, nw):
                raise ValueError("omega_seq has shape %s, expected (%d, S, %d, %d)" % (omega_seq.shape, B, K, nw))
            omega_seq = np.ascontiguousarray(omega_seq)
            S = omega_seq.shape[1]
        elif start is not None:
            st = self._start_array(start, 1)
            S = st.shape[1]
        else:
            S = 1
        rows = 0
        if cost_w is not None:
            cost_w = np.asarray(cost_w, dtype=np.float64)
            if cost_w.ndim == 2:
                cost_w = np.broadcast_to(cost_w, (self.model.n_models,) + cost_w.shape)
            if cost_w.ndim != 3 or cost_w.shape[0] not in (self.model.n_models, B) or cost_w.shape[1:] != (K, nv):
                raise ValueError("cost_w has shape %s, expected (%d, %d, %d), (%d, %d, %d) or (%d, %d)" % (cost_w.shape, self.model.n_models, K, nv, B, K, nv, K, nv))
            cost_w = np.ascontiguousarray(cost_w)
            rows = cost_w.shape[0]
        karr = ktabs = kthr = pst = None
        if kpis is None:
            if price_start is not None:
                raise ValueError("price_start given without kpis (it prices the KPIs of the rollout)")
        else:
            if kpis.n_models != self.model.n_models:
                raise ValueError("the KPI table has %d models, the problem %d" % (kpis.n_models, self.model.n_models))
            want = dict(w_x=nx, w_v=nv, w_y=ny, w_omega=nw, w_xk1=nx)
            if kpis.widths != want:
                raise ValueError("the KPI table was built for other dimensions (%s, this problem %s)" % (kpis.widths, want))
            karr = kpis.arrays()
            ktabs = [None if karr[k] is None else np.ascontiguousarray(karr[k]) for k in simlog.KPI_TABLES]
            kthr = None if karr["thresh"] is None else np.ascontiguousarray(karr["thresh"])
            if price_start is not None:
                pst = self._price_start(price_start)
            elif np.any(karr["price_chan"] >= 0):
                raise ValueError("KPI %r is priced, but price_start is None (the starts of the realised prices, one per instance)"
                                 % (kpis.names[int(np.flatnonzero(karr["price_chan"] >= 0)[0])],))
        return omega_seq, st, S, cost_w, rows, karr, ktabs, kthr, pst

    @_completes(True)
    def rollout(self, resolve, K=None, u_seq=None, omega_seq=None, start=None, step=0, cost_w=None, trajectories=False, policy=False, u_prev=None,
                kpis=None, price_start=None, vio_tol=1e-6, risk=None, per_trajectory=True):
        """open-loop rollout of the resident batch under S realised disturbances, on device (mld_rollout_batch, kernel k_rollout): the reference's
        MldModel.lsim / lsim_k in a loop with _compute_aux at every step (models/mld_model.py:543-642, 647-699, 701-766), batch x S trajectories in one launch.
        resolve: an aux_resolve.BatchAuxResolver(..., small_lds=True) over the same models.  u_seq (batch, K, nu) / (K, nu), or None = the inputs of the
        resident plan (K <= N_tilde).  Exactly one of omega_seq (batch, S, K, nomega) and start (batch, S, n_groups) / (S, n_groups) offsets into the
        resident profile library (windows of K steps from `step`).  cost_w (n_models, K, nv), (batch, K, nv) or (K, nv): weights of cost = sum_k w_k . v_k.
        K=None: N_tilde with the plan's u, u_seq.shape[-2] otherwise.  The handle is not changed (the what-if of sim_step(advance=False)).
        Returns dict(cost, mu_total, worst_vio, worst_step, steps_done, end_status: (batch, S); stats: dict(trajectories, complete, infeasible, declined,
        not_attempted, finished_on_host)); trajectories=True adds x (batch, S, K + 1, nx), v (batch, S, K, nv), y, cons_vio, cons_row (batch, S, K).
        end_status 0 complete, 1 the auxiliary problem of step steps_done is infeasible (NaN / -1 from there on, summaries NaN), -1 not attempted (no usable
        plan).  Trajectories the device's LDS solver declined (2) are finished on the host -- resolve.resolve per remaining step, whose own solve falls back
        to the dense kernel, then simlog.lsim_k_batch -- and end 0 or 1; they are counted in stats["finished_on_host"].
        policy=True: the closed loop of the resident rule-based policy instead (upload_policy; mld_rollout_policy, kernel k_rollout_policy) -- at every step
        the ruled channels of u_k come from the trajectory's own x_k and u_{k-1}, u_seq / the plan supply the passed-through channels only (no plan is
        needed when every channel is ruled); u_prev (batch, nu) / (nu,) is the input before step 0, None = the resident policy state, which the call
        leaves as it is.  The result carries switches (batch, S): the (step, ruled channel) pairs whose input changed, -1 unless the trajectory ended 0.
        The host completion applies the rule too.
        kpis: a simlog.KpiTable over this problem's models -- the campaign's column statistics of every trajectory, reduced inside the same kernel
        (mld_rollout_kpi, kernels k_rollout_kpi / k_rollout_policy_kpi).  The record of step k is x_k, v_k, y_k, omega_k, x_{k+1}; a priced KPI multiplies
        by lib[price_start[b] + (step + k) n_chan + ch] of the resident price library (upload_prices), price_start (batch,) or a scalar: one tariff for the
        S realisations of an instance, the price sim_step(step=step + k) records.  The result gains kpi = dict(names, sum, min, max (batch, S, n_kpi),
        min_step, max_step, n_above, n_changes (batch, S, n_kpi) int32, n_vio (batch, S) int32: steps with cons_vio > vio_tol); a trajectory that does not
        end 0 has NaN / -1.  The figures are those of the logged stepwise campaign's sim_log_summary and of simlog.rollout_kpis_np, bit for bit;
        trajectories finished on the host get theirs from rollout_kpis_np.  Without kpis the call is what it was.
        risk: a simlog.RiskTable -- the statistics ACROSS the S realisations of every instance, reduced on the device behind the rollout (mld_rollout_risk,
        kernel k_rollout_risk): per column (cost, mu_total, worst_vio, switches, n_vio or a KPI's statistic; a table that names KPIs is built over `kpis`)
        over the realisations that ended 0, sorted by (value, c).  The result gains risk = dict(names, levels, mean, min, max (batch, G), min_c, max_c,
        n_exceed (batch, G) int32, quantile, cvar_hi, cvar_lo (batch, G, L), quantile_c (batch, G, L) int32, n_complete, n_infeasible, n_declined,
        n_not_attempted (batch,) int32); an instance without a complete realisation has NaN / +inf / -inf / -1 / 0.  S <= 64.  The figures are those of
        simlog.rollout_risk_np on the same result, bit for bit; the instances with a trajectory finished on the host take theirs from rollout_risk_np of
        the finished arrays.  per_trajectory=False (with risk only) asks for nothing per trajectory: every (batch, S, ...) entry, kpi included, is neither
        downloaded nor returned.  With risk=None the call and its result are what they were.
        complete: None or "host" -- the host completion above; "device" -- the declined trajectories are finished on the device instead (mld.h: device
        completion; re-run from step 0, the declined steps by the dense kernel on the resolver's handle), before the KPIs' and the risk's consumers read
        them: nothing more is downloaded, per_trajectory=False downloads nothing per trajectory whatever declined, stats gains finished_on_device and
        completion_rounds, finished_on_host is 0 and declined counts what the rollout kernel declined."""
        from . import simlog
        d, B, nv = self.model.dims, self.batch, self.model.nv
        nx, nu, nw, ny = d["nx"], d["nu"], d["nomega"], d["ny"]
        if u_seq is not None:
            u_seq = self._u_seq_array(u_seq, K)
            K = u_seq.shape[1]
        K = self.N_tilde if K is None else int(K)
        u_prev = self._u_prev_array(u_prev, policy)
        omega_seq, st, S, cost_w, rows, karr, ktabs, kthr, pst = self._rollout_inputs(K, omega_seq, start, cost_w, kpis, price_start)
        aux = resolve.problem._h if resolve is not None and resolve.problem is not None else None
        ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32)) if a is not None else None
        lp = lambda a: a.ctypes.data_as(C.POINTER(C.c_int64)) if a is not None else None

        rarr = None
        if risk is None:
            if not per_trajectory:
                raise ValueError("per_trajectory=False without risk (nothing would be returned)")
        else:
            if trajectories and not per_trajectory:
                raise ValueError("trajectories=True with per_trajectory=False")
            if S > simlog.RISK_S_MAX:
                raise ValueError("risk: S = %d realisations (at most %d)" % (S, simlog.RISK_S_MAX))
            rarr = risk.arrays()
            if np.any(rarr["col_src"] == 3) and not policy:
                raise ValueError("risk column %r reads switches, but the rollout has no policy (policy=True)" % (risk.names[int(np.flatnonzero(rarr["col_src"] == 3)[0])],))
            if np.any(rarr["col_src"] >= 4):
                if kpis is None:
                    raise ValueError("risk column %r reads the KPIs, but kpis is None" % (risk.names[int(np.flatnonzero(rarr["col_src"] >= 4)[0])],))
                if risk.kpis is not kpis and list(risk.kpis.names) != list(kpis.names):
                    raise ValueError("the risk table was built over another KPI table (%s, this call's %s)" % (risk.kpis.names, kpis.names))

        def call_risk(full, per):
            """mld_rollout_risk: the per-trajectory arrays only with per, the trajectories only with full"""
            G, L = len(risk), len(risk.levels)
            o = {}
            if per:
                o.update(cost=np.zeros((B, S)), mu_total=np.zeros((B, S)), worst_vio=np.zeros((B, S)), worst_step=np.zeros((B, S), np.int32),
                         steps_done=np.zeros((B, S), np.int32), end_status=np.zeros((B, S), np.int32))
                if policy:
                    o["switches"] = np.zeros((B, S), np.int32)
            if full:
                o.update(x=np.zeros((B, S, K + 1, nx)), v=np.zeros((B, S, K, nv)), y=np.zeros((B, S, K, ny)), cons_vio=np.zeros((B, S, K)),
                         cons_row=np.zeros((B, S, K), np.int32))
            stats = np.zeros(4, np.int64)
            Q, kp, tabs, chan = 0, {}, [None] * 5, None
            if kpis is not None:
                Q, tabs, chan = len(kpis), ktabs, karr["price_chan"]
                if per:
                    kp = dict(names=list(kpis.names), sum=np.zeros((B, S, Q)), min=np.zeros((B, S, Q)), max=np.zeros((B, S, Q)), min_step=np.zeros((B, S, Q), np.int32),
                              max_step=np.zeros((B, S, Q), np.int32), n_above=np.zeros((B, S, Q), np.int32), n_changes=np.zeros((B, S, Q), np.int32),
                              n_vio=np.zeros((B, S), np.int32))
            rk = dict(names=list(risk.names), levels=list(risk.levels), mean=np.zeros((B, G)), min=np.zeros((B, G)), min_c=np.zeros((B, G), np.int32),
                      max=np.zeros((B, G)), max_c=np.zeros((B, G), np.int32), n_exceed=np.zeros((B, G), np.int32), quantile=np.zeros((B, G, L)),
                      quantile_c=np.zeros((B, G, L), np.int32), cvar_hi=np.zeros((B, G, L)), cvar_lo=np.zeros((B, G, L)))
            counts = np.zeros((B, 4), np.int32)
            check(_lib.load().mld_rollout_risk(
                self._h, aux, 1 if policy else 0, K, S, _lib.dptr(u_seq), _lib.dptr(u_prev), _lib.dptr(omega_seq) if nw else None, lp(st), int(step),
                _lib.dptr(cost_w), rows, Q, *([_lib.dptr(t) for t in tabs] + [ip(chan), _lib.dptr(kthr), float(vio_tol), lp(pst)]),
                _lib.dptr(o.get("x")), _lib.dptr(o.get("v")), _lib.dptr(o.get("y")), _lib.dptr(o.get("cons_vio")), ip(o.get("cons_row")),
                _lib.dptr(o.get("cost")), _lib.dptr(o.get("mu_total")), _lib.dptr(o.get("worst_vio")), ip(o.get("worst_step")), ip(o.get("steps_done")),
                ip(o.get("end_status")), ip(o.get("switches")), lp(stats), _lib.dptr(kp.get("sum")), _lib.dptr(kp.get("min")), _lib.dptr(kp.get("max")),
                ip(kp.get("min_step")), ip(kp.get("max_step")), ip(kp.get("n_above")), ip(kp.get("n_changes")), ip(kp.get("n_vio")),
                G, ip(rarr["col_src"]), ip(rarr["col_q"]), _lib.dptr(rarr["level"]), L, _lib.dptr(rarr["alpha"]),
                _lib.dptr(rk["mean"]), _lib.dptr(rk["min"]), _lib.dptr(rk["max"]), ip(rk["min_c"]), ip(rk["max_c"]), ip(rk["n_exceed"]),
                _lib.dptr(rk["quantile"]), ip(rk["quantile_c"]), _lib.dptr(rk["cvar_hi"]), _lib.dptr(rk["cvar_lo"]), ip(counts)))
            for i, key in enumerate(simlog.RISK_COUNTS):
                rk[key] = np.ascontiguousarray(counts[:, i])
            if kp:
                o["kpi"] = kp
            o["risk"] = rk
            return o, stats

        def call(full, per=True):
            if risk is not None:
                return call_risk(full, per)
            o = dict(cost=np.zeros((B, S)), mu_total=np.zeros((B, S)), worst_vio=np.zeros((B, S)), worst_step=np.zeros((B, S), np.int32),
                     steps_done=np.zeros((B, S), np.int32), end_status=np.zeros((B, S), np.int32))
            if full:
                o.update(x=np.zeros((B, S, K + 1, nx)), v=np.zeros((B, S, K, nv)), y=np.zeros((B, S, K, ny)), cons_vio=np.zeros((B, S, K)),
                         cons_row=np.zeros((B, S, K), np.int32))
            stats = np.zeros(4, np.int64)
            if kpis is not None:
                Q = len(kpis)
                kp = dict(names=list(kpis.names), sum=np.zeros((B, S, Q)), min=np.zeros((B, S, Q)), max=np.zeros((B, S, Q)), min_step=np.zeros((B, S, Q), np.int32),
                          max_step=np.zeros((B, S, Q), np.int32), n_above=np.zeros((B, S, Q), np.int32), n_changes=np.zeros((B, S, Q), np.int32),
                          n_vio=np.zeros((B, S), np.int32))
                if policy:
                    o["switches"] = np.zeros((B, S), np.int32)
                check(_lib.load().mld_rollout_kpi(
                    self._h, aux, 1 if policy else 0, K, S, _lib.dptr(u_seq), _lib.dptr(u_prev), _lib.dptr(omega_seq) if nw else None, lp(st), int(step),
                    _lib.dptr(cost_w), rows, Q, *([_lib.dptr(t) for t in ktabs] + [ip(karr["price_chan"]), _lib.dptr(kthr), float(vio_tol), lp(pst)]),
                    _lib.dptr(o.get("x")), _lib.dptr(o.get("v")), _lib.dptr(o.get("y")), _lib.dptr(o.get("cons_vio")), ip(o.get("cons_row")),
                    _lib.dptr(o["cost"]), _lib.dptr(o["mu_total"]), _lib.dptr(o["worst_vio"]), ip(o["worst_step"]), ip(o["steps_done"]), ip(o["end_status"]),
                    ip(o.get("switches")), lp(stats), _lib.dptr(kp["sum"]), _lib.dptr(kp["min"]), _lib.dptr(kp["max"]), ip(kp["min_step"]), ip(kp["max_step"]),
                    ip(kp["n_above"]), ip(kp["n_changes"]), ip(kp["n_vio"])))
                o["kpi"] = kp
                return o, stats
            if policy:
                o["switches"] = np.zeros((B, S), np.int32)
                check(_lib.load().mld_rollout_policy(
                    self._h, aux, K, S, _lib.dptr(u_seq), _lib.dptr(u_prev), _lib.dptr(omega_seq) if nw else None, lp(st), int(step), _lib.dptr(cost_w), rows,
                    _lib.dptr(o.get("x")), _lib.dptr(o.get("v")), _lib.dptr(o.get("y")), _lib.dptr(o.get("cons_vio")), ip(o.get("cons_row")),
                    _lib.dptr(o["cost"]), _lib.dptr(o["mu_total"]), _lib.dptr(o["worst_vio"]), ip(o["worst_step"]), ip(o["steps_done"]), ip(o["end_status"]),
                    ip(o["switches"]), lp(stats)))
                return o, stats
            check(_lib.load().mld_rollout_batch(
                self._h, aux, K, S, _lib.dptr(u_seq), _lib.dptr(omega_seq) if nw else None, lp(st), int(step), _lib.dptr(cost_w), rows,
                _lib.dptr(o.get("x")), _lib.dptr(o.get("v")), _lib.dptr(o.get("y")), _lib.dptr(o.get("cons_vio")), ip(o.get("cons_row")),
                _lib.dptr(o["cost"]), _lib.dptr(o["mu_total"]), _lib.dptr(o["worst_vio"]), ip(o["worst_step"]), ip(o["steps_done"]), ip(o["end_status"]),
                lp(stats)))
            return o, stats

        out, stats = call(trajectories, per_trajectory)
        n_host = 0 if getattr(self, "_ro_dev", False) else int(stats[3])
        if n_host:
            if not trajectories or not per_trajectory:
                out, stats = call(True)      # (the completion continues from the states and slices the device left: it needs the trajectories)
            midx = getattr(self, "_model_idx", None)
            midx = np.zeros(B, np.int64) if midx is None else np.asarray(midx, np.int64)
            if midx.shape != (B,):
                raise MldGpuError("rollout: the model indices of the resident batch are not known on the host (upload() keeps them)")
            P = getattr(self, "_policy", None) if policy else None
            if policy and P is None:
                raise MldGpuError("rollout: the resident policy is not known on the host (upload_policy() keeps it)")
            if u_seq is None and P is not None and P.all_ruled:
                u_all = np.zeros((B, K, nu))      # (never read: every channel is ruled)
            elif u_seq is None:
                u_all = np.ascontiguousarray(self.download()["v"].reshape(B, self.N_tilde, nv)[:, :K, :nu])
            else:
                u_all = u_seq
            up_t = None
            if P is not None:
                up_t = np.repeat(self.policy_state() if u_prev is None else u_prev, S, axis=0)
            if omega_seq is None and nw:
                from . import profiles
                om_all = profiles.windows(self._pf_lib, st.reshape(B * S, -1), int(step), K, self._pf_width).reshape(B, S, K, nw)
            else:
                om_all = omega_seq if nw else np.zeros((B, S, K, 0))
            T = B * S
            kpi_dev, risk_dev = out.pop("kpi", None), out.pop("risk", None)
            flat = {k: out[k].reshape((T,) + out[k].shape[2:]) for k in out}
            todo = np.where(flat["end_status"] == 2)[0]
            n_host = int(todo.size)
            cw_t = None
            if cost_w is not None:
                cw_t = np.repeat(cost_w if rows != self.model.n_models else cost_w[midx], S, axis=0)
            simlog.rollout_continue(resolve.mats, d, np.repeat(midx, S), np.repeat(u_all, S, axis=0), om_all.reshape(T, K, nw), flat, todo, resolve.resolve, cw_t,
                                    policy=P, u_prev=up_t)
            out = {k: flat[k].reshape(out[k].shape) for k in out}
            if kpi_dev is not None:      # the trajectories finished here take the numpy rule's figures of the finished trajectory: one convention for the caller
                price = None
                if pst is not None and np.any(karr["price_chan"] >= 0):
                    from . import prices
                    if getattr(self, "_pr_lib", None) is None:
                        raise MldGpuError("rollout: the price library is not known on the host (upload_prices() keeps it)")
                    price = prices.windows(self._pr_lib, pst, int(step), K, self._pr_chan).reshape(B, K, self._pr_chan)
                host = simlog.rollout_kpis_np(out, kpis, price=price, vio_tol=vio_tol, omega_seq=om_all if nw else None, model_idx=midx)
                sel = todo // S, todo % S
                for key in simlog.KPI_ROLLOUT_KEYS:
                    kpi_dev[key][sel] = host[key][sel]
                out["kpi"] = kpi_dev
            if risk_dev is not None:      # the instances with a trajectory finished here take the numpy rule's figures of the finished arrays
                host = simlog.rollout_risk_np(out, risk, policy=bool(policy))
                sel = np.unique(todo // S)
                for key in simlog.RISK_COL_KEYS + simlog.RISK_LEVEL_KEYS + simlog.RISK_COUNTS:
                    risk_dev[key][sel] = host[key][sel]
                out["risk"] = risk_dev
        es = out.get("end_status")
        out["stats"] = dict(trajectories=int(stats[0]), complete=int((es == 0).sum()) if n_host else int(stats[1]), infeasible=int((es == 1).sum()) if n_host else int(stats[2]),
                            declined=int(stats[3]), not_attempted=int(stats[0] - stats[1] - stats[2] - stats[3]), finished_on_host=n_host)
        if getattr(self, "_ro_dev", False):
            out["stats"] = self._device_stats(stats)
        if n_host and not trajectories:
            for k in ("x", "v", "y", "cons_vio", "cons_row"):
                del out[k]
        if not per_trajectory:
            out = dict(risk=out["risk"], stats=out["stats"])
        return out

    @_completes(True)
    @_keeps
    def select_plan(self, resolve, selector, candidates=None, plan_first=False, K=None, omega_seq=None, start=None, step=0, cost_w=None, kpis=None,
                    price_start=None, vio_tol=1e-6, min_complete=None, per_candidate=False, per_trajectory=False):
        """choose, per instance, among P candidate input sequences by their rollout risk, on device (mld_rollout_select; kernels k_rollout_cand /
        k_rollout_cand_kpi, k_rollout_risk, k_plan_select): every candidate is rolled out open loop under the SAME S realisations in one launch, each
        candidate's risk is rollout(risk=...)'s, and the admissible candidate of least objective statistic wins (simlog.PlanSelector; the smaller p on a tie).
        selector: a simlog.PlanSelector over the simlog.RiskTable of the call.  candidates (batch, P', K, nu) or (P', K, nu) for every instance;
        plan_first=True puts the resident plan's inputs in front as candidate 0 (P = P' + 1; candidates=None certifies the plan alone; an instance
        without a usable plan ends -1 for that candidate only).  resolve, K, omega_seq / start, step, cost_w, kpis, price_start, vio_tol: rollout()'s.
        min_complete: the least number of complete realisations of an admissible candidate, 1 .. S, None = S.  The handle is not changed.
        Returns dict(choice (batch,) int32, -1 = no admissible candidate; score (batch,), its objective, NaN without one; n_admissible (batch,) int32;
        admissible (batch, P) bool; u (batch, K, nu) the chosen sequence and u0 (batch, nu) its step 0 -- what sim_step(resolve=R, u0=...) takes --, NaN
        without a choice; stats as rollout()'s over batch P S trajectories).  per_candidate=True adds risk: rollout(risk=...)'s dict with a candidate axis,
        (batch, P, G[, L]) and (batch, P) counts; per_trajectory=True adds cost, mu_total, worst_vio, worst_step, steps_done, end_status (batch, P, S) and,
        with kpis, kpi (batch, P, S, n_kpi).  The figures are those of simlog.select_plan_np on that risk, bit for bit.  Trajectories the device's LDS solver
        declined are finished on the host as rollout() finishes them: the instances they belong to take every candidate's risk from rollout() itself and
        their choice from select_plan_np.  complete="device" (rollout()'s): they are finished on the device before k_rollout_risk and k_plan_select read
        them, and the host route is never entered.
        keep=True (a keyword of the wrapper, like complete=): the choice and the chosen inputs also stay on the device as the kept selection
        (mld_keep_selection; selection() reads it), which sim_step(resolve=R, selected=True) applies; instances finished on the host are corrected there
        (set_selection), so the device holds what this method returns.  keep=False (the default) allocates nothing, queues no extra copy and drops a
        selection an earlier keep=True left."""
        from . import simlog
        d, B, nv = self.model.dims, self.batch, self.model.nv
        nx, nu, nw, ny = d["nx"], d["nu"], d["nomega"], d["ny"]
        pf = 1 if plan_first else 0
        cand = None
        if candidates is not None:
            cand = np.asarray(candidates, dtype=np.float64)
            if cand.ndim == 3:
                cand = np.broadcast_to(cand, (B,) + cand.shape)
            if cand.ndim != 4 or cand.shape[0] != B or cand.shape[3] != nu or (K is not None and cand.shape[2] != int(K)):
                raise ValueError("candidates has shape %s, expected (%d, P, K, %d) or (P, K, %d)%s" % (cand.shape, B, nu, nu, "" if K is None else " with K = %d" % int(K)))
            cand = np.ascontiguousarray(cand)
            K = cand.shape[2]
        elif not plan_first:
            raise ValueError("no candidate: candidates is None and plan_first is False")
        K = self.N_tilde if K is None else int(K)
        n_own = 0 if cand is None else cand.shape[1]
        P = n_own + pf
        if P < 1 or P > simlog.SELECT_P_MAX:
            raise ValueError("P = %d candidates (1 .. %d)" % (P, simlog.SELECT_P_MAX))
        if not isinstance(selector, simlog.PlanSelector):
            raise ValueError("selector: a simlog.PlanSelector")
        risk = selector.risk
        sarr, rarr = selector.arrays(), risk.arrays()
        omega_seq, st, S, cost_w, rows, karr, ktabs, kthr, pst = self._rollout_inputs(K, omega_seq, start, cost_w, kpis, price_start)
        if S > simlog.RISK_S_MAX:
            raise ValueError("risk: S = %d realisations (at most %d)" % (S, simlog.RISK_S_MAX))
        min_complete = S if min_complete is None else int(min_complete)
        if not 1 <= min_complete <= S:
            raise ValueError("min_complete = %d (1 .. S = %d)" % (min_complete, S))
        if np.any(rarr["col_src"] == 3):
            raise ValueError("risk column %r reads switches, but a selection rolls out open loop" % (risk.names[int(np.flatnonzero(rarr["col_src"] == 3)[0])],))
        Q, chan = 0, None
        if kpis is None:
            ktabs = [None] * 5
            if np.any(rarr["col_src"] >= 4):
                raise ValueError("risk column %r reads the KPIs, but kpis is None" % (risk.names[int(np.flatnonzero(rarr["col_src"] >= 4)[0])],))
        else:
            if np.any(rarr["col_src"] >= 4) and risk.kpis is not kpis and list(risk.kpis.names) != list(kpis.names):
                raise ValueError("the risk table was built over another KPI table (%s, this call's %s)" % (risk.kpis.names, kpis.names))
            Q, chan = len(kpis), karr["price_chan"]
        aux = resolve.problem._h if resolve is not None and resolve.problem is not None else None
        ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32)) if a is not None else None
        lp = lambda a: a.ctypes.data_as(C.POINTER(C.c_int64)) if a is not None else None
        G, L = len(risk), len(risk.levels)
        out = dict(choice=np.zeros(B, np.int32), score=np.zeros(B), n_admissible=np.zeros(B, np.int32), admissible=np.zeros((B, P), np.uint8),
                   u=np.zeros((B, K, nu)), u0=np.zeros((B, nu)))
        rk = dict(names=list(risk.names), levels=list(risk.levels))
        if per_candidate:
            rk.update(mean=np.zeros((B, P, G)), min=np.zeros((B, P, G)), min_c=np.zeros((B, P, G), np.int32), max=np.zeros((B, P, G)), max_c=np.zeros((B, P, G), np.int32),
                      n_exceed=np.zeros((B, P, G), np.int32), quantile=np.zeros((B, P, G, L)), quantile_c=np.zeros((B, P, G, L), np.int32),
                      cvar_hi=np.zeros((B, P, G, L)), cvar_lo=np.zeros((B, P, G, L)))
        counts = np.zeros((B, P, 4), np.int32)
        per, kp = {}, {}
        if per_trajectory:
            per = dict(cost=np.zeros((B, P, S)), mu_total=np.zeros((B, P, S)), worst_vio=np.zeros((B, P, S)), worst_step=np.zeros((B, P, S), np.int32),
                       steps_done=np.zeros((B, P, S), np.int32), end_status=np.zeros((B, P, S), np.int32))
            if kpis is not None:
                kp = dict(names=list(kpis.names), sum=np.zeros((B, P, S, Q)), min=np.zeros((B, P, S, Q)), max=np.zeros((B, P, S, Q)), min_step=np.zeros((B, P, S, Q), np.int32),
                          max_step=np.zeros((B, P, S, Q), np.int32), n_above=np.zeros((B, P, S, Q), np.int32), n_changes=np.zeros((B, P, S, Q), np.int32),
                          n_vio=np.zeros((B, P, S), np.int32))
        stats = np.zeros(4, np.int64)
        oc, ok, ol = sarr["obj"]
        nc = sarr["n_cons"]
        check(_lib.load().mld_rollout_select(
            self._h, aux, K, S, P, pf, _lib.dptr(cand), _lib.dptr(omega_seq) if nw else None, lp(st), int(step), _lib.dptr(cost_w), rows, Q,
            *([_lib.dptr(t) for t in ktabs] + [ip(chan), _lib.dptr(kthr), float(vio_tol), lp(pst)]),
            G, ip(rarr["col_src"]), ip(rarr["col_q"]), _lib.dptr(rarr["level"]), L, _lib.dptr(rarr["alpha"]),
            int(oc), int(ok), int(ol), nc, ip(sarr["cons_col"]) if nc else None, ip(sarr["cons_kind"]) if nc else None, ip(sarr["cons_level"]) if nc else None,
            _lib.dptr(sarr["cons_bound"]) if nc else None, min_complete,
            ip(out["choice"]), _lib.dptr(out["score"]), ip(out["n_admissible"]), out["admissible"].ctypes.data_as(C.POINTER(C.c_uint8)), _lib.dptr(out["u"]), _lib.dptr(out["u0"]),
            _lib.dptr(rk.get("mean")), _lib.dptr(rk.get("min")), _lib.dptr(rk.get("max")), ip(rk.get("min_c")), ip(rk.get("max_c")), ip(rk.get("n_exceed")),
            _lib.dptr(rk.get("quantile")), ip(rk.get("quantile_c")), _lib.dptr(rk.get("cvar_hi")), _lib.dptr(rk.get("cvar_lo")), ip(counts),
            _lib.dptr(per.get("cost")), _lib.dptr(per.get("mu_total")), _lib.dptr(per.get("worst_vio")), ip(per.get("worst_step")), ip(per.get("steps_done")),
            ip(per.get("end_status")), lp(stats), _lib.dptr(kp.get("sum")), _lib.dptr(kp.get("min")), _lib.dptr(kp.get("max")),
            ip(kp.get("min_step")), ip(kp.get("max_step")), ip(kp.get("n_above")), ip(kp.get("n_changes")), ip(kp.get("n_vio"))))
        out["admissible"] = out["admissible"].astype(bool)
        n_host = 0 if getattr(self, "_ro_dev", False) else int(stats[3])
        n_done = [int(stats[1]), int(stats[2])]
        if n_host:      # finished on the host, by rollout() itself: one call per candidate, the route this entry point replaces
            sel = np.flatnonzero((counts[:, :, 2] > 0).any(axis=1))
            host = []
            for p in range(P):
                kw = dict(K=K) if (pf and p == 0) else dict(u_seq=cand[:, p - pf])
                host.append(self.rollout(resolve, omega_seq=omega_seq, start=start, step=step, cost_w=cost_w, kpis=kpis, price_start=price_start, vio_tol=vio_tol,
                                         risk=risk, **kw))
            keys = simlog.RISK_COL_KEYS + simlog.RISK_LEVEL_KEYS
            full = {k: np.stack([h["risk"][k][sel] for h in host], axis=1) for k in keys + simlog.RISK_COUNTS}
            for i, key in enumerate(simlog.RISK_COUNTS):
                counts[sel, :, i] = full[key]
            if per_candidate:
                for k in keys:
                    rk[k][sel] = full[k]
            for k in per:
                per[k][sel] = np.stack([h[k][sel] for h in host], axis=1)
            for k in kp:
                if k != "names":
                    kp[k][sel] = np.stack([h["kpi"][k][sel] for h in host], axis=1)
            allc = cand
            if pf:
                plan_u = self.download()["v"].reshape(B, self.N_tilde, nv)[:, None, :K, :nu]
                allc = plan_u if cand is None else np.concatenate([plan_u, cand], axis=1)
            pick = simlog.select_plan_np(full, selector, min_complete, candidates=allc[sel])
            for k in ("choice", "score", "n_admissible", "admissible", "u", "u0"):
                out[k][sel] = pick[k]
            es = np.stack([h["end_status"] for h in host], axis=1)
            n_done = [int((es == 0).sum()), int((es == 1).sum())]
        out["stats"] = dict(trajectories=int(stats[0]), complete=n_done[0], infeasible=n_done[1], declined=int(stats[3]),
                            not_attempted=int(stats[0] - stats[1] - stats[2] - stats[3]), finished_on_host=n_host)
        if getattr(self, "_ro_dev", False):
            out["stats"] = self._device_stats(stats)
        if per_candidate:
            for i, key in enumerate(simlog.RISK_COUNTS):
                rk[key] = np.ascontiguousarray(counts[:, :, i])
            out["risk"] = rk
        if per_trajectory:
            out.update(per)
            if kp:
                out["kpi"] = kp
        return out

    @_completes(False)
    @_keeps
    def select_plan_policies(self, resolve, selector, policies=None, u_prev=None, candidates=None, plan_first=False, K=None, omega_seq=None, start=None, step=0,
                             cost_w=None, kpis=None, price_start=None, vio_tol=1e-6, min_complete=None, per_candidate=False, per_trajectory=False):
        """select_plan() with closed-loop rule policies among the candidates (mld_rollout_select_policy; kernels k_rollout_cand_policy /
        k_rollout_cand_policy_kpi, k_rollout_risk, k_plan_select, k_select_inputs).  Every argument of select_plan() means what it means there.
        policies: a list of policy.ThresholdPolicy, every channel ruled -- T more candidates BEHIND the plan and the sequences, each stepped in CLOSED loop
        under the same realisations: the reference's thermostat as the yardstick of the comparison and as the fall-back of the safety filter, or a family of
        bands to tune.  u_prev (batch, nu) / (nu,): the input before step 0, None = the resident policy state (upload_policy), which the call leaves as it
        is, like everything else on the handle.  Returns what select_plan() returns and policy (batch,) int32, the index into `policies` of the choice or
        -1; for an instance whose choice is a policy u0 is the rule's step 0 on (x0, u_prev) -- what sim_step(resolve=R, u0=...) takes --, u[:, 0] that row
        and u[:, 1:] NaN (the later inputs differ from realisation to realisation); per_trajectory=True adds switches (batch, P, S): 0 for a complete plan or
        sequence trajectory, -1 where it did not end 0.  A risk column of source switches is accepted.  Nothing is finished on the host on this route: a
        trajectory the LDS solver declines stays 2, counts as n_declined and, with min_complete = S, makes its candidate inadmissible;
        stats["finished_on_host"] is 0.  complete="device" (rollout()'s): such a trajectory is finished on the device before the risk is reduced, so no
        candidate is lost to a decline; complete="host" is refused.  policies None or empty: select_plan() itself, its code path and its result.  keep: select_plan()'s; the kept policy (batch)
        is the returned one."""
        if policies is None or not len(policies):
            if u_prev is not None:
                raise ValueError("u_prev given without policies (an open-loop candidate has no previous input)")
            return self.select_plan(resolve, selector, candidates=candidates, plan_first=plan_first, K=K, omega_seq=omega_seq, start=start, step=step, cost_w=cost_w,
                                    kpis=kpis, price_start=price_start, vio_tol=vio_tol, min_complete=min_complete, per_candidate=per_candidate,
                                    per_trajectory=per_trajectory, **(dict(complete="device") if getattr(self, "_ro_dev", False) else {}))
        policies = list(policies)
        from . import simlog, policy as _policy
        d, B, nv = self.model.dims, self.batch, self.model.nv
        nx, nu, nw = d["nx"], d["nu"], d["nomega"]
        pf = 1 if plan_first else 0
        cand = None
        if candidates is not None:
            cand = np.asarray(candidates, dtype=np.float64)
            if cand.ndim == 3:
                cand = np.broadcast_to(cand, (B,) + cand.shape)
            if cand.ndim != 4 or cand.shape[0] != B or cand.shape[3] != nu or (K is not None and cand.shape[2] != int(K)):
                raise ValueError("candidates has shape %s, expected (%d, P, K, %d) or (P, K, %d)%s" % (cand.shape, B, nu, nu, "" if K is None else " with K = %d" % int(K)))
            cand = np.ascontiguousarray(cand)
            K = cand.shape[2]
        K = self.N_tilde if K is None else int(K)
        n_own, T = 0 if cand is None else cand.shape[1], len(policies)
        P = pf + n_own + T
        if P > simlog.SELECT_P_MAX:
            raise ValueError("P = %d candidates, the %d policies among them (1 .. %d)" % (P, T, simlog.SELECT_P_MAX))
        for t, pol in enumerate(policies):
            if not isinstance(pol, _policy.ThresholdPolicy):
                raise ValueError("policies[%d]: a policy.ThresholdPolicy" % t)
            if (pol.n_models, pol.nu, pol.nx) != (self.model.n_models, nu, nx):
                raise ValueError("policies[%d] is shaped (n_models %d, nu %d, nx %d), the problem (%d, %d, %d)" % (t, pol.n_models, pol.nu, pol.nx, self.model.n_models, nu, nx))
            if not pol.all_ruled:
                m, j = np.argwhere(pol.mode == 0)[0]
                raise ValueError("policies[%d] passes channel %d of model %d through: a policy candidate rules every channel (a candidate that rules some channels and "
                                 "takes the plan for the others is not built)" % (t, j, m))
        u_prev = self._u_prev_array(u_prev, True)
        if not isinstance(selector, simlog.PlanSelector):
            raise ValueError("selector: a simlog.PlanSelector")
        risk = selector.risk
        sarr, rarr = selector.arrays(), risk.arrays()
        omega_seq, st, S, cost_w, rows, karr, ktabs, kthr, pst = self._rollout_inputs(K, omega_seq, start, cost_w, kpis, price_start)
        if S > simlog.RISK_S_MAX:
            raise ValueError("risk: S = %d realisations (at most %d)" % (S, simlog.RISK_S_MAX))
        min_complete = S if min_complete is None else int(min_complete)
        if not 1 <= min_complete <= S:
            raise ValueError("min_complete = %d (1 .. S = %d)" % (min_complete, S))
        Q, chan = 0, None
        if kpis is None:
            ktabs = [None] * 5
            if np.any(rarr["col_src"] >= 4):
                raise ValueError("risk column %r reads the KPIs, but kpis is None" % (risk.names[int(np.flatnonzero(rarr["col_src"] >= 4)[0])],))
        else:
            if np.any(rarr["col_src"] >= 4) and risk.kpis is not kpis and list(risk.kpis.names) != list(kpis.names):
                raise ValueError("the risk table was built over another KPI table (%s, this call's %s)" % (risk.kpis.names, kpis.names))
            Q, chan = len(kpis), karr["price_chan"]
        tabs = {k: np.ascontiguousarray(np.stack([getattr(pol, k) for pol in policies])) for k in ("sel", "on_at", "off_at", "u_on", "u_off")}
        modes = np.ascontiguousarray(np.stack([pol.mode for pol in policies]), dtype=np.int32)
        aux = resolve.problem._h if resolve is not None and resolve.problem is not None else None
        ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32)) if a is not None else None
        lp = lambda a: a.ctypes.data_as(C.POINTER(C.c_int64)) if a is not None else None
        G, L = len(risk), len(risk.levels)
        out = dict(choice=np.zeros(B, np.int32), score=np.zeros(B), n_admissible=np.zeros(B, np.int32), admissible=np.zeros((B, P), np.uint8),
                   u=np.zeros((B, K, nu)), u0=np.zeros((B, nu)))
        rk = dict(names=list(risk.names), levels=list(risk.levels))
        if per_candidate:
            rk.update(mean=np.zeros((B, P, G)), min=np.zeros((B, P, G)), min_c=np.zeros((B, P, G), np.int32), max=np.zeros((B, P, G)), max_c=np.zeros((B, P, G), np.int32),
                      n_exceed=np.zeros((B, P, G), np.int32), quantile=np.zeros((B, P, G, L)), quantile_c=np.zeros((B, P, G, L), np.int32),
                      cvar_hi=np.zeros((B, P, G, L)), cvar_lo=np.zeros((B, P, G, L)))
        counts = np.zeros((B, P, 4), np.int32)
        per, kp = {}, {}
        if per_trajectory:
            per = dict(cost=np.zeros((B, P, S)), mu_total=np.zeros((B, P, S)), worst_vio=np.zeros((B, P, S)), worst_step=np.zeros((B, P, S), np.int32),
                       steps_done=np.zeros((B, P, S), np.int32), end_status=np.zeros((B, P, S), np.int32), switches=np.zeros((B, P, S), np.int32))
            if kpis is not None:
                kp = dict(names=list(kpis.names), sum=np.zeros((B, P, S, Q)), min=np.zeros((B, P, S, Q)), max=np.zeros((B, P, S, Q)), min_step=np.zeros((B, P, S, Q), np.int32),
                          max_step=np.zeros((B, P, S, Q), np.int32), n_above=np.zeros((B, P, S, Q), np.int32), n_changes=np.zeros((B, P, S, Q), np.int32),
                          n_vio=np.zeros((B, P, S), np.int32))
        stats = np.zeros(4, np.int64)
        oc, ok, ol = sarr["obj"]
        nc = sarr["n_cons"]
        check(_lib.load().mld_rollout_select_policy(
            self._h, aux, K, S, P, pf, _lib.dptr(cand), _lib.dptr(omega_seq) if nw else None, lp(st), int(step), _lib.dptr(cost_w), rows, Q,
            *([_lib.dptr(t) for t in ktabs] + [ip(chan), _lib.dptr(kthr), float(vio_tol), lp(pst)]),
            G, ip(rarr["col_src"]), ip(rarr["col_q"]), _lib.dptr(rarr["level"]), L, _lib.dptr(rarr["alpha"]),
            int(oc), int(ok), int(ol), nc, ip(sarr["cons_col"]) if nc else None, ip(sarr["cons_kind"]) if nc else None, ip(sarr["cons_level"]) if nc else None,
            _lib.dptr(sarr["cons_bound"]) if nc else None, min_complete,
            ip(out["choice"]), _lib.dptr(out["score"]), ip(out["n_admissible"]), out["admissible"].ctypes.data_as(C.POINTER(C.c_uint8)), _lib.dptr(out["u"]), _lib.dptr(out["u0"]),
            _lib.dptr(rk.get("mean")), _lib.dptr(rk.get("min")), _lib.dptr(rk.get("max")), ip(rk.get("min_c")), ip(rk.get("max_c")), ip(rk.get("n_exceed")),
            _lib.dptr(rk.get("quantile")), ip(rk.get("quantile_c")), _lib.dptr(rk.get("cvar_hi")), _lib.dptr(rk.get("cvar_lo")), ip(counts),
            _lib.dptr(per.get("cost")), _lib.dptr(per.get("mu_total")), _lib.dptr(per.get("worst_vio")), ip(per.get("worst_step")), ip(per.get("steps_done")),
            ip(per.get("end_status")), lp(stats), _lib.dptr(kp.get("sum")), _lib.dptr(kp.get("min")), _lib.dptr(kp.get("max")),
            ip(kp.get("min_step")), ip(kp.get("max_step")), ip(kp.get("n_above")), ip(kp.get("n_changes")), ip(kp.get("n_vio")),
            T, _lib.dptr(tabs["sel"]), _lib.dptr(tabs["on_at"]), _lib.dptr(tabs["off_at"]), _lib.dptr(tabs["u_on"]), _lib.dptr(tabs["u_off"]), ip(modes),
            _lib.dptr(u_prev), ip(per.get("switches"))))
        out["admissible"] = out["admissible"].astype(bool)
        out["policy"] = np.where(out["choice"] >= P - T, out["choice"] - (P - T), -1).astype(np.int32)
        out["stats"] = dict(trajectories=int(stats[0]), complete=int(stats[1]), infeasible=int(stats[2]), declined=int(stats[3]),
                            not_attempted=int(stats[0] - stats[1] - stats[2] - stats[3]), finished_on_host=0)
        if getattr(self, "_ro_dev", False):
            out["stats"] = self._device_stats(stats)
        if per_candidate:
            for i, key in enumerate(simlog.RISK_COUNTS):
                rk[key] = np.ascontiguousarray(counts[:, :, i])
            out["risk"] = rk
        if per_trajectory:
            out.update(per)
            if kp:
                out["kpi"] = kp
        return out

    # -- the kept selection ---------------------------------------------------------------------------------
    def _keep_selection(self, keep):
        """the sticky switch of the select calls as this call wants it; switching it off frees what it kept (a set_selection() of the caller's stays)"""
        if bool(keep) != getattr(self, "_sel_keep", False):
            check(_lib.load().mld_keep_selection(self._h, 1 if keep else 0))
            self._sel_keep = bool(keep)

    def selection(self):
        """the kept selection (mld_download_selection): dict(K, choice (batch,) int32, policy (batch,) int32, u (batch, K, nu), valid) -- what the last
        select_plan(..., keep=True) / select_plan_policies(..., keep=True) chose, or set_selection() set; valid: it was made for the current inputs, so
        sim_step(resolve=R, selected=True) takes it.  The arrays are None where the batch it belonged to is gone."""
        B, nu = self.batch, self.model.dims["nu"]
        K, valid = C.c_int32(0), C.c_int32(0)
        check(_lib.load().mld_download_selection(self._h, C.byref(K), None, None, None, C.byref(valid)))
        out = dict(K=int(K.value), choice=None, policy=None, u=None, valid=bool(valid.value))
        arr = dict(choice=np.zeros(B, np.int32), policy=np.zeros(B, np.int32), u=np.zeros((B, out["K"], nu)))
        ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
        if _lib.load().mld_download_selection(self._h, None, ip(arr["choice"]), ip(arr["policy"]), _lib.dptr(arr["u"]), None) == 0:
            out.update(arr)
        elif out["valid"]:
            check(-1)
        return out

    def set_selection(self, choice, u, policy=None):
        """a selection of the caller's as the kept one (mld_set_selection): choice (batch,) ints, -1 = none; u (batch, K, nu) the chosen inputs, row 0
        finite where there is a choice and every row for a plan or sequence pick; policy (batch,) ints or None (every pick a sequence).  It is made for
        the current inputs, and sim_step(resolve=R, selected=True) applies it like a kept one."""
        B, nu = self.batch, self.model.dims["nu"]
        choice = np.asarray(choice)
        if choice.shape != (B,) or not np.issubdtype(choice.dtype, np.integer):
            raise ValueError("choice has shape %s and dtype %s, expected (%d,) integers" % (choice.shape, choice.dtype, B))
        u = np.asarray(u, dtype=np.float64)
        if u.ndim != 3 or u.shape[0] != B or u.shape[2] != nu:
            raise ValueError("u has shape %s, expected (%d, K, %d)" % (u.shape, B, nu))
        if policy is not None:
            policy = np.asarray(policy)
            if policy.shape != (B,) or not np.issubdtype(policy.dtype, np.integer):
                raise ValueError("policy has shape %s and dtype %s, expected (%d,) integers" % (policy.shape, policy.dtype, B))
            policy = np.ascontiguousarray(policy, dtype=np.int32)
        choice, u = np.ascontiguousarray(choice, dtype=np.int32), np.ascontiguousarray(u)
        ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32)) if a is not None else None
        check(_lib.load().mld_set_selection(self._h, u.shape[1], ip(choice), ip(policy), _lib.dptr(u)))

    def sim_log(self, first=0, count=None):
        """records [first, first + count) of the resident log (mld_download_sim_log; count=None: all from first): dict of arrays (count, batch, width) --
        x, v, y, omega, x_k1, cons (bool), cons_vio, cons_row, obj, lower_bound, status, nodes.  simlog.to_mld_sim_log turns one instance into the
        reference's MldSimLog."""
        d, B = self.model.dims, self.batch
        first = int(first)
        if count is None:
            count = self.sim_log_count()[0] - first
        K = int(count)
        if K < 0:
            raise ValueError("sim_log: first = %d lies beyond the %d logged steps" % (first, K + first))
        out = dict(x=np.zeros((K, B, d["nx"])), v=np.zeros((K, B, self.model.nv)), y=np.zeros((K, B, d["ny"])), omega=np.zeros((K, B, d["nomega"])),
                   x_k1=np.zeros((K, B, d["nx"])), cons=np.zeros((K, B, d["nc"]), np.uint8), cons_vio=np.zeros((K, B)), cons_row=np.zeros((K, B), np.int32),
                   obj=np.zeros((K, B)), lower_bound=np.zeros((K, B)), status=np.zeros((K, B), np.int32), nodes=np.zeros((K, B), np.int32))
        ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
        check(_lib.load().mld_download_sim_log(
            self._h, first, K, _lib.dptr(out["x"]), _lib.dptr(out["v"]), _lib.dptr(out["y"]), _lib.dptr(out["omega"]), _lib.dptr(out["x_k1"]),
            out["cons"].ctypes.data_as(C.POINTER(C.c_uint8)), _lib.dptr(out["cons_vio"]), ip(out["cons_row"]), _lib.dptr(out["obj"]),
            _lib.dptr(out["lower_bound"]), ip(out["status"]), ip(out["nodes"])))
        out["cons"] = out["cons"].astype(bool)
        return out

    def sim_log_aux(self, first=0, count=None):
        """the resolver's status per record and instance (mld_download_sim_log_aux), (count, batch) int32: what sim_step(resolve=...) returned as aux_status,
        -2 for the records a plain sim_step wrote"""
        first = int(first)
        if count is None:
            count = self.sim_log_count()[0] - first
        K = int(count)
        if K < 0:
            raise ValueError("sim_log_aux: first = %d lies beyond the %d logged steps" % (first, K + first))
        out = np.zeros((K, self.batch), np.int32)
        check(_lib.load().mld_download_sim_log_aux(self._h, first, K, out.ctypes.data_as(C.POINTER(C.c_int32))))
        return out

    def sim_log_source(self, first=0, count=None):
        """the source of u per record and instance (mld_download_sim_log_source), (count, batch) int32: what sim_step(resolve=R, fallback=...) returned as
        u_source (0 plan, 1 memory, 2 policy, -1 none), -2 for the records any other step wrote"""
        first = int(first)
        if count is None:
            count = self.sim_log_count()[0] - first
        K = int(count)
        if K < 0:
            raise ValueError("sim_log_source: first = %d lies beyond the %d logged steps" % (first, K + first))
        out = np.zeros((K, self.batch), np.int32)
        check(_lib.load().mld_download_sim_log_source(self._h, first, K, out.ctypes.data_as(C.POINTER(C.c_int32))))
        return out

    def sim_log_pick(self, first=0, count=None):
        """the candidate applied per record and instance (mld_download_sim_log_pick), (count, batch) int32: what sim_step(resolve=R, selected=True)
        returned as pick (the choice where the source is 3, -1 elsewhere), -2 for the records any other step wrote"""
        first = int(first)
        if count is None:
            count = self.sim_log_count()[0] - first
        K = int(count)
        if K < 0:
            raise ValueError("sim_log_pick: first = %d lies beyond the %d logged steps" % (first, K + first))
        out = np.zeros((K, self.batch), np.int32)
        check(_lib.load().mld_download_sim_log_pick(self._h, first, K, out.ctypes.data_as(C.POINTER(C.c_int32))))
        return out

    def sim_log_summary(self, kpis, first=0, count=None, vio_tol=1e-6):
        """column statistics of records [first, first + count) of the resident log, reduced on the device (mld_sim_log_summary, kernel k_log_summary;
        count=None: all from first) -- the figures the reference quotes from grid_sim_dataframe, without downloading the records.  kpis: a
        simlog.KpiTable over this problem's models.  Returns dict(names, sum, min, max (batch, n_kpi), min_step, max_step, n_above, n_changes (batch, n_kpi)
        int32, n_stepped, vio_step, n_vio (batch,) int32, vio_max (batch,), nodes_total (batch,) int64, n_source (batch, 3) int32); simlog.summary_np
        states the rule and gives the same bits from the downloaded log.  Nothing on the handle changes."""
        from .simlog import KPI_TABLES
        if kpis.n_models != self.model.n_models:
            raise ValueError("the KPI table has %d models, the problem %d" % (kpis.n_models, self.model.n_models))
        d = self.model.dims
        want = dict(w_x=d["nx"], w_v=self.model.nv, w_y=d["ny"], w_omega=d["nomega"], w_xk1=d["nx"])
        if kpis.widths != want:
            raise ValueError("the KPI table was built for other dimensions (%s, this problem %s)" % (kpis.widths, want))
        arr = kpis.arrays()
        first = int(first)
        if count is None:
            count = self.sim_log_count()[0] - first
        K, B, Q = int(count), self.batch, len(kpis)
        if K < 0:
            raise ValueError("sim_log_summary: first = %d lies beyond the %d logged steps" % (first, K + first))
        out = dict(names=list(kpis.names), sum=np.zeros((B, Q)), min=np.zeros((B, Q)), max=np.zeros((B, Q)), min_step=np.zeros((B, Q), np.int32),
                   max_step=np.zeros((B, Q), np.int32), n_above=np.zeros((B, Q), np.int32), n_changes=np.zeros((B, Q), np.int32),
                   n_stepped=np.zeros(B, np.int32), vio_max=np.zeros(B), vio_step=np.zeros(B, np.int32), n_vio=np.zeros(B, np.int32),
                   nodes_total=np.zeros(B, np.int64), n_source=np.zeros((B, 3), np.int32))
        ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
        tabs = [None if arr[k] is None else np.ascontiguousarray(arr[k]) for k in KPI_TABLES]
        thr = None if arr["thresh"] is None else np.ascontiguousarray(arr["thresh"])
        check(_lib.load().mld_sim_log_summary(
            self._h, first, K, Q, *([_lib.dptr(t) for t in tabs] + [ip(arr["price_chan"]), _lib.dptr(thr), float(vio_tol)]),
            _lib.dptr(out["sum"]), _lib.dptr(out["min"]), _lib.dptr(out["max"]), ip(out["min_step"]), ip(out["max_step"]), ip(out["n_above"]),
            ip(out["n_changes"]), ip(out["n_stepped"]), _lib.dptr(out["vio_max"]), ip(out["vio_step"]), ip(out["n_vio"]),
            out["nodes_total"].ctypes.data_as(C.POINTER(C.c_int64)), ip(out["n_source"])))
        return out

    def set_warm_start(self, bin_start):
        """MIP start of the resident batch (mld_set_warm_start): (batch, n_bin) values of the binaries, a row starting with 255 = no
        start for that instance; None clears.  A full decision vector (batch, n) is accepted too (its binaries are rounded)."""
        if bin_start is None:
            check(_lib.load().mld_set_warm_start(self._h, None))
            return
        a = np.asarray(bin_start)
        if a.ndim >= 1 and a.reshape(self.batch, -1).shape[1] == self.n and self.n != self.n_bin:
            a = np.rint(a.reshape(self.batch, self.n)[:, self.is_bin])
        a = np.ascontiguousarray(a.reshape(self.batch, self.n_bin), dtype=np.uint8)
        check(_lib.load().mld_set_warm_start(self._h, a.ctypes.data_as(C.POINTER(C.c_uint8))))

    def warm_start_from_previous(self, shift=0):
        """MIP start from the last solution, on device (mld_warm_start_from_previous): shift 0 = the plan as it is (warm_start=True of
        the reference's backend), shift k = moved k steps on with the last step repeated (after advance())"""
        check(_lib.load().mld_warm_start_from_previous(self._h, int(shift)))

    @_completes(False)
    def warm_start_from_rollout(self, resolve, policy=False, u_seq=None, u_prev=None, keep=False):
        """MIP start from a rollout of the current x0 under the resident forecast, on device (mld_warm_start_from_rollout, kernels k_rollout[_policy] and
        k_warm_from_rollout): the start for the instances warm_start_from_previous leaves without one, and for the first solve after an upload.
        policy=True: the resident rule-based policy in closed loop over N_tilde steps (upload_policy; u_prev (batch, nu) / (nu,), None = the resident policy
        state; u_seq only for passed-through channels); policy=False: the caller's u_seq (batch, N_tilde, nu) / (N_tilde, nu) -- another controller's plan,
        its auxiliaries re-derived for this handle's forecast.  resolve: as rollout().  keep=True: an instance whose resident start is not 255 keeps it.
        Returns dict(source (batch,) int32: 1 written, 0 kept, -1 infeasible auxiliaries, -2 the LDS solver declined, -3 not attempted (the last three: row
        255 = no start); stats: dict(trajectories, written, kept, none)).  Nothing else on the handle changes; a problem without binaries gets no start and
        an empty stats.  complete="device" (rollout()'s): an instance whose trajectory the LDS solver declined is finished on the device and gets its start
        (source 1, or -1) instead of -2; stats gains finished_on_device and completion_rounds.  complete="host" is refused."""
        B = self.batch
        if u_seq is not None:
            u_seq = self._u_seq_array(u_seq, self.N_tilde)
        u_prev = self._u_prev_array(u_prev, policy)
        aux = resolve.problem._h if resolve is not None and resolve.problem is not None else None
        source, stats = np.zeros(B, np.int32), np.zeros(4, np.int64)
        check(_lib.load().mld_warm_start_from_rollout(self._h, aux, 1 if policy else 0, _lib.dptr(u_seq), _lib.dptr(u_prev), _lib.MLD_START_KEEP if keep else 0,
                                                      source.ctypes.data_as(C.POINTER(C.c_int32)), stats.ctypes.data_as(C.POINTER(C.c_int64))))
        if not self.n_bin:
            return dict(source=None, stats={})
        st = dict(trajectories=int(stats[0]), written=int(stats[1]), kept=int(stats[2]), none=int(stats[3]))
        if getattr(self, "_ro_dev", False):
            cs = self.rollout_completion_stats()
            st.update(finished_on_device=cs["finished_on_device"], completion_rounds=cs["rounds"])
        return dict(source=source, stats=st)

    def stage(self, x0_sets, omega_sets):
        """input sets of the uploaded batch's size resident in HBM (mld_stage_inputs): x0_sets (n_sets, batch, nx), omega_sets
        (n_sets, batch, N_tilde*nomega); select(k) makes set k current without host traffic"""
        d = self.model.dims
        n_sets = int(np.shape(omega_sets)[0] if self.nW else np.shape(x0_sets)[0])
        x0s = _lib.as_f64(x0_sets).reshape(n_sets, self.batch, d["nx"]) if d["nx"] else None
        oms = _lib.as_f64(omega_sets).reshape(n_sets, self.batch, self.nW) if self.nW else None
        check(_lib.load().mld_stage_inputs(self._h, n_sets, _lib.dptr(x0s), _lib.dptr(oms)))
        return n_sets

    def select(self, k):
        check(_lib.load().mld_select_inputs(self._h, int(k)))

    def inputs(self):
        """current (x0, omega) of the resident batch"""
        d = self.model.dims
        x0, om = np.zeros((self.batch, d["nx"])), np.zeros((self.batch, self.nW))
        check(_lib.load().mld_download_inputs(self._h, _lib.dptr(x0) if d["nx"] else None, _lib.dptr(om) if self.nW else None))
        return x0, om

    def solve_resident(self):
        st = _lib.Stats()
        check(_lib.load().mld_solve_resident(self._h, C.byref(st)))
        return {k: getattr(st, k) for k, _ in _lib.Stats._fields_}

    def use_stream(self):
        """give this problem its own HIP stream (launch / finish of several problems then overlap on the device)"""
        check(_lib.load().mld_problem_use_stream(self._h))

    def launch(self):
        """queue K3 + K5/K6 for the resident batch and return (mld_solve_launch)"""
        check(_lib.load().mld_solve_launch(self._h))

    def finish(self):
        """wait for the launched solve; statistics as solve_resident (mld_solve_finish)"""
        st = _lib.Stats()
        check(_lib.load().mld_solve_finish(self._h, C.byref(st)))
        return {k: getattr(st, k) for k, _ in _lib.Stats._fields_}

    def download(self):
        b = self.batch
        v, obj, lbnd = np.zeros((b, self.n)), np.zeros(b), np.zeros(b)
        status, nodes, pivots = np.zeros(b, np.int32), np.zeros(b, np.int32), np.zeros(b, np.int32)
        ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
        check(_lib.load().mld_download_results(self._h, _lib.dptr(v), _lib.dptr(obj), ip(status), _lib.dptr(lbnd),
                                               ip(nodes), ip(pivots)))
        return dict(v=v, obj=obj, status=status, lower_bound=lbnd, nodes=nodes, pivots=pivots)

    def debug_trace(self, path):
        """diagnostics: every resident workgroup of the solver writes (instance, stage, pivots, queue position) into a file-backed host buffer that
        survives a GPU fault (internal entry mld_debug_trace; None switches it off).  Read it with numpy.fromfile(path, numpy.int32).reshape(-1, 16)."""
        lib = _lib.load()
        lib.mld_debug_trace.restype = C.c_int
        lib.mld_debug_trace.argtypes = [C.c_void_p, C.c_char_p]
        check(lib.mld_debug_trace(self._h, None if path is None else str(path).encode()))

    _SHAPE_KEYS = ("n", "m0", "mcap", "first_cap", "ld", "mir_cap", "lds_bytes", "ws_stride",
                   "lXB", "lBasic", "lSkip", "lAtUp", "lNonbasic", "lXN", "lLo", "lHi", "lDw", "lCost", "lMirLine", "lMirCache",
                   "lds_budget", "slot_mask", "n_slots", "lPair")

    def debug_shape(self):
        """diagnostics: the solver's shape as build_shape placed it (internal entry mld_debug_shape) -- dims, LDS bytes, and the LDS byte offset of
        every hot array (-1: it stays in the slot, e.g. under MLD_SOL_SLOT).  all_lds is true when k_solve runs its typed all-LDS pivot loop."""
        lib = _lib.load()
        lib.mld_debug_shape.restype = C.c_int
        lib.mld_debug_shape.argtypes = [C.c_void_p, C.POINTER(C.c_int64)]
        out = (C.c_int64 * 24)()
        check(lib.mld_debug_shape(self._h, out))
        d = {k: int(out[i]) for i, k in enumerate(self._SHAPE_KEYS)}
        d["all_lds"] = all(d[k] >= 0 for k in ("lXB", "lXN", "lLo", "lHi", "lBasic", "lNonbasic", "lAtUp", "lSkip", "lDw", "lCost"))
        return d

    def debug_warm_start(self):
        """diagnostics: the MIP start the next solve would read (internal entry mld_debug_warm_start) -- (batch, n_bin) uint8, a row starting with 255 = no
        start for that instance; None when no start is set"""
        lib = _lib.load()
        lib.mld_debug_warm_start.restype = C.c_int
        lib.mld_debug_warm_start.argtypes = [C.c_void_p, C.POINTER(C.c_uint8), C.POINTER(C.c_int)]
        out, has = np.zeros((self.batch, self.n_bin), np.uint8), C.c_int(0)
        check(lib.mld_debug_warm_start(self._h, out.ctypes.data_as(C.POINTER(C.c_uint8)), C.byref(has)))
        return out if has.value else None

    def telemetry(self):
        """per-instance in-kernel latency (ns) and dictionary rows updated; row_bytes = bytes per row"""
        b = self.batch
        lat, rows = np.zeros(b, np.int64), np.zeros(b, np.int64)
        rb = C.c_int64()
        ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int64))
        check(_lib.load().mld_download_telemetry(self._h, ip(lat), ip(rows), C.byref(rb)))
        return dict(latency_ns=lat, rows_updated=rows, row_bytes=int(rb.value))

    def solve(self, x0, omega, model_idx=None, fixed_bin=None, omega_cols=None, col_rows=None, x_cols=None, warm_start=None, inst_cost=None, trajectories=False, quality=False,
              col_start=None, col_step=0, price_start=None, price_step=0):
        """upload, solve, download.  col_start / col_step: the constraint blocks gathered from the resident profile library
        (constraint_blocks_from_profiles) instead of uploaded as omega_cols -- one or the other.  price_start / price_step: the per-instance cost built on the device from
        price windows (instance_cost_from_prices; the tables of set_price_cost) instead of uploaded as inst_cost -- one or the other.  inst_cost: dict(lin_v=..., lin_x=..., lin_y=...) of upload_instance_cost for this batch; trajectories=True adds
        the predicted x / y of trajectories() to the result; quality=True adds out["quality"], evaluate() of the plans just computed on the problem
        as posed"""
        if col_start is not None and omega_cols is not None:
            raise ValueError("col_start and omega_cols both given: the constraint blocks come from the profile library or from the caller, not both")
        if price_start is not None and inst_cost:
            raise ValueError("price_start and inst_cost both given: the per-instance cost comes from the price library or from the caller, not both")
        self.upload(x0, omega, model_idx, fixed_bin)
        if inst_cost:
            self.upload_instance_cost(**inst_cost)
        if price_start is not None:
            self.instance_cost_from_prices(price_start, price_step)
        if omega_cols is not None:
            self.upload_constraint_blocks(omega_cols, col_rows, x_cols)
        if col_start is not None:
            self.constraint_blocks_from_profiles(col_start, col_step, col_rows, x_cols)
        if warm_start is not None:
            self.set_warm_start(warm_start)
        stats = self.solve_resident()
        out = self.download()
        out["stats"] = stats
        if trajectories:
            out.update(self.trajectories())
        if quality:
            out["quality"] = self.evaluate()
        return out

    # -- sub-tree hand-off ---------------------------------------------------------------------------
    def set_cutoffs(self, cutoff):
        """objective (constant term included) every instance of the resident batch has to beat (mld_set_cutoffs); inf = none, None clears"""
        if cutoff is None:
            check(_lib.load().mld_set_cutoffs(self._h, None))
            return
        c = _lib.as_f64(cutoff).reshape(self.batch)
        check(_lib.load().mld_set_cutoffs(self._h, _lib.dptr(c)))

    def record_open_nodes(self, enable=True):
        check(_lib.load().mld_record_open_nodes(self._h, 1 if enable else 0))

    def open_nodes(self):
        """search stacks of the instances that stopped at a limit inside a complete search (mld_download_open_nodes):
        depth (batch; -1 = none), var / val / flag (batch, n_bin)"""
        b, nb = self.batch, max(1, self.n_bin)
        depth = np.zeros(b, np.int32)
        var, val, flag = np.zeros((b, nb), np.int16), np.zeros((b, nb), np.uint8), np.zeros((b, nb), np.uint8)
        check(_lib.load().mld_download_open_nodes(self._h, depth.ctypes.data_as(C.POINTER(C.c_int32)), var.ctypes.data_as(C.POINTER(C.c_int16)),
                                                  val.ctypes.data_as(C.POINTER(C.c_uint8)), flag.ctypes.data_as(C.POINTER(C.c_uint8))))
        return depth, var, val, flag

    def set_std_block(self, enable=True):
        """the standard constraint block in or out of the problem (mld_set_std_block): out = only the uploaded constraint blocks constrain"""
        check(_lib.load().mld_set_std_block(self._h, 1 if enable else 0))

    def set_handoff(self, enable=True, sub_nodes=0, max_gen=8, max_children=64, max_tree=160, room_factor=0.0, donate=0, rounds=0):
        """in-kernel sub-tree hand-off (mld_set_handoff): searches that stop at their node limit publish their open nodes as entries of the same
        launch's work queue; takes effect with the next upload().  sub_nodes 0 = the problem's max_nodes for items too.  Switching it on or off,
        or another room_factor while it is on, lays the result arrays out anew: the library drops the resident batch (upload() again before
        solve_resident()), and so does this handle."""
        lib = _lib.load()
        lib.mld_set_handoff.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double]
        check(lib.mld_set_handoff(self._h, 1 if enable else 0, int(sub_nodes), int(max_gen), int(max_children), int(max_tree), float(room_factor)))
        on, factor = self._handoff
        if bool(enable) != on or (enable and room_factor > 0.0 and float(room_factor) != factor):
            self.batch = 0
        self._handoff = (bool(enable), float(room_factor) if room_factor > 0.0 else factor)
        check(lib.mld_set_handoff_policy(self._h, int(donate), int(rounds)))

    def handoff_stats(self):
        out = (C.c_int64 * 4)()
        check(_lib.load().mld_handoff_stats(self._h, out))
        return dict(items=int(out[0]), given_up=int(out[1]), unfinished=int(out[2]), queue_full=int(out[3]))

    def small_lds_stats(self):
        """the small-problem path (flags=_lib.MLD_SMALL_LDS): eligible (the flag is set and the shape fits a wave's LDS), and of the last solve the
        instances answered in LDS and the instances it declined, which the dense kernel re-solved (both 0 when the solve took another path)"""
        out = (C.c_int64 * 3)()
        check(_lib.load().mld_small_lds_stats(self._h, out))
        return dict(eligible=bool(out[0]), lds=int(out[1]), dense=int(out[2]))

    def solve_handoff_device(self, x0, omega, model_idx=None, fixed_bin=None, first_nodes=None, sub_nodes=None, max_gen=8, max_children=64, max_tree=160, room_factor=0.0, donate=0, rounds=0, inst_cost=None, trajectories=False, quality=False,
                             omega_cols=None, col_rows=None, x_cols=None, col_start=None, col_step=0):
        """the batch with the hand-off inside ONE launch (set_handoff): upload, solve, download -- the merged results per instance plus `handoff`
        statistics.  The problem's own limits and the hand-off switch are restored afterwards; switching it drops the resident batch, before and
        after, so a batch that was resident is LOST and none is resident on return (upload() again).  inst_cost: as solve() (items use their source
        instance's cost).  trajectories=True adds the predicted x / y of the merged plans, quality=True out["quality"] = evaluate() of them (both read before the
        resident batch is dropped).  omega_cols / col_start, col_step with col_rows, x_cols: constraint blocks as in solve() (the items see their source
        instance's blocks)."""
        if col_start is not None and omega_cols is not None:
            raise ValueError("col_start and omega_cols both given: the constraint blocks come from the profile library or from the caller, not both")
        keep_nodes = int(self.opts.max_nodes)
        try:
            if first_nodes is not None:
                self.set_opts(max_nodes=int(first_nodes))
            self.set_handoff(True, sub_nodes=int(sub_nodes or 0), max_gen=max_gen, max_children=max_children, max_tree=max_tree, room_factor=room_factor, donate=donate, rounds=rounds)
            self.upload(x0, omega, model_idx, fixed_bin)
            if inst_cost:
                self.upload_instance_cost(**inst_cost)
            if omega_cols is not None:
                self.upload_constraint_blocks(omega_cols, col_rows, x_cols)
            if col_start is not None:
                self.constraint_blocks_from_profiles(col_start, col_step, col_rows, x_cols)
            stats = self.solve_resident()
            out = self.download()
            out["stats"] = stats
            out["handoff"] = self.handoff_stats()
            if trajectories:
                out.update(self.trajectories())
            if quality:
                out["quality"] = self.evaluate()
            return out
        finally:
            self.set_handoff(False)
            self.set_opts(max_nodes=keep_nodes)

    def solve_handoff(self, x0, omega, model_idx=None, fixed_bin=None, rounds=3, first_nodes=None, sub_nodes=None, max_sub=None, sub_opts=None,
                      max_open=128):
        """The batch solved with sub-tree hand-off: a first pass over all instances (node limit `first_nodes`, default the problem's), then up to
        `rounds` passes in which the OPEN NODES of the instances that stopped at the limit -- read off their depth-first stacks -- are solved as
        instances of their own (node limit `sub_nodes` each, the parent's incumbent value as cutoff), so the whole device works on the few large
        trees instead of one workgroup per tree (a quadratic cost included: the open nodes and cutoffs carry the instance's quadratic constant
        through its objective).  An instance is proven once every one of its nodes has been closed; one whose open nodes
        outnumber `max_open` after a pass is given up (NODE_LIMIT with its incumbent and bound); a node that comes back unsplit twice, or
        UNBOUNDED, is dropped -- its tree stays NODE_LIMIT and its bound stays in the tree's.  Returns the dict of
        download() (v, obj, status, lower_bound; nodes / pivots summed over all passes) plus `handoff` statistics; the resident batch afterwards
        is the last pass's sub-batch (upload again before advance() / warm starts)."""
        d = self.model.dims
        x0 = _lib.as_f64(x0).reshape(-1, d["nx"]) if d["nx"] else np.zeros((np.shape(omega)[0], 0))
        B = x0.shape[0] if d["nx"] else int(np.asarray(omega).reshape(-1, max(self.nW, 1)).shape[0])
        omega = _lib.as_f64(omega).reshape(B, self.nW) if self.nW else np.zeros((B, 0))
        mi = np.ascontiguousarray(model_idx, dtype=np.int32) if model_idx is not None else None
        nb = self.n_bin
        base = np.full((B, nb), 255, np.uint8) if fixed_bin is None else np.ascontiguousarray(fixed_bin, dtype=np.uint8).reshape(B, nb).copy()
        pos = np.full(self.n, -1, np.int64)
        pos[np.flatnonzero(self.is_bin)] = np.arange(nb)
        keep_nodes = int(self.opts.max_nodes)
        gap_rel, gap_abs = float(self.opts.gap_rel), float(self.opts.gap_abs)
        self.record_open_nodes(True)
        try:
            if first_nodes is not None:
                self.set_opts(max_nodes=int(first_nodes))
            out = self.solve(x0, omega, mi, None if fixed_bin is None else base)
            depth, var, val, flag = self.open_nodes()
            obj, v, status, lb = out["obj"].copy(), out["v"].copy(), out["status"].copy(), out["lower_bound"].copy()
            nodes, pivots = out["nodes"].astype(np.int64), out["pivots"].astype(np.int64)
            stats = dict(first_pass_ms=out["stats"]["solve_ms"], rounds=[], handed_off=0)

            def expand(fix, dep, vr, vl, fl):
                return expand_open_nodes(fix, dep, vr, vl, fl, pos)

            open_list = {}      # parent -> list of (fixings, lower bound valid for that node)
            for i in np.flatnonzero(status == 2):
                # a search that stopped before it became a plain depth-first search below an incumbent (deepening passes, dive, RINS) has no
                # stack that describes what is left: its one open node is the root, searched again under the incumbent's value as cutoff
                open_list[int(i)] = [(f, lb[i]) for f in (expand(base[i], depth[i], var[i], val[i], flag[i]) if depth[i] >= 0 else [base[i].copy()])]
            stats["handed_off"] = len(open_list)
            if sub_nodes is not None:
                self.set_opts(max_nodes=int(sub_nodes))
            keep_sub = {}
            if sub_opts:                                            # e.g. a shallower root cut loop for the open nodes
                keep_sub = {k: getattr(self.opts, k) for k in sub_opts}
                self.set_opts(**sub_opts)
            stuck_before = set()
            dropped_lb, given_up = {}, set()      # tree -> smallest bound among its dropped nodes (they stay open for good); trees given up by max_open
            for r in range(int(rounds)):
                if not open_list:
                    break
                par = np.array([i for i, lst in open_list.items() for _ in lst], dtype=np.int64)
                fix = np.stack([f for lst in open_list.values() for f, _ in lst])
                nlb = np.array([b_ for lst in open_list.values() for _, b_ in lst])
                if max_sub is not None and par.size > max_sub:
                    break
                self.upload(x0[par], omega[par], mi[par] if mi is not None else None, fix)
                self.set_cutoffs(obj[par])
                if os.environ.get("MLD_HANDOFF_DUMP"):      # diagnostics: the sub-batch about to be solved (post-mortem replay)
                    np.savez(os.environ["MLD_HANDOFF_DUMP"], x0=x0[par], omega=omega[par], midx=(mi[par] if mi is not None else np.zeros(par.size, np.int32)), fix=fix, cutoff=obj[par], round=r)
                st = self.solve_resident()
                sub = self.download()
                d2, v2, l2, f2 = self.open_nodes()
                stats["rounds"].append(dict(sub_instances=int(par.size), parents=len(open_list), ms=st["solve_ms"]))
                rstat = stats["rounds"][-1]
                new_open, stuck = {}, set()
                for s_ in range(par.size):
                    i = int(par[s_])
                    nodes[i] += sub["nodes"][s_]; pivots[i] += sub["pivots"][s_]
                    if np.isfinite(sub["obj"][s_]) and sub["obj"][s_] < obj[i]:
                        obj[i], v[i] = sub["obj"][s_], sub["v"][s_]
                    ss = int(sub["status"][s_])
                    if ss in (0, 1):
                        continue                                    # closed: optimum of the node found, or nothing better than the cutoff in it
                    nl = max(nlb[s_], sub["lower_bound"][s_]) if np.isfinite(sub["lower_bound"][s_]) else nlb[s_]
                    if ss == 2 and d2[s_] >= 0:
                        new_open.setdefault(i, []).extend((f, nl) for f in expand(fix[s_], d2[s_], v2[s_], l2[s_], f2[s_]))
                    else:
                        # a node that could not be split (numerical trouble, no complete search yet) is retried ONCE as it is; coming back unsplit a second
                        # time it stays open for good (the tree ends NODE_LIMIT) instead of being solved again and again with the same budget
                        key = (i, fix[s_].tobytes())
                        if key in stuck_before or ss == 4:
                            stats["dropped"] = stats.get("dropped", 0) + 1
                            dropped_lb[i] = min(dropped_lb.get(i, np.inf), nl)
                            continue
                        stuck_before.add(key)
                        stuck.add(i)
                        new_open.setdefault(i, []).append((fix[s_], nl))
                for i in list(open_list):
                    tol = max(gap_abs, gap_rel * abs(obj[i])) if np.isfinite(obj[i]) else 0.0
                    # what the tree still has open: this round's nodes and every node dropped so far (not proven: the tree stays NODE_LIMIT)
                    left = [b_ for _, b_ in new_open.get(i, ())] + ([dropped_lb[i]] if i in dropped_lb else [])
                    if not left:                                    # every node closed: proven
                        status[i] = 0 if np.isfinite(obj[i]) else 1
                        lb[i] = min(obj[i], max(lb[i], obj[i] - tol)) if np.isfinite(obj[i]) else lb[i]
                    else:
                        lb[i] = max(lb[i], min(min(left), obj[i] - tol if np.isfinite(obj[i]) else np.inf))
                open_list = {i: lst for i, lst in new_open.items()}
                if max_open is not None:                            # a tree that keeps growing is given up (it stays NODE_LIMIT with its incumbent and bound)
                    gave_up = [i for i, lst in open_list.items() if len(lst) > max_open]
                    for i in gave_up:
                        del open_list[i]
                    given_up.update(gave_up)
                    stats["given_up"] = len(given_up)
                rstat["parents_left"] = len(open_list)
                if stuck and all(i in stuck for i in open_list) and r + 1 < rounds:
                    pass                                            # (stuck nodes are simply retried with the next round's budget)
            stats["unfinished"] = len(set(open_list) | given_up | set(dropped_lb))      # each tree once, whatever kept it from being proven
            return dict(v=v, obj=obj, status=status, lower_bound=lb, nodes=nodes, pivots=pivots, stats=out["stats"], handoff=stats)
        finally:
            self.record_open_nodes(False)
            self.set_opts(max_nodes=keep_nodes)
            if sub_opts and keep_sub:
                self.set_opts(**keep_sub)
            self.set_cutoffs(None)

    def rhs(self, x0, omega, model_idx=None, scenarios=1):
        """h = H_x x_k + H_omega omega + H_5 (row-min over `scenarios` omega columns), original model"""
        d = self.model.dims
        omega = _lib.as_f64(omega)
        batch = int(np.asarray(x0).reshape(-1, d["nx"]).shape[0]) if d["nx"] else int(omega.size // max(1, scenarios * self.nW))
        x0 = _lib.as_f64(x0).reshape(batch, d["nx"]) if d["nx"] else np.zeros((batch, 0))
        omega = omega.reshape(batch, scenarios, self.nW) if self.nW else np.zeros((batch, scenarios, 0))
        mi = np.ascontiguousarray(model_idx, dtype=np.int32) if model_idx is not None else None
        h = np.zeros((batch, self.m))
        check(_lib.load().mld_rhs_batch(self._h, batch, int(scenarios),
                                        mi.ctypes.data_as(C.POINTER(C.c_int32)) if mi is not None else None,
                                        _lib.dptr(x0) if d["nx"] else None, _lib.dptr(omega) if self.nW else None, _lib.dptr(h)))
        return h


def debug_update_shape():
    """diagnostics: the row-block sizes of k_solve's row update (internal entry mld_debug_update_shape; no device needed) -- RB[k - 1] rows a wave takes at
    a time when a chunk of the active sectors has k groups, and the constants of the sector grid"""
    lib = _lib.load()
    lib.mld_debug_update_shape.restype = C.c_int
    lib.mld_debug_update_shape.argtypes = [C.POINTER(C.c_int32)]
    out = (C.c_int32 * 8)()
    check(lib.mld_debug_update_shape(out))
    return dict(RB=[int(out[k]) for k in range(4)], waves=int(out[4]), sectors_per_group=int(out[5]), sector_doubles=int(out[6]), groups_per_chunk=int(out[7]))


def debug_update_rows(D, n, rowr, colc, r, c, second=None, reserved=0):
    """diagnostics: the rows' update of one pivot of k_solve -- or, with second = (rowr2, colc2, r2, c2), of a fused pair -- on the dictionary D (m x ld)
    (internal entry mld_debug_update_rows).  rowr[n + 1] / colc[m]: the staged pivot row and multiplier column of pivot (r, c).  reserved = 0 runs the
    default instantiation, _lib.MLD_DBG_UPDATE_R7 the earlier templates.  Returns (the updated copy of D, the (row, sector) pairs accounted)."""
    lib = _lib.load()
    dp = C.POINTER(C.c_double)
    lib.mld_debug_update_rows.restype = C.c_int
    lib.mld_debug_update_rows.argtypes = [dp, C.c_int, C.c_int, C.c_int, dp, dp, C.c_int, C.c_int, dp, dp, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int64)]
    D = np.array(D, dtype=np.float64, order="C")
    if D.ndim != 2:
        raise ValueError("D must be a matrix (rows x ld)")
    m, ld = D.shape
    rowr, colc = _lib.as_f64(rowr), _lib.as_f64(colc)
    if rowr.size != int(n) + 1 or colc.size != m:
        raise ValueError("rowr needs n + 1 entries and colc one per row")
    r2 = c2 = -1
    rowr2 = colc2 = None
    if second is not None:
        rowr2, colc2, r2, c2 = second
        rowr2, colc2 = _lib.as_f64(rowr2), _lib.as_f64(colc2)
        if rowr2.size != int(n) + 1 or colc2.size != m:
            raise ValueError("rowr2 needs n + 1 entries and colc2 one per row")
    rows = C.c_int64(0)
    check(lib.mld_debug_update_rows(_lib.dptr(D), m, ld, int(n), _lib.dptr(rowr), _lib.dptr(colc), int(r), int(c), _lib.dptr(rowr2), _lib.dptr(colc2),
                                    int(r2), int(c2), int(reserved), C.byref(rows)))
    return D, int(rows.value)
