"""Resident disturbance profiles on the device (mld_upload_profiles, mld_forecast_from_profiles, mld_constraint_blocks_from_profiles,
mld_evaluate_batch_profiles, mld_download_constraint_blocks; kernel k_profile_windows): a window of the flat library is gathered where the reference
slices a time series (examples/.../modelling/micro_grid_agents.py:206-298).  Checked against pyhybridcontrol_amd.profiles.windows, the numpy statement
of the window rule (itself checked against the literal rule and the reference's slicing in tests/test_profiles_host.py): the forecast, the constraint
blocks and their read-back, the same solve and the same audit as with uploaded columns, a closed loop of three steps, the states of the handle and
every refusal.

Everything here moves doubles without arithmetic: every comparison is np.array_equal, never a tolerance."""
import ctypes as C

import numpy as np
import pytest

import _paths
from pyhybridcontrol_amd import gpu, profiles, _lib
from _traj_shapes import SHAPES, TV_SHAPE
from test_gpu_trajectories import _problem, _half_without_a_plan
from test_gpu_blocks import _draw_profiles

pytestmark = pytest.mark.gpu

SHAPE_NAMES = ["below16", "odd3", "nx0", "nx17", "tv"]          # odd3: N_tilde * nomega = 273, odd; tv: a time-varying handle
KEYS = ("v", "obj", "status", "lower_bound", "nodes", "pivots")
LP = C.POINTER(C.c_int64)


def _handle(shape, seed):
    """two models (horizons) of the shape behind one problem without a cost: (model, problem, N, dims)"""
    if shape == "tv":
        N, dims = TV_SHAPE
        mats = [_paths.random_horizon(seed + i, N, **dims)[0] for i in range(2)]
    else:
        N, dims = SHAPES[shape]
        mats = [_paths.random_mld(seed * 1000 + i, **dims)[0] for i in range(2)]
    d = _paths.make_dims(**dims)
    m = gpu.GpuModel(mats, d, time_varying=shape == "tv")
    return m, gpu.GpuProblem(m, N - 1, N, None), N, d


def _widths(nomega):
    """one group; nomega groups of width 1; an uneven split"""
    return [(nomega,), (1,) * nomega, (1, nomega - 1) if nomega > 1 else (1,)]


def _lib_len(N, gw):
    return (8 + N) * max(gw) + 50          # short: windows of different instances overlap


def _draw(rng, lead, gw, N, smax, L):
    """starts of shape lead + (n_groups,) that are valid up to step smax: row 0 is 0, the last row is the exact last valid offset of every group
    (s + (smax + N) w == L), rows 1 and 2 are the same"""
    hi = np.array([L - (smax + N) * w for w in gw])
    assert hi.min() >= 0
    R = int(np.prod(lead))
    s = np.stack([rng.integers(0, h + 1, size=R) for h in hi], axis=-1)
    if R > 1:
        s[0] = 0
    s[R - 1] = hi
    if R > 3:
        s[2] = s[1]
    return s.reshape(tuple(lead) + (len(gw),)).astype(np.int64)


def _inputs(rng, B, d, N):
    return rng.standard_normal((B, d["nx"])), rng.standard_normal((B, N * d["nomega"]))


def _same_blocks(a, b):
    assert np.array_equal(a["omega_cols"], b["omega_cols"]) and np.array_equal(a["col_rows"], b["col_rows"])
    assert (a["x_cols"] is None) == (b["x_cols"] is None) and (a["x_cols"] is None or np.array_equal(a["x_cols"], b["x_cols"]))


# ---- 1. the forecast --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPE_NAMES)
def test_forecast_is_the_window(shape):
    m, p, N, d = _handle(shape, 4100)
    rng = np.random.default_rng(4101 + len(shape))
    try:
        for gw in _widths(d["nomega"]):
            L = _lib_len(N, gw)
            lib = rng.standard_normal(L)
            p.upload_profiles(lib, None if len(gw) == 1 else gw)
            for B in (1, 3, 65, 257):                              # 257 instances: more than one 256-thread block of rows
                x0, om = _inputs(rng, B, d, N)
                p.upload(x0, om, (np.arange(B) % 2).astype(np.int32) if B == 65 else None)
                for step in (0, 1, 7):
                    start = _draw(rng, (B,), gw, N, step + 1, L)
                    p.forecast_from_profiles(start, step)
                    gx, gom = p.inputs()
                    assert np.array_equal(gom, profiles.windows(lib, start, step, N, gw)), (gw, B, step)
                    assert np.array_equal(gx, x0)
                    p.forecast_from_profiles(None, step + 1)       # the resident starts, one step on: B > 1 has a window that ends at the library's end
                    gx, gom = p.inputs()
                    assert np.array_equal(gom, profiles.windows(lib, start, step + 1, N, gw)), (gw, B, step)
                    assert np.array_equal(gx, x0)
                one = _draw(rng, (1,), gw, N, 0, L)[0]             # the same start for every instance: (n_groups,) is broadcast over the batch
                p.forecast_from_profiles(one, 0)
                assert np.array_equal(p.inputs()[1], np.tile(profiles.windows(lib, one, 0, N, gw), (B, 1)))
    finally:
        p.close(); m.close()


# ---- 2. the constraint blocks and their read-back ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPE_NAMES)
def test_blocks_are_the_windows_and_read_back(shape):
    m, p, N, d = _handle(shape, 4200)
    rng = np.random.default_rng(4201 + len(shape))
    nx, m0 = d["nx"], N * d["nc"]
    try:
        cases = [(1, 20, 0), (3, 3, 1), (65, 1, 7), (257, 20, 1), (65, 3, 0)]
        for i, (B, Cn, step) in enumerate(cases):
            gw = _widths(d["nomega"])[i % 3]
            L = _lib_len(N, gw)
            lib = rng.standard_normal(L)
            p.upload_profiles(lib, None if len(gw) == 1 else gw)
            x0, om = _inputs(rng, B, d, N)
            p.upload(x0, om, (np.arange(B) % 2).astype(np.int32) if i == 4 else None)
            assert p.constraint_blocks()["omega_cols"].shape == (B, 0, N * d["nomega"])
            start = _draw(rng, (B, Cn), gw, N, step + 1, L)
            ref = profiles.windows(lib, start, step, N, gw)
            assert ref.shape == (B, Cn, N * d["nomega"])
            # without col_rows / x_cols: every column covers all rows and uses the instance's x0
            assert p.constraint_blocks_from_profiles(start, step) == Cn
            got = p.constraint_blocks()
            assert np.array_equal(got["omega_cols"], ref), (B, Cn, step, gw)
            assert np.array_equal(got["col_rows"], np.full(Cn, m0)) and got["x_cols"] is None
            # with both; the resident starts one step on
            cr = rng.integers(0, m0 + 1, size=Cn).astype(np.int32)
            xc = rng.standard_normal((B, Cn, nx)) if nx else None
            p.constraint_blocks_from_profiles(start, step, col_rows=cr, x_cols=xc)
            _same_blocks(p.constraint_blocks(), dict(omega_cols=ref, col_rows=cr, x_cols=xc))
            p.constraint_blocks_from_profiles(None, step + 1, col_rows=cr)
            _same_blocks(p.constraint_blocks(), dict(omega_cols=profiles.windows(lib, start, step + 1, N, gw), col_rows=cr, x_cols=None))
            assert np.array_equal(p.inputs()[1], om)             # the forecast is not the blocks' business
            # (n_cols, n_groups) is broadcast over the batch
            p.constraint_blocks_from_profiles(start[B - 1], step)
            assert np.array_equal(p.constraint_blocks()["omega_cols"], np.tile(ref[B - 1], (B, 1, 1)))
            # uploaded blocks come back as uploaded; n_cols = 0 clears
            up, xu = rng.standard_normal((B, 2, N * d["nomega"])), rng.standard_normal((B, 2, nx)) if nx else None
            p.upload_constraint_blocks(up, [m0, 1], xu)
            _same_blocks(p.constraint_blocks(), dict(omega_cols=up, col_rows=np.array([m0, 1], np.int32), x_cols=xu))
            assert _lib.load().mld_constraint_blocks_from_profiles(p._h, 0, None, 0, None, None) == 0
            assert p.constraint_blocks()["omega_cols"].shape[1] == 0
    finally:
        p.close(); m.close()


# ---- a cfg2 batch whose disturbance data lives in a library -----------------------------------------------------------------------------------
def _cfg2_library(wl, ag, B, Cn, rng, extra=8):
    """per instance one net-load series (width 1) and Cn hot-water-draw series (width n_h), N_tilde + extra steps each: the profiles of
    tests/test_gpu_blocks.py::_draw_profiles -- the draws scaled per column, the load kept, because the tie rows encode z = max(0, y) exactly --
    continued past the horizon with rescaled copies of their first steps.  Returns (lib, group widths, forecast starts (B, 2), column starts (B, Cn, 2))."""
    N, n_h = wl["N_tilde"], ag["dims"]["nx"]
    series, fstart, cstart = [], np.zeros((B, 2), np.int64), np.zeros((B, Cn, 2), np.int64)
    for b in range(B):
        cols = _draw_profiles(dict(ag, omega=ag["omega"][b:b + 1]), wl, rng, Cn).reshape(Cn, N, n_h + 1) if Cn else []
        own = ag["omega"][b].reshape(N, n_h + 1)
        tail = rng.uniform(0.7, 1.3, size=(extra, 1))
        series.append(np.vstack([own[:, n_h:], own[:extra, n_h:] * tail]))                      # the load, shared by all windows of the instance
        series.append(np.vstack([own[:, :n_h], own[:extra, :n_h] * tail]))                      # the instance's own draws: its forecast
        for c in range(Cn):
            series.append(np.vstack([cols[c][:, :n_h], cols[c][:extra, :n_h] * tail]))
    lib, base = profiles.pack(series)
    base = base.reshape(B, 2 + Cn)
    fstart[:, 0], fstart[:, 1] = base[:, 1], base[:, 0]
    cstart[:, :, 0], cstart[:, :, 1] = base[:, 2:], base[:, :1]
    return lib, (n_h, 1), fstart, cstart


def _same_results(a, b, what):
    for k in KEYS:
        assert np.array_equal(a[k], b[k], equal_nan=True), (what, k)


# ---- 3. the same solve --------------------------------------------------------------------------------------------------------------------------
def test_solve_is_the_same_as_with_uploaded_columns():
    B, Cn = 65, 3
    wl, ag, d, m, p = _problem("cfg2", B, gap_rel=0.0, max_nodes=2000)
    N, m0, nc = wl["N_tilde"], wl["N_tilde"] * d["nc"], d["nc"]
    rng = np.random.default_rng(4300)
    lib, gw, fstart, cstart = _cfg2_library(wl, ag, B, Cn, rng)
    x0 = ag["x0"][:B]
    try:
        p.upload_profiles(lib, gw)
        xc = x0[:, None, :] + 0.01 * rng.standard_normal((B, Cn, d["nx"]))
        variants = [("plain", 0, None, None, True), ("reduced col_rows", 2, np.array([m0, 8 * nc, 3 * nc], np.int32), None, True),
                    ("x_cols", 1, None, xc, True), ("no standard block", 3, np.array([m0, m0, 5 * nc], np.int32), None, False)]
        n_opt = 0
        for what, step, cr, xcv, std in variants:
            om_w = profiles.windows(lib, fstart, step, N, gw)
            cols_w = profiles.windows(lib, cstart, step, N, gw)
            if step == 0:
                assert np.array_equal(om_w, ag["omega"][:B])      # the library holds the workload's own forecast
            p.set_std_block(std)
            p.upload(x0, ag["omega"][:B])
            p.forecast_from_profiles(fstart, step)
            p.constraint_blocks_from_profiles(cstart, step, col_rows=cr, x_cols=xcv)
            p.solve_resident()
            a = p.download()
            p.upload(x0, om_w)
            p.upload_constraint_blocks(cols_w, cr, xcv)
            p.solve_resident()
            b = p.download()
            _same_results(a, b, what)
            print("%s: statuses %s" % (what, np.bincount(a["status"], minlength=5).tolist()))
            n_opt += int(np.isfinite(a["obj"]).sum())
            # the convenience call
            c = p.solve(x0, om_w, col_start=cstart, col_step=step, col_rows=cr, x_cols=xcv)
            _same_results(a, c, what + " solve()")
        assert n_opt >= B                                          # plans were found (the comparison is not one of failures only)
        p.set_std_block(True)
        # once with the in-kernel hand-off: the items read their source instance's blocks
        ho = dict(first_nodes=3, sub_nodes=12, max_gen=8, max_children=64, max_tree=100000, room_factor=64.0)
        a = p.solve_handoff_device(x0, ag["omega"][:B], col_start=cstart, col_step=0, **ho)
        b = p.solve_handoff_device(x0, ag["omega"][:B], omega_cols=profiles.windows(lib, cstart, 0, N, gw), **ho)
        _same_results(a, b, "hand-off")
        assert a["handoff"]["items"] == b["handoff"]["items"]
    finally:
        p.close(); m.close()


# ---- 4. the same audit --------------------------------------------------------------------------------------------------------------------------
def _same_audit(a, b, what):
    assert set(a) == set(b) == {"obj", "constr_vio", "constr_row", "int_vio", "bound_vio"}
    for k in a:
        assert a[k].shape == b[k].shape and np.array_equal(a[k], b[k], equal_nan=True), (what, k)


def test_audit_of_the_resident_plans_with_instances_without_a_plan():
    B, Cn = 16, 3
    wl, ag, d, m, p = _problem("cfg2", B, gap_rel=0.0, max_nodes=100000)
    N, m0 = wl["N_tilde"], wl["N_tilde"] * d["nc"]
    rng = np.random.default_rng(4400)
    lib, gw, fstart, cstart = _cfg2_library(wl, ag, B, Cn, rng)
    try:
        p.upload_profiles(lib, gw)
        masked, out = _half_without_a_plan(p, ag, B)
        p.constraint_blocks_from_profiles(cstart[:, :2], 1, col_rows=[m0, 7])      # resident blocks and starts the call must neither use nor change
        before = p.constraint_blocks()
        for step, cr in ((0, None), (2, np.array([m0, 0, 40], np.int32))):
            a = p.evaluate_profiles(cstart, step, col_rows=cr)
            b = p.evaluate(omega_cols=profiles.windows(lib, cstart, step, N, gw), col_rows=cr)
            _same_audit(a, b, "v=None step %d" % step)
            assert np.all(np.isnan(a["constr_vio"][masked])) and np.all(np.isfinite(a["constr_vio"][~masked][:, 0])) and np.all(a["constr_row"][masked] == -1)
        _same_blocks(p.constraint_blocks(), before)
        assert p.constraint_blocks_from_profiles(None, 2) == 2     # the resident starts are still those of the two columns
        assert np.array_equal(p.constraint_blocks()["omega_cols"], profiles.windows(lib, cstart[:, :2], 2, N, gw))
    finally:
        p.close(); m.close()


@pytest.mark.parametrize("shape,B,Cn", [("odd3", 257, 480), ("tv", 65, 3), ("nx0", 3, 20)])
def test_audit_of_the_callers_plans(shape, B, Cn):
    """caller's v on two interleaved models.  odd3 with 257 instances and 480 columns: a column is 8 * 257 * 273 = 561 288 bytes, so a slice of 256 MB
    holds 478 of them -- the call takes two slices (478 + 2 columns; the second has another leading dimension) for both sources."""
    m, p, N, d = _handle(shape, 4500)
    rng = np.random.default_rng(4501 + B)
    nx, m0 = d["nx"], N * d["nc"]
    if shape == "odd3":
        assert Cn > (256 << 20) // (8 * B * N * d["nomega"]) >= 1
    try:
        gw = _widths(d["nomega"])[2]
        L = _lib_len(N, gw)
        lib = rng.standard_normal(L)
        p.upload_profiles(lib, gw)
        x0, om = _inputs(rng, B, d, N)
        p.upload(x0, om, (np.arange(B) % 2).astype(np.int32))
        v = rng.standard_normal((B, p.n))
        start = _draw(rng, (B, Cn), gw, N, 1, L)
        cr = rng.integers(0, m0 + 1, size=Cn).astype(np.int32)
        xc = rng.standard_normal((B, Cn, nx)) if nx and shape != "odd3" else None
        held = rng.standard_normal((B, 1, N * d["nomega"]))
        p.upload_constraint_blocks(held)
        a = p.evaluate_profiles(start, 1, v=v, col_rows=cr, x_cols=xc)
        b = p.evaluate(v=v, omega_cols=profiles.windows(lib, start, 1, N, gw), col_rows=cr, x_cols=xc)
        _same_audit(a, b, shape)
        assert a["constr_vio"].shape == (B, Cn) and np.all(np.isfinite(a["constr_vio"][:, cr > 0])) and np.all(a["constr_row"][:, cr == 0] == -1)
        assert np.array_equal(p.constraint_blocks()["omega_cols"], held)
    finally:
        p.close(); m.close()


# ---- 5. closed loop -----------------------------------------------------------------------------------------------------------------------------
def test_closed_loop_of_three_steps():
    """handle A slides every instance's window along its own series on the device; handle B gets the numpy window uploaded and A's MIP start"""
    B = 65
    wl, ag, d, m, pa = _problem("cfg2", B, gap_rel=0.0, max_nodes=2000)
    from pyhybridcontrol_amd import host
    pb = gpu.GpuProblem(m, wl["N_p"], wl["N_tilde"], host.cost_from_atoms(ag["atoms"], d, wl["N_p"], wl["N_tilde"]), gap_rel=0.0, max_nodes=2000)
    N = wl["N_tilde"]
    rng = np.random.default_rng(4600)
    lib, gw, fstart, _ = _cfg2_library(wl, ag, B, 0, rng)
    x0, om = ag["x0"][:B], ag["omega"][:B]
    try:
        pa.upload_profiles(lib, gw)
        pa.upload(x0, om)
        pa.forecast_from_profiles(fstart, 0)
        pb.upload(x0, om)
        moved = 0
        for k in range(3):
            xa, wa = pa.inputs()
            xb, wb = pb.inputs()
            assert np.array_equal(xa, xb) and np.array_equal(wa, wb), k
            assert np.array_equal(wa, profiles.windows(lib, fstart, k, N, gw)), k
            pa.solve_resident(); pb.solve_resident()
            oa = pa.download()
            _same_results(oa, pb.download(), "step %d" % k)
            assert (np.isin(oa["status"], (0, 2)) & np.isfinite(oa["obj"])).sum() >= B - 2
            skipped = pa.advance()
            pa.warm_start_from_previous(1)
            ws = pa.debug_warm_start()
            pa.forecast_from_profiles(None, k + 1)
            after = pa.debug_warm_start()
            assert ws is not None and after is not None and np.array_equal(ws, after), k      # the start survives the new forecast
            assert pb.advance() == skipped
            xb, _ = pb.inputs()
            pb.upload(xb, profiles.windows(lib, fstart, k + 1, N, gw))
            pb.set_warm_start(ws)
            moved += int(not np.array_equal(xb, xa))
        xa, wa = pa.inputs()
        xb, wb = pb.inputs()
        assert np.array_equal(xa, xb) and np.array_equal(wa, wb) and moved == 3
        pa.solve_resident(); pb.solve_resident()
        _same_results(pa.download(), pb.download(), "after the loop")
    finally:
        pa.close(); pb.close(); m.close()


# ---- 6. the states of the handle ----------------------------------------------------------------------------------------------------------------
def test_handle_states():
    B = 8
    wl, ag, d, m, p = _problem("cfg2", B, gap_rel=1e-4, max_nodes=2000)
    N = wl["N_tilde"]
    rng = np.random.default_rng(4700)
    lib, gw, fstart, cstart = _cfg2_library(wl, ag, B, 2, rng)
    x0, om = ag["x0"][:B], ag["omega"][:B]
    try:
        p.upload_profiles(lib, gw)
        p.upload(x0, om)
        p.solve_resident()
        p.constraint_blocks_from_profiles(cstart, 0)
        p.set_warm_start(np.zeros((B, p.n_bin), np.uint8))
        assert p.constraint_blocks()["omega_cols"].shape[1] == 2 and p.debug_warm_start() is not None
        p.trajectories()
        # outside the advanced state the call is new inputs: blocks, start and solved state go
        p.forecast_from_profiles(fstart, 1)
        assert p.constraint_blocks()["omega_cols"].shape[1] == 0 and p.debug_warm_start() is None
        with pytest.raises(gpu.MldGpuError, match="not been solved"):
            p.trajectories()
        # the library survives an upload at another batch size, the resident starts do not
        p.constraint_blocks_from_profiles(cstart, 0)
        p.upload(x0[:5], om[:5])
        with pytest.raises(gpu.MldGpuError, match="error -1.*no starts of this batch"):
            p.forecast_from_profiles(None, 1)
        with pytest.raises(gpu.MldGpuError, match="error -1.*no column starts of this batch"):
            p.constraint_blocks_from_profiles(None, 1)
        assert np.array_equal(p.inputs()[1], om[:5])
        p.forecast_from_profiles(fstart[:5], 2)
        assert np.array_equal(p.inputs()[1], profiles.windows(lib, fstart[:5], 2, N, gw))
        p.upload(np.tile(x0, (3, 1)), np.tile(om, (3, 1)))         # a larger batch: the batch buffers are laid out anew
        p.constraint_blocks_from_profiles(np.tile(cstart, (3, 1, 1)), 3)
        assert np.array_equal(p.constraint_blocks()["omega_cols"], np.tile(profiles.windows(lib, cstart, 3, N, gw), (3, 1, 1)))
        # a second library invalidates the starts
        p.forecast_from_profiles(np.tile(fstart, (3, 1)), 0)
        p.upload_profiles(lib[::-1].copy(), gw)
        with pytest.raises(gpu.MldGpuError, match="error -1.*no starts of this batch"):
            p.forecast_from_profiles(None, 0)
        with pytest.raises(gpu.MldGpuError, match="error -1.*no column starts of this batch"):
            p.constraint_blocks_from_profiles(None, 0)
        p.forecast_from_profiles(np.tile(fstart, (3, 1)), 0)
        assert np.array_equal(p.inputs()[1], np.tile(profiles.windows(lib[::-1], fstart, 0, N, gw), (3, 1)))
        # length 0 frees it: every consumer is refused
        p.upload_profiles(np.zeros(0))
        w = p.inputs()[1]
        for call in (lambda: p.forecast_from_profiles(np.tile(fstart, (3, 1)), 0), lambda: p.forecast_from_profiles(None, 0),
                     lambda: p.constraint_blocks_from_profiles(np.tile(cstart, (3, 1, 1)), 0),
                     lambda: p.evaluate_profiles(np.tile(cstart, (3, 1, 1)), 0, v=np.zeros(p.n))):
            with pytest.raises(gpu.MldGpuError, match="error -1.*no profile library resident"):
                call()
        assert np.array_equal(p.inputs()[1], w)
    finally:
        p.close(); m.close()


# ---- 7. refusals --------------------------------------------------------------------------------------------------------------------------------
def _refused(rc, text):
    err = _lib.load().mld_last_error().decode()
    assert rc == -1 and all(t in err for t in ([text] if isinstance(text, str) else text)), (rc, err)


def test_refusals_change_nothing():
    """host-side checks: none of them launches a kernel"""
    m, p, N, d = _handle("below16", 4800)
    lib_ = _lib.load()
    rng = np.random.default_rng(4801)
    gw = (1, 2)
    B, Cn, L = 6, 3, 200
    lib = rng.standard_normal(L)
    x0, om = _inputs(rng, B, d, N)
    ptr = lambda a: a.ctypes.data_as(LP)
    ev = lambda st, n_cols, step, v: lib_.mld_evaluate_batch_profiles(p._h, _lib.dptr(v), n_cols, ptr(st) if st is not None else None, step, None, None,
                                                                       _lib.dptr(np.zeros(B)), _lib.dptr(np.zeros((B, max(1, n_cols)))), None, None, None)
    v = rng.standard_normal((B, p.n))
    fs, cs = _draw(rng, (B,), gw, N, 2, L), _draw(rng, (B, Cn), gw, N, 2, L)
    try:
        p.upload(x0, om)
        held = rng.standard_normal((B, 2, N * d["nomega"]))
        p.upload_constraint_blocks(held, [3, 9])

        def unchanged():
            gx, gom = p.inputs()
            assert np.array_equal(gx, x0) and np.array_equal(gom, om)
            _same_blocks(p.constraint_blocks(), dict(omega_cols=held, col_rows=np.array([3, 9], np.int32), x_cols=None))

        # no library
        _refused(lib_.mld_forecast_from_profiles(p._h, ptr(fs), 0), "no profile library resident")
        _refused(lib_.mld_constraint_blocks_from_profiles(p._h, Cn, ptr(cs), 0, None, None), "no profile library resident")
        _refused(ev(cs, Cn, 0, v), "no profile library resident")
        unchanged()
        # a library that cannot be: nothing becomes resident
        w3 = np.array([1, 1], np.int32)
        _refused(lib_.mld_upload_profiles(p._h, L, _lib.dptr(lib), 2, w3.ctypes.data_as(C.POINTER(C.c_int32))), "sum to 2, not to nomega = 3")
        _refused(lib_.mld_upload_profiles(p._h, -1, _lib.dptr(lib), 0, None), "lib_len = -1")
        _refused(lib_.mld_upload_profiles(p._h, L, None, 0, None), "without a library")
        _refused(lib_.mld_forecast_from_profiles(p._h, ptr(fs), 0), "no profile library resident")
        p.upload_profiles(lib, gw)
        # NULL before any starts are resident
        _refused(lib_.mld_forecast_from_profiles(p._h, None, 0), "no starts of this batch")
        _refused(lib_.mld_constraint_blocks_from_profiles(p._h, Cn, None, 0, None, None), "no column starts of this batch")
        _refused(ev(None, Cn, 0, v), "start == NULL")
        _refused(ev(cs, 0, 0, v), "at least one")
        # a negative start, and one element past the last valid one: instance, column and group are named
        for bad, where in ((-1, (4, 1, 0)), (L - (2 + N) * 2 + 1, (5, 2, 1))):
            b_, c_, g_ = where
            f2, c2 = fs.copy(), cs.copy()
            f2[b_, g_] = bad
            c2[b_, c_, g_] = bad
            _refused(lib_.mld_forecast_from_profiles(p._h, ptr(f2), 2), ["start %d of instance %d, column 0, group %d" % (bad, b_, g_), "leaves the library"])
            names = ["start %d of instance %d, column %d, group %d" % (bad, b_, c_, g_), "leaves the library"]
            _refused(lib_.mld_constraint_blocks_from_profiles(p._h, Cn, ptr(c2), 2, None, None), names)
            _refused(ev(c2, Cn, 2, v), names)
        # step < 0
        _refused(lib_.mld_forecast_from_profiles(p._h, ptr(fs), -1), "step = -1")
        _refused(lib_.mld_constraint_blocks_from_profiles(p._h, Cn, ptr(cs), -1, None, None), "step = -1")
        _refused(ev(cs, Cn, -1, v), "step = -1")
        # a col_rows entry outside [0, N_tilde * nc]
        bad_rows = np.array([0, N * d["nc"] + 1, 0], np.int32)
        _refused(lib_.mld_constraint_blocks_from_profiles(p._h, Cn, ptr(cs), 0, bad_rows.ctypes.data_as(C.POINTER(C.c_int32)), None), "col_rows[1]")
        unchanged()
        # resident starts (last row: the exact last valid offset at step 2), then a step that pushes the remembered maximum past the end
        p2 = gpu.GpuProblem(m, N - 1, N, None)
        try:
            p2.upload(x0, om)
            p2.upload_profiles(lib, gw)
            p2.forecast_from_profiles(fs, 2)
            p2.constraint_blocks_from_profiles(cs, 2)
            w2, blocks2 = p2.inputs()[1], p2.constraint_blocks()
            assert np.array_equal(w2, profiles.windows(lib, fs, 2, N, gw))
            _refused(lib_.mld_forecast_from_profiles(p2._h, None, 3), ["step 3 moves the largest resident start of group", "past the end"])
            _refused(lib_.mld_constraint_blocks_from_profiles(p2._h, Cn, None, 3, None, None), ["step 3 moves the largest resident start of group", "past the end"])
            _refused(lib_.mld_forecast_from_profiles(p2._h, None, -1), "step = -1")
            # n_cols changed with start == NULL
            _refused(lib_.mld_constraint_blocks_from_profiles(p2._h, Cn - 1, None, 0, None, None), "resident starts are those of 3 columns")
            assert np.array_equal(p2.inputs()[1], w2)
            _same_blocks(p2.constraint_blocks(), blocks2)
            p2.forecast_from_profiles(None, 1); p2.constraint_blocks_from_profiles(None, 0)      # and the handle goes on working
            assert np.array_equal(p2.inputs()[1], profiles.windows(lib, fs, 1, N, gw))
            assert np.array_equal(p2.constraint_blocks()["omega_cols"], profiles.windows(lib, cs, 0, N, gw))
        finally:
            p2.close()
    finally:
        p.close(); m.close()


def test_no_disturbance_no_library():
    N, dims = SHAPES["nw0"]
    d = _paths.make_dims(**dims)
    m = gpu.GpuModel([_paths.random_mld(4900, **dims)[0]], d)
    p = gpu.GpuProblem(m, N - 1, N, None)
    try:
        p.upload(np.zeros((2, d["nx"])), None)
        lib = np.zeros(10)
        _refused(_lib.load().mld_upload_profiles(p._h, 10, _lib.dptr(lib), 0, None), "nomega = 0")
        _refused(_lib.load().mld_forecast_from_profiles(p._h, None, 0), "no profile library resident")
    finally:
        p.close(); m.close()


def test_refused_between_launch_and_finish():
    B = 8
    wl, ag, d, m, p = _problem("cfg2", B, gap_rel=1e-4, max_nodes=2000)
    N = wl["N_tilde"]
    lib, gw, fstart, cstart = _cfg2_library(wl, ag, B, 2, np.random.default_rng(4950))
    lib_ = _lib.load()
    ptr = lambda a: a.ctypes.data_as(LP)
    try:
        p.upload_profiles(lib, gw)
        p.upload(ag["x0"][:B], ag["omega"][:B])
        p.constraint_blocks_from_profiles(cstart, 0)
        p.launch()
        gwa = np.array(gw, np.int32)
        _refused(lib_.mld_upload_profiles(p._h, lib.size, _lib.dptr(lib), 2, gwa.ctypes.data_as(C.POINTER(C.c_int32))), "not been finished")
        _refused(lib_.mld_forecast_from_profiles(p._h, ptr(fstart), 1), "not been finished")
        _refused(lib_.mld_constraint_blocks_from_profiles(p._h, 2, ptr(cstart), 1, None, None), "not been finished")
        _refused(lib_.mld_evaluate_batch_profiles(p._h, None, 2, ptr(cstart), 1, None, None, _lib.dptr(np.zeros(B)), None, None, None, None), "not been finished")
        _refused(lib_.mld_download_constraint_blocks(p._h, None, None, None, None), "not been finished")
        p.finish()
        assert np.array_equal(p.inputs()[1], ag["omega"][:B])
        assert np.array_equal(p.constraint_blocks()["omega_cols"], profiles.windows(lib, cstart, 0, N, gw))
        a = p.evaluate_profiles(cstart, 1)                         # the finished solve's plans under the columns one step on
        _same_audit(a, p.evaluate(omega_cols=profiles.windows(lib, cstart, 1, N, gw)), "after finish")
    finally:
        p.close(); m.close()
