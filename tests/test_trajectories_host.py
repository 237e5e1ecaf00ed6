"""Host side of the predicted trajectories (mld_predict_batch): the entry point is declared, listed and exported; the shape checks of
GpuProblem.trajectories (made before any C call); the absence of a CPU fallback; the causal structure of the condensed maps that
k_trajectory's skip relies on -- every block the kernel may leave out is exactly zero; and a replay of the kernel's own mask arithmetic
(which groups of four inner indices a block of 16 rows reads in which chunk) against those maps.  No GPU needed."""
import os
import re
import types

import numpy as np
import pytest

import _paths
import _tv
import condense_np as cn
from pyhybridcontrol_amd import gpu, synthetic as syn, _lib
from _traj_shapes import SHAPES, TV_SHAPE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_predict_batch_is_declared_listed_and_exported():
    with open(os.path.join(ROOT, "include", "mldgpu.h")) as f:
        header = f.read()
    assert re.search(r"\bint\s+mld_predict_batch\s*\(\s*mld_problem_t\s*\*\s*,\s*const\s+double\s*\*\s*v\s*,\s*double\s*\*\s*x_out\s*,\s*double\s*\*\s*y_out\s*\)\s*;", header)
    assert "variables.py:246-286" in header                      # declared with the reference lines it replaces
    assert "mld_predict_batch" in _lib.EXPORTS
    assert hasattr(_lib.load(), "mld_predict_batch")
    assert _lib.version().startswith("mldgpu 0.6 ")


def _shell(batch, nx=3, ny=1, nv=11, N=5):
    """a GpuProblem without a handle: what the shape checks read"""
    p = gpu.GpuProblem.__new__(gpu.GpuProblem)
    p.model = types.SimpleNamespace(dims=dict(nx=nx, ny=ny), nv=nv)
    p.N_tilde, p.n, p.batch, p._h = N, N * nv, batch, None
    return p


def test_shape_errors_raise_before_any_c_call():
    p = _shell(4)
    assert p._plan_array(None) is None
    for good in (np.ones(55), np.ones((4, 55)), [[1.0] * 55] * 4):
        a = p._plan_array(good)
        assert a.shape == (4, 55) and a.dtype == np.float64 and a.flags["C_CONTIGUOUS"]
    for bad in (np.ones(54), np.ones((3, 55)), np.ones((4, 54)), np.ones((4, 55, 1)), np.ones((55, 1)), 1.0):
        with pytest.raises(ValueError, match="v has shape"):
            p.trajectories(v=bad)                    # (_h is None: a C call would have raised MldGpuError instead)


def test_no_cpu_fallback_for_the_trajectories():
    """the handle-less shell reaches the C entry with a null problem: without a device that is MLD_ERR_NO_DEVICE, as everywhere; with one
    it is the refusal of a call without a resident batch"""
    expect = "no HIP device" if _lib.device_count() <= 0 else "no batch resident"
    with pytest.raises(gpu.MldGpuError, match=expect):
        _shell(4).trajectories(v=np.ones(55))
    with pytest.raises(gpu.MldGpuError, match=expect):
        _shell(4).trajectories()


def _assert_causal(evo, N, d, what):
    """block (i, j) of Gamma_v / Gamma_omega is exactly zero for j >= i, of L_v / L_omega for j > i -- so every block with j > i, which is what
    k_trajectory skips in both families (one conservative rule), is exactly zero; block 0 of Phi_x is the identity"""
    for name, rows, cols, strict in (("Gamma_v", d["nx"], d["nv"], False), ("Gamma_omega", d["nx"], d["nomega"], False),
                                     ("L_v", d["ny"], d["nv"], True), ("L_omega", d["ny"], d["nomega"], True)):
        M = np.asarray(evo[name])
        assert M.shape == (N * rows, N * cols), (what, name, M.shape)
        if M.size == 0:
            continue
        B = M.reshape(N, rows, N, cols)
        seen = 0
        for i in range(N):
            for j in range(i + (1 if strict else 0), N):
                assert not np.any(B[i, :, j, :]), (what, name, i, j)          # exactly 0.0: not a tolerance
                seen += 1
        assert seen == (N * (N - 1) // 2 if strict else N * (N + 1) // 2)
        assert np.any(M), (what, name)                                        # (the map is not simply empty)
    if d["nx"]:
        assert np.array_equal(np.asarray(evo["Phi_x"])[:d["nx"]], np.eye(d["nx"])), what


@pytest.mark.parametrize("shape", list(SHAPES))
def test_causal_zero_blocks_of_every_shape_the_gpu_test_uses(shape):
    N, dims = SHAPES[shape]
    d = _paths.make_dims(**dims)
    for i in range(3):
        mats = _paths.random_mld(1234 + i, **dims)[0]
        _assert_causal(cn.condense(mats, N), N, d, shape)


def test_causal_zero_blocks_of_time_varying_horizons():
    """the horizon of independent step models the GPU test uses, and one built as tests/_tv.py builds them from a synthetic agent"""
    N, dims = TV_SHAPE
    _assert_causal(cn.condense_tv(_paths.random_horizon(90, N, **dims)[0]), N, _paths.make_dims(**dims), "random horizon")
    wl = syn.make_workload("cfg2", batch=1)
    ag = wl["agents"][0]
    N = wl["N_tilde"]
    d = dict(ag["dims"])
    d["nv"] = d["nu"] + d["ndelta"] + d["nz"] + d["nmu"]
    _assert_causal(cn.condense_tv(_tv.step_models(ag["mats"], N, seed=3)), N, d, "_tv.step_models")
    _assert_causal(cn.condense(ag["mats"], N), N, d, "cfg2")


# ---- replay of k_trajectory's skip mask (csrc/trajectory.inc: imax, ga / gc, the chunk offset g0; csrc/mfma.inc: ig_bits, IG_KC = 256), restated line by line -------
TJ_KC, TJ_KS = 256, 64


def _tj_bits(lo, hi):
    lo, hi = max(lo, 0), min(hi, TJ_KS)
    return 0 if hi <= lo else (((1 << (hi - lo)) - 1) << lo) & ((1 << 64) - 1)


def _replay_mask(evo, N, d, r_begin, r_end):
    """every element of the stacked maps [Gamma_v Phi_x Gamma_w ; L_v L_x L_w] in rows r_begin .. r_end that the kernel does NOT stage or
    multiply must be exactly zero.  Returns (groups multiplied, groups in all, (row block, chunk) passes made, passes in all)."""
    nxs, nys, nv, nw = d["nx"], d["ny"], d["nv"], d["nomega"]
    NX, NY, n, nx, nW = N * nxs, N * nys, N * nv, nxs, N * nw
    K = n + nx + nW
    M = np.zeros((NX + NY, K))
    if NX:
        M[:NX] = np.hstack([evo["Gamma_v"], evo["Phi_x"], evo["Gamma_omega"]])
    if NY:
        M[NX:] = np.hstack([evo["L_v"], evo["L_x"], evo["L_omega"]])
    seen = np.zeros_like(M)
    used = tot = passes = all_passes = 0
    kc0 = 0
    while kc0 < K or kc0 == 0:
        ks, g0 = (min(TJ_KC, K - kc0) + 3) >> 2, kc0 >> 2
        for rb in range(r_begin, r_end, 16):
            last = min(rb + 15, r_end - 1)
            imax = 0
            if rb < NX:
                imax = min(last, NX - 1) // nxs
            if last >= NX:
                imax = max(imax, (last - NX) // nys)
            ga, gc = (min(n, (imax + 1) * nv) + 3) >> 2, (n + nx + min(nW, (imax + 1) * nw) + 3) >> 2
            need = (_tj_bits(-g0, ga - g0) | _tj_bits((n >> 2) - g0, gc - g0)) & _tj_bits(0, ks)
            tot += ks; all_passes += 1
            if not need and kc0 > 0:
                continue
            passes += 1
            for s in range(TJ_KS):
                if need >> s & 1:
                    used += 1
                    k0 = kc0 + 4 * s
                    seen[rb:last + 1, k0:min(k0 + 4, K)] = M[rb:last + 1, k0:min(k0 + 4, K)]
        kc0 += TJ_KC
    assert np.array_equal(seen[r_begin:r_end], M[r_begin:r_end]), "a skipped group holds a non-zero"
    return used, tot, passes, all_passes


def _replay_all_row_ranges(evo, N, d):
    NX, NY = N * d["nx"], N * d["ny"]
    out = _replay_mask(evo, N, d, 0, NX + NY)
    if NX:
        _replay_mask(evo, N, d, 0, NX)              # x_out only
    if NY:
        _replay_mask(evo, N, d, NX, NX + NY)        # y_out only: the row blocks start at NX
    return out


@pytest.mark.parametrize("shape", list(SHAPES))
def test_skip_mask_replay_on_every_shape(shape):
    N, dims = SHAPES[shape]
    d = _paths.make_dims(**dims)
    used, tot, _, _ = _replay_all_row_ranges(cn.condense(_paths.random_mld(5, **dims)[0], N), N, d)
    print("%s: %d of %d groups multiplied" % (shape, used, tot))
    assert used <= tot and (N < 8 or used < tot)          # (and on the longer horizons something IS skipped)


def test_skip_mask_replay_time_varying_and_cfg3():
    N, dims = TV_SHAPE
    _replay_all_row_ranges(cn.condense_tv(_paths.random_horizon(90, N, **dims)[0]), N, _paths.make_dims(**dims))
    wl = syn.make_workload("cfg3", batch=1)
    ag = wl["agents"][0]
    d = dict(ag["dims"])
    d["nv"] = d["nu"] + d["ndelta"] + d["nz"] + d["nmu"]
    used, tot, passes, all_passes = _replay_all_row_ranges(cn.condense(ag["mats"], wl["N_tilde"]), wl["N_tilde"], d)
    print("cfg3 / cfg4 shape: %d of %d groups, %d of %d (row block, chunk) passes" % (used, tot, passes, all_passes))
    assert (passes, all_passes) == (37, 52) and abs(used / tot - 0.62) < 0.01          # the figures DESIGN section 3 / 6 quote
