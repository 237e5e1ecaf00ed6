"""CPU tests of the plant step with the whole step-0 slice (mld_sim_step_batch / GpuProblem.sim_step, pyhybridcontrol_amd/simlog.py): the numpy
statement `simlog.lsim_k_batch` against the REFERENCE's MldModel.lsim_k(x_k, v_k=, omega_k=) recorded in tests/golden/lsim_vk_ref.npz (written by
scripts/gen_lsim_golden.py) and against the package's own MldModel.lsim_k, the MldSimLog bridge, and the C ABI's declarations."""
import os
import re
import subprocess

import numpy as np
import pytest

import pyhybridcontrol_amd as phc
from pyhybridcontrol_amd import _lib, simlog

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIM_NAMES = ("nx", "nu", "ndelta", "nz", "nmu", "nomega", "ny", "nc")
MAT_NAMES = _lib.MAT_NAMES
NEW = ("mld_sim_log_begin", "mld_sim_log_count", "mld_sim_step_batch", "mld_download_sim_log")


@pytest.fixture(scope="module")
def golden():
    g = np.load(os.path.join(ROOT, "tests", "golden", "lsim_vk_ref.npz"))
    models = []
    for k in range(int(g["n_models"])):
        dims = dict(zip(DIM_NAMES, (int(t) for t in g["m%d_dims" % k])))
        mats = {n: g["m%d_%s" % (k, n)] for n in MAT_NAMES}
        rec = {f: g["m%d_%s" % (k, f)] for f in ("x_k1", "x", "u", "delta", "z", "mu", "v", "y", "omega", "cons", "resid")}
        models.append((dims, mats, rec))
    return models


def test_the_fixture_covers_what_it_claims(golden):
    assert any(d["nmu"] > 0 for d, _, _ in golden) and any(d["ny"] == 0 for d, _, _ in golden) and any(d["nc"] == 0 for d, _, _ in golden)
    seen = set()
    for d, _, rec in golden:
        assert rec["x"].shape[0] == 8 and rec["v"].shape == (8, d["nu"] + d["ndelta"] + d["nz"] + d["nmu"])
        assert np.array_equal(rec["v"], np.hstack([rec["u"], rec["delta"], rec["z"], rec["mu"]]))
        if d["nc"]:
            assert np.abs(rec["resid"] - 1e-6).min() >= 1e-9          # no truth value within rounding of the threshold
            assert np.array_equal(rec["cons"], rec["resid"] <= 1e-6)
        seen |= set(bool(c) for c in rec["cons"].ravel())
    assert seen == {True, False}


def test_lsim_k_batch_equals_the_reference(golden):
    for k, (d, mats, rec) in enumerate(golden):
        got = simlog.lsim_k_batch([mats], d, None, rec["x"], rec["v"], rec["omega"])
        bound = simlog.sum_bound(d)
        K = d["nx"] + d["nu"] + d["ndelta"] + d["nz"] + d["nmu"] + d["nomega"] + 1
        assert bound == (K + d["ny"]) * 2.0 ** -52
        for name, ref, terms in (("x_k1", rec["x_k1"], got["terms_x"]), ("y", rec["y"], got["terms_y"]), ("resid", rec["resid"], got["terms_r"])):
            err = np.abs(got[name] - ref)
            assert got[name].shape == ref.shape and np.all(err <= bound * terms), (k, name, float((err / np.maximum(terms, 1e-300)).max()), bound)
        assert np.array_equal(got["cons"], rec["cons"]), k
        if d["nc"]:
            assert np.array_equal(got["cons_row"], rec["resid"].argmax(axis=1)) and np.all(np.abs(got["cons_vio"] - rec["resid"].max(axis=1)) <= bound * got["terms_r"].max(axis=1))
        else:
            assert np.all(got["cons_vio"] == -np.inf) and np.all(got["cons_row"] == -1) and got["cons"].shape == (8, 0)


def test_lsim_k_batch_two_models_interleaved_equals_each_alone(golden):
    """model_idx selects the matrices per instance: models 0 and 3 of the fixture share no shape, so two random models of one shape are used"""
    import _paths
    dims = dict(nx=3, nu=2, ndelta=1, nz=1, nmu=1, nomega=2, ny=2, nc=4)
    ma, d, _ = _paths.random_mld(61, **dims)
    mb, _, _ = _paths.random_mld(62, **dims)
    rng = np.random.default_rng(63)
    x, v, w = rng.standard_normal((6, 3)), rng.standard_normal((6, 5)), rng.standard_normal((6, 2))
    midx = np.array([0, 1, 1, 0, 1, 0])
    both = simlog.lsim_k_batch([ma, mb], d, midx, x, v, w)
    for k, mats in enumerate((ma, mb)):
        sel = midx == k
        one = simlog.lsim_k_batch([mats], d, None, x[sel], v[sel], w[sel])
        for name in ("x_k1", "y", "resid", "cons", "cons_vio", "cons_row"):
            assert np.array_equal(both[name][sel], one[name]), (k, name)
    assert not np.array_equal(both["x_k1"], simlog.lsim_k_batch([ma], d, None, x, v, w)["x_k1"])


def test_lsim_k_batch_equals_the_package_model_instance_by_instance(golden):
    for k, (d, mats, rec) in enumerate(golden):
        given = {n: m for n, m in mats.items() if m.size}
        if d["ny"] == 0:
            given["C"] = np.zeros((0, d["nx"]))      # an explicit empty C: an absent one gets the reference's C = I default (another model)
        model = phc.MldModel(**given)
        got = simlog.lsim_k_batch([mats], d, None, rec["x"], rec["v"], rec["omega"])
        bound = simlog.sum_bound(d)
        for i in range(rec["x"].shape[0]):
            one = model.lsim_k(x_k=rec["x"][i], v_k=rec["v"][i], omega_k=rec["omega"][i])
            assert np.all(np.abs(one["x_k1"][:, 0] - got["x_k1"][i]) <= bound * got["terms_x"][i]), (k, i)
            assert np.all(np.abs(one["y"][:, 0] - got["y"][i]) <= bound * got["terms_y"][i]), (k, i)
            assert np.array_equal(np.asarray(one["cons"]).reshape(-1), got["cons"][i]), (k, i)
            assert np.array_equal(one["v"][:, 0], rec["v"][i])


def test_log_frame_has_the_reference_columns_and_one_row_per_step(golden):
    d, mats, rec = golden[0]
    K, B = 4, 2
    got = [simlog.lsim_k_batch([mats], d, None, rec["x"][2 * s:2 * s + 2], rec["v"][2 * s:2 * s + 2], rec["omega"][2 * s:2 * s + 2]) for s in range(K)]
    log = dict(x=np.stack([rec["x"][2 * s:2 * s + 2] for s in range(K)]), v=np.stack([rec["v"][2 * s:2 * s + 2] for s in range(K)]),
               omega=np.stack([rec["omega"][2 * s:2 * s + 2] for s in range(K)]), y=np.stack([g["y"] for g in got]),
               x_k1=np.stack([g["x_k1"] for g in got]), cons=np.stack([g["cons"] for g in got]))
    sl = simlog.to_mld_sim_log(log, 1, d, k0=10)
    assert isinstance(sl, phc.controllers.MldSimLog) and sorted(sl) == [10, 11, 12, 13]
    assert set(sl[10]) == {"x_k1", "x", "u", "delta", "z", "mu", "v", "y", "omega", "cons"}      # the names lsim_k returns (mld_model.py:696-699)
    df = sl.get_concat_log()
    assert list(df.columns.names) == ["var_names", "var_index"] and df.index.name == "k" and list(df.index) == [10, 11, 12, 13]
    widths = dict(x_k1=d["nx"], x=d["nx"], u=d["nu"], delta=d["ndelta"], z=d["nz"], mu=d["nmu"], v=rec["v"].shape[1], y=d["ny"], omega=d["nomega"], cons=d["nc"])
    assert {n: int((df.columns.get_level_values(0) == n).sum()) for n in widths} == widths
    assert np.array_equal(df["x_k1"].to_numpy(), log["x_k1"][:, 1]) and np.array_equal(df["u"].to_numpy(), log["v"][:, 1, :d["nu"]])
    assert np.array_equal(df["cons"].to_numpy().astype(bool), log["cons"][:, 1])


def test_the_four_entry_points_are_declared_listed_and_exported():
    with open(os.path.join(ROOT, "include", "mldgpu.h")) as f:
        header = f.read()
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(\s*mld_problem_t\s*\*" % name, header), name
        assert name in _lib.EXPORTS and hasattr(_lib.load(), name), name
        assert getattr(_lib.load(), name).argtypes is not None, name
    for flag, val in (("MLD_SIM_ADVANCE", 1), ("MLD_SIM_ACTUAL", 2), ("MLD_SIM_LOG", 4)):
        assert re.search(r"#define\s+%s\s+%d\b" % (flag, val), header) and getattr(_lib, flag) == val
    assert "mld_model.py:647-699" in header and "controller_base.py:58-146" in header      # declared with the reference lines it replaces
    syms = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in NEW:
        assert re.search(r"\bT %s\b" % name, syms), name
    assert "plant step" in _lib.version()


def test_sim_step_has_no_cpu_fallback_and_checks_shapes_first():
    """a handle-less shell reaches the C entry with a null problem: without a device MLD_ERR_NO_DEVICE, with one the refusal of a call without a batch;
    a v0 of the wrong shape is a ValueError before any C call"""
    from pyhybridcontrol_amd import gpu

    class _M(object):
        dims = dict(nx=2, nu=1, ndelta=1, nz=0, nmu=0, nomega=1, ny=1, nc=2, nu_l=0, nmu_l=0)
        nv = 2
    p = gpu.GpuProblem.__new__(gpu.GpuProblem)
    p.model, p.batch, p._h = _M(), 3, None
    with pytest.raises(ValueError, match="v0 has shape"):
        p.sim_step(v0=np.zeros((3, 5)))
    with pytest.raises(ValueError, match="expected integers"):
        p.sim_step(act_start=np.zeros((3, 1)))
    expect = "no HIP device" if _lib.device_count() <= 0 else "no batch resident"
    for call in (lambda: p.sim_step(v0=np.zeros(2), log=False), lambda: p.sim_log_begin(2), lambda: p.sim_log(0, 0)):
        with pytest.raises(phc.MldGpuError, match=expect):
            call()
