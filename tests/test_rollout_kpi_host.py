"""CPU tests of the rollout KPIs (simlog.rollout_kpis_np; mld_rollout_kpi / GpuProblem.rollout(kpis=...)): the numpy rule against simlog.summary_np on a
log assembled record by record from simlog.rollout_np's trajectory, the unfinished endings, the price window's edges, the ABI, the argument checks of the
Python wrapper that come before any C call, and the stand-alone host check of ro_run's KPI variant under the address and undefined-behaviour sanitizers.
No GPU needed."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import _aux_ref
import _rollout_ref
from pyhybridcontrol_amd import _lib, gpu, prices, simlog, synthetic as syn
from pyhybridcontrol_amd.simlog import KpiTable

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, S, K, N = 4, 3, 5, 3
STEP, N_CHAN = 2, 2


def _trajectories(hard=False):
    """tests/test_rollout_host.py's scenario: make_agent(3) x 2 models, 4 instances x 3 realisations x 5 steps, the closed form as resolver"""
    mats_list, xs, oms = [], [], []
    for k in range(2):
        rng = np.random.default_rng(8800 + k)
        mats, d, _ = syn.make_agent(3, rng, tie=True)
        if hard:
            mats, d = _aux_ref.hard_variant(mats, d)
        x0, om = syn.make_scenarios(3, N, B, rng, tie=True)
        mats_list.append(mats); xs.append(x0); oms.append(om)
    midx = np.arange(B) % 2
    x0, om = np.stack(xs)[midx, np.arange(B)], np.stack(oms)[midx, np.arange(B)]
    if hard:
        x0[1, 0] = 90.0                                                               # above T_max without slack: infeasible at step 0
    else:
        x0[1, 0], x0[2, 2] = 47.0, 80.5                                               # slack on both sides
    rng = np.random.default_rng(8810)
    u_seq = (rng.uniform(size=(B, K, d["nu"])) < 0.4).astype(float)
    _, _, _, om_seq = _rollout_ref.realised_library(om, N, d["nomega"], d["nx"], S, K, 1, rng)
    traj = simlog.rollout_np(mats_list, d, midx, x0, u_seq, om_seq, _rollout_ref.closed_form_resolver(mats_list, d))
    return d, midx, om_seq, traj


def _table(d, rng, M=2):
    nv = sum(d[k] for k in ("nu", "ndelta", "nz", "nmu"))
    t = KpiTable(M, d)
    t.add("x_only", w_x=rng.normal(size=d["nx"]), thresh=60.0)
    t.add("v_only", w_v=rng.normal(size=(M, nv)))
    t.add("y_only", w_y=np.ones(d["ny"]), thresh=np.array([0.0, 500.0]))
    t.add("omega_only", w_omega=rng.normal(size=d["nomega"]))
    t.add("xk1_only", w_xk1=rng.normal(size=(M, d["nx"])))
    t.add("all_five", w_x=rng.normal(size=d["nx"]), w_v=rng.normal(size=nv), w_y=rng.normal(size=d["ny"]), w_omega=rng.normal(size=d["nomega"]),
          w_xk1=rng.normal(size=d["nx"]), thresh=0.0)
    t.add("priced", w_v=rng.normal(size=nv), price_chan=1)
    t.add("u_0", w_v=np.eye(nv)[0])
    return t


def test_rollout_kpis_np_equals_summary_np_on_the_assembled_log():
    """per realisation the log a stepwise campaign would hold, assembled record by record from the trajectory: summary_np of it is the rule, in every bit"""
    d, midx, om_seq, traj = _trajectories()
    assert np.all(traj["end_status"] == 0)
    rng = np.random.default_rng(8820)
    t = _table(d, rng)
    plib = rng.uniform(0.5, 2.0, (STEP + K + 2) * N_CHAN)
    pstart = ((np.arange(B) % 3) * N_CHAN).astype(np.int64)
    price = prices.windows(plib, pstart, STEP, K, N_CHAN).reshape(B, K, N_CHAN)
    got = simlog.rollout_kpis_np(traj, t, price=price, vio_tol=1e-6, omega_seq=om_seq, model_idx=midx)
    assert got["names"] == t.names and got["sum"].shape == (B, S, len(t)) and got["n_vio"].shape == (B, S)
    assert got["min_step"].dtype == np.int32 and got["n_vio"].dtype == np.int32 and sorted(got) == sorted(("names",) + simlog.KPI_ROLLOUT_KEYS)
    for c in range(S):
        log = dict(x=np.zeros((K, B, d["nx"])), v=np.zeros((K, B, traj["v"].shape[-1])), y=np.zeros((K, B, d["ny"])), omega=np.zeros((K, B, d["nomega"])),
                   x_k1=np.zeros((K, B, d["nx"])), cons_vio=np.zeros((K, B)), nodes=np.zeros((K, B), np.int32))
        pr = np.zeros((K, B, N_CHAN))
        for k in range(K):
            log["x"][k], log["v"][k], log["y"][k], log["omega"][k] = traj["x"][:, c, k], traj["v"][:, c, k], traj["y"][:, c, k], om_seq[:, c, k]
            log["x_k1"][k], log["cons_vio"][k] = traj["x"][:, c, k + 1], traj["cons_vio"][:, c, k]
            pr[k] = plib[pstart[:, None] + (STEP + k) * N_CHAN + np.arange(N_CHAN)]      # what sim_step(step=STEP + k) records
        ref = simlog.summary_np(log, t, midx, price=pr, vio_tol=1e-6)
        assert np.all(ref["n_stepped"] == K)
        for key in simlog.KPI_ROLLOUT_KEYS:
            a, b = got[key][:, c], ref[key]
            assert a.dtype == b.dtype and np.array_equal(a, b), (c, key)
        assert np.array_equal(got["sum"][:, c].view(np.uint64), ref["sum"].view(np.uint64)), c
    assert (got["n_vio"] > 0).any() and (got["n_vio"] == 0).any() and (got["n_changes"][..., t.names.index("u_0")] > 0).any()
    assert np.all((got["min_step"] >= 0) & (got["max_step"] < K))                     # step indices k, the record indices of a log begun at 0
    # what the caller left out is named
    with pytest.raises(ValueError, match="needs omega_seq"):
        simlog.rollout_kpis_np(traj, t, price=price, model_idx=midx)
    with pytest.raises(ValueError, match="needs price"):
        simlog.rollout_kpis_np(traj, t, omega_seq=om_seq, model_idx=midx)


def test_unfinished_trajectories_get_nan_and_minus_one():
    d, midx, om_seq, traj = _trajectories(hard=True)
    dead = traj["end_status"] != 0
    assert dead[1].all() and not dead[0].any()
    t = KpiTable(2, d).add("x", w_x=np.ones(d["nx"]), thresh=0.0).add("y", w_y=np.ones(d["ny"]))
    got = simlog.rollout_kpis_np(traj, t, model_idx=midx)
    for key in simlog.KPI_ROLLOUT_KEYS:
        a = got[key]
        assert np.all(np.isnan(a[dead])) if a.dtype.kind == "f" else np.all(a[dead] == -1), key
        assert np.all(np.isfinite(a[~dead])) and (a.dtype.kind == "f" or np.all(a[~dead] >= 0)), key


def test_price_window_edges():
    """the window rule with len = K: s = 0 and s = lib_len - (step + K) n_chan are the first and the last valid start"""
    lib = np.arange(40.0)
    last = lib.size - (STEP + K) * N_CHAN
    w = prices.windows(lib, np.array([0, last]), STEP, K, N_CHAN).reshape(2, K, N_CHAN)
    assert w[0, 0, 0] == STEP * N_CHAN and w[1, K - 1, N_CHAN - 1] == lib.size - 1
    for bad in (last + 1, -1):
        with pytest.raises(IndexError, match="leaves the library"):
            prices.windows(lib, np.array([0, bad]), STEP, K, N_CHAN)
    d, midx, om_seq, traj = _trajectories()
    t = KpiTable(2, d).add("cost", w_v=np.eye(traj["v"].shape[-1])[d["nu"] + d["ndelta"]], price_chan=0)
    lib = np.random.default_rng(8830).uniform(0.5, 2.0, 40)
    start = np.array([0, last, 0, last])
    got = simlog.rollout_kpis_np(traj, t, price=prices.windows(lib, start, STEP, K, N_CHAN).reshape(B, K, N_CHAN), model_idx=midx)
    z = traj["v"][..., d["nu"] + d["ndelta"]]
    for b in range(B):
        for c in range(S):
            s = 0.0
            for k in range(K):
                s = s + lib[start[b] + (STEP + k) * N_CHAN] * z[b, c, k]
            assert abs(got["sum"][b, c, 0] - s) <= 1e-12 * abs(s)                     # (w_v = e_z: the dot product adds zeros to z)


def test_abi_declares_and_binds_the_entry_point():
    assert "mld_rollout_kpi" in _lib.EXPORTS
    with open(os.path.join(ROOT, "include", "mldgpu.h")) as fh:
        header = fh.read()
    assert re.search(r"\bint mld_rollout_kpi\(mld_problem_t \*p, mld_problem_t \*aux, int policy, int K, int S,", header)
    assert "price_start[b] + (step + k) * n_chan + ch" in header
    lib = _lib.load()
    assert hasattr(lib, "mld_rollout_kpi") and len(lib.mld_rollout_kpi.argtypes) == 43
    assert list(lib.mld_rollout_policy.argtypes) == list(lib.mld_rollout_kpi.argtypes[:2]) + list(lib.mld_rollout_kpi.argtypes[3:12]) + list(lib.mld_rollout_kpi.argtypes[22:35])
    x, es, sm = np.full(8, 7.0), np.full(2, 7, np.int32), np.full(2, 7.0)
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    rc = lib.mld_rollout_kpi(None, None, 0, 2, 1, None, None, None, None, 0, None, 0, 1, None, None, None, None, None, None, None, 1e-6, None,
                             _lib.dptr(x), None, None, None, None, None, None, None, None, None, ip(es), None, None, _lib.dptr(sm), None, None, None, None, None, None, None)
    if _lib.device_count() < 1:
        assert rc == -2 and b"no HIP device" in lib.mld_last_error()
    else:
        assert rc == -1 and b"no batch resident" in lib.mld_last_error()
    assert np.all(x == 7.0) and np.all(es == 7) and np.all(sm == 7.0)


def test_wrapper_signature():
    import inspect
    sig = inspect.signature(gpu.GpuProblem.rollout)
    assert [sig.parameters[k].default for k in ("kpis", "price_start", "vio_tol")] == [None, None, 1e-6]
    assert list(sig.parameters)[:11] == ["self", "resolve", "K", "u_seq", "omega_seq", "start", "step", "cost_w", "trajectories", "policy", "u_prev"]


def test_host_check_is_clean_under_the_sanitizers(tmp_path):
    """scripts/rollout_kpi_host_check.cpp, its own executable: ro_run's KPI variant with and without the policy, n_kpi = 1 and 64, K = 1, declined
    trajectories and a tabled model without auxiliaries, under ASan and UBSan"""
    exe = str(tmp_path / "rollout_kpi_host_check")
    cmd = ["c++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "pyhybridcontrol_amd", "csrc"),
           os.path.join(ROOT, "scripts", "rollout_kpi_host_check.cpp"), "-o", exe]
    built = subprocess.run(cmd + ["-static-libasan", "-static-libubsan"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    if built.returncode != 0:
        built = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert built.returncode == 0, built.stdout
    ran = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert ran.returncode == 0 and "every statistic as the log route's functions give it" in ran.stdout, ran.stdout
