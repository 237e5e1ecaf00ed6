"""CPU tests of the plan selection with closed-loop policies among the candidates (simlog.select_plan_np(policy_u0=...); mld_rollout_select_policy /
GpuProblem.select_plan_policies(policies=...)): the numpy convention of the chosen inputs against a restated Python loop, the ABI export and the wrapper's signature,
the unchanged argtypes of mld_rollout_select and the older rollout entries, the entry guard, and the stand-alone host check of what the entry adds to the
kernels under the address and undefined-behaviour sanitizers.  No GPU needed."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from pyhybridcontrol_amd import _lib, gpu, simlog
from pyhybridcontrol_amd.simlog import PlanSelector, RiskTable

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, G, S, K, NU = 30, 2, 4, 3, 2


def _risk(rng, P):
    r = dict(mean=rng.integers(-3, 4, size=(B, P, G)) / 2.0, n_complete=rng.integers(0, S + 1, size=(B, P)).astype(np.int32))      # dyadic, many ties
    r["mean"][rng.uniform(size=(B, P, G)) < 0.1] = np.nan
    return r


def _shape(risk, n_seq):
    """every third instance: no sequence is admissible (only a policy can win); every fifth: nobody is"""
    risk["n_complete"][::3, :n_seq] = 0
    risk["n_complete"][::5] = 0
    return risk


@pytest.mark.parametrize("n_seq,T", [(0, 1), (0, 3), (1, 1), (2, 2), (3, 1), (61, 3)])
def test_chosen_inputs_against_a_restated_loop(n_seq, T):
    """the choice is the rule's over all P candidates; u, u0 and policy by the convention: a sequence pick is copied, a policy pick has its step-0 row in
    u0 and u[:, 0] and NaN behind it, no pick is all NaN"""
    rng = np.random.default_rng(9400 + 10 * n_seq + T)
    P = n_seq + T
    t = RiskTable(None, ()).add("cost", "cost").add("mu", "mu_total")
    sel = PlanSelector(t).minimise("cost", "mean").subject_to("mu", "mean", 0.5)
    risk = _shape(_risk(rng, P), n_seq)
    cand = rng.standard_normal((B, n_seq, K, NU))
    pu0 = rng.standard_normal((B, T, NU))
    seen = set()
    for mc in (1, S):
        plain = simlog.select_plan_np(risk, sel, mc)
        got = simlog.select_plan_np(risk, sel, mc, candidates=cand, policy_u0=pu0)
        for k in simlog.SELECT_KEYS:
            assert np.array_equal(got[k], plain[k], equal_nan=True), k
        assert got["u"].shape == (B, K, NU) and got["u0"].shape == (B, NU) and got["policy"].dtype == np.int32 and got["policy"].shape == (B,)
        for b in range(B):
            ch = int(got["choice"][b])
            u, u0, pol = np.full((K, NU), np.nan), np.full(NU, np.nan), -1
            if ch >= n_seq:
                pol = ch - n_seq
                u0 = pu0[b, pol]
                u[0] = u0
            elif ch >= 0:
                u, u0 = cand[b, ch], cand[b, ch, 0]
            assert got["policy"][b] == pol and np.array_equal(got["u"][b], u, equal_nan=True) and np.array_equal(got["u0"][b], u0, equal_nan=True), (mc, b)
            seen.add("none" if ch < 0 else ("policy" if ch >= n_seq else "sequence"))
    assert seen >= ({"none", "policy"} | ({"sequence"} if n_seq else set())), seen
    # without sequences candidates may be None (K = 1) or the empty array that carries K
    if n_seq == 0:
        lone = simlog.select_plan_np(risk, sel, 1, policy_u0=pu0)
        assert lone["u"].shape == (B, 1, NU) and np.array_equal(lone["u0"], simlog.select_plan_np(risk, sel, 1, candidates=cand, policy_u0=pu0)["u0"], equal_nan=True)
    else:
        with pytest.raises(ValueError, match="candidates is None"):
            simlog.select_plan_np(risk, sel, 1, policy_u0=pu0)
    with pytest.raises(ValueError, match="candidates has shape"):
        simlog.select_plan_np(risk, sel, 1, candidates=rng.standard_normal((B, n_seq + 1, K, NU)), policy_u0=pu0)
    with pytest.raises(ValueError, match="policy_u0 has shape"):
        simlog.select_plan_np(risk, sel, 1, candidates=cand, policy_u0=rng.standard_normal((B, P + 1, NU)))
    # without policy_u0 the function is what it was
    old = simlog.select_plan_np(risk, sel, 1, candidates=rng.standard_normal((B, P, K, NU)))
    assert sorted(old) == ["admissible", "choice", "n_admissible", "score", "u", "u0"]


def test_abi_declares_and_binds_the_entry_point():
    assert "mld_rollout_select_policy" in _lib.EXPORTS
    with open(os.path.join(ROOT, "include", "mldgpu.h")) as fh:
        header = fh.read()
    assert re.search(r"\bint mld_rollout_select_policy\(mld_problem_t \*p, mld_problem_t \*aux, int K, int S, int P, int plan_first, const double \*u_cand,", header)
    assert re.search(r"int T, const double \*pol_sel, const double \*pol_on_at, const double \*pol_off_at, const double \*pol_u_on, const double \*pol_u_off,\s+"
                     r"const int32_t \*pol_mode, const double \*u_prev, int32_t \*switches_out\);", header)
    lib = _lib.load()
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    assert hasattr(lib, "mld_rollout_select_policy") and len(lib.mld_rollout_select_policy.argtypes) == 78
    assert list(lib.mld_rollout_select_policy.argtypes[:69]) == list(lib.mld_rollout_select.argtypes)
    assert list(lib.mld_rollout_select_policy.argtypes[69:]) == [C.c_int, dp, dp, dp, dp, dp, ip, dp, ip]
    # mld_rollout_select and the older rollout entries are bound as they were
    assert len(lib.mld_rollout_select.argtypes) == 69 and len(lib.mld_rollout_kpi.argtypes) == 43 and len(lib.mld_rollout_risk.argtypes) == 60
    assert list(lib.mld_rollout_risk.argtypes[:43]) == list(lib.mld_rollout_kpi.argtypes)
    assert len(lib.mld_rollout_batch.argtypes) == 22 and len(lib.mld_rollout_policy.argtypes) == 24 and len(lib.mld_upload_policy.argtypes) == 7
    # the entry guard on a NULL handle: refused, nothing written
    ipp = lambda a: a.ctypes.data_as(ip)
    src, alpha = np.zeros(1, np.int32), np.array([0.5])
    choice, score, u0, sw = np.full(2, 7, np.int32), np.full(2, 7.0), np.full(2, 7.0), np.full(2, 7, np.int32)
    args = [None, None, 2, 1, 1, 0, None, None, None, 0, None, 0, 0, None, None, None, None, None, None, None, 1e-6, None,
            1, ipp(src), None, None, 1, _lib.dptr(alpha), 0, 0, 0, 0, None, None, None, None, 1,
            ipp(choice), _lib.dptr(score), None, None, None, _lib.dptr(u0)] + [None] * 26 + [1, None, None, None, None, None, None, None, ipp(sw)]
    assert len(args) == 78
    rc = lib.mld_rollout_select_policy(*args)
    if _lib.device_count() < 1:
        assert rc == -2 and b"no HIP device" in lib.mld_last_error()
    else:
        assert rc == -1 and b"mld_rollout_select_policy" in lib.mld_last_error() and b"no batch resident" in lib.mld_last_error()
    assert np.all(choice == 7) and np.all(score == 7.0) and np.all(u0 == 7.0) and np.all(sw == 7)


def test_wrapper_signature():
    old = inspect.signature(gpu.GpuProblem.select_plan)
    assert list(old.parameters) == ["self", "resolve", "selector", "candidates", "plan_first", "K", "omega_seq", "start", "step", "cost_w", "kpis", "price_start",
                                    "vio_tol", "min_complete", "per_candidate", "per_trajectory"]      # select_plan() is what it was
    sig = inspect.signature(gpu.GpuProblem.select_plan_policies)
    names = list(sig.parameters)
    assert names[:5] == ["self", "resolve", "selector", "policies", "u_prev"] and sig.parameters["policies"].default is None and sig.parameters["u_prev"].default is None
    assert names[5:] == list(old.parameters)[3:]                                                       # ... and every argument of it, with its default
    assert all(sig.parameters[k].default == old.parameters[k].default for k in names[5:])
    sig = inspect.signature(simlog.select_plan_np)
    assert list(sig.parameters) == ["risk_per_candidate", "selector", "min_complete", "candidates", "policy_u0"] and sig.parameters["policy_u0"].default is None
    # rollout() is what it was
    assert list(inspect.signature(gpu.GpuProblem.rollout).parameters) == ["self", "resolve", "K", "u_seq", "omega_seq", "start", "step", "cost_w", "trajectories", "policy",
                                                                          "u_prev", "kpis", "price_start", "vio_tol", "risk", "per_trajectory"]


def test_host_check_is_clean_under_the_sanitizers(tmp_path):
    """scripts/select_policy_host_check.cpp, its own executable: ro_run<true> with the all-pass-through table against ro_run<false> bit for bit, the table
    index arithmetic at its edges on a buffer of exactly the tables' length, and the input rule of k_select_inputs, under ASan and UBSan"""
    exe = str(tmp_path / "select_policy_host_check")
    cmd = ["c++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "pyhybridcontrol_amd", "csrc"),
           os.path.join(ROOT, "scripts", "select_policy_host_check.cpp"), "-o", exe]
    built = subprocess.run(cmd + ["-static-libasan", "-static-libubsan"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    if built.returncode != 0:
        built = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert built.returncode == 0, built.stdout
    ran = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert ran.returncode == 0 and "the pass-through table is the open loop, bit for bit; every index as restated" in ran.stdout, ran.stdout
