"""Applying a kept selection (pyhybridcontrol_amd/fallback.py: choose_selected_np / commit_selected_np; mld_keep_selection / mld_set_selection /
mld_download_selection / mld_sim_step_selected / mld_download_sim_log_pick) at the boundary of the library and in numpy, without a GPU: header and binding
agree, the entry points follow the conventions of their neighbours, the two rules on an example written out by hand -- every source, K == N_tilde and
K < N_tilde, a policy pick, and an instance without a choice that must NOT take a usable plan --, their refusals, and the stand-alone host check of the
kernels' rule functions under the address and undefined-behaviour sanitizers."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from pyhybridcontrol_amd import _lib, fallback, gpu, policy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = open(os.path.join(ROOT, "include", "mldgpu.h")).read()
NEW = dict(mld_keep_selection=2, mld_set_selection=5, mld_download_selection=6, mld_sim_step_selected=16, mld_download_sim_log_pick=4)


def _args(name):
    m = re.search(r"int\s+%s\s*\(([^;]*?)\)\s*;" % name, HDR)
    assert m, name
    return [a.strip() for a in m.group(1).split(",")]


def test_header_and_binding_agree_on_the_prototypes():
    lib = _lib.load()
    for name, n in NEW.items():
        assert name in _lib.EXPORTS and hasattr(lib, name), name
        assert len(_args(name)) == n == len(getattr(lib, name).argtypes), name
    last = lambda args: [(a.split("*")[-1].split() or [""])[-1] for a in args]      # the argument's name ("" for an unnamed handle)
    step, fb = _args("mld_sim_step_selected"), _args("mld_sim_step_fallback")
    assert step[:15] == fb and step[15] == "int32_t *pick_out"                      # mld_sim_step_fallback's, and pick_out behind them
    assert lib.mld_sim_step_selected.argtypes[:15] == lib.mld_sim_step_fallback.argtypes
    assert last(_args("mld_set_selection"))[1:] == ["K", "choice", "policy", "u"]
    assert last(_args("mld_download_selection"))[1:] == ["K_out", "choice", "policy", "u", "valid_out"]
    assert last(_args("mld_download_sim_log_pick"))[1:] == ["first", "count", "pick"] and last(_args("mld_keep_selection"))[1:] == ["enable"]
    assert "kept selection" in _lib.version()
    # the Python surface: new keywords with defaults that change nothing, at the end
    for fn in (gpu.GpuProblem.select_plan, gpu.GpuProblem.select_plan_policies):      # keep= is the wrapper's, like complete=: the method's signature stays
        par = inspect.signature(fn.__wrapped__, follow_wrapped=False).parameters      # (behind complete='s wrapper, which tests its word first)
        assert par["keep"].default is False and par["keep"].kind is inspect.Parameter.KEYWORD_ONLY and "keep" not in inspect.signature(fn).parameters, fn
    par = inspect.signature(gpu.GpuProblem.sim_step).parameters
    assert list(par)[-1] == "selected" and par["selected"].default is False
    for name in ("selection", "set_selection", "sim_log_pick"):
        assert callable(getattr(gpu.GpuProblem, name)), name


def test_entry_points_without_a_device_or_a_handle():
    lib = _lib.load()
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    x, i4 = np.full(8, 7.0), [np.full(2, 7, np.int32) for _ in range(6)]
    calls = (("mld_set_selection", lambda: lib.mld_set_selection(None, 1, ip(i4[0]), ip(i4[1]), _lib.dptr(x))),
             ("mld_download_selection", lambda: lib.mld_download_selection(None, ip(i4[2]), ip(i4[0]), ip(i4[1]), _lib.dptr(x), ip(i4[3]))),
             ("mld_sim_step_selected", lambda: lib.mld_sim_step_selected(None, None, 3, None, 0, 0, _lib.dptr(x), None, None, None, None, None, ip(i4[0]), ip(i4[1]),
                                                                         ip(i4[4]), ip(i4[5]))),
             ("mld_download_sim_log_pick", lambda: lib.mld_download_sim_log_pick(None, 0, 1, ip(i4[0]))))
    for name, call in calls:
        rc = call()
        if _lib.device_count() < 1:
            assert rc == -2 and b"no HIP device" in lib.mld_last_error(), name           # MLD_ERR_NO_DEVICE, before anything else
        else:
            assert rc == -1 and b"no batch resident" in lib.mld_last_error(), name        # MLD_ERR_INVALID: no handle
    assert lib.mld_keep_selection(None, 1) == -1 and b"p is NULL" in lib.mld_last_error()      # sticky switch: mld_set_rollout_completion's convention
    assert np.all(x == 7.0) and all(np.all(a == 7) for a in i4)


N = 3
CHOICE = np.array([[0, 2, -1, -1, 1, -1], [-1, -1, -1, 0, 1, 2]], np.int32)
POLICY = np.array([[-1, 0, -1, -1, -1, -1], [-1, -1, -1, -1, -1, 0]], np.int32)
X = np.array([[55.0, 55.0, 55.0, 55.0, 55.0, 45.0], [55.0, 55.0, 55.0, 65.0, 55.0, 55.0]])[:, :, None]


def _example(K, fb=("memory", "policy")):
    """two steps, six instances, N_tilde = 3, one channel on one state (scripts/selected_host_check.cpp runs the same example through the C functions); the
    thermostat on (1) at x <= 50, off (0) at x >= 60, in between what it was.  The selection of step s holds u[b, k] = 100 s + 10 b + k, a policy pick
    100 s + 10 b + 2 in row 0 and NaN behind it; the memory before step 0 holds -(10 b + k); ages -1, -1, 2, 3, 1, -1."""
    P = policy.ThresholdPolicy(np.ones((1, 1, 1)), 50.0, 60.0)
    mem = -(10.0 * np.arange(6)[:, None] + np.arange(N)[None, :])[:, :, None]
    age = np.array([-1, -1, 2, 3, 1, -1], np.int32)
    up = np.zeros((6, 1))
    us, srcs, picks, ages = [], [], [], []
    for s in range(2):
        sel = (100.0 * s + 10.0 * np.arange(6)[:, None] + np.arange(K)[None, :])[:, :, None]
        pol = POLICY[s] >= 0
        sel[pol, 0, 0] += 2.0
        sel[pol, 1:] = np.nan
        u, src, pick = fallback.choose_selected_np(CHOICE[s], sel, mem, age, fb, P=P, midx=None, x=X[s], u_prev=up)
        mem, age = fallback.commit_selected_np(src, POLICY[s], sel, mem, age, N)
        us.append(u[:, 0]); srcs.append(src); picks.append(pick); ages.append(age)
        up = np.where((src >= 0)[:, None], u, up)
    return np.array(us), np.array(srcs), np.array(picks), np.array(ages), mem


def test_the_example_by_hand_full_horizon():
    u, src, pick, age, mem = _example(N)
    # step 0: a sequence (remembered), a policy pick (row 0, not remembered), the memory's row 2 (age 2 = N_tilde - 1), the policy (age 3: exhausted; inside
    #         the band, u_prev = 0 is not u_on: off), a sequence (remembered over an age-1 memory), the policy (nothing remembered; x = 45 <= 50: on)
    # step 1: the memory's row 1 of what step 0 remembered, the policy (u_prev = 12 is not u_on: off), the policy (off), a sequence, a sequence, a policy pick
    assert src.tolist() == [[3, 3, 1, 2, 3, 2], [1, 2, 2, 3, 3, 3]] and src.dtype == np.int32            # every source occurs
    assert u.tolist() == [[0.0, 12.0, -22.0, 0.0, 40.0, 1.0], [1.0, 0.0, 0.0, 130.0, 140.0, 152.0]]
    assert pick.tolist() == [[0, 2, -1, -1, 1, -1], [-1, -1, -1, 0, 1, 2]] and pick.dtype == np.int32
    assert age.tolist() == [[1, -1, 3, 3, 1, -1], [2, -1, 3, 1, 1, -1]] and age.dtype == np.int32
    assert mem[:, :, 0].tolist() == [[0.0, 1.0, 2.0], [-10.0, -11.0, -12.0], [-20.0, -21.0, -22.0], [130.0, 131.0, 132.0], [140.0, 141.0, 142.0], [-50.0, -51.0, -52.0]]
    # memory only: where the policy stood in nothing is left -- source -1, u = 0 (not applied); the memory moves as before
    u1, src1, pick1, age1, mem1 = _example(N, ("memory",))
    assert src1.tolist() == [[3, 3, 1, -1, 3, -1], [1, -1, -1, 3, 3, 3]] and u1.tolist() == [[0.0, 12.0, -22.0, 0.0, 40.0, 0.0], [1.0, 0.0, 0.0, 130.0, 140.0, 152.0]]
    assert np.array_equal(pick1, pick) and np.array_equal(age1, age) and np.array_equal(mem1, mem)
    # nothing allowed: a choice or nothing
    _, src0, _, age0, _ = _example(N, ())
    assert src0.tolist() == [[3, 3, -1, -1, 3, -1], [-1, -1, -1, 3, 3, 3]] and np.array_equal(age0, age)


def test_the_example_by_hand_short_sequences():
    """K = 2 < N_tilde: nothing is remembered, every age moves on"""
    u, src, pick, age, mem = _example(2)
    # step 1, instance 0: nothing was remembered at step 0, so the policy (inside the band, u_prev = 0: off) instead of the memory
    assert src.tolist() == [[3, 3, 1, 2, 3, 2], [2, 2, 2, 3, 3, 3]]
    assert u.tolist() == [[0.0, 12.0, -22.0, 0.0, 40.0, 1.0], [0.0, 0.0, 0.0, 130.0, 140.0, 152.0]]
    assert pick.tolist() == [[0, 2, -1, -1, 1, -1], [-1, -1, -1, 0, 1, 2]]
    assert age.tolist() == [[-1, -1, 3, 3, 2, -1], [-1, -1, 3, 3, 3, -1]]
    assert np.array_equal(mem[:, :, 0], -(10.0 * np.arange(6)[:, None] + np.arange(N)[None, :]))


def test_no_choice_does_not_take_a_usable_plan():
    """the same inputs through choose_np with every plan usable and through choose_selected_np with no choice: the first takes the plan everywhere, the
    second never -- there is no argument through which a plan could reach it"""
    B, nu = 4, 2
    rng = np.random.default_rng(9300)
    plan, mem = rng.normal(size=(B, N, nu)), rng.normal(size=(B, N, nu))
    age = np.array([-1, 1, 2, 3], np.int32)
    P = policy.ThresholdPolicy(np.ones((1, nu, 1)), 50.0, 60.0)
    kw = dict(P=P, x=np.full((B, 1), 40.0), u_prev=np.zeros((B, nu)))
    u_fb, src_fb = fallback.choose_np(np.ones(B, bool), plan[:, 0], mem, age, 3, **kw)
    assert np.array_equal(src_fb, np.zeros(B, np.int32)) and np.array_equal(u_fb, plan[:, 0])
    u, src, pick = fallback.choose_selected_np(np.full(B, -1), plan, mem, age, 3, **kw)
    assert src.tolist() == [2, 1, 1, 2] and np.all(pick == -1)
    assert np.array_equal(u[1], mem[1, 1]) and np.array_equal(u[2], mem[2, 2]) and np.all(u[[0, 3]] == 1.0)      # x = 40 <= 50: on
    assert "usable" not in inspect.signature(fallback.choose_selected_np).parameters and "plan_u" not in inspect.signature(fallback.choose_selected_np).parameters
    # the memory of a usable plan is not written either: no choice ages it
    mem2, age2 = fallback.commit_selected_np(src, np.full(B, -1), plan, mem, age, N)
    assert np.array_equal(mem2, mem) and age2.tolist() == [-1, 2, 3, 3]
    assert age.tolist() == [-1, 1, 2, 3]                                            # the arguments are left as they are


def test_refusals():
    B, nu = 2, 2
    sel = np.zeros((B, N, nu))
    with pytest.raises(ValueError, match=r"choice has shape"):
        fallback.choose_selected_np(np.zeros((B, 1), int), sel, None, None, 0)
    with pytest.raises(ValueError, match=r"choice has shape"):
        fallback.choose_selected_np(np.zeros(B), sel, None, None, 0)
    with pytest.raises(ValueError, match=r"sel_u has shape"):
        fallback.choose_selected_np(np.zeros(B, int), sel[:, :, 0], None, None, 0)
    with pytest.raises(ValueError, match=r"sel_u has shape"):
        fallback.choose_selected_np(np.zeros(B, int), sel[:, :0], None, None, 0)
    with pytest.raises(ValueError, match="choice of instance 1 is -2"):
        fallback.choose_selected_np(np.array([0, -2]), sel, None, None, 0)
    bad = sel.copy()
    bad[1, 0, 1] = np.nan
    with pytest.raises(ValueError, match="sel_u of instance 1, step 0 is not finite"):
        fallback.choose_selected_np(np.zeros(B, int), bad, None, None, 0)
    u, src, pick = fallback.choose_selected_np(np.array([0, -1]), bad, None, None, 0)      # ... which is not read without a choice
    assert src.tolist() == [3, -1] and pick.tolist() == [0, -1] and np.all(u == 0.0)
    with pytest.raises(ValueError, match="needs mem_u and age"):
        fallback.choose_selected_np(np.zeros(B, int), sel, None, None, 1)
    with pytest.raises(ValueError, match="needs P, x and u_prev"):
        fallback.choose_selected_np(np.zeros(B, int), sel, None, None, 2)
    with pytest.raises(ValueError, match="not one of"):
        fallback.choose_selected_np(np.zeros(B, int), sel, None, None, ("plan",))
    with pytest.raises(ValueError, match=r"sel_policy has shape"):
        fallback.commit_selected_np(np.zeros(B, int), np.zeros(B + 1, int), sel, sel, np.ones(B, int), N)
    with pytest.raises(ValueError, match=r"sel_u has shape"):
        fallback.commit_selected_np(np.zeros(B, int), np.zeros(B, int), sel[0], sel, np.ones(B, int), N)


def test_host_check_is_clean_under_the_sanitizers(tmp_path):
    """scripts/selected_host_check.cpp, its own executable: the C functions k_selected_inputs and k_selected_commit call, over choice -1 / 0 / 63, policy
    -1 / 0, age -1 / 1 / N - 1 / N, K 1 / N - 1 / N and every fb on arrays of exactly the length the rule may read, and the example above, under ASan and UBSan"""
    exe = str(tmp_path / "selected_host_check")
    cmd = ["c++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "pyhybridcontrol_amd", "csrc"),
           os.path.join(ROOT, "scripts", "selected_host_check.cpp"), "-o", exe]
    built = subprocess.run(cmd + ["-static-libasan", "-static-libubsan"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    if built.returncode != 0:
        built = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert built.returncode == 0, built.stdout
    ran = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert ran.returncode == 0 and "edges: 240 combinations" in ran.stdout and "all values as written out" in ran.stdout, ran.stdout
