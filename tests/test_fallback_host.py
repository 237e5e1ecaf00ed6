"""Fallback inputs for instances without a usable plan (pyhybridcontrol_amd/fallback.py, mld_plan_memory / mld_set_plan_memory / mld_download_plan_memory /
mld_sim_step_fallback / mld_download_sim_log_source) at the boundary of the library and in numpy, without a GPU: header and binding agree, the entry points
follow the conventions of their neighbours, and the two rules -- the choice of the source and the ageing of the memory -- on an example written out by hand."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from pyhybridcontrol_amd import _lib, fallback, policy

HDR = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mldgpu.h")).read()
NEW = dict(mld_plan_memory=2, mld_set_plan_memory=3, mld_download_plan_memory=3, mld_sim_step_fallback=15, mld_download_sim_log_source=4)


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
    step, res = _args("mld_sim_step_fallback"), _args("mld_sim_step_resolve")
    assert step[2] == "int fb" and last(step[3:13]) == last(res[3:13])                 # mld_sim_step_resolve's, fb in the place of u0 ...
    assert step[13] == "int32_t *u_source_out" and step[14] == res[13] == "int32_t *n_skipped_out"      # ... and u_source_out in front of the skip count
    assert last(_args("mld_download_sim_log_source"))[1:] == ["first", "count", "u_source"]
    assert last(_args("mld_set_plan_memory"))[1:] == ["u", "age"] and last(_args("mld_download_plan_memory"))[1:] == ["u_out", "age_out"]
    assert re.search(r"#define\s+MLD_FB_MEMORY\s+1\b", HDR) and re.search(r"#define\s+MLD_FB_POLICY\s+2\b", HDR)
    assert (_lib.MLD_FB_MEMORY, _lib.MLD_FB_POLICY) == (1, 2) == (fallback.FB_BITS["memory"], fallback.FB_BITS["policy"])
    assert "micro_grid_agents.py:728-735" in HDR and "controller_base.py:229-253" in HDR      # declared with the reference lines they replace
    assert "fallback inputs" in _lib.version()


def test_entry_points_without_a_device_or_a_handle():
    lib = _lib.load()
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    x, es, src, sk, age = np.full(8, 7.0), np.full(2, 7, np.int32), np.full(2, 7, np.int32), np.full(1, 7, np.int32), np.full(2, 7, np.int32)
    calls = (("mld_plan_memory", lambda: lib.mld_plan_memory(None, 1)),
             ("mld_set_plan_memory", lambda: lib.mld_set_plan_memory(None, _lib.dptr(x), ip(age))),
             ("mld_download_plan_memory", lambda: lib.mld_download_plan_memory(None, _lib.dptr(x), ip(age))),
             ("mld_sim_step_fallback", lambda: lib.mld_sim_step_fallback(None, None, 3, None, 0, 0, _lib.dptr(x), None, None, None, None, None, ip(es), ip(src), ip(sk))),
             ("mld_download_sim_log_source", lambda: lib.mld_download_sim_log_source(None, 0, 1, ip(src))))
    for name, call in calls:
        rc = call()
        if _lib.device_count() < 1:
            assert rc == -2 and b"no HIP device" in lib.mld_last_error(), name           # MLD_ERR_NO_DEVICE, before anything else
        else:
            assert rc == -1 and b"no batch resident" in lib.mld_last_error(), name        # MLD_ERR_INVALID: no handle
    assert np.all(x == 7.0) and np.all(es == 7) and np.all(src == 7) and np.all(sk == 7) and np.all(age == 7)


def test_fb_bits():
    assert fallback.fb_bits(()) == 0 and fallback.fb_bits(("memory",)) == 1 and fallback.fb_bits("policy") == 2
    assert fallback.fb_bits(("policy", "memory")) == 3 == fallback.fb_bits(3)
    with pytest.raises(ValueError, match="not one of"):
        fallback.fb_bits(("memory", "plan"))


def test_every_plan_usable_returns_the_plan_and_ages_of_one():
    rng = np.random.default_rng(9100)
    B, N, nu = 5, 3, 2
    plan = rng.normal(size=(B, N, nu))
    mem, age = rng.normal(size=(B, N, nu)), np.array([-1, 1, 2, 3, -1], np.int32)
    P = policy.ThresholdPolicy(np.ones((1, nu, 1)), 50.0, 60.0)
    for fb in (0, 1, 2, 3, ("memory", "policy")):
        u, src = fallback.choose_np(np.ones(B, bool), plan[:, 0], mem, age, fb, P=P, x=np.full((B, 1), 40.0), u_prev=np.zeros((B, nu)))
        assert np.array_equal(u, plan[:, 0]) and np.array_equal(src, np.zeros(B, np.int32)) and src.dtype == np.int32, fb
        mem2, age2 = fallback.commit_np(src, plan, mem, age, N)
        assert np.array_equal(mem2, plan) and np.array_equal(age2, np.ones(B, np.int32)) and age2.dtype == np.int32, fb
    assert age[0] == -1 and not np.array_equal(mem, plan)                                 # the arguments are left as they are


def _example(fb):
    """three steps, four instances, N_tilde = 3, one channel; the thermostat on at x <= 50, off at x >= 60, inputs 1 / 0.  plan of step s: u[b, k] =
    100 s + 10 b + k; the memory before step 0 holds -(10 b + k), and only instance 2 remembers anything: age 2."""
    N = 3
    P = policy.ThresholdPolicy(np.ones((1, 1, 1)), 50.0, 60.0)
    plan = lambda s: (100.0 * s + 10.0 * np.arange(4)[:, None] + np.arange(N)[None, :])[:, :, None]
    mem = -(10.0 * np.arange(4)[:, None] + np.arange(N)[None, :])[:, :, None]
    age = np.array([-1, -1, 2, -1], np.int32)
    usable = np.array([[1, 1, 0, 0], [1, 0, 0, 0], [1, 0, 0, 0]], bool)
    x = np.array([[55.0, 55.0, 55.0, 45.0], [55.0, 55.0, 55.0, 55.0], [55.0, 55.0, 65.0, 65.0]])[:, :, None]
    up = np.zeros((4, 1))
    us, srcs, ages = [], [], []
    for s in range(3):
        u, src = fallback.choose_np(usable[s], plan(s)[:, 0], mem, age, fb, P=P, midx=None, x=x[s], u_prev=up)
        mem, age = fallback.commit_np(src, plan(s), mem, age, N)
        us.append(u[:, 0]); srcs.append(src); ages.append(age)
        up = u
    return np.array(us), np.array(srcs), np.array(ages), mem


def test_the_example_by_hand():
    # memory and policy
    u, src, age, mem = _example(("memory", "policy"))
    # step 0: plan, plan, the memory's row 2 (age 2 = N_tilde - 1, the last usable row), policy (x = 45 <= 50: on)
    # step 1: plan, the memory's row 1, policy (age 3 = N_tilde: exhausted; inside the band, u_prev = -22 is not u_on: off), policy (inside, u_prev = 1: holds)
    # step 2: plan, the memory's row 2, policy (x = 65 >= 60: off), policy (off)
    assert src.tolist() == [[0, 0, 1, 2], [0, 1, 2, 2], [0, 1, 2, 2]]
    assert u.tolist() == [[0.0, 10.0, -22.0, 1.0], [100.0, 11.0, 0.0, 1.0], [200.0, 12.0, 0.0, 0.0]]
    assert age.tolist() == [[1, 1, 3, -1], [1, 2, 3, -1], [1, 3, 3, -1]]           # 3 is the cap; -1 stays -1 whatever is applied
    assert mem[:, :, 0].tolist() == [[200.0, 201.0, 202.0], [10.0, 11.0, 12.0], [-20.0, -21.0, -22.0], [-30.0, -31.0, -32.0]]
    # memory only: where the policy stood in, nothing is left -- source -1, u = 0 (not applied); the memory moves as before
    u1, src1, age1, mem1 = _example(("memory",))
    assert src1.tolist() == [[0, 0, 1, -1], [0, 1, -1, -1], [0, 1, -1, -1]]
    assert u1.tolist() == [[0.0, 10.0, -22.0, 0.0], [100.0, 11.0, 0.0, 0.0], [200.0, 12.0, 0.0, 0.0]]
    assert np.array_equal(age1, age) and np.array_equal(mem1, mem)
    # policy only: the memory is not consulted, but it is still kept
    u2, src2, age2, mem2 = _example(("policy",))
    assert src2.tolist() == [[0, 0, 2, 2], [0, 2, 2, 2], [0, 2, 2, 2]]
    assert u2.tolist() == [[0.0, 10.0, 0.0, 1.0], [100.0, 0.0, 0.0, 1.0], [200.0, 0.0, 0.0, 0.0]]
    assert np.array_equal(age2, age) and np.array_equal(mem2, mem)
    # nothing allowed: the step of today
    _, src0, age0, _ = _example(())
    assert src0.tolist() == [[0, 0, -1, -1], [0, -1, -1, -1], [0, -1, -1, -1]] and np.array_equal(age0, age)


def test_choose_np_refusals():
    B, N, nu = 2, 3, 2
    z = np.zeros((B, nu))
    with pytest.raises(ValueError, match="needs mem_u and age"):
        fallback.choose_np(np.zeros(B, bool), z, None, None, 1)
    with pytest.raises(ValueError, match="needs P, x and u_prev"):
        fallback.choose_np(np.zeros(B, bool), z, None, None, 2)
    mixed = policy.ThresholdPolicy(np.ones((1, nu, 1)), 50.0, 60.0, mode=[1, 0])
    with pytest.raises(ValueError, match="passes a channel through"):
        fallback.choose_np(np.zeros(B, bool), z, None, None, 2, P=mixed, x=np.zeros((B, 1)), u_prev=z)
