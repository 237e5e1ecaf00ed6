"""Device completion of declined rollout trajectories at the boundary of the library and on the CPU, without a GPU: header, binding and export agreeing
on the two entries and the mode bits, the refusals that need no handle, the Python entries' `complete` argument, and ro_run's FIX flag under the host sanitizers
(scripts/rollout_complete_host_check.cpp)."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from pyhybridcontrol_amd import gpu, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "include", "mldgpu.h")) as _f:
    HDR = _f.read()


def test_header_binding_and_exports_agree():
    assert re.search(r"int\s+mld_set_rollout_completion\s*\(\s*mld_problem_t\s*\*\s*p\s*,\s*int\s+mode\s*\)\s*;", HDR)
    assert re.search(r"int\s+mld_rollout_completion_stats\s*\(\s*mld_problem_t\s*\*\s*p\s*,\s*int64_t\s+out\[4\]\s*\)\s*;", HDR)
    for name, value in (("MLD_ROLLOUT_COMPLETE_DEVICE", 1), ("MLD_ROLLOUT_COMPLETE_DBG_FIRST_ONLY", 2)):
        m = re.search(r"#define\s+%s\s+(\d+)" % name, HDR)
        assert m and int(m.group(1)) == value == getattr(_lib, name), name
    lib = _lib.load()
    for name in ("mld_set_rollout_completion", "mld_rollout_completion_stats"):
        assert name in _lib.EXPORTS and hasattr(lib, name), name
    assert lib.mld_set_rollout_completion.argtypes == [C.c_void_p, C.c_int]
    assert lib.mld_rollout_completion_stats.argtypes == [C.c_void_p, C.POINTER(C.c_int64)]
    # the entries of the family keep their argument lists: the mode is the handle's, not an argument
    assert len(lib.mld_rollout_batch.argtypes) == 22 and len(lib.mld_warm_start_from_rollout.argtypes) == 8


def test_refusals_without_a_handle():
    lib = _lib.load()
    out = np.full(4, -7, np.int64)
    assert lib.mld_set_rollout_completion(None, 1) == -1 and b"mld_set_rollout_completion: p is NULL" in lib.mld_last_error()
    assert lib.mld_rollout_completion_stats(None, out.ctypes.data_as(C.POINTER(C.c_int64))) == -1 and b"mld_rollout_completion_stats: p is NULL" in lib.mld_last_error()
    assert np.all(out == -7)


def test_the_python_entries():
    """`complete` is the wrapper's keyword, the wrapped signatures are what they were; the word is tested before anything touches the handle"""
    for name in ("rollout", "select_plan", "select_plan_policies", "warm_start_from_rollout"):
        fn = getattr(gpu.GpuProblem, name)
        assert "complete" not in inspect.signature(fn).parameters and hasattr(fn, "__wrapped__") and "complete" in fn.__doc__, name
    for name, args in (("rollout", (None,)), ("select_plan", (None, None)), ("select_plan_policies", (None, None)), ("warm_start_from_rollout", (None,))):
        with pytest.raises(ValueError, match="complete = 'gpu'"):
            getattr(gpu.GpuProblem, name)(None, *args, complete="gpu")      # (self is never read)
    for name, args in (("select_plan_policies", (None, None)), ("warm_start_from_rollout", (None,))):
        with pytest.raises(ValueError, match="complete = 'host': %s\\(\\) has no host completion" % name):
            getattr(gpu.GpuProblem, name)(None, *args, complete="host")


def test_host_check_is_clean_under_the_sanitizers(tmp_path):
    """scripts/rollout_complete_host_check.cpp, its own executable: ro_run<., ., true> over a table, marks, slot and step of exactly the rule's lengths -- the
    empty table, a decline with the table empty, the rounds, a fix at step 0 and at step K - 1, a "no feasible point" mark -- under ASan and UBSan"""
    exe = str(tmp_path / "rollout_complete_host_check")
    cmd = ["c++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "pyhybridcontrol_amd", "csrc"),
           os.path.join(ROOT, "scripts", "rollout_complete_host_check.cpp"), "-o", exe]
    built = subprocess.run(cmd + ["-static-libasan", "-static-libubsan"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    if built.returncode != 0:
        built = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert built.returncode == 0, built.stdout
    ran = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert ran.returncode == 0 and "table, marks, slot and step as the rule states them, bit for bit" in ran.stdout, ran.stdout
    assert "first decline at step 0" in ran.stdout and re.search(r"first decline at step [1-9]", ran.stdout), ran.stdout      # both kinds of decline were met
