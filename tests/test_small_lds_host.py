"""The small-problem path (MLD_SMALL_LDS, k_small_milp) at the boundary of the library, without a GPU: the header and the binding agree on the new names,
the options struct kept its size, and the new entry point follows the conventions of the others."""
import ctypes as C
import os
import re

from pyhybridcontrol_amd import _lib
from pyhybridcontrol_amd.aux_resolve import AuxResolver, BatchAuxResolver

HDR = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mldgpu.h")).read()


def test_header_and_binding_agree_on_the_new_names():
    assert int(re.search(r"#define\s+MLD_SMALL_LDS\s+(\d+)", HDR).group(1)) == _lib.MLD_SMALL_LDS == 2
    assert _lib.MLD_SMALL_LDS & _lib.MLD_F32 == 0                                     # the two flags compose
    m = re.search(r"MLD_DBG_SMALL_PIVOT_CAP\s*=\s*1\s*<<\s*(\d+)", HDR)
    assert 1 << int(m.group(1)) == _lib.MLD_DBG_SMALL_PIVOT_CAP == 1 << 25
    bits = [int(b) for b in re.findall(r"MLD_DBG_[A-Z0-9_]+\s*=\s*1\s*<<\s*(\d+)", HDR)]
    assert len(bits) == len(set(bits))                                                # no diagnostic bit is taken twice
    assert re.search(r"int\s+mld_small_lds_stats\s*\(\s*mld_problem_t\s*\*\s*,\s*int64_t\s+out\[3\]\s*\)\s*;", HDR)
    assert "mld_small_lds_stats" in _lib.EXPORTS and hasattr(_lib.load(), "mld_small_lds_stats")


def test_opts_size_is_unchanged():
    assert int(_lib.load().mld_opts_size()) == C.sizeof(_lib.Opts) == 64
    assert "sizeof(mld_opts) = 64" in _lib.version()


def test_stats_entry_point_without_a_device_or_a_handle():
    lib = _lib.load()
    out = (C.c_int64 * 3)(7, 7, 7)
    rc = lib.mld_small_lds_stats(None, out)
    if _lib.device_count() < 1:
        assert rc == -2 and b"no HIP device" in lib.mld_last_error()                  # MLD_ERR_NO_DEVICE, before anything else
    else:
        assert rc == -1                                                               # MLD_ERR_INVALID: no handle
    assert list(out) == [7, 7, 7]


def test_resolvers_take_the_keyword():
    # a model without auxiliaries builds no handle: the keyword is accepted and nothing needs a device
    mats = dict(A=[[0.9]], B1=[[1.0]], E=[[1.0]], F1=[[0.0]], f5=[[10.0]])
    dims = dict(nx=1, nu=1, ndelta=0, nz=0, nmu=0, nomega=0, ny=0, nc=1, nu_l=1, nmu_l=0)
    assert BatchAuxResolver([mats], dims, small_lds=True).problem is None
    assert AuxResolver(mats, dims, small_lds=True).nv2 == 0
