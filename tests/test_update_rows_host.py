"""Host side of the internal entry mld_debug_update_rows (the rows' update of one pivot of k_solve or of a fused pair on a caller-supplied
dictionary): bad arguments are refused before any device is touched, the shape query needs no device, and without a device there is no CPU
fallback.  No GPU needed."""
import numpy as np
import pytest

from pyhybridcontrol_amd import gpu, _lib
from pyhybridcontrol_amd._lib import MLD_DBG_UPDATE_R7, MLD_DBG_PIVOT_SYNC_R5

M, LD = 12, 24
N = LD - 1


def _good():
    rng = np.random.default_rng(0)
    rowr = np.zeros(N + 1)
    rowr[:8] = rng.standard_normal(8)
    colc = rng.standard_normal(M)
    return dict(D=rng.standard_normal((M, LD)), n=N, rowr=rowr, colc=colc, r=3, c=2)


def test_shape_query_needs_no_device():
    s = gpu.debug_update_shape()
    assert len(s["RB"]) == 4 and all(isinstance(rb, int) and rb >= 1 for rb in s["RB"]), s      # rows a wave takes at a time with 1, 2, 3, 4 groups of sectors
    assert s["RB"] == sorted(s["RB"], reverse=True), s      # (more groups per row: fewer rows at a time, the registers are the same)
    assert s["waves"] >= 1 and s["sectors_per_group"] * s["sector_doubles"] * 8 == 1024 and s["groups_per_chunk"] == 4, s


@pytest.mark.parametrize("change", [
    dict(D=np.zeros((1, LD)), colc=np.ones(1), r=0),            # fewer than two rows
    dict(D=np.zeros((1025, LD)), colc=np.ones(1025)),           # more rows than the kernel's LDS holds
    dict(D=np.zeros((M, LD + 4)), n=N + 4, rowr=np.zeros(N + 5)),    # ld no multiple of 8
    dict(D=np.zeros((M, 1032)), n=1031, rowr=np.zeros(1032)),   # ld past the kernel's LDS
    dict(D=np.zeros((M, LD + 8))),                              # ld is not n + 1 rounded up: a whole sector of padding
    dict(r=-1), dict(r=M), dict(c=-1), dict(c=N),               # the pivot outside the dictionary (column n is the right-hand side)
    dict(reserved=1), dict(reserved=MLD_DBG_UPDATE_R7 | (1 << 27)),      # only bits 26 and 28 select a path here
    dict(second=(np.zeros(N + 1), np.zeros(M), M, 1)), dict(second=(np.zeros(N + 1), np.zeros(M), 1, N)), dict(second=(np.zeros(N + 1), np.zeros(M), -1, 0)),
])
def test_bad_arguments_are_refused_before_any_device_call(change):
    kw = dict(_good(), **change)
    with pytest.raises(gpu.MldGpuError, match="bad arguments"):
        gpu.debug_update_rows(**kw)


def test_wrapper_checks_the_staged_arrays():
    g = _good()
    for change in (dict(rowr=np.zeros(N)), dict(colc=np.zeros(M + 1)), dict(D=np.zeros(LD)), dict(second=(np.zeros(N), np.zeros(M), 1, 1)),
                   dict(second=(np.zeros(N + 1), np.zeros(M - 1), 1, 1))):
        with pytest.raises(ValueError):
            gpu.debug_update_rows(**dict(g, **change))


@pytest.mark.parametrize("reserved", (0, MLD_DBG_UPDATE_R7, MLD_DBG_UPDATE_R7 | MLD_DBG_PIVOT_SYNC_R5))
def test_good_arguments_reach_the_device_or_say_there_is_none(reserved):
    g = _good()
    if _lib.device_count() > 0:
        out, pairs = gpu.debug_update_rows(reserved=reserved, **g)
        assert out.shape == (M, LD) and pairs == (M - 1) * 1      # every row but the pivot's has a multiplier; one active sector
        return
    with pytest.raises(gpu.MldGpuError, match="no HIP device"):
        gpu.debug_update_rows(reserved=reserved, **g)
