"""What every entry point that changes the inputs of a resident batch leaves of the state that belongs to the previous inputs: the extra constraint
blocks, the MIP start and the plan of the last solve (the input-state transitions of the handle, csrc/handle.inc).  Observed from outside only:
mld_debug_warm_start (has_warm), mld_download_constraint_blocks (n_cols_out), and whether mld_predict_batch(v = NULL) is accepted, refused with "not been
solved" or refused with "moved the inputs on".  Every case starts from a batch with resident blocks, a set start and a finished solve.

Model: the smallest golden one with binaries and a disturbance (ref_dewh_N3: nx 1, nv 3, one binary per step, nomega 1, N 3), batch 3, a profile library
of N + 1 values -- with start 0 just long enough for the windows of steps 0 and 1.  Nothing here is arithmetic: flags, counts and np.array_equal."""
import os

import numpy as np
import pytest

import _golden as g
from pyhybridcontrol_amd import gpu

pytestmark = pytest.mark.gpu

B = 3
SOLVED, UNSOLVED, MOVED_ON = "accepted", "not been solved", "moved the inputs on"


@pytest.fixture(scope="module")
def handle():
    _, mats, d, N_p, N = g.load_case(os.path.join(g.GDIR, "ref_dewh_N3.npz"))
    m = gpu.GpuModel([mats], d)
    p = gpu.GpuProblem(m, N_p, N, None)
    rng = np.random.default_rng(7300)
    data = dict(N=N, nv=m.nv, m0=N * d["nc"], x0=50.0 + rng.random((B, d["nx"])), om=rng.random((B, N * d["nomega"])),
                cols=rng.random((B, 2, N * d["nomega"])), rows=np.array([N * d["nc"], 1], np.int32),
                warm=rng.integers(0, 2, (B, p.n_bin)).astype(np.uint8), lib=rng.random(N + 1), start=np.zeros((B, 1), np.int64))
    p.upload(data["x0"], data["om"])
    p.upload_profiles(data["lib"])                                 # owned by the problem: no upload of a batch touches it
    yield p, data
    p.close(); m.close()


def _prime(p, data):
    """a new batch with resident blocks, a set start and a finished solve"""
    p.upload(data["x0"], data["om"])
    p.upload_constraint_blocks(data["cols"], data["rows"])
    p.set_warm_start(data["warm"])
    p.solve_resident()
    assert _state(p) == (2, True, SOLVED)


def _plan(p):
    try:
        p.trajectories()
        return SOLVED
    except gpu.MldGpuError as e:
        for text in (UNSOLVED, MOVED_ON):
            if text in str(e):
                return text
        raise


def _state(p):
    """(resident block columns, a start is set, what mld_predict_batch says of the resident plan)"""
    return p.constraint_blocks()["omega_cols"].shape[1], p.debug_warm_start() is not None, _plan(p)


def test_upload_batch(handle):
    p, data = handle
    _prime(p, data)
    p.upload(data["x0"], data["om"])
    assert _state(p) == (0, False, UNSOLVED)


def test_select_inputs(handle):
    p, data = handle
    _prime(p, data)
    p.stage(data["x0"][None], data["om"][None])                    # staging itself changes nothing
    assert _state(p) == (2, True, SOLVED)
    p.select(0)
    assert _state(p) == (0, False, UNSOLVED)


def test_forecast_before_an_advance(handle):
    p, data = handle
    _prime(p, data)
    p.forecast_from_profiles(data["start"], 0)
    assert _state(p) == (0, False, UNSOLVED)


def test_forecast_after_an_advance(handle):
    """only the forecast is replaced: the start built from the plan stays, and the plan is still the one that has been applied"""
    p, data = handle
    _prime(p, data)
    p.advance()
    p.warm_start_from_previous(1)
    warm = p.debug_warm_start()
    assert _state(p) == (0, True, MOVED_ON)
    p.forecast_from_profiles(data["start"], 1)
    assert _state(p) == (0, True, MOVED_ON)
    assert np.array_equal(p.debug_warm_start(), warm)
    assert np.array_equal(p.inputs()[1], np.tile(data["lib"][1:1 + data["N"]], (B, 1)))


def test_advance_batch(handle):
    p, data = handle
    _prime(p, data)
    p.advance()
    assert _state(p) == (0, False, MOVED_ON)


def test_sim_step_advance_with_the_resident_plan(handle):
    p, data = handle
    _prime(p, data)
    p.sim_step(advance=True, log=False)
    assert _state(p) == (0, False, MOVED_ON)


def test_sim_step_advance_with_the_callers_v0(handle):
    p, data = handle
    _prime(p, data)
    p.sim_step(v0=np.zeros(data["nv"]), advance=True, log=False)
    assert _state(p) == (0, False, UNSOLVED)


def test_sim_step_without_advance(handle):
    p, data = handle
    _prime(p, data)
    warm, blocks, inputs = p.debug_warm_start(), p.constraint_blocks(), p.inputs()
    p.sim_step(advance=False, log=False, outputs=True)
    p.sim_step(v0=np.zeros(data["nv"]), advance=False, log=False, outputs=True)
    assert _state(p) == (2, True, SOLVED)
    assert np.array_equal(p.debug_warm_start(), warm) and np.array_equal(warm, data["warm"])
    after = p.constraint_blocks()
    assert np.array_equal(after["omega_cols"], blocks["omega_cols"]) and np.array_equal(after["col_rows"], blocks["col_rows"])
    assert np.array_equal(p.inputs()[0], inputs[0]) and np.array_equal(p.inputs()[1], inputs[1])


def test_refused_col_rows_leave_the_blocks(handle):
    """mld_upload_constraint_blocks: an entry of col_rows outside [0, m0] is named, and the resident blocks stay as they were"""
    p, data = handle
    _prime(p, data)
    for bad in (data["m0"] + 1, -1):
        with pytest.raises(gpu.MldGpuError, match=r"col_rows\[1\]"):
            p.upload_constraint_blocks(data["cols"][:, ::-1], [0, bad])
        assert _state(p) == (2, True, SOLVED)
        got = p.constraint_blocks()
        assert np.array_equal(got["omega_cols"], data["cols"]) and np.array_equal(got["col_rows"], data["rows"]) and got["x_cols"] is None
