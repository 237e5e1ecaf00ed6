"""Host side of the per-instance linear cost (mld_upload_instance_cost): host.instance_costs against cost_from_atoms, the
refusal of quadratic atoms, the shape checks of GpuProblem.upload_instance_cost (made before any C call), and the absence of a CPU
fallback.  No GPU needed."""
import types

import numpy as np
import pytest

from pyhybridcontrol_amd import gpu, host, synthetic as syn, _lib


def _atoms_list(wl, ag, B, seed=3):
    rng = np.random.default_rng(seed)
    d, N = ag["dims"], wl["N_tilde"]
    out = []
    for _ in range(B):
        a = dict(ag["atoms"])
        a["q_z"] = a["q_z"] * rng.uniform(0.5, 2.0)
        a["q_y"] = 0.1 * a["q_z"] * rng.uniform(0, 1, size=a["q_z"].shape)
        a["q_x"] = 1e-6 * rng.uniform(0, 1, size=(N * d["nx"], 1))
        out.append(a)
    return out


def test_instance_costs_equal_cost_from_atoms_per_instance():
    wl = syn.make_workload("cfg2", batch=4)
    ag = wl["agents"][0]
    d, N_p, N = ag["dims"], wl["N_p"], wl["N_tilde"]
    atoms = _atoms_list(wl, ag, 5)
    got = host.instance_costs(atoms, d, N_p, N)
    for k, ln in (("lin_v", N * (d["nu"] + d["ndelta"] + d["nz"] + d["nmu"])), ("lin_x", N * d["nx"]), ("lin_y", N * d["ny"])):
        assert got[k].shape == (5, ln) and got[k].dtype == np.float64
        for i, a in enumerate(atoms):
            assert np.array_equal(got[k][i], host.cost_from_atoms(a, d, N_p, N)[k]), (k, i)
    # a family nobody weighs is None (lin_v only: nothing to pull back)
    only_v = host.instance_costs([{"q_z": a["q_z"]} for a in atoms], d, N_p, N)
    assert only_v["lin_x"] is None and only_v["lin_y"] is None
    assert np.array_equal(only_v["lin_v"][2], host.cost_from_atoms({"q_z": atoms[2]["q_z"]}, d, N_p, N)["lin_v"])
    assert np.count_nonzero(only_v["lin_v"][0]) == N * d["nz"]


def test_instance_costs_refuse_a_quadratic_atom_by_name():
    wl = syn.make_workload("cfg2", batch=2)
    ag = wl["agents"][0]
    d = ag["dims"]
    atoms = [dict(ag["atoms"]), dict(ag["atoms"], Q_x=1e-3 * np.eye(d["nx"]))]
    with pytest.raises(ValueError, match="Q_x"):
        host.instance_costs(atoms, d, wl["N_p"], wl["N_tilde"])


@pytest.mark.parametrize("key,val", [("q_du", np.ones(3)), ("q_omega", np.ones(4)), ("q_L1_x", np.ones(3)), ("q_Linf_u", np.ones(3)), ("q_L22_x", np.ones(3))])
def test_instance_costs_refuse_what_a_linear_cost_cannot_carry(key, val):
    """rate atoms, epigraph atoms and atoms on omega are left out of a cost dict by cost_from_atoms (they live elsewhere): a per-instance cost
    that silently lacked them would be another objective, so they are refused by name"""
    wl = syn.make_workload("cfg2", batch=2)
    ag = wl["agents"][0]
    with pytest.raises(ValueError, match=key):
        host.instance_costs([dict(ag["atoms"]), dict(ag["atoms"], **{key: val})], ag["dims"], wl["N_p"], wl["N_tilde"])


def _shell(batch, nx=3, ny=1, nv=11, N=5):
    """a GpuProblem without a handle: what the shape checks read"""
    p = gpu.GpuProblem.__new__(gpu.GpuProblem)
    p.model = types.SimpleNamespace(dims=dict(nx=nx, ny=ny), nv=nv)
    p.N_tilde, p.n, p.batch, p._h = N, N * nv, batch, None
    return p


def test_shape_errors_raise_before_any_c_call():
    p = _shell(4)
    good = p._inst_cost_arrays(lin_v=np.ones(55), lin_x=np.ones((4, 15)), lin_y=np.ones((5, 1)))
    assert [a.shape for a in good] == [(4, 55), (4, 15), (4, 5)] and all(a.flags["C_CONTIGUOUS"] for a in good)
    assert p._inst_cost_arrays() == [None, None, None]
    for kw in (dict(lin_v=np.ones(54)), dict(lin_v=np.ones((3, 55))), dict(lin_x=np.ones((4, 16))), dict(lin_y=np.ones((4, 5, 1))),
               dict(lin_v=np.ones((4, 55)), lin_y=np.ones(6))):
        with pytest.raises(ValueError):
            p.upload_instance_cost(**kw)            # (_h is None: a C call would have raised MldGpuError instead)
    with pytest.raises(ValueError, match="lin_x"):
        _shell(4, nx=0).upload_instance_cost(lin_x=np.ones((4, 0)))
    with pytest.raises(ValueError, match="lin_y"):
        _shell(4, ny=0).upload_instance_cost(lin_y=np.ones(5))


def test_no_cpu_fallback_for_the_instance_cost():
    if _lib.device_count() > 0:
        pytest.skip("a GPU is present")
    with pytest.raises(gpu.MldGpuError, match="no HIP device"):
        _shell(4).upload_instance_cost(lin_v=np.ones(55))


def test_new_entry_points_are_declared_and_exported():
    lib = _lib.load()
    for name in ("mld_upload_instance_cost", "mld_download_instance_cost"):
        assert name in _lib.EXPORTS and hasattr(lib, name)
