"""The CPU references of tests/test_gpu_kernel_paths.py checked on their own (no GPU): the random MLD generator hits the
requested dimensions and spectral radius, and ref_cost (K4 written out from the condensed maps) equals the oracle's
atom-driven cost assembly, non-symmetric matrix weights included."""
import numpy as np
import pytest

import _paths
import condense_np as cn
from pyhybridcontrol_amd import host


@pytest.mark.parametrize("dims", [dict(nx=4, nu=2, ndelta=1, nz=1, nmu=2, nomega=3, ny=2, nc=5),
                                  dict(nx=17, nu=3, nomega=0, ny=0, nc=4),
                                  dict(nx=0, nu=5, nomega=4, ny=3, nc=4),
                                  dict(nx=3, nu=1, ndelta=0, nz=0, nmu=0, nomega=2, ny=1, nc=2)])
def test_random_mld_hits_requested_dims_and_spectral_radius(dims):
    for seed in range(3):
        mats, d, rho = _paths.random_mld(seed, **dims)
        got = cn.mld_dims(mats)
        for k in ("nx", "nu", "ndelta", "nz", "nmu", "nomega", "ny", "nc", "nv"):
            assert got[k] == d[k], (k, got[k], d[k])
        for name, (r, c) in _paths.MAT_SHAPES.items():
            assert mats[name].shape == (d[r], d[c] if isinstance(c, str) else c), name
        if d["nx"]:
            assert 0.9 <= rho <= 1.05
            assert abs(_paths.spectral_radius(mats["A"]) - rho) <= 1e-12
    _, _, rho = _paths.random_mld(0, rho=0.95, **dims)
    assert rho == 0.95
    ms, d = _paths.random_horizon(5, 4, **dims)
    assert len(ms) == 4 and not np.array_equal(ms[0]["F1"], ms[1]["F1"])


@pytest.mark.parametrize("time_varying", [False, True], ids=["ti", "tv"])
def test_ref_cost_equals_atom_cost_assembly(time_varying):
    """non-symmetric matrix weights on x, y and u, vector weights on x, y, z, a linear atom on mu"""
    N_p, N = 5, 6
    mats, d, _ = _paths.random_mld(3, nx=3, nu=2, ndelta=1, nz=1, nmu=2, nomega=2, ny=2, nc=4)
    rng = np.random.default_rng(4)
    atoms = {"Q_x": rng.standard_normal((3, 3)), "q_x": rng.standard_normal(3), "Q_y": rng.standard_normal((2, 2)),
             "q_Quadratic_y": rng.standard_normal(2), "q_y": rng.standard_normal(2), "Q_u": rng.standard_normal((2, 2)),
             "q_z": rng.standard_normal(1), "q_mu": rng.standard_normal(2)}
    assert not np.allclose(atoms["Q_x"], atoms["Q_x"].T)
    if time_varying:
        ms, _ = _paths.random_horizon(7, N, nx=3, nu=2, ndelta=1, nz=1, nmu=2, nomega=2, ny=2, nc=4)
        evo = cn.condense_tv(ms)
    else:
        evo = cn.condense(mats, N)
    ref = cn.assemble_cost(cn.build_weights(atoms, evo["dims"], N_p, N), evo, evo["dims"], N)
    cost = host.cost_from_atoms(atoms, d, N_p, N)
    assert cost["quad_x"] is not None and not np.allclose(cost["quad_x"], cost["quad_x"].T)
    got = _paths.ref_cost(evo, **{k: cost.get(k) for k in ("lin_v", "lin_x", "lin_y", "quad_v", "quad_x", "quad_y")})
    for k in ("P", "q0", "Qx", "Qw"):
        scale = np.abs(ref[k]).max()
        assert scale > 0, k
        assert np.abs(got[k] - ref[k]).max() <= 1e-13 * scale, k


def test_rhs_terms_and_fp32_bound():
    mats, d, _ = _paths.random_mld(1, nx=3, nu=2, nomega=2, ny=1, nc=3)
    evo = cn.condense(mats, 4)
    rng = np.random.default_rng(2)
    x0, om = rng.standard_normal((5, 3)), rng.standard_normal((5, 8))
    h, s = _paths.rhs_terms(evo, x0, om)
    for b in range(5):
        assert np.allclose(h[b], cn.rhs(evo, x0[b], om[b]), rtol=0, atol=1e-14)
    assert np.all(s >= np.abs(h) - 1e-14)
    # the bound really bounds an fp32 evaluation of the same rows
    z = np.hstack([x0, om, np.ones((5, 1))]).astype(np.float32)
    H = np.hstack([evo["H_x"], evo["H_omega"], evo["H_5"]]).astype(np.float32)
    h32 = (z @ H.T).astype(np.float64)
    assert np.all(np.abs(h32 - h) <= _paths.fp32_dot_bound(12) * s)
    assert _paths.fp32_dot_bound(318) == pytest.approx(320 * 2.0 ** -24, rel=1e-4)
