"""CPU tests of the plant step with re-derived auxiliaries (mld_sim_step_resolve / GpuProblem.sim_step(resolve=...), aux_resolve.BatchAuxResolver): the fold
of a list of models, the C ABI's declarations, the Python shape checks, and the closed form of tests/_aux_ref.py -- the reference for the device tests --
against the C oracle on the folded model (as tests/test_gpu_aux.py poses it)."""
import os
import re
import subprocess

import numpy as np
import pytest

import _aux_ref
import condense_np as cn
import orc
import pyhybridcontrol_amd as phc
from pyhybridcontrol_amd import _lib, aux_resolve, synthetic as syn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mld_sim_step_resolve", "mld_download_sim_log_aux")


def test_batch_resolver_folds_every_model_as_fold_known_does():
    wl = syn.make_workload("cfg2", batch=2, n_agents=3)
    d = wl["agents"][0]["dims"]
    mats = [a["mats"] for a in wl["agents"]]
    folded, d2 = aux_resolve.fold_models(mats, d)
    assert len(folded) == 3
    assert (d2["nu"], d2["nu_l"], d2["nomega"]) == (0, 0, d["nomega"] + d["nu"])
    assert all(d2[k] == d[k] for k in ("nx", "ny", "nc", "ndelta", "nz", "nmu", "nmu_l"))
    for m, f in zip(mats, folded):
        want, dw, known = aux_resolve.fold_known(m, d, ("delta", "z", "mu"))
        assert known == ["u"] and dw == d2 and set(f) == set(want)
        for k in want:
            assert (f[k] is None and want[k] is None) or np.array_equal(f[k], want[k]), k
        assert np.array_equal(f["B4"], np.hstack([m["B4"], m["B1"]])) and np.array_equal(f["D4"], np.hstack([m["D4"], m["D1"]]))
        assert np.array_equal(f["F4"], np.hstack([m["F4"], m["F1"]]))
    assert not np.array_equal(folded[0]["B4"], folded[1]["B4"])          # three models, not one three times


def test_batch_resolver_without_auxiliaries_builds_no_handle(monkeypatch):
    from pyhybridcontrol_amd import gpu
    built = []
    monkeypatch.setattr(gpu, "GpuModel", lambda *a, **k: built.append("model"))
    monkeypatch.setattr(gpu, "GpuProblem", lambda *a, **k: built.append("problem"))
    mats, d, _ = syn.make_agent(3, np.random.default_rng(5), tie=False)
    hard, dh = _aux_ref.hard_variant(mats, d)
    r = aux_resolve.BatchAuxResolver([hard, hard], dh)
    assert r.nv2 == 0 and r.problem is None and built == [] and r.dims2["nomega"] == d["nomega"] + d["nu"]
    out = r.resolve(np.zeros((4, 3)), np.zeros((4, 3)), np.zeros((4, 3)))
    assert out["v"].shape == (4, 0) and out["delta"].shape == (4, 0) and np.all(out["status"] == 0)
    r.close()
    soft = aux_resolve.BatchAuxResolver([mats], d, max_nodes=7)          # with auxiliaries: one model handle, one problem handle
    assert soft.nv2 == d["nmu"] and built == ["model", "problem"]


def test_the_two_entry_points_are_declared_listed_and_exported():
    with open(os.path.join(ROOT, "include", "mldgpu.h")) as f:
        header = f.read()
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(\s*mld_problem_t\s*\*" % name, header), name
        assert name in _lib.EXPORTS and hasattr(_lib.load(), name), name
        assert getattr(_lib.load(), name).argtypes is not None, name
    assert re.search(r"mld_sim_step_resolve\s*\(\s*mld_problem_t\s*\*\s*,\s*mld_problem_t\s*\*\s*aux\s*,\s*const double\s*\*\s*u0", header)
    assert "controller_base.py:229-253" in header and "mld_model.py:683-686" in header and ":701-766" in header      # declared with the reference lines they replace
    syms = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in NEW:
        assert re.search(r"\bT %s\b" % name, syms), name
    assert "auxiliaries re-derived" in _lib.version()


def test_sim_step_resolve_checks_shapes_first_and_has_no_cpu_fallback():
    from pyhybridcontrol_amd import gpu

    class _M(object):
        dims = dict(nx=2, nu=3, ndelta=1, nz=0, nmu=0, nomega=1, ny=1, nc=2, nu_l=0, nmu_l=0)
        nv = 4

    class _R(object):
        problem = None
    p = gpu.GpuProblem.__new__(gpu.GpuProblem)
    p.model, p.batch, p._h = _M(), 5, None
    with pytest.raises(ValueError, match="u0 has shape"):
        p.sim_step(resolve=_R(), u0=np.zeros((5, 2)))
    with pytest.raises(ValueError, match="resolve and v0 both given"):
        p.sim_step(resolve=_R(), v0=np.zeros(4))
    with pytest.raises(ValueError, match="u0 given without resolve"):
        p.sim_step(u0=np.zeros(3))
    expect = "no HIP device" if _lib.device_count() <= 0 else "no batch resident"
    for call in (lambda: p.sim_step(resolve=_R(), u0=np.zeros(3), log=False), lambda: p.sim_log_aux(0, 0)):
        with pytest.raises(phc.MldGpuError, match=expect):
            call()


@pytest.mark.parametrize("name", ["cfg2", "cfg3"])
def test_closed_form_equals_the_oracle_on_the_folded_model(name):
    """3 agents x 40 triples per shape; no triple is left out, and every |y| >= 1e-3 so that delta = [y >= 0] is unambiguous.  The closed form's point has
    the oracle's delta exactly, the oracle's optimal sum(mu) to 1e-6 max(1, sum(mu)), and satisfies the reference's own feasibility statement to 1e-6 max(1,
    max|x|): it is an optimal point of the auxiliary problem.  The oracle's OWN z is only printed: it sits on the big-M rows z = y to the oracle's
    tolerance at |y| of a few thousand (cfg3: worst residual 3.0 times that bound, |z - z_closed| <= 3.0e-7 max(1, |y|); cfg2: 1.3e-7 and 6e-14)."""
    wl = syn.make_workload(name, batch=16, n_agents=3)
    rng = np.random.default_rng(dict(cfg2=4102, cfg3=4103)[name])
    worst_z, worst_r, least_y = 0.0, 0.0, np.inf
    for ag in wl["agents"]:
        d, mats = ag["dims"], ag["mats"]
        x, u, om = _aux_ref.draw_triples(ag, 40, rng)
        cf = _aux_ref.closed_form(mats, d, x, u, om)
        assert np.all(np.abs(cf["y"]) >= 1e-3)
        least_y = min(least_y, float(np.abs(cf["y"]).min()))
        assert (cf["mu"] > 0).any() and (cf["delta"] == 0).any() and (cf["delta"] == 1).any()          # the draws reach both bounds and both signs
        m2, d2, _ = aux_resolve.fold_known(mats, d, ("delta", "z", "mu"))
        sf = cn.standard_form(m2, {"q_mu": np.ones((d2["nmu"], 1))}, 0, 1, nu_l=0)
        for s in range(40):
            w2 = np.concatenate([om[s], u[s]])
            ref = orc.solve_milp(cn.lin_cost(sf["cost"], x[s], w2), sf["G"], cn.rhs(sf["evo"], x[s], w2), sf["lb"], sf["ub"], sf["is_bin"], max_nodes=20000, presolve=0)
            assert ref["status"] == "optimal", s
            v = np.asarray(ref["x"])
            dl, z, mu = v[:1], v[1:2], v[2:]
            assert np.array_equal(dl, cf["delta"][s]), (s, dl, cf["y"][s])
            tot = cf["mu"][s].sum()
            assert abs(mu.sum() - tot) <= 1e-6 * max(1.0, tot) and abs(ref["obj"] - tot) <= 1e-6 * max(1.0, tot), (s, mu.sum(), ref["obj"], tot)
            bound = 1e-6 * max(1.0, np.abs(x[s]).max())
            assert _aux_ref.residual(mats, d, x[s], u[s], om[s], cf["delta"][s], cf["z"][s], cf["mu"][s]).max() <= bound, s
            worst_r = max(worst_r, _aux_ref.residual(mats, d, x[s], u[s], om[s], dl, z, mu).max() / bound)
            worst_z = max(worst_z, abs(z[0] - cf["z"][s, 0]) / max(1.0, abs(cf["y"][s])))
    print("%s: smallest |y| %.3g, worst |z - z_closed| / max(1, |y|) %.3g, worst residual of the oracle's own point / bound %.3g" % (name, least_y, worst_z, worst_r))
