"""Golden fixture of the plant step with the whole step-0 slice: the REFERENCE's MldModel.lsim_k(x_k, v_k=, omega_k=) (models/mld_model.py:647-699)
on a few random models -> tests/golden/lsim_vk_ref.npz (read by tests/test_sim_step_host.py).

    python scripts/gen_lsim_golden.py

(The name does not start with ref_: tests/_golden.py reads every tests/golden/ref_*.npz as a condensing case.)  Needs the reference tree
(oracle/ref_harness.py imports it where it lies; nothing of it is copied).  Per model: the 20 matrices as handed to the reference, the dimensions, P points (x, v, omega) and every field lsim_k returns (x_k1, x, u, delta, z, mu, v, y, omega, cons).  The reference returns
`cons` only as truth values; the residual r = E x + F1 u + F2 delta + F3 z + F4 omega + G y - f5 is recomputed here from the REFERENCE model's own
matrices and the y it returned, with its expression (:692-694), stored as `resid`, and used to keep every point away from the threshold: a point is
redrawn until every |r_i - 1e-6| >= 1e-9, so that no rounding of another evaluation order can flip a truth value.  No point is left out.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ref_harness  # noqa: E402
from _paths import MAT_SHAPES, random_mld  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "lsim_vk_ref.npz")
POINTS = 8
MARGIN, TOL = 1e-9, 1e-6
# (seed, dims): a soft-constrained model (nmu > 0: the Psi term must drop out), one without outputs, one without constraint rows, one plain
MODELS = [(4101, dict(nx=3, nu=2, ndelta=1, nz=1, nmu=2, nomega=2, ny=2, nc=5)),
          (4102, dict(nx=4, nu=2, ndelta=1, nz=2, nomega=3, ny=0, nc=4)),
          (4103, dict(nx=2, nu=3, ndelta=1, nz=1, nomega=1, ny=2, nc=0)),
          (4104, dict(nx=5, nu=1, ndelta=2, nz=1, nomega=2, ny=3, nc=6))]
FIELDS = ("x_k1", "x", "u", "delta", "z", "mu", "v", "y", "omega", "cons")


def main():
    ref_harness.install()
    from models.mld_model import MldModel
    out = {"n_models": np.array(len(MODELS)), "points": np.array(POINTS)}
    truth = set()
    for k, (seed, dd) in enumerate(MODELS):
        mats, d, _ = random_mld(seed, **dd)
        given = {n: m for n, m in mats.items() if m.size}      # (the reference pads what is missing: models/mld_model.py:910-928)
        if d["ny"] == 0:
            given["C"] = np.zeros((0, d["nx"]))                 # an explicit empty C: without it the reference defaults C = I (:515-520)
        ref = MldModel(dict(given), ts=1)
        info = ref.mld_info
        for n in ("nx", "nu", "ndelta", "nz", "nmu", "nomega", "ny"):
            assert int(info[n]) == d[n], (k, n, int(info[n]), d[n])
        assert int(info["n_constraints"]) == d["nc"], (k, int(info["n_constraints"]), d["nc"])
        rng = np.random.default_rng(seed + 50)
        rec = {f: [] for f in FIELDS + ("resid",)}
        draws = 0
        while len(rec["x"]) < POINTS:
            draws += 1
            assert draws <= 100 * POINTS, "no point with every residual %g away from the threshold in %d draws" % (MARGIN, draws)
            x, v, w = rng.standard_normal(d["nx"]), rng.standard_normal(d["nv"]), rng.standard_normal(d["nomega"])
            v[d["nu"]:d["nu"] + d["ndelta"]] = rng.integers(0, 2, d["ndelta"])
            r = ref.lsim_k(x_k=x, v_k=v, omega_k=w)
            u_, dl_, z_ = (np.asarray(r[n], dtype=np.float64) for n in ("u", "delta", "z"))
            resid = (ref.E @ r["x"] + ref.F1 @ u_ + ref.F2 @ dl_ + ref.F3 @ z_ + ref.F4 @ r["omega"] + ref.G @ r["y"] - ref.f5) if d["nc"] else np.zeros((0, 1))
            resid = np.asarray(resid, dtype=np.float64).reshape(d["nc"])
            if d["nc"] and np.abs(resid - TOL).min() < MARGIN:
                continue                                           # redrawn, not dropped: the loop runs until POINTS points are in
            cons = np.asarray(r["cons"]).reshape(d["nc"])
            assert np.array_equal(cons, resid <= TOL), (k, cons, resid)
            truth |= set(bool(c) for c in cons)
            for f in FIELDS:
                rec[f].append(np.asarray(r[f], dtype=bool if f == "cons" else np.float64).reshape(-1))
            rec["resid"].append(resid)
        assert len(rec["x"]) == POINTS
        for n in MAT_SHAPES:
            out["m%d_%s" % (k, n)] = np.asarray(mats[n], dtype=np.float64)
        out["m%d_dims" % k] = np.array([d[n] for n in ("nx", "nu", "ndelta", "nz", "nmu", "nomega", "ny", "nc")], dtype=np.int32)
        for f, rows in rec.items():
            out["m%d_%s" % (k, f)] = np.stack(rows)
    assert truth == {True, False}, "both truth values of cons must occur: %s" % truth
    ref_harness.uninstall()
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
