"""Small host-side helpers shared by the controller mirror, the batch harness and the tests."""
import numpy as np

from .objective_atoms import ObjectiveAtoms


def cost_from_atoms(atoms, dims, N_p, N_tilde):
    """string-keyed objective atoms (reference syntax) -> tiled cost dict for gpu.GpuProblem"""
    oa = ObjectiveAtoms(dims, N_p, N_tilde, atoms)
    c = oa.to_cost()
    c.pop("_omega_atoms", None)
    return c


def instance_costs(atoms_list, dims, N_p, N_tilde):
    """one string-keyed atom dict per instance (reference syntax) -> dict(lin_v, lin_x, lin_y) of (batch, len) arrays for
    gpu.GpuProblem.upload_instance_cost; a family nobody weighs (or the model lacks) is None.  A per-instance cost is a linear
    weight on v, x or y: an atom that is anything else -- quadratic / L22, L1 / Linf (epigraph rows), a rate atom (lag-state
    augmentation), an atom on omega (a constant) -- raises ValueError naming it instead of being left out silently.  An atom whose
    weight the parser takes for zero (np.isclose(w, 0), as the reference's objective_atoms.py) contributes nothing, as in a model cost."""
    costs = []
    for i, atoms in enumerate(atoms_list):
        bad = []
        for key in atoms:
            for (var, atype, _wtype, rate) in ObjectiveAtoms(dims, N_p, N_tilde, {key: atoms[key]}).weights:
                if rate or atype != "Linear" or var == "omega":
                    bad.append("%r (%s%s on %s)" % (key, "rate " if rate else "", atype, var))
        if bad:
            raise ValueError("instance %d: a per-instance cost carries linear atoms on u, delta, z, mu, v, x, y only; got %s" % (i, ", ".join(bad)))
        costs.append(cost_from_atoms(atoms, dims, N_p, N_tilde))
    out = {}
    for k in ("lin_v", "lin_x", "lin_y"):
        a = np.stack([np.asarray(c[k], np.float64) for c in costs]) if costs else np.zeros((0, 0))
        out[k] = a if a.size and np.any(a) else None
    return out


def stack_costs(cost_list):
    """list of per-model cost dicts -> one dict of (n_models, ...) arrays (None where nobody has a term)"""
    out = {}
    for k in ("lin_v", "lin_x", "lin_y", "quad_v", "quad_x", "quad_y"):
        vals = [c.get(k) for c in cost_list]
        if all(v is None for v in vals):
            out[k] = None
            continue
        ref = next(v for v in vals if v is not None)
        out[k] = np.stack([np.zeros_like(ref) if v is None else np.asarray(v, np.float64) for v in vals])
    return out
