"""Models with HARD rows, whose instances can be truly infeasible (tests/test_gpu_hard_rows.py; checked by tests/test_hard_refs.py): the seeded models
of _paths.fuzz_mld with the slack taken off a chosen set of rows, a product-shaped tank model with every slack taken off, and a classification of
each instance by scipy's HiGHS with a margin -- an instance counts as feasible only if it stays feasible with every row tightened by 1e-3 of its
scale, as infeasible only if it stays infeasible with every row loosened by as much; what lies between is dropped, because there "infeasible" is a
matter of tolerance and two correct solvers may disagree.  CPU only."""
import numpy as np
from scipy.optimize import Bounds, LinearConstraint, linprog, milp

import _aux_ref
import condense_np as cn
import tighten_np
from _paths import fuzz_mld

MARGIN = 1e-3           # of the row scale: the guard between "feasible" and "infeasible"
RESID = 1e-6            # of the row scale: the residual tests/test_gpu_fuzz.py accepts on a returned point
MAX_DROPPED = 0.05      # of a family's instances
NB = 6                  # instances per seed

# family -> (hard rows of a model with nc rows, N_tilde, scale of x0)
FAMILIES = {"F5": (lambda nc: range(1, nc), 5, 1.5),
            "F8": (lambda nc: range(0, nc, 2), 8, 2.0)}
SEEDS = range(12)
F5_ROUTE_SEEDS = (1, 4, 9, 11, 0, 2)      # the F5 seeds with infeasible instances (HiGHS) and two without: the modes of tests/test_gpu_hard_rows.py item 2


def hard_variant(mats, dims, atoms, hard_rows):
    """the model with the slack of `hard_rows` taken away: Psi = -I[:, soft], nmu = len(soft), q_mu = q_mu[soft]; everything else as drawn"""
    nc = dims["nc"]
    hard = set(int(i) for i in hard_rows)
    soft = [i for i in range(nc) if i not in hard]
    m = dict(mats, Psi=-np.eye(nc)[:, soft])
    a = dict(atoms)
    a["q_mu"] = np.asarray(atoms["q_mu"], float)[soft]
    if not soft:
        del a["q_mu"]
    return m, dict(dims, nmu=len(soft)), a


def family_instances(family, seed, N=None, xs=None):
    """(mats, dims, atoms, N_p, N, x0 (6, nx), om (6, N nomega)) of one seed; N / xs override the family's (the small-problem path's horizon)"""
    rows, N_f, xs_f = FAMILIES[family]
    N = N_f if N is None else N
    xs = xs_f if xs is None else xs
    mats, dims, atoms, rng = fuzz_mld(seed)
    mats, dims, atoms = hard_variant(mats, dims, atoms, rows(dims["nc"]))
    x0 = xs * rng.standard_normal((NB, dims["nx"]))
    om = rng.standard_normal((NB, N * dims["nomega"]))
    return mats, dims, atoms, N - 1, N, x0, om


def t3_instances():
    """T3: three tanks, N_tilde = 6, 24 scenarios, every comfort bound hard; tanks drawn around T_min and the draws tripled"""
    from pyhybridcontrol_amd import synthetic
    rng = np.random.default_rng(9109)
    mats, dims, params = synthetic.make_agent(3, rng, tie=False)
    atoms = synthetic.make_cost(3, 6, params, tie=False)
    x0, om = synthetic.make_scenarios(3, 6, 24, rng, tie=False)
    x0 = rng.uniform(49.5, 54.0, x0.shape)
    nw = dims["nomega"]
    om = om.reshape(24, 6, nw).copy()
    om[:, :, :3] *= 3.0
    om = om.reshape(24, 6 * nw)
    mats, dims = _aux_ref.hard_variant(mats, dims)
    atoms = {k: v for k, v in atoms.items() if k != "q_mu"}
    return mats, dims, atoms, 5, 6, x0, om


def row_scale(G):
    return np.maximum(1.0, np.abs(G).max(axis=1))


def _milp(raw, h, q):
    return milp(q, constraints=LinearConstraint(raw["G"], -np.inf, h), integrality=raw["is_bin"].astype(int), bounds=Bounds(raw["lb"], raw["ub"]),
                options=dict(mip_rel_gap=0.0))


def classify(raw, h, q):
    """three HiGHS solves on the ORIGINAL rows, at h - 1e-3 rs, h and h + 1e-3 rs.  Returns dict(cls = "feasible" | "infeasible" | "dropped") and, for a
    feasible instance, opt = the optimum at h, lo = the optimum at h + 1e-6 rs (what a point with residuals within 1e-6 rs can reach) and x = HiGHS's
    optimal point at h"""
    rs = row_scale(raw["G"])
    if _milp(raw, h - MARGIN * rs, q).status == 0:
        mid, lo = _milp(raw, h, q), _milp(raw, h + RESID * rs, q)
        assert mid.status == 0 and lo.status == 0, (mid.status, lo.status)          # (a looser right-hand side cannot lose the optimum)
        return dict(cls="feasible", opt=float(mid.fun), lo=float(lo.fun), x=mid.x)
    return dict(cls="infeasible" if _milp(raw, h + MARGIN * rs, q).status == 2 else "dropped")


def classify_lp(raw, h, q, lb, ub):
    """classify for an LP (the binaries fixed through lb = ub): scipy's linprog, the same margin"""
    rs = row_scale(raw["G"])
    lp = lambda hh: linprog(q, A_ub=raw["G"], b_ub=hh, bounds=np.stack([lb, ub], axis=1), method="highs")
    if lp(h - MARGIN * rs).status == 0:
        mid, lo = lp(h), lp(h + RESID * rs)
        assert mid.status == 0 and lo.status == 0, (mid.status, lo.status)
        return dict(cls="feasible", opt=float(mid.fun), lo=float(lo.fun), x=mid.x)
    return dict(cls="infeasible" if lp(h + MARGIN * rs).status == 2 else "dropped")


_cache = {}


def reference(family, seed=0, N=None, xs=None):
    """everything the tests need of one (family, seed), computed once and shared: the instances, the standard forms on the original (raw) and on the
    tightened rows, and per instance h, q, the cost constant r and the classification"""
    key = (family, seed, N, xs)
    if key in _cache:
        return _cache[key]
    mats, dims, atoms, N_p, N_t, x0, om = t3_instances() if family == "T3" else family_instances(family, seed, N, xs)
    nu_l = dims["nu_l"]
    raw = cn.standard_form(mats, atoms, N_p, N_t, nu_l=nu_l)
    tight = cn.standard_form(tighten_np.tighten(mats, dims, nu_l=nu_l), atoms, N_p, N_t, nu_l=nu_l)
    inst = []
    for s in range(len(x0)):
        w = om[s] if dims["nomega"] else np.zeros(0)
        h, q = cn.rhs(raw["evo"], x0[s], w), cn.lin_cost(raw["cost"], x0[s], w)
        c = classify(raw, h, q)
        c.update(h=h, q=q, r=cn.cost_const(raw["cost"]["const_terms"], x0[s], w), w=w,
                 ht=cn.rhs(tight["evo"], x0[s], w), qt=cn.lin_cost(tight["cost"], x0[s], w))
        inst.append(c)
    ref = dict(mats=mats, dims=dims, atoms=atoms, N_p=N_p, N=N_t, x0=x0, om=om, raw=raw, tight=tight, rs=row_scale(raw["G"]), inst=inst)
    _cache[key] = ref
    return ref


def counts(refs):
    """(feasible, infeasible, dropped) over a list of reference() results"""
    cl = [c["cls"] for r in refs for c in r["inst"]]
    return cl.count("feasible"), cl.count("infeasible"), cl.count("dropped")


def sandwich(c, obj):
    """lo + r - 1e-6 s <= obj <= opt + r + 1e-6 s, s = max(1, |opt + r|); returns (ok, (obj - opt - r) / s)"""
    tot = c["opt"] + c["r"]
    s = max(1.0, abs(tot))
    return (c["lo"] + c["r"] - RESID * s <= obj <= tot + RESID * s), (obj - tot) / s
