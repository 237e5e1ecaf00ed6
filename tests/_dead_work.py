"""Pools of tests/test_gpu_dead_work_paths.py and of their CPU check tests/test_dead_work_pools.py: the instances (P35 of tests/_history.py, the
synthetic configurations), one handle layout per pool, and the oracle's verdict on a pool.  Importing this module needs no GPU; Pool.handle() does."""
import numpy as np

import condense_np as cn
import orc
import tighten_np
import _history as hist
from pyhybridcontrol_amd import host, synthetic as syn

GENEROUS = dict(max_nodes=50000, max_pivots=400000)          # (the budgets of tests/test_gpu_hard_rows.py)
# cfg3: the 16 of make_workload("cfg3", batch=64) on which the oracle makes the most nodes (at NodeLimit 50 five of them stop at the limit, at 800 one does)
CFG3_HARD = (4, 6, 13, 18, 19, 20, 23, 26, 32, 33, 39, 40, 52, 54, 57, 59)
Q_U = 0.05                                                   # the quadratic variant of P35: Q_u = 0.05 I (the small case of tests/test_gpu_miqp.py)

_pools = {}


class Pool(object):
    """instances that share one handle layout: models, cost, inputs, optional per-instance arrays (one row per instance), and per instance what the
    oracle needs (oracle[i] = dict(P or None, q, G, h, lb, ub, is_bin); None where the pool has no CPU restatement here)"""

    def __init__(self, name, mats_list, dims, cost, N_p, N, x0, om, midx=None, fixed=None, warm=None, cutoff=None, lin_v=None, oracle=None):
        self.name, self.mats_list, self.dims, self.cost, self.N_p, self.N = name, mats_list, dims, cost, N_p, N
        self.x0, self.om, self.midx, self.fixed, self.warm, self.cutoff, self.lin_v = x0, om, midx, fixed, warm, cutoff, lin_v
        self.oracle = oracle
        self.size = len(x0)

    def handle(self, **opts):
        return Handle(self, opts)

    def oracle_nodes(self, max_nodes, idx=None):
        """(nodes, node-limited count) of the oracle's search on the instances idx (all), NodeLimit max_nodes"""
        res = []
        for i in (range(self.size) if idx is None else idx):
            o = self.oracle[int(i)]
            args = (o["q"], o["G"], o["h"], o["lb"], o["ub"], o["is_bin"])
            res.append(orc.solve_miqp(o["P"], *args, max_nodes=max_nodes, presolve=0) if o["P"] is not None else orc.solve_milp(*args, max_nodes=max_nodes, presolve=0))
        return np.array([r["nodes"] for r in res]), sum(r["status"] == "node_limit" for r in res)


class Handle(object):
    def __init__(self, pool, opts):
        from pyhybridcontrol_amd import gpu
        self.pool = pool
        self.model = gpu.GpuModel(pool.mats_list, pool.dims)
        self.prob = gpu.GpuProblem(self.model, pool.N_p, pool.N, pool.cost, **opts)

    def run(self, idx):
        """the instances idx of the pool as one batch, in that order: results, rows_updated and the launch's statistics"""
        P, p = self.pool, self.prob
        idx = np.atleast_1d(np.asarray(idx, np.int64))
        pick = lambda a: None if a is None else np.ascontiguousarray(a[idx])
        p.upload(P.x0[idx], P.om[idx], pick(P.midx), pick(P.fixed))
        if P.lin_v is not None:
            p.upload_instance_cost(lin_v=pick(P.lin_v))
        p.set_warm_start(pick(P.warm))
        p.set_cutoffs(pick(P.cutoff))
        stats = p.solve_resident()
        out = p.download()
        out["rows_updated"] = p.telemetry()["rows_updated"].copy()
        out["stats"] = stats
        return out

    def close(self):
        self.prob.close()
        self.model.close()


def p35(variant="plain", N=hist.P35_N):
    """P35 of tests/_history.py on one six-model handle: "plain", "quadratic" (Q_u = 0.05 I) or "inputs" (fixings, MIP starts, cutoffs, a per-instance
    cost: no oracle restatement here, tests/test_gpu_history.py anchors those against HiGHS)"""
    key = ("p35", variant, N)
    if key in _pools:
        return _pools[key]
    P = hist.p35(N)
    d = P["dims"]
    costs, quadP = [], []
    for m in P["models"]:
        atoms = dict(m["atoms"])
        if variant == "quadratic":
            atoms["Q_u"] = Q_U * np.eye(d["nu"])
            quadP.append(cn.standard_form(m["mats"], atoms, P["N_p"], P["N"], nu_l=d["nu_l"])["cost"]["P"])
        costs.append(host.cost_from_atoms(atoms, d, P["N_p"], P["N"]))
    extra, oracle = {}, None
    if variant == "inputs":
        inp = hist.p35_inputs()
        extra = {k: inp[k] for k in ("fixed", "warm", "cutoff", "lin_v")}
    else:
        oracle = []
        for c in P["inst"]:
            raw = P["models"][c["model"]]["raw"]
            oracle.append(dict(P=quadP[c["model"]] if variant == "quadratic" else None, q=c["q"], G=raw["G"], h=c["h"], lb=raw["lb"], ub=raw["ub"], is_bin=raw["is_bin"]))
    pool = Pool("P35 %s%s" % (variant, "" if N == hist.P35_N else " N_tilde %d" % N), [m["mats"] for m in P["models"]], d, host.stack_costs(costs), P["N_p"], P["N"],
                P["x0"], P["om"], midx=P["midx"], oracle=oracle, **extra)
    _pools[key] = pool
    return pool


def medium(name, batch, n_agents=1, quadratic=False):
    """batch instances of each of n_agents models of a synthetic configuration, the models interleaved; the oracle sees the tightened model, as smoke() does"""
    key = (name, batch, n_agents, quadratic)
    if key in _pools:
        return _pools[key]
    wl = syn.make_workload(name, batch=batch, n_agents=n_agents, quadratic=quadratic)
    ags = wl["agents"]
    d = ags[0]["dims"]
    costs = [host.cost_from_atoms(a["atoms"], d, wl["N_p"], wl["N_tilde"]) for a in ags]
    x0, om = np.concatenate([a["x0"] for a in ags]), np.concatenate([a["omega"] for a in ags])
    oracle = []
    for a in ags:
        sf = cn.standard_form(tighten_np.tighten(a["mats"], d, nu_l=d["nu_l"]), a["atoms"], wl["N_p"], wl["N_tilde"], nu_l=d["nu_l"])
        for s in range(batch):
            oracle.append(dict(P=sf["cost"]["P"] if quadratic else None, q=cn.lin_cost(sf["cost"], a["x0"][s], a["omega"][s]), G=sf["G"],
                               h=cn.rhs(sf["evo"], a["x0"][s], a["omega"][s]), lb=sf["lb"], ub=sf["ub"], is_bin=sf["is_bin"]))
    midx = None
    if n_agents > 1:      # interleaved: every instance follows another model's
        perm = np.arange(n_agents * batch).reshape(n_agents, batch).T.ravel()
        x0, om, midx, oracle = x0[perm], om[perm], (perm // batch).astype(np.int32), [oracle[i] for i in perm]
    pool = Pool("%s x%d%s%s" % (name, batch, " MIQP" if quadratic else "", " %d models" % n_agents if n_agents > 1 else ""), [a["mats"] for a in ags], d,
                host.stack_costs(costs) if n_agents > 1 else costs[0], wl["N_p"], wl["N_tilde"], x0, om, midx=midx, oracle=oracle)
    _pools[key] = pool
    return pool
