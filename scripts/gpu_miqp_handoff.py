"""MIQP with and without the in-kernel sub-tree hand-off on bench's MIQP workload (BASELINE cfg3 shape, Q_x = 1e-3 I): per gap, alternating runs
off / on in one process so that the spread is visible -- kernel ms, proven fraction, unfinished and given-up trees -- and batch-1 MpcController.solve()
p50 / p99 on the hardest 1 % of the instances (by nodes of the plain solve at the first gap), without and with handoff=...
   python scripts/gpu_miqp_handoff.py [n_inst=4096] [reps=2] [gaps=1e-2,1e-6] [out.json]"""
import json
import sys
import time

sys.path.insert(0, ".")
import numpy as np

import pyhybridcontrol_amd as phc
from pyhybridcontrol_amd import gpu, host, synthetic as syn

n_inst = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 2
gaps = [float(g) for g in (sys.argv[3] if len(sys.argv) > 3 else "1e-2,1e-6").split(",")]
out_path = sys.argv[4] if len(sys.argv) > 4 else None

# plain solve: NodeLimit / IterationLimit of bench's MIQP leg at gap 1e-2, of its 1e-6 contract leg at gap 1e-6; hand-off: the contract leg's settings
LIMITS = {True: dict(max_nodes=800, max_pivots=40000), False: dict(max_nodes=20000, max_pivots=400000)}
HAND = dict(first_nodes=400, sub_nodes=200, max_gen=8, max_children=64, max_tree=160, room_factor=3.0)
HO1 = dict(first_nodes=100, sub_nodes=200, max_gen=8, max_children=64, max_tree=160)

wl = syn.make_workload("cfg3", batch=n_inst, quadratic=True)
ag = wl["agents"][0]
d = ag["dims"]
m = gpu.GpuModel([ag["mats"]], d)
p = gpu.GpuProblem(m, wl["N_p"], wl["N_tilde"], host.cost_from_atoms(ag["atoms"], d, wl["N_p"], wl["N_tilde"]), gap_rel=gaps[0], **LIMITS[gaps[0] >= 1e-3])
res = dict(workload="BASELINE cfg3 shape (n_h=7, N_p=24), Q_x = 1e-3 I; %d instances" % n_inst, handoff=HAND, runs=[])


def save():
    if out_path:
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1)


plain_nodes = None
for gap in gaps:
    lim = LIMITS[gap >= 1e-3]
    p.set_opts(gap_rel=gap, **lim)
    p.solve(ag["x0"], ag["omega"])                     # (first solve at these options: learns the queue order)
    for r in range(reps):
        for ho in (False, True):
            if ho:
                out = p.solve_handoff_device(ag["x0"], ag["omega"], **HAND)
                hs = out["handoff"]
            else:
                out = p.solve(ag["x0"], ag["omega"])
                hs = dict(items=0, given_up=0, unfinished=int((out["status"] == 2).sum()), queue_full=0)
                if plain_nodes is None:
                    plain_nodes = out["nodes"].copy()
            row = dict(gap=gap, rep=r, handoff=ho, kernel_ms=round(float(out["stats"]["solve_ms"]), 1), proven_fraction=round(float((out["status"] == 0).mean()), 5),
                       unfinished=int(hs["unfinished"]), given_up=int(hs["given_up"]), items=int(hs["items"]), queue_full=int(hs["queue_full"]),
                       no_incumbent=int((~np.isfinite(out["obj"])).sum()), **({} if ho else dict(max_nodes=lim["max_nodes"])))
            res["runs"].append(row)
            print(json.dumps(row), flush=True)
            save()
p.close(); m.close()

# batch 1: MpcController.solve() on the hardest 1 % (nodes of the first plain solve), to the first gap, without and with the hand-off
hard = np.argsort(-plain_nodes, kind="stable")[: max(1, n_inst // 100)]
lat = {False: [], True: []}
proven = {False: 0, True: 0}
items = 0
for ho in (False, True):
    c = phc.MpcController(phc.MldModel(ag["mats"], nu_l=d["nu_l"]), N_p=wl["N_p"], handoff=(HO1 if ho else None), gap_rel=gaps[0], max_nodes=20000, max_pivots=400000)
    c.set_std_obj_atoms(**ag["atoms"])
    c.build()
    c.solve(0, x_k=ag["x0"][hard[0]], omega_tilde_k=ag["omega"][hard[0]], warm_start=False)      # (first call: allocations)
    for i in hard:
        t0 = time.perf_counter()
        c.solve(0, x_k=ag["x0"][i], omega_tilde_k=ag["omega"][i], warm_start=False)
        lat[ho].append((time.perf_counter() - t0) * 1e3)
        proven[ho] += c._status == "optimal"
        if ho:
            items += c._problem.handoff_stats()["items"]
    del c
pq = lambda a, f: round(float(np.sort(a)[min(len(a) - 1, int(len(a) * f))]), 2)
res["batch_1"] = dict(gap=gaps[0], calls=int(len(hard)), plain_nodes_min=int(plain_nodes[hard].min()), handoff=HO1, items=int(items),
                      off=dict(p50_ms=pq(lat[False], 0.5), p99_ms=pq(lat[False], 0.99), proven=int(proven[False])),
                      on=dict(p50_ms=pq(lat[True], 0.5), p99_ms=pq(lat[True], 0.99), proven=int(proven[True])))
print(json.dumps(res["batch_1"]), flush=True)
save()
