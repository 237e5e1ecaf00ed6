"""Per-instance linear cost at the bench shard (64 models x 512 scenarios, the bench's options): what it costs.

    python scripts/gpu_inst_cost_probe.py [--model-only] [--pullback-only] [--out FILE.json]

* solve: the bench's cost as the MODEL cost against zero model q_z plus the same q_z per instance (mld_upload_instance_cost, lin_v only): same
  instances, same numbers -- nodes and pivots per instance must be identical; median solve_ms of five launches each.  --model-only runs the first
  half alone (it needs nothing this entry point adds, so the same file measures an older library).
* upload: wall time of upload_instance_cost with lin_v only (batch x n doubles host to device).
* pull-back: wall time of upload_instance_cost with random lin_x / lin_y beside lin_v only (the difference is the copies of the weights plus
  k_inst_pullback), and rhs_ms (K3) of the same run.  --pullback-only does just the uploads and one solve (for K3), for a run under
  `rocprofv3 --kernel-trace --stats -- python scripts/gpu_inst_cost_probe.py --pullback-only`.
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench                                                            # noqa: E402
from pyhybridcontrol_amd import gpu, host, _lib                         # noqa: E402


def median_solve(p, reps=5):
    ms, last = [], None
    for _ in range(reps):
        st = p.solve_resident()
        ms.append(st["solve_ms"]); last = st
    out = p.download()
    return float(np.median(ms)), [round(float(v), 3) for v in ms], last, out


def main():
    model_only, pb_only = "--model-only" in sys.argv, "--pullback-only" in sys.argv
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    agents, N_p, N_t, x0, om, midx = bench.make_shard(64, 512, 0)
    d = agents[0]["dims"]
    B, n = x0.shape[0], N_t * (d["nu"] + d["ndelta"] + d["nz"] + d["nmu"])
    res = dict(version=_lib.version(), batch=B, n=n)
    model = gpu.GpuModel([a["mats"] for a in agents], d)
    opts = dict(gap_rel=1e-2, max_nodes=800, max_pivots=40000)
    full = host.stack_costs([host.cost_from_atoms(a["atoms"], d, N_p, N_t) for a in agents])
    if not pb_only:
        p = gpu.GpuProblem(model, N_p, N_t, full, **opts)
        p.upload(x0, om, midx)
        p.solve_resident()                                              # warm-up (also learns the work-queue order)
        med, all_ms, st, ref = median_solve(p)
        res["model_cost"] = dict(solve_ms_median=round(med, 3), solve_ms=all_ms, rhs_ms=round(st["rhs_ms"], 3), nodes=int(st["nodes"]), pivots=int(st["pivots"]),
                                 n_optimal=int(st["n_optimal"]))
        p.close()
        print("model cost:", res["model_cost"], flush=True)
    if not model_only:
        common = host.stack_costs([host.cost_from_atoms({"q_mu": a["atoms"]["q_mu"]}, d, N_p, N_t) for a in agents])
        per_model_qz = np.stack([host.cost_from_atoms({"q_z": a["atoms"]["q_z"]}, d, N_p, N_t)["lin_v"] for a in agents])
        lin_v = np.ascontiguousarray(per_model_qz[midx])
        q = gpu.GpuProblem(model, N_p, N_t, common, **opts)
        q.upload(x0, om, midx)
        ups = []
        for _ in range(3):
            t = time.perf_counter(); q.upload_instance_cost(lin_v=lin_v); ups.append((time.perf_counter() - t) * 1e3)
        res["upload_lin_v"] = dict(bytes=int(lin_v.nbytes), ms=[round(v, 2) for v in ups], gb_per_s=round(lin_v.nbytes / (min(ups) * 1e-3) / 1e9, 2))
        print("upload lin_v:", res["upload_lin_v"], flush=True)
        if pb_only:
            st = q.solve_resident()                                     # one launch under the bench's own cost, so that K3 (k_rhs_mfma) is in the same kernel trace
            res["rhs_ms_same_run"] = round(st["rhs_ms"], 3)
        else:
            q.solve_resident()
            med, all_ms, st, got = median_solve(q)
            same = bool(np.array_equal(got["nodes"], ref["nodes"]) and np.array_equal(got["pivots"], ref["pivots"]) and np.array_equal(got["obj"], ref["obj"]))
            res["instance_cost"] = dict(solve_ms_median=round(med, 3), solve_ms=all_ms, rhs_ms=round(st["rhs_ms"], 3), nodes=int(st["nodes"]), pivots=int(st["pivots"]),
                                        n_optimal=int(st["n_optimal"]), identical_nodes_pivots_objectives=same)
            print("per-instance cost:", res["instance_cost"], flush=True)
        rng = np.random.default_rng(0)
        NX, NY = N_t * d["nx"], N_t * d["ny"]
        lin_x, lin_y = rng.standard_normal((B, NX)), rng.standard_normal((B, NY))
        pbs = []
        for _ in range(3):
            t = time.perf_counter(); q.upload_instance_cost(lin_v=lin_v, lin_x=lin_x, lin_y=lin_y); pbs.append((time.perf_counter() - t) * 1e3)
        ncol = n + d["nx"] + N_t * d["nomega"] + 1
        res["pullback"] = dict(K=NX + NY, ncol=ncol, gflop=round(2.0 * B * (NX + NY) * ncol / 1e9, 2), algorithmic_bytes=int(8 * B * (NX + NY + 2 * ncol)),
                               upload_with_pullback_ms=[round(v, 2) for v in pbs])
        print("pull-back:", res["pullback"], flush=True)
        q.close()
    model.close()
    print(json.dumps(res))
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
