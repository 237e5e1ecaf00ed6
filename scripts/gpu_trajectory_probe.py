"""Predicted trajectories at the bench shard (64 models x 512 scenarios = 32 768 instances, the bench's options): what mld_predict_batch costs.

    python scripts/gpu_trajectory_probe.py [--kernel-only] [--out FILE.json]

* device route: wall time of mld_predict_batch on the solved shard -- the resident plans (v = NULL), x_out and y_out downloaded (52 MB) into arrays
  that exist already; the same through GpuProblem.trajectories() (which allocates its result); and with the caller's v (151 MB uploaded first).
  Two warm-up calls, then ten timed ones: median and minimum.
* K3 of the same shard: rhs_ms of the solve's mld_stats; the k_inst_pullback time recorded in profiles/inst_cost_probe.json.
* host route of today: download v, then numpy per model on the downloaded condensed maps (the maps' own download timed apart: it is paid once).
* --kernel-only: upload, one solve and five calls, nothing else -- for ONE run under
  `rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python scripts/gpu_trajectory_probe.py --kernel-only` (the kernel's own time).
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


def timed(fn, warm=2, reps=10):
    for _ in range(warm):
        fn()
    ms = []
    for _ in range(reps):
        t = time.perf_counter(); fn(); ms.append((time.perf_counter() - t) * 1e3)
    return dict(median_ms=round(float(np.median(ms)), 3), min_ms=round(min(ms), 3), ms=[round(v, 3) for v in ms])


def main():
    kernel_only = "--kernel-only" in sys.argv
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    agents, N_p, N_t, x0, om, midx = bench.make_shard(64, 512, 0)
    d = agents[0]["dims"]
    nv = d["nu"] + d["ndelta"] + d["nz"] + d["nmu"]
    B, n, NX, NY, nW = x0.shape[0], N_t * nv, N_t * d["nx"], N_t * d["ny"], N_t * d["nomega"]
    K = n + d["nx"] + nW + 1
    res = dict(version=_lib.version(), batch=B, models=len(agents), n=n, inner=K, rows=NX + NY, gflop_dense=round(2.0 * B * (NX + NY) * K / 1e9, 2),
               bytes=dict(v=8 * B * n, inputs=8 * B * (d["nx"] + nW), output=8 * B * (NX + NY), maps=8 * len(agents) * (NX + NY) * K))
    model = gpu.GpuModel([a["mats"] for a in agents], d)
    cost = host.stack_costs([host.cost_from_atoms(a["atoms"], d, N_p, N_t) for a in agents])
    p = gpu.GpuProblem(model, N_p, N_t, cost, gap_rel=1e-2, max_nodes=800, max_pivots=40000)
    p.upload(x0, om, midx)
    st = p.solve_resident()
    res["solve"] = dict(solve_ms=round(st["solve_ms"], 3), rhs_ms=round(st["rhs_ms"], 3), n_optimal=int(st["n_optimal"]))
    print("solve:", res["solve"], flush=True)
    lib = _lib.load()
    xo, yo = np.zeros((B, NX)), np.zeros((B, NY))                        # (touched: no page faults inside the timed copies)

    def c_entry(v=None):
        gpu.check(lib.mld_predict_batch(p._h, _lib.dptr(v), _lib.dptr(xo), _lib.dptr(yo)))

    if kernel_only:
        for _ in range(5):
            c_entry()
        print(json.dumps(res))
        p.close(); model.close()
        return
    res["device_route"] = dict(c_entry_resident_plans=timed(c_entry), python_trajectories=timed(lambda: p.trajectories()))
    v = p.download()["v"]
    res["device_route"]["c_entry_callers_v"] = timed(lambda: c_entry(v))
    print("device route:", res["device_route"], flush=True)
    got_x, got_y = xo.copy(), yo.copy()

    # the host route of today
    t = time.perf_counter()
    evo = model.condense(N_t, names=("Phi_x", "Gamma_v", "Gamma_omega", "Gamma_5", "L_x", "L_v", "L_omega", "L_5"))
    maps_ms = (time.perf_counter() - t) * 1e3
    vh = np.zeros((B, n))
    hx, hy = np.zeros((B, NX)), np.zeros((B, NY))

    def host_route():
        gpu.check(lib.mld_download_results(p._h, _lib.dptr(vh), None, None, None, None, None))
        for k in range(len(agents)):
            s = midx == k
            hx[s] = vh[s] @ evo["Gamma_v"][k].T + x0[s] @ evo["Phi_x"][k].T + om[s] @ evo["Gamma_omega"][k].T + evo["Gamma_5"][k][:, 0]
            hy[s] = vh[s] @ evo["L_v"][k].T + x0[s] @ evo["L_x"][k].T + om[s] @ evo["L_omega"][k].T + evo["L_5"][k][:, 0]

    res["host_route"] = dict(download_v_and_numpy_per_model=timed(host_route, warm=1, reps=3), maps_download_once_ms=round(maps_ms, 2),
                             numpy_threads=os.environ.get("OMP_NUM_THREADS"))
    ok = np.isfinite(got_x).all(axis=1)
    res["agreement"] = dict(rows_with_a_plan=int(ok.sum()), max_abs_x=float(np.abs(hx[ok]).max()), max_err_x=float(np.abs(got_x[ok] - hx[ok]).max()),
                            max_abs_y=float(np.abs(hy[ok]).max()), max_err_y=float(np.abs(got_y[ok] - hy[ok]).max()))
    print("host route:", res["host_route"], res["agreement"], flush=True)
    try:
        with open(os.path.join(ROOT, "profiles", "inst_cost_probe.json")) as f:
            pb = [k for k in json.load(f)["kernel_trace"] if "k_inst_pullback" in k["name"]]
        res["k_inst_pullback_recorded_us"] = pb[0]["avg_us"] if pb else None
    except OSError:
        res["k_inst_pullback_recorded_us"] = None
    p.close(); model.close()
    print(json.dumps(res))
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
