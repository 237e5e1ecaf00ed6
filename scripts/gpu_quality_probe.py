"""Solution quality at the bench shard (64 models x 512 scenarios = 32 768 instances, the bench's options): what mld_evaluate_batch costs.

    python scripts/gpu_quality_probe.py [--kernel-only] [--out FILE.json]

* device route: wall time of GpuProblem.evaluate() on the solved shard -- the resident plans as posed; the same with 20 validation columns
  (1.05 GB of omega_cols uploaded in slices of 256 MB); and with the caller's v (151 MB uploaded first).  Two warm-up calls, then ten timed ones (three
  with the columns): median and minimum.
* host route of today (tests/test_gpu_solve.py::check_solution): download() of every plan, then numpy per model on the downloaded H maps
  (the maps' own download timed apart: it is paid once).
* --kernel-only: upload, one solve, one mld_predict_batch and five as-posed calls, nothing else -- for ONE run under
  `rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python scripts/gpu_quality_probe.py --kernel-only`: k_evaluate next to K3
  (k_rhs_mfma) and k_trajectory in the same trace.
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
    B, n, m0, nW = x0.shape[0], N_t * nv, N_t * d["nc"], N_t * d["nomega"]
    C = 20
    res = dict(version=_lib.version(), batch=B, models=len(agents), n=n, rows=m0, inner_columns=d["nx"] + nW, n_validation_columns=C,
               gflop_dense=dict(H_v=round(2.0 * B * m0 * n / 1e9, 2), per_column=round(2.0 * B * m0 * (d["nx"] + nW) / 1e9, 2)),
               bytes=dict(v=8 * B * n, inputs=8 * B * (d["nx"] + nW), hv_scratch=8 * B * m0, validation_columns=8 * B * C * nW,
                          maps=8 * len(agents) * m0 * (n + d["nx"] + nW + 1)))
    model = gpu.GpuModel([a["mats"] for a in agents], d)
    cost = host.stack_costs([host.cost_from_atoms(a["atoms"], d, N_p, N_t) for a in agents])
    p = gpu.GpuProblem(model, N_p, N_t, cost, gap_rel=1e-2, max_nodes=800, max_pivots=40000)
    p.upload(x0, om, midx)
    st = p.solve_resident()
    res["solve"] = dict(solve_ms=round(st["solve_ms"], 3), rhs_ms=round(st["rhs_ms"], 3), n_optimal=int(st["n_optimal"]))
    print("solve:", res["solve"], flush=True)
    if kernel_only:
        p.trajectories()
        for _ in range(5):
            p.evaluate()
        print(json.dumps(res))
        p.close(); model.close()
        return
    res["device_route"] = dict(evaluate_resident_plans=timed(lambda: p.evaluate()))
    q = p.evaluate()
    v = p.download()["v"]
    res["device_route"]["evaluate_callers_v"] = timed(lambda: p.evaluate(v))
    rng = np.random.default_rng(1)
    cols = om[:, None, :] * rng.uniform(0.8, 1.25, size=(B, C, 1))       # C scaled copies of every instance's own forecast
    res["device_route"]["evaluate_20_validation_columns"] = timed(lambda: p.evaluate(omega_cols=cols), warm=1, reps=3)
    qc = p.evaluate(omega_cols=cols)
    print("device route:", res["device_route"], flush=True)

    # the host route of today
    t = time.perf_counter()
    evo = model.condense(N_t, names=("H_x", "H_v", "H_omega", "H_5"))
    maps_ms = (time.perf_counter() - t) * 1e3
    hv, hr = np.zeros(B), np.zeros(B, np.int64)

    def host_route():
        vh = p.download()["v"]
        for k in range(len(agents)):
            s = midx == k
            r = vh[s] @ evo["H_v"][k].T - (x0[s] @ evo["H_x"][k].T + om[s] @ evo["H_omega"][k].T + evo["H_5"][k][:, 0])
            hv[s], hr[s] = r.max(axis=1), r.argmax(axis=1)

    res["host_route"] = dict(download_and_numpy_per_model=timed(host_route, warm=1, reps=3), maps_download_once_ms=round(maps_ms, 2),
                             numpy_threads=os.environ.get("OMP_NUM_THREADS"))
    ok = np.isfinite(q["constr_vio"])
    rown = np.stack([np.maximum(1.0, np.abs(evo["H_v"][k]).max(axis=1)) for k in range(len(agents))])      # check_solution's row norm
    rel = q["constr_vio"][ok] / rown[midx[ok], q["constr_row"][ok]]
    res["agreement"] = dict(instances_with_a_plan=int(ok.sum()), max_abs_err_constr_vio=float(np.abs(q["constr_vio"][ok] - hv[ok]).max()),
                            worst_constr_vio=float(q["constr_vio"][ok].max()), worst_constr_vio_over_row_norm=float(rel.max()),
                            instances_over_1e6_of_row_norm=int((rel > 1e-6).sum()), worst_int_vio=float(q["int_vio"][ok].max()),
                            worst_bound_vio=float(q["bound_vio"][ok].max()),
                            worst_obj_gap=float(np.abs(q["obj"][ok] - p.download()["obj"][ok]).max()),
                            validation_columns_violated_gt_1e6=int((qc["constr_vio"][ok] > 1e-6).sum()), validation_columns=int(ok.sum()) * C)
    print("host route:", res["host_route"], res["agreement"], flush=True)
    p.close(); model.close()
    print(json.dumps(res))
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
