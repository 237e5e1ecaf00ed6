"""Plant step and simulation log at the bench shard (64 models x 512 scenarios = 32 768 instances): what stepping and logging on the device costs
against downloading the plans and redoing lsim_k on the host, and k_sim_step against the parent's k_advance.

    python scripts/gpu_sim_step_probe.py [--out FILE.json]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python scripts/gpu_sim_step_probe.py --kernel-only
    python scripts/gpu_sim_step_probe.py --summarise DIR [--merge FILE.json]

* default: wall times on ONE solved handle, the two routes alternating, one warm-up pair and then seven timed pairs, median (the host clock around calls
  that end in a stream synchronise): sim_step(advance=False, log=True) -- the record stays in HBM -- against download() plus simlog.lsim_k_batch on the
  host; that both give the same step; and the bytes of each route.
* --kernel-only: for ONE trace of its own -- three times: solve, sim_step(advance=True, log=True) (k_sim_step with ADVANCE | LOG), solve, advance()
  (k_advance), on the same handle.
* --summarise: reads the trace's csv files (no device needed): the two kernels' durations, and k_sim_step against the yardstick -- k_advance's time times the
  ratio of the two kernels' algorithmic bytes, plus 25 % for the nv-double slices read out of n-double rows.
"""
import csv
import glob
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MARGIN = 1.25


def kernel_bytes(d, N):
    """algorithmic bytes per instance: k_advance, k_sim_step with ADVANCE | LOG, and the record alone"""
    nx, nv, nw, ny, nc = d["nx"], d["nu"] + d["ndelta"] + d["nz"] + d["nmu"], d["nomega"], d["ny"], d["nc"]
    nW = N * nw
    advance = 8 * (nx + nv + nW) + 12 + 8 * (nx + nW)            # reads x, the step-0 slice, the forecast, status + objective; writes x and the forecast
    record = 8 * (2 * nx + nv + ny + nw + 3) + nc + 12
    return dict(k_advance=advance, k_sim_step_advance_log=advance + record + 12, record=record)      # (+ 12: lower bound and nodes are read too)


def timed_pair(fa, fb, warm=1, reps=7):
    """the two routes alternating on the same handle: milliseconds of each"""
    a, b = [], []
    for r in range(warm + reps):
        t = time.perf_counter(); fa(); ta = (time.perf_counter() - t) * 1e3
        t = time.perf_counter(); fb(); tb = (time.perf_counter() - t) * 1e3
        if r >= warm:
            a.append(ta); b.append(tb)
    stat = lambda ms: dict(median_ms=round(float(np.median(ms)), 3), min_ms=round(min(ms), 3), ms=[round(v, 3) for v in ms])
    return stat(a), stat(b)


def summarise(d, ratio=None):
    out = dict(kernels={})
    for f in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            name = r["Name"].split("(")[0]
            if name in ("k_sim_step", "k_advance"):
                out["kernels"][name] = dict(calls=int(r["Calls"]), average_ns=float(r["AverageNs"]), min_ns=float(r["MinNs"]), max_ns=float(r["MaxNs"]))
    k = out["kernels"]
    if ratio and "k_sim_step" in k and "k_advance" in k:
        yard = k["k_advance"]["average_ns"] * ratio * MARGIN
        out["yardstick"] = dict(bytes_ratio=ratio, margin=MARGIN, allowed_ns=yard, k_sim_step_over_allowed=k["k_sim_step"]["average_ns"] / yard)
    return out


def main():
    if "--summarise" in sys.argv:
        rec, path = {}, None
        if "--merge" in sys.argv:
            path = sys.argv[sys.argv.index("--merge") + 1]
            rec = json.load(open(path)) if os.path.exists(path) else {}
        kb = rec.get("kernel_bytes_per_instance")
        s = summarise(sys.argv[sys.argv.index("--summarise") + 1], kb["k_sim_step_advance_log"] / kb["k_advance"] if kb else None)
        print(json.dumps(s, indent=1))
        if path:
            rec["trace"] = s
            json.dump(rec, open(path, "w"), indent=1)
        return
    import bench
    from pyhybridcontrol_amd import gpu, host, simlog, _lib
    kernel_only = "--kernel-only" in sys.argv
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    agents, N_p, N_t, x0, om, midx = bench.make_shard(64, 512, 0)
    d = agents[0]["dims"]
    B, nw, nv = x0.shape[0], d["nomega"], d["nu"] + d["ndelta"] + d["nz"] + d["nmu"]
    kb = kernel_bytes(d, N_t)
    res = dict(version=_lib.version(), batch=B, models=len(agents), dims={k: int(v) for k, v in d.items()}, N_tilde=N_t, kernel_bytes_per_instance=kb,
               bytes_per_step=dict(record_in_hbm=kb["record"] * B, v_downloaded=8 * B * N_t * nv, actual_starts_per_group=8 * B, actual_values=8 * B * nw))
    model = gpu.GpuModel([a["mats"] for a in agents], d)
    cost = host.stack_costs([host.cost_from_atoms(a["atoms"], d, N_p, N_t) for a in agents])
    p = gpu.GpuProblem(model, N_p, N_t, cost, gap_rel=1e-2, max_nodes=800, max_pivots=40000)
    p.upload(x0, om, midx)
    if kernel_only:
        p.sim_log_begin(3)
        for _ in range(3):
            p.solve_resident()
            p.sim_step(advance=True, log=True)
            p.solve_resident()
            p.advance()
        print(json.dumps(res))
        p.close(); model.close()
        return
    st = p.solve_resident()
    res["solve"] = dict(solve_ms=round(st["solve_ms"], 3), n_optimal=int(st["n_optimal"]))
    print("solve:", res["solve"], flush=True)
    mats = [a["mats"] for a in agents]
    host_step = {}

    def on_host():
        out = p.download()
        host_step.update(simlog.lsim_k_batch(mats, d, midx, x0, out["v"][:, :nv], om[:, :nw]), status=out["status"], obj=out["obj"])

    def on_device():
        if p.sim_log_count()[0] == p.sim_log_count()[1]:
            p.sim_log_begin(8)
        p.sim_step(advance=False, log=True)

    p.sim_log_begin(8)
    dev, hst = timed_pair(on_device, on_host)
    res["wall"] = dict(sim_step_log=dev, download_plus_numpy=hst)
    rec = p.sim_log(0, 1)
    usable = np.isin(host_step["status"], (0, 2)) & np.isfinite(host_step["obj"])
    scale = max(1.0, float(np.abs(host_step["x_k1"][usable]).max()))
    res["same_step"] = dict(usable=int(usable.sum()), x_k1_max_rel_err=float(np.abs(rec["x_k1"][0][usable] - host_step["x_k1"][usable]).max() / scale),
                            cons_equal=float((rec["cons"][0][usable] == host_step["cons"][usable]).mean()))
    print("wall:", res["wall"], res["same_step"], flush=True)
    p.close(); model.close()
    print(json.dumps(res))
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
