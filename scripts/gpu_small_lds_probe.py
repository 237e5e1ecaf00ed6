"""The resolving plant step at the bench shard (64 models x 512 scenarios = 32 768 instances) with the resolver on the small-problem path (MLD_SMALL_LDS,
k_small_milp) against the same step with the resolver on the dense path -- the parent's code path, measured in the same session.

    python scripts/gpu_small_lds_probe.py [--out profiles/small_lds_probe.json]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python scripts/gpu_small_lds_probe.py --kernel-only
    python scripts/gpu_small_lds_probe.py --summarise DIR [--merge FILE.json]

* default: two resolvers over the same models, one flagged and one not, ALTERNATING on the same stepped handle: one warm-up pair, seven timed pairs, median
  and range of the resolving step's wall time (ADVANCE | ACTUAL | LOG, u0 = None; a solve, not timed, before every step) and of the resolver's solve_ms
  (host route over the resolver's handle, the same triples for both); the counts of small_lds_stats; and that both routes leave every instance with the same
  delta, and sum(mu) and x_k1 within the test tolerances (worst deviations recorded).
* --kernel-only: for ONE kernel trace of its own -- three what-if steps (u0 given, nothing advances) per resolver.
* --summarise: k_small_milp next to the resolver's k_solve from the trace's csv files (no device needed).
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


def stat(ms):
    return dict(median_ms=round(float(np.median(ms)), 3), min_ms=round(min(ms), 3), max_ms=round(max(ms), 3), ms=[round(v, 3) for v in ms])


def summarise(d):
    seen = {}
    for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            name = r["Kernel_Name"].split("(")[0]
            if name.startswith("k_"):
                seen.setdefault(name, []).append(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
    return dict(kernels={k: dict(calls=len(v), average_ns=float(np.mean(v)), min_ns=float(min(v)), max_ns=float(max(v))) for k, v in sorted(seen.items())})


def main():
    if "--summarise" in sys.argv:
        rec, path = {}, None
        if "--merge" in sys.argv:
            path = sys.argv[sys.argv.index("--merge") + 1]
            rec = json.load(open(path)) if os.path.exists(path) else {}
        s = summarise(sys.argv[sys.argv.index("--summarise") + 1])
        print(json.dumps(s, indent=1))
        if path:
            rec["trace"] = s
            json.dump(rec, open(path, "w"), indent=1)
        return
    import bench
    from pyhybridcontrol_amd import gpu, host, _lib
    from pyhybridcontrol_amd.aux_resolve import BatchAuxResolver
    kernel_only = "--kernel-only" in sys.argv
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    agents, N_p, N_t, x0, om, midx = bench.make_shard(64, 512, 0)
    d = agents[0]["dims"]
    B, nx, nu, nw = x0.shape[0], d["nx"], d["nu"], d["nomega"]
    res = dict(version=_lib.version(), batch=B, models=len(agents), dims={k: int(v) for k, v in d.items()}, N_tilde=N_t)
    mats = [a["mats"] for a in agents]
    model = gpu.GpuModel(mats, d)
    cost = host.stack_costs([host.cost_from_atoms(a["atoms"], d, N_p, N_t) for a in agents])
    p = gpu.GpuProblem(model, N_p, N_t, cost, gap_rel=1e-2, max_nodes=800, max_pivots=40000)
    R = dict(small=BatchAuxResolver(mats, d, small_lds=True), dense=BatchAuxResolver(mats, d))
    steps = 48
    rng = np.random.default_rng(20)
    series = np.tile(om.reshape(B, N_t, nw), (1, steps // N_t + 1, 1))[:, :steps].copy()
    series[:, :, nx] += rng.normal(0.0, 800.0, (B, steps))
    lib, astart = np.ascontiguousarray(series).ravel(), (np.arange(B, dtype=np.int64) * steps * nw).reshape(B, 1)
    p.upload(x0, om, midx)
    p.upload_profiles(lib)
    u_fix = (rng.uniform(size=(B, nu)) < 0.4).astype(float)
    if kernel_only:
        for name in ("small", "dense"):
            for _ in range(3):
                p.sim_step(resolve=R[name], u0=u_fix, act_start=astart, step=0, advance=False, log=False)
        res["small_lds_stats"] = R["small"].problem.small_lds_stats()
        print(json.dumps(res))
        for r in R.values():
            r.close()
        p.close(); model.close()
        return
    k = [0]

    def step(name):
        if p.sim_log_count()[0] == p.sim_log_count()[1]:
            p.sim_log_begin(8)
        p.sim_step(resolve=R[name], act_start=astart if k[0] == 0 else None, step=k[0], actual=True, advance=True, log=True)
        k[0] += 1

    wall, solve_ms, counts = dict(small=[], dense=[]), dict(small=[], dense=[]), None
    for r in range(8):                                           # one warm-up pair, seven timed pairs, alternating
        for name in ("small", "dense"):
            p.solve_resident()
            t = time.perf_counter(); step(name); ms = (time.perf_counter() - t) * 1e3
            if name == "small":
                counts = R["small"].problem.small_lds_stats()
            if r >= 1:
                wall[name].append(ms)
    res["step_wall"] = {n: stat(v) for n, v in wall.items()}
    res["small_lds_stats_of_a_step"] = counts
    print("step wall:", res["step_wall"], counts, flush=True)
    # the resolver's own solve (K3 and the solver) on the same triples, host-fed, alternating
    x_in, w_in = p.inputs()
    w2 = np.ascontiguousarray(np.hstack([w_in[:, :nw], u_fix]))
    for r in range(8):
        for name in ("small", "dense"):
            q = R[name].problem
            q.upload(x_in, w2, midx)
            st = q.solve_resident()
            if r >= 1:
                solve_ms[name].append(st["solve_ms"])
    res["resolver_solve_ms"] = {n: stat(v) for n, v in solve_ms.items()}
    res["small_lds_stats"] = R["small"].problem.small_lds_stats()
    print("resolver solve_ms:", res["resolver_solve_ms"], res["small_lds_stats"], flush=True)
    # the same step by both resolvers from one solved state (what-ifs: nothing moves)
    p.solve_resident()
    a = p.sim_step(resolve=R["small"], step=k[0], actual=True, advance=False, log=False, outputs=True)
    b = p.sim_step(resolve=R["dense"], step=k[0], actual=True, advance=False, log=False, outputs=True)
    ok = (a["aux_status"] == 0) & (b["aux_status"] == 0)
    mu_a, mu_b = a["v0"][ok, nu + 2:].sum(axis=1), b["v0"][ok, nu + 2:].sum(axis=1)
    res["same_step"] = dict(instances=int(B), resolved_by_both=int(ok.sum()), statuses_equal=bool(np.array_equal(a["aux_status"], b["aux_status"])),
                            delta_equal=bool(np.array_equal(a["v0"][ok, nu], b["v0"][ok, nu])),
                            worst_sum_mu_dev=float((np.abs(mu_a - mu_b) / np.maximum(1.0, np.abs(mu_b))).max()),
                            worst_x_k1_dev=float((np.abs(a["x_k1"][ok] - b["x_k1"][ok]) / np.maximum(1.0, np.abs(b["x_k1"][ok]))).max()))
    print("same step:", res["same_step"], flush=True)
    for r in R.values():
        r.close()
    p.close(); model.close()
    print(json.dumps(res))
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
