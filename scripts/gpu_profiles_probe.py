"""Resident disturbance profiles at the bench shard (64 models x 512 scenarios = 32 768 instances, 20 columns, the model's group widths: seven
heaters and the grid tie, one disturbance channel each): what gathering windows on the device costs against uploading them.

    python scripts/gpu_profiles_probe.py [--out FILE.json]
    rocprofv3 --kernel-trace --memory-copy-trace --stats --output-format csv -d DIR -- python scripts/gpu_profiles_probe.py --kernel-only
    python scripts/gpu_profiles_probe.py --summarise DIR [--merge FILE.json]

* default: wall times on ONE handle, the two routes alternating, one warm-up pair and then seven timed pairs, median (the host clock around calls
  that end in a stream synchronise): upload_constraint_blocks(windows) against constraint_blocks_from_profiles(starts); evaluate(omega_cols=windows)
  against evaluate_profiles(starts); the bytes each route moves over PCIe; and that both routes give the same blocks and the same audit.
* --kernel-only: for ONE trace of its own -- five forecasts from the library (k_profile_windows, batch x N_tilde*nomega doubles) beside five
  mld_select_inputs (the device-to-device copy of the SAME number of destination bytes), then five block gathers of 20 columns (1.05 GB each).
* --summarise: reads the trace's csv files (no device needed) and prints / merges the kernel and copy durations and the store bandwidths.
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

C_COLS = 20
EXTRA = C_COLS          # steps a series has beyond the horizon: column c of an instance starts c steps into its series


def make_library(om, N, nomega):
    """per instance and channel one series of N + EXTRA steps (its forecast, continued periodically), all of width 1; the flat library and the base
    offset of every series, (batch, nomega)"""
    from pyhybridcontrol_amd import profiles
    B = om.shape[0]
    w = om.reshape(B, N, nomega)
    series = np.concatenate([w, w[:, :EXTRA]], axis=1).transpose(0, 2, 1)          # (B, nomega, N + EXTRA)
    lib, base = profiles.pack([series])
    return lib, (base[0] + np.arange(B * nomega, dtype=np.int64) * (N + EXTRA)).reshape(B, nomega)


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


def summarise(d):
    """kernel and copy durations of one rocprofv3 --kernel-trace --memory-copy-trace --stats run"""
    out = dict(kernels={}, copies={})
    for f in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            if any(k in r["Name"] for k in ("k_profile_windows", "copyBuffer", "k_evaluate", "k_rhs_mfma")):
                out["kernels"][r["Name"].split("(")[0]] = dict(calls=int(r["Calls"]), average_ns=float(r["AverageNs"]), min_ns=float(r["MinNs"]), max_ns=float(r["MaxNs"]))
    for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        rows = [r for r in csv.DictReader(open(f)) if "k_profile_windows" in r["Kernel_Name"]]
        out["k_profile_windows_ns"] = [int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in rows]
    for f in glob.glob(os.path.join(d, "**", "*memory_copy_trace.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            key = r.get("Direction") or r.get("Name") or "copy"
            out["copies"].setdefault(key, []).append(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
    return out


def main():
    if "--summarise" in sys.argv:
        s = summarise(sys.argv[sys.argv.index("--summarise") + 1])
        print(json.dumps(s, indent=1))
        if "--merge" in sys.argv:
            path = sys.argv[sys.argv.index("--merge") + 1]
            rec = json.load(open(path)) if os.path.exists(path) else {}
            rec["trace"] = s
            json.dump(rec, open(path, "w"), indent=1)
        return
    import bench
    from pyhybridcontrol_amd import gpu, host, profiles, _lib
    kernel_only = "--kernel-only" in sys.argv
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    agents, N_p, N_t, x0, om, midx = bench.make_shard(64, 512, 0)
    d = agents[0]["dims"]
    B, nomega, nW = x0.shape[0], d["nomega"], N_t * d["nomega"]
    gw = (1,) * nomega
    lib, base = make_library(om, N_t, nomega)
    fstart = base
    cstart = base[:, None, :] + np.arange(C_COLS, dtype=np.int64)[None, :, None]          # (B, C, G): column c starts c steps on (width 1)
    res = dict(version=_lib.version(), batch=B, models=len(agents), n_cols=C_COLS, nW=nW, group_width=list(gw), library_doubles=int(lib.size),
               bytes_over_pcie=dict(forecast_uploaded=8 * B * nW, forecast_starts=8 * B * len(gw), columns_uploaded=8 * B * C_COLS * nW,
                                    column_starts=8 * B * C_COLS * len(gw), library_once=8 * int(lib.size)),
               destination_bytes=dict(forecast=8 * B * nW, blocks=8 * B * C_COLS * nW))
    model = gpu.GpuModel([a["mats"] for a in agents], d)
    cost = host.stack_costs([host.cost_from_atoms(a["atoms"], d, N_p, N_t) for a in agents])
    p = gpu.GpuProblem(model, N_p, N_t, cost, gap_rel=1e-2, max_nodes=800, max_pivots=40000)
    p.upload(x0, om, midx)
    p.upload_profiles(lib, gw)
    if kernel_only:
        p.stage(x0[None], om[None])
        for _ in range(5):
            p.forecast_from_profiles(fstart, 0)
            p.select(0)
        for _ in range(5):
            p.constraint_blocks_from_profiles(cstart, 0)
        print(json.dumps(res))
        p.close(); model.close()
        return
    st = p.solve_resident()
    res["solve"] = dict(solve_ms=round(st["solve_ms"], 3), n_optimal=int(st["n_optimal"]))
    print("solve:", res["solve"], flush=True)
    cols = profiles.windows(lib, cstart, 0, N_t, gw)
    up, ga = timed_pair(lambda: p.upload_constraint_blocks(cols), lambda: p.constraint_blocks_from_profiles(cstart, 0))
    res["blocks"] = dict(upload_constraint_blocks=up, constraint_blocks_from_profiles=ga,
                         resident_starts_next_step=timed_pair(lambda: p.constraint_blocks_from_profiles(None, 1), lambda: None)[0])
    p.constraint_blocks_from_profiles(cstart, 0)
    same_blocks = bool(np.array_equal(p.constraint_blocks()["omega_cols"], cols))
    print("blocks:", res["blocks"], same_blocks, flush=True)
    eu, eg = timed_pair(lambda: p.evaluate(omega_cols=cols), lambda: p.evaluate_profiles(cstart, 0))
    res["evaluate"] = dict(evaluate_uploaded_columns=eu, evaluate_profiles=eg, evaluate_no_columns=timed_pair(lambda: p.evaluate(), lambda: None)[0])
    qa, qb = p.evaluate(omega_cols=cols), p.evaluate_profiles(cstart, 0)
    res["same_results"] = dict(blocks=same_blocks, audit=bool(all(np.array_equal(qa[k], qb[k], equal_nan=True) for k in qa)))
    print("evaluate:", res["evaluate"], res["same_results"], flush=True)
    p.close(); model.close()
    print(json.dumps(res))
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
