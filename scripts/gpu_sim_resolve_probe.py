"""Plant step with re-derived auxiliaries at the bench shard (64 models x 512 scenarios = 32 768 instances): what a resolving step on the device costs
against the host route assembled from the entry points that were there before it, and where its time goes.

    python scripts/gpu_sim_resolve_probe.py [--out FILE.json]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python scripts/gpu_sim_resolve_probe.py --kernel-only
    python scripts/gpu_sim_resolve_probe.py --summarise DIR [--merge FILE.json]

* default: wall times on ONE pair of handles, the two routes alternating, one warm-up pair and then seven timed pairs, median (the host clock around calls
  that end in a stream synchronise); a solve, not timed, goes before every step.  Device route: sim_step(resolve=R) with ADVANCE | ACTUAL | LOG, u0 = None.
  Host route: download of x and of the plans, the realised omega cut out of the host's copy of the library, BatchAuxResolver.resolve fed from the host,
  sim_step(v0=...) with the same flags.  Also: that both give the same step, and the bytes each route moves over PCIe.
* --kernel-only: for ONE trace of its own -- three times: solve, sim_step(resolve=R) with ADVANCE | ACTUAL | LOG; then, three times each, a device-to-device
  hipMemcpyAsync of the destination bytes of k_aux_inputs and of k_aux_merge (the yardstick of the two copy kernels).
* --summarise: reads the trace's csv files (no device needed): k_aux_inputs, k_aux_merge, k_sim_step, the resolver's k_solve (the one that follows
  k_aux_inputs) as a share of the same step's main k_solve, and the copy kernels against their yardstick times 1.25 (short runs per instance: the margin the
  profiles probe gives its gather).
"""
import csv
import ctypes as C
import glob
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MARGIN = 1.25


def step_bytes(d, B):
    """destination bytes of the two copy kernels, and what each route moves over PCIe per step (the host route as its entry points move it, and the least
    it could move: x, the step-0 slice and omega down, the resolver's inputs and the slice up)"""
    nx, nu, nw = d["nx"], d["nu"], d["nomega"]
    nv = nu + d["ndelta"] + d["nz"] + d["nmu"]
    return dict(k_aux_inputs=8 * B * (nx + nw + nu), k_aux_merge=B * (8 * nv + 1 + 4),
                host_route_least=dict(down=8 * B * (nx + nv + nw), up=8 * B * (nx + nw + nu + nv)), device_route=0)


def timed_pair(fa, fb, between, warm=1, reps=7):
    """the two routes alternating on the same handles, `between` (not timed) before each: milliseconds of each"""
    a, b = [], []
    for r in range(warm + reps):
        between(); t = time.perf_counter(); fa(); ta = (time.perf_counter() - t) * 1e3
        between(); t = time.perf_counter(); fb(); tb = (time.perf_counter() - t) * 1e3
        if r >= warm:
            a.append(ta); b.append(tb)
    stat = lambda ms: dict(median_ms=round(float(np.median(ms)), 3), min_ms=round(min(ms), 3), ms=[round(v, 3) for v in ms])
    return stat(a), stat(b)


def summarise(d, nbytes=None):
    rows = []
    for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]) - int(r["Start_Timestamp"]), r["Kernel_Name"].split("(")[0]))
    rows.sort()
    seen = {}
    prev = None
    for _, ns, name in rows:
        key = name
        if name.startswith("k_solve"):
            key = "k_solve_aux" if prev == "k_aux_inputs" else "k_solve_main"
        elif "copyBuffer" in name:
            key = "copy_kernel"
        if name.startswith("k_") or key == "copy_kernel":
            seen.setdefault(key, []).append(ns)
        if name.startswith("k_"):
            prev = name
    stat = lambda v: dict(calls=len(v), average_ns=float(np.mean(v)), min_ns=float(min(v)), max_ns=float(max(v)))
    out = dict(kernels={k: stat(v) for k, v in seen.items() if k in ("k_aux_inputs", "k_aux_merge", "k_sim_step", "k_solve_aux", "k_solve_main")})
    k = out["kernels"]
    if "k_solve_aux" in k and "k_solve_main" in k:
        out["aux_solve_share_of_main_solve"] = k["k_solve_aux"]["average_ns"] / k["k_solve_main"]["average_ns"]
    copies = seen.get("copy_kernel", [])
    if len(copies) >= 6 and "k_aux_inputs" in k and "k_aux_merge" in k:      # the last six are the yardstick: three of each size
        ya, yb = float(np.mean(copies[-6:-3])), float(np.mean(copies[-3:]))
        out["yardstick"] = dict(margin=MARGIN, bytes=nbytes, copy_of_inputs_bytes_ns=ya, copy_of_merge_bytes_ns=yb,
                                k_aux_inputs_over_allowed=k["k_aux_inputs"]["average_ns"] / (ya * MARGIN),
                                k_aux_merge_over_allowed=k["k_aux_merge"]["average_ns"] / (yb * MARGIN))
    else:
        out["yardstick"] = "the device-to-device copies did not show as kernels in this trace (%d copy kernels seen)" % len(copies)
    return out


def d2d_copies(sizes, reps=3):
    """device-to-device hipMemcpyAsync of `sizes` bytes, `reps` times each, through the HIP runtime the library has loaded"""
    hip = C.CDLL("libamdhip64.so")
    for n in sizes:
        a, b = C.c_void_p(), C.c_void_p()
        assert hip.hipMalloc(C.byref(a), C.c_size_t(n)) == 0 and hip.hipMalloc(C.byref(b), C.c_size_t(n)) == 0
        assert hip.hipMemset(b, 0, C.c_size_t(n)) == 0
        for _ in range(reps):
            assert hip.hipMemcpyAsync(a, b, C.c_size_t(n), 3, None) == 0      # 3 = hipMemcpyDeviceToDevice
            assert hip.hipDeviceSynchronize() == 0
        hip.hipFree(a); hip.hipFree(b)


def main():
    if "--summarise" in sys.argv:
        rec, path = {}, None
        if "--merge" in sys.argv:
            path = sys.argv[sys.argv.index("--merge") + 1]
            rec = json.load(open(path)) if os.path.exists(path) else {}
        s = summarise(sys.argv[sys.argv.index("--summarise") + 1], rec.get("bytes_per_step"))
        print(json.dumps(s, indent=1))
        if path:
            rec["trace"] = s
            json.dump(rec, open(path, "w"), indent=1)
        return
    import bench
    from pyhybridcontrol_amd import gpu, host, profiles, _lib
    from pyhybridcontrol_amd.aux_resolve import BatchAuxResolver
    kernel_only = "--kernel-only" in sys.argv
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    agents, N_p, N_t, x0, om, midx = bench.make_shard(64, 512, 0)
    d = agents[0]["dims"]
    B, nx, nu, nw = x0.shape[0], d["nx"], d["nu"], d["nomega"]
    nv = nu + d["ndelta"] + d["nz"] + d["nmu"]
    nb = step_bytes(d, B)
    res = dict(version=_lib.version(), batch=B, models=len(agents), dims={k: int(v) for k, v in d.items()}, N_tilde=N_t, bytes_per_step=nb)
    mats = [a["mats"] for a in agents]
    model = gpu.GpuModel(mats, d)
    cost = host.stack_costs([host.cost_from_atoms(a["atoms"], d, N_p, N_t) for a in agents])
    p = gpu.GpuProblem(model, N_p, N_t, cost, gap_rel=1e-2, max_nodes=800, max_pivots=40000)
    R = BatchAuxResolver(mats, d)
    # the realised series: the forecast's rows with the load channel moved by N(0, 800), one series of `steps` rows per instance (one group of width nomega)
    steps = 40
    rng = np.random.default_rng(20)
    series = np.tile(om.reshape(B, N_t, nw), (1, steps // N_t + 1, 1))[:, :steps].copy()
    series[:, :, nx] += rng.normal(0.0, 800.0, (B, steps))
    lib, astart = np.ascontiguousarray(series).ravel(), (np.arange(B, dtype=np.int64) * steps * nw).reshape(B, 1)
    p.upload(x0, om, midx)
    p.upload_profiles(lib)
    k = [0]

    def solve():
        p.solve_resident()

    def on_device():
        if p.sim_log_count()[0] == p.sim_log_count()[1]:
            p.sim_log_begin(8)
        out = p.sim_step(resolve=R, act_start=astart if k[0] == 0 else None, step=k[0], actual=True, advance=True, log=True)
        k[0] += 1
        return out

    if kernel_only:
        p.sim_log_begin(3)
        for _ in range(3):
            solve()
            on_device()
        d2d_copies([nb["k_aux_inputs"], nb["k_aux_merge"]])
        print(json.dumps(res))
        R.close(); p.close(); model.close()
        return
    moved = dict(down=0, up=0)

    def on_host():
        if p.sim_log_count()[0] == p.sim_log_count()[1]:
            p.sim_log_begin(8)
        x = np.zeros((B, nx))
        _lib.check(_lib.load().mld_download_inputs(p._h, _lib.dptr(x), None))
        plan = p.download()                                     # (the parent has no download of the step-0 slices alone: the whole plans come down)
        w = profiles.windows(lib, astart, k[0], 1, (nw,))       # the host holds the library it uploaded
        usable = np.isin(plan["status"], (0, 2)) & np.isfinite(plan["obj"])
        u = np.where(usable[:, None], plan["v"][:, :nu], 0.0)
        h = R.resolve(x, u, w, midx)
        v0 = np.hstack([u, h["v"]])
        v0[~usable] = np.nan
        out = p.sim_step(v0=np.nan_to_num(v0), step=k[0], actual=True, advance=True, log=True)
        k[0] += 1
        moved.update(down=8 * (x.size + plan["v"].size + 2 * B) + 4 * 3 * B + 8 * h["v"].size + 12 * B, up=8 * (x.size + w.size + u.size + v0.size) + 4 * B)
        return out

    solve(); on_device()                                        # the starts become resident; the resolver's batch is laid out
    dev, hst = timed_pair(on_device, on_host, solve)
    res["wall"] = dict(device_route=dev, host_route=hst, host_route_bytes_moved=dict(moved))
    print("wall:", res["wall"], flush=True)
    # the same step by both routes, from one solved state (what-ifs: nothing moves)
    solve()
    got = p.sim_step(resolve=R, step=k[0], actual=True, advance=False, log=False, outputs=True)
    x_in = p.inputs()[0]
    plan = p.download()
    usable = got["aux_status"] >= 0
    h = R.resolve(x_in, np.where(usable[:, None], plan["v"][:, :nu], 0.0), profiles.windows(lib, astart, k[0], 1, (nw,)), midx)
    ref = p.sim_step(v0=np.nan_to_num(np.hstack([plan["v"][:, :nu], h["v"]])), step=k[0], actual=True, advance=False, log=False, outputs=True)
    ok = got["aux_status"] == 0
    res["same_step"] = dict(resolved=int(ok.sum()), not_attempted=int((~usable).sum()), x_k1_equal=bool(np.array_equal(got["x_k1"][ok], ref["x_k1"][ok])),
                            v0_equal=bool(np.array_equal(got["v0"][ok, nu:], h["v"][ok])), cons_all_true=float(got["cons"][ok].all(axis=1).mean()))
    print("same step:", res["same_step"], flush=True)
    R.close(); p.close(); model.close()
    print(json.dumps(res))
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
