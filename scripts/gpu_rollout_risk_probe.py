"""Rollout risk on the device (GpuProblem.rollout(risk=...), mld_rollout_risk; kernel k_rollout_risk) at the bench shard (64 models x 512 scenarios =
32 768 instances), K = 25 steps under S = 20 realisations, the thermostat in closed loop and the microgrid KPIs of scripts/gpu_rollout_kpi_probe.py.

    python scripts/gpu_rollout_risk_probe.py [--out profiles/rollout_risk_probe.json] [--pairs 7]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python scripts/gpu_rollout_risk_probe.py --kernel-only
    python scripts/gpu_rollout_risk_probe.py --summarise DIR [--merge FILE.json]
    python scripts/gpu_rollout_risk_probe.py --bench PARENT_TREE [--merge FILE.json] [--pairs 3]

* default: wall time of rollout(policy=True, kpis=..., risk=..., per_trajectory=False) against the route the parent commit has for the same figures,
  rollout(policy=True, kpis=...) plus simlog.rollout_risk_np on the host, ALTERNATING in one session: one warm-up round, then --pairs timed rounds, the figure
  is the median.  Whether the two give the same bits, and the bytes each downloads.
* --kernel-only: for ONE kernel trace of its own -- three risk rollouts, then three device-to-device copies of the bytes k_rollout_risk reads.
* --summarise: k_rollout_risk against that copy x 1.25, the project's yardstick for a read-once kernel (recorded, not gated).
* --bench: bench.py --gpus 1 of this tree and of the parent commit's tree (built, at PARENT_TREE), alternating, each in a fresh process.

The scenario is scripts/gpu_policy_probe.py's: one realised series per instance, realisation c reads the load c steps later.
"""
import csv
import ctypes as C
import glob
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BATCH_MODELS, BATCH_SCEN, K, S = 64, 512, 25, 20
T_ON, T_OFF = 57.5, 60.5
MARGIN = 1.25
LEVELS = (0.05, 0.5, 0.95)


def stat(ms):
    return dict(median_ms=round(float(np.median(ms)), 3), min_ms=round(min(ms), 3), max_ms=round(max(ms), 3), ms=[round(v, 3) for v in ms])


def arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def summarise(d, nbytes):
    seen, rows = {}, []
    for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        rows += list(csv.DictReader(open(f)))
    for r in sorted(rows, key=lambda r: int(r["Start_Timestamp"])):
        name = r["Kernel_Name"].split("(")[0]
        key = "copy_kernel" if "copyBuffer" in name else name
        if key in ("k_rollout_risk", "k_rollout_policy_kpi", "copy_kernel"):
            seen.setdefault(key, []).append(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
    out = dict(kernels={k: dict(calls=len(v), average_ns=float(np.mean(v)), min_ns=float(min(v)), max_ns=float(max(v)), ns=v[-6:]) for k, v in sorted(seen.items())})
    copies = seen.get("copy_kernel", [])
    if len(copies) >= 3 and "k_rollout_risk" in seen:      # the three large ones are this script's
        y = float(np.mean(sorted(copies)[-3:]))
        t = float(np.mean(seen["k_rollout_risk"][-3:]))
        out["k_rollout_risk_yardstick"] = dict(margin=MARGIN, bytes=nbytes, copy_ns=y, kernel_ns=t, over_allowed=t / (y * MARGIN), hit=bool(t <= y * MARGIN),
                                               gated=False, read_GB_per_s=(nbytes / t) if nbytes else None)
    else:
        out["yardstick"] = "the device-to-device copies did not show as kernels in this trace (%d copy kernels seen)" % len(copies)
    if "k_rollout_risk" in seen and "k_rollout_policy_kpi" in seen:
        out["share_of_the_rollout_kernel"] = float(np.mean(seen["k_rollout_risk"][-3:])) / float(np.mean(seen["k_rollout_policy_kpi"][-3:]))
    return out


def d2d_copies(n, reps=3):
    """device-to-device hipMemcpyAsync of n bytes, `reps` times, through the HIP runtime the library has loaded"""
    hip = C.CDLL("libamdhip64.so")
    a, b = C.c_void_p(), C.c_void_p()
    assert hip.hipMalloc(C.byref(a), C.c_size_t(n)) == 0 and hip.hipMalloc(C.byref(b), C.c_size_t(n)) == 0
    assert hip.hipMemset(b, 0, C.c_size_t(n)) == 0
    for _ in range(reps):
        assert hip.hipMemcpyAsync(a, b, C.c_size_t(n), 3, None) == 0      # 3 = hipMemcpyDeviceToDevice
        assert hip.hipDeviceSynchronize() == 0
    hip.hipFree(a); hip.hipFree(b)


def bench_alternating(parent, pairs):
    """bench.py of the two trees, alternating, a fresh process each: the flagship workload does not pass through the rollout, so the two should agree"""
    def line(tree):
        out = subprocess.run([sys.executable, os.path.join(tree, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "3"], cwd=tree, stdout=subprocess.PIPE,
                             universal_newlines=True, timeout=600, check=True).stdout
        return json.loads([l for l in out.splitlines() if l.startswith("{")][-1])
    rec = dict(this=[], parent=[])
    for r in range(pairs):
        for name, tree in (("this", ROOT), ("parent", parent)) if r % 2 == 0 else (("parent", parent), ("this", ROOT)):
            rec[name].append(line(tree))
            print(name, json.dumps(rec[name][-1]), flush=True)
    return rec


def main():
    if "--summarise" in sys.argv or "--bench" in sys.argv:
        rec, path = {}, None
        if "--merge" in sys.argv:
            path = sys.argv[sys.argv.index("--merge") + 1]
            rec = json.load(open(path)) if os.path.exists(path) else {}
        if "--bench" in sys.argv:
            rec["bench_alternating"] = s = bench_alternating(os.path.abspath(sys.argv[sys.argv.index("--bench") + 1]), arg("--pairs", 3))
        else:
            rec["trace"] = s = summarise(sys.argv[sys.argv.index("--summarise") + 1], (rec.get("bytes") or {}).get("k_rollout_risk_reads"))
        print(json.dumps(s, indent=1))
        if path:
            json.dump(rec, open(path, "w"), indent=1)
        return
    import bench
    from pyhybridcontrol_amd import gpu, host, policy, simlog, _lib
    from pyhybridcontrol_amd.aux_resolve import BatchAuxResolver
    kernel_only = "--kernel-only" in sys.argv
    out_path = arg("--out", "")
    pairs = arg("--pairs", 7)
    agents, N_p, N_t, x0, om, midx = bench.make_shard(BATCH_MODELS, BATCH_SCEN, 0)
    d = agents[0]["dims"]
    B, nx, nw = x0.shape[0], d["nx"], d["nomega"]
    mats = [a["mats"] for a in agents]
    model = gpu.GpuModel(mats, d)
    cost = host.stack_costs([host.cost_from_atoms(a["atoms"], d, N_p, N_t) for a in agents])
    p = gpu.GpuProblem(model, N_p, N_t, cost, gap_rel=1e-2, max_nodes=800, max_pivots=40000)
    R = BatchAuxResolver(mats, d, small_lds=True)
    P = policy.ThresholdPolicy.thermostat(T_ON, T_OFF, len(mats), nx=nx)
    kpis = simlog.KpiTable.microgrid(d, n_models=len(mats), price_chan=0)
    Q = len(kpis)
    # a dozen columns: the figures the reference averages over its runs, and their tails
    risk = simlog.RiskTable(kpis, LEVELS)
    risk.add("cost", "kpi_sum", kpi="cost").add("p_imp", "kpi_sum", kpi="p_imp").add("p_exp", "kpi_sum", kpi="p_exp")
    risk.add("mu_over", "kpi_sum", kpi="mu_over", level=0.0).add("mu_under", "kpi_sum", kpi="mu_under", level=0.0)
    risk.add("peak_import", "kpi_max", kpi="p_imp").add("steps_over", "kpi_n_above", kpi="mu_over", level=0.0)
    risk.add("steps_under", "kpi_n_above", kpi="mu_under", level=0.0).add("switches", "switches").add("n_vio", "n_vio", level=0.0)
    risk.add("mu_total", "mu_total", level=0.0).add("worst_vio", "worst_vio", level=1e-6)
    G, L = len(risk), len(LEVELS)
    need = sorted(set(int(s) for s in risk.arrays()["col_src"]))
    T = B * S
    reads = T * (4 + 8 * sum(s in need for s in (0, 1, 2)) + 4 * sum(s in need for s in (3, 4)) + Q * (8 * sum(s in need for s in (5, 6, 7)) + 4 * sum(s in need for s in (8, 9))))
    res = dict(version=_lib.version(), batch=B, models=len(agents), dims={k: int(v) for k, v in d.items()}, N_tilde=N_t, K=K, S=S, T_on=T_ON, T_off=T_OFF,
               kpis=list(kpis.names), columns=list(risk.names), levels=list(LEVELS), pairs=pairs,
               bytes=dict(k_rollout_risk_reads=reads, risk_downloads=B * (G * (3 * 8 + 3 * 4) + G * L * (3 * 8 + 4) + 16),
                          per_trajectory_downloads=T * (3 * 8 + 4 * 4 + Q * (3 * 8 + 4 * 4) + 4)))
    assert nw == nx + 1
    rng = np.random.default_rng(21)
    Tl = K + S
    series = np.tile(om.reshape(B, N_t, nw), (1, Tl // N_t + 1, 1))[:, :Tl].copy()
    series[:, :, nx] += rng.normal(0.0, 800.0, (B, Tl))
    lib = np.concatenate([series[:, :, :nx].reshape(B, Tl * nx), series[:, :, nx].reshape(B, Tl)], axis=1).ravel()
    base = np.arange(B, dtype=np.int64) * Tl * nw
    start = np.ascontiguousarray(np.stack([np.broadcast_to(base[:, None], (B, S)), base[:, None] + Tl * nx + np.arange(S, dtype=np.int64)[None, :]], axis=2))
    plib = rng.uniform(0.5, 2.0, 96 + K)
    pstart = (np.arange(B) % 96).astype(np.int64)
    p.upload(x0, om, midx)
    p.upload_profiles(lib, (nx, 1))
    p.upload_policy(P)
    p.upload_prices(plib, 1)
    on_device = lambda: p.rollout(R, K=K, start=start, policy=True, kpis=kpis, price_start=pstart, risk=risk, per_trajectory=False)
    if kernel_only:
        for _ in range(3):
            res["stats"] = on_device()["stats"]
        d2d_copies(reads)
        print(json.dumps(res))
        R.close(); p.close(); model.close()
        return

    def on_host():
        out = p.rollout(R, K=K, start=start, policy=True, kpis=kpis, price_start=pstart)
        return simlog.rollout_risk_np(out, risk, policy=True)

    wall = dict(rollout_risk_on_device=[], rollout_kpi_plus_rollout_risk_np=[])
    dev = ref = None
    for r in range(pairs + 1):                                  # one warm-up round, then the timed rounds, alternating
        t = time.perf_counter(); dev = on_device(); ms_d = (time.perf_counter() - t) * 1e3
        t = time.perf_counter(); ref = on_host(); ms_h = (time.perf_counter() - t) * 1e3
        print("round %d: rollout(risk, per_trajectory=False) %.1f ms, rollout(kpis) + rollout_risk_np %.1f ms" % (r, ms_d, ms_h), flush=True)
        if r >= 1:
            wall["rollout_risk_on_device"].append(ms_d); wall["rollout_kpi_plus_rollout_risk_np"].append(ms_h)
    res["wall"] = {n: stat(v) for n, v in wall.items()}
    res["host_route_over_device"] = round(res["wall"]["rollout_kpi_plus_rollout_risk_np"]["median_ms"] / res["wall"]["rollout_risk_on_device"]["median_ms"], 2)
    res["stats"] = dev["stats"]
    keys = simlog.RISK_COL_KEYS + simlog.RISK_LEVEL_KEYS + simlog.RISK_COUNTS
    res["device_equals_rollout_risk_np"] = bool(all(np.array_equal(dev["risk"][k], ref[k], equal_nan=True) for k in keys))
    res["means"] = {n: float(np.nanmean(dev["risk"]["mean"][:, j])) for j, n in enumerate(risk.names)}
    R.close(); p.close(); model.close()
    print(json.dumps(res))
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
