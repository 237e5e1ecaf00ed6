"""The open-loop rollout (GpuProblem.rollout, kernel k_rollout) at the bench shard (64 models x 512 scenarios = 32 768 instances), K = 25 steps under
S = 20 realisations, against the stepwise route the library already has: K advancing sim_step(resolve=R) calls for ONE realisation, resolver flagged.

    python scripts/gpu_rollout_probe.py [--out profiles/rollout_probe.json]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python scripts/gpu_rollout_probe.py --kernel-only
    python scripts/gpu_rollout_probe.py --summarise DIR [--merge FILE.json]

* default: rollout(...) with summaries only and the stepwise route ALTERNATING in one session, one warm-up pair and seven timed pairs: median and range of
  both wall times and the ratio per realisation; the counts (trajectories, complete, infeasible, declined); the worst deviation of the rollout from the
  stepwise route on a 256-instance sample.
* --kernel-only: for ONE kernel trace of its own -- two rollouts and three what-if resolving steps (k_small_milp, k_sim_step: the yardstick).
* --summarise: k_rollout per trajectory-step next to k_small_milp + k_sim_step per instance from the trace's csv files (no device needed).

The realisations of an instance are windows of ONE realised series per instance, realisation c starting c steps later: the library stays at
batch x (K + S) x nomega doubles and the windows are cut out on the device.
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

BATCH_MODELS, BATCH_SCEN, K, S = 64, 512, 25, 20


def stat(ms):
    return dict(median_ms=round(float(np.median(ms)), 3), min_ms=round(min(ms), 3), max_ms=round(max(ms), 3), ms=[round(v, 3) for v in ms])


def summarise(d):
    seen = {}
    for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            name = r["Kernel_Name"].split("(")[0]
            if name.startswith("k_"):
                seen.setdefault(name, []).append(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
    out = dict(kernels={k: dict(calls=len(v), average_ns=float(np.mean(v)), min_ns=float(min(v)), max_ns=float(max(v))) for k, v in sorted(seen.items())})
    ks = out["kernels"]
    if all(k in ks for k in ("k_rollout", "k_small_milp", "k_sim_step")):
        B = BATCH_MODELS * BATCH_SCEN
        per_step = ks["k_rollout"]["average_ns"] / (B * S * K)
        yard = (ks["k_small_milp"]["average_ns"] + ks["k_sim_step"]["average_ns"]) / B
        out["per_trajectory_step_ns"] = dict(k_rollout=per_step, k_small_milp_plus_k_sim_step=yard, ratio=per_step / yard, allowed=1.25)
    return out


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
    agents, N_p, N_t, x0, om, midx = bench.make_shard(BATCH_MODELS, BATCH_SCEN, 0)
    d = agents[0]["dims"]
    B, nx, nu, nw = x0.shape[0], d["nx"], d["nu"], d["nomega"]
    assert K <= N_t
    res = dict(version=_lib.version(), batch=B, models=len(agents), dims={k: int(v) for k, v in d.items()}, N_tilde=N_t, K=K, S=S)
    mats = [a["mats"] for a in agents]
    model = gpu.GpuModel(mats, d)
    cost = host.stack_costs([host.cost_from_atoms(a["atoms"], d, N_p, N_t) for a in agents])
    p = gpu.GpuProblem(model, N_p, N_t, cost, gap_rel=1e-2, max_nodes=800, max_pivots=40000)
    R = BatchAuxResolver(mats, d, small_lds=True)
    rng = np.random.default_rng(21)
    T = K + S
    series = np.tile(om.reshape(B, N_t, nw), (1, T // N_t + 1, 1))[:, :T].copy()
    series[:, :, nx] += rng.normal(0.0, 800.0, (B, T))
    lib = np.ascontiguousarray(series).ravel()
    start = ((np.arange(B, dtype=np.int64) * T)[:, None] + np.arange(S, dtype=np.int64)[None, :])[:, :, None] * nw      # (B, S, 1): realisation c starts c steps later
    u_seq = (rng.uniform(size=(B, K, nu)) < 0.4).astype(float)
    p.upload(x0, om, midx)
    p.upload_profiles(lib)
    if kernel_only:
        for _ in range(2):
            out = p.rollout(R, u_seq=u_seq, start=start)
        for _ in range(3):
            p.sim_step(resolve=R, u0=u_seq[:, 0], act_start=np.ascontiguousarray(start[:, 0]), step=0, advance=False, log=False)
        res["stats"] = out["stats"]
        print(json.dumps(res))
        R.close(); p.close(); model.close()
        return

    def stepwise(outputs=False):
        """ONE realisation: K advancing resolving steps from the uploaded state"""
        a0 = np.ascontiguousarray(start[:, 0])
        outs = []
        for k in range(K):
            outs.append(p.sim_step(resolve=R, u0=u_seq[:, k], act_start=a0 if k == 0 else None, step=k, actual=True, advance=True, log=False, outputs=outputs))
        return outs

    wall = dict(rollout=[], stepwise=[])
    stats = None
    for r in range(8):                                           # one warm-up pair, seven timed pairs, alternating
        p.upload(x0, om, midx)
        t = time.perf_counter(); out = p.rollout(R, u_seq=u_seq, start=start); ms_r = (time.perf_counter() - t) * 1e3
        stats = out["stats"]
        t = time.perf_counter(); stepwise(); ms_s = (time.perf_counter() - t) * 1e3
        if r >= 1:
            wall["rollout"].append(ms_r); wall["stepwise"].append(ms_s)
    res["wall"] = {n: stat(v) for n, v in wall.items()}
    mr, msw = res["wall"]["rollout"]["median_ms"], res["wall"]["stepwise"]["median_ms"]
    res["per_realisation"] = dict(rollout_ms=round(mr / S, 3), stepwise_ms=msw, ratio=round(msw / (mr / S), 2))
    res["stats"] = stats
    res["end_status_counts"] = {str(k): int((out["end_status"] == k).sum()) for k in (-1, 0, 1, 2)}
    print("wall:", res["wall"], res["per_realisation"], stats, flush=True)
    # the worst deviation from the stepwise route on a 256-instance sample, every realisation
    n = 256
    p.upload(x0[:n], om[:n], midx[:n])
    got = p.rollout(R, u_seq=u_seq[:n], start=start[:n], trajectories=True)
    worst, equal = 0.0, True
    for c in range(S):
        p.upload(x0[:n], om[:n], midx[:n])
        a0 = np.ascontiguousarray(start[:n, c])
        for k in range(K):
            o = p.sim_step(resolve=R, u0=u_seq[:n, k], act_start=a0 if k == 0 else None, step=k, actual=True, advance=True, log=False, outputs=True)
            ok = got["steps_done"][:, c] > k
            equal = equal and bool(np.array_equal(ok, o["aux_status"] == 0)) and bool(np.array_equal(got["v"][ok, c, k, :nu + 1], o["v0"][ok, :nu + 1]))
            for a, b in ((got["x"][ok, c, k + 1], o["x_k1"][ok]), (got["v"][ok, c, k], o["v0"][ok]), (got["cons_vio"][ok, c, k], o["cons_vio"][ok])):
                if a.size:
                    worst = max(worst, float((np.abs(a - b) / np.maximum(1.0, np.abs(b))).max()))
    res["sample"] = dict(instances=n, realisations=S, steps=K, binaries_and_endings_equal=equal, worst_deviation=worst, stats=got["stats"])
    print("sample:", res["sample"], flush=True)
    R.close(); p.close(); model.close()
    print(json.dumps(res))
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
