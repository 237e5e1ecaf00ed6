"""Rollout KPIs on the device (GpuProblem.rollout(kpis=...), mld_rollout_kpi; kernels k_rollout_kpi, k_rollout_policy_kpi) at the bench shard (64 models x
512 scenarios = 32 768 instances), K = 25 steps under S = 20 realisations, the reference's 8 microgrid columns (simlog.KpiTable.microgrid, cost priced).

    python scripts/gpu_rollout_kpi_probe.py [--out profiles/rollout_kpi_probe.json] [--pairs 7] [--np-reps 7] [--np-instances N]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python scripts/gpu_rollout_kpi_probe.py --kernel-only
    python scripts/gpu_rollout_kpi_probe.py --summarise DIR [--merge FILE.json]

* default: rollout(policy=True, kpis=...) against the two routes the parent commit has for the same figures, ALTERNATING in one session, one warm-up round
  and --pairs timed rounds: (a) rollout(policy=True, trajectories=True) plus simlog.rollout_kpis_np on the host -- on the first --np-instances instances
  (default: all) and --np-reps of the rounds, because it downloads batch x S x K x (nx + nv + ny) doubles and reduces them on one core --; (b) the stepwise
  logged campaign of ONE realisation, K sim_step(resolve=R, policy=True) calls with the stage cost armed, plus sim_log_summary.  Medians and ranges, the
  counts, and whether the three routes give the same bits on a 256-instance sample.
* --kernel-only: for ONE kernel trace of its own -- two rollouts each of k_rollout_policy_kpi, k_rollout_policy, k_rollout_kpi and k_rollout on identical
  inputs (the open-loop pair's u_seq is the policy's inputs).
* --summarise: each KPI kernel per trajectory-step against the kernel it extends (allowed: 1.25 x; recorded, not gated).

The scenario is scripts/gpu_policy_probe.py's: one realised series per instance, realisation c reads the load c steps later.
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
T_ON, T_OFF = 57.5, 60.5
MARGIN = 1.25
PAIRS = (("k_rollout_policy_kpi", "k_rollout_policy"), ("k_rollout_kpi", "k_rollout"))


def stat(ms):
    return dict(median_ms=round(float(np.median(ms)), 3), min_ms=round(min(ms), 3), max_ms=round(max(ms), 3), ms=[round(v, 3) for v in ms])


def arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def summarise(d):
    seen, rows = {}, []
    for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        rows += list(csv.DictReader(open(f)))
    for r in sorted(rows, key=lambda r: int(r["Start_Timestamp"])):
        name = r["Kernel_Name"].split("(")[0]
        if name.startswith("k_rollout"):
            seen.setdefault(name, []).append(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
    out = dict(kernels={k: dict(calls=len(v), average_ns=float(np.mean(v)), min_ns=float(min(v)), max_ns=float(max(v))) for k, v in sorted(seen.items())})
    n = BATCH_MODELS * BATCH_SCEN * S * K
    out["per_trajectory_step_ns"] = {}
    for new, old in PAIRS:      # the last two launches of each are the full-size ones
        if len(seen.get(new, [])) >= 2 and len(seen.get(old, [])) >= 2:
            a, b = float(np.mean(seen[new][-2:])) / n, float(np.mean(seen[old][-2:])) / n
            out["per_trajectory_step_ns"][new] = dict(ns=a, yardstick=old, yardstick_ns=b, ratio=a / b, allowed=MARGIN, hit=bool(a / b <= MARGIN), gated=False)
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
    from pyhybridcontrol_amd import gpu, host, policy, prices, simlog, _lib
    from pyhybridcontrol_amd.aux_resolve import BatchAuxResolver
    kernel_only = "--kernel-only" in sys.argv
    out_path = arg("--out", "")
    pairs, np_reps = arg("--pairs", 7), arg("--np-reps", 7)
    agents, N_p, N_t, x0, om, midx = bench.make_shard(BATCH_MODELS, BATCH_SCEN, 0)
    d = agents[0]["dims"]
    B, nx, nu, nw = x0.shape[0], d["nx"], d["nu"], d["nomega"]
    n_np = min(B, arg("--np-instances", B))
    mats = [a["mats"] for a in agents]
    model = gpu.GpuModel(mats, d)
    cost = host.stack_costs([host.cost_from_atoms(a["atoms"], d, N_p, N_t) for a in agents])
    p = gpu.GpuProblem(model, N_p, N_t, cost, gap_rel=1e-2, max_nodes=800, max_pivots=40000)
    R = BatchAuxResolver(mats, d, small_lds=True)
    P = policy.ThresholdPolicy.thermostat(T_ON, T_OFF, len(mats), nx=nx)
    kpis = simlog.KpiTable.microgrid(d, n_models=len(mats), price_chan=0)
    res = dict(version=_lib.version(), batch=B, models=len(agents), dims={k: int(v) for k, v in d.items()}, N_tilde=N_t, K=K, S=S, T_on=T_ON, T_off=T_OFF,
               kpis=list(kpis.names), pairs=pairs, np_reps=np_reps, np_instances=n_np)
    assert nw == nx + 1
    rng = np.random.default_rng(21)
    T = K + S
    series = np.tile(om.reshape(B, N_t, nw), (1, T // N_t + 1, 1))[:, :T].copy()
    series[:, :, nx] += rng.normal(0.0, 800.0, (B, T))
    lib = np.concatenate([series[:, :, :nx].reshape(B, T * nx), series[:, :, nx].reshape(B, T)], axis=1).ravel()
    base = np.arange(B, dtype=np.int64) * T * nw
    start = np.ascontiguousarray(np.stack([np.broadcast_to(base[:, None], (B, S)), base[:, None] + T * nx + np.arange(S, dtype=np.int64)[None, :]], axis=2))
    plib = rng.uniform(0.5, 2.0, 96 + K)                      # one tariff of a day and K steps, every instance begins at its own quarter hour
    pstart = (np.arange(B) % 96).astype(np.int64)
    p.upload(x0, om, midx)
    p.upload_profiles(lib, (nx, 1))
    p.upload_policy(P)
    p.upload_prices(plib, 1)
    if kernel_only:
        one = p.rollout(R, K=K, start=np.ascontiguousarray(start[:, :1]), policy=True, trajectories=True)
        u_pol = np.ascontiguousarray(one["v"][:, 0, :, :nu])
        u_pol = np.where(np.isfinite(u_pol), u_pol, 0.0)
        del one
        st = {}
        for _ in range(2):
            st["policy_kpi"] = p.rollout(R, K=K, start=start, policy=True, kpis=kpis, price_start=pstart)["stats"]
        for _ in range(2):
            st["policy"] = p.rollout(R, K=K, start=start, policy=True)["stats"]
        for _ in range(2):
            st["open_loop_kpi"] = p.rollout(R, u_seq=u_pol, start=start, kpis=kpis, price_start=pstart)["stats"]
        for _ in range(2):
            st["open_loop"] = p.rollout(R, u_seq=u_pol, start=start)["stats"]
        res["stats"] = st
        print(json.dumps(res))
        R.close(); p.close(); model.close()
        return

    def logged(n=B, c=0):
        """ONE realisation by the stepwise route: a log begun, the stage cost armed, K logged advancing policy steps, then the summary on the device"""
        p.sim_log_begin(K)
        p.sim_log_cost_begin(pstart[:n])
        a0 = np.ascontiguousarray(start[:n, c])
        for k in range(K):
            p.sim_step(resolve=R, policy=True, act_start=a0 if k == 0 else None, step=k, actual=True, advance=True, log=True)
        return p.sim_log_summary(kpis)

    def by_numpy(n):
        tr = p.rollout(R, K=K, start=start[:n], policy=True, trajectories=True)
        price = prices.windows(plib, pstart[:n], 0, K, 1).reshape(n, K, 1)
        return tr, simlog.rollout_kpis_np(tr, kpis, price=price, model_idx=midx[:n])

    p.set_stage_cost(w_v=np.eye(model.nv)[d["nu"] + d["ndelta"]])
    wall = dict(rollout_kpi=[], rollout_summaries_only=[], logged_campaign_one_realisation=[], trajectories_plus_numpy=[])
    stats = None
    for r in range(pairs + 1):                                  # one warm-up round, then the timed rounds, alternating
        p.upload(x0, om, midx)
        t = time.perf_counter(); out = p.rollout(R, K=K, start=start, policy=True, kpis=kpis, price_start=pstart); ms_k = (time.perf_counter() - t) * 1e3
        stats = out["stats"]
        t = time.perf_counter(); p.rollout(R, K=K, start=start, policy=True); ms_p = (time.perf_counter() - t) * 1e3
        t = time.perf_counter(); logged(); ms_l = (time.perf_counter() - t) * 1e3
        ms_n = None
        if r == 0 or r <= np_reps:
            p.upload(x0[:n_np], om[:n_np], midx[:n_np])
            t = time.perf_counter(); by_numpy(n_np); ms_n = (time.perf_counter() - t) * 1e3
        print("round %d: rollout(kpis) %.1f ms, rollout %.1f ms, logged campaign (1 realisation) %.1f ms, trajectories + numpy (%d instances) %s ms"
              % (r, ms_k, ms_p, ms_l, n_np, "%.1f" % ms_n if ms_n is not None else "-"), flush=True)
        if r >= 1:
            wall["rollout_kpi"].append(ms_k); wall["rollout_summaries_only"].append(ms_p); wall["logged_campaign_one_realisation"].append(ms_l)
            if ms_n is not None:
                wall["trajectories_plus_numpy"].append(ms_n)
    res["wall"] = {n: stat(v) for n, v in wall.items() if v}
    mk = res["wall"]["rollout_kpi"]["median_ms"]
    res["per_realisation"] = dict(rollout_kpi_ms=round(mk / S, 3), logged_campaign_ms=res["wall"]["logged_campaign_one_realisation"]["median_ms"],
                                  ratio=round(res["wall"]["logged_campaign_one_realisation"]["median_ms"] / (mk / S), 2))
    if "trajectories_plus_numpy" in res["wall"]:
        mn = res["wall"]["trajectories_plus_numpy"]["median_ms"]
        res["against_numpy"] = dict(instances=n_np, numpy_ms_per_instance=mn / n_np, rollout_kpi_ms_per_instance=mk / B, ratio=round((mn / n_np) / (mk / B), 2))
    res["stats"] = stats
    res["kpi_means"] = {n: float(np.nanmean(out["kpi"]["sum"][..., q])) for q, n in enumerate(kpis.names)}
    # the three routes on a 256-instance sample: the same bits?
    n = 256
    p.upload(x0[:n], om[:n], midx[:n])
    dev = p.rollout(R, K=K, start=start[:n], policy=True, kpis=kpis, price_start=pstart[:n])
    tr, ref = by_numpy(n)
    keys = simlog.KPI_ROLLOUT_KEYS
    same_np = all(np.array_equal(dev["kpi"][k], ref[k], equal_nan=True) for k in keys)
    same_log = True
    for c in range(S):
        p.upload(x0[:n], om[:n], midx[:n])
        s = logged(n, c)
        done = dev["end_status"][:, c] == 0
        same_log = same_log and all(np.array_equal(dev["kpi"][k][done, c], s[k][done], equal_nan=True) for k in keys)
    res["sample"] = dict(instances=n, realisations=S, equals_rollout_kpis_np=bool(same_np), equals_logged_campaign=bool(same_log), stats=dev["stats"])
    print("sample:", res["sample"], flush=True)
    p.sim_log_begin(0)
    R.close(); p.close(); model.close()
    print(json.dumps(res))
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
