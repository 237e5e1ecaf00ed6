"""Device completion of declined rollout trajectories at the cfg4 shard, on the UNREPLACED instances (complete="device"; kernels k_ro_collect, k_rollout_redo_kpi,
k_ro_fix_merge, and k_solve on the resolver's handle): the shard, KPIs, risk columns, band and inputs of scripts/gpu_select_policy_probe.py -- 32 768
instances, K = 25, S = 20, the thermostat in closed loop, the 12 microgrid KPIs and 12 risk columns --, nothing redrawn.

    python scripts/gpu_rollout_complete_probe.py --out profiles/rollout_complete_probe.json [--pairs 7] [--no-host]
    python scripts/gpu_rollout_complete_probe.py --kernel-only            # three device-completing calls and three on the replaced shard, for a kernel trace

(a) rollout(policy=True, kpis=, risk=, per_trajectory=False, complete="device") against the same call with complete="host" -- the route every consumer had:
    the call repeated with trajectories=True, everything downloaded, the rest in numpy.  The host call runs ONCE (--no-host skips it).
(b) the same call on the REPLACED shard, where nothing declines (an instance with a declined trajectory takes the inputs of the nearest instance of its model
    that has none, as the older probes do), routes alternating, medians of --pairs.  The yardstick for (a) minus (b) is rounds x (one dense solve of a list
    that small on the resolver + one k_rollout_redo_kpi launch), both read from a kernel trace of their own; allowed 1.25 x; recorded, not gated.
The risk of the two routes on the unreplaced shard is compared: equal bits for the instances without a declined trajectory, within 1e-6 relative for the
others (the completions differ in the right-hand side's summation order)."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import gpu_plan_select_probe as base      # noqa: E402  (stat, arg)

BATCH_MODELS, BATCH_SCEN, K, S = 64, 512, 25, 20
LEVELS = (0.05, 0.5, 0.95)
BAND = (57.5, 60.5)
MARGIN = 1.25


def main():
    import bench
    from pyhybridcontrol_amd import gpu, host, policy, simlog, _lib
    from pyhybridcontrol_amd.aux_resolve import BatchAuxResolver
    kernel_only, no_host = "--kernel-only" in sys.argv, "--no-host" in sys.argv
    out_path, pairs = base.arg("--out", ""), base.arg("--pairs", 7)
    agents, N_p, N_t, x0, om, midx = bench.make_shard(BATCH_MODELS, BATCH_SCEN, 0)
    d = agents[0]["dims"]
    B, nx, nw, nu = x0.shape[0], d["nx"], d["nomega"], d["nu"]
    mats = [a["mats"] for a in agents]
    model = gpu.GpuModel(mats, d)
    cost = host.stack_costs([host.cost_from_atoms(a["atoms"], d, N_p, N_t) for a in agents])
    p = gpu.GpuProblem(model, N_p, N_t, cost, gap_rel=1e-2, max_nodes=800, max_pivots=40000)
    R = BatchAuxResolver(mats, d, small_lds=True)
    kpis = simlog.KpiTable.microgrid(d, n_models=len(mats), price_chan=0)
    risk = simlog.RiskTable(kpis, LEVELS)
    risk.add("cost", "kpi_sum", kpi="cost").add("p_imp", "kpi_sum", kpi="p_imp").add("p_exp", "kpi_sum", kpi="p_exp")
    risk.add("mu_over", "kpi_sum", kpi="mu_over", level=0.0).add("mu_under", "kpi_sum", kpi="mu_under", level=0.0)
    risk.add("peak_import", "kpi_max", kpi="p_imp").add("steps_over", "kpi_n_above", kpi="mu_over", level=0.0)
    risk.add("steps_under", "kpi_n_above", kpi="mu_under", level=0.0).add("cost_max", "kpi_max", kpi="cost").add("n_vio", "n_vio", level=0.0)
    risk.add("mu_total", "mu_total", level=0.0).add("switches", "switches", level=0.0)
    assert nw == nx + 1 and nu == nx
    thermo = policy.ThresholdPolicy(np.broadcast_to(np.eye(nx), (len(mats), nu, nx)), *BAND)
    res = dict(version=_lib.version(), batch=B, models=len(agents), dims={k: int(v) for k, v in d.items()}, N_tilde=N_t, K=K, S=S, band=list(BAND),
               kpis=list(kpis.names), columns=list(risk.names), levels=list(LEVELS), pairs=pairs, margin=MARGIN)
    rng = np.random.default_rng(21)
    Tl = K + S
    series = np.tile(om.reshape(B, N_t, nw), (1, Tl // N_t + 1, 1))[:, :Tl].copy()
    series[:, :, nx] += rng.normal(0.0, 800.0, (B, Tl))
    lib = np.concatenate([series[:, :, :nx].reshape(B, Tl * nx), series[:, :, nx].reshape(B, Tl)], axis=1).ravel()
    plib = rng.uniform(0.5, 2.0, 96 + K)
    up = (rng.uniform(size=(B, nu)) < 0.5).astype(float)
    p.upload_profiles(lib, (nx, 1))
    p.upload_prices(plib, 1)
    p.upload_policy(thermo)

    def load(src):
        """instance b runs the inputs of instance src[b]; returns the call's keyword arguments"""
        basep = src * Tl * nw
        start = np.ascontiguousarray(np.stack([np.broadcast_to(basep[:, None], (B, S)), basep[:, None] + Tl * nx + np.arange(S, dtype=np.int64)[None, :]], axis=2))
        p.upload(np.ascontiguousarray(x0[src]), np.ascontiguousarray(om[src]), midx)
        return dict(K=K, policy=True, u_prev=np.ascontiguousarray(up[src]), start=start, kpis=kpis, price_start=(src % 96).astype(np.int64), risk=risk, per_trajectory=False)

    drawn = np.arange(B, dtype=np.int64)
    # the replaced shard.  The instances with a declined trajectory are named by an entry that finishes nothing (the thermostat as the only candidate of a
    # selection: the same closed loop, its n_declined per instance); rollout(complete=None) would finish them on the host, which this probe times once
    src, replaced = drawn.copy(), []
    only = simlog.PlanSelector(risk).minimise("cost", "mean")
    for _ in range(5):
        kw = load(src)
        raw = p.select_plan_policies(R, only, policies=[thermo], u_prev=kw["u_prev"], K=K, start=kw["start"], kpis=kpis,
                                     price_start=kw["price_start"], per_candidate=True)["risk"]["n_declined"][:, 0]
        bad = np.flatnonzero(raw > 0)
        replaced.append(int(bad.size))
        if len(replaced) == 1:
            res["unreplaced"] = dict(instances_with_a_declined_trajectory=int(bad.size), declined_trajectories=int(raw.sum()))
        if not bad.size:
            break
        clean = raw == 0
        for b in bad:
            same = np.flatnonzero(clean & (midx == midx[b]))
            src[b] = src[same[np.argmin(np.abs(same - b))]]
    else:
        sys.exit("trajectories are still declined after 5 rounds: %s" % (replaced,))
    res["instances_replaced_for_b"] = replaced

    def device():
        kw = load(drawn)
        t = time.perf_counter(); out = p.rollout(R, complete="device", **kw); ms = (time.perf_counter() - t) * 1e3
        return out, ms, p.rollout_completion_stats()

    def replaced_shard():
        kw = load(src)
        t = time.perf_counter(); out = p.rollout(R, complete="device", **kw); ms = (time.perf_counter() - t) * 1e3
        return out, ms

    if kernel_only:
        for _ in range(3):
            res["completion"] = device()[2]
        for _ in range(3):
            replaced_shard()
        print(json.dumps(res))
        R.close(); p.close(); model.close()
        return
    wall = dict(device_unreplaced=[], device_replaced=[])
    dev = None
    for r in range(pairs + 1):      # one warm-up round, then the timed rounds, alternating
        dev, ms_a, cs = device()
        _, ms_b = replaced_shard()
        print("round %d: complete=\"device\" on the unreplaced shard %.1f ms (%s), on the replaced shard %.1f ms" % (r, ms_a, cs, ms_b), flush=True)
        if r >= 1:
            wall["device_unreplaced"].append(ms_a); wall["device_replaced"].append(ms_b)
    res["wall"] = {n: base.stat(v) for n, v in wall.items()}
    res["completion"] = cs
    res["stats"] = dev["stats"]
    res["a_minus_b_ms"] = res["wall"]["device_unreplaced"]["median_ms"] - res["wall"]["device_replaced"]["median_ms"]
    res["yardstick"] = "rounds x (one dense resolver solve of the list + one k_rollout_redo_kpi launch), from a kernel trace of --kernel-only: not taken by this run"
    if not no_host:
        kw = load(drawn)
        t = time.perf_counter(); ref = p.rollout(R, complete="host", **kw); ms_h = (time.perf_counter() - t) * 1e3
        res["host_route_once_ms"] = ms_h
        res["host_route_over_device"] = round(ms_h / res["wall"]["device_unreplaced"]["median_ms"], 1)
        res["host_stats"] = ref["stats"]
        keys = simlog.RISK_COL_KEYS + simlog.RISK_LEVEL_KEYS
        worst = 0.0
        for k in keys:
            a, b = np.asarray(dev["risk"][k], float), np.asarray(ref["risk"][k], float)
            ok = np.isfinite(a) & np.isfinite(b)
            if ok.any():
                worst = max(worst, float((np.abs(a - b)[ok] / np.maximum(1.0, np.abs(b[ok]))).max()))
        res["risk_device_against_host_worst_relative"] = worst
        res["risk_counts_equal"] = all(bool(np.array_equal(dev["risk"][k], ref["risk"][k])) for k in simlog.RISK_COUNTS)
    R.close(); p.close(); model.close()
    print(json.dumps(res))
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
