"""Plan selection with a closed-loop policy among the candidates (GpuProblem.select_plan_policies(policies=...), mld_rollout_select_policy; kernels
k_rollout_cand_policy_kpi, k_rollout_risk, k_plan_select, k_select_inputs) at the bench shard (64 models x 512 scenarios = 32 768 instances), K = 25 steps
under S = 20 realisations, 3 candidate input sequences and 1 thermostat, the microgrid KPIs and the risk columns of scripts/gpu_plan_select_probe.py.

    python scripts/gpu_select_policy_probe.py [--out profiles/select_policy_probe.json] [--pairs 7]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python scripts/gpu_select_policy_probe.py --kernel-only
    python scripts/gpu_select_policy_probe.py --summarise DIR [--merge FILE.json]
    python scripts/gpu_select_policy_probe.py --bench PARENT_TREE [--merge FILE.json] [--pairs 3]

* default: wall time of select_plan_policies(policies=[P]) against the route the parent commit has for the same choice -- select_plan for the sequences
  (per_candidate=True), upload_policy(P), rollout(policy=True, kpis, risk, per_trajectory=False), upload_policy(None), then the merge of the two risks and
  simlog.select_plan_np on the host -- ALTERNATING in one session: one warm-up round, then --pairs timed rounds, the figure is the median.  Whether the two give
  the same bits, and the bytes each route moves.
* --kernel-only: for ONE kernel trace of its own on identical inputs -- three selections with the policy, three selections of the sequences alone
  (k_rollout_cand_kpi), three policy rollouts (k_rollout_policy_kpi), then three device-to-device copies of the bytes k_select_inputs writes.
* --summarise: k_rollout_cand_policy_kpi in ns per trajectory-step against the two kernels that exist unchanged in the parent, k_rollout_cand_kpi for the
  sequence candidates and k_rollout_policy_kpi for the policy candidate (the standing margin of a rollout variant, 1.25 x; recorded, not gated), and
  k_select_inputs against that copy x 1.25 (recorded, not gated).
* --bench: bench.py --gpus 1 of this tree and of the parent commit's tree (built, at PARENT_TREE), alternating, each in a fresh process.

The new entry finishes nothing on the host; the parent's route does, downloading every trajectory.  An instance with a trajectory the LDS solver declines
(a few in a million) is REPLACED before anything is timed by a neighbour of the same model that has none, so the inputs are changed and the host-completion
route is never measured here; the count is recorded as `instances_replaced`.  --unreplaced keeps the shard as drawn and passes complete="device" to every
call of both routes instead (the trajectories are finished on the device); the default is what it was.
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import gpu_plan_select_probe as base      # noqa: E402  (stat, arg, d2d_copies, bench_alternating, the trace reader's conventions)

BATCH_MODELS, BATCH_SCEN, K, S, N_SEQ = 64, 512, 25, 20, 3
P = N_SEQ + 1
MARGIN = 1.25
LEVELS = (0.05, 0.5, 0.95)
DUTY = 0.4
BAND = (57.5, 60.5)
NAMES = ("k_rollout_cand_policy_kpi", "k_rollout_cand_kpi", "k_rollout_policy_kpi", "k_rollout_risk", "k_plan_select", "k_select_inputs", "copy_kernel")


def summarise(d, rec):
    import csv
    import glob
    seen, rows = {}, []
    for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        rows += list(csv.DictReader(open(f)))
    for r in sorted(rows, key=lambda r: int(r["Start_Timestamp"])):
        name = r["Kernel_Name"].split("(")[0]
        key = "copy_kernel" if "copyBuffer" in name else name
        if key in NAMES:
            seen.setdefault(key, []).append(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
    out = dict(kernels={k: dict(calls=len(v), average_ns=float(np.mean(v)), min_ns=float(min(v)), max_ns=float(max(v)), ns=v[-12:]) for k, v in sorted(seen.items())})
    B = rec.get("batch", BATCH_MODELS * BATCH_SCEN)
    new, seq, pol = seen.get("k_rollout_cand_policy_kpi", []), seen.get("k_rollout_cand_kpi", []), seen.get("k_rollout_policy_kpi", [])
    if len(new) >= 3 and len(seq) >= 3 and len(pol) >= 3:      # the last three of each are this script's
        t_new, t_seq, t_pol = float(np.mean(new[-3:])), float(np.mean(seq[-3:])), float(np.mean(pol[-3:]))
        per = dict(k_rollout_cand_policy_kpi=t_new / (B * P * S * K), k_rollout_cand_kpi=t_seq / (B * N_SEQ * S * K), k_rollout_policy_kpi=t_pol / (B * S * K))
        out["ns_per_trajectory_step"] = per
        out["k_rollout_cand_policy_kpi_against_the_parents_kernels"] = dict(
            margin=MARGIN, new_ns=t_new, sequences_ns=t_seq, policy_ns=t_pol, ratio_to_their_sum=t_new / (t_seq + t_pol),
            ratio_per_step_to_k_rollout_cand_kpi=per["k_rollout_cand_policy_kpi"] / per["k_rollout_cand_kpi"],
            ratio_per_step_to_k_rollout_policy_kpi=per["k_rollout_cand_policy_kpi"] / per["k_rollout_policy_kpi"],
            hit=bool(t_new <= MARGIN * (t_seq + t_pol)), gated=False)
    copies = seen.get("copy_kernel", [])
    if len(copies) >= 3 and "k_select_inputs" in seen:
        y, t = float(np.mean(sorted(copies)[-3:])), float(np.mean(seen["k_select_inputs"][-3:]))
        out["k_select_inputs_yardstick"] = dict(margin=MARGIN, bytes=(rec.get("bytes") or {}).get("k_select_inputs_writes"), copy_ns=y, kernel_ns=t,
                                                over_allowed=t / (y * MARGIN), hit=bool(t <= y * MARGIN), gated=False)
    else:
        out["yardstick"] = "the device-to-device copies did not show as kernels in this trace (%d copy kernels seen)" % len(copies)
    return out


def main():
    if "--summarise" in sys.argv or "--bench" in sys.argv:
        rec, path = {}, None
        if "--merge" in sys.argv:
            path = sys.argv[sys.argv.index("--merge") + 1]
            rec = json.load(open(path)) if os.path.exists(path) else {}
        if "--bench" in sys.argv:
            rec["bench_alternating"] = s = base.bench_alternating(os.path.abspath(sys.argv[sys.argv.index("--bench") + 1]), base.arg("--pairs", 3))
        else:
            rec["trace"] = s = summarise(sys.argv[sys.argv.index("--summarise") + 1], rec)
        print(json.dumps(s, indent=1))
        if path:
            json.dump(rec, open(path, "w"), indent=1)
        return
    import bench
    from pyhybridcontrol_amd import gpu, host, policy, simlog, _lib
    from pyhybridcontrol_amd.aux_resolve import BatchAuxResolver
    kernel_only = "--kernel-only" in sys.argv
    unreplaced = "--unreplaced" in sys.argv      # the shard as drawn: declined trajectories are finished on the device (complete="device"), by both routes
    how = dict(complete="device") if unreplaced else {}
    out_path = base.arg("--out", "")
    pairs = base.arg("--pairs", 7)
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
    risk.add("mu_total", "mu_total", level=0.0).add("worst_vio", "worst_vio", level=1e-6)
    sel = simlog.PlanSelector(risk).minimise("cost", "cvar_hi", level=0.95).subject_to("steps_under", "mean", 0.5 * K).subject_to("mu_under", "cvar_hi", 1e4, level=0.95)
    G, L = len(risk), len(LEVELS)
    assert nw == nx + 1 and nu == nx
    thermo = policy.ThresholdPolicy(np.broadcast_to(np.eye(nx), (len(mats), nu, nx)), *BAND)
    seq = B * K * nu * 8
    per_cand_down = B * (G * (3 * 8 + 3 * 4) + G * L * (3 * 8 + 4) + 16)
    pick_down = B * (4 + 8 + 4) + seq + B * nu * 8
    res = dict(version=_lib.version(), batch=B, models=len(agents), dims={k: int(v) for k, v in d.items()}, N_tilde=N_t, K=K, S=S, sequences=N_SEQ, policies=1, band=list(BAND),
               duty=DUTY, kpis=list(kpis.names), columns=list(risk.names), levels=list(LEVELS), pairs=pairs,
               bytes=dict(k_select_inputs_writes=seq + B * nu * 8,
                          select_plan_with_policies=dict(uploads=B * N_SEQ * K * nu * 8 + B * S * 2 * 8 + B * nu * 8 + 2 * len(mats) * nu * (nx + 5) * 8,
                                                         downloads=pick_down + B * P + B * P * 16),
                          parents_route=dict(uploads=B * N_SEQ * K * nu * 8 + 2 * B * S * 2 * 8 + B * nu * 8 + len(mats) * nu * (nx + 5) * 8,
                                             downloads=pick_down + B * N_SEQ + (N_SEQ + 1) * per_cand_down),
                          omega_windows_gathered_per_call=B * S * K * nw * 8, omega_window_gathers=dict(select_plan_with_policies=1, parents_route=2)))
    rng = np.random.default_rng(21)
    Tl = K + S
    series = np.tile(om.reshape(B, N_t, nw), (1, Tl // N_t + 1, 1))[:, :Tl].copy()
    series[:, :, nx] += rng.normal(0.0, 800.0, (B, Tl))
    lib = np.concatenate([series[:, :, :nx].reshape(B, Tl * nx), series[:, :, nx].reshape(B, Tl)], axis=1).ravel()
    at = np.arange(B, dtype=np.int64)
    plib = rng.uniform(0.5, 2.0, 96 + K)
    cand = np.ascontiguousarray((rng.uniform(size=(B, N_SEQ, K, nu)) < DUTY).astype(float))
    up = (rng.uniform(size=(B, nu)) < 0.5).astype(float)
    src = at.copy()      # instance b runs the inputs of instance src[b]

    def inputs():
        basep = src * Tl * nw
        start = np.ascontiguousarray(np.stack([np.broadcast_to(basep[:, None], (B, S)), basep[:, None] + Tl * nx + np.arange(S, dtype=np.int64)[None, :]], axis=2))
        return np.ascontiguousarray(cand[src]), np.ascontiguousarray(up[src]), start, (src % 96).astype(np.int64)

    p.upload_profiles(lib, (nx, 1))
    p.upload_prices(plib, 1)
    replaced = []
    for _ in range(1 if unreplaced else 5):      # an instance with a declined trajectory takes the inputs of the nearest instance of its model that has none
        cd, upv, start, pstart = inputs()
        p.upload(np.ascontiguousarray(x0[src]), np.ascontiguousarray(om[src]), midx)
        n_dec = p.select_plan_policies(R, sel, candidates=cd, policies=[thermo], u_prev=upv, start=start, kpis=kpis, price_start=pstart, per_candidate=True)["risk"]["n_declined"]
        bad = np.flatnonzero(n_dec.any(axis=1))
        replaced.append(int(bad.size))
        if not bad.size or unreplaced:
            break
        clean = ~n_dec.any(axis=1)
        for b in bad:
            same = np.flatnonzero(clean & (midx == midx[b]))
            src[b] = src[same[np.argmin(np.abs(same - b))]]
    else:
        sys.exit("trajectories are still declined after 5 rounds: %s" % (replaced,))
    if unreplaced:      # (c) of the device completion's measurement: the candidates that were inadmissible only because of a decline
        res["unreplaced"] = dict(instances_with_a_declined_trajectory=replaced[0], candidates_with_a_declined_trajectory=int((n_dec > 0).sum()))
    else:
        res["instances_replaced"] = replaced
    on_device = lambda **kw: p.select_plan_policies(R, sel, candidates=cd, policies=[thermo], u_prev=upv, start=start, kpis=kpis, price_start=pstart, **dict(how, **kw))
    sequences = lambda **kw: p.select_plan(R, sel, candidates=cd, start=start, kpis=kpis, price_start=pstart, **dict(how, **kw))

    def closed_loop():
        p.upload_policy(thermo)
        try:
            return p.rollout(R, K=K, policy=True, u_prev=upv, start=start, kpis=kpis, price_start=pstart, risk=risk, per_trajectory=False, **how)
        finally:
            p.upload_policy(None)

    if kernel_only:
        for _ in range(3):
            res["stats"] = on_device()["stats"]
        for _ in range(3):
            sequences()
        for _ in range(3):
            closed_loop()
        base.d2d_copies(res["bytes"]["k_select_inputs_writes"])
        print(json.dumps(res))
        R.close(); p.close(); model.close()
        return

    keys = simlog.RISK_COL_KEYS + simlog.RISK_LEVEL_KEYS + simlog.RISK_COUNTS
    xin = np.ascontiguousarray(x0[src])

    def parents_route():
        a, b = sequences(per_candidate=True), closed_loop()
        full = {k: np.concatenate([a["risk"][k], b["risk"][k][:, None]], axis=1) for k in keys}
        return full, simlog.select_plan_np(full, sel, S, candidates=cd, policy_u0=policy.apply_np(thermo, midx, xin, upv)[:, None])

    wall = dict(select_plan_with_policies=[], parents_route=[])
    dev = ref = None
    for r in range(pairs + 1):                                  # one warm-up round, then the timed rounds, alternating
        t = time.perf_counter(); dev = on_device(); ms_d = (time.perf_counter() - t) * 1e3
        t = time.perf_counter(); ref = parents_route(); ms_h = (time.perf_counter() - t) * 1e3
        print("round %d: select_plan_policies(policies) %.1f ms, select_plan + upload_policy + rollout(policy) + merge + select_plan_np %.1f ms" % (r, ms_d, ms_h), flush=True)
        if dev["stats"]["declined"] and not unreplaced:
            sys.exit("trajectories were declined (%s): the parent's route would finish them on the host, which this probe does not measure" % (dev["stats"],))
        if r >= 1:
            wall["select_plan_with_policies"].append(ms_d); wall["parents_route"].append(ms_h)
    res["wall"] = {n: base.stat(v) for n, v in wall.items()}
    res["parents_route_over_select_plan_with_policies"] = round(res["wall"]["parents_route"]["median_ms"] / res["wall"]["select_plan_with_policies"]["median_ms"], 2)
    res["stats"] = dev["stats"]
    full = on_device(per_candidate=True)
    same = lambda a, b: bool(np.array_equal(a, b, equal_nan=True))
    res["device_equals_parents_route"] = all(same(dev[k], ref[1][k]) for k in ("choice", "score", "n_admissible", "admissible", "u", "u0", "policy"))
    res["per_candidate_risk_equals_parents_route"] = all(same(full["risk"][k], ref[0][k]) for k in keys)
    res["choices"] = {str(q): int((dev["choice"] == q).sum()) for q in range(-1, P)}
    res["policy_chosen"] = int((dev["policy"] >= 0).sum())
    res["mean_score"] = float(np.nanmean(dev["score"])) if np.any(dev["choice"] >= 0) else None
    R.close(); p.close(); model.close()
    print(json.dumps(res))
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
