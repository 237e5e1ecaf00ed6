"""Plan selection on the device (GpuProblem.select_plan, mld_rollout_select; kernels k_rollout_cand_kpi, k_rollout_risk, k_plan_select) at the bench shard
(64 models x 512 scenarios = 32 768 instances), K = 25 steps under S = 20 realisations, P = 4 candidate input sequences, the microgrid KPIs and the risk
columns of scripts/gpu_rollout_risk_probe.py (its `switches` column, which an open-loop rollout does not have, replaced by the maximum of the cost KPI).

    python scripts/gpu_plan_select_probe.py [--out profiles/plan_select_probe.json] [--pairs 7]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python scripts/gpu_plan_select_probe.py --kernel-only
    python scripts/gpu_plan_select_probe.py --summarise DIR [--merge FILE.json]
    python scripts/gpu_plan_select_probe.py --bench PARENT_TREE [--merge FILE.json] [--pairs 3]

* default: wall time of select_plan(...) against the route the parent commit has for the same choice, P calls of rollout(u_seq=..., kpis=..., risk=...,
  per_trajectory=False) plus simlog.select_plan_np on the host, ALTERNATING in one session: one warm-up round, then --pairs timed rounds, the figure is the
  median.  Whether the two give the same bits, and the bytes each route moves.
* --kernel-only: for ONE kernel trace of its own on identical inputs -- three selections, three times the P per-candidate rollouts, then three
  device-to-device copies of the bytes k_plan_select reads and writes.
* --summarise: k_rollout_cand_kpi per trajectory-step against k_rollout_kpi run once per candidate (the standing margin of a rollout variant, 1.25 x), and
  k_plan_select against that copy x 1.25 (recorded, not gated: the project's convention for small kernels).
* --bench: bench.py --gpus 1 of this tree and of the parent commit's tree (built, at PARENT_TREE), alternating, each in a fresh process.

The scenario is scripts/gpu_rollout_risk_probe.py's: one realised series per instance, realisation c reads the load c steps later.  The candidates are
independent random binary sequences of duty cycle 0.4, the inputs of scripts/gpu_rollout_probe.py.  A few trajectories in a million are declined by the LDS
solver, and select_plan() as rollout() would finish them on the host, downloading every trajectory: the candidates that have one are REPLACED before anything
is timed (redraw_declined), so the inputs are changed and the host-completion route is never measured here; the count is recorded as `instances_redrawn`.
--unreplaced keeps the shard as drawn and passes complete="device" to every call of both routes instead; the default is what it was.
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

BATCH_MODELS, BATCH_SCEN, K, S, P = 64, 512, 25, 20, 4
MARGIN = 1.25
LEVELS = (0.05, 0.5, 0.95)
DUTY = 0.4


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
        if key in ("k_rollout_cand_kpi", "k_rollout_kpi", "k_rollout_risk", "k_plan_select", "copy_kernel"):
            seen.setdefault(key, []).append(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
    out = dict(kernels={k: dict(calls=len(v), average_ns=float(np.mean(v)), min_ns=float(min(v)), max_ns=float(max(v)), ns=v[-12:]) for k, v in sorted(seen.items())})
    cand, per = seen.get("k_rollout_cand_kpi", []), seen.get("k_rollout_kpi", [])
    if len(cand) >= 3 and len(per) >= 3 * P:      # the same trajectory-steps either way: one launch over batch P S, or P launches over batch S
        t_cand, t_per = float(np.mean(cand[-3:])), float(np.sum(per[-3 * P:])) / 3.0
        out["k_rollout_cand_kpi_against_k_rollout_kpi_per_candidate"] = dict(margin=MARGIN, cand_ns=t_cand, per_candidate_sum_ns=t_per, ratio=t_cand / t_per,
                                                                              hit=bool(t_cand <= MARGIN * t_per))
    copies = seen.get("copy_kernel", [])
    if len(copies) >= 3 and "k_plan_select" in seen:      # the three large ones are this script's
        y = float(np.mean(sorted(copies)[-3:]))
        t = float(np.mean(seen["k_plan_select"][-3:]))
        out["k_plan_select_yardstick"] = dict(margin=MARGIN, bytes=nbytes, copy_ns=y, kernel_ns=t, over_allowed=t / (y * MARGIN), hit=bool(t <= y * MARGIN), gated=False)
    else:
        out["yardstick"] = "the device-to-device copies did not show as kernels in this trace (%d copy kernels seen)" % len(copies)
    if "k_plan_select" in seen and cand:
        out["k_plan_select_share_of_the_rollout_kernel"] = float(np.mean(seen["k_plan_select"][-3:])) / float(np.mean(cand[-3:]))
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


def redraw_declined(p, R, cand, start, pstart, kpis, risk, rng, rounds=4):
    """The LDS solver declines a few trajectories in a million, and select_plan() as rollout() then finishes them on the host, which is not the route this probe
    measures: the C entry itself, asked for the counts alone, names the instances and the candidates, and those are replaced (by a copy of another candidate of the instance, which then ties with it).  Returns how many
    instances were touched, per round."""
    from pyhybridcontrol_amd import simlog, _lib
    B, nP = cand.shape[0], cand.shape[1]
    dp = _lib.dptr
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32)) if a is not None else None
    lp = lambda a: a.ctypes.data_as(C.POINTER(C.c_int64)) if a is not None else None
    karr, rarr = kpis.arrays(), risk.arrays()
    tabs = [None if karr[k] is None else np.ascontiguousarray(karr[k]) for k in simlog.KPI_TABLES]
    thr = None if karr["thresh"] is None else np.ascontiguousarray(karr["thresh"])
    redrawn = []
    for _ in range(rounds):
        counts, stats = np.zeros((B, nP, 4), np.int32), np.zeros(4, np.int64)
        rc = _lib.load().mld_rollout_select(
            p._h, R.problem._h, K, S, nP, 0, dp(cand), None, lp(start), 0, None, 0, len(kpis), *([dp(t) for t in tabs] + [ip(karr["price_chan"]), dp(thr), 1e-6, lp(pstart)]),
            len(risk), ip(rarr["col_src"]), ip(rarr["col_q"]), dp(rarr["level"]), len(risk.levels), dp(rarr["alpha"]), 0, 0, 0, 0, None, None, None, None, S,
            None, None, None, None, None, None, None, None, None, None, None, None, None, None, None, None, ip(counts),
            None, None, None, None, None, None, lp(stats), None, None, None, None, None, None, None, None)
        _lib.check(rc)
        bad = np.flatnonzero((counts[:, :, 2] > 0).any(axis=1))
        redrawn.append(int(bad.size))
        if not bad.size:
            return redrawn
        for b in bad:      # a declined candidate becomes a copy of one of the instance's that was not; drawn again where all were
            ok = np.flatnonzero(counts[b, :, 2] == 0)
            if ok.size:
                cand[b, counts[b, :, 2] > 0] = cand[b, ok[0]]
            else:
                cand[b] = (rng.uniform(size=cand.shape[1:]) < DUTY).astype(float)
    sys.exit("trajectories are still declined after %d redraws: %s" % (rounds, redrawn))


def bench_alternating(parent, pairs):
    """bench.py of the two trees, alternating, a fresh process each: the flagship workload launches none of the new code, so the two should agree"""
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
            rec["trace"] = s = summarise(sys.argv[sys.argv.index("--summarise") + 1], (rec.get("bytes") or {}).get("k_plan_select_reads_and_writes"))
        print(json.dumps(s, indent=1))
        if path:
            json.dump(rec, open(path, "w"), indent=1)
        return
    import bench
    from pyhybridcontrol_amd import gpu, host, simlog, _lib
    from pyhybridcontrol_amd.aux_resolve import BatchAuxResolver
    kernel_only = "--kernel-only" in sys.argv
    out_path = arg("--out", "")
    pairs = arg("--pairs", 7)
    agents, N_p, N_t, x0, om, midx = bench.make_shard(BATCH_MODELS, BATCH_SCEN, 0)
    d = agents[0]["dims"]
    B, nx, nw, nu = x0.shape[0], d["nx"], d["nomega"], d["nu"]
    mats = [a["mats"] for a in agents]
    model = gpu.GpuModel(mats, d)
    cost = host.stack_costs([host.cost_from_atoms(a["atoms"], d, N_p, N_t) for a in agents])
    p = gpu.GpuProblem(model, N_p, N_t, cost, gap_rel=1e-2, max_nodes=800, max_pivots=40000)
    R = BatchAuxResolver(mats, d, small_lds=True)
    kpis = simlog.KpiTable.microgrid(d, n_models=len(mats), price_chan=0)
    Q = len(kpis)
    risk = simlog.RiskTable(kpis, LEVELS)
    risk.add("cost", "kpi_sum", kpi="cost").add("p_imp", "kpi_sum", kpi="p_imp").add("p_exp", "kpi_sum", kpi="p_exp")
    risk.add("mu_over", "kpi_sum", kpi="mu_over", level=0.0).add("mu_under", "kpi_sum", kpi="mu_under", level=0.0)
    risk.add("peak_import", "kpi_max", kpi="p_imp").add("steps_over", "kpi_n_above", kpi="mu_over", level=0.0)
    risk.add("steps_under", "kpi_n_above", kpi="mu_under", level=0.0).add("cost_max", "kpi_max", kpi="cost").add("n_vio", "n_vio", level=0.0)
    risk.add("mu_total", "mu_total", level=0.0).add("worst_vio", "worst_vio", level=1e-6)
    # the tail of the cost, among the candidates whose comfort slack stays small on average and whose upper tail of it is bounded
    sel = simlog.PlanSelector(risk).minimise("cost", "cvar_hi", level=0.95).subject_to("steps_under", "mean", 0.5 * K).subject_to("mu_under", "cvar_hi", 1e4, level=0.95)
    G, L = len(risk), len(LEVELS)
    T = B * P * S
    seq = B * K * nu * 8
    n_stats = 1 + len(sel.constraints)
    sel_bytes = B * P * (n_stats * 8 + 4) + B * (4 + 8 + 4) + B * P + 2 * seq + B * nu * 8      # the objective's and the constraints' statistics and one count per candidate; the outputs; the sequence read and written; step 0
    per_call_down = B * (G * (3 * 8 + 3 * 4) + G * L * (3 * 8 + 4) + 16)
    res = dict(version=_lib.version(), batch=B, models=len(agents), dims={k: int(v) for k, v in d.items()}, N_tilde=N_t, K=K, S=S, P=P, duty=DUTY,
               kpis=list(kpis.names), columns=list(risk.names), levels=list(LEVELS), pairs=pairs,
               bytes=dict(k_plan_select_reads_and_writes=sel_bytes,
                          select_plan=dict(uploads=B * P * K * nu * 8 + B * S * 2 * 8, downloads=B * (4 + 8 + 4 + P + 4 * P * 4) + seq + B * nu * 8),
                          per_candidate_route=dict(uploads=P * (seq + B * S * 2 * 8), downloads=P * per_call_down),
                          omega_windows_gathered_per_rollout_call=B * S * K * nw * 8))
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
    cand = np.ascontiguousarray(np.stack([(rng.uniform(size=(B, K, nu)) < duty).astype(float) for duty in (DUTY,) * P], axis=1))
    p.upload(x0, om, midx)
    p.upload_profiles(lib, (nx, 1))
    p.upload_prices(plib, 1)
    unreplaced = "--unreplaced" in sys.argv      # the shard as drawn: declined trajectories are finished on the device (complete="device"), by both routes
    how = dict(complete="device") if unreplaced else {}
    if not unreplaced:
        res["instances_redrawn"] = redraw_declined(p, R, cand, start, pstart, kpis, risk, rng)
    per_cand = [np.ascontiguousarray(cand[:, q]) for q in range(P)]
    on_device = lambda **kw: p.select_plan(R, sel, candidates=cand, start=start, kpis=kpis, price_start=pstart, **dict(how, **kw))
    one = lambda q: p.rollout(R, u_seq=per_cand[q], start=start, kpis=kpis, price_start=pstart, risk=risk, per_trajectory=False, **how)
    if kernel_only:
        for _ in range(3):
            res["stats"] = on_device()["stats"]
        for _ in range(3):
            for q in range(P):
                one(q)
        d2d_copies(sel_bytes)
        print(json.dumps(res))
        R.close(); p.close(); model.close()
        return

    keys = simlog.RISK_COL_KEYS + simlog.RISK_LEVEL_KEYS + simlog.RISK_COUNTS

    def on_host():
        outs = [one(q) for q in range(P)]
        full = {k: np.stack([o["risk"][k] for o in outs], axis=1) for k in keys}
        return full, simlog.select_plan_np(full, sel, S, candidates=cand)

    wall = dict(select_plan_on_device=[], rollouts_per_candidate_plus_select_plan_np=[])
    dev = ref = None
    for r in range(pairs + 1):                                  # one warm-up round, then the timed rounds, alternating
        t = time.perf_counter(); dev = on_device(); ms_d = (time.perf_counter() - t) * 1e3
        t = time.perf_counter(); ref = on_host(); ms_h = (time.perf_counter() - t) * 1e3
        print("round %d: select_plan %.1f ms, %d x rollout(risk, per_trajectory=False) + select_plan_np %.1f ms" % (r, ms_d, P, ms_h), flush=True)
        if dev["stats"]["finished_on_host"] or (dev["stats"]["declined"] and not unreplaced):
            sys.exit("trajectories were declined and finished on the host (%s): not the route this probe measures" % (dev["stats"],))
        if r >= 1:
            wall["select_plan_on_device"].append(ms_d); wall["rollouts_per_candidate_plus_select_plan_np"].append(ms_h)
    res["wall"] = {n: stat(v) for n, v in wall.items()}
    res["per_candidate_route_over_select_plan"] = round(res["wall"]["rollouts_per_candidate_plus_select_plan_np"]["median_ms"] / res["wall"]["select_plan_on_device"]["median_ms"], 2)
    res["stats"] = dev["stats"]
    full = on_device(per_candidate=True)
    same = lambda a, b: bool(np.array_equal(a, b, equal_nan=True))
    res["device_equals_select_plan_np"] = all(same(dev[k], ref[1][k]) for k in ("choice", "score", "n_admissible", "admissible", "u", "u0"))
    res["per_candidate_risk_equals_rollout_risk"] = all(same(full["risk"][k], ref[0][k]) for k in keys)
    res["choices"] = {str(q): int((dev["choice"] == q).sum()) for q in range(-1, P)}
    res["mean_score"] = float(np.nanmean(dev["score"]))
    R.close(); p.close(); model.close()
    print(json.dumps(res))
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
