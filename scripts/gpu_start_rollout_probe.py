"""The MIP start from a baseline rollout on the device (GpuProblem.warm_start_from_rollout, kernels k_rollout_policy and k_warm_from_rollout) at the bench
shard (64 models x 512 scenarios = 32 768 instances, N_tilde = 25), thermostat on every channel.

    python scripts/gpu_start_rollout_probe.py [--out profiles/start_rollout_probe.json] [--unreplaced]      # --unreplaced: complete="device" in every call

Medians of seven runs behind one warm-up, the routes ALTERNATING in one session:
* entry_vs_kernel_work: the entry against rollout(policy=True, K=N_tilde, omega_seq=forecast) with summaries only -- the same kernel work plus an upload of
  the forecast.  That call's time is the yardstick; the entry may take 25 % more.  Recorded whether met or missed.
* entry_vs_host_route: against the route the library had -- rollout(trajectories=True), simlog.start_from_rollout_np, set_warm_start.
* solve: the solve with and without the start (three alternating pairs each), on the first step after an upload with a start for all, and on a step where
  1 % of the instances were cut off (unbeatable cutoff, advancing fallback step, warm_start_from_previous(1); then keep=True fills the cut instances):
  solve_ms, the proven share, instances without a plan, the worst obj / baseline, nodes.  k_solve is the parent's, so the solve without the start is the
  parent's solve.
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BATCH_MODELS, BATCH_SCEN = 64, 512
T_ON, T_OFF = 57.5, 60.5
MARGIN = 1.25
CUT = -1e30


def stat(ms):
    return dict(median_ms=round(float(np.median(ms)), 3), min_ms=round(min(ms), 3), max_ms=round(max(ms), 3), ms=[round(v, 3) for v in ms])


def timed(fn):
    t = time.perf_counter()
    out = fn()
    return out, (time.perf_counter() - t) * 1e3


def main():
    import bench
    from pyhybridcontrol_amd import gpu, host, policy, simlog, _lib
    from pyhybridcontrol_amd.aux_resolve import BatchAuxResolver
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    agents, N_p, N_t, x0, om, midx = bench.make_shard(BATCH_MODELS, BATCH_SCEN, 0)
    d = agents[0]["dims"]
    B, nx, nw = x0.shape[0], d["nx"], d["nomega"]
    mats = [a["mats"] for a in agents]
    model = gpu.GpuModel(mats, d)
    cost = host.stack_costs([host.cost_from_atoms(a["atoms"], d, N_p, N_t) for a in agents])
    p = gpu.GpuProblem(model, N_p, N_t, cost, gap_rel=1e-2, max_nodes=800, max_pivots=40000)
    R = BatchAuxResolver(mats, d, small_lds=True)
    P = policy.ThresholdPolicy.thermostat(T_ON, T_OFF, len(mats), nx=nx)
    bins = np.flatnonzero(p.is_bin)
    res = dict(version=_lib.version(), batch=B, models=len(agents), dims={k: int(v) for k, v in d.items()}, N_tilde=N_t, n_bin=int(p.n_bin), T_on=T_ON, T_off=T_OFF,
               bytes=dict(v_down=8 * B * N_t * model.nv, start_up=B * int(p.n_bin), forecast_up=8 * B * N_t * nw))
    p.upload(x0, om, midx)
    p.upload_policy(P)
    forecast = np.ascontiguousarray(p.inputs()[1].reshape(B, 1, N_t, nw))

    unreplaced = "--unreplaced" in sys.argv      # declined trajectories are finished on the device (complete="device") by the entry and by both yardsticks
    how = dict(complete="device") if unreplaced else {}

    def host_route():
        ro = p.rollout(R, omega_seq=forecast, policy=True, trajectories=True, **how)
        start, source = simlog.start_from_rollout_np(ro["v"], ro["end_status"], bins)
        p.set_warm_start(start)
        return start, source, ro

    wall = dict(entry=[], rollout_summaries=[], host_route=[])
    for r in range(8):                                           # one warm-up round, seven timed rounds, alternating
        got, ms_e = timed(lambda: p.warm_start_from_rollout(R, policy=True, **how))
        dev_start = p.debug_warm_start()
        lean, ms_r = timed(lambda: p.rollout(R, omega_seq=forecast, policy=True, **how))
        (start, source, ro), ms_h = timed(host_route)
        if r >= 1:
            wall["entry"].append(ms_e); wall["rollout_summaries"].append(ms_r); wall["host_route"].append(ms_h)
    res["wall"] = {n: stat(v) for n, v in wall.items()}
    e, y, h = (res["wall"][n]["median_ms"] for n in ("entry", "rollout_summaries", "host_route"))
    res["entry_vs_kernel_work"] = dict(entry_ms=e, yardstick_ms=y, ratio=round(e / y, 3), allowed=MARGIN, met=bool(e <= MARGIN * y))
    res["entry_vs_host_route"] = dict(entry_ms=e, host_route_ms=h, ratio=round(h / e, 2))
    res["stats"] = dict(entry=got["stats"], rollout=lean["stats"])
    # the host route finishes on the host what the LDS solver declined; the entry has no host completion and leaves such a row without a start
    dec = got["source"] == -2
    res["bytes_equal_host_route"] = dict(declined_on_device=int(dec.sum()), rows_255_there=bool(np.all(dev_start[dec] == 255)),
                                         other_rows_and_sources_equal=bool(np.array_equal(dev_start[~dec], start[~dec]) and np.array_equal(got["source"][~dec], source[~dec])))
    print("wall:", res["wall"], res["entry_vs_kernel_work"], res["entry_vs_host_route"], res["stats"], res["bytes_equal_host_route"], flush=True)

    def solve_record(base_obj, sel=None):
        st = p.solve_resident()
        out = p.download()
        usable = np.isin(out["status"], (0, 2)) & np.isfinite(out["obj"])
        ratio = np.where(usable, out["obj"] / base_obj, np.nan)
        rec = dict(solve_ms=round(float(st["solve_ms"]), 3), proven_share=float((out["status"] == 0).mean()), without_plan=int((~usable).sum()),
                   worst_obj_over_baseline=float(np.nanmax(ratio)), above_baseline=int((out["obj"][usable] > base_obj[usable] * (1 + 1e-6)).sum()), nodes=int(out["nodes"].sum()))
        if sel is not None:
            rec["cut_instances"] = dict(n=int(sel.sum()), proven_share=float((out["status"][sel] == 0).mean()), without_plan=int((~usable[sel]).sum()),
                                        worst_obj_over_baseline=float(np.nanmax(ratio[sel])) if usable[sel].any() else None, nodes=int(out["nodes"][sel].sum()))
        return rec

    # ---- the first step after an upload: a start for all against none
    base = p.evaluate(ro["v"].reshape(B, -1))
    res["baseline"] = dict(constr_vio_max=float(base["constr_vio"].max()), int_vio_max=float(base["int_vio"].max()), bound_vio_max=float(base["bound_vio"].max()),
                           obj_min=float(base["obj"].min()), obj_max=float(base["obj"].max()),
                           instances_above_1e_9=int((base["constr_vio"] > 1e-9).sum()), instances_above_1e_6=int((base["constr_vio"] > 1e-6).sum()),
                           rows_of_the_worst=np.bincount(base["constr_row"][base["constr_vio"] > 1e-6] % d["nc"], minlength=d["nc"]).tolist())
    del ro
    first = dict(with_start=[], without_start=[])
    for r in range(3):
        p.upload(x0, om, midx)
        p.warm_start_from_rollout(R, policy=True)
        first["with_start"].append(solve_record(base["obj"]))
        p.upload(x0, om, midx)
        first["without_start"].append(solve_record(base["obj"]))
    res["first_step"] = first
    print("first step:", first, flush=True)

    # ---- a step where 1 % of the instances were cut off
    chosen = np.zeros(B, bool)
    chosen[::100] = True
    cut = np.where(chosen, CUT, np.inf)

    def to_second_step():
        p.upload(x0, om, midx)
        p.set_cutoffs(cut)
        p.solve_resident()
        step = p.sim_step(resolve=R, fallback=("policy",), outputs=True)
        p.warm_start_from_previous(1)
        return step

    second = dict(with_start=[], without_start=[])
    for r in range(3):
        step = to_second_step()
        fc = np.ascontiguousarray(p.inputs()[1].reshape(B, 1, N_t, nw))
        b2 = p.evaluate(p.rollout(R, omega_seq=fc, policy=True, trajectories=True)["v"].reshape(B, -1))
        got, ms = timed(lambda: p.warm_start_from_rollout(R, policy=True, keep=True))
        rec = solve_record(b2["obj"], chosen)
        rec.update(entry_ms=round(ms, 3), entry_stats=got["stats"])
        second["with_start"].append(rec)
        to_second_step()
        second["without_start"].append(solve_record(b2["obj"], chosen))
    res["cut_step"] = dict(second, cut_instances=int(chosen.sum()), u_source_counts={str(k): int((step["u_source"] == k).sum()) for k in (-1, 0, 1, 2)})
    print("cut step:", res["cut_step"], flush=True)
    R.close(); p.close(); model.close()
    print(json.dumps(res))
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
