"""The resolving plant step that applies a kept selection (GpuProblem.sim_step(resolve=R, selected=True), kernels k_selected_inputs / k_selected_commit) and
the kept copy of a select call (select_plan_policies(keep=True)) at the bench shard (64 models x 512 scenarios = 32 768 instances); P = 3 candidates -- the
plan first, one random binary sequence of duty 0.4, the thermostat 57.5 / 60.5 --, K = N_tilde, S = 2 realisations of the forecast with its load channel moved.

    python scripts/gpu_selected_step_probe.py [--out profiles/selected_step_probe.json]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python scripts/gpu_selected_step_probe.py --kernel-only
    python scripts/gpu_selected_step_probe.py --summarise DIR [--merge FILE.json]
    python scripts/gpu_selected_step_probe.py --bench PARENT_TREE [--merge FILE.json]

* default, the routes ALTERNATING in one session, one warm-up round and seven timed rounds, median and range:
  (1) an advancing, logging sim_step(resolve=R, selected=True, fallback=("memory", "policy")) against today's route -- the NaN rows of the select call's u0
      patched on the host, sim_step(resolve=R, u0=...) -- and against sim_step(resolve=R, fallback=...), the parent's entry point in the same session: the
      same step with the plan as first source.  Every step is the SECOND after an upload (none pays for laying out the resolver's batch, the policy's reset
      state or the memory), on the same inputs; the selection is put back with set_selection() before every selected step, outside the timing.
  (3) select_plan_policies(keep=True) against keep=False on the same inputs.
* --kernel-only: for ONE kernel trace of its own -- three selected steps and three device-to-device copies each of the bytes k_selected_inputs and
  k_selected_commit write.  --summarise: (2) each of the two kernels against its copy x 1.25 (recorded, not gated, as for k_fallback_*).
* --bench: (4) bench.py --gpus 1 --steps 20 --warmup 3 of this tree alternating with the one at PARENT_TREE, a fresh process each, four pairs.
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

BATCH_MODELS, BATCH_SCEN = 64, 512
T_ON, T_OFF = 57.5, 60.5
MARGIN = 1.25
S = 2
BOTH = ("memory", "policy")


def stat(ms):
    return dict(median_ms=round(float(np.median(ms)), 3), min_ms=round(min(ms), 3), max_ms=round(max(ms), 3), ms=[round(v, 3) for v in ms])


def summarise(d, nbytes):
    seen, rows = {}, []
    for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        rows += list(csv.DictReader(open(f)))
    for r in sorted(rows, key=lambda r: int(r["Start_Timestamp"])):
        name = r["Kernel_Name"].split("(")[0]
        key = "copy_kernel" if "copyBuffer" in name else name
        if name.startswith("k_") or key == "copy_kernel":
            seen.setdefault(key, []).append(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
    keep = ("k_selected_inputs", "k_selected_commit", "k_selection_policy", "k_policy_commit", "k_aux_inputs", "k_aux_merge", "k_small_milp", "k_sim_step")
    out = dict(kernels={k: dict(calls=len(v), average_ns=float(np.mean(v)), min_ns=float(min(v)), max_ns=float(max(v))) for k, v in sorted(seen.items()) if k in keep})
    copies = seen.get("copy_kernel", [])
    if len(copies) >= 6 and "k_selected_inputs" in out["kernels"] and "k_selected_commit" in out["kernels"]:      # the last six: three per kernel, inputs first
        for name, ys in (("k_selected_inputs", copies[-6:-3]), ("k_selected_commit", copies[-3:])):
            y = float(np.mean(ys))
            over = out["kernels"][name]["average_ns"] / (y * MARGIN)
            out[name + "_yardstick"] = dict(margin=MARGIN, bytes=(nbytes or {}).get(name), copy_ns=y, over_allowed=over, met=bool(over <= 1.0), gated=False)
    else:
        out["yardstick"] = "the device-to-device copies did not show as kernels in this trace (%d copy kernels seen)" % len(copies)
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


def merge(path, key, value):
    rec = json.load(open(path)) if path and os.path.exists(path) else {}
    rec[key] = value
    if path:
        json.dump(rec, open(path, "w"), indent=1)


def bench_pairs(parent, pairs=4):
    """bench.py of this tree and of the parent's, alternating, a fresh process each"""
    vals = dict(this=[], parent=[])
    for _ in range(pairs):
        for name, tree in (("this", ROOT), ("parent", parent)):
            out = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "20", "--warmup", "3"], cwd=tree, stdout=subprocess.PIPE, universal_newlines=True,
                                 timeout=400, check=True).stdout
            line = [l for l in out.splitlines() if l.startswith("{")][-1]
            vals[name].append(float(json.loads(line)["value"]))
            print(name, vals[name][-1], flush=True)
    lo, hi = (min(vals["this"]), max(vals["this"])), (min(vals["parent"]), max(vals["parent"]))
    return dict(command="bench.py --gpus 1 --steps 20 --warmup 3", unit="agent-solves/s", this=vals["this"], parent=vals["parent"],
                ranges_overlap=bool(lo[0] <= hi[1] and hi[0] <= lo[1]))


def main():
    path = sys.argv[sys.argv.index("--merge") + 1] if "--merge" in sys.argv else None
    if "--summarise" in sys.argv:
        rec = json.load(open(path)) if path and os.path.exists(path) else {}
        s = summarise(sys.argv[sys.argv.index("--summarise") + 1], rec.get("kernel_bytes"))
        print(json.dumps(s, indent=1))
        merge(path, "trace", s)
        return
    if "--bench" in sys.argv:
        b = bench_pairs(os.path.abspath(sys.argv[sys.argv.index("--bench") + 1]))
        print(json.dumps(b, indent=1))
        merge(path, "flagship", b)
        return
    import bench
    from pyhybridcontrol_amd import gpu, host, policy, simlog, _lib
    from pyhybridcontrol_amd.aux_resolve import BatchAuxResolver
    kernel_only = "--kernel-only" in sys.argv
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    agents, N_p, N_t, x0, om, midx = bench.make_shard(BATCH_MODELS, BATCH_SCEN, 0)
    d = agents[0]["dims"]
    B, nx, nu, nw = x0.shape[0], d["nx"], d["nu"], d["nomega"]
    res = dict(version=_lib.version(), batch=B, models=len(agents), dims={k: int(v) for k, v in d.items()}, N_tilde=N_t, K=N_t, S=S, P=3,
               kernel_bytes=dict(k_selected_inputs=8 * B * nu + 9 * B, k_selected_commit=8 * B * N_t * nu + 4 * B))
    mats = [a["mats"] for a in agents]
    model = gpu.GpuModel(mats, d)
    cost = host.stack_costs([host.cost_from_atoms(a["atoms"], d, N_p, N_t) for a in agents])
    p = gpu.GpuProblem(model, N_p, N_t, cost, gap_rel=1e-2, max_nodes=800, max_pivots=40000)
    R = BatchAuxResolver(mats, d, small_lds=True)
    P = policy.ThresholdPolicy.thermostat(T_ON, T_OFF, len(mats), nx=nx)
    rng = np.random.default_rng(41)
    om_seq = np.repeat(om.reshape(B, 1, N_t, nw), S, axis=1).copy()
    if nx < nw:
        om_seq[:, :, :, nx] += rng.normal(0.0, 800.0, (B, S, N_t))
    cand = (rng.uniform(size=(B, 1, N_t, nu)) < 0.4).astype(float)
    cw = rng.uniform(0.5, 2.0, size=(N_t, model.nv))
    risk = simlog.RiskTable(None, (0.5,)).add("cost", "cost", level=0.0).add("vio", "worst_vio", level=1e-6)

    def fresh(log=2):
        p.upload(x0, om, midx)
        p.sim_log_begin(log)

    def timed(fn):
        t = time.perf_counter()
        out = fn()
        return (time.perf_counter() - t) * 1e3, out

    def select(sel, **kw):
        return p.select_plan_policies(R, sel, policies=[P], candidates=cand, plan_first=True, K=N_t, omega_seq=om_seq, cost_w=cw, complete="device", **kw)

    fresh()
    p.upload_policy(P)
    p.plan_memory()
    p.solve_resident()
    probe = select(simlog.PlanSelector(risk).minimise("cost", "mean"), per_candidate=True)
    worst = np.where(probe["admissible"], probe["risk"]["max"][:, :, 0], np.inf).min(axis=1)
    sel = simlog.PlanSelector(risk).minimise("cost", "mean").subject_to("cost", "max", float(np.quantile(worst[np.isfinite(worst)], 0.9)))      # about a tenth end without a choice
    first = select(sel, keep=True)
    kept = p.selection()
    res["selection"] = dict(no_choice=int((kept["choice"] < 0).sum()), plan=int((kept["choice"] == 0).sum()), sequence=int((kept["choice"] == 1).sum()),
                            policy=int((kept["policy"] >= 0).sum()), stats=first["stats"])
    u0_patched = np.where(np.isnan(first["u0"]), 0.0, first["u0"])

    def second_step(step_fn, before=None):
        """the timed step: the second after an upload, on the same inputs"""
        fresh()
        p.solve_resident()
        p.sim_step(resolve=R, fallback=BOTH)
        p.solve_resident()
        if before:
            before()
        return timed(step_fn)

    put_back = lambda: p.set_selection(kept["choice"], kept["u"], policy=kept["policy"])
    if kernel_only:
        for _ in range(3):
            second_step(lambda: p.sim_step(resolve=R, selected=True, fallback=BOTH), put_back)
        for name in ("k_selected_inputs", "k_selected_commit"):
            d2d_copies(res["kernel_bytes"][name])
        print(json.dumps(res))
        R.close(); p.close(); model.close()
        return
    # (1) the step
    wall = dict(selected_step=[], host_route=[], fallback_step=[])
    src = None
    for r in range(8):
        t_s, o = second_step(lambda: p.sim_step(resolve=R, selected=True, fallback=BOTH, outputs=True), put_back)
        src = o["u_source"]
        t_h, _ = second_step(lambda: p.sim_step(resolve=R, u0=np.where(np.isnan(first["u0"]), 0.0, first["u0"]), outputs=True))
        t_f, _ = second_step(lambda: p.sim_step(resolve=R, fallback=BOTH, outputs=True))
        if r >= 1:
            wall["selected_step"].append(t_s); wall["host_route"].append(t_h); wall["fallback_step"].append(t_f)
    w = {k: stat(v) for k, v in wall.items()}
    res["step"] = dict(wall=w, sources={str(k): int((src == k).sum()) for k in (-1, 1, 2, 3)},
                       host_route_over_selected=round(w["host_route"]["median_ms"] / w["selected_step"]["median_ms"], 3),
                       selected_minus_fallback_ms=round(w["selected_step"]["median_ms"] - w["fallback_step"]["median_ms"], 3))
    print("step:", res["step"], flush=True)
    # (3) the kept copy
    wall = dict(keep=[], no_keep=[])
    fresh()
    p.solve_resident()
    same = True
    for r in range(8):
        t_k, a = timed(lambda: select(sel, keep=True))
        t_n, b = timed(lambda: select(sel))
        same = same and all(np.array_equal(a[k], b[k], equal_nan=True) for k in ("choice", "policy", "u", "u0", "score"))
        if r >= 1:
            wall["keep"].append(t_k); wall["no_keep"].append(t_n)
    w = {k: stat(v) for k, v in wall.items()}
    res["kept_copy"] = dict(wall=w, same_results=bool(same), keep_minus_no_keep_ms=round(w["keep"]["median_ms"] - w["no_keep"]["median_ms"], 3),
                            bytes_copied=8 * B * N_t * nu + 8 * B)
    print("kept copy:", res["kept_copy"], flush=True)
    R.close(); p.close(); model.close()
    print(json.dumps(res))
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        rec = json.load(open(out_path)) if os.path.exists(out_path) else {}
        rec.update(res)
        with open(out_path, "w") as f:
            json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
