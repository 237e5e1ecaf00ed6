"""The resolving plant step with fallback inputs (GpuProblem.sim_step(resolve=R, fallback=...), kernels k_fallback_inputs / k_fallback_commit) at the bench
shard (64 models x 512 scenarios = 32 768 instances), thermostat on every channel as the second source.

    python scripts/gpu_fallback_probe.py [--out profiles/fallback_probe.json]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python scripts/gpu_fallback_probe.py --kernel-only
    python scripts/gpu_fallback_probe.py --summarise DIR [--merge FILE.json]

* default, every pair ALTERNATING in one session, one warm-up pair and seven timed pairs, median and range:
  (a) the wall time of an advancing, logging fallback step with the memory on and every plan usable against sim_step(resolve=R) -- each the SECOND step
      after an upload, so that neither pays for laying out the resolver's batch, the policy's reset state or the memory (--resolve-only times that step
      alone: run from a checkout of the parent with this file copied in, it gives the parent's own number);
  (b) the same step with 1 % of the instances cut off (set_cutoffs -1e30) one step after a step that filled the memory, against the host route: download(),
      fallback.choose_np / commit_np with the memory in numpy, sim_step(resolve=R, u0=u).  The solves in front of the steps are not timed.
* --kernel-only: for ONE kernel trace of its own -- three advancing, logging fallback steps and three device-to-device copies each of the bytes
  k_fallback_inputs and k_fallback_commit write.
* --summarise: each of the two kernels against its copy x 1.25 (recorded, not gated, like the copy kernels of the resolving step).
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

BATCH_MODELS, BATCH_SCEN = 64, 512
T_ON, T_OFF = 57.5, 60.5
MARGIN = 1.25
CUT_SHARE = 0.01


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
    keep = ("k_fallback_inputs", "k_fallback_commit", "k_policy_commit", "k_aux_inputs", "k_aux_merge", "k_small_milp", "k_sim_step")
    out = dict(kernels={k: dict(calls=len(v), average_ns=float(np.mean(v)), min_ns=float(min(v)), max_ns=float(max(v))) for k, v in sorted(seen.items()) if k in keep})
    copies = seen.get("copy_kernel", [])
    if len(copies) >= 6 and "k_fallback_inputs" in out["kernels"] and "k_fallback_commit" in out["kernels"]:      # the last six: three per kernel, inputs first
        for name, ys in (("k_fallback_inputs", copies[-6:-3]), ("k_fallback_commit", copies[-3:])):
            y = float(np.mean(ys))
            out[name + "_yardstick"] = dict(margin=MARGIN, bytes=(nbytes or {}).get(name), copy_ns=y, over_allowed=out["kernels"][name]["average_ns"] / (y * MARGIN), gated=False)
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


def main():
    if "--summarise" in sys.argv:
        rec, path = {}, None
        if "--merge" in sys.argv:
            path = sys.argv[sys.argv.index("--merge") + 1]
            rec = json.load(open(path)) if os.path.exists(path) else {}
        s = summarise(sys.argv[sys.argv.index("--summarise") + 1], rec.get("kernel_bytes"))
        print(json.dumps(s, indent=1))
        if path:
            rec["trace"] = s
            json.dump(rec, open(path, "w"), indent=1)
        return
    import bench
    from pyhybridcontrol_amd import gpu, host, policy, _lib
    from pyhybridcontrol_amd.aux_resolve import BatchAuxResolver
    kernel_only, resolve_only = "--kernel-only" in sys.argv, "--resolve-only" in sys.argv
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    agents, N_p, N_t, x0, om, midx = bench.make_shard(BATCH_MODELS, BATCH_SCEN, 0)
    d = agents[0]["dims"]
    B, nx, nu = x0.shape[0], d["nx"], d["nu"]
    res = dict(version=_lib.version(), batch=B, models=len(agents), dims={k: int(v) for k, v in d.items()}, N_tilde=N_t, cut_share=CUT_SHARE,
               kernel_bytes=dict(k_fallback_inputs=8 * B * nu + 5 * B, k_fallback_commit=8 * B * N_t * nu + 4 * B))
    mats = [a["mats"] for a in agents]
    model = gpu.GpuModel(mats, d)
    cost = host.stack_costs([host.cost_from_atoms(a["atoms"], d, N_p, N_t) for a in agents])
    p = gpu.GpuProblem(model, N_p, N_t, cost, gap_rel=1e-2, max_nodes=800, max_pivots=40000)
    R = BatchAuxResolver(mats, d, small_lds=True)
    nv = model.nv

    def fresh(log=2):
        p.upload(x0, om, midx)
        p.sim_log_begin(log)

    def timed(fn):
        t = time.perf_counter()
        out = fn()
        return (time.perf_counter() - t) * 1e3, out

    if resolve_only:
        ms = []
        for r in range(8):
            fresh()
            p.solve_resident()
            p.sim_step(resolve=R)
            p.solve_resident()
            t, _ = timed(lambda: p.sim_step(resolve=R))
            if r >= 1:
                ms.append(t)
        res["wall"] = dict(resolve_step=stat(ms))
        print(json.dumps(res))
        R.close(); p.close(); model.close()
        return
    from pyhybridcontrol_amd import fallback      # (not in a parent build: --resolve-only has returned)
    P = policy.ThresholdPolicy.thermostat(T_ON, T_OFF, len(mats), nx=nx)
    both = ("memory", "policy")
    fresh()
    p.upload_policy(P)
    p.plan_memory()
    if kernel_only:
        for _ in range(3):
            fresh()
            p.solve_resident()
            p.sim_step(resolve=R, fallback=both)
        for name in ("k_fallback_inputs", "k_fallback_commit"):
            d2d_copies(res["kernel_bytes"][name])
        print(json.dumps(res))
        R.close(); p.close(); model.close()
        return
    # (a) every plan usable
    wall = dict(fallback_step=[], resolve_step=[])
    for r in range(8):
        fresh()
        p.solve_resident()
        p.sim_step(resolve=R, fallback=both)
        p.solve_resident()
        t_f, n_f = timed(lambda: p.sim_step(resolve=R, fallback=both))
        fresh()
        p.solve_resident()
        p.sim_step(resolve=R)
        p.solve_resident()
        t_r, n_r = timed(lambda: p.sim_step(resolve=R))
        if r >= 1:
            wall["fallback_step"].append(t_f); wall["resolve_step"].append(t_r)
    res["all_usable"] = dict(wall={k: stat(v) for k, v in wall.items()}, skipped=dict(fallback_step=n_f, resolve_step=n_r))
    a = res["all_usable"]["wall"]
    res["all_usable"]["difference_ms"] = round(a["fallback_step"]["median_ms"] - a["resolve_step"]["median_ms"], 3)
    print("all usable:", res["all_usable"], flush=True)
    # (b) 1 % cut off, one step after a step that filled the memory
    rng = np.random.default_rng(31)
    chosen = rng.choice(B, max(1, int(CUT_SHARE * B)), replace=False)
    cut = np.full(B, np.inf)
    cut[chosen] = -1e30

    def plan_u(plan):
        return np.ascontiguousarray(plan["v"].reshape(B, N_t, nv)[:, :, :nu])

    def host_step(state, cutoffs):
        """one step by the route the library had; the solve is not timed"""
        if cutoffs is not None:
            p.set_cutoffs(cutoffs)
        p.solve_resident()
        t = time.perf_counter()
        plan = p.download()
        usable = np.isin(plan["status"], (0, 2)) & np.isfinite(plan["obj"])
        x = p.inputs()[0]
        u, src = fallback.choose_np(usable, plan["v"][:, :nu], state["mem"], state["age"], both, P=P, midx=midx, x=x, u_prev=state["up"])
        o = p.sim_step(resolve=R, u0=u, outputs=True)
        state["mem"], state["age"] = fallback.commit_np(src, plan_u(plan), state["mem"], state["age"], N_t)
        adv = o["aux_status"] == 0
        state["up"] = np.where(adv[:, None], u, state["up"])
        return (time.perf_counter() - t) * 1e3, src

    def device_step(cutoffs):
        if cutoffs is not None:
            p.set_cutoffs(cutoffs)
        p.solve_resident()
        t, o = timed(lambda: p.sim_step(resolve=R, fallback=both, outputs=True))
        return t, o["u_source"]

    wall = dict(fallback_step=[], host_route=[])
    src_d = src_h = None
    for r in range(8):
        fresh()
        device_step(None)
        t_d, src_d = device_step(cut)
        fresh()
        state = dict(mem=np.zeros((B, N_t, nu)), age=np.full(B, -1, np.int32), up=P.initial_state(midx))
        host_step(state, None)
        t_h, src_h = host_step(state, cut)
        if r >= 1:
            wall["fallback_step"].append(t_d); wall["host_route"].append(t_h)
    res["cut_off"] = dict(wall={k: stat(v) for k, v in wall.items()}, instances_cut=int(chosen.size),
                          sources_device={str(k): int((src_d == k).sum()) for k in (-1, 0, 1, 2)}, sources_equal=bool(np.array_equal(src_d, src_h)))
    b = res["cut_off"]["wall"]
    res["cut_off"]["ratio"] = round(b["host_route"]["median_ms"] / b["fallback_step"]["median_ms"], 2)
    print("cut off:", res["cut_off"], flush=True)
    R.close(); p.close(); model.close()
    print(json.dumps(res))
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
