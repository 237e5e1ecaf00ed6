"""The rule-based feedback policy on the device (GpuProblem.rollout(policy=True), kernel k_rollout_policy; sim_step(resolve=R, policy=True), kernel
k_policy_inputs) at the bench shard (64 models x 512 scenarios = 32 768 instances), K = 25 steps under S = 20 realisations, thermostat on every channel.

    python scripts/gpu_policy_probe.py [--out profiles/policy_probe.json]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python scripts/gpu_policy_probe.py --kernel-only
    python scripts/gpu_policy_probe.py --summarise DIR [--merge FILE.json]

* default: rollout(policy=True) with summaries only against the only route the library had for a rule -- per realisation, K x (download x, policy.apply_np
  on the host, advancing sim_step(resolve=R, u0=...)) --, ALTERNATING in one session, one warm-up pair and seven timed pairs: median and range of both wall
  times and the ratio per realisation; the counts (complete / infeasible / declined); the worst deviation on a 256-instance sample.
* --kernel-only: for ONE kernel trace of its own -- two policy rollouts, two open-loop rollouts whose u_seq is set to the inputs the policy produced (both
  kernels then solve the same auxiliary problems), three what-if policy steps (k_policy_inputs) and three device-to-device copies of the bytes it writes.
* --summarise: k_rollout_policy per trajectory-step against k_rollout (allowed: 1.25 x), k_policy_inputs against the copy x 1.25 (recorded, not gated).

The realisations of an instance are windows of ONE realised series per instance (scripts/gpu_rollout_probe.py), here in two channel groups: the draws are
read from the series' start, the load c steps later.
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

BATCH_MODELS, BATCH_SCEN, K, S = 64, 512, 25, 20
T_ON, T_OFF = 57.5, 60.5
MARGIN = 1.25


def stat(ms):
    return dict(median_ms=round(float(np.median(ms)), 3), min_ms=round(min(ms), 3), max_ms=round(max(ms), 3), ms=[round(v, 3) for v in ms])


def summarise(d, nbytes=None):
    seen, rows = {}, []
    for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        rows += list(csv.DictReader(open(f)))
    for r in sorted(rows, key=lambda r: int(r["Start_Timestamp"])):
        name = r["Kernel_Name"].split("(")[0]
        key = "copy_kernel" if "copyBuffer" in name else name
        if name.startswith("k_") or key == "copy_kernel":
            seen.setdefault(key, []).append(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
    keep = ("k_rollout_policy", "k_rollout", "k_policy_inputs", "k_policy_commit", "k_aux_inputs", "k_aux_merge", "k_small_milp", "k_sim_step")
    out = dict(kernels={k: dict(calls=len(v), average_ns=float(np.mean(v)), min_ns=float(min(v)), max_ns=float(max(v))) for k, v in sorted(seen.items()) if k in keep})
    ks = out["kernels"]
    if len(seen.get("k_rollout_policy", [])) >= 2 and len(seen.get("k_rollout", [])) >= 2:      # the last two launches of each are the full-size ones
        n = BATCH_MODELS * BATCH_SCEN * S * K
        a, b = float(np.mean(seen["k_rollout_policy"][-2:])) / n, float(np.mean(seen["k_rollout"][-2:])) / n
        out["per_trajectory_step_ns"] = dict(k_rollout_policy=a, k_rollout=b, ratio=a / b, allowed=MARGIN, hit=bool(a / b <= MARGIN))
    copies = seen.get("copy_kernel", [])
    if len(copies) >= 3 and "k_policy_inputs" in ks:      # the last three are the yardstick
        y = float(np.mean(copies[-3:]))
        out["k_policy_inputs_yardstick"] = dict(margin=MARGIN, bytes=nbytes, copy_ns=y, over_allowed=ks["k_policy_inputs"]["average_ns"] / (y * MARGIN), gated=False)
    else:
        out["k_policy_inputs_yardstick"] = "the device-to-device copies did not show as kernels in this trace (%d copy kernels seen)" % len(copies)
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
        s = summarise(sys.argv[sys.argv.index("--summarise") + 1], rec.get("k_policy_inputs_bytes"))
        print(json.dumps(s, indent=1))
        if path:
            rec["trace"] = s
            json.dump(rec, open(path, "w"), indent=1)
        return
    import bench
    from pyhybridcontrol_amd import gpu, host, policy, _lib
    from pyhybridcontrol_amd.aux_resolve import BatchAuxResolver
    kernel_only = "--kernel-only" in sys.argv
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    agents, N_p, N_t, x0, om, midx = bench.make_shard(BATCH_MODELS, BATCH_SCEN, 0)
    d = agents[0]["dims"]
    B, nx, nu, nw = x0.shape[0], d["nx"], d["nu"], d["nomega"]
    res = dict(version=_lib.version(), batch=B, models=len(agents), dims={k: int(v) for k, v in d.items()}, N_tilde=N_t, K=K, S=S, T_on=T_ON, T_off=T_OFF,
               k_policy_inputs_bytes=8 * B * nu)
    mats = [a["mats"] for a in agents]
    model = gpu.GpuModel(mats, d)
    cost = host.stack_costs([host.cost_from_atoms(a["atoms"], d, N_p, N_t) for a in agents])
    p = gpu.GpuProblem(model, N_p, N_t, cost, gap_rel=1e-2, max_nodes=800, max_pivots=40000)
    R = BatchAuxResolver(mats, d, small_lds=True)
    P = policy.ThresholdPolicy.thermostat(T_ON, T_OFF, len(mats), nx=nx)
    # ONE realised series per instance in two channel groups, the draws (width nx) and the load (width 1): realisation c reads the draws from the series' start
    # and the load c steps later, so the realisations differ in the load alone -- the tanks, and with them the thermostat's inputs, are the instance's, and an
    # open-loop rollout can be given exactly the inputs the policy produces
    assert nw == nx + 1
    rng = np.random.default_rng(21)
    T = K + S
    series = np.tile(om.reshape(B, N_t, nw), (1, T // N_t + 1, 1))[:, :T].copy()
    series[:, :, nx] += rng.normal(0.0, 800.0, (B, T))
    lib = np.concatenate([series[:, :, :nx].reshape(B, T * nx), series[:, :, nx].reshape(B, T)], axis=1).ravel()
    base = np.arange(B, dtype=np.int64) * T * nw
    start = np.stack([np.broadcast_to(base[:, None], (B, S)), base[:, None] + T * nx + np.arange(S, dtype=np.int64)[None, :]], axis=2)      # (B, S, 2)
    start = np.ascontiguousarray(start)
    p.upload(x0, om, midx)
    p.upload_profiles(lib, (nx, 1))
    p.upload_policy(P)
    if kernel_only:
        # the inputs the policy produced: realisation 0's of every instance; on a 256-instance sample, whether the other realisations' are the same
        n = 256
        p.upload(x0[:n], om[:n], midx[:n])
        few = p.rollout(R, K=K, start=start[:n], policy=True, trajectories=True)
        done = few["end_status"] == 0
        same = [np.array_equal(few["v"][b, c, :, :nu], few["v"][b, 0, :, :nu]) for b in range(n) for c in range(S) if done[b, c] and done[b, 0]]
        res["policy_inputs_equal_across_realisations"] = dict(instances=n, share=float(np.mean(same)))
        p.upload(x0, om, midx)
        one = p.rollout(R, K=K, start=np.ascontiguousarray(start[:, :1]), policy=True, trajectories=True)
        u_pol = np.ascontiguousarray(one["v"][:, 0, :, :nu])
        u_pol = np.where(np.isfinite(u_pol), u_pol, 0.0)
        del few, one
        for _ in range(2):
            out = p.rollout(R, K=K, start=start, policy=True)
        for _ in range(2):
            open_loop = p.rollout(R, u_seq=u_pol, start=start)
        for _ in range(3):
            p.sim_step(resolve=R, policy=True, act_start=np.ascontiguousarray(start[:, 0]), step=0, advance=False, log=False)
        d2d_copies(res["k_policy_inputs_bytes"])
        res["stats"] = dict(policy=out["stats"], open_loop=open_loop["stats"])
        print(json.dumps(res))
        R.close(); p.close(); model.close()
        return

    def host_loop(n=B, c=0, outputs=False):
        """ONE realisation by the route the library had: K x (download x, apply_np on the host, advancing resolving step with u0)"""
        a0 = np.ascontiguousarray(start[:n, c])
        up, outs = P.initial_state(midx[:n]), []
        for k in range(K):
            x = p.inputs()[0]
            u = policy.apply_np(P, midx[:n], x, up)
            outs.append((u, p.sim_step(resolve=R, u0=u, act_start=a0 if k == 0 else None, step=k, actual=True, advance=True, log=False, outputs=outputs)))
            up = u
        return outs

    wall = dict(rollout_policy=[], host_loop=[])
    stats = None
    for r in range(8):                                           # one warm-up pair, seven timed pairs, alternating
        p.upload(x0, om, midx)
        t = time.perf_counter(); out = p.rollout(R, K=K, start=start, policy=True); ms_r = (time.perf_counter() - t) * 1e3
        stats = out["stats"]
        t = time.perf_counter(); host_loop(); ms_s = (time.perf_counter() - t) * 1e3
        if r >= 1:
            wall["rollout_policy"].append(ms_r); wall["host_loop"].append(ms_s)
    res["wall"] = {n: stat(v) for n, v in wall.items()}
    mr, msw = res["wall"]["rollout_policy"]["median_ms"], res["wall"]["host_loop"]["median_ms"]
    res["per_realisation"] = dict(rollout_policy_ms=round(mr / S, 3), host_loop_ms=msw, ratio=round(msw / (mr / S), 2))
    res["stats"] = stats
    res["end_status_counts"] = {str(k): int((out["end_status"] == k).sum()) for k in (-1, 0, 1, 2)}
    res["switches"] = dict(mean=float(out["switches"][out["end_status"] == 0].mean()), max=int(out["switches"].max()))
    print("wall:", res["wall"], res["per_realisation"], stats, flush=True)
    # the worst deviation from the host loop on a 256-instance sample, every realisation
    n = 256
    p.upload(x0[:n], om[:n], midx[:n])
    got = p.rollout(R, K=K, start=start[:n], policy=True, trajectories=True)
    worst, equal, margin = 0.0, True, np.inf
    for c in range(S):
        p.upload(x0[:n], om[:n], midx[:n])
        steps = host_loop(n, c, outputs=True)
        for k, (u, o) in enumerate(steps):
            ok = got["steps_done"][:, c] > k
            s = policy.selector_values(P, midx[:n], got["x"][ok, c, k])
            if s.size:
                margin = min(margin, float(np.minimum(np.abs(s - T_ON), np.abs(s - T_OFF)).min()))
            equal = equal and bool(np.array_equal(ok, o["aux_status"] == 0)) and bool(np.array_equal(got["v"][ok, c, k, :nu + 1], o["v0"][ok, :nu + 1]))
            for a, b in ((got["x"][ok, c, k + 1], o["x_k1"][ok]), (got["v"][ok, c, k], o["v0"][ok]), (got["cons_vio"][ok, c, k], o["cons_vio"][ok])):
                if a.size:
                    worst = max(worst, float((np.abs(a - b) / np.maximum(1.0, np.abs(b))).max()))
    res["sample"] = dict(instances=n, realisations=S, steps=K, inputs_binaries_and_endings_equal=equal, worst_deviation=worst, selector_margin=margin, stats=got["stats"])
    print("sample:", res["sample"], flush=True)
    R.close(); p.close(); model.close()
    print(json.dumps(res))
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
