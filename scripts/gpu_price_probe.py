"""Resident price profiles (GpuProblem.upload_prices / instance_cost_from_prices / sim_log_cost_begin, kernels k_price_cost and k_stage_cost) at the bench
shard (64 models x 512 scenarios = 32 768 instances): what the device routes cost against the host routes they replace.

    python scripts/gpu_price_probe.py [--out profiles/price_profiles_probe.json]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python scripts/gpu_price_probe.py --kernel-only
    python scripts/gpu_price_probe.py --summarise DIR [--merge FILE.json]

* default, every pair ALTERNATING in one session, one warm-up round and seven timed rounds, median and range:
  (a) the wall time of instance_cost_from_prices(start, step) and of instance_cost_from_prices(None, step) against upload_instance_cost(lin_v=...) with
      the same weights, built on the host beforehand (prices.cost_np, not timed) -- the upload route as the parent commit has it;
  (b) the wall time of a logging, advancing, resolving step (small_lds resolver) with the stage cost armed against the same step unarmed -- each the
      SECOND step after an upload -- and against the unarmed step followed by the host's product: the record's v downloaded and multiplied by the price.
* --kernel-only: for ONE kernel trace of its own -- three instance_cost_from_prices, three device-to-device copies of the bytes k_price_cost writes, and
  three armed steps.
* --summarise: k_price_cost against the copy x 1.25 (recorded, not gated), k_stage_cost's time and its share of the step's kernels.
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
MARGIN = 1.25
STEP_KERNELS = ("k_aux_inputs", "k_small_milp", "k_aux_merge", "k_sim_step", "k_stage_cost")


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
    keep = ("k_price_cost",) + STEP_KERNELS
    out = dict(kernels={k: dict(calls=len(v), average_ns=float(np.mean(v)), min_ns=float(min(v)), max_ns=float(max(v))) for k, v in sorted(seen.items()) if k in keep})
    copies = seen.get("copy_kernel", [])
    if len(copies) >= 3 and "k_price_cost" in out["kernels"]:      # the three large ones are this script's (the library's own device copies are a batch of ints)
        y = float(np.mean(sorted(copies)[-3:]))
        out["k_price_cost_yardstick"] = dict(margin=MARGIN, bytes=nbytes, copy_ns=y, over_allowed=out["kernels"]["k_price_cost"]["average_ns"] / (y * MARGIN), gated=False)
    else:
        out["yardstick"] = "the device-to-device copies did not show as kernels in this trace (%d copy kernels seen)" % len(copies)
    if "k_stage_cost" in out["kernels"]:
        step = sum(out["kernels"][k]["average_ns"] for k in STEP_KERNELS if k in out["kernels"])
        out["k_stage_cost_share_of_step_kernels"] = out["kernels"]["k_stage_cost"]["average_ns"] / step
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
        s = summarise(sys.argv[sys.argv.index("--summarise") + 1], (rec.get("bytes") or {}).get("k_price_cost_writes"))
        print(json.dumps(s, indent=1))
        if path:
            rec["trace"] = s
            json.dump(rec, open(path, "w"), indent=1)
        return
    import bench
    from pyhybridcontrol_amd import gpu, prices, synthetic as syn, _lib
    from pyhybridcontrol_amd.aux_resolve import BatchAuxResolver
    kernel_only = "--kernel-only" in sys.argv
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    agents, N_p, N_t, x0, om, midx = bench.make_shard(BATCH_MODELS, BATCH_SCEN, 0)
    d = agents[0]["dims"]
    B, nu, n_h = x0.shape[0], d["nu"], d["nx"]
    mats = [a["mats"] for a in agents]
    model = gpu.GpuModel(mats, d)
    nv = model.nv
    n = N_t * nv
    res = dict(version=_lib.version(), batch=B, models=len(agents), dims={k: int(v) for k, v in d.items()}, N_tilde=N_t, n=n,
               bytes=dict(price_route_starts_per_step=8 * B, price_route_resident_starts_per_step=0, upload_route_per_step=8 * B * n, k_price_cost_writes=8 * B * n))
    # the tariff: four series of two days, every instance on one of them at its own time of day; q_z = prices_tilde on the z column, q_mu = sum * P_h_Nom * (10, 1)
    T = 192 + N_t + 8
    rng = np.random.default_rng(5)
    lib = np.concatenate([syn.price_vector(T) * f for f in (1.0, 0.6, 1.7, 1.2)])
    start = (rng.integers(0, 4, B) * T + rng.integers(0, 192, B)).astype(np.int64)
    z, mu = nu + d["ndelta"], nu + d["ndelta"] + d["nz"]
    a_v, sum_v = np.zeros((len(agents), 1, nv)), np.zeros((len(agents), 1, nv))
    a_v[:, 0, z] = 1.0
    for k, a in enumerate(agents):
        sum_v[k, 0, mu:mu + 2 * n_h:2], sum_v[k, 0, mu + 1:mu + 2 * n_h:2] = 10.0 * a["params"]["P_h_Nom"], a["params"]["P_h_Nom"]
    p = gpu.GpuProblem(model, N_p, N_t, None, gap_rel=1e-2, max_nodes=800, max_pivots=40000)
    p.upload(x0, om, midx)
    p.upload_prices(lib)
    p.set_price_cost(a_v=a_v, sum_v=sum_v)
    w_v = np.zeros((len(agents), 1, nv))
    w_v[:, 0, z] = 1.0
    p.set_stage_cost(w_v=w_v)
    R = BatchAuxResolver(mats, d, small_lds=True)

    def timed(fn):
        t = time.perf_counter()
        out = fn()
        return (time.perf_counter() - t) * 1e3, out

    def fresh(arm):
        p.upload(x0, om, midx)
        p.instance_cost_from_prices(start, 0)
        p.sim_log_begin(2)
        if arm:
            p.sim_log_cost_begin(start)

    if kernel_only:
        for k in range(3):
            p.instance_cost_from_prices(start, k)
        d2d_copies(8 * B * n)
        for _ in range(3):
            fresh(True)
            p.solve_resident()
            p.sim_step(resolve=R, step=0)
        print(json.dumps(res))
        R.close(); p.close(); model.close()
        return
    # (a) the cost route
    lin_v, _ = prices.cost_np(lib, start, 1, N_t, 1, a_v=a_v, sum_v=sum_v, model_idx=midx, n_models=len(agents))
    p.instance_cost_from_prices(start, 1)
    same = bool(np.array_equal(p.instance_cost()["q"], lin_v))
    wall = dict(from_prices_with_starts=[], from_prices_resident_starts=[], upload_instance_cost=[])
    for r in range(8):      # (every call builds the cost in a buffer of its own and releases the one it replaces: all three pay for that alike)
        t_n, _ = timed(lambda: p.instance_cost_from_prices(None, 1))
        t_s, _ = timed(lambda: p.instance_cost_from_prices(start, 1))
        t_u, _ = timed(lambda: p.upload_instance_cost(lin_v=lin_v))
        if r >= 1:
            wall["from_prices_with_starts"].append(t_s); wall["from_prices_resident_starts"].append(t_n); wall["upload_instance_cost"].append(t_u)
    res["cost_route"] = dict(wall={k: stat(v) for k, v in wall.items()}, device_weights_equal_numpy_bitwise=same)
    w = res["cost_route"]["wall"]
    res["cost_route"]["upload_over_price_route"] = round(w["upload_instance_cost"]["median_ms"] / w["from_prices_with_starts"]["median_ms"], 2)
    res["cost_route"]["upload_over_resident_starts"] = round(w["upload_instance_cost"]["median_ms"] / w["from_prices_resident_starts"]["median_ms"], 2)
    print("cost route:", res["cost_route"], flush=True)
    # (b) the step
    dp = C.POINTER(C.c_double)

    def host_cost():
        """the route the library had: the last record's v to the host, times the price of its step"""
        v = np.zeros((1, B, nv))
        gpu.check(_lib.load().mld_download_sim_log(p._h, 1, 1, None, v.ctypes.data_as(dp), None, None, None, None, None, None, None, None, None, None))
        return lib[start + 1] * v[0, :, z]

    wall = dict(armed_step=[], unarmed_step=[], unarmed_step_and_host_product=[])
    equal = None
    for r in range(8):
        fresh(True)
        p.solve_resident()
        p.sim_step(resolve=R, step=0)
        p.solve_resident()
        t_a, _ = timed(lambda: p.sim_step(resolve=R, step=1))
        dev = p.sim_log_cost(1, 1)["cost"][0]
        fresh(False)
        p.solve_resident()
        p.sim_step(resolve=R, step=0)
        p.solve_resident()
        t_u, _ = timed(lambda: p.sim_step(resolve=R, step=1))
        t_h, hc = timed(host_cost)
        equal = bool(np.array_equal(dev, hc, equal_nan=True))
        if r >= 1:
            wall["armed_step"].append(t_a); wall["unarmed_step"].append(t_u); wall["unarmed_step_and_host_product"].append(t_u + t_h)
    res["step"] = dict(wall={k: stat(v) for k, v in wall.items()}, device_cost_equals_host_product_bitwise=equal)
    s = res["step"]["wall"]
    res["step"]["armed_minus_unarmed_ms"] = round(s["armed_step"]["median_ms"] - s["unarmed_step"]["median_ms"], 3)
    res["step"]["host_route_over_armed"] = round(s["unarmed_step_and_host_product"]["median_ms"] / s["armed_step"]["median_ms"], 2)
    print("step:", res["step"], flush=True)
    R.close(); p.close(); model.close()
    print(json.dumps(res))
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
