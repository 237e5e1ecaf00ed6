"""Campaign KPIs on the device (GpuProblem.sim_log_summary, kernel k_log_summary) at the bench shard (64 models x 512 scenarios = 32 768 instances): 25
logged records, 8 KPIs (the reference's columns: p_imp, p_exp, cost, mu over and under, three switch counts), against the routes the summary replaces.

    python scripts/gpu_log_summary_probe.py [--out profiles/log_summary_probe.json]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python scripts/gpu_log_summary_probe.py --kernel-only
    python scripts/gpu_log_summary_probe.py --summarise DIR [--merge FILE.json]

* default, the routes ALTERNATING in one session, one warm-up round and seven timed rounds, median and range: the wall time of sim_log_summary() against
  sim_log() + sim_log_cost() + simlog.summary_np (the restatement, loops over k and i), and against the same downloads + a vectorised numpy reduction
  (einsum and axis reductions: sum, min, max, n_above, n_stepped).
* --kernel-only: for ONE kernel trace of its own -- three summaries and three device-to-device copies of the bytes k_log_summary reads.
* --summarise: k_log_summary against the copy x 1.25 (recorded, not gated).

The log is filled through sim_step(v0=...) with drawn step inputs (no solve: the summary does not care where a record came from), the stage cost armed.
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

BATCH_MODELS, BATCH_SCEN, RECORDS = 64, 512, 25
MARGIN = 1.25


def stat(ms):
    return dict(median_ms=round(float(np.median(ms)), 3), min_ms=round(min(ms), 3), max_ms=round(max(ms), 3), ms=[round(v, 3) for v in ms])


def summarise(d, nbytes):
    seen, rows = {}, []
    for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        rows += list(csv.DictReader(open(f)))
    for r in sorted(rows, key=lambda r: int(r["Start_Timestamp"])):
        name = r["Kernel_Name"].split("(")[0]
        key = "copy_kernel" if "copyBuffer" in name else name
        if key in ("k_log_summary", "copy_kernel"):
            seen.setdefault(key, []).append(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
    out = dict(kernels={k: dict(calls=len(v), average_ns=float(np.mean(v)), min_ns=float(min(v)), max_ns=float(max(v)), ns=v[-6:]) for k, v in sorted(seen.items())})
    copies = seen.get("copy_kernel", [])
    if len(copies) >= 3 and "k_log_summary" in seen:      # the three large ones are this script's
        y = float(np.mean(sorted(copies)[-3:]))
        t = float(np.mean(seen["k_log_summary"][-3:]))
        out["k_log_summary_yardstick"] = dict(margin=MARGIN, bytes=nbytes, copy_ns=y, kernel_ns=t, over_allowed=t / (y * MARGIN), under_the_copy=bool(t < y), gated=False,
                                              read_GB_per_s=(nbytes / t) if nbytes else None)
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


def vectorised(log, price, arr, midx):
    """the reduction as numpy would write it: one einsum per table, axis reductions over the stepped records"""
    f = np.einsum("bqi,kbi->kbq", arr["w_v"][midx], np.nan_to_num(log["v"])) + np.einsum("bqi,kbi->kbq", arr["w_y"][midx], np.nan_to_num(log["y"]))
    for q in np.flatnonzero(arr["price_chan"] >= 0):
        f[:, :, q] *= price[:, :, arr["price_chan"][q]]
    on = ~np.isnan(log["x_k1"][:, :, :1])
    return dict(sum=np.where(on, f, 0.0).sum(axis=0), min=np.where(on, f, np.inf).min(axis=0), max=np.where(on, f, -np.inf).max(axis=0),
                n_above=(on & (f > arr["thresh"][midx][None])).sum(axis=0), n_stepped=on[:, :, 0].sum(axis=0))


def main():
    if "--summarise" in sys.argv:
        rec, path = {}, None
        if "--merge" in sys.argv:
            path = sys.argv[sys.argv.index("--merge") + 1]
            rec = json.load(open(path)) if os.path.exists(path) else {}
        s = summarise(sys.argv[sys.argv.index("--summarise") + 1], (rec.get("bytes") or {}).get("k_log_summary_reads"))
        print(json.dumps(s, indent=1))
        if path:
            rec["trace"] = s
            json.dump(rec, open(path, "w"), indent=1)
        return
    import bench
    from pyhybridcontrol_amd import gpu, simlog, synthetic as syn, _lib
    kernel_only = "--kernel-only" in sys.argv
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    agents, N_p, N_t, x0, om, midx = bench.make_shard(BATCH_MODELS, BATCH_SCEN, 0)
    d = agents[0]["dims"]
    B, nu, M = x0.shape[0], d["nu"], len(agents)
    model = gpu.GpuModel([a["mats"] for a in agents], d)
    nv = model.nv
    # the reference's columns, 8 of them
    ref = simlog.KpiTable.microgrid(d, n_models=M, price_chan=0)
    kpis = simlog.KpiTable(M, d)
    for q in range(8):
        kpis.add(ref.names[q], price_chan=None if ref._chan[q] < 0 else ref._chan[q], thresh=ref._thresh[q], **ref._rows[q])
    arr = kpis.arrays()
    read = RECORDS * B * (8 * (nv + d["ny"] + 1 + 1 + 1) + 4)      # v, y, x_k1[0], price, cons_vio; nodes
    res = dict(version=_lib.version(), batch=B, models=M, records=RECORDS, kpis=kpis.names, dims={k: int(v) for k, v in d.items()},
               bytes=dict(record_per_instance=8 * (2 * d["nx"] + nv + d["ny"] + d["nomega"] + 3) + d["nc"] + 12, k_log_summary_reads=read,
                          summary_downloads=B * (len(kpis) * (3 * 8 + 4 * 4) + 3 * 4 + 8 + 8 + 12),
                          log_download=RECORDS * B * (8 * (2 * d["nx"] + nv + d["ny"] + d["nomega"] + 3) + d["nc"] + 12 + 16)))
    p = gpu.GpuProblem(model, N_p, N_t, None, gap_rel=1e-2, max_nodes=800, max_pivots=40000)
    p.upload(x0, om, midx)
    T = RECORDS + 4
    lib = np.concatenate([syn.price_vector(T) * f for f in (1.0, 0.6, 1.7, 1.2)])
    rng = np.random.default_rng(6)
    start = (rng.integers(0, 4, B) * T).astype(np.int64)
    w_v = np.zeros((M, 1, nv))
    w_v[:, 0, nu + d["ndelta"]] = 1.0
    p.upload_prices(lib)
    p.set_stage_cost(w_v=w_v)
    p.sim_log_begin(RECORDS)
    p.sim_log_cost_begin(start)
    for k in range(RECORDS):
        v0 = np.zeros((B, nv))
        v0[:, :nu] = rng.uniform(size=(B, nu)) < 0.3
        v0[:, nu:] = rng.uniform(0.0, 2000.0, (B, nv - nu)) * (rng.uniform(size=(B, nv - nu)) < 0.5)
        p.sim_step(v0=v0, step=k, advance=True)
    assert p.sim_log_count() == (RECORDS, RECORDS)

    def timed(fn):
        t = time.perf_counter()
        out = fn()
        return (time.perf_counter() - t) * 1e3, out

    if kernel_only:
        for _ in range(3):
            p.sim_log_summary(kpis)
        d2d_copies(read)
        print(json.dumps(res))
        p.close(); model.close()
        return

    def host_np():
        log, price = p.sim_log(), p.sim_log_cost()["price"]
        return simlog.summary_np(log, kpis, midx, price=price)

    def host_vec():
        log, price = p.sim_log(), p.sim_log_cost()["price"]
        return vectorised(log, price, arr, midx)

    wall = dict(sim_log_summary=[], sim_log_and_summary_np=[], sim_log_and_vectorised_numpy=[], sim_log_download_alone=[])
    same = close = None
    for r in range(8):
        t_d, dev = timed(lambda: p.sim_log_summary(kpis))
        t_n, ref_np = timed(host_np)
        t_v, ref_v = timed(host_vec)
        t_l, _ = timed(lambda: (p.sim_log(), p.sim_log_cost()))
        same = bool(all(np.array_equal(dev[k], ref_np[k]) for k in ref_np if k != "names") and np.array_equal(dev["sum"].view(np.uint64), ref_np["sum"].view(np.uint64)))
        close = bool(np.allclose(dev["sum"], ref_v["sum"], rtol=1e-10, atol=1e-6) and np.array_equal(dev["n_stepped"], ref_v["n_stepped"]))
        if r >= 1:
            wall["sim_log_summary"].append(t_d); wall["sim_log_and_summary_np"].append(t_n); wall["sim_log_and_vectorised_numpy"].append(t_v)
            wall["sim_log_download_alone"].append(t_l)
    res["wall"] = {k: stat(v) for k, v in wall.items()}
    res["device_equals_summary_np_bitwise"] = same
    res["device_close_to_vectorised_numpy"] = close
    w = res["wall"]
    res["summary_np_route_over_device"] = round(w["sim_log_and_summary_np"]["median_ms"] / w["sim_log_summary"]["median_ms"], 1)
    res["vectorised_route_over_device"] = round(w["sim_log_and_vectorised_numpy"]["median_ms"] / w["sim_log_summary"]["median_ms"], 1)
    p.close(); model.close()
    print(json.dumps(res))
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
