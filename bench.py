#!/usr/bin/env python3
"""Benchmark of the MPC hot path on MI355X:  python bench.py --gpus N --steps K --warmup W

Workload (BASELINE.json metric "MPC steps/sec ... 64-agent microgrid N=24", configs[3]): 64 distinct agents
(cluster of 7 water heaters + grid tie, N_p=24 -> n=575 variables / 200 binaries / 500 rows each) x scenarios;
the full configuration is 4096 scenarios x 64 agents over 8 GPUs, i.e. 512 scenarios x 64 agents = 32768
independent MILP instances per GPU.  WEAK scaling: every rank solves that per-GPU shard, instance ids are
contiguous blocks of the flattened (scenario, agent) index.

One "step" = one pass of the hot path over the rank's resident batch with NEW inputs: before the timed region K + W + 2 independent
scenario sets (the same seeded distribution) are staged in HBM (mld_stage_inputs); a step makes the next set current by a
device-to-device copy (mld_select_inputs), then K3 (right-hand sides, MFMA GEMM) and K5/K6 (cut-and-branch), followed by the RCCL
gather of (objective, status, step-0 inputs) when N > 1.  One "MPC step" of the metric = one agent-solve.  The longest-first work
queue is learnt from the PREVIOUS step, i.e. from different instances of the same agents.  After the timed region a closed-loop leg
(mld_advance_batch: plant update with the inputs just computed, forecast shifted; the shifted plan as MIP start) reports how the rate
moves when the population drifts out of the seeded regime towards its steady state (harder instances than the synthetic distribution,
DESIGN section 6).

No torch anywhere: ranks / addresses come from the environment `python -m torch.distributed.run` exports, the RCCL
unique id travels over a small TCP side channel (pyhybridcontrol_amd.batch.TcpRendezvous).

Prints ONE JSON line on rank 0: `metric`, `value` (agent-solves/s over the K timed steps), `unit`, `higher_is_better`, `dtype`, `ms_per_step`
(milliseconds of one timed step) and a `config` that describes the workload and the timed region.  A plain run does nothing else: set-up,
staging, warm-up + timed steps, the result line.  `--dump-outputs DIR` writes what the last timed step computed (dump_outputs) after the
timed region.

`--full` adds every other leg: `roofline` (dominant kernel k_solve) and `cpu_baseline` (the C oracle and scipy's HiGHS on a bounded sample:
one thread and every core this container may use), the exact-gap (1e-6) leg -- with sub-tree hand-off and, for continuity, in one pass --
checked against the committed HiGHS optima, and the same hand-off at the bench's own contract.  Order of a --full run: CPU leg (before the
first HIP call: its HiGHS pool forks), exact leg, hand-off leg, staging, warm-up + timed steps, fixed-cost steps, reference steps,
queue-order check, closed loop (24 steps, MIP start from the shifted plan), single-instance / MIQP / cfg5 legs, condensing.  Progress lines
go to stderr.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0   # MI355X HBM3E spec peak (guides/MI355X_MICROARCH.md)


def pattern_ceiling():
    """what the memory system delivers for k_solve's update pattern on every CU at once (scripts/micro/sector_rmw.hip): read from the committed
    measurement, newest round first -- (GB/s at 38 % active sectors, GB/s with every sector active, file)"""
    import re
    for name in ("r04_sector_rmw.txt", "r03_sector_rmw.txt"):
        path = os.path.join(ROOT, "profiles", name)
        if not os.path.exists(path):
            continue
        part = full = None
        for line in open(path):
            m = re.search(r"mode 0 .*wgs\s+256 threads 512 sector\s+64 B active\s+([0-9.]+)%.*?([0-9.]+)\s+GB/s", line)
            if not m:
                continue
            if abs(float(m.group(1)) - 38.0) < 0.5 and part is None:
                part = float(m.group(2))
            if abs(float(m.group(1)) - 100.0) < 0.5 and full is None:
                full = float(m.group(2))
        if part:
            return part, full, "profiles/" + name
    return None, None, None


def parse_kwargs(text):
    """'mir_per_round=10,cut_rounds=4' -> dict (ints / floats); replaces the eval() of round 3"""
    out = {}
    for item in filter(None, (t.strip() for t in text.split(","))):
        k, _, v = item.partition("=")
        try:
            out[k.strip()] = int(v)
        except ValueError:
            out[k.strip()] = float(v)
    return out


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--agents", type=int, default=64)
    ap.add_argument("--scenarios", type=int, default=512, help="scenarios per GPU (4096 over 8 GPUs)")
    ap.add_argument("--mip-gap", type=float, default=1e-2, help="relative MIP gap; 1e-2 is the reference's own setting "
                    "(micro_grid_control_simulation.py:232 MIPGap=1e-2)")
    ap.add_argument("--node-limit", type=int, default=800, help="per-instance node limit (stands in for the reference's TimeLimit)")
    ap.add_argument("--pivot-limit", type=int, default=40000, help="per-instance simplex iteration limit")
    ap.add_argument("--full", action="store_true", help="every leg besides the timed steps (CPU baseline, exact-gap and hand-off legs, fixed-cost and "
                    "reference steps, roofline, queue-order check, closed loop, single-instance / MIQP / cfg5 legs, condensing roofline); the "
                    "options below that name a leg act only with --full")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="write what the last timed step computed to DIR/<name>.npy (float64; "
                    "rank 0's shard, v for a seeded sample of instances)")
    ap.add_argument("--cpu-sample", type=int, default=1024, help="instances timed with the CPU oracle on all cores (0 = skip)")
    ap.add_argument("--exact-sample", type=int, default=-1, help="instances of the exact-gap leg (-1 = the whole shard, 0 = skip)")
    ap.add_argument("--closed-loop-steps", type=int, default=24, help="steps of the closed-loop leg after the timed region (0 = skip)")
    ap.add_argument("--closed-loop-cold", action="store_true", help="closed-loop leg without the MIP start from the shifted previous plan")
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--handles", type=int, default=2, help="problem handles (each with its own HIP stream and workspace) the timed steps alternate over: "
                    "the workgroups of step k+1 move onto the CUs the stragglers of step k leave idle; 1 = one step after another")
    ap.add_argument("--reference-steps", type=int, default=2, help="steps solved strictly one after another after the timed region (roofline, latency, value_one_at_a_time)")
    ap.add_argument("--reserved", type=int, default=0, help="diagnostics: opts.reserved bits for the solver (include/mldgpu.h), e.g. 16384 = no long-step ratio test in the root LP")
    ap.add_argument("--solver-opts", type=str, default="", help="diagnostics: extra solver options, e.g. 'mir_per_round=10,cut_rounds=4'")
    ap.add_argument("--fixed-cost", action="store_true", help="keep one cost for every timed step (round 3) instead of new prices per step (mld_problem_set_cost inside the timed region)")
    ap.add_argument("--no-extra-legs", action="store_true", help="skip the cfg5 / MIQP / single-instance legs after the timed region")
    ap.add_argument("--rehearse", action="store_true", help="multi-rank rehearsal on ONE GPU: every rank on device 0, gather over the TCP side channel")
    args = ap.parse_args(argv)
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be at least 1 and --warmup at least 0")
    return args


def make_shard(n_agents, n_scen, scen_offset):
    """agents (models + costs) are the same on every rank; scenarios are seeded by their GLOBAL index"""
    from pyhybridcontrol_amd import synthetic as syn
    cfg = syn.CONFIGS["cfg4"]
    n_h, N_p = cfg["n_h"], cfg["N_p"]
    N_t = N_p + 1
    agents = []
    for a in range(n_agents):
        rng = np.random.Generator(np.random.PCG64(cfg["seed"] * 1000 + a))
        mats, dims, params = syn.make_agent(n_h, rng)
        atoms = syn.make_cost(n_h, N_t, params)
        agents.append(dict(mats=mats, dims=dims, params=params, atoms=atoms))
    nx, nW = n_h, N_t * (n_h + 1)
    x0 = np.zeros((n_scen, n_agents, nx))
    om = np.zeros((n_scen, n_agents, nW))
    for s in range(n_scen):
        for a in range(n_agents):
            rng = np.random.Generator(np.random.PCG64([cfg["seed"], scen_offset + s, a]))
            xs, ws = syn.make_scenarios(n_h, N_t, 1, rng)
            x0[s, a], om[s, a] = xs[0], ws[0]
    # flatten i = s * n_agents + a  
    midx = np.tile(np.arange(n_agents, dtype=np.int32), n_scen)
    return agents, N_p, N_t, x0.reshape(-1, nx), om.reshape(-1, nW), midx


def progress(msg):
    """one line on stderr (rank 0): a bench run prints its single JSON line at the very end, and a silent command is taken to be hung"""
    if int(os.environ.get("RANK", "0")) == 0:
        print("[bench %s] %s" % (time.strftime("%H:%M:%S"), msg), file=sys.stderr, flush=True)


def step_scenarios(rank, t, n_local):
    """scenario set t >= 1 of a rank's timed region: (x0, omega) of its n_local instances, instance i on agent i % n_agents like set 0.
    Seeded by (cfg4 seed, 7919, rank, t) -- tests/golden/solve_cfg4_timed.npz pins the first instances of (rank 0, t = 1)."""
    from pyhybridcontrol_amd import synthetic as syn
    cfg = syn.CONFIGS["cfg4"]
    rng = np.random.Generator(np.random.PCG64([cfg["seed"], 7919, rank, t]))
    return syn.make_scenarios(cfg["n_h"], cfg["N_p"] + 1, n_local, rng)


def host_description():
    model = "unknown"
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                model = line.split(":", 1)[1].strip()
                break
    except OSError:
        pass
    try:
        usable = len(os.sched_getaffinity(0))
    except AttributeError:
        usable = os.cpu_count() or 1
    quota = None
    try:        # the container's CPU share (cgroup v2 cpu.max / v1 cfs quota): a one-GPU box grants a fraction of the host's hardware threads
        txt = open("/sys/fs/cgroup/cpu.max").read().split()
        if txt[0] != "max":
            quota = float(txt[0]) / float(txt[1])
    except (OSError, ValueError, IndexError):
        try:
            q, per = int(open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read()), int(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
            if q > 0 and per > 0:
                quota = q / per
        except (OSError, ValueError):
            pass
    if quota is not None:
        usable = max(1, min(usable, int(round(quota))))
    return dict(cpu_model=model, nproc=os.cpu_count() or 1, usable_cores=usable, cpu_quota=quota)


def cpu_baseline(agents, N_p, N_t, x0, om, midx, n_sample, gap, node_limit, pivot_limit):
    """the C oracle (oracle/mld_oracle.c, kind "port": same algorithm, same options) on a bounded sample drawn ACROSS the shard
    (every agent, scenarios spread over the whole range: the hard tail is represented): one host thread and, with OpenMP
    over instances, every core this process may use.  scipy's HiGHS on the original rows beside it."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import condense_np as cn
    import orc
    import tighten_np
    host = host_description()
    n_sample = min(n_sample, x0.shape[0])
    n_ag = len(agents)
    n_sc = x0.shape[0] // n_ag
    k = np.arange(n_sample)
    idx = np.unique(((k * n_sc) // n_sample) * n_ag + (k * 37) % n_ag)      # instance i = scenario * n_agents + agent: scenarios spread over the shard, every agent
    forms, raw = {}, {}
    qs, Gs, hs = [], [], []
    for i in idx:
        a = int(midx[i])
        ag = agents[a]
        if a not in forms:   # condensing + tightening is per model: problem set-up, not timed (like on the GPU)
            d = ag["dims"]
            forms[a] = cn.standard_form(tighten_np.tighten(ag["mats"], d, nu_l=d["nu_l"]), ag["atoms"], N_p, N_t, nu_l=d["nu_l"])
        sf = forms[a]
        qs.append(cn.lin_cost(sf["cost"], x0[i], om[i]))
        hs.append(cn.rhs(sf["evo"], x0[i], om[i]))
        Gs.append(sf["G"])
    sf0 = forms[int(midx[idx[0]])]
    # (first: the pool forks its workers, and a fork after the OpenMP region of the oracle below is not safe with libgomp)
    # an independent third-party CPU solver on the SAME sample (original, un-tightened rows): scipy's HiGHS at the same MIPGap, one process per
    # core (the instances are independent -- SURVEY 8d "as an independent third-party CPU reference"), and the one-thread rate beside it
    try:
        import multiprocessing as mp
        for i in idx:
            a = int(midx[i])
            if a not in raw:
                raw[a] = cn.standard_form(agents[a]["mats"], agents[a]["atoms"], N_p, N_t, nu_l=agents[a]["dims"]["nu_l"])
        _HIGHS.update(raw=raw, x0=x0, om=om, midx=midx, gap=gap)
        progress("cpu baseline: HiGHS on %d instances, 1 thread then a fork pool" % len(idx))
        procs = max(1, min(host["usable_cores"], len(idx)))
        t0 = time.perf_counter()
        # fork, never spawn / exec: nothing in this process has touched the GPU yet (main() runs this leg first) -- and the parent has not run
        # HiGHS yet either (its global task executor owns threads that a forked child would wait for in vain)
        with mp.get_context("fork").Pool(procs, initializer=_highs_init) as pool:
            res = pool.map_async(_highs_one, [int(i) for i in idx], chunksize=max(1, len(idx) // (4 * procs))).get(timeout=240)      # (a stuck pool must not stall the bench)
        t_all = time.perf_counter() - t0
        t0 = time.perf_counter()
        one = [_highs_one(int(i)) for i in idx[:8]]
        t_1 = time.perf_counter() - t0
        third = dict(solver="scipy.optimize.milp (HiGHS), mip_rel_gap=%g, original rows" % gap, value_all=round(len(idx) / t_all, 3),
                                  cores=procs, value=round(len(one) / t_1, 3), unit="agent-solves/s", solved=int(sum(r[0] for r in res)),
                                  cpu_seconds_per_instance=round(float(np.mean([r[1] for r in res])), 4),
                                  sample="value_all: the same %d instances, one process per core (%d processes, multiprocessing fork pool, wall clock "
                                         "incl. pool start-up); value: the first %d of them on one thread" % (len(idx), procs, len(one)))
    except Exception as e:      # noqa: BLE001 -- reported, not fatal: the baseline above stands on its own
        third = dict(solver="scipy.optimize.milp (HiGHS)", error=str(e)[:200])
    opts = dict(gap_rel=gap, max_nodes=node_limit, presolve=4, max_pivots=pivot_limit)      # (presolve bit 2: the per-instance presolve the kernel runs -- the port restates the SAME algorithm)
    n1 = min(32, len(idx))
    progress("cpu baseline: the C oracle on %d instances (1 thread, then OpenMP on %d threads)" % (len(idx), host["usable_cores"]))
    t0 = time.perf_counter()
    r1, _ = orc.solve_milp_batch(qs[:n1], Gs[:n1], hs[:n1], sf0["lb"], sf0["ub"], sf0["is_bin"], threads=1, **opts)
    t1 = time.perf_counter() - t0
    t0 = time.perf_counter()
    ra, used = orc.solve_milp_batch(qs, Gs, hs, sf0["lb"], sf0["ub"], sf0["is_bin"], threads=host["usable_cores"], **opts)
    ta = time.perf_counter() - t0
    out = dict(value=round(len(idx) / ta, 3), unit="agent-solves/s", cores=int(used), kind="port",
               value_all=round(len(idx) / ta, 3), value_1t=round(n1 / t1, 3), nproc=host["nproc"], cpu_quota=host["cpu_quota"], cpu_model=host["cpu_model"],
               sample="%d instances spread over the rank-0 shard (all %d agents, scenarios 0..%d), same MIPGap/NodeLimit/IterationLimit, "
                      "oracle/mld_oracle.c with OpenMP over instances on %d threads (%d proven, %d node-limited); value_1t: the first %d of them on one thread"
                      % (len(idx), len(forms), x0.shape[0] // len(agents) - 1, used, int((ra["status"] == 0).sum()), int((ra["status"] == 2).sum()), n1))
    out["third_party"] = third
    out["note"] = "Gurobi at MIPGap=1e-2 (the reference's backend) is not installable here and was not measured"
    return out


_HIGHS = {}


def _highs_init():
    """pool worker: one thread per process (numpy's BLAS pool would otherwise start a thread per hardware thread in every worker)"""
    try:
        import threadpoolctl
        threadpoolctl.threadpool_limits(1)
    except Exception:       # noqa: BLE001
        pass


def _highs_one(i):
    """one instance of the CPU sample with scipy's HiGHS (worker of cpu_baseline's process pool); returns (solved, seconds)"""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import condense_np as cn
    from scipy.optimize import milp, LinearConstraint, Bounds
    sf = _HIGHS["raw"][int(_HIGHS["midx"][i])]
    h = cn.rhs(sf["evo"], _HIGHS["x0"][i], _HIGHS["om"][i])
    q = cn.lin_cost(sf["cost"], _HIGHS["x0"][i], _HIGHS["om"][i])
    t0 = time.perf_counter()
    r = milp(q, constraints=LinearConstraint(sf["G"], -np.inf, h), bounds=Bounds(sf["lb"], sf["ub"]),
             integrality=sf["is_bin"].astype(int), options=dict(mip_rel_gap=_HIGHS["gap"]))
    return int(r.x is not None), time.perf_counter() - t0


def _lib_n_cu():
    from pyhybridcontrol_amd import _lib
    return _lib.device_info()["n_cu"]


def _against_gold(out, k_max, tag="solve_cfg4_bench.npz"):
    """objectives against the committed HiGHS optima of the shard's first instances (tests/golden/)"""
    gpath = os.path.join(ROOT, "tests", "golden", tag)
    if not os.path.exists(gpath):
        return {}
    opt = np.load(gpath)["obj"]
    k = min(k_max, opt.size)
    rel = (out["obj"][:k] - opt[:k]) / np.maximum(1e-9, np.abs(opt[:k]))
    pk = out["status"][:k] == 0
    return dict(oracle="tests/golden/%s (scipy HiGHS, mip_rel_gap=0, original rows)" % tag, checked=int(k),
                worst_rel_diff_proven=(float(np.abs(rel[pk]).max()) if pk.any() else None),
                worst_rel_above_optimum_all=float(rel[np.isfinite(rel)].max()), below_optimum=int((rel < -1e-6).sum()))


def exact_leg(prob, x0, om, midx, n_exact, args):
    """north star: "within 1e-6 objective of CPU reference".  The same problem at gap 1e-6 on the first n_exact instances of the shard, objectives
    checked against the committed HiGHS optima.  `value_exact` is measured WITH the in-kernel sub-tree hand-off (GpuProblem.solve_handoff_device: 400
    nodes per instance, its open nodes as queue entries of the same launch with 200 nodes each, up to 8 generations, a tree with more than 160 open
    nodes in one generation given up) -- wall clock of upload + launch + download; `single_pass` is round 2's measurement: one workgroup per
    instance, NodeLimit 20 000, where one instance running to its limits holds the launch while the other CUs idle.  (Round 3 drove the same
    hand-off from the host, one launch per generation: GpuProblem.solve_handoff, kept for callers that want the rounds.)"""
    n_exact = x0.shape[0] if n_exact < 0 else min(n_exact, x0.shape[0])
    # the longest-first work queue is learnt from the previous solve of the handle, as in the timed region: one untimed pass at the bench's own
    # options over ANOTHER scenario set of the same agents (agent-level information only)
    xs, ws = step_scenarios(int(os.environ.get("RANK", "0")), 1, x0.shape[0])
    prob.upload(xs[:n_exact], ws[:n_exact], midx[:n_exact])
    prob.solve_resident()
    prob.set_opts(gap_rel=1e-6, max_nodes=20000, max_pivots=400000)
    hand = dict(first_nodes=400, sub_nodes=200, max_gen=8, max_children=64, max_tree=160, room_factor=3.0)      # (scripts/gpu_handoff_device_probe.py: 5.8 k/s at 99.948 % proven;
                                                                              #  300 / 200: 5.2 k/s at 99.939 %, 300 / 150: 6.0 k/s at 99.930 %, tree cap 96: 6.7 k/s at 99.911 %)
    t0 = time.perf_counter()
    out = prob.solve_handoff_device(x0[:n_exact], om[:n_exact], midx[:n_exact], **hand)
    wall = time.perf_counter() - t0
    proven = out["status"] == 0
    res = dict(gap_rel=1e-6, instances=int(n_exact), value_exact=round(n_exact / wall, 2), unit="agent-solves/s", ms=round(wall * 1e3, 2), kernel_ms=round(float(out["stats"]["solve_ms"]), 1),
               proven_fraction=round(float(proven.mean()), 5), nodes_per_instance=round(float(out["nodes"].mean()), 1),
               pivots_per_instance=round(float(out["pivots"].mean()), 1),
               method="in-kernel sub-tree hand-off (mld_set_handoff): ONE launch -- searches that stop at their node limit publish their open nodes as entries of the same "
                      "work queue, idle workgroups solve them, the trees are merged on the device; wall clock of upload + solve + download",
               handoff=dict(hand, **out["handoff"]))
    if args.agents == 64:
        res.update(_against_gold(out, n_exact))
    # round 2's measurement for continuity: one pass, one workgroup per instance, NodeLimit 20 000 / IterationLimit 400 000
    prob.upload(xs[:n_exact], ws[:n_exact], midx[:n_exact])
    prob.set_opts(gap_rel=args.mip_gap, max_nodes=args.node_limit, max_pivots=args.pivot_limit)
    prob.solve_resident()
    prob.set_opts(gap_rel=1e-6, max_nodes=20000, max_pivots=400000)
    prob.upload(x0[:n_exact], om[:n_exact], midx[:n_exact])
    t0 = time.perf_counter()
    st = prob.solve_resident()
    wall1 = time.perf_counter() - t0
    out1 = prob.download()
    tel = prob.telemetry()
    busy = float(tel["latency_ns"].sum()) * 1e-9 / max(1, _lib_n_cu())
    single = dict(node_limit=20000, iteration_limit=400000, value_exact=round(n_exact / wall1, 2), ms=round(wall1 * 1e3, 2), kernel_ms=round(st["solve_ms"], 2),
                  proven_fraction=round(float((out1["status"] == 0).mean()), 5), nodes_per_instance=round(float(out1["nodes"].mean()), 1),
                  pivots_per_instance=round(float(out1["pivots"].mean()), 1), value_no_idle_bound=round(n_exact / busy, 2),
                  slowest_instance_ms=round(float(tel["latency_ns"].max()) * 1e-6, 1),
                  queue="longest-first order learnt from one untimed pass over another scenario set of the same agents at the bench's options")
    if args.agents == 64:
        single.update(_against_gold(out1, n_exact))
    res["single_pass"] = single
    prob.set_opts(gap_rel=args.mip_gap, max_nodes=args.node_limit, max_pivots=args.pivot_limit)
    return res


def handoff_leg(prob, x0, om, midx, args):
    """the bench's own contract (MIPGap / NodeLimit of the timed region) on scenario set 0 with sub-tree hand-off: what the node-limited tail of a
    step becomes when its open nodes are re-queued (quality mode: slower than one pass, nearly everything proven)"""
    hand = dict(first_nodes=args.node_limit, sub_nodes=max(50, args.node_limit // 2), max_gen=4, max_children=64, max_tree=64, room_factor=2.0)
    t0 = time.perf_counter()
    out = prob.solve_handoff_device(x0, om, midx, **hand)
    wall = time.perf_counter() - t0
    fin = np.isfinite(out["obj"])
    lim = out["status"] == 2
    with np.errstate(invalid="ignore"):
        gap = np.where(fin, (out["obj"] - out["lower_bound"]) / np.maximum(1e-9, np.abs(out["obj"])), np.nan)
    res = dict(hand, value=round(x0.shape[0] / wall, 2), unit="agent-solves/s", ms=round(wall * 1e3, 2), proven_fraction=round(float((out["status"] == 0).mean()), 5),
               node_limited=int(lim.sum()), kernel_ms=round(float(out["stats"]["solve_ms"]), 1), queue=out["handoff"],
               gap_of_limited=({"median": round(float(np.nanmedian(gap[lim])), 5), "max": round(float(np.nanmax(gap[lim])), 5)} if lim.any() else None),
               note="wall clock of GpuProblem.solve_handoff_device on scenario set 0 (upload + one launch + download)")
    if args.agents == 64:
        res.update(_against_gold(out, x0.shape[0]))
    return res



def cfg5_leg():
    """BASELINE configs[4] (n_h = 15, N_p = 48: n = 2303, 784 binaries, m = 1764) on the 128 instances that have a committed HiGHS bracket
    (tests/golden/solve_cfg5.npz): proven share, distance from HiGHS's incumbent, rate, dictionary bytes per instance, and the fp32 condensing
    roofline at that shape (16 jittered models per launch)."""
    from pyhybridcontrol_amd import gpu, host, synthetic as syn
    gpath = os.path.join(ROOT, "tests", "golden", "solve_cfg5.npz")
    if not os.path.exists(gpath):
        return None
    gold = np.load(gpath)
    nb = int(gold["n_scen"])
    wl = syn.make_workload("cfg5", batch=nb)
    ag = wl["agents"][0]
    d, N_p, N_t = ag["dims"], wl["N_p"], wl["N_tilde"]
    m = gpu.GpuModel([ag["mats"]], d)
    opts = dict(gap_rel=1e-2, max_nodes=400, max_pivots=160000)
    p = gpu.GpuProblem(m, N_p, N_t, host.cost_from_atoms(ag["atoms"], d, N_p, N_t), **opts)
    p.upload(ag["x0"], ag["omega"])
    t0 = time.perf_counter()
    st = p.solve_resident()
    wall = time.perf_counter() - t0
    out, tel = p.download(), p.telemetry()
    ok = np.isfinite(gold["obj"]) & np.isfinite(gold["dual_bound"])
    rel = (out["obj"][ok] - gold["obj"][ok]) / np.maximum(1e-9, np.abs(gold["obj"][ok]))
    piv = int(out["pivots"].sum())
    upd = 2.0 * int(tel["rows_updated"].sum()) * tel["row_bytes"] + piv * (2 * 8.0 * (p.n + 1) + 2 * 8.0 * p.n + 64.0 * p.m)
    res = dict(workload="BASELINE cfg5 shape, %d instances of one agent (n=%d, %d binaries, m=%d)" % (nb, p.n, p.n_bin, p.m), options=opts,
               value=round(nb / wall, 2), unit="agent-solves/s", kernel_ms=round(float(st["solve_ms"]), 1),
               proven_fraction=round(float((out["status"] == 0).mean()), 4), no_incumbent=int((~np.isfinite(out["obj"])).sum()),
               within_1pct_of_highs_incumbent=round(float((rel <= 1e-2).mean()), 4), worst_rel_above_highs_incumbent=round(float(rel.max()), 4),
               below_highs_dual_bound=int((out["obj"][ok] < gold["dual_bound"][ok] - 1e-6 * np.abs(gold["obj"][ok])).sum()),
               nodes_per_instance=round(float(out["nodes"].mean()), 1), pivots_per_instance=round(piv / nb, 1),
               bytes_per_instance=int(upd / nb), hbm_rate_GBs=round(upd / (float(st["solve_ms"]) * 1e-3) / 1e9, 1),
               oracle="tests/golden/solve_cfg5.npz (scipy HiGHS, mip_rel_gap 1e-4, 240 s per instance: incumbent and dual bound)",
               note="128 instances keep only half of the 256 workgroups busy: the rate is that of a partly filled device (a per-GPU shard of cfg5 is 1024)")
    p.close(); m.close()
    # fp32 condensing at the shape (configs[4]: 'fp32 condensing ... rocprof roofline reported'): 16 jittered agents per launch
    mods = []
    for a in range(16):
        rng = np.random.Generator(np.random.PCG64(syn.CONFIGS["cfg5"]["seed"] * 1000 + a))
        mods.append(syn.make_agent(syn.CONFIGS["cfg5"]["n_h"], rng)[0])
    mm = gpu.GpuModel(mods, d)
    nx, ny, nc, nw, nv = d["nx"], d["ny"], d["nc"], d["nomega"], mm.nv
    cols = N_t * nv + nx + N_t * nw + 1
    small = 8.0 * ((nx + ny + nc) * (nx + nv + nw + 1) + nc * ny)
    b64, b32 = 8.0 * N_t * (nc + nx + ny) * cols + small, 4.0 * N_t * (nc + nx + ny) * cols + small
    ms64 = min(mm.condense_device(N_t) for _ in range(5))
    ms32 = min(mm.condense_device(N_t, f32=True) for _ in range(5))
    res["condense"] = {"models": 16, "bytes_per_model_f32": int(b32), "kernel_ms_f32": round(ms32, 4), "achieved_f32": round(16 * b32 / (ms32 * 1e-3) / 1e9, 1),
                       "frac_f32": round(16 * b32 / (ms32 * 1e-3) / 1e9 / HBM_PEAK_GBS, 4), "bytes_per_model_f64": int(b64), "kernel_ms_f64": round(ms64, 4),
                       "achieved_f64": round(16 * b64 / (ms64 * 1e-3) / 1e9, 1), "frac_f64": round(16 * b64 / (ms64 * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
                       "unit": "GB/s", "peak": HBM_PEAK_GBS, "bound": "hbm", "kernel": "k_condense_model / k_condense_blocks + k_condense_flat<float|double>",
                       "note": "SURVEY 8d algorithmic bytes (outputs + inputs) / min-of-5 HIP-event time; the block arithmetic stays fp64 (inner dimension nx = 15: no MFMA), "
                               "every output element is rounded once to fp32 on its way to HBM"}
    mm.close()
    return res


def miqp_leg(n_inst=4096):
    """The quadratic-cost path (north star: 'batched MIQP'): BASELINE cfg3 shape with the MIQP variant's Q_x = 1e-3 I, same MIPGap /
    NodeLimit as the timed region, next to the MILP of the same instances.  4 096 instances = 16 per resident workgroup: with the 512 of the first version
    of this leg a launch was as long as its slowest instance (two instances per workgroup; 232 solves/s), which says nothing about the path."""
    from pyhybridcontrol_amd import gpu, host, synthetic as syn
    res = {}
    for quad in (False, True):
        wl = syn.make_workload("cfg3", batch=n_inst, quadratic=quad)
        ag = wl["agents"][0]
        d = ag["dims"]
        m = gpu.GpuModel([ag["mats"]], d)
        p = gpu.GpuProblem(m, wl["N_p"], wl["N_tilde"], host.cost_from_atoms(ag["atoms"], d, wl["N_p"], wl["N_tilde"]), gap_rel=1e-2, max_nodes=800, max_pivots=40000)
        p.upload(ag["x0"], ag["omega"])
        p.solve_resident()                      # (first solve: learns the queue order)
        t0 = time.perf_counter()
        st = p.solve_resident()
        wall = time.perf_counter() - t0
        out = p.download()
        res["miqp" if quad else "milp_same_instances"] = dict(value=round(n_inst / wall, 1), kernel_ms=round(float(st["solve_ms"]), 1),
                                                              proven_fraction=round(float((out["status"] == 0).mean()), 4), no_incumbent=int((~np.isfinite(out["obj"])).sum()),
                                                              nodes_per_instance=round(float(out["nodes"].mean()), 1), pivots_per_instance=round(float(out["pivots"].mean()), 1))
        p.close(); m.close()
    res.update(unit="agent-solves/s", instances=n_inst,
               workload="BASELINE cfg3 shape (n_h=7, N_p=24), Q_x = 1e-3 I added to the example's linear atoms; MIPGap 1e-2, NodeLimit 800; parity: tests/test_gpu_miqp.py")
    return res


def single_instance_leg(agents, N_p, N_t, x0, om, midx, latency_ns, opts, n_hard=64):
    """What ONE solve() call of the reference costs here (controller_base.py:491-540 solves one instance per call, and its backend runs that one
    tree to the gap): the hardest instances of the last reference step (largest in-kernel latency), solved TO THE GAP (MIPGap of the bench, node /
    pivot limits out of the way) (i) each alone through MpcController.solve -- upload, K3, K5/K6, download of one instance -- on one workgroup and with
    the in-kernel hand-off, and (ii) all n_hard as one batch through the batched harness, both ways."""
    import pyhybridcontrol_amd as phc
    from pyhybridcontrol_amd import gpu, host
    opts = dict(opts, max_nodes=20000, max_pivots=400000)          # to the gap: the limits of the timed region would end the hardest searches unproven
    order = np.argsort(-latency_ns)
    top1 = order[: max(1, len(order) // 100)]
    hard = order[:n_hard]
    # batch-1 calls: controllers for the (at most 4) agents that own most of the hardest 1 %
    ag_ids, counts = np.unique(midx[top1], return_counts=True)
    pick = ag_ids[np.argsort(-counts)][:4]
    HO = dict(first_nodes=100, sub_nodes=200, max_gen=8, max_children=64, max_tree=160)
    lat1, lat1h, n_calls, proven1, proven1h = [], [], 0, 0, 0
    for a in pick:
        ag = agents[int(a)]
        d = ag["dims"]
        mine = [i for i in top1 if midx[i] == a][:8]
        for ho in (None, HO):
            ctrl = phc.MpcController(phc.MldModel(ag["mats"], nu_l=d["nu_l"]), N_p=N_p, handoff=ho, **opts)
            ctrl.set_std_obj_atoms(**ag["atoms"])
            ctrl.build()
            ctrl.solve(0, x_k=x0[mine[0]], omega_tilde_k=om[mine[0]], warm_start=False)      # (first call: allocations)
            for i in mine:
                t0 = time.perf_counter()
                ctrl.solve(0, x_k=x0[i], omega_tilde_k=om[i], warm_start=False)
                (lat1 if ho is None else lat1h).append((time.perf_counter() - t0) * 1e3)
                if ho is None:
                    n_calls += 1; proven1 += ctrl._status == "optimal"
                else:
                    proven1h += ctrl._status == "optimal"
            del ctrl
    lat1, lat1h = np.sort(np.array(lat1)), np.sort(np.array(lat1h))
    # one batch of the n_hard hardest
    d = agents[0]["dims"]
    model = gpu.GpuModel([a["mats"] for a in agents], d)
    prob = gpu.GpuProblem(model, N_p, N_t, host.stack_costs([host.cost_from_atoms(a["atoms"], d, N_p, N_t) for a in agents]), **opts)
    prob.solve(x0[hard], om[hard], midx[hard])
    t0 = time.perf_counter()
    out = prob.solve(x0[hard], om[hard], midx[hard])
    wall = (time.perf_counter() - t0) * 1e3
    tel = np.sort(prob.telemetry()["latency_ns"]) * 1e-6
    prob.solve_handoff_device(x0[hard], om[hard], midx[hard], **dict(HO, first_nodes=200))
    t0 = time.perf_counter()
    oh = prob.solve_handoff_device(x0[hard], om[hard], midx[hard], **dict(HO, first_nodes=200))
    wall_h = (time.perf_counter() - t0) * 1e3
    pq = lambda a, f: round(float(a[min(len(a) - 1, int(len(a) * f))]), 2)
    res = dict(batch_1=dict(calls=n_calls, agents=int(len(pick)), p50_ms=pq(lat1, 0.5), p99_ms=pq(lat1, 0.99), max_ms=round(float(lat1[-1]), 2), proven=int(proven1),
                            what="wall time of MpcController.solve(k, x_k, omega_tilde_k) per call, instances drawn from the hardest 1 % of the step: one workgroup per solve"),
               batch_1_handoff=dict(calls=n_calls, p50_ms=pq(lat1h, 0.5), p99_ms=pq(lat1h, 0.99), max_ms=round(float(lat1h[-1]), 2), proven=int(proven1h), handoff=HO,
                                    p99_speedup=round(pq(lat1, 0.99) / max(1e-9, pq(lat1h, 0.99)), 2),
                                    what="the same calls with MpcController(..., handoff=...): the instance's open nodes spread over the idle workgroups of the launch (mld_set_handoff)"),
               batch_64=dict(instances=int(len(hard)), wall_ms=round(wall, 2), p50_ms=round(float(tel[len(tel) // 2]), 2), p99_ms=round(float(tel[min(len(tel) - 1, int(len(tel) * 0.99))]), 2),
                             max_ms=round(float(tel[-1]), 2), proven_fraction=round(float((out["status"] == 0).mean()), 4),
                             what="the %d hardest instances of the step as one batch: wall time of the call and in-kernel latency per instance" % len(hard)),
               batch_64_handoff=dict(wall_ms=round(wall_h, 2), proven_fraction=round(float((oh["status"] == 0).mean()), 4), queue=oh["handoff"], speedup=round(wall / max(1e-9, wall_h), 2),
                                     what="the same batch with the in-kernel hand-off (first 200 / sub 200 nodes): the 192 workgroups without an instance take open nodes"),
               in_step_latency_ms=dict(p50=round(float(np.median(latency_ns[hard])) * 1e-6, 2), max=round(float(latency_ns[hard].max()) * 1e-6, 2),
                                       what="the same instances inside the full 32768-instance step (every CU busy)"))
    prob.close(); model.close()
    return res


class SideChannelGather(object):
    """--rehearse: the result gather over the TCP side channel (several ranks share one GPU, where RCCL cannot run)"""

    def __init__(self, rd):
        self.rd = rd

    def gather_results(self, prob):
        out = prob.download()
        nv = prob.model.nv
        loc = np.concatenate([out["obj"][:, None], out["status"][:, None].astype(np.float64), out["v"][:, :nv]], axis=1)
        return np.stack([np.frombuffer(b, dtype=np.float64).reshape(loc.shape) for b in self.rd.all_gather_bytes(loc.tobytes())])


def run_pipelined(probs, count, state, n_sets, gatherer, costs=None):
    """`count` steps over the handles `probs`: step j is launched on handle j % H as soon as that handle's previous step has been finished
    (statistics, learnt queue order, result gather); returns the per-step statistics once every step has finished.  The order of
    launches, finishes and gathers depends on (count, H) alone -- never on which solve happens to end first -- so every rank issues the
    same sequence of collectives (tests/test_shard_gloo.py rehearses two ranks x two handles with stub problems)."""
    H = len(probs)
    res, pending = [None] * count, [None] * H
    for j in range(count + H):
        q = probs[j % H]
        if pending[j % H] is not None:
            res[pending[j % H]] = q.finish()
            if gatherer is not None:
                gatherer.gather_results(q)
            pending[j % H] = None
        if j < count:
            if costs is not None:
                q.set_cost(costs[state["k"] % len(costs)])      # this step's prices (the reference rebuilds its objective before every solve)
            q.select(state["k"] % n_sets)
            state["k"] += 1
            q.launch()
            pending[j % H] = j
    return res


DUMP_V_ROWS = 4096                  # rows of v in a dump: 4096 x 575 fp64 = 18.8 MB
DUMP_INSTANCE_BYTES = 40 << 20      # per-instance arrays of a dump; with the v rows the files stay under 64 MB


def _dump_sample(b, k, seed):
    """sorted, seeded choice of k of b instances (all of them when b <= k)"""
    if b <= k:
        return np.arange(b)
    return np.sort(np.random.Generator(np.random.PCG64(seed)).choice(b, k, replace=False))


def dump_outputs(path, prob):
    """What a caller of the timed path receives for the handle's last solve (GpuProblem.download), as float64 DIR/<name>.npy:
    obj, lower_bound, status, nodes, pivots and u0 (the step-0 slice of v: what the controller applies) for the instances in `index`
    (every instance of the shard unless that exceeds DUMP_INSTANCE_BYTES), and v itself for the seeded sample of instances in `v_index`."""
    out = prob.download()
    b = out["v"].shape[0]
    nv = prob.model.nv
    idx = _dump_sample(b, DUMP_INSTANCE_BYTES // (8 * (6 + nv)), 1)
    vidx = _dump_sample(b, DUMP_V_ROWS, 2)
    arrays = {"index": idx, "u0": out["v"][idx, :nv], "v_index": vidx, "v": out["v"][vidx]}
    for k in ("obj", "lower_bound", "status", "nodes", "pivots"):
        arrays[k] = out[k][idx]
    os.makedirs(path, exist_ok=True)
    for k, a in arrays.items():
        np.save(os.path.join(path, k + ".npy"), np.ascontiguousarray(a, dtype=np.float64))
    return sorted(arrays)


def headline(args, world, n_local, elapsed, stats_timed, H, cost_update, gatherer):
    """the result line of every run: the rate of the K timed steps and what they were"""
    hist = lambda s: {"optimal": int(s["n_optimal"]), "node_limit": int(s["n_node_limit"]), "infeasible": int(s["n_infeasible"]), "other": int(s["n_numerical"])}
    return {
        "metric": "MPC steps/sec (whole node) + p50 solve latency, 64-agent microgrid N=24",
        "value": round(world * n_local * args.steps / elapsed, 2),
        "unit": "agent-solves/s",
        "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": round(elapsed / args.steps * 1e3, 2),
        "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
        "dtype": "f64", "data": "synthetic",
        "config": {"workload": "BASELINE cfg4 shard: %d agents x %d scenarios per GPU (n_h=7, N_p=24: n=575, 200 binaries, m=500), "
                               "full branch-and-cut MILP (library defaults: per-model big-M tightening, per-instance presolve, Gomory + c-MIR cuts), MIPGap=%g, NodeLimit=%d, IterationLimit=%d; every step solves a fresh, independently seeded "
                               "scenario set of the same distribution" % (args.agents, args.scenarios, args.mip_gap, args.node_limit, args.pivot_limit),
                   "timed_region": "K x (%smld_select_inputs [D2D copy of the next staged scenario set] + mld_solve_launch / mld_solve_finish [K3 + K5/K6] (+ RCCL gather of "
                                   "(obj, status, step-0 inputs) from device buffers when N > 1)), the steps alternating over %d problem handles on their own HIP "
                                   "streams: step k+1 is queued while step k runs, so its workgroups take the CUs the stragglers of step k leave idle (results are "
                                   "bit-identical to one-at-a-time solves); all inputs were staged in HBM before the region, results stay in HBM; the host "
                                   "download of the full results is outside (download_ms)" % ("mld_problem_set_cost [this step's tariff: new q_z / q_mu weights to the device] + " if cost_update else "", H),
                   "instances_per_gpu": n_local, "microgrid_steps_per_s": round(world * n_local * args.steps / elapsed / args.agents, 3),
                   "status_per_step": [hist(s) for s in stats_timed],
                   "proven_fraction": round(float(np.mean([s["n_optimal"] for s in stats_timed]) / n_local), 5),
                   "result_gather": (None if gatherer is None else type(gatherer).__name__),
                   "cost_update_per_step": cost_update},
    }


def latency_ms(tel):
    """p50 / p99 of the in-kernel per-instance solve latency of a handle's last solve"""
    lat = np.sort(tel["latency_ns"]) * 1e-6
    return {"p50_solve_latency_ms": round(float(lat[len(lat) // 2]), 3), "p99_solve_latency_ms": round(float(lat[int(len(lat) * 0.99)]), 3)}


def main():
    args = parse()
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    from pyhybridcontrol_amd import _lib, gpu, host
    from pyhybridcontrol_amd.batch import RcclGather, TcpRendezvous
    rd = TcpRendezvous() if world > 1 else None
    agents, N_p, N_t, x0, om, midx = make_shard(args.agents, args.scenarios, rank * args.scenarios)
    cpu = None
    if args.full and rank == 0 and world == 1 and not args.no_cpu and args.cpu_sample > 0:
        # CPU leg: rank 0 at N=1 only, and BEFORE the first HIP call of this process -- its HiGHS pool forks workers
        cpu = cpu_baseline(agents, N_p, N_t, x0, om, midx, args.cpu_sample, args.mip_gap, args.node_limit, args.pivot_limit)
    _lib.check(_lib.load().mld_set_device(0 if args.rehearse else local_rank))
    d = agents[0]["dims"]
    model = gpu.GpuModel([a["mats"] for a in agents], d)
    cost = host.stack_costs([host.cost_from_atoms(a["atoms"], d, N_p, N_t) for a in agents])
    prob = gpu.GpuProblem(model, N_p, N_t, cost, gap_rel=args.mip_gap, max_nodes=args.node_limit, max_pivots=args.pivot_limit, reserved=args.reserved, **parse_kwargs(args.solver_opts))
    n_local = x0.shape[0]
    exact = None
    if args.full and world == 1 and args.exact_sample != 0:
        progress("exact-gap leg (1e-6) on the shard")
        exact = exact_leg(prob, x0, om, midx, args.exact_sample, args)
    hand1 = None
    if args.full and world == 1 and args.exact_sample != 0:
        progress("hand-off leg at the bench's own contract")
        hand1 = handoff_leg(prob, x0, om, midx, args)
    # fresh scenario sets for every step (set 0 = the shard's own scenarios), all resident in HBM before the timed region; step k solves set k
    # in both kinds of run, so a plain run and a --full run time the same inputs
    n_sets = args.warmup + args.steps
    if args.full:
        n_sets += max(1, args.reference_steps) + 5      # (+ 3 for the fixed-cost continuity steps, + 2 spare)
    progress("staging %d scenario sets" % n_sets)
    prob.upload(x0, om, midx)                       # inputs resident in HBM before the timed region
    from pyhybridcontrol_amd import synthetic as syn
    x0_sets = np.empty((n_sets,) + x0.shape)
    om_sets = np.empty((n_sets,) + om.shape)
    x0_sets[0], om_sets[0] = x0, om
    for t in range(1, n_sets):
        x0_sets[t], om_sets[t] = step_scenarios(rank, t, n_local)
    prob.stage(x0_sets, om_sets)
    # the timed steps alternate over `handles` problem handles on their own HIP streams (consecutive steps are independent scenario sets)
    H = max(1, args.handles)
    probs = [prob]
    for _ in range(1, H):
        q = gpu.GpuProblem(model, N_p, N_t, cost, gap_rel=args.mip_gap, max_nodes=args.node_limit, max_pivots=args.pivot_limit, reserved=args.reserved, **parse_kwargs(args.solver_opts))
        q.upload(x0, om, midx); q.stage(x0_sets, om_sets)
        probs.append(q)
    if H > 1:
        for q in probs:
            q.use_stream()
    del x0_sets, om_sets
    # prices move with the clock: step k of the timed region starts 15 minutes after step k - 1, so its tariff vector is the previous one moved on by
    # one control period (the reference recomputes q_z / q_mu from the tariff before every solve, micro_grid_control_simulation.py:194-198,229).
    # The weight tables are host data prepared before the region; handing them to the device (mld_problem_set_cost) is part of every timed step.
    cost_sets = None
    if not args.fixed_cost:
        import datetime as _dt
        t_base = _dt.datetime(2018, 12, 10, 5, 0)
        cost_sets = []
        for t in range(n_sets):
            t0 = t_base + _dt.timedelta(seconds=syn.TS * t)
            cost_sets.append(host.stack_costs([host.cost_from_atoms(syn.make_cost(syn.CONFIGS["cfg4"]["n_h"], N_t, a["params"], t0=t0), d, N_p, N_t) for a in agents]))
    gatherer = None
    if world > 1:
        if args.rehearse:
            gatherer = SideChannelGather(rd)
        else:
            uid = rd.broadcast(RcclGather.unique_id() if rank == 0 else b"", src=0)
            try:
                gatherer = RcclGather(world, rank, uid)
            except Exception as e:      # noqa: BLE001 -- every rank must take the same path: agreed below
                print("rank %d: RCCL communicator failed (%s)" % (rank, e), file=sys.stderr)
            if not all(b == b"1" for b in rd.all_gather_bytes(b"1" if gatherer is not None else b"0")):
                gatherer = SideChannelGather(rd)        # the same gather over the TCP side channel (results staged through the host)

    def sync():     # the library's calls return after hipEventSynchronize / hipStreamSynchronize: the device is idle here
        if rd is not None:
            rd.barrier()

    state = dict(k=0)

    def step(closed_loop=False):
        if closed_loop:
            prob.advance()                          # next MPC step of the same scenarios: plant update + forecast shift, on device
            if not args.closed_loop_cold:
                prob.warm_start_from_previous(1)    # warm_start=True of the reference's solve(): the previous plan, moved on one step, as MIP start
            if os.environ.get("BENCH_CL_TRACE"):      # diagnostics: the inputs of the solve that follows, for a post-mortem replay
                xk_, wk_ = prob.inputs()
                np.savez("/tmp/cl_in.npz", x0=xk_, omega=wk_, midx=midx, step=-1)
        else:
            if cost_sets is not None:
                prob.set_cost(cost_sets[state["k"] % len(cost_sets)])      # this step's prices: mld_problem_set_cost (H2D of 64 x 575 weights + scaling, on the problem's stream)
            prob.select(state["k"] % n_sets)        # next scenario set: device-to-device copy
            state["k"] += 1
        st = prob.solve_resident()                  # K3 + K5/K6 on resident inputs, HIP-event timed inside
        if gatherer is not None:                    # the trivial result gather (RCCL over xGMI), from device buffers
            gatherer.gather_results(prob)
        return st

    def run_steps(count):
        if H == 1:
            return [step() for _ in range(count)]
        return run_pipelined(probs, count, state, n_sets, gatherer, cost_sets)

    progress("warm-up (%d) and timed steps (%d)" % (args.warmup, args.steps))
    run_steps(args.warmup)
    sync()
    t0 = time.perf_counter()
    stats_timed = run_steps(args.steps)
    sync()
    elapsed = time.perf_counter() - t0
    if rd is not None:
        elapsed = rd.all_max(elapsed)
    result = headline(args, world, n_local, elapsed, stats_timed, H, cost_sets is not None, gatherer)
    last = probs[(args.steps - 1) % H]      # the handle of the last timed step: its results and telemetry are still on the device
    if args.dump_outputs and rank == 0:
        progress("outputs of the last timed step to %s" % args.dump_outputs)
        dump_outputs(args.dump_outputs, last)
    if not args.full:
        result["config"].update(latency_ms(last.telemetry()), latency_measured_on="last timed step")
        if rank == 0:
            print(json.dumps(result), flush=True)
        if rd is not None:
            rd.close()
        return
    # continuity with rounds 1-3, whose timed steps all ran under the 05:00 tariff: two more pipelined steps with that one cost (outside `value`)
    value_fixed = None
    if cost_sets is not None and world == 1:
        for q in probs:
            q.set_cost(cost)
        keep_sets, cost_sets = cost_sets, None
        run_steps(1)
        sync()
        t0 = time.perf_counter()
        run_steps(2)
        sync()
        value_fixed = round(world * n_local * 2 / (time.perf_counter() - t0), 2)
        cost_sets = keep_sets
    # reference: the same kind of step strictly one after another on one handle (clean per-kernel timing for the roofline, latency telemetry)
    sync()
    t0 = time.perf_counter()
    stats = [step() for _ in range(max(1, args.reference_steps))]
    sync()
    elapsed_ref = time.perf_counter() - t0
    if rd is not None:
        elapsed_ref = rd.all_max(elapsed_ref)
    k_ref_last = (state["k"] - 1) % n_sets      # scenario set of the last reference step (single-instance leg)
    # ---- roofline of the dominant kernel (k_solve) on the LAST timed step: bytes its rank-1 dictionary updates streamed / its HIP-event time
    t0 = time.perf_counter()
    out = prob.download()
    download_ms = (time.perf_counter() - t0) * 1e3
    tel = prob.telemetry()
    kernel_ms = float(stats[-1]["solve_ms"])
    rows = int(tel["rows_updated"].sum())
    pivots = int(out["pivots"].sum())
    row_bytes = tel["row_bytes"]
    # bytes the simplex pivots stream: 64-byte sectors of the updated rows (read + write), the pivot row (read + write),
    # the cost row (read + write) and the multiplier column (one 64-byte sector per row: it is a strided gather)
    upd_bytes = 2.0 * rows * row_bytes + pivots * (2 * 8.0 * (prob.n + 1) + 2 * 8.0 * prob.n + 64.0 * prob.m)
    io_bytes = 8.0 * n_local * (prob.n + prob.m + d["nx"] + prob.nW)           # SURVEY 8d input/output minimum
    achieved = upd_bytes / (kernel_ms * 1e-3) / 1e9
    traffic, traffic_src = None, None
    for name in ("r04_pmc_solve.json", "r03_pmc_solve.json", "r02_pmc_solve.json", "r01_pmc_solve.json"):
        pmc = os.path.join(ROOT, "profiles", name)
        if os.path.exists(pmc):
            try:
                traffic = json.load(open(pmc)).get("hbm_bytes_per_launch")
                traffic_src = "profiles/%s (rocprofv3 --pmc FETCH_SIZE + WRITE_SIZE, separate passes; not measured in this run)" % name
            except Exception:
                traffic = None
            break
    # in-kernel phase clocks of the same step (thread 0 of every workgroup, summed over the instances): the share of the workgroup time spent in
    # the rank-1 dictionary updates -- the only phase that streams HBM -- and the rate of that phase alone
    import ctypes as C
    prof = (C.c_int64 * 8)()
    _lib.load().mld_debug_profile(prob._h, prof)
    ticks = np.array(list(prof)[:7], dtype=np.float64)
    share = float(ticks[0] / ticks.sum()) if ticks.sum() > 0 else None
    phase_names = ("rank1_update", "pivot_selection", "cut_separation", "leaf_checks", "bound_changes", "verification_refactor", "setup")
    status = out["status"]
    fin = np.isfinite(out["obj"])
    with np.errstate(invalid="ignore"):
        gap = np.where(fin, (out["obj"] - out["lower_bound"]) / np.maximum(1e-9, np.abs(out["obj"])), np.nan)
    lim = status == 2
    PATTERN = pattern_ceiling()
    result["config"].update(latency_ms(tel), latency_measured_on="last reference step")
    result["config"].update({
                   "status_last_step": {"optimal": int((status == 0).sum()), "infeasible": int((status == 1).sum()), "node_limit": int(lim.sum()),
                                        "numerical": int((status == 3).sum()), "unbounded": int((status == 4).sum())},
                   "no_incumbent": int((~fin).sum()),
                   "gap_of_limited": ({"median": round(float(np.nanmedian(gap[lim])), 5), "p90": round(float(np.nanpercentile(gap[lim], 90)), 5),
                                       "max": round(float(np.nanmax(gap[lim])), 5)} if lim.any() else None),
                   "nodes_per_instance": round(float(out["nodes"].mean()), 1), "pivots_per_instance": round(pivots / n_local, 1),
                   "pivots_per_s": round(pivots / (kernel_ms * 1e-3)), "rhs_ms": round(float(np.mean([s["rhs_ms"] for s in stats])), 3),
                   "kernel_ms_per_step_reference": [round(float(s["solve_ms"]), 1) for s in stats],
                   "download_ms": round(download_ms, 2)})
    result.update({
        "roofline": {"kernel": "k_solve", "bound": "hbm", "achieved": round(achieved, 2), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                     "frac": round(achieved / HBM_PEAK_GBS, 5), "traffic": traffic, "traffic_source": traffic_src,
                     "algorithmic_bytes_per_launch": int(upd_bytes), "bytes_per_instance": int(upd_bytes / n_local),
                     "io_minimum_bytes_per_launch": int(io_bytes), "algorithmic_over_io_minimum": round(upd_bytes / io_bytes, 1),
                     "traffic_over_io_minimum": (round(traffic / io_bytes, 1) if traffic else None),
                     "streaming_phase": (None if not share else {
                         "phase": "rank-1 dictionary update (s_pivot_inl): the phase that moves the counted bytes", "share_of_kernel_time": round(share, 4),
                         "achieved": round(achieved / share, 1), "unit": "GB/s", "frac_of_peak": round(achieved / share / HBM_PEAK_GBS, 4),
                         "frac_of_measured_copy_rate": round(achieved / share / 6300.0, 4),
                         "phases": {nm: round(float(t / ticks.sum()), 4) for nm, t in zip(phase_names, ticks)},
                         "note": "frac (above) divides the streamed bytes by the WHOLE kernel time; the other phases (row / column selection, cut separation, "
                                 "set-up, verification) stream nothing that is counted.  `achieved` here is the rate a workgroup reaches while it is inside the pivot "
                                 "routine, times the CUs -- NOT a rate the memory system sees: at any moment only this share of the workgroups is in that phase "
                                 "(see access_pattern for what the memory system delivers when all of them are).  6.3 TB/s is the copy rate the guide measures on "
                                 "this part (MI355X_MICROARCH.md)"}),
                     "access_pattern": {
                         "ceiling": PATTERN[0], "unit": "GB/s", "full_rows_ceiling": PATTERN[1], "source": PATTERN[2],
                         "what": "read-modify-write of 38 % of the 64-byte sectors of 107 scattered rows of a private fp64 matrix per iteration, with s_update_rows' lane "
                                 "layout and loads in flight, on every CU at once and nothing else (scripts/micro/sector_rmw.hip; the committed measurement named in `source`, "
                                 "first 675 MB line); full_rows_ceiling: the same with every sector active",
                         "traffic_rate": (round(traffic / (kernel_ms * 1e-3) / 1e9, 1) if traffic else None),
                         "frac": (round(traffic / (kernel_ms * 1e-3) / 1e9 / PATTERN[0], 4) if (traffic and PATTERN[0]) else None),
                         "note": "HBM bytes by PMC per launch / kernel time, against what the memory system delivers for this access pattern: the kernel keeps it at about "
                                 "two thirds of that ceiling ALL launch long although only a quarter of the workgroups are in the update loop at a time "
                                 "(profiles/r03_resident_workgroups.txt: a workgroup is 40 % slower with 256 resident than with 64) -- the shared memory system, "
                                 "not the latency of one CU, is the bound; two workgroups per CU buy nothing (DESIGN.md section 6)"},
                     "kernel_ms": round(kernel_ms, 3), "measured_on": "last reference step after the timed region (one launch at a time: HIP events around k_solve on "
                                                                    "the launch stream; in the timed region the launches overlap)"},
        "pipeline": {"handles": H, "value_one_at_a_time": round(world * n_local * len(stats) / elapsed_ref, 2), "ms_per_step_one_at_a_time": round(elapsed_ref / len(stats) * 1e3, 2),
                     "reference_steps": len(stats),
                     "value_no_idle_bound": round(world * n_local / (float(tel["latency_ns"].sum()) * 1e-9 / max(1, _lib.device_info()["n_cu"])), 2),
                     "note": "value: K timed steps alternating over the handles (mld_solve_launch / mld_solve_finish on per-problem HIP streams); value_one_at_a_time: "
                             "the following steps with mld_solve_resident on one handle -- the difference is the ragged end of a step (0.5-1.2 s node-limited "
                             "instances at random positions of the work queue) that the next step's workgroups fill; value_no_idle_bound: instances / (sum of the "
                             "in-kernel latencies of the last reference step / CUs), the rate of a device that never waits for a straggler"},
    })
    # K3 on the matrix cores: one [m0 x (nx + N nw)] . [(nx + N nw) x instances-of-the-model] GEMM per model
    rhs_ms = float(np.mean([s["rhs_ms"] for s in stats]))
    flops = 2.0 * prob.m * (d["nx"] + prob.nW) * n_local
    result["mfma"] = {"kernel": "k_rhs_mfma (v_mfma_f64_16x16x4_f64)", "dtype": "f64", "flops_per_launch": int(flops), "ms": round(rhs_ms, 4),
                      "tflops": round(flops / (rhs_ms * 1e-3) / 1e12, 3), "peak_tflops": 78.6,
                      "frac_of_peak": round(flops / (rhs_ms * 1e-3) / 1e12 / 78.6, 5),
                      "note": "fp64 matrix peak 78.6 TFLOP/s is AMD's MI355X figure (the guide lists 157.3 TFLOP/s for fp32 MFMA only); the launch moves "
                              "%d MB of H + inputs + outputs, so it is bound by HBM / L2, not by the matrix cores" % int((64 * prob.m * (d["nx"] + prob.nW) * 8 + io_bytes) / 1e6),
                      "condensing": "K1 + K2 carry NO matrix-core work: the block products of the condensing have inner dimension nx = %d (<= 15 on every BASELINE shape), so a "
                                    "16x16x4 MFMA tile would be > 75 %% padding for %.2f MFLOP per model against %.2f MB written -- the kernels are priced as the HBM write "
                                    "stream they are (roofline_condense); the fp32 variant of configs[4] rounds the fp64 block arithmetic once on its way to HBM "
                                    "(mld_condense_f32)" % (d["nx"], 2e-6 * N_t * (d["nx"] ** 2 * model.nv + d["nc"] * d["nx"] * model.nv), 8e-6 * N_t * (d["nc"] + d["nx"] + d["ny"]) * (N_t * model.nv + d["nx"] + N_t * d["nomega"] + 1))}
    # the single-stream rate a closed-loop user gets (step k+1 of the SAME microgrids needs step k): beside `value` at top level
    result["value_one_at_a_time"] = result["pipeline"]["value_one_at_a_time"]
    if exact is not None:
        result["value_exact"] = exact["value_exact"]
        result["exact"] = exact
    if hand1 is not None:
        result["handoff"] = hand1
    # work queue: the SAME scenario set as the last reference step, once more in plain instance order (opts.reserved bit 3) -- identical
    # instances, so the two kernel times differ by the queue order alone
    prob.set_opts(reserved=8 | args.reserved)
    state["k"] -= 1
    sync()
    t0 = time.perf_counter()
    st_nl = step()
    sync()
    t_nl = time.perf_counter() - t0
    if rd is not None:
        t_nl = rd.all_max(t_nl)
    prob.set_opts(reserved=args.reserved)
    result["work_queue"] = {"kernel_ms_learnt": round(kernel_ms, 1), "kernel_ms_fifo": round(float(st_nl["solve_ms"]), 1),
                            "learnt_over_fifo": round(float(st_nl["solve_ms"]) / kernel_ms, 4),
                            "note": "the last reference step's scenario set solved twice, one launch at a time: with the longest-first order learnt from the previous step "
                                    "(other scenarios of the same agents: agent-level information only) and in plain instance order; learnt_over_fifo > 1 = the learnt order is faster"}
    if cost_sets is not None:
        prob.set_cost(cost)         # the legs below use the cost every fixture was generated with
    if args.closed_loop_steps > 0:
        # closed loop: the SAME scenarios advanced step by step (plant update with the inputs just computed, forecast shifted)
        rates, prov = [], []
        progress("closed loop: %d steps" % args.closed_loop_steps)
        cl_trace = os.environ.get("BENCH_CL_TRACE")       # diagnostics: post-mortem trace of the solver's workgroups + the inputs of every closed-loop step
        if cl_trace:
            prob.debug_trace(os.path.join(cl_trace, "cl_trace.bin"))
        for k_cl in range(args.closed_loop_steps):
            if cl_trace:
                progress("closed loop step %d" % k_cl)
            sync()
            t0 = time.perf_counter()
            st_c = step(closed_loop=True)
            sync()
            t_c = time.perf_counter() - t0
            if rd is not None:
                t_c = rd.all_max(t_c)
            rates.append(round(world * n_local / t_c, 1))
            prov.append(round(st_c["n_optimal"] / n_local, 4))
        last_handoff = None
        if world == 1:      # the last step's inputs once more with sub-tree hand-off: what the steady state costs when its tail has to be proven too
            xk, wk = prob.inputs()
            hand = dict(first_nodes=args.node_limit, sub_nodes=max(50, args.node_limit // 2), max_gen=4, max_children=64, max_tree=64, room_factor=2.0)
            t0 = time.perf_counter()
            oh = prob.solve_handoff_device(xk, wk, midx, **hand)
            t_h = time.perf_counter() - t0
            last_handoff = dict(hand, value=round(n_local / t_h, 1), proven_fraction=round(float((oh["status"] == 0).mean()), 4), queue=oh["handoff"])
        result["closed_loop"] = {"steps": args.closed_loop_steps, "value_per_step": rates, "proven_per_step": prov, "last_step_with_handoff": last_handoff,
                                 "value_last_step": rates[-1], "proven_last_step": prov[-1], "mip_start": not args.closed_loop_cold,
                                 "note": "mld_advance_batch between solves (reference: sim_step_k -> lsim_k)%s; the population drifts out of the seeded regime "
                                         "(x0 in 55..64: most tanks need no heating inside the horizon) towards its steady state and the instances get harder "
                                         "(DESIGN section 6)" % ("" if args.closed_loop_cold else ", the previous plan moved on one step as MIP start "
                                         "(mld_warm_start_from_previous: warm_start=True of controller_base.py:493,509-512)")}
    if rank == 0 and world == 1 and not args.no_extra_legs:
        xs_l, ws_l = (x0, om) if k_ref_last == 0 else step_scenarios(rank, k_ref_last, n_local)
        base_opts = dict(gap_rel=args.mip_gap, max_nodes=args.node_limit, max_pivots=args.pivot_limit)
        for q in probs[1:]:
            q.close()
        progress("single-instance leg")
        result["single_instance"] = single_instance_leg(agents, N_p, N_t, xs_l, ws_l, midx, tel["latency_ns"], base_opts)
        prob.close()
        progress("MIQP leg (cfg3 shape, Q_x = 1e-3 I)")
        result["miqp"] = miqp_leg()
        progress("cfg5 leg (128 golden instances, fp32 condensing at the shape)")
        result["cfg5"] = cfg5_leg()
    # the driver keeps `config` whole (of other top-level keys only the names): the legs' headline numbers are repeated there
    cfgd = result["config"]
    cfgd["value_one_at_a_time"] = result["value_one_at_a_time"]
    if exact is not None:
        cfgd["value_exact"] = exact["value_exact"]
        cfgd["exact_proven_fraction"] = exact["proven_fraction"]
        cfgd["exact_worst_rel_above_optimum"] = exact.get("worst_rel_above_optimum_all")
    if "closed_loop" in result:
        cfgd["closed_loop_value_last_step"] = result["closed_loop"]["value_last_step"]
        cfgd["closed_loop_proven_last_step"] = result["closed_loop"]["proven_last_step"]
        cfgd["closed_loop_steps"] = result["closed_loop"]["steps"]
    for leg in ("single_instance", "miqp", "cfg5"):
        if result.get(leg) is not None:
            cfgd[leg] = result[leg]
    if value_fixed is not None:
        cfgd["value_fixed_cost"] = value_fixed
        cfgd["value_fixed_cost_note"] = ("two pipelined steps under the 05:00 tariff of every earlier round's timed region (same scenario distribution): with the clock moving, "
                                         "later steps see the morning peak earlier in their horizon and cost more pivots per instance (pivots_per_instance)")
    if rank == 0:
        # secondary roofline: condensing K1+K2 (SURVEY 8d formula: outputs + inputs), 64 models per launch
        ms = min(model.condense_device(N_t) for _ in range(5))
        nx, ny, nc, nw, nv = d["nx"], d["ny"], d["nc"], d["nomega"], model.nv
        cols = N_t * nv + nx + N_t * nw + 1
        bytes_cond = 8.0 * (N_t * (nc + nx + ny) * cols + (nx + ny + nc) * (nx + nv + nw + 1) + nc * ny)
        ach = args.agents * bytes_cond / (ms * 1e-3) / 1e9
        result["roofline_condense"] = {"kernel": "k_condense_model+k_condense_flat", "bound": "hbm", "achieved": round(ach, 1),
                                       "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(ach / HBM_PEAK_GBS, 4),
                                       "bytes_per_model": int(bytes_cond), "models": args.agents, "kernel_ms": round(ms, 4)}
        ms32 = min(model.condense_device(N_t, f32=True) for _ in range(5))      # fp32 materialisation (mld_condense_f32): half the output bytes
        bytes32 = 4.0 * N_t * (nc + nx + ny) * cols + 8.0 * ((nx + ny + nc) * (nx + nv + nw + 1) + nc * ny)
        result["roofline_condense_f32"] = {"kernel": "k_condense_model+k_condense_flat<float>", "bound": "hbm", "achieved": round(args.agents * bytes32 / (ms32 * 1e-3) / 1e9, 1),
                                           "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(args.agents * bytes32 / (ms32 * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
                                           "bytes_per_model": int(bytes32), "models": args.agents, "kernel_ms": round(ms32, 4),
                                           "speedup_vs_fp64_output": round(ms / ms32, 3)}
        try:        # HBM bytes of the two condensing launches from the same PMC passes (FETCH + WRITE, per launch of each kernel)
            allc = json.load(open(pmc)).get("all", {})
            # (kernel names in the PMC summary are demangled signatures, e.g. "void k_condense_flat<double>(...)": match by substring)
            kb = sum(v.get("kb_per_launch", 0.0) for c in ("FETCH_SIZE", "WRITE_SIZE") for k, v in allc.get(c, {}).items()
                     if ("k_condense_model" in k or "k_condense_flat<double>" in k or k.strip() == "k_condense_flat"))
            result["roofline_condense"]["traffic"] = kb * 1024.0 if kb > 0 else None
        except Exception:
            result["roofline_condense"]["traffic"] = None
        result["cpu_baseline"] = cpu            # (measured before the GPU part, see main())
        print(json.dumps(result), flush=True)
    if rd is not None:
        rd.close()


if __name__ == "__main__":
    main()
