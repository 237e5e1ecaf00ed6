"""Phase clocks of k_solve on the bench shard, for the work around the pivot loop ("Work nobody reads"): scenario set 0 under the
05:00 tariff, comparable with profiles/walks_*.txt, and set 5 under its own tariff, the first timed set of `bench.py --warmup 5`; two launches each, so
that the spread of a clock between two launches is on record.

    python scripts/gpu_dead_work_prof.py TAG [reserved]                               # the normal build: prof[0..6] summed over the instances
    MLDGPU_LIB=<-DMLD_PIVOT_PROF=2 build> python scripts/gpu_dead_work_prof.py TAG    # the long-step loop: ticks, pivots, groups examined and passed

The diagnostic build is recognised by "pivprof" in the library's file name, e.g.
    MLD_OUT=$PWD/libmldgpu_pivprof2.so MLD_CXXFLAGS=-DMLD_PIVOT_PROF=2 python -m pyhybridcontrol_amd.build --force
reserved: mld_opts.reserved of the solve (1 << 29 = MLD_DBG_DEAD_WORK_R8, the bound changes' earlier walk over every row, on the same binary).  The table goes
to stdout and to prof_out/dead_work_TAG.txt."""
import os
import ctypes as C
import datetime as dt
import sys

import numpy as np

sys.path.insert(0, ".")
import bench
from pyhybridcontrol_amd import gpu, host, _lib, synthetic as syn

tag = sys.argv[1]
reserved = int(sys.argv[2], 0) if len(sys.argv) > 2 else 0
pivprof = "pivprof" in _lib.LIB_PATH
agents, N_p, N_t, x0, om, midx = bench.make_shard(64, 512, 0)
d = agents[0]["dims"]
model = gpu.GpuModel([a["mats"] for a in agents], d)
cost0 = host.stack_costs([host.cost_from_atoms(a["atoms"], d, N_p, N_t) for a in agents])
prob = gpu.GpuProblem(model, N_p, N_t, cost0, gap_rel=1e-2, max_nodes=800, max_pivots=40000, reserved=reserved)
names = ("pivot_update", "simplex_select", "cuts", "leaf", "set_bounds", "residual/refactor", "setup")
pnames = ("single pivots", "pairs", "long-step ticks", "long-step pivots", "groups examined", "groups passed", "pivots with flips", "-")
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def launch(label):
    st = prob.solve_resident()
    out = (C.c_int64 * 8)()
    _lib.load().mld_debug_profile(prob._h, out)
    ticks = np.array(list(out), dtype=float)
    tel = prob.telemetry()
    lat = tel["latency_ns"].sum()
    status = np.bincount(prob.download()["status"].astype(np.int64)).tolist()
    say("%s | %s | lib %s reserved 0x%x: solve_ms %.1f pivots %d nodes %d cuts %d refactors %d; workgroup latency sum %.3f s status %s" % (
        tag, label, _lib.LIB_PATH.split("/")[-1], reserved, st["solve_ms"], st["pivots"], st["nodes"], st["cuts"], st["refactors"], lat * 1e-9, status))
    wg = lat * 0.1
    if pivprof:
        for k, nm in enumerate(pnames):
            say("    %-18s %16.0f" % (nm, ticks[k]))
        say("    long-step loop: %.4f of workgroup time, %.3f us per long-step pivot, %.3f groups per pivot" % (
            ticks[2] / wg, ticks[2] * 0.01 / max(ticks[3], 1), ticks[4] / max(ticks[3], 1)))
    else:
        tot = ticks[:7].sum()
        for k, nm in enumerate(names):
            say("    %-18s %14.0f ticks  %7.4f of the clocks' sum  %7.4f of workgroup time" % (nm, ticks[k], ticks[k] / tot, ticks[k] / wg))


prob.upload(x0, om, midx)
prob.solve_resident()          # warm-up launch
launch("set 0 launch 1")
launch("set 0 launch 2")
t0 = dt.datetime(2018, 12, 10, 5, 0) + dt.timedelta(seconds=syn.TS * 5)
cost5 = host.stack_costs([host.cost_from_atoms(syn.make_cost(syn.CONFIGS["cfg4"]["n_h"], N_t, a["params"], t0=t0), d, N_p, N_t) for a in agents])
x5, o5 = bench.step_scenarios(0, 5, x0.shape[0])
prob.set_cost(cost5)
prob.upload(x5, o5, midx)
launch("set 5 launch 1")
launch("set 5 launch 2")
prob.close()
model.close()
os.makedirs("prof_out", exist_ok=True)
with open("prof_out/dead_work_%s.txt" % tag, "w") as f:
    f.write("\n".join(lines) + "\n")
