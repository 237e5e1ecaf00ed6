"""Sub-phase timing of k_solve's dual-simplex pivot on one launch of the bench shard, on the diagnostic builds of the library:

    MLD_OUT=pyhybridcontrol_amd/libmldgpu_pprof2.so MLD_CXXFLAGS=-DMLD_PIVOT_PROF=2 python -m pyhybridcontrol_amd.build --force
    MLD_OUT=pyhybridcontrol_amd/libmldgpu_pprof1.so MLD_CXXFLAGS=-DMLD_PIVOT_PROF=1 python -m pyhybridcontrol_amd.build --force
    MLDGPU_LIB=pyhybridcontrol_amd/libmldgpu_pprof2.so python scripts/gpu_pivot_prof.py counts [n_scen=512] [counts.json]
    MLDGPU_LIB=pyhybridcontrol_amd/libmldgpu_pprof1.so python scripts/gpu_pivot_prof.py clocks [n_scen=512] [counts.json]
    MLD_OUT=pyhybridcontrol_amd/libmldgpu_pprof3.so MLD_CXXFLAGS=-DMLD_PIVOT_PROF=3 python -m pyhybridcontrol_amd.build --force
    MLD_OUT=pyhybridcontrol_amd/libmldgpu_pprof4.so MLD_CXXFLAGS=-DMLD_PIVOT_PROF=4 python -m pyhybridcontrol_amd.build --force
    MLDGPU_LIB=pyhybridcontrol_amd/libmldgpu_pprof3.so python scripts/gpu_pivot_prof.py select [n_scen=512]
    MLDGPU_LIB=pyhybridcontrol_amd/libmldgpu_pprof4.so python scripts/gpu_pivot_prof.py lookahead [n_scen=512]

`counts` (-DMLD_PIVOT_PROF=2): single pivots, pairs, long-step pivots with the groups they examined and passed, pivots with flips, and the clock of
the long-step loop; written to counts.json too.  `clocks` (-DMLD_PIVOT_PROF=1): thread 0's clock over the first half (for a pair: both first halves
and the look-ahead), the sector list, the row list and the update loop, for single pivots and for pairs apart -- per pivot where counts.json of the
same launch exists (the solver is deterministic: the counts of the two builds are the same), and as a share of the workgroups' time.  Each
configuration is solved twice and the second launch is reported: the barrier sequence before it was halved (opts.reserved bit 26) and the present
one, each with pivot pairs and without (bit 21).  On the one-exchange path of the lists the "sector list" is the flags of both lists and their
exchange, the "row list" the scatter of both.

`select` (-DMLD_PIVOT_PROF=3) and `lookahead` (=4): thread 0's clock over the parts of the choice of (row, column) -- in the loop of the dual simplex: the
loop top, the pricing scan with its arg-max, the row load with pass 1 and emax, pass 2 with tmax, pass 3 with its arg-max (plain pivots); in the pair's
look-ahead the same four parts without the loop top -- with the selection as it was (opts.reserved bit 27) and the present one, as a share of the
workgroups' time.  The selection clock of the launch (mld_debug_profile slot 1 of the product build) is printed beside them; it holds the loop's
selection and everything in the loop that has no clock of its own, not the look-ahead (that is inside the pivot's clock)."""
import json, os, sys, ctypes as C, numpy as np
sys.path.insert(0, '.')
import bench
from pyhybridcontrol_amd import gpu, host, _lib

mode = sys.argv[1] if len(sys.argv) > 1 else "clocks"
n_scen = int(sys.argv[2]) if len(sys.argv) > 2 else 512
cfile = sys.argv[3] if len(sys.argv) > 3 else "prof_out/pivot_prof_counts.json"      # (prof_out/: the profiler output folder, kept out of git)
SYNC_R5, NO_PAIRS, SELECT_R6 = 1 << 26, 1 << 21, 1 << 27
TICK = 1e-8      # wall_clock64: 100 MHz
agents, N_p, N_t, x0, om, midx = bench.make_shard(64, n_scen, 0)
d = agents[0]['dims']
model = gpu.GpuModel([a['mats'] for a in agents], d)
prob = gpu.GpuProblem(model, N_p, N_t, host.stack_costs([host.cost_from_atoms(a['atoms'], d, N_p, N_t) for a in agents]), gap_rel=1e-2, max_nodes=800, max_pivots=40000)
print("library", _lib.LIB_PATH, "mode", mode, "instances", x0.shape[0])
counts = json.load(open(cfile)) if mode == "clocks" and os.path.exists(cfile) else {}
CONFIGS = (("barriers as before, pairs", SYNC_R5), ("halved barriers, pairs", 0), ("barriers as before, single pivots", SYNC_R5 | NO_PAIRS), ("halved barriers, single pivots", NO_PAIRS))
if mode in ("select", "lookahead"):
    CONFIGS = (("selection as before", SELECT_R6), ("selection now", 0))
PARTS = ("loop top", "pricing scan + arg-max", "row load + pass 1 + emax", "pass 2 + tmax", "pass 3 + arg-max")
for tag, reserved in CONFIGS:
    prob.set_opts(reserved=reserved)
    prob.upload(x0, om, midx); st = prob.solve_resident(); st = prob.solve_resident()
    out = (C.c_int64 * 8)(); _lib.load().mld_debug_profile(prob._h, out)
    t = np.array(list(out), dtype=float)
    wg = prob.telemetry()["latency_ns"].sum() * 1e-9      # seconds the workgroups spent on instances
    print("== %s (reserved %d): solve_ms %.1f  pivots %d  workgroup time %.3f s" % (tag, reserved, st['solve_ms'], st['pivots'], wg))
    if mode in ("select", "lookahead"):
        names = PARTS if mode == "select" else PARTS[1:]
        for name, v in zip(names, t[:len(names)] * TICK):
            print("   %-10s %-26s %8.3f s  %5.2f %% of the workgroup time  %6.2f us per pivot" % ("loop" if mode == "select" else "look-ahead", name, v, 100.0 * v / wg, 1e6 * v / max(1, st['pivots'])))
        tot = t[:len(names)].sum() * TICK
        print("   %-10s %-26s %8.3f s  %5.2f %% of the workgroup time" % ("", "sum of the parts", tot, 100.0 * tot / wg))
        print("   %-10s %-26s %8.3f s  %5.2f %% of the workgroup time" % ("", "selection clock", t[7] * TICK, 100.0 * t[7] * TICK / wg))
    elif mode == "counts":
        c = dict(single=int(t[0]), pairs=int(t[1]), long_step_s=t[2] * TICK, long_step_pivots=int(t[3]), groups_examined=int(t[4]), groups_passed=int(t[5]), pivots_with_flips=int(t[6]))
        counts[str(reserved)] = c
        print("   single pivots %d, pairs %d (2 pivots each): %d of %d pivots" % (c["single"], c["pairs"], c["single"] + 2 * c["pairs"], st['pivots']))
        print("   long-step pivots %d (%.1f %% of all), groups examined %d, passed %d, pivots with flips %d" % (
            c["long_step_pivots"], 100.0 * c["long_step_pivots"] / max(1, st['pivots']), c["groups_examined"], c["groups_passed"], c["pivots_with_flips"]))
        print("   long-step loop %.3f s = %.2f %% of the workgroup time, %.2f us per long-step pivot" % (
            c["long_step_s"], 100.0 * c["long_step_s"] / wg, 1e6 * c["long_step_s"] / max(1, c["long_step_pivots"])))
    else:
        c = counts.get(str(reserved))
        for kind, o, per in (("single pivot", 0, c["single"] if c else 0), ("pair", 4, c["pairs"] if c else 0)):
            for name, v in zip(("first half", "sector list", "row list", "update loop"), t[o:o + 4] * TICK):
                print("   %-12s %-12s %8.3f s  %5.2f %% of the workgroup time%s" % (kind, name, v, 100.0 * v / wg, "  %6.2f us each" % (1e6 * v / per) if per else ""))
if mode == "counts":
    os.makedirs(os.path.dirname(cfile) or ".", exist_ok=True)
    json.dump(counts, open(cfile, "w"))
