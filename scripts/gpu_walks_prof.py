"""Per-phase clocks of one k_solve launch of the bench shard, for the phases outside the pivot loop ("Loads in flight outside the pivot loop").

    python scripts/gpu_walks_prof.py [n_scen] [reserved]                      # the normal build: prof[0..6] summed over the instances
    MLDGPU_LIB=<-DMLD_CUT_PROF=3 build> python scripts/gpu_walks_prof.py ...  # phase A of the c-MIR round split into its four sub-clocks

The diagnostic build is recognised by "cutprof" in the library's file name, e.g.
    MLD_OUT=$PWD/libmldgpu_cutprof3.so MLD_CXXFLAGS=-DMLD_CUT_PROF=3 python -m pyhybridcontrol_amd.build --force
reserved: mld_opts.reserved of the solve (1 << 24 = MLD_DBG_WALKS_SERIAL, the one-load-at-a-time walks on the same binary).
"""
import ctypes as C
import sys

import numpy as np

sys.path.insert(0, ".")
import bench
from pyhybridcontrol_amd import gpu, host, _lib

n_scen = int(sys.argv[1]) if len(sys.argv) > 1 else 512
reserved = int(sys.argv[2], 0) if len(sys.argv) > 2 else 0
cut_prof = "cutprof" in _lib.LIB_PATH
agents, N_p, N_t, x0, om, midx = bench.make_shard(64, n_scen, 0)
d = agents[0]["dims"]
model = gpu.GpuModel([a["mats"] for a in agents], d)
prob = gpu.GpuProblem(model, N_p, N_t, host.stack_costs([host.cost_from_atoms(a["atoms"], d, N_p, N_t) for a in agents]), gap_rel=1e-2, max_nodes=800, max_pivots=40000,
                      reserved=reserved)
prob.upload(x0, om, midx)
st = prob.solve_resident()
st = prob.solve_resident()
out = (C.c_int64 * 8)()
_lib.load().mld_debug_profile(prob._h, out)
ticks = np.array(list(out), dtype=float)
lat = prob.telemetry()["latency_ns"].sum()
print("lib %s reserved 0x%x: solve_ms %.1f pivots %d nodes %d cuts %d refactors %d instances %d; sum of workgroup latency %.3f s" % (
    _lib.LIB_PATH.split("/")[-1], reserved, st["solve_ms"], st["pivots"], st["nodes"], st["cuts"], st["refactors"], x0.shape[0], lat * 1e-9))
if cut_prof:
    names = ("A: x gather + fractional list", "A: screen", "A: pass 1 + wave sums (wave 0)", "A: divisor loop (wave 0)", "phase A (c-MIR scoring)", "cut separation")
    wg = lat * 0.1      # wall_clock64 ticks (100 MHz) of the summed workgroup latency
    for k, nm in enumerate(names):
        print("%-34s %14.0f ticks  %6.3f of phase A  %7.4f of workgroup time" % (nm, ticks[k], ticks[k] / max(ticks[4], 1.0), ticks[k] / wg))
else:
    names = ("pivot_update", "simplex_select", "cuts", "leaf", "set_bounds", "residual/refactor", "setup")
    tot = ticks[:7].sum()
    for k, nm in enumerate(names):
        print("%-18s %14.0f ticks  %7.4f of workgroup time" % (nm, ticks[k], ticks[k] / tot))
prob.close()
model.close()
