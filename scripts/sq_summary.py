"""Summarise the SQ counter passes of scripts/collect_profiles_r4.sh for k_solve into profiles/<tag>_sq_solve.json.
usage: python scripts/sq_summary.py <out.json> [--pivots=N] [--command=TEXT] <pass_dir> [<pass_dir> ...]

With the instruction-cache passes (SQC_ICACHE_REQ / _HITS / _MISSES / _MISSES_DUPLICATE and SQ_IFETCH / SQ_IFETCH_LEVEL beside SQ_WAIT_INST_ANY / SQ_WAVE_CYCLES)
the derived block also holds the hit rate, the mean fetch latency over ALL fetches, hits included (SQ_IFETCH_LEVEL / SQ_IFETCH: the level counter adds the
fetches in flight every cycle) and the fetches in flight as a share of the wave cycles -- an upper bound on what instruction fetch can cost, if both counters
tick in the same unit; --pivots=N (dual-simplex pivots of one launch) adds the misses per pivot."""
import csv, glob, json, os, sys
args = [a for a in sys.argv[2:] if not a.startswith("--")]
opt = dict(a[2:].split("=", 1) for a in sys.argv[2:] if a.startswith("--") and "=" in a)
out = {}
for d in args:
    for f in glob.glob(os.path.join(d, "**", "*_counter_collection.csv"), recursive=True):
        for row in csv.DictReader(open(f)):
            if not row["Kernel_Name"].startswith("k_solve"):
                continue
            e = out.setdefault(row["Counter_Name"], {"launches": set(), "sum": 0.0})
            e["launches"].add(row["Dispatch_Id"]); e["sum"] += float(row["Counter_Value"])
doc = {k: {"launches": len(v["launches"]), "per_launch": v["sum"] / max(1, len(v["launches"]))} for k, v in sorted(out.items())}
g = lambda k: doc.get(k, {}).get("per_launch", 0.0)
der = {}
if g("SQ_WAVE_CYCLES"):
    for name, num in (("wave_parked_share", "SQ_WAIT_ANY"), ("issue_stall_share", "SQ_WAIT_INST_ANY"), ("issuing_share", "SQ_ACTIVE_INST_ANY")):
        if num in doc:      # (a share only where its numerator was collected in these passes)
            der["%s (%s / SQ_WAVE_CYCLES)" % (name, num)] = g(num) / g("SQ_WAVE_CYCLES")
if g("SQ_LDS_IDX_ACTIVE"):
    der["lds_bank_conflict_share (SQ_LDS_BANK_CONFLICT / SQ_LDS_IDX_ACTIVE)"] = g("SQ_LDS_BANK_CONFLICT") / g("SQ_LDS_IDX_ACTIVE")
if g("SQ_INSTS_FLAT"):
    der["flat_share_of_memory_instructions"] = g("SQ_INSTS_FLAT") / max(1.0, g("SQ_INSTS_FLAT") + g("SQ_INSTS_LDS"))
if g("SQC_ICACHE_REQ"):
    der["icache_hit_rate (SQC_ICACHE_HITS / SQC_ICACHE_REQ)"] = g("SQC_ICACHE_HITS") / g("SQC_ICACHE_REQ")
    der["icache_miss_rate ((SQC_ICACHE_MISSES + SQC_ICACHE_MISSES_DUPLICATE) / SQC_ICACHE_REQ)"] = (g("SQC_ICACHE_MISSES") + g("SQC_ICACHE_MISSES_DUPLICATE")) / g("SQC_ICACHE_REQ")
    if "pivots" in opt:
        der["pivots_per_launch"] = float(opt["pivots"])
        der["icache_requests_per_pivot"] = g("SQC_ICACHE_REQ") / float(opt["pivots"])
        der["icache_misses_per_pivot (without duplicates)"] = g("SQC_ICACHE_MISSES") / float(opt["pivots"])
        der["icache_duplicate_misses_per_pivot"] = g("SQC_ICACHE_MISSES_DUPLICATE") / float(opt["pivots"])
if g("SQ_IFETCH"):
    lat = g("SQ_IFETCH_LEVEL") / g("SQ_IFETCH")
    der["mean_fetch_latency_cycles (SQ_IFETCH_LEVEL / SQ_IFETCH)"] = lat
    if "pivots" in opt:
        der["wave_fetches_per_pivot (SQ_IFETCH)"] = g("SQ_IFETCH") / float(opt["pivots"])
    if g("SQ_WAVE_CYCLES"):
        der["fetch_in_flight_share (SQ_IFETCH_LEVEL / SQ_WAVE_CYCLES)"] = g("SQ_IFETCH_LEVEL") / g("SQ_WAVE_CYCLES")
cmd = opt.get("command", "rocprofv3 --pmc <8 SQ counters per pass> -- python3 bench.py --full --steps 2 --warmup 1 --no-cpu --exact-sample 0 --handles 1 --closed-loop-steps 0 --no-extra-legs")
json.dump({"kernel": "k_solve", "command": cmd,
           "counters_per_launch": doc, "derived": der,
           "units": "SQ_WAVE_CYCLES / SQ_WAIT_* / SQ_ACTIVE_INST_* count quad-cycles summed over waves (MI355X_MICROARCH.md); instruction counters count wave instructions"}, open(sys.argv[1], "w"), indent=1)
print(json.dumps(der, indent=1))
