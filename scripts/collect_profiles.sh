#!/bin/bash
# Run on the GPU box: kernel-trace stats and the two PMC passes for the default bench workload (the --full run: its reference steps and
# roofline are what the profiles are about).  scripts/collect_profiles.sh [OUT=prof_out]; copy the summaries into profiles/ afterwards
# (scripts/pmc_summary.py).
set -e
export TMPDIR=/tmp
R=${GRAFT_REPO_ROOT:-$(pwd)}
cd "$R"
CMD="bench.py --full --steps 2 --warmup 1 --no-cpu --exact-sample 0 --handles 1 --closed-loop-steps 0"
mkdir -p "${1:-prof_out}"
OUT=$(cd "${1:-prof_out}" && pwd)
rm -rf "$OUT/prof_stats" "$OUT/pmc_fetch" "$OUT/pmc_write"
rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/prof_stats" -- python3 $CMD > "$OUT/prof_stats.log" 2>&1
tail -1 "$OUT/prof_stats.log" | cut -c1-400
rocprofv3 --pmc FETCH_SIZE --output-format csv -d "$OUT/pmc_fetch" -- python3 $CMD > "$OUT/pmc_fetch.log" 2>&1
rocprofv3 --pmc WRITE_SIZE --output-format csv -d "$OUT/pmc_write" -- python3 $CMD > "$OUT/pmc_write.log" 2>&1
echo profiles collected
