"""Vector loads outstanding before each `s_waitcnt vmcnt(N)` of a gfx9 assembly listing, per function.

    hipcc --offload-arch=gfx950 -O3 -std=c++17 --cuda-device-only -S -o mldgpu.s pyhybridcontrol_amd/csrc/mldgpu.hip
    python scripts/asm_loads_in_flight.py mldgpu.s s_check_residual s_presolve s_refactor s_leaf_eval s_mir_round k_solve

A function is named by a substring of its (mangled) symbol.  The listing is walked in program order: every global_load / flat_load / buffer_load
adds one to the count (spill reloads, scratch_load, are left out), a wait for vmcnt(N) reports the count before it and leaves min(count, N).  Branches
are not followed and stores are not counted, so a figure is what the straight-line code around a wait keeps in flight -- a report to read beside the
source, not a test.  Per function: the number of waits, how many of them had 1, 2-3, 4-7, 8-15, 16-31 or 32 and more loads outstanding, and the
largest count.  Code that the compiler inlined is reported under the function it was inlined into.
"""
import re
import sys

LOAD = re.compile(r"^\s+(global_load|flat_load|buffer_load)\w*\s")
WAIT = re.compile(r"^\s+s_waitcnt\b.*\bvmcnt\((\d+)\)")
FUNC = re.compile(r"^([A-Za-z_][\w$.]*):\s*(;.*)?$")
END = re.compile(r"^\s+\.size\s+([\w$.]+),")
BUCKETS = ((1, 1), (2, 3), (4, 7), (8, 15), (16, 31), (32, 1 << 30))


def scan(path, names):
    out = {}
    cur, fly, waits = None, 0, None
    with open(path) as f:
        for line in f:
            if cur is None:
                m = FUNC.match(line)
                if m and not m.group(1).startswith("."):
                    hit = [n for n in names if n in m.group(1)]
                    if hit:
                        cur, fly, waits = m.group(1), 0, []
                continue
            m = END.match(line)
            if m and m.group(1) == cur:
                out[cur] = waits
                cur = None
                continue
            if LOAD.match(line):
                fly += 1
                continue
            m = WAIT.match(line)
            if m:
                if fly > 0:
                    waits.append(fly)
                fly = min(fly, int(m.group(1)))
    return out


def main(argv):
    if len(argv) < 3:
        print(__doc__)
        return 2
    res = scan(argv[1], argv[2:])
    print("%-58s %6s | %s | %4s" % ("function", "waits", " ".join("%6s" % ("%d" % lo if lo == hi else ("%d+" % lo if hi > 1000 else "%d-%d" % (lo, hi))) for lo, hi in BUCKETS), "max"))
    for name in sorted(res):
        w = res[name]
        hist = [sum(1 for v in w if lo <= v <= hi) for lo, hi in BUCKETS]
        print("%-58s %6d | %s | %4d" % (name[:58], len(w), " ".join("%6d" % h for h in hist), max(w) if w else 0))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
