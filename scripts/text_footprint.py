"""Bytes of device text per function, and of one function per source region, for the product build of libmldgpu.

    python scripts/text_footprint.py [--function SUBSTRING] [--out FILE] [--keep DIR]

The device code is compiled with the flags of pyhybridcontrol_amd/build.py plus `-gline-tables-only --cuda-device-only -c` (line tables do not change
the code), the gfx950 code object is taken out of the bundle, `llvm-readelf -sW` gives the size of every function and `llvm-objdump -d -l` the source
line of every instruction of the named function (default: the bench's loop, s_dual_simplex_impl<true, false, false>).  An instruction's bytes go to
the region its line falls into: the body of one of the device functions of problem.inc listed in REGIONS (inlined code keeps the line of the function
it was written in), the rest of problem.inc, or another file (HIP headers).  The report holds bytes only -- per function, per region, and per 4 KiB
window of the function's text which regions fill it (so that one can see whether the code of a plain pivot lies together) -- no opcodes.
"""
import argparse
import collections
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "pyhybridcontrol_amd", "csrc", "mldgpu.hip")
INC = os.path.join(ROOT, "pyhybridcontrol_amd", "csrc", "problem.inc")
LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/llvm/bin")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fno-gpu-rdc", "-Wno-unused-result"]      # (build.py's, without the link)
REGIONS = ("s_update_rows2_r7", "s_upd2_unit", "s_update_rows_r7", "s_update_rows2", "s_update_rows", "s_group_holds", "s_ld16", "s_st16", "s_uni_ptr", "s_pair_update", "s_pivot_pair",
           "s_pivot_head", "s_pivot_update", "s_look_ahead", "s_loop_verify", "s_loop_flips", "s_dual_simplex_impl")
REPORT = ("k_solve", "s_dual_simplex_impl", "s_mir_round", "s_cut_round", "s_pivot", "s_loop_verify", "s_loop_flips", "k_debug_update")
WINDOW = 4096


def run(cmd):
    return subprocess.run(cmd, check=True, stdout=subprocess.PIPE, universal_newlines=True).stdout


def region_ranges():
    """(first line, last line, name) of the definition of every function of REGIONS in problem.inc: from its `name(` line to the next `}` in column 0"""
    lines = open(INC).read().split("\n")
    out = []
    for name in REGIONS:
        for k, ln in enumerate(lines):
            if re.search(r"\b%s\(" % name, ln) and ln.startswith("__device__") and not ln.rstrip().endswith(";"):
                end = next(j for j in range(k, len(lines)) if lines[j].startswith("}"))
                out.append((k + 1, end + 1, name))
    return out


def symbols(elf, demangle):
    """(size, name) of every function of the code object, in symbol-table order"""
    out, seen = [], set()
    for ln in run([os.path.join(LLVM, "llvm-readelf"), "-sW"] + (["--demangle"] if demangle else []) + [elf]).split("\n"):
        f = ln.split(None, 7)
        if len(f) >= 8 and f[3] == "FUNC" and f[2].isdigit() and int(f[2]) > 0 and f[1] not in seen:      # (a kernel has two symbols at one address)
            seen.add(f[1])
            out.append((int(f[2]), f[7].strip()))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--function", default="s_dual_simplex_impl<true, false, false>", help="substring of the demangled name whose text is attributed")
    ap.add_argument("--out", default=None)
    ap.add_argument("--keep", default=None, help="directory for the object files (default: a temporary one)")
    ap.add_argument("--reuse", action="store_true", help="do not compile again when --keep already holds the object file")
    a = ap.parse_args()
    tmp = a.keep or tempfile.mkdtemp(prefix="text_footprint_")
    os.makedirs(tmp, exist_ok=True)
    obj, elf = os.path.join(tmp, "mldgpu_dev.o"), os.path.join(tmp, "mldgpu_gfx950.elf")
    if not (a.reuse and os.path.exists(obj)):
        subprocess.check_call([HIPCC] + FLAGS + os.environ.get("MLD_CXXFLAGS", "").split() + ["-gline-tables-only", "--cuda-device-only", "-c", "-o", obj, SRC])
    if open(obj, "rb").read(4) == b"\x7fELF":
        elf = obj
    else:
        subprocess.check_call([os.path.join(LLVM, "clang-offload-bundler"), "--type=o", "--targets=" + TARGET, "--input=" + obj, "--output=" + elf, "--unbundle"])
    funcs = symbols(elf, False)      # (size, mangled)
    names = dict(zip((m for _, m in funcs), (d for _, d in symbols(elf, True))))
    rep = []
    rep.append("device text per function (bytes), functions whose name holds one of: " + ", ".join(REPORT))
    target = None
    for size, m in sorted(funcs, reverse=True):
        d = names.get(m, m)
        short = d.split("(")[0]
        if any(k in short for k in REPORT):
            rep.append("  %8d  %s" % (size, short))
        if a.function in d and target is None:
            target = (size, m, short)
    rep.append("  %8d  all %d device functions" % (sum(s for s, _ in funcs), len(funcs)))
    if target is None:
        print("\n".join(rep))
        sys.exit("no function matches %r" % a.function)
    size, mangled, short = target
    dis = run([os.path.join(LLVM, "llvm-objdump"), "-d", "-l", "--disassemble-symbols=" + mangled, elf])
    rng = region_ranges()
    inc_name = os.path.basename(INC)

    def region(path, line):
        if os.path.basename(path) != inc_name:
            return "other files (HIP headers)"
        for lo, hi, name in rng:
            if lo <= line <= hi:
                return name
        return "other helpers of problem.inc"

    insts = []      # (address, region)
    cur = "other files (HIP headers)"
    loc = re.compile(r"^; (\S+):(\d+)\s*$")
    ins = re.compile(r"//\s*([0-9A-Fa-f]+):\s+[0-9A-Fa-f]{8}")
    for ln in dis.split("\n"):
        m = loc.match(ln)
        if m:
            cur = region(m.group(1), int(m.group(2)))
            continue
        m = ins.search(ln)
        if m:
            insts.append((int(m.group(1), 16), cur))
    if not insts:
        sys.exit("no instructions found in the listing of " + short)
    start = insts[0][0]
    by = collections.Counter()
    win = collections.defaultdict(collections.Counter)
    for k, (addr, reg) in enumerate(insts):
        nb = (insts[k + 1][0] if k + 1 < len(insts) else start + size) - addr
        by[reg] += nb
        win[(addr - start) // WINDOW][reg] += nb
    tot = sum(by.values())
    rep.append("")
    rep.append("%s: %d bytes, %d instructions; by source region (inlined code counts where it was written)" % (short, size, len(insts)))
    for reg, nb in by.most_common():
        rep.append("  %8d  %5.1f %%  %s" % (nb, 100.0 * nb / tot, reg))
    rep.append("")
    rep.append("layout: regions with at least 10 %% of each %d-byte window, in address order" % WINDOW)
    for wk in sorted(win):
        parts = ["%s %d" % (r, nb) for r, nb in win[wk].most_common() if nb * 10 >= WINDOW]
        rep.append("  +%6d  %s" % (wk * WINDOW, "; ".join(parts)))
    text = "\n".join(rep) + "\n"
    sys.stdout.write(text)
    if a.out:
        open(a.out, "w").write(text)


if __name__ == "__main__":
    main()
