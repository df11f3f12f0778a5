#!/usr/bin/env python3
"""Function-by-function comparison of the device ISA of two source trees.

Each unit is compiled to gfx950 assembly with the library's flags
(csrc/Makefile, `-x hip --cuda-device-only -S`) from a base tree and from the
working tree.  Every function is keyed by its symbol; its body is compared with
comments stripped and basic-block labels renumbered per function, and the
compiler's own resource lines (VGPRs, SGPRs, LDS bytes, scratch bytes,
occupancy) are printed for both trees.  It diffs and reports, nothing else.

    python tools/isa_diff.py                          # HEAD against the working tree
    python tools/isa_diff.py --base-rev main~1 --units proposal.hip eval.hip
    python tools/isa_diff.py --base-dir /path/to/other/csrc
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = "replication_faster_rcnn_amd/csrc"
UNITS = ["proposal.hip", "fpn_proposal.hip", "eval.hip", "eval_coco.hip", "losses.hip", "targets.hip", "detect.hip"]
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off",
         "-fhip-fp32-correctly-rounded-divide-sqrt", "-x", "hip", "--cuda-device-only", "-S"]
STATS = [("vgpr", r"; NumVgprs: (\d+)"), ("sgpr", r"; TotalNumSgprs: (\d+)"),
         ("lds", r"; LDSByteSize: (\d+)"), ("scratch", r"; ScratchSize: (\d+)"), ("occ", r"; Occupancy: (\d+)")]


def compile_unit(csrc, unit, out):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.run([hipcc, *FLAGS, unit, "-o", out], cwd=csrc, check=True, stderr=subprocess.DEVNULL)


def demangle(names):
    try:
        r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True)
        return dict(zip(names, r.stdout.splitlines()))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def parse(path):
    """symbol -> (body lines, stats dict) of every function of one assembly file."""
    funcs, sym, body, stats = {}, None, None, None
    with open(path) as f:
        lines = f.read().splitlines()
    ftype = re.compile(r"\s*\.type\s+(\S+),@function")
    pending = None
    for ln in lines:
        m = ftype.match(ln)
        if m:
            pending, stats = m.group(1), None
            continue
        if pending and ln.startswith(pending + ":"):
            sym, body, pending = pending, [], None
            continue
        if sym is not None and body is not None:
            if ln.startswith(".Lfunc_end"):
                stats = {}
                funcs[sym] = (body, stats)
                body = None
                continue
            code = ln.split(";", 1)[0].rstrip()
            if not code.strip():
                continue
            tok = code.strip()
            if tok.startswith(".") and not tok.endswith(":"):
                continue  # directives (sections, alignment, the kernel descriptor)
            body.append(re.sub(r"\.LBB\d+_", ".LBB_", code))
        elif stats is not None:
            for key, pat in STATS:
                m = re.match(pat, ln)
                if m and key not in stats:
                    stats[key] = int(m.group(1))
    return funcs


def fmt(st):
    return "vgpr %3s sgpr %3s lds %6s scratch %4s occ %s" % tuple(st.get(k, "-") for k, _ in STATS)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--base-rev", default="HEAD", help="git revision of the base tree (default HEAD)")
    ap.add_argument("--base-dir", help="a csrc directory to use as the base instead of a revision")
    ap.add_argument("--units", nargs="+", default=UNITS)
    args = ap.parse_args()
    worse = 0
    with tempfile.TemporaryDirectory() as tmp:
        base = args.base_dir
        if not base:
            ar = subprocess.run(["git", "archive", args.base_rev, CSRC, "include"], cwd=ROOT, check=True,
                                capture_output=True).stdout
            subprocess.run(["tar", "-x", "-C", tmp], input=ar, check=True)
            base = os.path.join(tmp, CSRC)
        for unit in args.units:
            a_s, b_s = os.path.join(tmp, unit + ".base.s"), os.path.join(tmp, unit + ".new.s")
            compile_unit(base, unit, a_s)
            compile_unit(os.path.join(ROOT, CSRC), unit, b_s)
            fa, fb = parse(a_s), parse(b_s)
            names = demangle(sorted(set(fa) | set(fb)))
            same = sum(1 for s in fa if s in fb and fa[s][0] == fb[s][0])
            print("== %s: %d functions, %d identical" % (unit, len(set(fa) | set(fb)), same))
            for s in sorted(set(fa) | set(fb), key=lambda x: names[x]):
                short = names[s].replace("(anonymous namespace)::", "").replace("frcnn::", "")
                short = re.sub(r"^void ", "", re.sub(r"\(.*", "", short))
                if s not in fa or s not in fb:
                    print("  %-9s %s" % ("base only" if s in fa else "new only", short))
                    continue
                (ba, sa), (bb, sb) = fa[s], fb[s]
                if ba == bb and sa == sb:
                    print("  identical %-48s %4d lines  %s" % (short, len(ba), fmt(sa)))
                    continue
                flag = ""
                if sb.get("scratch", 0) > sa.get("scratch", 0) or sb.get("occ", 0) < sa.get("occ", 0):
                    flag, worse = "  <-- more scratch or lower occupancy", worse + 1
                print("  DIFFERENT %-48s %4d -> %4d lines%s" % (short, len(ba), len(bb), flag))
                print("      base  %s" % fmt(sa))
                print("      new   %s" % fmt(sb))
    print("functions with more scratch or lower occupancy than the base: %d" % worse)
    return 0


if __name__ == "__main__":
    sys.exit(main())
