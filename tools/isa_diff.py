#!/usr/bin/env python3
"""Per-kernel comparison of two builds of one translation unit: two .s files in, one table out.

  hipcc <flags> --cuda-device-only -S x.hip -o old.s -Rpass-analysis=kernel-resource-usage 2> old.remarks   (and the same for new)
  tools/isa_diff.py old.s new.s [--remarks old.remarks new.remarks] [--map REGEX=REPL ...]

Kernels are matched by demangled name; --map rewrites the OLD names first (a kernel that was renamed or lost a template argument).
Per kernel: the instruction counts, the first differing line of the instruction streams (directives, comments and blank lines
stripped, block labels renumbered) and the number of differing lines, then the resource rows of both builds.
"""
import argparse, difflib, re, shutil, subprocess

KEYS = ["VGPRs", "AGPRs", "VGPRs Spill", "ScratchSize [bytes/lane]", "LDS Size [bytes/block]", "Occupancy [waves/SIMD]", "TotalSGPRs", "SGPRs Spill"]


def demangle(names):
    filt = shutil.which("llvm-cxxfilt") or shutil.which("c++filt") or "/opt/rocm/llvm/bin/llvm-cxxfilt"
    out = subprocess.run([filt], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
    return {m: re.sub(r"^void |\(.*\)$", "", d) for m, d in zip(names, out)}


def kernels(path):
    """mangled name -> instruction stream of every .amdhsa_kernel of the file"""
    text = open(path).read()
    wanted = set(re.findall(r"^\s*\.amdhsa_kernel (\S+)", text, re.M))
    out, cur = {}, None
    for line in text.split("\n"):
        m = re.match(r"^(\w+):", line)
        if m and m.group(1) in wanted:
            cur = out.setdefault(m.group(1), [])
            continue
        if cur is None:
            continue
        if line.startswith(".Lfunc_end"):
            cur = None
            continue
        line = re.sub(r"\.LBB\d+_", ".LBB_", line.split(";")[0]).strip()
        if line and (not line.startswith(".") or line.startswith(".LBB_")):
            cur.append(line)
    return out


def remarks(path):
    out, cur = {}, None
    for line in open(path):
        m = re.search(r"remark:\s+(.*?): (\S+) \[-Rpass-analysis", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            cur = out.setdefault(m.group(2), {})
        elif cur is not None:
            cur[m.group(1)] = m.group(2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("old"), ap.add_argument("new")
    ap.add_argument("--remarks", nargs=2)
    ap.add_argument("--map", action="append", default=[])
    args = ap.parse_args()
    ko, kn = kernels(args.old), kernels(args.new)
    dm = demangle(sorted(set(ko) | set(kn)))
    ren = {}
    for m in ko:
        name = dm[m]
        for rule in args.map:
            pat, repl = rule.split("=", 1)
            name = re.sub(pat, repl, name)
        ren[name] = m
    new = {dm[m]: m for m in kn}
    ro, rn = (remarks(args.remarks[0]), remarks(args.remarks[1])) if args.remarks else ({}, {})
    print(f"kernels: old {len(ko)}, new {len(kn)}; only old: {sorted(set(ren) - set(new))}; only new: {sorted(set(new) - set(ren))}")
    same = moved = 0
    for name in sorted(set(ren) & set(new)):
        a, b = ko[ren[name]], kn[new[name]]
        first = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), None if len(a) == len(b) else min(len(a), len(b)))
        if first is None:
            verdict, same = "identical", same + 1
        else:
            ops = [o for o in difflib.SequenceMatcher(None, a, b, autojunk=False).get_opcodes() if o[0] != "equal"]
            nd = sum(max(o[2] - o[1], o[4] - o[3]) for o in ops)
            # the epilogue: from the last barrier of the stream (the one behind the body, where there is one) to the end
            bar = max(i for i, x in enumerate(a) if x.startswith("s_barrier")) if any(x.startswith("s_barrier") for x in a) else -1
            verdict, moved = f"first difference at line {first}, {nd} lines differ (old lines {ops[0][1]}..{ops[-1][2]}; last s_barrier at {bar})", moved + 1
        print(f"\n{name}" + (f"   [old: {dm[ren[name]]}]" if dm[ren[name]] != name else ""))
        print(f"  instructions old {len(a)} new {len(b)}: {verdict}")
        if args.remarks:
            o, n = ro.get(ren[name], {}), rn.get(new[name], {})
            for tag, r in (("old", o), ("new", n)):
                print(f"  {tag}: " + ", ".join(f"{k.split(' [')[0]} {r.get(k, '?')}" for k in KEYS))
            bad = [k for k in KEYS[:6] if o.get(k) != n.get(k)]
            if bad:
                print(f"  RESOURCES DIFFER: {bad}")
    print(f"\n{same} identical, {moved} differ")


main()
