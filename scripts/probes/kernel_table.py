#!/usr/bin/env python3
"""Kernel table of two trees' device assembly (no GPU): for every kernel instantiation of every translation unit, whether the instruction text is the
same, and the compiler's resource figures on both sides.

    kernel_table.py PARENT_ASM_DIR TREE_ASM_DIR > table.txt

Each directory holds one <unit>.s per csrc/<unit>.hip, made with the Makefile's flags plus --offload-device-only -S.  Instruction text is compared
position by position after dropping comments and directives and renaming block labels.  v = VGPRs (+a = AGPRs), s = SGPRs, scr = scratch bytes per
lane, lds = static LDS bytes, occ = waves per SIMD as the compiler reports them, n = instructions.  Exit status 1 if a kernel was added or removed."""
import os
import re
import subprocess
import sys

FIG = {"NumVgprs": "v", "NumAgprs": "a", "TotalNumSgprs": "s", "ScratchSize": "scr", "LDSByteSize": "lds", "Occupancy": "occ"}


def demangle(names):
    if not names:
        return {}
    try:
        out = subprocess.run(["c++filt"] + names, capture_output=True, text=True, check=True).stdout.split("\n")
        return {m: re.sub(r"\(.*\)$", "", d) for m, d in zip(names, out)}
    except (OSError, subprocess.CalledProcessError):
        return {m: m for m in names}


def kernels(path):
    """[(mangled name, [instructions], {figure: value})] in file order"""
    lines = open(path).read().split("\n")
    entry = {m.group(1) for m in (re.match(r"\s*\.amdhsa_kernel\s+(\S+)", ln) for ln in lines) if m}
    out, i = [], 0
    while i < len(lines):
        m = re.match(r"^([A-Za-z_][\w$.]*):", lines[i])
        if not m or m.group(1) not in entry:
            i += 1
            continue
        name, ins, fig, labels = m.group(1), [], {}, {}
        i += 1
        while i < len(lines) and not lines[i].startswith(".Lfunc_end"):
            t = lines[i].split(";")[0].strip()
            i += 1
            if not t or t.startswith("."):
                if re.match(r"^\.LBB\d+_\d+:", t):
                    ins.append("L:")
                continue
            ins.append(t)
        while i < len(lines) and "Occupancy" not in fig and not re.match(r"^[A-Za-z_][\w$.]*:", lines[i]):      # the "; Kernel info:" block behind the body
            f = re.match(r"^;\s*(\w+):\s*(\d+)", lines[i])
            if f and f.group(1) in FIG:
                fig[f.group(1)] = int(f.group(2))
            i += 1

        def rename(t):
            return re.sub(r"\.LBB\d+_\d+", lambda g: "L%d" % labels.setdefault(g.group(0), len(labels)), t)
        out.append((name, [rename(t) for t in ins], fig))
    return out


def figures(ins, fig):
    v = "v%d" % fig.get("NumVgprs", -1) + ("+a%d" % fig["NumAgprs"] if fig.get("NumAgprs") else "")
    return "%s s%d scr%d lds%d occ%d n%d" % (v, fig.get("TotalNumSgprs", -1), fig.get("ScratchSize", -1), fig.get("LDSByteSize", -1), fig.get("Occupancy", -1),
                                             sum(1 for t in ins if t != "L:"))


def main(a, b):
    total = same = 0
    status = 0
    print("%-11s %-50s | parent | this tree" % ("file", "kernel"))
    for unit in sorted(f for f in os.listdir(a) if f.endswith(".s")):
        ka, kb = kernels(os.path.join(a, unit)), kernels(os.path.join(b, unit))
        names = demangle([k[0] for k in ka] + [k[0] for k in kb])
        if [k[0] for k in ka] != [k[0] for k in kb]:
            print("%-11s the kernels or their order differ: %s" % (unit[:-2], sorted({k[0] for k in ka} ^ {k[0] for k in kb})))
            status = 1
        other = {k[0]: k for k in kb}
        for name, ins, fig in ka:
            if name not in other:
                continue
            _, ins2, fig2 = other[name]
            total += 1
            ident = ins == ins2
            same += ident
            print("%-11s %-50s %-10s | %s | %s" % (unit[:-2], names[name], "IDENTICAL" if ident else "DIFFERS", figures(ins, fig), figures(ins2, fig2)))
    print("%d kernel instantiations, %d IDENTICAL" % (total, same))
    return status


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
