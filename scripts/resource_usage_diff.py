#!/usr/bin/env python3
"""Compare two `make -C csrc resource-usage` reports (hipcc -Rpass-analysis=kernel-resource-usage, stderr saved to a file).

    python scripts/resource_usage_diff.py parent.txt change.txt [--family NAME=VALUE ...] [--only REGEX]

Kernels are matched by demangled name without the argument list (a change may add a kernel parameter; it is the
instantiation that is matched).  A change that adds a trailing bool template parameter to a kernel family (TEX of the
path-trace kernels) is compared with `--family NAME=false`: the parent's `NAME<...>` is matched with the change's
`NAME<..., false>`.  A change that turns the last template parameter of a family from bool into int (TEX again, for the mip
instantiations) is compared with `--retype NAME=false:0` (and `NAME=true:1`): the parent's `NAME<..., false>` is matched with the
change's `NAME<..., 0>`.  Prints every kernel of the parent with both sets of numbers, marks the rows that differ, then lists the
kernels only the change has.  `--only REGEX` prints the rows of the kernels whose name matches and counts the other
unchanged ones in the last line only (the whole report of this library is 0.9 MB).  Exit status 1 when a matched kernel
differs or is missing."""
import argparse
import re
import subprocess
import sys

KEYS = ["TotalSGPRs", "VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "SGPRs Spill", "VGPRs Spill",
        "LDS Size [bytes/block]"]
SHORT = ["sgpr", "vgpr", "agpr", "scratch", "occ", "sspill", "vspill", "lds"]


def parse(path):
    out, cur = {}, None
    for line in open(path, errors="replace"):
        m = re.search(r"remark:\s+(.*?):\s+(\S+) \[-Rpass-analysis", line)
        if not m:
            continue
        key, val = m.group(1).strip(), m.group(2)
        if key == "Function Name":
            cur = out.setdefault(val, {})
        elif cur is not None:
            cur[key] = val
    names = list(out)
    dem = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    return {short(re.sub(r"\(anonymous namespace\)::", "", d)): out[n] for n, d in zip(names, dem)}


def short(n):
    """the name without its argument list (a change may add a kernel parameter: the instantiation is what is matched)"""
    return re.sub(r"\((rt::|HIP_|unsigned|float|int|char|bool|void|long|hip).*\)$", "", n)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parent")
    ap.add_argument("change")
    ap.add_argument("--family", action="append", default=[], help="NAME=VALUE: the change appended template argument VALUE to kernel NAME")
    ap.add_argument("--retype", action="append", default=[], help="NAME=OLD:NEW: the change spells the last template argument OLD of kernel NAME as NEW")
    ap.add_argument("--only", default=None, help="print only the kernels whose demangled name matches this regular expression")
    a = ap.parse_args()
    p, c = parse(a.parent), parse(a.change)
    fam = dict(f.split("=") for f in a.family)
    retype = {}
    for r in a.retype:
        name, pair = r.split("=")
        retype.setdefault(name, {}).update([pair.split(":")])

    def renamed(name):
        m = re.match(r"(void )?(rt::)?(\w+)<(.*)>$", name)
        if m and m.group(3) in fam:
            return f"{m.group(1) or ''}{m.group(2) or ''}{m.group(3)}<{m.group(4)}, {fam[m.group(3)]}>"
        if m and m.group(3) in retype:
            args = m.group(4).split(", ")
            args[-1] = retype[m.group(3)].get(args[-1], args[-1])
            return f"{m.group(1) or ''}{m.group(2) or ''}{m.group(3)}<{', '.join(args)}>"
        return name
    show = (lambda n: re.search(a.only, n)) if a.only else (lambda n: True)
    bad, matched, hidden = 0, set(), 0
    print("kernel | " + " ".join(SHORT) + " | parent -> change")
    for name, pv in p.items():
        cn = renamed(name)
        cv = c.get(cn)
        matched.add(cn)
        pa = [pv.get(k, "?") for k in KEYS]
        if cv is None:
            print(f"MISSING {short(name)}: {' '.join(pa)}")
            bad += 1
            continue
        ca = [cv.get(k, "?") for k in KEYS]
        same = pa == ca
        bad += not same
        if same and not show(cn):
            hidden += 1
            continue
        print(f"{'same  ' if same else 'DIFFER'} {short(cn)}: {' '.join(pa)}" + ("" if same else f" -> {' '.join(ca)}"))
    print("\nkernels only the change has:")
    for name, cv in c.items():
        if name not in matched:
            print(f"new    {short(name)}: {' '.join(cv.get(k, '?') for k in KEYS)}")
    print(f"\n{len(p)} kernels of the parent, {bad} differ or are missing" + (f" ({hidden} unchanged ones not listed)" if hidden else ""))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
