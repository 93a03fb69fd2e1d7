#!/usr/bin/env python3
"""Compare the gfx950 device code of two copies of csrc/, kernel by kernel.

    scripts/device_asm_diff.py <parent csrc> <new csrc> [--by-kernel] [--pair-renamed] [-o summary.txt] [-j jobs] [-D macro ...]

For a refactor that must not change what the GPU executes.  Every .hip file of the new directory is compiled in both
directories with the Makefile's own HIPCC / CXXFLAGS plus `--cuda-device-only -S` (no GPU needed), and the two assembly
texts are compared function by function, from a function's `.type <name>,@function` line to its `.end_amdhsa_kernel`
(the instructions AND the .amdhsa_* descriptor: registers, LDS, scratch), and `.amdgpu_metadata` entry by entry, sorted
by kernel name.  Three things are normalised, nothing else:
  * the `__hip_cuid_<hash>` symbol (a hash of the source path),
  * the numbering of `.LBB<n>_<m>` and `.Lfunc_begin<n>` / `.Lfunc_end<n>` (n = order of instantiation in the file),
  * comments (`;` to the end of the line) and column padding.
Prints one line per file (kernels compared, kernels equal) and exits 1 if any set of symbols or any text differs.

--by-kernel: for a refactor that moves kernels between files.  Every .hip file of EITHER directory is compiled where it lies,
the kernels, the other device functions and the metadata entries of a side are pooled over its files, and the two pools are
compared by name, with the same normalisations.  A name that two files of one side define cannot be pooled (the pool would hold
one of them): it is compared as `name [file]`, file by file as without the option, and counted in the side's line — a library's
template kernels that two files instantiate (rocprim's, in the two tree builders).  Such a kernel that also moved between files
therefore shows as "only in".  Prints one line per side (files, kernels) and one for the comparison.

--pair-renamed: for a refactor that changes a kernel's signature or template parameters, and with them its mangled name.  Only
names found on ONE side are treated: in such an entry's text its own symbol (the .kd symbol carries it too) is replaced by a
placeholder, and a parent-only name pairs with a new-only name when the two placeholder texts are equal and the qualified function
name agrees — the length-prefixed components of the mangled name in front of its template arguments; no demangler is needed.
Names pair as a multiset, a pair counts as compared once and as equal, and the comparison's line gains `renamed N, paired N`.
Whatever finds no partner is reported as "only in", as without the option.
"""
import argparse
import concurrent.futures
import difflib
import os
import re
import subprocess
import sys
import tempfile


def make_vars(csrc):
    """HIPCC and the expanded CXXFLAGS of csrc/Makefile (EXTRA empty, the environment's HIPCC / ARCH honoured)."""
    text = open(os.path.join(csrc, "Makefile")).read().replace("\\\n", " ")
    var = {}
    for m in re.finditer(r"^(\w+)\s*\??=\s*(.*)$", text, re.M):
        var.setdefault(m.group(1), m.group(2).strip())
    var["EXTRA"] = ""
    for k in ("HIPCC", "ARCH"):
        var[k] = os.environ.get(k, var[k])
    expand = lambda s: re.sub(r"\$\((\w+)\)", lambda m: expand(var.get(m.group(1), "")), s)
    return expand(var["HIPCC"]), expand(var["CXXFLAGS"]).split()


def device_asm(csrc, name, defines, tmp, tag):
    hipcc, flags = make_vars(csrc)
    out = os.path.join(tmp, f"{tag}_{name}.s")
    cmd = [hipcc] + flags + [f"-D{d}" for d in defines] + ["--cuda-device-only", "-S", "-o", out, name]
    r = subprocess.run(cmd, cwd=csrc, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"{' '.join(cmd)} (in {csrc}) failed:\n{r.stderr}")
    return open(out).read()


def normalise(line):
    line = line.split(";", 1)[0]
    line = re.sub(r"__hip_cuid_[0-9a-f]+", "__hip_cuid_", line)
    line = re.sub(r"\.LBB\d+_", ".LBB_", line)
    line = re.sub(r"\.Lfunc_(begin|end)\d+", r".Lfunc_\1", line)
    return " ".join(line.split())


def functions(asm):
    """name -> (normalised text, is a kernel); a block ends at .end_amdhsa_kernel, or at .Lfunc_end for a plain function"""
    out, name, lines = {}, None, []

    def close():
        if name is None:
            return
        ends = [i for i, l in enumerate(lines) if l == ".end_amdhsa_kernel"]
        if ends:
            out[name] = ("\n".join(lines[: ends[0] + 1]), True)
        else:
            ends = [i for i, l in enumerate(lines) if l.startswith(".Lfunc_end")]
            out[name] = ("\n".join(lines[: ends[0] + 1] if ends else lines), False)

    for raw in asm.splitlines():
        m = re.match(r"\s*\.type\s+(\S+),@function", raw)
        if m or raw.strip() == ".amdgpu_metadata":
            close()
            name, lines = (m.group(1), []) if m else (None, [])
        if name is not None:
            l = normalise(raw)
            if l:
                lines.append(l)
    close()
    return out


def metadata(asm):
    """kernel name -> normalised text of its entry of amdhsa.kernels"""
    m = re.search(r"^\s*\.amdgpu_metadata\n(.*?)^\s*\.end_amdgpu_metadata", asm, re.M | re.S)
    if not m or "amdhsa.kernels:" not in m.group(1):
        return {}
    body = m.group(1).split("amdhsa.kernels:", 1)[1]
    body = re.split(r"^amdhsa\.\w+:", body, 1, re.M)[0]
    out = {}
    for entry in re.split(r"^  - (?=\.)", body, flags=re.M)[1:]:
        text = "\n".join(filter(None, (normalise(l) for l in entry.splitlines())))
        out[re.search(r"^\.name: *(\S+)", text, re.M).group(1)] = text
    return out


def qualified_name(symbol):
    """_ZN2rt12_GLOBAL__N_111k_pathtraceILi1E... -> ("rt", "_GLOBAL__N_1", "k_pathtrace"); a name that is not mangled is itself"""
    m = re.match(r"_ZN?(?=\d)", symbol)
    if not m:
        return (symbol,)
    rest, parts = symbol[m.end():], []
    while m := re.match(r"\d+", rest):
        end = m.end() + int(m.group())
        parts.append(rest[m.end():end])
        rest = rest[end:]
    return tuple(parts)


def pair_renamed(old, new):
    """--pair-renamed: (parent-only names, new-only names, how many of each found a partner), the partners taken out of both lists"""
    def by_text(d, names):
        out = {}
        for n in names:
            symbol = n.split(" [")[0]
            out.setdefault((qualified_name(symbol), d[n].replace(symbol, "@renamed")), []).append(n)
        return out

    only_old, only_new = by_text(old, sorted(set(old) - set(new))), by_text(new, sorted(set(new) - set(old)))
    paired = 0
    for k in only_old.keys() & only_new.keys():
        c = min(len(only_old[k]), len(only_new[k]))
        paired += c
        del only_old[k][:c], only_new[k][:c]
    return sorted(sum(only_old.values(), [])), sorted(sum(only_new.values(), [])), paired


def compare(what, old, new, report, pair=False):
    """"<names compared>, equal <names whose text is equal>" for the summary line; differences go to report"""
    only_old, only_new, paired, note = sorted(set(old) - set(new)), sorted(set(new) - set(old)), 0, ""
    if pair:
        renamed = len(only_old)
        only_old, only_new, paired = pair_renamed(old, new)
        note = f", renamed {renamed}, paired {paired}"
    equal = paired
    for n in only_old:
        report.append(f"  {what} only in the parent: {n}")
    for n in only_new:
        report.append(f"  {what} only in the new code: {n}")
    for n in sorted(set(old) & set(new)):
        if old[n] == new[n]:
            equal += 1
            continue
        d = list(difflib.unified_diff(old[n].splitlines(), new[n].splitlines(), "parent", "new", lineterm="", n=1))
        report.append(f"  {what} differs: {n} ({sum(l[0] in '+-' for l in d) - 2} changed lines)")
        report.extend("    " + l for l in d[:12])
    return f"{len(set(old) | set(new)) - paired}, equal {equal}{note}"


def pooled(asms):
    """(kernels, other device functions, metadata entries, names in two files) of one side, name -> text, over all of its files"""
    where = {}
    per_file = {f: (functions(asms[f]), metadata(asms[f])) for f in sorted(asms)}
    for f, (fns, _) in per_file.items():
        for n in fns:
            where.setdefault(n, []).append(f)
    twice = {n for n, fs in where.items() if len(fs) > 1}
    key = lambda n, f: f"{n} [{f}]" if n in twice else n
    kern, plain, meta = {}, {}, {}
    for f, (fns, md) in per_file.items():
        for n, (t, k) in fns.items():
            (kern if k else plain)[key(n, f)] = t
        for n, t in md.items():
            meta[key(n, f)] = t
    return kern, plain, meta, len(twice)


def by_kernel(a):
    sides = {"parent": a.parent, "new": a.new}
    with tempfile.TemporaryDirectory() as tmp, concurrent.futures.ThreadPoolExecutor(a.jobs) as pool:
        jobs = {side: {f: pool.submit(device_asm, d, f, a.defines, tmp, side) for f in sorted(os.listdir(d)) if f.endswith(".hip")}
                for side, d in sides.items()}
        asms = {side: {f: j.result() for f, j in fs.items()} for side, fs in jobs.items()}
    report, summary = [], []
    (ko, po, mo, to), (kn, pn, mn, tn) = (pooled(asms[side]) for side in ("parent", "new"))
    for side, k, twice in (("parent", ko, to), ("new", kn, tn)):
        summary.append(f"{side}: {len(asms[side])} files, {len(k)} kernels" + (f" ({twice} names in two files, compared per file)" if twice else ""))
    k_eq = compare("kernel", ko, kn, report, a.pair_renamed)
    p_eq = compare("device function", po, pn, report)
    m_eq = compare("metadata entry", mo, mn, report, a.pair_renamed)
    line = f"by kernel: kernels compared {k_eq}; metadata entries {m_eq}"
    if po or pn:
        line += f"; other device functions {p_eq}"
    summary.append(line)
    if report:
        print("\n".join(report))
    return summary, not report


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("parent")
    ap.add_argument("new")
    ap.add_argument("-o", "--out", help="also write the summary lines to this file")
    ap.add_argument("-j", "--jobs", type=int, default=4)
    ap.add_argument("-D", dest="defines", action="append", default=[], help="macro for both sides (e.g. RTPT_AB_VARIANTS=1)")
    ap.add_argument("--by-kernel", action="store_true", help="pool the kernels of each side over its files and compare by kernel name")
    ap.add_argument("--pair-renamed", action="store_true", help="pair kernels found on one side only by their text and qualified function name")
    a = ap.parse_args()
    if a.by_kernel:
        summary, ok = by_kernel(a)
        text = "\n".join(summary) + "\n" + ("all equal\n" if ok else "DIFFERENCES\n")
        print(text, end="")
        if a.out:
            open(a.out, "w").write(text)
        return 0 if ok else 1
    names = sorted(f for f in os.listdir(a.new) if f.endswith(".hip"))
    missing = [f for f in sorted(os.listdir(a.parent)) if f.endswith(".hip") and f not in names]
    summary, ok = [], not missing
    for f in missing:
        summary.append(f"{f}: only in the parent")
    with tempfile.TemporaryDirectory() as tmp, concurrent.futures.ThreadPoolExecutor(a.jobs) as pool:
        jobs = {f: (pool.submit(device_asm, a.parent, f, a.defines, tmp, "parent") if os.path.exists(os.path.join(a.parent, f)) else None,
                    pool.submit(device_asm, a.new, f, a.defines, tmp, "new")) for f in names}
        for f in names:
            if jobs[f][0] is None:
                summary.append(f"{f}: only in the new code")
                ok = False
                continue
            old, new = jobs[f][0].result(), jobs[f][1].result()
            report = []
            fo, fn = functions(old), functions(new)
            ko, kn = ({n: t for n, (t, k) in d.items() if k} for d in (fo, fn))
            po, pn = ({n: t for n, (t, k) in d.items() if not k} for d in (fo, fn))
            mo, mn = metadata(old), metadata(new)
            k_eq = compare("kernel", ko, kn, report, a.pair_renamed)
            p_eq = compare("device function", po, pn, report)
            m_eq = compare("metadata entry", mo, mn, report, a.pair_renamed)
            line = f"{f}: kernels compared {k_eq}; metadata entries {m_eq}"
            if po or pn:
                line += f"; other device functions {p_eq}"
            summary.append(line)
            if report:
                ok = False
                print(line)
                print("\n".join(report))
    text = "\n".join(summary) + "\n" + ("all equal\n" if ok else "DIFFERENCES\n")
    print(text, end="")
    if a.out:
        open(a.out, "w").write(text)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
