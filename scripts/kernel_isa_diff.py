#!/usr/bin/env python3
"""Per-kernel comparison of two hipcc -S listings (--offload-device-only -S with the Makefile's flags): is the instruction stream the
same, how many instructions, and the registers / scratch / LDS of the amdhsa metadata (what kernel_regs.py prints) plus the occupancy
the compiler states.

usage: kernel_isa_diff.py OLD.s NEW.s [--rename 'REGEX=REPLACEMENT' ...]

A stream is the kernel's instructions and labels with comments stripped, `.LBB<n>_` label numbers and mangled symbol names
normalised (both only number / name the function, they do not change what runs).  Kernels are paired by their demangled name without the
parameter list; --rename rewrites OLD names first (first matching rule wins), for kernels that were renamed or gained a template
argument, e.g.  --rename 'nlr_encode8_kernel<(.*)>=nlr_encode8_kernel<\\1, true>'.
Exit status 1 when a kernel of OLD has no partner in NEW and no rule names one."""
import re
import shutil
import subprocess
import sys


def demangle(names):
    tool = shutil.which("llvm-cxxfilt") or shutil.which("llvm-cxxfilt", path="/opt/rocm/lib/llvm/bin") or shutil.which("c++filt")
    if not tool or not names:
        return {n: n for n in names}
    out = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")

    def short(d):  # "void nlr_k<float, 1>(CastParams, ...)" -> "nlr_k<float, 1>"
        depth = 0
        for i, ch in enumerate(d):
            depth += (ch == "<") - (ch == ">")
            if ch == "(" and depth == 0:
                d = d[:i]
                break
        return re.sub(r"^void ", "", d)

    return {n: short(d) for n, d in zip(names, out)}


def kernels(path):
    txt = open(path).read()
    meta = {}
    for blk in txt.split("  - .agpr_count:")[1:]:
        g = lambda k: (re.search(r"\." + k + r":\s+(\S+)", blk) or [None, "?"])[1]
        meta[g("symbol")[:-3]] = dict(vgpr=g("vgpr_count"), agpr=blk.split()[0], sgpr=g("sgpr_count"), scratch=g("private_segment_fixed_size"),
                                      lds=g("group_segment_fixed_size"))
    res = {}
    for m in re.finditer(r"^(\w+):[^\n]*\n(.*?)^\s+\.section\s+\.rodata.*?^; Occupancy: (\d+)", txt, re.M | re.S):
        name, body, occ = m.groups()
        if name not in meta:
            continue
        stream = []
        for line in body.split("\n"):
            line = line.split(";")[0].strip()
            if not line or (line.startswith(".") and not line.endswith(":")):
                continue  # comments, directives
            line = re.sub(r"\.LBB\d+_", ".LBB_", line)
            line = re.sub(r"\b_Z\w+", "SYM", line)
            stream.append(line)
        res[name] = dict(meta[name], occ=occ, stream=stream, insts=sum(1 for s in stream if not s.endswith(":")))
    return res


def main():
    args, rules = [], []
    it = iter(sys.argv[1:])
    for a in it:
        if a == "--rename":
            pat, rep = next(it).split("=", 1)
            rules.append((re.compile("^" + pat + "$"), rep))
        else:
            args.append(a)
    old, new = kernels(args[0]), kernels(args[1])
    dn = demangle(list(old) + list(new))
    new_by = {dn[n]: k for n, k in new.items()}
    fig = lambda k: f"{k['insts']:5d} insts vgpr {k['vgpr']:>3s} sgpr {k['sgpr']:>3s} scratch {k['scratch']:>3s} lds {k['lds']:>5s} occ {k['occ']}"
    missing, seen = 0, set()
    for n, k in old.items():
        want = dn[n]
        for pat, rep in rules:
            if pat.match(want):
                want = pat.sub(rep, want)
                break
        seen.add(want)
        other = new_by.get(want)
        if other is None:
            missing += 1
            print(f"{dn[n]}\n    NO PARTNER ({want})   old {fig(k)}")
            continue
        verdict = "identical" if other["stream"] == k["stream"] else "DIFFERENT"
        label = dn[n] if want == dn[n] else f"{dn[n]} -> {want}"
        print(f"{label}\n    {verdict:9s}  old {fig(k)}\n               new {fig(other)}")
    for d, k in new_by.items():
        if d not in seen:
            print(f"{d}\n    only in NEW    {fig(k)}")
    return 1 if missing else 0


if __name__ == "__main__":
    sys.exit(main())
