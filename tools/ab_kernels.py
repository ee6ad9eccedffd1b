#!/usr/bin/env python3
"""Compare the gfx950 machine code of every kernel in two source trees, symbol by symbol.

    tools/ab_kernels.py PARENT_TREE NEW_TREE [--jobs N] [--keep DIR]

For a pure move/delete refactor: each csrc/*.hip of both trees is compiled with the exact command
`make` would use for it (taken from `make -n -B`, so per-file flags are included) plus
`--cuda-device-only -S`; the assembly is cut into one block per kernel symbol (from its label through
s_endpgm and the kernel descriptor — register, scratch and LDS figures — to the end of the function),
comments, blank lines and trailing whitespace are dropped and the per-file counters in local
labels (.LBB<n>_, .LJTI<n>_, .Ltmp<n>) are replaced by a placeholder.  Blocks are then compared by symbol
over the union of all files: a kernel may change files, its text may not.  Needs hipcc, no GPU.
Exit status 0 when no symbol differs (missing / new symbols are listed but are the caller's to judge).
"""
import argparse
import concurrent.futures as cf
import os
import re
import subprocess
import sys
import tempfile

CSRC = os.path.join("spark-text-clustering_amd", "csrc")
LABEL = re.compile(r"\.(LBB|LJTI|Ltmp|Lfunc_begin|Lfunc_end)\d+")


def compile_cmds(csrc):
    """{file.hip: argv} from the Makefile's own rules."""
    out = subprocess.run(["make", "-C", csrc, "-n", "-B", "BUILD=ab"], check=True, capture_output=True, text=True).stdout
    cmds = {}
    for line in out.splitlines():
        m = re.search(r" -c (\S+\.hip) -o \S+$", line)
        if m:
            cmds[m.group(1)] = line[: m.start()].split()
    return cmds


def kernels(asm):
    """{symbol: normalised text} for every .amdhsa_kernel symbol of one assembly file."""
    lines = [l.split(";", 1)[0].rstrip() for l in asm.splitlines()]
    names = {l.split()[1] for l in lines if l.lstrip().startswith(".amdhsa_kernel ")}
    blocks, cur = {}, None
    for l in lines:
        if cur is None:
            if l.endswith(":") and l[:-1] in names:
                cur = l[:-1]
                blocks[cur] = []
        elif l.startswith(".Lfunc_end"):
            cur = None
        elif l:
            blocks[cur].append(LABEL.sub(r".\1#", l))
    return {k: "\n".join(v) for k, v in blocks.items()}


def tree_kernels(tree, jobs, keep):
    csrc = os.path.join(tree, CSRC)
    tmp = keep or tempfile.mkdtemp(prefix="ab_kernels_")
    os.makedirs(tmp, exist_ok=True)

    def one(item):
        src, argv = item
        s = os.path.join(os.path.abspath(tmp), src[:-4] + ".s")
        subprocess.run(argv + ["--cuda-device-only", "-S", src, "-o", s], cwd=csrc, check=True)
        with open(s) as f:
            return src, kernels(f.read())

    syms = {}
    with cf.ThreadPoolExecutor(jobs) as ex:
        for src, ks in ex.map(one, sorted(compile_cmds(csrc).items())):
            for name, text in ks.items():
                if name in syms and syms[name][1] != text:
                    print(f"{tree}: {name} differs between {syms[name][0]} and {src}")
                syms[name] = (src, text)
    return syms


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("parent")
    ap.add_argument("new")
    ap.add_argument("--jobs", type=int, default=8)
    ap.add_argument("--keep", help="keep the .s files under DIR/parent and DIR/new")
    a = ap.parse_args()
    A = tree_kernels(a.parent, a.jobs, a.keep and os.path.join(a.keep, "parent"))
    B = tree_kernels(a.new, a.jobs, a.keep and os.path.join(a.keep, "new"))
    demangle = lambda s: subprocess.run(["c++filt", s], capture_output=True, text=True).stdout.strip() or s
    same = moved = differ = 0
    for name in sorted(set(A) | set(B)):
        if name not in B:
            print(f"only in parent ({A[name][0]}): {demangle(name)}")
        elif name not in A:
            print(f"only in new    ({B[name][0]}): {demangle(name)}")
        elif A[name][1] != B[name][1]:
            differ += 1
            print(f"DIFFERS ({A[name][0]} -> {B[name][0]}): {demangle(name)}")
        else:
            same += 1
            moved += A[name][0] != B[name][0]
    print(f"ab_kernels: {len(A)} parent / {len(B)} new kernel symbols; {same} identical ({moved} of them "
          f"in another file), {differ} differ, {len(set(A) - set(B))} only in parent, {len(set(B) - set(A))} only in new")
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
