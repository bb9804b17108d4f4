#!/usr/bin/env python3
"""Are two builds the same device code?  Compares two sets of `hipcc -S --cuda-device-only` listings
function by function: the instruction lines of each symbol, comments stripped and the .LBB<n>_ block
labels' function number normalised (it counts the functions of a file, so it moves with the split).
usage: isa_same.py A.s [A2.s ...] -- B.s [B2.s ...]   (without "--": the first file is side A)
Prints the kernel and function counts, the symbols only one side has, those a side defines twice and
those that differ; exits 1 if any of the three lists is non-empty."""
import re
import sys


def functions(paths):
    """symbol -> instruction lines, the kernels among them, and the symbols defined more than once"""
    out, kernels, twice = {}, set(), []
    for path in paths:
        name = typed = None
        for line in open(path):
            m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", line)
            if m:
                kernels.add(m.group(1))
            m = re.match(r"\s*\.type\s+(\w+),@function", line)
            if m:
                typed = m.group(1)
            m = re.match(r"(\w+):", line)
            if name is None and m and m.group(1) == typed:
                name = typed
                if name in out:
                    twice.append(name)
                out[name] = []
            elif name is not None and line.startswith(".Lfunc_end"):
                name = None
            elif name is not None:
                text = re.sub(r"\.LBB\d+_", ".LBB_", line.split(";")[0]).strip()
                if text:
                    out[name].append(text)
    return out, kernels, twice


args = sys.argv[1:]
cut = args.index("--") if "--" in args else 1
(a, ka, ta), (b, kb, tb) = functions(args[:cut]), functions([p for p in args[cut:] if p != "--"])
only = sorted(set(a) ^ set(b))
differ = sorted(k for k in set(a) & set(b) if a[k] != b[k])
same = len(set(a) & set(b)) - len(differ)
print(f"A: {len(ka)} kernels, {len(a)} functions, {sum(map(len, a.values()))} instruction lines")
print(f"B: {len(kb)} kernels, {len(b)} functions, {sum(map(len, b.values()))} instruction lines")
print(f"identical: {same}   differ: {len(differ)}   on one side only: {len(only)}   defined twice: {len(ta) + len(tb)}")
for k in only:
    print("ONLY", "A" if k in a else "B", k)
for k in ta + tb:
    print("TWICE", k)
for k in differ:
    print("DIFFER", k, len(a[k]), len(b[k]))
sys.exit(1 if only or differ or ta or tb else 0)
