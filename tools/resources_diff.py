#!/usr/bin/env python3
"""Compare two -Rpass-analysis=kernel-resource-usage logs kernel by kernel (full mangled names).

usage: resources_diff.py PARENT.log BRANCH.log
Each log is the stderr of `hipcc ... -c FILE -o /dev/null -Rpass-analysis=kernel-resource-usage` for one kernel
translation unit or, one after the other in one log, for several (the Makefile's KERNEL_SRCS: kernels_exact.hip,
kernels_path.hip, kernels_query.hip, kernels_fold.hip; `make -C raytracercore_amd/csrc resources` shows the flags
and prints such a log).  Prints the kernels only one side has and
every figure that differs for a kernel both have; exit status 1 if a common kernel differs.
"""
import re
import sys


def parse(path):
    rows, cur = {}, None
    for line in open(path):
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = rows.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = int(m.group(2))
    return rows


def main():
    a, b = parse(sys.argv[1]), parse(sys.argv[2])
    bad = 0
    for k in sorted(set(a) - set(b)):
        print(f"only in {sys.argv[1]}: {k}")
    for k in sorted(set(b) - set(a)):
        v = b[k]
        print(f"new: {k}\n     VGPR {v.get('VGPRs')} AGPR {v.get('AGPRs')} SGPR {v.get('TotalSGPRs')} scratch {v.get('ScratchSize')} "
              f"occupancy {v.get('Occupancy')} LDS {v.get('LDS Size')}")
    common = sorted(set(a) & set(b))
    for k in common:
        if a[k] != b[k]:
            bad += 1
            print(f"DIFFERS: {k}\n  {a[k]}\n  {b[k]}")
    print(f"{len(common)} kernels in both logs, {len(common) - bad} identical in every figure, {bad} differ")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
