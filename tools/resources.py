#!/usr/bin/env python3
"""Register / occupancy / LDS report of every kernel of the kernel translation units (the Makefile's
KERNEL_SRCS), compiled for gfx950; run from the repository root."""
import re
import subprocess
import sys

KERNEL_SRCS = ["kernels_exact.hip", "kernels_path.hip", "kernels_query.hip", "kernels_fold.hip"]
extra = sys.argv[1:]
out = ""
for src in KERNEL_SRCS:
    cmd = ["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-slp-vectorize", "--offload-arch=gfx950", "-x", "hip",
           "-c", "raytracercore_amd/csrc/" + src, "-o", "/dev/null", "-Rpass-analysis=kernel-resource-usage"] + extra
    out += subprocess.run(cmd, capture_output=True, text=True).stderr
cur = None
rows = {}
for line in out.splitlines():
    m = re.search(r"remark: Function Name: (\S+)", line)
    if m:
        cur = m.group(1)
        k = re.search(r"N_1\d+(\w+?)I(.*?)EEEv", cur)
        cur = (k.group(1) + "<" + k.group(2) + ">") if k else cur[:40]
        rows[cur] = {}
        continue
    m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", line)
    if m and cur:
        rows[cur][m.group(1).strip()] = m.group(2)
for k, v in rows.items():
    print(f"{k:40s} VGPR {v.get('VGPRs','?'):>4} SGPR {v.get('SGPRs','?'):>4} spillV {v.get('VGPRs Spill','?'):>3} "
          f"spillS {v.get('SGPRs Spill','?'):>3} scratch {v.get('ScratchSize','?'):>4} occ {v.get('Occupancy','?')} "
          f"LDS {v.get('LDS Size','?')}")
