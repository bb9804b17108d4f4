"""Diagnostic: do consecutive path kernels overlap?  Reads the kernel trace of a rocprofv3 --kernel-trace run
(every *kernel_trace.csv under DIR) and reports, for the kernels whose name contains NAME (default rt_path):
the hardware queues they were dispatched on, how many began before the one before them (by start time) had
ended and by how much, and the summed kernel time of all kernels per path kernel (one per step).
usage: python tools/kernel_overlap.py DIR [NAME]"""
import csv
import glob
import os
import sys

root = sys.argv[1]
name = sys.argv[2] if len(sys.argv) > 2 else "rt_path"
rows = []
for f in glob.glob(os.path.join(root, "**", "*kernel_trace.csv"), recursive=True):
    rows += list(csv.DictReader(open(f)))
if not rows:
    raise SystemExit(f"no *kernel_trace.csv under {root}")
for r in rows:
    r["t0"], r["t1"] = int(r["Start_Timestamp"]), int(r["End_Timestamp"])
path = sorted((r for r in rows if name in r["Kernel_Name"]), key=lambda r: r["t0"])
if len(path) < 2:
    raise SystemExit(f"fewer than two kernels named *{name}* among {len(rows)} dispatches")
queues = {}
for r in path:
    queues[r["Queue_Id"]] = queues.get(r["Queue_Id"], 0) + 1
print(f"{len(path)} {name} kernels of {len(rows)} dispatches; per hardware queue: {queues}")
others = {}
for r in rows:
    if name not in r["Kernel_Name"] and r["t0"] >= path[0]["t0"]:
        key = (r["Kernel_Name"].split("(")[0][-40:], r["Queue_Id"])
        others[key] = others.get(key, 0) + 1
for (kn, q), c in sorted(others.items(), key=lambda kv: -kv[1])[:6]:
    print(f"  other kernels from the first one on: {c} x {kn} on queue {q}")
by_queue = {}
for a, b in zip(path, path[1:]):
    d = by_queue.setdefault(b["Queue_Id"], [0, 0])
    d[0] += 1
    d[1] += b["t0"] < a["t1"]
print("  began before the previous ended, by the later kernel's queue:", {q: f"{v[1]} of {v[0]}" for q, v in by_queue.items()})
gaps = [(b["t0"] - a["t1"]) * 1e-3 for a, b in zip(path, path[1:])]  # us; negative: began before the last one ended
over = [g for g in gaps if g < 0]
print(f"pairs in which the next kernel began before the previous ended: {len(over)} of {len(gaps)}")
if over:
    over.sort()
    print(f"  overlap us: median {-over[len(over) // 2]:.1f}, longest {-over[0]:.1f}, shortest {-over[-1]:.1f}")
idle = sorted(g for g in gaps if g >= 0)
if idle:
    print(f"  gap us of the others: median {idle[len(idle) // 2]:.1f}, shortest {idle[0]:.1f}, longest {idle[-1]:.1f}")
dur = sorted((r["t1"] - r["t0"]) * 1e-6 for r in path)
print(f"{name} duration ms: median {dur[len(dur) // 2]:.4f}, min {dur[0]:.4f}, max {dur[-1]:.4f}")
total = sum((r["t1"] - r["t0"]) for r in rows if r["t0"] >= path[0]["t0"]) * 1e-6
print(f"kernel time of all kernels from the first {name} on: {total / len(path):.4f} ms per {name} kernel; "
      f"wall first start to last end: {(max(r['t1'] for r in rows) - path[0]['t0']) * 1e-6 / len(path):.4f} ms each")
