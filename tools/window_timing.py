"""Diagnostic: the path kernel's time on windows of the C2 frame (bounce.txt camera 0, 1920x1080 x 256
spp) that the fp64 oracle's primary_ids class as all-miss, all-hit, and the whole frame.  The
all-miss windows price a camera sample that meets nothing (the scene bound's skip), the
all-hit window prices the guard that in-room waves pay.

usage: python tools/window_timing.py [--reps N] [--spp S] [--only NAME] [--scene die.txt]
       python tools/window_timing.py --pmc DIR     (per-dispatch counters of a rocprofv3 --pmc run of
                                                    this script with --reps 1, in window order)
RTCORE_LIB names the library build, RTCORE_SCENE_BOUND=0 turns the skip off."""
import argparse
import csv
import glob
import os
import sys

sys.path.insert(0, os.getcwd())

W, H = 1920, 1080
# (x0, y0, w, h), block-aligned; by the oracle's primary_ids at 1080p the image of bounce.txt's room
# spans x 575..1345, y 63..1017, and 640..1279 x 424..679 lies wholly inside it
WINDOWS = {
    "miss_top": (0, 0, 1920, 56),
    "miss_left": (0, 0, 568, 1080),
    "hit": (640, 424, 640, 256),
    "frame": (0, 0, 1920, 1080),
}


def pmc_report(d):
    rows = {}
    for f in glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            if "path_kernel" in r["Kernel_Name"] or "rt_path_const" in r["Kernel_Name"]:
                rows.setdefault(int(r["Dispatch_Id"]), {})[r["Counter_Name"]] = float(r["Counter_Value"])
    for k, disp in enumerate(sorted(rows)):
        c = rows[disp]
        print(f"dispatch {k} (id {disp}): " + " ".join(f"{n}={v:.6g}" for n, v in sorted(c.items())))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--spp", type=int, default=256)
    ap.add_argument("--only", default="")
    ap.add_argument("--scene", default="bounce.txt")
    ap.add_argument("--pmc", default="")
    a = ap.parse_args()
    if a.pmc:
        return pmc_report(a.pmc)
    import torch

    import raytracercore_amd as rc

    scene = rc.SceneLoader.from_file(rc.scene_path(a.scene))
    g = rc.GpuRaytracer(scene, 0, size=(W, H))
    dev = torch.device("cuda", 0)
    rays = torch.zeros(1, dtype=torch.int64, device=dev)
    print(f"lib={os.environ.get('RTCORE_LIB', '') or 'default'} bound={os.environ.get('RTCORE_SCENE_BOUND', 'default')} "
          f"scene={a.scene} spp={a.spp}", flush=True)
    for name, (x0, y0, w, h) in WINDOWS.items():
        if a.only and name != a.only:
            continue
        s_ = torch.zeros(3 * w * h, dtype=torch.float64, device=dev)
        n_ = torch.zeros(w * h, dtype=torch.int32, device=dev)
        m_ = torch.zeros(w * h, dtype=torch.int32, device=dev)
        ms = []
        for rep in range(a.reps + 1):  # the first is the warm-up
            rays.zero_()
            n_.zero_()
            m_.zero_()
            g.render_device(x0, y0, w, h, a.spp, 0, 0, s_.data_ptr(), n_.data_ptr(), m_.data_ptr(), rays.data_ptr(), 0)
            torch.cuda.synchronize()
            ms.append(g.last_kernel_ms())
        ms = ms[1:]
        smp = w * h * a.spp
        print(f"{name:9s} {w}x{h}+{x0}+{y0}: kernel ms min {min(ms):.4f} max {max(ms):.4f} | rays {int(rays.item())} "
              f"samples {smp} hits {int(n_.sum().item())} misses {int(m_.sum().item())} | "
              f"ns/sample {1e6 * min(ms) / smp:.4f} ns/ray {1e6 * min(ms) / max(1, int(rays.item())):.4f}", flush=True)
    g.close()


if __name__ == "__main__":
    main()
