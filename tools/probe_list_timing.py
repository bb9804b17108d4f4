"""What the adaptive probes cost: rt_render_probe_list_device against rt_render_probes_device, and an adaptive
bake against a fixed one.

usage: python tools/probe_list_timing.py [--scene bounce.txt | --mesh] [--mode BRUTE] [--n 4096,65536] [--spp 64,1024]
                                         [--reps 3] [--only a,b,c,d,e] [--tol 0.1] [--min 64] [--batch 64]

The probes are tools/probes_timing.py's: the cell centres of a cubic grid over the scene's bound, the first n of
them, x fastest.  Per (n, spp), on one stream, device events round every timed window, after warming each:
  (a) rt_render_probes_device: n probes, spp samples.  With RTCORE_LIB naming a build of the parent commit and
      --only a this is the parent's number (that build has none of the entries below).
  (b) rt_render_probe_list_device with the identity list and no moments: the same launch, the templated fold.
  (c) the same with moments.
  (d) the same with a list of every second entry: half the work, the records and accumulators strided.
  (e) bake_probes_adaptive(--tol, --min, max = spp, --batch) against (c) at spp: wall time of the whole loop
      (host synchronisation included: one 4-byte read per iteration), samples and rays traced.
(b), (c) against (a): sh, the counts and the ray count are compared bit for bit.  One JSON line per (n, spp).
The fold kernels' own times are not in these windows: read them from a kernel trace taken in a run of its own
(rocprofv3 --kernel-trace --stats -- python tools/probe_list_timing.py --only c ...), the rows
accumulate_probes_kernel and accumulate_probe_list_kernel<1>.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def stats(ms):
    return {"min": round(min(ms), 3), "max": round(max(ms), 3), "median": round(float(np.median(ms)), 3)}


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scene", default="bounce.txt")
    ap.add_argument("--mesh", action="store_true")
    ap.add_argument("--mode", default="BRUTE", choices=["BRUTE", "GROUPED", "BVH"])
    ap.add_argument("--n", default="4096,65536")
    ap.add_argument("--spp", default="64,1024")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--only", default="a,b,c,d,e")
    ap.add_argument("--tol", type=float, default=0.1)
    ap.add_argument("--min", type=int, default=64, dest="min_spp")
    ap.add_argument("--batch", type=int, default=64)
    a = ap.parse_args(argv)

    import torch

    import raytracercore_amd as rc
    from bake_probes import probe_grid

    if rc.device_count() < 1:
        raise RuntimeError("probe_list_timing: no HIP device (a timing needs the GPU)")
    if a.mesh:
        from raytracercore_amd.scenes import mesh_scene_text

        scene, name = rc.SceneLoader.from_text(mesh_scene_text()), "mesh"
    else:
        path = a.scene if os.path.exists(a.scene) else rc.scene_path(a.scene)
        scene, name = rc.SceneLoader.from_file(path), os.path.basename(path)
    b = rc.scene_bound(list(scene.prims))
    lo, hi = np.array(b["lo"], np.float64), np.array(b["hi"], np.float64)
    pad = 0.05 * (hi - lo)
    sizes = [int(v) for v in a.n.split(",")]
    side = int(np.ceil(max(sizes) ** (1.0 / 3.0)))
    grid = probe_grid(list(lo + pad) + list(hi - pad), (side, side, side))
    which = a.only.split(",")
    gpu = rc.GpuRaytracer(scene, 0, traversal=getattr(rc, "RT_TRAVERSAL_" + a.mode))
    assert gpu.info().traversal == getattr(rc, "RT_TRAVERSAL_" + a.mode)
    st = torch.cuda.Stream()
    for n in sizes:
        probes = rc._pack_surfels(grid[:n], np.tile([0.0, 0.0, 1.0], (n, 1)))
        d_probes = torch.from_numpy(probes.view(np.uint8)).cuda()
        d_half = torch.arange(0, n, 2, dtype=torch.int32, device="cuda")
        for spp in (int(v) for v in a.spp.split(",")):
            if 64 * ((n + 63) // 64) * (1 << (spp - 1).bit_length()) > 1 << 26:
                print(json.dumps({"scene": name, "n": n, "spp": spp, "skipped": "above one launch's 2^26 work items"}), flush=True)
                continue
            acc = {k: (torch.zeros((n, 9, 4), dtype=torch.float64, device="cuda"), torch.zeros(n, dtype=torch.int32, device="cuda"),
                       torch.zeros(n, dtype=torch.int32, device="cuda"), torch.zeros((n, 4, 2), dtype=torch.float64, device="cuda"))
                   for k in "abcd"}
            d_count = torch.zeros(1, dtype=torch.int64, device="cuda")

            def zero(key):
                for t in acc[key]:
                    t.zero_()

            def run_a():
                zero("a")
                sh, ns, nm, _ = acc["a"]
                gpu.render_probes_device(d_probes, n, spp, 0, 0, 0, sh, ns, nm, d_count, stream=st.cuda_stream)

            def run_list(key, index, moments):
                zero(key)
                sh, ns, nm, mom = acc[key]
                gpu.render_probe_list_device(d_probes, n, index, n if index is None else index.numel(), spp, 0, 0, 0, sh, ns, nm,
                                             mom if moments else 0, d_count, stream=st.cuda_stream)

            runs = {"a": run_a, "b": lambda: run_list("b", None, False), "c": lambda: run_list("c", None, True),
                    "d": lambda: run_list("d", d_half, True)}
            keys = [k for k in which if k in runs]
            ms, traced = {}, {}
            with torch.cuda.stream(st):
                for key in keys:  # warm, and the calls' ray counts
                    d_count.zero_()
                    runs[key]()
                    st.synchronize()
                    traced[key] = int(d_count.item())
                    ms[key] = []
                for _ in range(a.reps):
                    for key in keys:
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record(st)
                        runs[key]()
                        e1.record(st)
                        e1.synchronize()
                        ms[key].append(e0.elapsed_time(e1))
            checks = {}
            for key in ("b", "c"):
                if "a" in keys and key in keys:
                    checks[key + "_equals_a"] = bool(all(torch.equal(x, y) for x, y in zip(acc["a"][:3], acc[key][:3]))
                                                     and traced["a"] == traced[key])
            if "c" in keys and "d" in keys:
                checks["d_equals_c_at_its_entries"] = bool(all(torch.equal(x[::2], y[::2]) for x, y in zip(acc["c"], acc["d"])))
            rec = {"scene": name, "mode": a.mode, "n": n, "spp": spp, "reps": a.reps, "ms": {k: stats(v) for k, v in ms.items()},
                   "rays_traced": traced, "checks": checks}
            if "e" in which and a.min_spp <= spp:
                with torch.cuda.stream(st):
                    wall = []
                    for _ in range(a.reps + 1):  # (the first warms)
                        st.synchronize()
                        t0 = time.perf_counter()
                        res = gpu.bake_probes_adaptive(probes, a.tol, a.min_spp, spp, a.batch, seed=0)
                        wall.append((time.perf_counter() - t0) * 1e3)
                taken = res["spp"].cpu().numpy()
                rec["adaptive"] = {"rel_tol": a.tol, "min": a.min_spp, "max": spp, "batch": a.batch, "wall_ms": stats(wall[1:]),
                                   "iterations": len(res["counts"]), "samples": int(taken.sum()), "samples_fixed": n * spp,
                                   "stopped_early": int((taken < res["params"].max_samples).sum()), "rays": res["rays"],
                                   "rays_fixed": traced.get("c")}
            print(json.dumps(rec), flush=True)
    gpu.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
