"""What falloff obscurance costs: rt_obscurance_surfels_device against rt_occluded_surfels_device at the same
surfels and samples, its two fold layouts against each other, and the adaptive loop against a fixed bake.

usage: python tools/obscurance_timing.py [--scene bounce.txt | --mesh] [--mode BRUTE] [--n 4096,262144] [--spp 64]
                                         [--radius 1.0] [--power 1] [--prim P] [--flip] [--reps 5]
                                         [--loop WIDTH] [--tol 0.02 --min 32 --max 256 --batch 16]

One process per scene; the surfels are the texel centres of triangle primitive P (tools/shade_probes.py),
RT_GATHER_COSINE.  Device events on one stream round every timed window, every window warmed once, the windows
alternating in one process, medians of --reps.  Per n:
  counts       rt_occluded_surfels_device with t_max = radius: the any-hit yardstick
  wave         rt_obscurance_surfels_device, the wave-per-entry fold (the default)
  thread       the same with RTCORE_OBSCURANCE_FOLD=thread: the thread-per-entry fold
  rays_query   rt_debug_surfel_rays_device + rt_query_rays_device over the same samples in one piece: the call
               without its fold (and without its chunking), so wave - rays_query estimates the fold
and, for power 0, how many samples differ between `hits` and the counts.  With --loop WIDTH: bake_ao's camera-0
surfels at that image width, obscurance_adaptive against one call of --max samples, in samples and in wall time
(the loop reads a count every iteration, so it is timed on the host, after a warm-up of both).
One JSON line per n and one for the loop.
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


def timed(torch, st, runs, order, reps):
    """Lists of milliseconds per window: every window warmed once, then reps rounds in `order`."""
    ms = {key: [] for key in order}
    with torch.cuda.stream(st):
        for key in order:
            runs[key]()
        st.synchronize()
        for _ in range(reps):
            for key in order:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(st)
                runs[key]()
                e1.record(st)
                e1.synchronize()
                ms[key].append(e0.elapsed_time(e1))
    return ms


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scene", default="bounce.txt")
    ap.add_argument("--mesh", action="store_true")
    ap.add_argument("--mode", default="BRUTE", choices=["BRUTE", "GROUPED", "BVH"])
    ap.add_argument("--n", default="4096,262144")
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--radius", type=float, default=1.0)
    ap.add_argument("--power", type=int, default=1)
    ap.add_argument("--prim", type=int)
    ap.add_argument("--flip", action="store_true")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--loop", type=int, default=0, metavar="WIDTH")
    ap.add_argument("--tol", type=float, default=0.02)
    ap.add_argument("--min", type=int, default=32, dest="min_spp")
    ap.add_argument("--max", type=int, default=256, dest="max_spp")
    ap.add_argument("--batch", type=int, default=16)
    a = ap.parse_args(argv)

    import torch

    import raytracercore_amd as rc
    from shade_probes import first_triangle, load_scene, texel_surfels

    if rc.device_count() < 1:
        raise RuntimeError("obscurance_timing: no HIP device (a timing needs the GPU)")
    scene, name = load_scene(rc, a.scene, a.mesh)
    p = first_triangle(rc, scene) if a.prim is None else a.prim
    gpu = rc.GpuRaytracer(scene, 0, traversal=getattr(rc, "RT_TRAVERSAL_" + a.mode))
    assert gpu.info().traversal == getattr(rc, "RT_TRAVERSAL_" + a.mode)
    st = torch.cuda.Stream()
    s = st.cuda_stream
    P = rc.obscurance_params(a.radius, a.power)
    COS = rc.RT_GATHER_COSINE

    def fold(layout):
        if layout == "thread":
            os.environ["RTCORE_OBSCURANCE_FOLD"] = "thread"
        else:
            os.environ.pop("RTCORE_OBSCURANCE_FOLD", None)

    for n in (int(v) for v in a.n.split(",") if v):
        w = 1 << ((n.bit_length() - 1) // 2)
        h = n // w
        pos, nrm = texel_surfels(scene.prims[p], w, h, 1e-3, a.flip)
        n = w * h
        d_surfels = torch.from_numpy(rc._pack_surfels(pos.reshape(-1, 3), nrm.reshape(-1, 3)).view(np.uint8)).cuda()
        d_acc = torch.zeros((n, 48), dtype=torch.uint8, device="cuda")
        d_occ, d_ns = (torch.zeros(n, dtype=torch.int32, device="cuda") for _ in range(2))
        d_t = torch.full((n,), a.radius, dtype=torch.float64, device="cuda")
        d_rays = torch.empty((n * a.spp, 64), dtype=torch.uint8, device="cuda")
        d_hits = torch.empty((n * a.spp, 48), dtype=torch.uint8, device="cuda")

        def obscurance(layout, par=P):
            fold(layout)
            gpu.obscurance_surfels_device(COS, d_surfels, n, None, n, par, a.spp, 0, 0, 0, d_acc, stream=s)
            fold("wave")

        def rays_query():
            rc._check(gpu.lib.rt_debug_surfel_rays_device(COS, d_surfels.data_ptr(), n, a.spp, 0, 0, 0, d_rays.data_ptr(), s))
            gpu.query_rays_device(d_rays.data_ptr(), n * a.spp, d_hits.data_ptr(), stream=s)

        runs = {
            "counts": lambda: gpu.occluded_surfels_device(COS, d_surfels, n, None, n, d_t, a.spp, 0, 0, 0, d_occ, d_ns, stream=s),
            "wave": lambda: obscurance("wave"),
            "thread": lambda: obscurance("thread"),
            "rays_query": rays_query,
        }
        ms = timed(torch, st, runs, ("counts", "wave", "thread", "rays_query"), a.reps)
        # power 0 on fresh arrays: `hits` against the any-hit counts
        d_acc.zero_()
        d_occ.zero_()
        with torch.cuda.stream(st):
            obscurance("wave", rc.obscurance_params(a.radius, 0))
            runs["counts"]()
        st.synchronize()
        acc = d_acc.cpu().numpy().reshape(-1).view(rc.OBSCURANCE_DTYPE)
        occ = d_occ.cpu().numpy().view(np.uint32).astype(np.int64)
        med = {key: float(np.median(v)) for key, v in ms.items()}
        print(json.dumps({"scene": name, "mode": a.mode, "n": n, "spp": a.spp, "radius": a.radius, "power": a.power, "reps": a.reps,
                          "prim": p, "ms": {key: stats(v) for key, v in ms.items()},
                          "wave_over_counts": round(med["wave"] / med["counts"], 3),
                          "thread_over_wave": round(med["thread"] / med["wave"], 3),
                          "fold_share_wave": round(max(0.0, med["wave"] - med["rays_query"]) / med["wave"], 3),
                          "fold_share_thread": round(max(0.0, med["thread"] - med["rays_query"]) / med["thread"], 3),
                          "hit_share": round(float(acc["hits"].sum()) / float(n * a.spp), 4),
                          "samples_differing_from_counts": int(np.abs(acc["hits"].astype(np.int64) - occ).sum())}), flush=True)
        del d_surfels, d_acc, d_occ, d_ns, d_t, d_rays, d_hits

    if a.loop:
        from bake_ao import ao_surfels

        height = max(1, round(a.loop * scene.params.height / max(1, scene.params.width)))
        cam = rc.GpuRaytracer(scene, 0, size=(a.loop, height), traversal=getattr(rc, "RT_TRAVERSAL_" + a.mode))
        _, pos, nrm = ao_surfels(cam.query_rays(cam.camera_rays()))
        up = -(-a.max_spp // a.batch) * a.batch
        wall = {"adaptive": [], "fixed": []}
        for rep in range(a.reps + 1):  # (the first round warms both)
            for key in ("adaptive", "fixed"):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                if key == "adaptive":
                    out = cam.obscurance_adaptive(pos, nrm, a.tol, a.min_spp, a.max_spp, a.batch, radius=a.radius, power=a.power)
                else:
                    fixed = cam.obscurance_surfels(pos, nrm, up, 0, a.radius, a.power)
                torch.cuda.synchronize()
                if rep:
                    wall[key].append(1e3 * (time.perf_counter() - t0))
        acc = out["acc"].cpu().numpy().reshape(-1).view(rc.OBSCURANCE_DTYPE)
        err = np.abs(rc.ambient_access(acc) - rc.ambient_access(fixed))
        print(json.dumps({"scene": name, "mode": a.mode, "loop_width": a.loop, "surfels": len(pos), "tol": a.tol, "min": a.min_spp,
                          "max": up, "batch": a.batch, "iterations": len(out["counts"]),
                          "samples_adaptive": int(acc["samples"].sum()), "samples_fixed": int(fixed["samples"].sum()),
                          "sample_share": round(float(acc["samples"].sum()) / float(fixed["samples"].sum()), 4),
                          "wall_ms": {key: stats(v) for key, v in wall.items()},
                          "adaptive_over_fixed": round(float(np.median(wall["adaptive"]) / np.median(wall["fixed"])), 3),
                          "max_abs_difference": round(float(err.max()), 4), "mean_abs_difference": round(float(err.mean()), 5)}),
              flush=True)
        cam.close()
    gpu.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
