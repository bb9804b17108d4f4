"""What the index list costs and what it saves: rt_render_list_device against the existing entry points.

usage: python tools/list_timing.py [--scene bounce.txt] [--modes BRUTE,GROUPED,BVH] [--log2-n 18] [--spp 16] [--reps 7]
                                   [--tol 0.05] [--min 16] [--max 256] [--batch 16]

The surfels are what an equirectangular panorama from camera 0's position sees (tools/surfels_timing.py's:
a hit gives its position moved 1e-3 along the normal and the normal, a miss the ray's origin and minus its
direction), gathered by Lambert's cosine.  Per traversal mode, device entries, event-timed on one stream,
--reps alternating repetitions after warming, median and range as one JSON line each:
  identity  rt_render_list_device without a list and without moments against rt_render_surfels_device: the
            same launch and the same sums; the difference is the fold kernel.  With moments as a third call.
  half      rt_render_list_device over every second entry (an index list into the resident array) against
            rt_render_surfels_device over those entries compacted into an array of their own (which gives
            them other streams): what the list's indirection costs.
  adaptive  gather_adaptive (--tol, --min, --max, --batch) against rt_render_surfels_device at --max samples
            for every entry: wall-clock ms of two repetitions after a warming one, rays traced, the list sizes and
            the samples taken per entry.
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
    ap.add_argument("--modes", default="BRUTE,GROUPED,BVH")
    ap.add_argument("--log2-n", type=int, default=18)
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--tol", type=float, default=0.05)
    ap.add_argument("--min", type=int, default=16, dest="min_spp")
    ap.add_argument("--max", type=int, default=256, dest="max_spp")
    ap.add_argument("--batch", type=int, default=16)
    a = ap.parse_args(argv)

    import torch

    import raytracercore_amd as rc
    import render_panorama as pano

    if rc.device_count() < 1:
        raise RuntimeError("list_timing: no HIP device (a timing needs the GPU)")
    gather = rc.RT_GATHER_COSINE
    path = a.scene if os.path.exists(a.scene) else rc.scene_path(a.scene)
    scene = rc.SceneLoader.from_file(path)
    cam = scene.cameras[0]
    pos = np.array([cam.position.x, cam.position.y, cam.position.z])
    forward = np.array([cam.look_at.x, cam.look_at.y, cam.look_at.z]) - pos
    n, spp = 1 << a.log2_n, a.spp
    width = 1 << ((a.log2_n + 2) // 2)  # width x width / 2 pixels, at least n
    first = (width * (width // 2) - n) // 2 // width * width  # whole rows about the horizon
    o, d = (v[first:first + n] for v in pano.panorama_rays(pos, forward, width))
    modes = a.modes.split(",")
    gpu = rc.GpuRaytracer(scene, 0, traversal=getattr(rc, "RT_TRAVERSAL_" + modes[0]))
    hits = gpu.query_rays(o, d)
    gpu.close()
    hit = (hits["prim_id"] >= 0) & np.isfinite(hits["normal"]).all(axis=1)
    surfels = rc._pack_surfels(np.where(hit[:, None], hits["position"] + 1e-3 * hits["normal"], o[:, :3]).astype(np.float64),
                               np.where(hit[:, None], hits["normal"], -d[:, :3]).astype(np.float64))
    half = np.arange(0, n, 2, dtype=np.uint32)
    d_all = torch.from_numpy(surfels.view(np.uint8)).cuda()
    d_half = torch.from_numpy(np.ascontiguousarray(surfels[half]).view(np.uint8)).cuda()
    d_index = torch.from_numpy(half.view(np.int32)).cuda()
    acc = {"sum": torch.zeros(3 * n, dtype=torch.float64, device="cuda"),
           "ns": torch.zeros(n, dtype=torch.int32, device="cuda"), "ms": torch.zeros(n, dtype=torch.int32, device="cuda"),
           "q": torch.zeros(n, dtype=torch.float64, device="cuda"), "nb": torch.zeros(n, dtype=torch.int32, device="cuda")}
    d_count = torch.zeros(1, dtype=torch.int64, device="cuda")
    st = torch.cuda.Stream()
    base = dict(scene=os.path.basename(path), n=n, spp=spp, reps=a.reps)

    def timed(calls):
        traced = {}
        for key, fn in calls.items():  # warm: code objects, scratch buffers; and the calls' ray counts
            d_count.zero_()
            torch.cuda.synchronize()
            fn()
            st.synchronize()
            traced[key] = int(d_count.item())
        ms = {key: [] for key in calls}
        for _ in range(a.reps):
            for key, fn in calls.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(st)
                fn()
                e1.record(st)
                e1.synchronize()
                ms[key].append(e0.elapsed_time(e1))
        return {key: stats(v) for key, v in ms.items()}, traced, {key: float(np.median(v)) for key, v in ms.items()}

    for mode in modes:
        gpu = rc.GpuRaytracer(scene, 0, traversal=getattr(rc, "RT_TRAVERSAL_" + mode))
        assert gpu.info().traversal == getattr(rc, "RT_TRAVERSAL_" + mode)
        out = (acc["sum"], acc["ns"], acc["ms"])
        kw = dict(d_rays=d_count, stream=st.cuda_stream)
        S = rc.RT_LIST_SURFELS
        ms, traced, med = timed({
            "render_surfels": lambda: gpu.render_surfels_device(d_all, n, spp, 0, gather, 0, 0, *out, d_count, st.cuda_stream),
            "render_list": lambda: gpu.render_list_device(S, gather, d_all, n, None, n, spp, 0, 0, 0, *out, **kw),
            "render_list_moments": lambda: gpu.render_list_device(S, gather, d_all, n, None, n, spp, 0, 0, 0, *out, acc["q"],
                                                                  acc["nb"], **kw)})
        print(json.dumps(dict(base, what="identity", mode=mode, ms=ms, rays_traced=traced,
                              list_over_surfels=round(med["render_list"] / med["render_surfels"], 4),
                              moments_over_surfels=round(med["render_list_moments"] / med["render_surfels"], 4))), flush=True)
        m = half.size
        ms, traced, med = timed({
            "compacted": lambda: gpu.render_surfels_device(d_half, m, spp, 0, gather, 0, 0, *out, d_count, st.cuda_stream),
            "indexed": lambda: gpu.render_list_device(S, gather, d_all, n, d_index, m, spp, 0, 0, 0, *out, acc["q"], acc["nb"],
                                                      **kw)})
        print(json.dumps(dict(base, what="half", mode=mode, entries=m, ms=ms, rays_traced=traced,
                              indexed_over_compacted=round(med["indexed"] / med["compacted"], 4))), flush=True)
        top = -(-a.max_spp // a.batch) * a.batch
        wall = {"adaptive": [], "fixed": []}
        for rep in range(3):  # (the first repetition warms and is not kept)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = gpu.gather_adaptive(S, surfels, a.tol, a.min_spp, a.max_spp, a.batch, mode=gather, shape=(width, n // width))
            t1 = time.perf_counter()
            d_count.zero_()
            for k in acc.values():
                k.zero_()
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            gpu.render_surfels_device(d_all, n, top, 0, gather, 0, 0, *out, d_count, st.cuda_stream)
            st.synchronize()
            t3 = time.perf_counter()
            if rep:
                wall["adaptive"].append((t1 - t0) * 1e3)
                wall["fixed"].append((t3 - t2) * 1e3)
        taken = res["spp"].cpu().numpy()
        print(json.dumps(dict(base, what="adaptive", mode=mode, reps=2, tol=a.tol, min=a.min_spp, max=top, batch=a.batch,
                              ms={k: stats(v) for k, v in wall.items()}, rays={"adaptive": res["rays"], "fixed": int(d_count.item())},
                              rays_ratio=round(res["rays"] / max(int(d_count.item()), 1), 4), counts=res["counts"],
                              taken={"min": int(taken.min()), "mean": round(float(taken.mean()), 2), "max": int(taken.max())})),
              flush=True)
        gpu.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
