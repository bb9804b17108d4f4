"""What lighting points from a probe grid costs: rt_shade_probes_device against the gather it replaces.

usage: python tools/shade_probes_timing.py [--scene bounce.txt | --mesh] [--mode BRUTE] [--grid 8,32] [--n 4096,1048576]
                                           [--spp 64] [--prim P] [--flip] [--reps 3]

The grid is G x G x G probes over the scene's bound shrunk by 5 % (tools/shade_probes.py), baked once per G with
--spp samples; the points are the texel centres of triangle primitive P (default the scene's first; --flip: on
its other side), n of them as a 2^a x 2^b raster, 1e-3 off the surface.  Per (G, n), on one stream, device events
round every timed window, after warming each, the windows alternating:
  pass      rt_shade_probes_device with RT_PROBE_GRID_VISIBILITY: per chunk of 2^16 points the segment kernel, the
            any-hit launch over 8 n segments and the blend
  blend     rt_shade_probes_device without the flag: the blend kernel alone
  segments  rt_debug_probe_segments_device: the segment kernel over all n points in one launch
  anyhit    rt_occluded_rays_device over those 8 n segments
  gather    rt_render_surfels_device, RT_GATHER_COSINE, --spp samples at the same points: the existing way to the
            same quantity (irradiance = pi x gather_mean)
pass is close to segments + anyhit + blend; what is left is the chunking.  The results are compared: the pass
against rt_debug_shade_probes' twin is the tests' business, here only the share of points with weight < 1 and 0.
One JSON line per (G, n).
"""
from __future__ import annotations

import argparse
import json
import os
import sys

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
    ap.add_argument("--grid", default="8,32")
    ap.add_argument("--n", default="4096,1048576")
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--prim", type=int)
    ap.add_argument("--flip", action="store_true")
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args(argv)

    import torch

    import raytracercore_amd as rc
    from shade_probes import bake_grid_device, first_triangle, load_scene, scene_grid, texel_surfels

    if rc.device_count() < 1:
        raise RuntimeError("shade_probes_timing: no HIP device (a timing needs the GPU)")
    scene, name = load_scene(rc, a.scene, a.mesh)
    p = first_triangle(rc, scene) if a.prim is None else a.prim
    amb = scene.params.ambient
    gpu = rc.GpuRaytracer(scene, 0, traversal=getattr(rc, "RT_TRAVERSAL_" + a.mode))
    assert gpu.info().traversal == getattr(rc, "RT_TRAVERSAL_" + a.mode)
    st = torch.cuda.Stream()
    for G in (int(v) for v in a.grid.split(",")):
        grid, positions = scene_grid(rc, scene, (G, G, G), bias=0.0)
        flat, _ = scene_grid(rc, scene, (G, G, G), visibility=False)
        d_L, bake_rays = bake_grid_device(rc, torch, gpu, positions, a.spp, 0, amb)
        for n in (int(v) for v in a.n.split(",")):
            w = 1 << ((n.bit_length() - 1) // 2)
            h = n // w
            pos, nrm = texel_surfels(scene.prims[p], w, h, 1e-3, a.flip)
            n = w * h
            d_pts = torch.from_numpy(rc._pack_surfels(pos.reshape(-1, 3), nrm.reshape(-1, 3)).view(np.uint8)).cuda()
            d_E = torch.empty((n, 3), dtype=torch.float64, device="cuda")
            d_W = torch.empty(n, dtype=torch.float64, device="cuda")
            d_rays = torch.empty(n * 8 * 64, dtype=torch.uint8, device="cuda")
            d_t = torch.empty(n * 8, dtype=torch.float64, device="cuda")
            d_occ = torch.empty(n * 8, dtype=torch.uint8, device="cuda")
            d_sum = torch.zeros(3 * n, dtype=torch.float64, device="cuda")
            d_ns, d_nm = (torch.zeros(n, dtype=torch.int32, device="cuda") for _ in range(2))
            s = st.cuda_stream
            runs = {
                "pass": lambda: gpu.shade_probes_device(grid, d_L, d_pts, n, d_E, d_W, stream=s),
                "blend": lambda: gpu.shade_probes_device(flat, d_L, d_pts, n, d_E, 0, stream=s),
                "segments": lambda: rc._check(gpu.lib.rt_debug_probe_segments_device(
                    rc.C.byref(grid), rc.C.c_void_p(d_pts.data_ptr()), n, rc.C.c_void_p(d_rays.data_ptr()),
                    rc.C.c_void_p(d_t.data_ptr()), rc.C.c_void_p(s))),
                "anyhit": lambda: gpu.occluded_rays_device(d_rays.data_ptr(), d_t.data_ptr(), n * 8, d_occ.data_ptr(), stream=s),
                "gather": lambda: gpu.render_surfels_device(d_pts, n, a.spp, 0, rc.RT_GATHER_COSINE, 0, 0, d_sum, d_ns, d_nm, stream=s),
            }
            order = ("segments", "anyhit", "blend", "pass", "gather")
            ms = {key: [] for key in order}
            with torch.cuda.stream(st):
                for key in order:  # warm
                    runs[key]()
                st.synchronize()
                weight = d_W.cpu().numpy()
                occluded = int(d_occ.sum(dtype=torch.int64).item())
                for _ in range(a.reps):
                    for key in order:
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record(st)
                        runs[key]()
                        e1.record(st)
                        e1.synchronize()
                        ms[key].append(e0.elapsed_time(e1))
            med = {key: float(np.median(v)) for key, v in ms.items()}
            rec = {"scene": name, "mode": a.mode, "grid": G, "n": n, "spp": a.spp, "reps": a.reps, "prim": p,
                   "ms": {key: stats(v) for key, v in ms.items()},
                   "pass_over_gather": round(med["pass"] / med["gather"], 4),
                   "parts_of_pass": {key: round(med[key] / med["pass"], 4) for key in ("segments", "anyhit", "blend")},
                   "segments_occluded": occluded, "weight_below_1": round(float((weight < 1 - 1e-12).mean()), 4),
                   "weight_0": round(float((weight == 0).mean()), 4), "bake_rays": bake_rays}
            print(json.dumps(rec), flush=True)
            del d_pts, d_E, d_W, d_rays, d_t, d_occ, d_sum, d_ns, d_nm
    gpu.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
