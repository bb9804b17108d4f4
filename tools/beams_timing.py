"""What a beam costs: rt_render_beams_device against rt_render_rays_device on the same n and spp.

usage: python tools/beams_timing.py [--scene bounce.txt] [--modes BRUTE,GROUPED,BVH] [--log2-n 20] [--spp 16] [--reps 7]

The rays are an equirectangular panorama from camera 0's position (tools/render_panorama.py), 2^log2-n of
them, row by row (the rows about the horizon when the panorama has more pixels); the beams are the same
pixels' (panorama_beams).  Per traversal mode, after warming both
calls: --reps alternating repetitions, each timed with device events on one stream; the median and the
range of each and the ratio of the medians are printed as one JSON line per mode.  The two calls do not
trace the same samples (a beam's samples spread over its pixel), so their ray counts are printed too.
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
    ap.add_argument("--modes", default="BRUTE,GROUPED,BVH")
    ap.add_argument("--log2-n", type=int, default=20)
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args(argv)

    import torch

    import raytracercore_amd as rc
    import render_panorama as pano

    if rc.device_count() < 1:
        raise RuntimeError("beams_timing: no HIP device (a timing needs the GPU)")
    path = a.scene if os.path.exists(a.scene) else rc.scene_path(a.scene)
    scene = rc.SceneLoader.from_file(path)
    cam = scene.cameras[0]
    pos = np.array([cam.position.x, cam.position.y, cam.position.z])
    forward = np.array([cam.look_at.x, cam.look_at.y, cam.look_at.z]) - pos
    n = 1 << a.log2_n
    width = 1 << ((a.log2_n + 2) // 2)  # width x width / 2 pixels, at least n
    assert width * (width // 2) >= n
    first = (width * (width // 2) - n) // 2 // width * width  # whole rows about the horizon
    sl = slice(first, first + n)
    o, d = pano.panorama_rays(pos, forward, width)
    rays = rc._pack_rays(o[sl], d[sl])
    bo, bd, bdu, bdv = pano.panorama_beams(pos, forward, width)
    z = np.zeros((n, 3))
    beams = rc._pack_beams(bo[sl], bd[sl], z, z, bdu[sl], bdv[sl])
    d_rays = torch.from_numpy(rays.view(np.uint8)).cuda()
    d_beams = torch.from_numpy(beams.view(np.uint8)).cuda()
    d_sum = torch.zeros(3 * n, dtype=torch.float64, device="cuda")
    d_ns = torch.zeros(n, dtype=torch.int32, device="cuda")
    d_ms = torch.zeros(n, dtype=torch.int32, device="cuda")
    d_count = torch.zeros(1, dtype=torch.int64, device="cuda")
    st = torch.cuda.Stream()
    for mode in a.modes.split(","):
        gpu = rc.GpuRaytracer(scene, 0, traversal=getattr(rc, "RT_TRAVERSAL_" + mode))
        assert gpu.info().traversal == getattr(rc, "RT_TRAVERSAL_" + mode)
        out = (d_sum.data_ptr(), d_ns.data_ptr(), d_ms.data_ptr(), d_count.data_ptr())
        calls = {"render_rays": lambda: gpu.render_rays_device(d_rays.data_ptr(), n, a.spp, 0, 0, 0, *out, stream=st.cuda_stream),
                 "render_beams": lambda: gpu.render_beams_device(d_beams.data_ptr(), n, a.spp, 0, 0, 0, *out, stream=st.cuda_stream)}
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
        gpu.close()
        rec = {"scene": os.path.basename(path), "mode": mode, "n": n, "spp": a.spp, "reps": a.reps,
               "ms": {key: stats(v) for key, v in ms.items()}, "rays_traced": traced,
               "beams_over_rays": round(float(np.median(ms["render_beams"]) / np.median(ms["render_rays"])), 4),
               "beams_over_rays_per_ray_traced": round(float(np.median(ms["render_beams"]) / traced["render_beams"] /
                                                             (np.median(ms["render_rays"]) / traced["render_rays"])), 4)}
        print(json.dumps(rec), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
