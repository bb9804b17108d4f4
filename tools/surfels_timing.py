"""What a surfel costs, and what it saves: rt_render_surfels against rt_render_rays on the same sample rays.

usage: python tools/surfels_timing.py [--scene bounce.txt] [--modes BRUTE,GROUPED,BVH] [--log2-n 20] [--spp 16]
                                      [--reps 7] [--gather diffuse|cosine|sphere] [--host-reps 3]

The surfels are what an equirectangular panorama from camera 0's position sees (tools/render_panorama.py,
2^log2-n pixels row by row): a hit gives its position moved 1e-3 along the normal and the normal, a miss
the ray's origin and minus its direction.  Device entries, per traversal mode: rt_render_surfels_device
(n surfels, spp samples) against rt_render_rays_device at spp 1 over the n x spp rays that
rt_debug_surfel_rays_device reports for them, so both trace the same first segments; after warming both,
--reps alternating repetitions, each timed with device events on one stream; median, range and the ratio
of the medians as one JSON line per mode, with both calls' ray counts.  Host entries, in the first mode:
rt_render_surfels (n surfels, spp) against rt_render_rays (n x spp rays, spp 1) on the same rays in host
memory, what a bake had to do before: wall-clock ms, --host-reps alternating repetitions.
"""
from __future__ import annotations

import argparse
import ctypes as C
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
    ap.add_argument("--log2-n", type=int, default=20)
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--gather", default="diffuse", choices=["diffuse", "cosine", "sphere"])
    ap.add_argument("--host-reps", type=int, default=3)
    a = ap.parse_args(argv)

    import torch

    import raytracercore_amd as rc
    import render_panorama as pano

    if rc.device_count() < 1:
        raise RuntimeError("surfels_timing: no HIP device (a timing needs the GPU)")
    gather = getattr(rc, "RT_GATHER_" + a.gather.upper())
    path = a.scene if os.path.exists(a.scene) else rc.scene_path(a.scene)
    scene = rc.SceneLoader.from_file(path)
    cam = scene.cameras[0]
    pos = np.array([cam.position.x, cam.position.y, cam.position.z])
    forward = np.array([cam.look_at.x, cam.look_at.y, cam.look_at.z]) - pos
    n, spp = 1 << a.log2_n, a.spp
    width = 1 << ((a.log2_n + 2) // 2)  # width x width / 2 pixels, at least n
    assert width * (width // 2) >= n
    first = (width * (width // 2) - n) // 2 // width * width  # whole rows about the horizon
    o, d = (v[first:first + n] for v in pano.panorama_rays(pos, forward, width))
    modes = a.modes.split(",")
    gpu = rc.GpuRaytracer(scene, 0, traversal=getattr(rc, "RT_TRAVERSAL_" + modes[0]))
    hits = gpu.query_rays(o, d)
    gpu.close()
    hit = (hits["prim_id"] >= 0) & np.isfinite(hits["normal"]).all(axis=1)
    surfels = rc._pack_surfels(np.where(hit[:, None], hits["position"] + 1e-3 * hits["normal"], o[:, :3]).astype(np.float64),
                               np.where(hit[:, None], hits["normal"], -d[:, :3]).astype(np.float64))
    d_surfels = torch.from_numpy(surfels.view(np.uint8)).cuda()
    d_rays = torch.empty(n * spp * 64, dtype=torch.uint8, device="cuda")
    rc._check(rc.load_library().rt_debug_surfel_rays_device(gather, C.c_void_p(d_surfels.data_ptr()), n, spp, 0, 0, 0,
                                                            C.c_void_p(d_rays.data_ptr()), None))
    torch.cuda.synchronize()
    m = n * spp
    d_sum = torch.zeros(3 * m, dtype=torch.float64, device="cuda")
    d_ns = torch.zeros(m, dtype=torch.int32, device="cuda")
    d_ms = torch.zeros(m, dtype=torch.int32, device="cuda")
    d_count = torch.zeros(1, dtype=torch.int64, device="cuda")
    st = torch.cuda.Stream()
    for mode in modes:
        gpu = rc.GpuRaytracer(scene, 0, traversal=getattr(rc, "RT_TRAVERSAL_" + mode))
        assert gpu.info().traversal == getattr(rc, "RT_TRAVERSAL_" + mode)
        out = (d_sum.data_ptr(), d_ns.data_ptr(), d_ms.data_ptr(), d_count.data_ptr())
        calls = {"render_rays": lambda: gpu.render_rays_device(d_rays.data_ptr(), m, 1, 0, 0, 0, *out, stream=st.cuda_stream),
                 "render_surfels": lambda: gpu.render_surfels_device(d_surfels, n, spp, 0, gather, 0, 0, *out, stream=st.cuda_stream)}
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
        rec = {"scene": os.path.basename(path), "entry": "device", "mode": mode, "gather": a.gather, "n": n, "spp": spp,
               "reps": a.reps, "ms": {key: stats(v) for key, v in ms.items()}, "rays_traced": traced,
               "surfels_over_rays": round(float(np.median(ms["render_surfels"]) / np.median(ms["render_rays"])), 4)}
        print(json.dumps(rec), flush=True)
    # the host entries: n records of 64 B and spp samples each, against n x spp records and one sample each
    del d_sum, d_ns, d_ms
    rays = np.empty(m, rc.RAY_DTYPE)
    rays.view(np.uint8).reshape(-1)[:] = d_rays.cpu().numpy()
    del d_rays
    gpu = rc.GpuRaytracer(scene, 0, traversal=getattr(rc, "RT_TRAVERSAL_" + modes[0]))
    out_s = (np.zeros((n, 3)), np.zeros(n, np.uint32), np.zeros(n, np.uint32))
    out_r = (np.zeros((m, 3)), np.zeros(m, np.uint32), np.zeros(m, np.uint32))
    calls = {"render_rays": lambda: gpu.render_rays(rays, None, 1, 0, out=out_r),
             "render_surfels": lambda: gpu.render_surfels(surfels, None, spp, 0, gather, out=out_s)}
    sec = {key: [] for key in calls}
    for rep in range(a.host_reps + 1):  # (the first repetition warms the staging buffers and is not kept)
        for key, fn in calls.items():
            t0 = time.perf_counter()
            fn()
            if rep:
                sec[key].append((time.perf_counter() - t0) * 1e3)
    gpu.close()
    rec = {"scene": os.path.basename(path), "entry": "host", "mode": modes[0], "gather": a.gather, "n": n, "spp": spp,
           "reps": a.host_reps, "input_MiB": {"render_rays": rays.nbytes >> 20, "render_surfels": surfels.nbytes >> 20},
           "ms": {key: stats(v) for key, v in sec.items()},
           "rays_over_surfels": round(float(np.median(sec["render_rays"]) / np.median(sec["render_surfels"])), 3)}
    print(json.dumps(rec), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
