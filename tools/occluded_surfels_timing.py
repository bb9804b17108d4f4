"""rt_occluded_surfels_device against the way to the same counts before it: rt_debug_surfel_rays_device into
an n x K ray buffer, then rt_occluded_rays_device over it with t_max as a full array.

usage: python tools/occluded_surfels_timing.py [--workloads bounce,die,mesh] [--k 4,16] [--reps 10] [--batch 20]
                                               [--size 1920 1080] [--variants LANES=1,REFILL=16] [--small]
                                               [--no-host]

Workloads: camera 0 of bounce.txt in BRUTE, of die.txt in GROUPED and of the 1001 x 501 mesh in BVH; the
surfels are the primary hits moved off their surface as tools/bake_ao.py moves them, in RT_GATHER_COSINE mode,
once with t_max of one scene unit and once with +inf (as arrays, for both ways).  Per workload, K and t_max,
after warming every call: --reps alternating repetitions of (a) the two launches of the yardstick, (b) its
any-hit launch alone and (c) the new entry, each a window of --batch calls between two device events on one
stream, reported per call as min .. max and median.  The counts of every timed window are compared with the
yardstick's (the new entry adds, so a window over zeroed counts must hold batch x them): differences counted.
--variants: the new entry again under each NAME=VALUE (several joined by +), which sets the planning switch
RTCORE_OCCLUDED_SURFELS_NAME (LANES, BLOCK: the brute-force kernels' unit; REFILL: the BVH kernel's refill
threshold), in the same alternation.  --small: 4096 of the surfels at 1024 samples, the few-entries case the
sample blocks exist for, with a block of all 1024 samples (the position's lanes own its entry), 64 and 16.
Then the host entries end to end: rt_occluded_surfels against rt_occluded_rays over the rays surfel_rays
reports (pageable numpy arrays, min .. max of 3).  Prints one JSON line per workload.
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

WORKLOADS = {"bounce": ("bounce.txt", "BRUTE"), "die": ("die.txt", "GROUPED"), "mesh": (None, "BVH")}
SEED = 1
ENV = "RTCORE_OCCLUDED_SURFELS_"
SWITCHES = ("LANES", "BLOCK", "REFILL")


def stats(ms):
    return {"min": round(min(ms), 3), "max": round(max(ms), 3), "median": round(float(np.median(ms)), 3)}


def device_case(rc, torch, gpu, st, d_surfels, n, k, t_max, reps, batch, variants):
    """One (K, t_max) case on the device; returns its record."""
    lib = gpu.lib
    d_tm = torch.full((n,), t_max, dtype=torch.float64, device="cuda")
    d_tm_rays = torch.full((n * k,), t_max, dtype=torch.float64, device="cuda")
    d_rays = torch.empty(n * k * rc.RAY_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    d_out = torch.empty(n * k, dtype=torch.uint8, device="cuda")
    d_occ = torch.zeros(n, dtype=torch.int32, device="cuda")

    def draw():
        rc._check(lib.rt_debug_surfel_rays_device(rc.RT_GATHER_COSINE, d_surfels.data_ptr(), n, k, SEED, 0, 0, d_rays.data_ptr(),
                                                  st.cuda_stream))

    def any_hit():
        gpu.occluded_rays_device(d_rays.data_ptr(), d_tm_rays.data_ptr(), n * k, d_out.data_ptr(), stream=st.cuda_stream)

    def both():
        draw()
        any_hit()

    def counts(variant):
        def call():
            for name in SWITCHES:
                os.environ.pop(ENV + name, None)
            for setting in filter(None, variant.split("+")):
                name, value = setting.split("=")
                os.environ[ENV + name] = value
            gpu.occluded_surfels_device(rc.RT_GATHER_COSINE, d_surfels, n, None, n, d_tm, k, SEED, 0, 0, d_occ, stream=st.cuda_stream)
        return call

    calls = {"draw_and_any_hit": both, "any_hit_alone": any_hit, "occluded_surfels": counts("")}
    for v in variants:
        calls["occluded_surfels " + v] = counts(v)
    with torch.cuda.stream(st):
        both()  # warm, and the yardstick's counts
        st.synchronize()
        want = d_out.view(n, k).sum(dim=1, dtype=torch.int32)
        differs = {}
        for key, fn in calls.items():
            if key.startswith("occluded_surfels"):
                d_occ.zero_()
                fn()
                st.synchronize()
                differs[key] = int((d_occ != want).sum().item())
        ms = {key: [] for key in calls}
        for _ in range(reps):
            for key, fn in calls.items():
                d_occ.zero_()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(st)
                for _ in range(batch):
                    fn()
                e1.record(st)
                e1.synchronize()
                ms[key].append(e0.elapsed_time(e1) / batch)
                if key.startswith("occluded_surfels"):  # every timed window's counts
                    differs[key] += int((d_occ != batch * want).sum().item())
                else:
                    differs[key] = differs.get(key, 0) + int((d_out.view(n, k).sum(dim=1, dtype=torch.int32) != want).sum().item())
    for name in SWITCHES:
        os.environ.pop(ENV + name, None)
    r = {key: stats(v) for key, v in ms.items()}
    r["count_differences"] = differs
    r["occluded_share"] = round(float(want.sum().item()) / (n * k), 4)
    return r


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workloads", default="bounce,die,mesh")
    ap.add_argument("--k", default="4,16")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--batch", type=int, default=20)
    ap.add_argument("--size", type=int, nargs=2, default=(1920, 1080))
    ap.add_argument("--variants", default="")
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--no-host", action="store_true")
    a = ap.parse_args(argv)

    import torch

    import bake_ao
    import raytracercore_amd as rc
    from raytracercore_amd.scenes import mesh_scene_text

    if rc.device_count() < 1:
        raise RuntimeError("occluded_surfels_timing: no HIP device (a timing needs the GPU)")
    ks = [int(v) for v in a.k.split(",") if v]
    variants = [v for v in a.variants.split(",") if v]
    for name in a.workloads.split(","):
        file, mode = WORKLOADS[name]
        scene = rc.SceneLoader.from_file(rc.scene_path(file)) if file else rc.SceneLoader.from_text(mesh_scene_text())
        gpu = rc.GpuRaytracer(scene, 0, size=tuple(a.size), traversal=getattr(rc, "RT_TRAVERSAL_" + mode))
        assert gpu.info().traversal == getattr(rc, "RT_TRAVERSAL_" + mode)
        _, pos, nrm = bake_ao.ao_surfels(gpu.query_rays(gpu.camera_rays()))
        surfels = rc._pack_surfels(pos, nrm)
        n = len(surfels)
        d_surfels = torch.from_numpy(surfels.view(np.uint8)).cuda()
        st = torch.cuda.Stream()
        rec = {"workload": name, "scene": file or "mesh 1001x501", "mode": mode, "size": list(a.size), "surfels": n, "batch": a.batch}
        for k in ks:
            for label, t_max in (("t_max=1", 1.0), ("t_max=inf", float("inf"))):
                rec[f"K={k} {label}"] = device_case(rc, torch, gpu, st, d_surfels, n, k, t_max, a.reps, a.batch,
                                                    [v for v in variants if ("REFILL" in v) == (mode == "BVH")])
        if a.small and mode != "BVH":
            m = 4096
            sub = np.ascontiguousarray(surfels[::max(1, n // m)][:m])
            d_sub = torch.from_numpy(sub.view(np.uint8)).cuda()
            rec["small 4096 x 1024 t_max=1"] = device_case(rc, torch, gpu, st, d_sub, len(sub), 1024, 1.0, a.reps, 2,
                                                           ["BLOCK=1024", "BLOCK=64", "BLOCK=16", "LANES=1", "LANES=64"])
        if not a.no_host:
            for k in ks:
                rays = gpu.surfel_rays(surfels, None, k, SEED, rc.RT_GATHER_COSINE)
                tm = np.full(rays.shape, 1.0)
                want = gpu.occluded_rays(rays, None, tm).sum(axis=1)  # (warm: staging, pages)
                got = gpu.occluded_surfels(surfels, None, k, SEED, rc.RT_GATHER_COSINE, t_max=1.0)[0]
                out = {"count_differences": int((got != want).sum())}
                for key in ("occluded_surfels", "occluded_rays"):
                    ts = []
                    for _ in range(3):
                        t0 = time.perf_counter()
                        if key == "occluded_surfels":
                            gpu.occluded_surfels(surfels, None, k, SEED, rc.RT_GATHER_COSINE, t_max=tm[:, 0])
                        else:
                            gpu.occluded_rays(rays, None, tm)
                        ts.append((time.perf_counter() - t0) * 1e3)
                    out[key] = stats(ts)
                rec[f"host_entry_ms K={k} t_max=1"] = out
                del rays, tm
        gpu.close()
        print(json.dumps(rec), flush=True)
        del d_surfels
        torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
