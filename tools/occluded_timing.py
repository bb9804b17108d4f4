"""rt_occluded_rays_device against the way the same question was answered before it: rt_query_rays_device
(RT_QUERY_FAST) on the same device ray buffer, with the comparison of `distance` left out of the timing.

usage: python tools/occluded_timing.py [--workloads bounce,die,mesh] [--reps 10] [--batch 1] [--rays-per-hit 4]
                                       [--size 1920 1080] [--no-host]

Workloads: camera 0 of bounce.txt in BRUTE, of die.txt in GROUPED and of the 1001 x 501 mesh in BVH; the
occlusion rays are tools/bake_ao.py's (cosine-distributed about each primary hit's normal), once with t_max
of one scene unit and once unbounded.  Per workload and t_max, after warming every call: --reps alternating
repetitions of the closest-hit call, the any-hit call and the any-hit call with the records outside the
main loop tested last (RTCORE_OCCLUDED_EARLY=0), each timed with device events on one stream (a window is
--batch calls back to back, reported per call); the range (min .. max) and the median of each are printed,
and the answers of the timed runs are compared: occluded == (prim_id >= 0 and distance < (float)t_max),
the differences counted and held against the slack of the box culling.  Then the host entries end to end
(rt_occluded_rays against rt_query_rays plus the comparison, pageable numpy arrays).  Prints one JSON
line per workload.
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


def stats(ms):
    return {"min": round(min(ms), 3), "max": round(max(ms), 3), "median": round(float(np.median(ms)), 3)}


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workloads", default="bounce,die,mesh")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--rays-per-hit", type=int, default=4)
    ap.add_argument("--size", type=int, nargs=2, default=(1920, 1080))
    ap.add_argument("--no-host", action="store_true")
    a = ap.parse_args(argv)

    import torch

    import bake_ao
    import raytracercore_amd as rc
    from raytracercore_amd.scenes import mesh_scene_text

    if rc.device_count() < 1:
        raise RuntimeError("occluded_timing: no HIP device (a timing needs the GPU)")
    for name in a.workloads.split(","):
        file, mode = WORKLOADS[name]
        scene = rc.SceneLoader.from_file(rc.scene_path(file)) if file else rc.SceneLoader.from_text(mesh_scene_text())
        gpu = rc.GpuRaytracer(scene, 0, size=tuple(a.size), traversal=getattr(rc, "RT_TRAVERSAL_" + mode))
        assert gpu.info().traversal == getattr(rc, "RT_TRAVERSAL_" + mode)
        primary = gpu.query_rays(gpu.camera_rays())
        _, o, d = bake_ao.ao_rays(primary, a.rays_per_hit, 1)
        rays = rc._pack_rays(o, d)
        n = len(rays)
        del o, d
        d_rays = torch.from_numpy(rays.view(np.uint8)).cuda()
        d_hits = torch.empty(n * rc.HIT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        d_out = torch.empty(n, dtype=torch.uint8, device="cuda")
        st = torch.cuda.Stream()
        rec = {"workload": name, "scene": file or "mesh 1001x501", "mode": mode, "size": list(a.size), "rays": n, "batch": a.batch,
               "primary_hits": int((primary["prim_id"] >= 0).sum())}
        for label, t_max in (("t_max=1", 1.0), ("t_max=inf", None)):
            d_tm = torch.full((n,), t_max, dtype=torch.float64, device="cuda") if t_max is not None else None
            tm_ptr = d_tm.data_ptr() if d_tm is not None else 0

            def closest():
                gpu.query_rays_device(d_rays.data_ptr(), n, d_hits.data_ptr(), stream=st.cuda_stream)

            def any_hit(late):
                if late:
                    os.environ["RTCORE_OCCLUDED_EARLY"] = "0"
                else:
                    os.environ.pop("RTCORE_OCCLUDED_EARLY", None)
                gpu.occluded_rays_device(d_rays.data_ptr(), tm_ptr, n, d_out.data_ptr(), stream=st.cuda_stream)

            calls = {"closest_hit": closest, "any_hit": lambda: any_hit(False), "any_hit_late": lambda: any_hit(True)}
            answers = {}
            for key, fn in calls.items():  # warm: code objects, scratch buffers
                fn()
                st.synchronize()
                if key != "closest_hit":
                    answers[key] = d_out.cpu().numpy().astype(bool)
            ms = {key: [] for key in calls}
            for _ in range(a.reps):
                for key, fn in calls.items():
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(st)
                    for _ in range(a.batch):
                        fn()
                    e1.record(st)
                    e1.synchronize()
                    ms[key].append(e0.elapsed_time(e1) / a.batch)
                    if key != "closest_hit":  # the timed runs' answers, every repetition
                        assert np.array_equal(d_out.cpu().numpy().astype(bool), answers[key]), (name, label, key)
            hits = d_hits.cpu().numpy().view(rc.HIT_DTYPE)
            bound = np.float32(np.inf if t_max is None else t_max)
            want = (hits["prim_id"] >= 0) & (hits["distance"] < np.float64(bound))
            r = {key: stats(v) for key, v in ms.items()}
            r["occluded_share"] = round(float(want.mean()), 4)
            for key, got in answers.items():
                diff = np.flatnonzero(got != want)
                r[key + "_differs"] = int(diff.size)
                if diff.size:  # only the slack of the box culling of t_max may differ (rtcore.h)
                    rel = np.abs(hits["distance"][diff] / np.float64(bound) - 1.0)
                    r[key + "_differs_max_rel"] = float(rel.max())
                    r[key + "_differs_within_slack"] = bool(rel.max() <= 2.4e-7)
            rec[label] = r
        os.environ.pop("RTCORE_OCCLUDED_EARLY", None)
        if not a.no_host:
            tm = np.full(n, 1.0)
            out = {}
            gpu.occluded_rays(rays, None, tm)
            gpu.query_rays(rays)  # warm: staging, pages
            for key in ("occluded_rays", "query_rays"):
                ts = []
                for _ in range(3):
                    t0 = time.perf_counter()
                    if key == "occluded_rays":
                        gpu.occluded_rays(rays, None, tm)
                    else:
                        h = gpu.query_rays(rays)
                        _ = (h["prim_id"] >= 0) & (h["distance"] < tm)
                    ts.append((time.perf_counter() - t0) * 1e3)
                out[key] = stats(ts)
            rec["host_entry_ms_t_max=1"] = out
        gpu.close()
        print(json.dumps(rec), flush=True)
        del d_rays, d_hits, d_out
        torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
