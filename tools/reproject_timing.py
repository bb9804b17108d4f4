"""The cost of the temporal reprojection, on the device, beside the passes around it.

usage: python tools/reproject_timing.py [--workload bounce] [--size 1920 1080] [--spp 16] [--move 0.02] [--reps 7] [--once]

Camera 0 of the workload in its AUTO mode; one whole-frame pass of --spp samples with the moments
(rt_render_pixels_device over every pixel in rt_adaptive_select_device's order) fills the accumulators and
rt_primary_hits_device the previous hits; then the camera moves --move of its distance to look_at along its
`side` vector and rt_primary_hits_device gives the current hits.  After warming every call, --reps alternating
repetitions, each timed with device events on one stream, the range and the median printed:
  reproject       rt_reproject_device with REPROJECT_DEFAULTS (the samples of the first pass are below
                  max_history: accepted pixels are copies)
  reproject_cap   the same with max_history = spp / 2: every accepted pixel takes the cap's arithmetic
  hits            rt_primary_hits_device over the frame, under the moved camera
  batch           one more whole-frame rt_render_pixels_device pass of --spp samples under the moved camera
The kernels' own durations come from a kernel trace of a run with --once (one call of each kind after the
warm-up).  One JSON line.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KEYS = ("sum", "samples", "misses", "q", "batches")


def stats(ms):
    return {"min": round(min(ms), 3), "max": round(max(ms), 3), "median": round(float(np.median(ms)), 3)}


def side_vector(cam) -> np.ndarray:
    """Camera.InitRender's `side` of an rt_camera."""
    v = lambda p: np.array([p.x, p.y, p.z])  # noqa: E731
    unit = lambda a: a / np.sqrt((a * a).sum())  # noqa: E731
    look = unit(v(cam.look_at) - v(cam.position))
    return -unit(np.cross(look, -v(cam.up)))


def moved_camera(rc, cam, distance: float):
    """`cam` with position and look_at moved `distance` along its side vector."""
    out = rc.rt_camera.from_buffer_copy(cam)
    step = distance * side_vector(cam)
    for name in ("position", "look_at"):
        p = getattr(cam, name)
        setattr(out, name, rc.rt_vec4d(p.x + step[0], p.y + step[1], p.z + step[2], p.w))
    return out


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workload", default="bounce")
    ap.add_argument("--size", type=int, nargs=2, default=(1920, 1080))
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--move", type=float, default=0.02)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--once", action="store_true", help="one timed call of each kind (for a kernel trace)")
    a = ap.parse_args(argv)

    import torch

    import raytracercore_amd as rc

    if rc.device_count() < 1:
        raise RuntimeError("reproject_timing: no HIP device (a timing needs the GPU)")
    W, H = a.size
    npix = W * H
    scene = rc.SceneLoader.from_file(rc.scene_path(a.workload + ".txt"))
    gpu = rc.GpuRaytracer(scene, 0, size=(W, H))
    cam0 = rc.rt_camera.from_buffer_copy(gpu.camera)
    p, l = cam0.position, cam0.look_at
    cam1 = moved_camera(rc, cam0, a.move * float(np.sqrt((l.x - p.x) ** 2 + (l.y - p.y) ** 2 + (l.z - p.z) ** 2)))
    st = torch.cuda.Stream()
    s = st.cuda_stream
    shapes = (("sum", (3, H, W), torch.float64), ("samples", (H, W), torch.int32), ("misses", (H, W), torch.int32),
              ("q", (H, W), torch.float64), ("batches", (H, W), torch.int32))
    acc = {k: torch.zeros(sh, dtype=dt, device="cuda") for k, sh, dt in shapes}
    out = {k: torch.empty(sh, dtype=dt, device="cuda") for k, sh, dt in shapes}
    nxt = {k: torch.zeros(sh, dtype=dt, device="cuda") for k, sh, dt in shapes}  # the moved camera's own accumulators
    ptr, optr, nptr = ([d[k].data_ptr() for k in KEYS] for d in (acc, out, nxt))
    d_src = torch.empty((H, W), dtype=torch.int32, device="cuda")
    d_count = torch.zeros(1, dtype=torch.int32, device="cuda")
    d_list = torch.empty(npix, dtype=torch.int32, device="cuda")
    d_prev = torch.empty((npix, rc.HIT_DTYPE.itemsize), dtype=torch.uint8, device="cuda")
    d_hits = torch.empty((npix, rc.HIT_DTYPE.itemsize), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    everything = rc.rt_adaptive_params(0.0, 1.0, 1 << 30, 1 << 31)  # N < min_samples: every pixel
    rc.adaptive_select_device(everything, *ptr, W, H, d_list.data_ptr(), npix, d_count.data_ptr(), stream=s)
    gpu.render_pixels_device(d_list.data_ptr(), npix, a.spp, 1, 0, *ptr, stream=s)
    gpu.primary_hits_device(d_prev.data_ptr(), stream=s)
    st.synchronize()
    gpu.set_camera(cam1)
    passes = [0]

    def batch():
        gpu.render_pixels_device(d_list.data_ptr(), npix, a.spp, 2, passes[0] * a.spp, *nptr, stream=s)
        passes[0] += 1

    def reproject(**kw):
        rc.reproject_device(rc.reproject_params(**kw), cam0, d_prev.data_ptr(), d_hits.data_ptr(), *ptr, W, H, *optr,
                            d_src.data_ptr(), stream=s)

    calls = {"reproject": reproject, "reproject_cap": lambda: reproject(max_history=max(1, a.spp // 2)),
             "hits": lambda: gpu.primary_hits_device(d_hits.data_ptr(), stream=s), "batch": batch}
    calls["hits"]()
    for fn in calls.values():  # warm
        fn()
    st.synchronize()
    ms = {key: [] for key in calls}
    for _ in range(1 if a.once else a.reps):
        for key, fn in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            fn()
            e1.record(st)
            e1.synchronize()
            ms[key].append(e0.elapsed_time(e1))
    reproject()
    st.synchronize()
    rec = {"workload": a.workload, "size": [W, H], "spp": a.spp, "move": a.move, "reps": len(ms["batch"]),
           "traversal": int(gpu.info().traversal), "accepted_share": round(float((d_src >= 0).double().mean().item()), 4)}
    rec.update({key: stats(v) for key, v in ms.items()})
    rec["reproject_over_batch"] = round(rec["reproject"]["median"] / rec["batch"]["median"], 4)
    rec["reproject_over_hits"] = round(rec["reproject"]["median"] / rec["hits"]["median"], 4)
    gpu.close()
    print(json.dumps(rec), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
