"""The cost of the denoising pass, on the device, beside the work it stands in for.

usage: python tools/denoise_timing.py [--workload bounce] [--size 1920 1080] [--spp 16] [--reps 7] [--once]

Camera 0 of the workload in its AUTO mode; one whole-frame pass of --spp samples with the moments
(rt_render_pixels_device over every pixel in rt_adaptive_select_device's order) fills the accumulators, and
rt_primary_hits_device the guides.  Then, after warming every call, --reps alternating repetitions, each timed
with device events on one stream, the range and the median printed:
  denoise_1 .. denoise_5   rt_denoise_device with iterations 1 .. 5 (preparation, then that many levels; the
                           last level writes the outputs instead of a state record)
  hits                     rt_primary_hits_device over the frame
  tonemap                  rt_tonemap_device over the frame
  batch                    one more whole-frame rt_render_pixels_device pass of --spp samples: the cost of the
                           samples a filter pass stands in for
"levels" are the differences of the medians, denoise_(k+1) - denoise_k: what level k (step 2^k) adds;
"prepare_and_level0" is denoise_1.  The kernels' own durations come from a kernel trace of a run with
--once (one call of each kind after the warm-up).  One JSON line.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def stats(ms):
    return {"min": round(min(ms), 3), "max": round(max(ms), 3), "median": round(float(np.median(ms)), 3)}


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workload", default="bounce")
    ap.add_argument("--size", type=int, nargs=2, default=(1920, 1080))
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--once", action="store_true", help="one timed call of each kind (for a kernel trace)")
    a = ap.parse_args(argv)

    import torch

    import raytracercore_amd as rc

    if rc.device_count() < 1:
        raise RuntimeError("denoise_timing: no HIP device (a timing needs the GPU)")
    W, H = a.size
    npix = W * H
    scene = rc.SceneLoader.from_file(rc.scene_path(a.workload + ".txt"))
    gpu = rc.GpuRaytracer(scene, 0, size=(W, H))
    st = torch.cuda.Stream()
    s = st.cuda_stream
    acc = {k: torch.zeros(sh, dtype=dt, device="cuda") for k, sh, dt in (
        ("sum", (3, H, W), torch.float64), ("samples", (H, W), torch.int32), ("misses", (H, W), torch.int32),
        ("q", (H, W), torch.float64), ("batches", (H, W), torch.int32))}
    ptr = [acc[k].data_ptr() for k in ("sum", "samples", "misses", "q", "batches")]
    d_count = torch.zeros(1, dtype=torch.int32, device="cuda")
    d_list = torch.empty(npix, dtype=torch.int32, device="cuda")
    d_hits = torch.empty((npix, rc.HIT_DTYPE.itemsize), dtype=torch.uint8, device="cuda")
    d_out = torch.empty((3, H, W), dtype=torch.float64, device="cuda")
    d_var = torch.empty((H, W), dtype=torch.float32, device="cuda")
    d_argb = torch.empty((H, W), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    everything = rc.rt_adaptive_params(0.0, 1.0, 1 << 30, 1 << 31)  # N < min_samples: every pixel
    rc.adaptive_select_device(everything, *ptr, W, H, d_list.data_ptr(), npix, d_count.data_ptr(), stream=s)
    passes = [0]

    def batch():
        gpu.render_pixels_device(d_list.data_ptr(), npix, a.spp, 1, passes[0] * a.spp, *ptr, stream=s)
        passes[0] += 1

    def denoise(k):
        rc.denoise_device(rc.denoise_params(iterations=k), *ptr, d_hits.data_ptr(), W, H, d_out.data_ptr(), d_var.data_ptr(),
                          stream=s)

    batch()
    calls = {f"denoise_{k}": (lambda k=k: denoise(k)) for k in range(1, 6)}
    calls["hits"] = lambda: gpu.primary_hits_device(d_hits.data_ptr(), stream=s)
    calls["tonemap"] = lambda: rc.tonemap_device(d_out.data_ptr(), ptr[1], ptr[2], W, H, d_argb.data_ptr(), stream=s)
    calls["batch"] = batch
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
    rec = {"workload": a.workload, "size": [W, H], "spp": a.spp, "reps": len(ms["batch"]), "traversal": int(gpu.info().traversal),
           "valid_pixels": int((acc["samples"] > 0).sum().item())}
    rec.update({key: stats(v) for key, v in ms.items()})
    med = [rec[f"denoise_{k}"]["median"] for k in range(1, 6)]
    rec["prepare_and_level0"] = med[0]
    rec["levels"] = {f"step_{1 << k}": round(med[k] - med[k - 1], 3) for k in range(1, 5)}
    rec["denoise_5_over_batch"] = round(med[4] / rec["batch"]["median"], 4)
    gpu.close()
    print(json.dumps(rec), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
