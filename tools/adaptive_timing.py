"""The cost of the list form and of the adaptive loop, on the device.

usage: python tools/adaptive_timing.py [--workloads bounce,die] [--size 1920 1080] [--spp 64] [--reps 5]
                                       [--tol 0.1] [--min 16] [--max 256] [--batch 16] [--no-host]

Per workload (camera 0 of bounce.txt in its AUTO mode and of die.txt in its AUTO mode, with rt_set_jit off so
that rt_render_device runs the generic kernels the list form always runs), after warming every call, --reps
alternating repetitions, each timed with device events on one stream, the range and the median printed:
  frame        rt_render_device over the whole frame at --spp (its block cull on, as a user gets it)
  frame_nocull the same with RTCORE_BLOCK_CULL=0
  list         rt_render_pixels_device over every pixel of the frame, in rt_adaptive_select_device's order,
               with the moments: the overhead of the list form (it has no block cull)
  list_rows    the same pixels listed row by row: what the block order is worth
  select       rt_adaptive_select_device over the frame's accumulators as the renders left them (few or no
               pixels active: the count and the scan alone)
  select_all   the same with a rule under which every pixel is active (the whole list written)
The sums of frame and list are compared (bit for bit where --spp is at most 24).  Then render_adaptive end to
end (host clock around the loop, which ends in a synchronise) against a uniform rt_render_device at --max, and
the host entry rt_render_pixels over the frame's pixels with the time of its duplicate check (a bitmap of the
frame) taken on its own through a list that fails the check at its last entry.  One JSON line per workload.
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

WORKLOADS = {"bounce": "bounce.txt", "die": "die.txt"}


def stats(ms):
    return {"min": round(min(ms), 3), "max": round(max(ms), 3), "median": round(float(np.median(ms)), 3)}


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workloads", default="bounce,die")
    ap.add_argument("--size", type=int, nargs=2, default=(1920, 1080))
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--tol", type=float, default=0.1)
    ap.add_argument("--min", type=int, default=16, dest="min_spp")
    ap.add_argument("--max", type=int, default=256, dest="max_spp")
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--no-host", action="store_true")
    a = ap.parse_args(argv)

    import torch

    import raytracercore_amd as rc

    if rc.device_count() < 1:
        raise RuntimeError("adaptive_timing: no HIP device (a timing needs the GPU)")
    rc.set_jit(False)
    W, H = a.size
    npix = W * H
    for name in a.workloads.split(","):
        scene = rc.SceneLoader.from_file(rc.scene_path(WORKLOADS[name]))
        gpu = rc.GpuRaytracer(scene, 0, size=(W, H))
        st = torch.cuda.Stream()
        acc = {k: torch.zeros(sh, dtype=dt, device="cuda") for k, sh, dt in (
            ("sum", (3, H, W), torch.float64), ("samples", (H, W), torch.int32), ("misses", (H, W), torch.int32),
            ("q", (H, W), torch.float64), ("batches", (H, W), torch.int32))}
        ptr = [acc[k].data_ptr() for k in ("sum", "samples", "misses", "q", "batches")]
        d_count = torch.zeros(1, dtype=torch.int32, device="cuda")
        d_rays = torch.zeros(1, dtype=torch.int64, device="cuda")
        d_block = torch.empty(npix, dtype=torch.int32, device="cuda")
        everything = rc.rt_adaptive_params(0.0, 1.0, 1 << 30, 1 << 31)  # N < min_samples: every pixel
        rc.adaptive_select_device(everything, *ptr, W, H, d_block.data_ptr(), npix, d_count.data_ptr(), stream=st.cuda_stream)
        st.synchronize()
        assert int(d_count.item()) == npix
        d_rows = torch.arange(npix, dtype=torch.int32, device="cuda")

        def clear():
            for t in acc.values():
                t.zero_()

        def frame(cull):
            if cull:
                os.environ.pop("RTCORE_BLOCK_CULL", None)
            else:
                os.environ["RTCORE_BLOCK_CULL"] = "0"
            gpu.render_device(0, 0, W, H, a.spp, 1, 0, ptr[0], ptr[1], ptr[2], d_rays.data_ptr(), stream=st.cuda_stream)
            os.environ.pop("RTCORE_BLOCK_CULL", None)

        def listed(d_list):
            gpu.render_pixels_device(d_list.data_ptr(), npix, a.spp, 1, 0, *ptr, stream=st.cuda_stream)

        par = rc.rt_adaptive_params(a.tol, 1e-3, a.min_spp, a.max_spp)
        d_sel = torch.empty(npix, dtype=torch.int32, device="cuda")
        calls = {"frame": lambda: frame(True), "frame_nocull": lambda: frame(False), "list": lambda: listed(d_block),
                 "list_rows": lambda: listed(d_rows),
                 "select": lambda: rc.adaptive_select_device(par, *ptr, W, H, d_sel.data_ptr(), npix, d_count.data_ptr(),
                                                             stream=st.cuda_stream),
                 "select_all": lambda: rc.adaptive_select_device(everything, *ptr, W, H, d_sel.data_ptr(), npix,
                                                                 d_count.data_ptr(), stream=st.cuda_stream)}
        sums = {}
        torch.cuda.synchronize()
        for key, fn in calls.items():  # warm, and keep what each render computes from zero
            if not key.startswith("select"):
                with torch.cuda.stream(st):
                    clear()
            fn()
            st.synchronize()
            if not key.startswith("select"):
                sums[key] = acc["sum"].cpu().numpy().copy()
        ms = {key: [] for key in calls}
        for _ in range(a.reps):
            for key, fn in calls.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(st)
                fn()
                e1.record(st)
                e1.synchronize()
                ms[key].append(e0.elapsed_time(e1))
        rec = {"workload": name, "size": [W, H], "spp": a.spp, "traversal": int(gpu.info().traversal),
               "jit": False}
        rec.update({key: stats(v) for key, v in ms.items()})
        rec["list_equals_frame_bits"] = bool(sums["list"].tobytes() == sums["frame"].tobytes())
        rec["list_rows_equals_list_bits"] = bool(sums["list_rows"].tobytes() == sums["list"].tobytes())
        rec["max_rel_diff_list_frame"] = float(np.max(np.abs(sums["list"] - sums["frame"]) / np.maximum(np.abs(sums["frame"]), 1e-300)))
        # the loop end to end against the uniform render at --max
        gpu.render_adaptive(a.tol, a.min_spp, a.max_spp, a.batch, seed=1)  # warm
        ad, un = [], []
        for _ in range(max(2, a.reps // 2)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = gpu.render_adaptive(a.tol, a.min_spp, a.max_spp, a.batch, seed=1)
            ad.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            gpu.render_device(0, 0, W, H, int(res["params"].max_samples), 1, 0, ptr[0], ptr[1], ptr[2], d_rays.data_ptr(), stream=st.cuda_stream)
            st.synchronize()
            un.append((time.perf_counter() - t0) * 1e3)
        spp = res["spp"]
        rec["adaptive"] = {"tol": a.tol, "min": int(res["params"].min_samples), "max": int(res["params"].max_samples),
                           "batch": a.batch, "passes": len(res["counts"]), "list_sizes": res["counts"],
                           "samples": int(spp.sum()), "share_of_uniform": round(float(spp.sum()) / (int(res["params"].max_samples) * npix), 4),
                           "loop_ms": stats(ad), "uniform_max_ms": stats(un)}
        if not a.no_host:
            px = d_block.cpu().numpy().view(np.uint32)
            out = gpu.render_pixels(px, 4, seed=1)  # warm: staging, pages
            ts, tc = [], []
            bad = px.copy()
            bad[-1] = bad[0]  # named twice: refused after the whole bitmap pass, before any launch
            for _ in range(3):
                t0 = time.perf_counter()
                gpu.render_pixels(px, 4, seed=1, out=out[:3])
                ts.append((time.perf_counter() - t0) * 1e3)
                t0 = time.perf_counter()
                try:
                    gpu.render_pixels(bad, 4, seed=1, out=out[:3])
                    raise AssertionError("a duplicate was accepted")
                except rc.RtError:
                    pass
                tc.append((time.perf_counter() - t0) * 1e3)
            rec["host_entry_4spp_ms"] = stats(ts)
            rec["host_entry_list_check_ms"] = stats(tc)
        gpu.close()
        print(json.dumps(rec), flush=True)
        torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
