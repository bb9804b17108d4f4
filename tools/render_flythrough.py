"""A camera drag with and without history: each frame rendered adaptively from the previous frame's
reprojected accumulators (GpuRaytracer.primary_hits, reproject and render_adaptive(history=...); include/rtcore.h,
"temporal reprojection") and, for comparison, from scratch.

usage: python tools/render_flythrough.py SCENE [--frames K] [--step D] [--size W H] [--tol T] [--min N] [--max N]
                                         [--batch N] [--seed S] [--history N] [--exposure E] [--traversal MODE]
                                         [--out PREFIX]

SCENE is a scene file (or the name of one shipped in tests/golden/scenes).  Frame 0 is camera 0 from scratch;
every later frame moves the camera --step (world units) along its `side` vector.  Frame f draws its samples at
sample_base = f * --max, so that a pixel that maps to itself never draws a stream twice.  --history is
max_history of rt_reproject_params.  Prints per frame the accepted share (of the pixels with a first hit, the
only ones that can carry a history, and of the frame), the rays of the continued and of the from-scratch render
and both renders' list sizes, then the totals, and writes the last continued frame toned with rt_tonemap_device
as PREFIX.npy / PREFIX.ppm (the ARGB codes as int32 [H, W] / a binary P6).
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("scene")
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--step", type=float, default=0.05)
    ap.add_argument("--size", type=int, nargs=2, default=None)
    ap.add_argument("--tol", type=float, default=0.05)
    ap.add_argument("--min", type=int, default=16, dest="min_spp")
    ap.add_argument("--max", type=int, default=256, dest="max_spp")
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--history", type=int, default=None)
    ap.add_argument("--exposure", type=float, default=1.0)
    ap.add_argument("--traversal", default="AUTO", choices=["AUTO", "BRUTE", "GROUPED", "BVH"])
    ap.add_argument("--out", default="flythrough")
    a = ap.parse_args(argv)
    if a.frames < 1 or a.batch < 1 or a.min_spp < 1 or a.max_spp < a.min_spp:
        ap.error("need --frames >= 1, --batch >= 1 and 1 <= --min <= --max")

    import torch

    import raytracercore_amd as rc
    from render_panorama import write_ppm
    from reproject_timing import moved_camera

    path = a.scene if os.path.exists(a.scene) else rc.scene_path(a.scene)
    scene = rc.SceneLoader.from_file(path)
    gpu = rc.GpuRaytracer(scene, 0, size=tuple(a.size) if a.size else None, traversal=getattr(rc, "RT_TRAVERSAL_" + a.traversal))
    par = {} if a.history is None else {"max_history": a.history}
    args = (a.tol, a.min_spp, a.max_spp, a.batch)
    try:
        W, H = gpu.width, gpu.height
        cam = rc.rt_camera.from_buffer_copy(gpu.camera)
        res = gpu.render_adaptive(*args, seed=a.seed)
        hits = gpu.primary_hits()
        print(f"{os.path.basename(path)} {W}x{H}: tol {a.tol}, {a.min_spp}..{a.max_spp} spp in batches of {a.batch}, "
              f"step {a.step}, max_history {rc.reproject_params(**par).max_history}")
        print(f"frame 0: from scratch {res['rays']} rays, lists {res['counts']}")
        total = [0, 0]
        for f in range(1, a.frames):
            prev_cam, cam = cam, moved_camera(rc, cam, a.step)
            gpu.set_camera(cam)
            h = gpu.reproject(res, prev_cam, hits, **par)
            res = gpu.render_adaptive(*args, seed=a.seed, history=h, sample_base=f * a.max_spp)
            scratch = gpu.render_adaptive(*args, seed=a.seed, sample_base=f * a.max_spp)
            hits = h["hits"]
            total[0] += res["rays"]
            total[1] += scratch["rays"]
            n_acc = int((h["src"] >= 0).sum().item())
            n_hit = int((hits.view(torch.int32)[:, 0] >= 0).sum().item())  # rt_hit.prim_id
            print(f"frame {f}: accepted {n_acc / max(1, n_hit):.4f} of the hits, {n_acc / (W * H):.4f} of the frame, "
                  f"rays continued {res['rays']} / from scratch {scratch['rays']} ({res['rays'] / max(1, scratch['rays']):.3f}), lists continued {res['counts']}, "
                  f"from scratch {scratch['counts']}")
        if a.frames > 1:
            print(f"frames 1..{a.frames - 1}: rays continued {total[0]} / from scratch {total[1]} ({total[0] / max(1, total[1]):.3f})")
        amb = scene.params.ambient
        with torch.cuda.device(gpu.device):
            d_argb = torch.empty((H, W), dtype=torch.int32, device=res["sum"].device)
            rc.tonemap_device(res["sum"].data_ptr(), res["samples"].data_ptr(), res["misses"].data_ptr(), W, H,
                              d_argb.data_ptr(), (amb.r, amb.g, amb.b), 1.0, a.exposure,
                              stream=torch.cuda.current_stream().cuda_stream)
            argb = d_argb.cpu().numpy()
    finally:
        gpu.close()
    np.save(a.out + ".npy", argb)
    write_ppm(a.out + ".ppm", argb)
    print(f"-> {a.out}.npy, {a.out}.ppm")
    return 0


if __name__ == "__main__":
    sys.exit(main())
