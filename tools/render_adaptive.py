"""Render a scene until every pixel's noise is below a tolerance: GpuRaytracer.render_adaptive (rt_render_pixels_device
and rt_adaptive_select_device in a loop, the image never leaving the device), toned with rt_tonemap_device.

usage: python tools/render_adaptive.py SCENE [--size W H] [--tol T] [--min N] [--max N] [--batch N] [--seed S]
                                       [--floor L] [--exposure E] [--traversal MODE] [--out PREFIX] [--denoise]

SCENE is a scene file (or the name of one shipped in tests/golden/scenes).  A pixel is sampled in batches of
--batch samples until the standard error of its mean luminance is at most --tol times that luminance (held
up to --floor for dark pixels), between --min and --max samples (include/rtcore.h, "adaptive sampling").
Writes PREFIX.npy / PREFIX.ppm (the ARGB codes as int32 [H, W] / a binary P6) and PREFIX_spp.npy /
PREFIX_spp.ppm (the samples every pixel got, int32 [H, W] / grey, white = --max), and prints the samples
taken against max x pixels.  With --denoise the result also goes through GpuRaytracer.denoise (rt_primary_hits_device
and rt_denoise_device, include/rtcore.h "denoising", its default parameters) and is written toned the same way as
PREFIX_denoised.npy / PREFIX_denoised.ppm.
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


def spp_map_argb(spp: np.ndarray, max_spp: int) -> np.ndarray:
    """Samples per pixel as grey ARGB codes, white at max_spp."""
    g = np.clip(spp.astype(np.int64) * 255 // max(1, max_spp), 0, 255).astype(np.uint32)
    return (0xFF000000 | (g << 16) | (g << 8) | g).astype(np.uint32).view(np.int32)


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("scene")
    ap.add_argument("--size", type=int, nargs=2, default=None)
    ap.add_argument("--tol", type=float, default=0.05)
    ap.add_argument("--min", type=int, default=16, dest="min_spp")
    ap.add_argument("--max", type=int, default=256, dest="max_spp")
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--floor", type=float, default=1e-3)
    ap.add_argument("--exposure", type=float, default=1.0)
    ap.add_argument("--traversal", default="AUTO", choices=["AUTO", "BRUTE", "GROUPED", "BVH"])
    ap.add_argument("--out", default="adaptive")
    ap.add_argument("--denoise", action="store_true")
    a = ap.parse_args(argv)
    if a.batch < 1 or a.min_spp < 1 or a.max_spp < a.min_spp or not a.tol >= 0 or not a.floor > 0:
        ap.error("need --batch >= 1, 1 <= --min <= --max, --tol >= 0 and --floor > 0")

    import torch

    import raytracercore_amd as rc
    from render_panorama import write_ppm

    path = a.scene if os.path.exists(a.scene) else rc.scene_path(a.scene)
    scene = rc.SceneLoader.from_file(path)
    gpu = rc.GpuRaytracer(scene, 0, size=tuple(a.size) if a.size else None, traversal=getattr(rc, "RT_TRAVERSAL_" + a.traversal))
    try:
        W, H = gpu.width, gpu.height
        res = gpu.render_adaptive(a.tol, a.min_spp, a.max_spp, a.batch, seed=a.seed, lum_floor=a.floor)
        amb = scene.params.ambient
        with torch.cuda.device(gpu.device):
            d_argb = torch.empty((H, W), dtype=torch.int32, device=res["sum"].device)
            rc.tonemap_device(res["sum"].data_ptr(), res["samples"].data_ptr(), res["misses"].data_ptr(), W, H,
                              d_argb.data_ptr(), (amb.r, amb.g, amb.b), 1.0, a.exposure,
                              stream=torch.cuda.current_stream().cuda_stream)
            argb = d_argb.cpu().numpy()
            if a.denoise:
                filtered = gpu.denoise(res)
                rc.tonemap_device(filtered.data_ptr(), res["samples"].data_ptr(), res["misses"].data_ptr(), W, H,
                                  d_argb.data_ptr(), (amb.r, amb.g, amb.b), 1.0, a.exposure,
                                  stream=torch.cuda.current_stream().cuda_stream)
                argb_denoised = d_argb.cpu().numpy()
        spp = res["spp"].cpu().numpy().astype(np.int32)
    finally:
        gpu.close()
    cap = int(res["params"].max_samples)
    np.save(a.out + ".npy", argb)
    write_ppm(a.out + ".ppm", argb)
    np.save(a.out + "_spp.npy", spp)
    write_ppm(a.out + "_spp.ppm", spp_map_argb(spp, cap))
    if a.denoise:
        np.save(a.out + "_denoised.npy", argb_denoised)
        write_ppm(a.out + "_denoised.ppm", argb_denoised)
    total = int(spp.sum())
    print(f"{os.path.basename(path)} {W}x{H}: tol {a.tol}, {int(res['params'].min_samples)}..{cap} spp in batches of {a.batch}: "
          f"{len(res['counts'])} passes, {total} samples of {cap * W * H} ({total / (cap * W * H):.1%}), {res['rays']} rays, "
          f"{int((spp < cap).sum())} of {W * H} pixels stopped early -> {a.out}.npy, {a.out}.ppm, {a.out}_spp.npy, {a.out}_spp.ppm"
          + (f", {a.out}_denoised.npy, {a.out}_denoised.ppm" if a.denoise else ""))
    return 0


if __name__ == "__main__":
    sys.exit(main())
