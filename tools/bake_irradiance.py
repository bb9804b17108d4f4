"""The radiance arriving at one primitive, baked over its own parallelogram: a lightmap of a triangle primitive.

usage: python tools/bake_irradiance.py SCENE --prim ID --size W H --spp N [--mode diffuse|cosine] [--flip]
                                       [--offset E] [--seed S] [--traversal MODE] [--out PREFIX]

SCENE is a scene file (or the name of one shipped in tests/golden/scenes), ID a triangle primitive of it
(v0, e01, e02).  The texel centres v0 + (i + 1/2) / W e01 + (j + 1/2) / H e02, moved E along the unit normal
e01 x e02 (--flip: the other side), are the surfels (prim_surfels); render_surfels gathers N samples at each,
drawn on the device as the reference's diffuse bounce (diffuse) or by Lambert's cosine (cosine), and the
texel is gather_mean with the scene's ambient colour: a sample that meets nothing counts as the ambient.
Writes PREFIX.npy (float32 [H, W, 3]) and PREFIX.ppm (the luminance, clipped to [0, 1], grey), through the
writers of tools/bake_ao.py.
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


def bake_irradiance(gpu, prim, width: int, height: int, spp: int, ambient, mode: int, offset: float = 1e-3,
                    flip: bool = False, seed: int = 0) -> np.ndarray:
    """The gathered mean at the texel centres of prim's parallelogram as float32 [H, W, 3]."""
    import raytracercore_amd as rc

    pos, nrm = rc.prim_surfels(prim, width, height, offset, flip)
    s, ns, ms, _ = gpu.render_surfels(pos.reshape(-1, 3), nrm.reshape(-1, 3), spp, seed, mode)
    mean = rc.gather_mean(s, ns, ms, ambient).reshape(width, height, 3)
    return np.ascontiguousarray(mean.transpose(1, 0, 2).astype(np.float32))


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("scene")
    ap.add_argument("--prim", type=int, required=True)
    ap.add_argument("--size", type=int, nargs=2, required=True, metavar=("W", "H"))
    ap.add_argument("--spp", type=int, required=True)
    ap.add_argument("--mode", default="diffuse", choices=["diffuse", "cosine"])
    ap.add_argument("--flip", action="store_true")
    ap.add_argument("--offset", type=float, default=1e-3)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--traversal", default="AUTO", choices=["AUTO", "BRUTE", "GROUPED", "BVH"])
    ap.add_argument("--out", default="irradiance")
    a = ap.parse_args(argv)
    if min(a.size) < 1 or a.spp < 1:
        ap.error("--size and --spp must be >= 1")

    import raytracercore_amd as rc
    from bake_ao import write_ppm

    path = a.scene if os.path.exists(a.scene) else rc.scene_path(a.scene)
    scene = rc.SceneLoader.from_file(path)
    if not 0 <= a.prim < scene.n_prims:
        ap.error(f"--prim must be in 0 .. {scene.n_prims - 1}")
    prim = scene.prims[a.prim]
    if prim.kind != rc.RT_PRIM_TRIANGLE:
        ap.error(f"primitive {a.prim} is not a triangle primitive")
    gpu = rc.GpuRaytracer(scene, 0, traversal=getattr(rc, "RT_TRAVERSAL_" + a.traversal))
    try:
        img = bake_irradiance(gpu, prim, a.size[0], a.size[1], a.spp, scene.params.ambient,
                              getattr(rc, "RT_GATHER_" + a.mode.upper()), a.offset, a.flip, a.seed)
    finally:
        gpu.close()
    np.save(a.out + ".npy", img)
    lum = img @ np.array([0.2126, 0.7152, 0.0722], np.float32)
    write_ppm(a.out + ".ppm", np.nan_to_num(lum))
    print(f"{os.path.basename(path)} primitive {a.prim}, {a.size[0]}x{a.size[1]} texels, {a.spp} spp ({a.mode}): "
          f"mean {np.nanmean(img, axis=(0, 1)).round(4).tolist()} -> {a.out}.npy, {a.out}.ppm")
    return 0


if __name__ == "__main__":
    sys.exit(main())
