"""The radiance arriving at one primitive, baked over its own parallelogram: a lightmap of a triangle primitive.

usage: python tools/bake_irradiance.py SCENE --prim ID --size W H --spp N [--mode diffuse|cosine] [--flip]
                                       [--offset E] [--seed S] [--traversal MODE] [--out PREFIX]
       python tools/bake_irradiance.py SCENE --prim ID --size W H --tol T [--min A] [--max B] [--batch S] ...

SCENE is a scene file (or the name of one shipped in tests/golden/scenes), ID a triangle primitive of it
(v0, e01, e02).  The texel centres v0 + (i + 1/2) / W e01 + (j + 1/2) / H e02, moved E along the unit normal
e01 x e02 (--flip: the other side), are the surfels (prim_surfels); render_surfels gathers N samples at each,
drawn on the device as the reference's diffuse bounce (diffuse) or by Lambert's cosine (cosine), and the
texel is gather_mean with the scene's ambient colour: a sample that meets nothing counts as the ambient.
Writes PREFIX.npy (float32 [H, W, 3]) and PREFIX.ppm (the luminance, clipped to [0, 1], grey), through the
writers of tools/bake_ao.py.

--tol T bakes adaptively instead (gather_adaptive): S samples at a time, between A and B per texel, until the
standard error of a texel's mean luminance is at most T of it.  The selection runs over the texel grid, so
neighbouring texels share a wave.  Also writes PREFIX_spp.npy (uint32 [H, W]) and PREFIX_spp.ppm (the samples
per texel, B = white), and prints the list size of every iteration and the rays spent against those of a
fixed bake at B samples per texel.  The error estimate counts a miss as black (rtcore.h, "indexed radiance
queries"): under a bright ambient colour texels that see the sky take more samples than they need.  A texel
whose first A samples all come back black has no variance to show and stops at A: where the light reaches a
texel only through rare paths, choose A large enough that a first batch meets it (profiles/render_list).
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


def bake_irradiance_adaptive(gpu, prim, width: int, height: int, tol: float, min_spp: int, max_spp: int, batch: int,
                             ambient, mode: int, offset: float = 1e-3, flip: bool = False, seed: int = 0):
    """The adaptive bake: (mean float32 [H, W, 3], samples per texel uint32 [H, W], gather_adaptive's result)."""
    import raytracercore_amd as rc

    pos, nrm = rc.prim_surfels(prim, width, height, offset, flip)
    surfels = rc._pack_surfels(pos.reshape(-1, 3), nrm.reshape(-1, 3))
    # texel [i, j] is entry i * height + j: a frame `height` wide and `width` tall to the selection
    res = gpu.gather_adaptive(rc.RT_LIST_SURFELS, surfels, tol, min_spp, max_spp, batch, seed=seed, mode=mode,
                              shape=(height, width))
    s = np.ascontiguousarray(res["sum"].cpu().numpy().T)
    ns = res["samples"].cpu().numpy().view(np.uint32)
    ms = res["misses"].cpu().numpy().view(np.uint32)
    mean = rc.gather_mean(s, ns, ms, ambient).reshape(width, height, 3)
    spp = (ns + ms).reshape(width, height)
    return np.ascontiguousarray(mean.transpose(1, 0, 2).astype(np.float32)), np.ascontiguousarray(spp.T), res


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("scene")
    ap.add_argument("--prim", type=int, required=True)
    ap.add_argument("--size", type=int, nargs=2, required=True, metavar=("W", "H"))
    ap.add_argument("--spp", type=int)
    ap.add_argument("--tol", type=float, help="adaptive bake: relative standard error of a texel's mean luminance")
    ap.add_argument("--min", type=int, default=16, dest="min_spp")
    ap.add_argument("--max", type=int, default=1024, dest="max_spp")
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--mode", default="diffuse", choices=["diffuse", "cosine"])
    ap.add_argument("--flip", action="store_true")
    ap.add_argument("--offset", type=float, default=1e-3)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--traversal", default="AUTO", choices=["AUTO", "BRUTE", "GROUPED", "BVH"])
    ap.add_argument("--out", default="irradiance")
    a = ap.parse_args(argv)
    if a.tol is None and a.spp is None:
        ap.error("the following arguments are required: --spp")
    if a.tol is None and (min(a.size) < 1 or a.spp < 1):
        ap.error("--size and --spp must be >= 1")
    if a.tol is not None and (min(a.size) < 1 or a.tol < 0 or a.batch < 1 or a.min_spp < 1 or a.max_spp < a.min_spp):
        ap.error("--tol needs --size >= 1, T >= 0, --batch >= 1 and 1 <= --min <= --max")

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
    if a.tol is not None:
        try:
            img, spp, res = bake_irradiance_adaptive(gpu, prim, a.size[0], a.size[1], a.tol, a.min_spp, a.max_spp, a.batch,
                                                     scene.params.ambient, getattr(rc, "RT_GATHER_" + a.mode.upper()),
                                                     a.offset, a.flip, a.seed)
            top = int(res["params"].max_samples)
            pos, nrm = rc.prim_surfels(prim, a.size[0], a.size[1], a.offset, a.flip)
            fixed = gpu.render_surfels(pos.reshape(-1, 3), nrm.reshape(-1, 3), top, a.seed,
                                       getattr(rc, "RT_GATHER_" + a.mode.upper()))
        finally:
            gpu.close()
        np.save(a.out + ".npy", img)
        np.save(a.out + "_spp.npy", spp)
        write_ppm(a.out + ".ppm", np.nan_to_num(img @ np.array([0.2126, 0.7152, 0.0722], np.float32)))
        write_ppm(a.out + "_spp.ppm", spp.astype(np.float32) / float(top))
        for i, n in enumerate(res["counts"]):
            print(f"iteration {i}: {n} texels x {a.batch} samples")
        print(f"{os.path.basename(path)} primitive {a.prim}, {a.size[0]}x{a.size[1]} texels, tol {a.tol} ({a.mode}), "
              f"{int(spp.min())} .. {int(spp.max())} spp, mean {spp.mean():.1f}: {res['rays']} rays against {fixed[3]} at "
              f"{top} spp fixed ({res['rays'] / max(fixed[3], 1):.3f}), mean "
              f"{np.nanmean(img, axis=(0, 1)).round(4).tolist()} -> {a.out}.npy, {a.out}.ppm, {a.out}_spp.npy, {a.out}_spp.ppm")
        return 0
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
