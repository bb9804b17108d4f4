"""An equirectangular 360 x 180 degree panorama of a scene from one point: a camera the library does not
have, rendered through rt_render_rays (GpuRaytracer.render_rays) and toned with rt_sample_output, the
host twin of rt_tonemap_device.

usage: python tools/render_panorama.py SCENE [--eye X Y Z] [--width W] [--spp N] [--seed S]
                                       [--exposure E] [--traversal MODE] [--aa] [--out PREFIX]

SCENE is a scene file (or the name of one shipped in tests/golden/scenes).  The eye defaults to
camera 0's position.  Column x is the azimuth about +z from the camera's line of sight, row y the
polar angle from +z (up) to -z; the image is W x W/2.  Writes PREFIX.npy (the ARGB codes as int32
[H, W]) and PREFIX.ppm (binary P6, which needs no library to read).  Rays are listed row by row, so
that the 64 rays of a wave are neighbours on a row.

Without --aa every sample of a pixel follows the ray through the pixel's centre: the shading converges
and the silhouettes stay stair-stepped.  --aa renders through rt_render_beams (GpuRaytracer.render_beams):
each pixel is a beam, the direction at its corner and the steps to the next column's and the next
row's corner, and every sample takes its own point of that footprint.
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def panorama_rays(eye, forward, width: int):
    """Origins and unit directions (fp64) of the width x width/2 pixel centres, row-major [y, x]."""
    height = width // 2
    az0 = np.arctan2(forward[1], forward[0])
    phi = az0 + np.pi - (np.arange(width) + 0.5) * (2.0 * np.pi / width)  # left edge: behind the eye
    theta = (np.arange(height) + 0.5) * (np.pi / height)
    st, ct = np.sin(theta)[:, None], np.cos(theta)[:, None]
    d = np.stack([st * np.cos(phi)[None, :], st * np.sin(phi)[None, :], np.broadcast_to(ct, (height, width))], axis=-1)
    d = d.reshape(-1, 3)
    o = np.broadcast_to(np.asarray(eye, np.float64), d.shape)
    return np.ascontiguousarray(o), d


def panorama_beams(eye, forward, width: int):
    """The pixels of panorama_rays as beams (fp64, row-major [y, x]): origins, the direction at each
    pixel's corner, and direction_du = dir(x + 1, y) - dir(x, y), direction_dv = dir(x, y + 1) - dir(x, y),
    the first-order footprint of an equirectangular pixel (at the poles, where a row of corners is one
    point, it narrows to the pixel's meridian).  The corner directions are snapped to multiples of 2^-30
    (a beam's direction need not be unit), so that the differences are exact and the footprints tile:
    beam (x, y) at (u, v) = (1, 0) is beam (x + 1, y) at (0, 0) bit for bit, and the last column closes
    on the first.  Returns (origins, directions, direction_du, direction_dv), each (width * height, 3)."""
    height = width // 2
    az0 = np.arctan2(forward[1], forward[0])
    phi = az0 + np.pi - np.arange(width) * (2.0 * np.pi / width)  # corner columns; column `width` is column 0
    theta = np.arange(height + 1) * (np.pi / height)
    st, ct = np.sin(theta)[:, None], np.cos(theta)[:, None]
    c = np.stack([st * np.cos(phi)[None, :], st * np.sin(phi)[None, :], np.broadcast_to(ct, (height + 1, width))], axis=-1)
    c = np.round(c * 2.0 ** 30) * 2.0 ** -30
    d = c[:-1]
    du = np.roll(c, -1, axis=1)[:-1] - d
    dv = c[1:] - d
    d, du, dv = (np.ascontiguousarray(a.reshape(-1, 3)) for a in (d, du, dv))
    o = np.ascontiguousarray(np.broadcast_to(np.asarray(eye, np.float64), d.shape))
    return o, d, du, dv


def write_ppm(path: str, argb: np.ndarray) -> None:
    """ARGB int32 [H, W] as a binary PPM (alpha dropped)."""
    u = argb.astype(np.uint32)
    rgb = np.stack([(u >> 16) & 255, (u >> 8) & 255, u & 255], axis=-1).astype(np.uint8)
    with open(path, "wb") as f:
        f.write(f"P6\n{argb.shape[1]} {argb.shape[0]}\n255\n".encode())
        f.write(rgb.tobytes())


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("scene")
    ap.add_argument("--eye", type=float, nargs=3, default=None)
    ap.add_argument("--width", type=int, default=512)
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--exposure", type=float, default=1.0)
    ap.add_argument("--traversal", default="AUTO", choices=["AUTO", "BRUTE", "GROUPED", "BVH"])
    ap.add_argument("--aa", action="store_true", help="sample each pixel's footprint (render_beams)")
    ap.add_argument("--out", default="panorama")
    a = ap.parse_args(argv)
    if a.width < 2 or a.width % 2 or a.spp < 1:
        ap.error("--width must be even and >= 2, --spp >= 1")

    import raytracercore_amd as rc

    path = a.scene if os.path.exists(a.scene) else rc.scene_path(a.scene)
    scene = rc.SceneLoader.from_file(path)
    cam = scene.cameras[0]
    pos = np.array([cam.position.x, cam.position.y, cam.position.z])
    forward = np.array([cam.look_at.x, cam.look_at.y, cam.look_at.z]) - pos
    eye = pos if a.eye is None else np.array(a.eye)
    gpu = rc.GpuRaytracer(scene, 0, traversal=getattr(rc, "RT_TRAVERSAL_" + a.traversal))
    try:
        if a.aa:
            o, d, du, dv = panorama_beams(eye, forward, a.width)
            s, n, m, rays = gpu.render_beams(o, d, np.zeros_like(o), np.zeros_like(o), du, dv, a.spp, a.seed)
        else:
            o, d = panorama_rays(eye, forward, a.width)
            s, n, m, rays = gpu.render_rays(o, d, a.spp, a.seed)
    finally:
        gpu.close()
    amb = scene.params.ambient
    argb = np.array([rc.sample_output(tuple(s[i]), int(n[i]), int(m[i]), (amb.r, amb.g, amb.b), 1.0, a.exposure)
                     for i in range(len(n))], np.int32).reshape(a.width // 2, a.width)
    np.save(a.out + ".npy", argb)
    write_ppm(a.out + ".ppm", argb)
    print(f"{os.path.basename(path)} panorama {a.width}x{a.width // 2} from {tuple(float(v) for v in eye)}: {a.spp} spp"
          f"{' (--aa)' if a.aa else ''}, "
          f"{rays} rays, {int((n == 0).sum())} pixels without a hit -> {a.out}.npy, {a.out}.ppm")
    return 0


if __name__ == "__main__":
    sys.exit(main())
