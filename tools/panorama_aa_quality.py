"""What --aa buys tools/render_panorama.py: the panorama of bounce.txt at 256 x 128, with rays through the
pixel centres (render_rays) and with beams (render_beams), at 16 and 256 spp and three seeds, against a
reference of 4 x 4 sub-pixel rays at 16 spp each (256 spp per pixel) made with render_rays.

usage: python tools/panorama_aa_quality.py      (needs the GPU; prints one JSON line)

Luminance MSE over the silhouette pixels (partly covered in the reference, or next to a pixel on the
other side of the scene's outline) and over all pixels, a primary miss showing the ambient colour; and
the MSE of the coverage (the share of a pixel's samples that hit anything) over the silhouette pixels,
which carries no shading noise: the aliasing alone."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import raytracercore_amd as rc
import render_panorama as pano

W, H = 256, 128
scene = rc.SceneLoader.from_file(rc.scene_path("bounce.txt"))
cam = scene.cameras[0]
pos = np.array([cam.position.x, cam.position.y, cam.position.z])
fwd = np.array([cam.look_at.x, cam.look_at.y, cam.look_at.z]) - pos
amb = scene.params.ambient
back = np.array([amb.r, amb.g, amb.b])
gpu = rc.GpuRaytracer(scene, 0)



def image(s, n, m):  # mean colour per pixel, a primary miss showing the ambient colour (SampleSet.GetOutput's back colour)
    return (s + m[:, None] * back) / (n + m)[:, None]


def lum(c):
    return 0.299 * c[..., 0] + 0.587 * c[..., 1] + 0.114 * c[..., 2]


# reference: 4 x 4 sub-pixel grid, 16 spp each (256 spp per pixel)
o, d = pano.panorama_rays(pos, fwd, 4 * W)
s, n, m, _ = gpu.render_rays(o, d, 16, 1234)
fine = np.stack([s[:, 0], s[:, 1], s[:, 2], n, m], axis=1).reshape(H, 4, W, 4, 5).sum(axis=(1, 3)).reshape(-1, 5)
ref = image(fine[:, :3], fine[:, 3], fine[:, 4])
cover = fine[:, 3] / (fine[:, 3] + fine[:, 4])
# silhouette pixels: partly covered in the reference, or next to a pixel whose coverage differs
cov2 = cover.reshape(H, W)
hit = cov2 > 0.5
edge = (cov2 > 0) & (cov2 < 1)
edge[:, 1:] |= hit[:, 1:] != hit[:, :-1]
edge[:, :-1] |= hit[:, 1:] != hit[:, :-1]
edge[1:] |= hit[1:] != hit[:-1]
edge[:-1] |= hit[1:] != hit[:-1]
edge = edge.reshape(-1)
out = {"width": W, "height": H, "silhouette_pixels": int(edge.sum())}
for spp in (16, 256):
    for seed in (0, 1, 2):
        o, d = pano.panorama_rays(pos, fwd, W)
        s, n, m, _ = gpu.render_rays(o, d, spp, seed)
        plain = image(s, n, m)
        bo, bd, bdu, bdv = pano.panorama_beams(pos, fwd, W)
        z = np.zeros_like(bo)
        s, n, m, _ = gpu.render_beams(bo, bd, z, z, bdu, bdv, spp, seed)
        aa = image(s, n, m)
        out[f"spp{spp}_seed{seed}"] = {"mse_silhouette_plain": float(np.mean((lum(plain) - lum(ref))[edge] ** 2)),
                              "mse_silhouette_aa": float(np.mean((lum(aa) - lum(ref))[edge] ** 2)),
                              "mse_all_plain": float(np.mean((lum(plain) - lum(ref)) ** 2)),
                              "mse_all_aa": float(np.mean((lum(aa) - lum(ref)) ** 2))}
    # coverage (the share of samples that hit anything) is free of shading noise: the aliasing alone
    o, d = pano.panorama_rays(pos, fwd, W)
    s, n, m, _ = gpu.render_rays(o, d, spp, 0)
    c_plain = n / (n + m)
    s, n, m, _ = gpu.render_beams(bo, bd, z, z, bdu, bdv, spp, 0)
    c_aa = n / (n + m)
    out[f"spp{spp}_coverage_mse_silhouette"] = {"plain": float(np.mean((c_plain - cover)[edge] ** 2)), "aa": float(np.mean((c_aa - cover)[edge] ** 2))}
gpu.close()
print(json.dumps(out))
