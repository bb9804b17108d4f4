"""A grid of light probes: the radiance arriving at points in the air, as L2 spherical harmonics.

usage: python tools/bake_probes.py SCENE --grid NX NY NZ [--bounds X0 Y0 Z0 X1 Y1 Z1] --spp N [--seed S]
                                   [--traversal MODE] [--show K] [--out probes.npz]
                                   [--tol T [--min A] [--max B] [--batch C]] [--relocate STEPS [--min-front X]]

SCENE is a scene file (or the name of one shipped in tests/golden/scenes).  The probes are the cell centres of
an NX x NY x NZ grid over --bounds (default: the box of the scene's primitives without the planes,
rc.scene_bound, shrunk by 5 % on every side).  render_probes takes N RT_GATHER_SPHERE samples at each and
keeps them as 27 spherical-harmonic sums and the projection of the directions that met nothing;
probe_radiance_sh closes those with the scene's ambient colour.  Writes positions [n, 3], L [n, 9, 3],
samples [n], misses [n] and the grid to the .npz.

--tol T bakes adaptively (GpuRaytracer.bake_probes_adaptive): every probe gets samples in batches of C
(--batch, default 16), at least A (--min, default 64) and at most B (--max, default --spp), until the estimated
standard error of its band-0/1 irradiance is at most T of its mean luminance.  The .npz then also holds the
samples each probe took (spp [n]), and the total is printed against n x B.  A probe whose samples so far all came
back black has an estimated error of zero and stops at A: choose --min so that a probe finds the scene's lights.

--relocate STEPS first moves the probes off nearby geometry (rtcore.h, "probe relocation";
GpuRaytracer.relocate_probes: STEPS steps of N samples each, min_front X, default a fifth of the smallest cell
side, then a classification) and bakes at the relocated positions.  The .npz then also holds offsets [n, 3] and
state [n] (RT_PROBE_INSIDE, RT_PROBE_IDLE), which shade_probes takes; positions are the relocated ones.

For the first K probes (--show, default 3) and the six axis normals it prints sh_irradiance(L, normal) beside
pi x gather_mean of a COSINE render_surfels of the same N samples at the same point: the irradiance by its
own estimator.  The two differ by Monte Carlo noise and by what nine coefficients cannot hold (a cosine lobe
keeps 99 % of its energy in bands 0 .. 2, sharp lighting less).  Information, not a test.
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

AXES = np.array([[1.0, 0, 0], [-1.0, 0, 0], [0, 1.0, 0], [0, -1.0, 0], [0, 0, 1.0], [0, 0, -1.0]])


def probe_grid(bounds, grid) -> np.ndarray:
    """The cell centres of a grid[0] x grid[1] x grid[2] grid over bounds = (x0, y0, z0, x1, y1, z1), [n, 3],
    x fastest: 64 consecutive probes are neighbours, so a wave's paths start close together."""
    lo, hi = np.array(bounds[:3], np.float64), np.array(bounds[3:], np.float64)
    axes = [lo[k] + (np.arange(grid[k]) + 0.5) / grid[k] * (hi[k] - lo[k]) for k in range(3)]
    z, y, x = np.meshgrid(axes[2], axes[1], axes[0], indexing="ij")
    return np.stack([x, y, z], axis=-1).reshape(-1, 3)


def bake_probes(gpu, positions, spp: int, ambient, seed: int = 0):
    """(L [n, 9, 3], samples, misses, rays) of render_probes at the positions."""
    import raytracercore_amd as rc

    sh, ns, ms, rays = gpu.render_probes(positions, spp, seed)
    return rc.probe_radiance_sh(sh, ns, ms, ambient), ns, ms, rays


def bake_probes_tol(gpu, positions, tol: float, min_spp: int, max_spp: int, batch: int, ambient, seed: int = 0):
    """(L [n, 9, 3], samples, misses, rays, spp [n]) of bake_probes_adaptive at the positions."""
    import raytracercore_amd as rc

    res = gpu.bake_probes_adaptive(positions, tol, min_spp, max_spp, batch, seed=seed, ambient=ambient)
    sh = res["sh"].cpu().numpy()
    ns, ms = (res[k].cpu().numpy().view(np.uint32) for k in ("samples", "misses"))
    return rc.probe_radiance_sh(sh, ns, ms, ambient), ns, ms, res["rays"], res["spp"].cpu().numpy()


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("scene")
    ap.add_argument("--grid", type=int, nargs=3, required=True, metavar=("NX", "NY", "NZ"))
    ap.add_argument("--bounds", type=float, nargs=6, metavar=("X0", "Y0", "Z0", "X1", "Y1", "Z1"))
    ap.add_argument("--spp", type=int, required=True)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--traversal", default="AUTO", choices=["AUTO", "BRUTE", "GROUPED", "BVH"])
    ap.add_argument("--show", type=int, default=3)
    ap.add_argument("--out", default="probes.npz")
    ap.add_argument("--tol", type=float, help="bake adaptively to this relative error of the band-0/1 irradiance")
    ap.add_argument("--min", type=int, default=64, dest="min_spp")
    ap.add_argument("--max", type=int, dest="max_spp", help="default: --spp")
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--relocate", type=int, default=0, metavar="STEPS")
    ap.add_argument("--min-front", type=float, default=None, metavar="X")
    a = ap.parse_args(argv)
    if min(a.grid) < 1 or a.spp < 1 or a.relocate < 0:
        ap.error("--grid and --spp must be >= 1, --relocate >= 0")
    max_spp = a.max_spp if a.max_spp is not None else a.spp
    if a.tol is not None and (a.tol < 0 or a.batch < 1 or a.min_spp < 1 or max_spp < a.min_spp):
        ap.error("--tol needs T >= 0, --batch >= 1 and 1 <= --min <= --max")

    import raytracercore_amd as rc

    path = a.scene if os.path.exists(a.scene) else rc.scene_path(a.scene)
    scene = rc.SceneLoader.from_file(path)
    bounds = a.bounds
    if bounds is None:
        b = rc.scene_bound(list(scene.prims))
        lo, hi = np.array(b["lo"], np.float64), np.array(b["hi"], np.float64)
        if not (np.isfinite(lo).all() and np.isfinite(hi).all() and (hi > lo).all()):
            ap.error("the scene has no bounded primitive: give --bounds")
        pad = 0.05 * (hi - lo)
        bounds = list(lo + pad) + list(hi - pad)
    positions = probe_grid(bounds, a.grid)
    amb = scene.params.ambient
    gpu = rc.GpuRaytracer(scene, 0, traversal=getattr(rc, "RT_TRAVERSAL_" + a.traversal))
    placement = {}
    try:
        if a.relocate:
            step = (np.array(bounds[3:]) - np.array(bounds[:3])) / np.array(a.grid)
            grid = rc.probe_grid(positions[0], step, a.grid, False)
            min_front = a.min_front if a.min_front is not None else 0.2 * float(step.min())
            d_o, d_state, _, moved = gpu.relocate_probes(grid, rc.probe_relocate_params(min_front), a.spp, a.relocate, a.seed)
            placement = {"offsets": d_o.cpu().numpy(), "state": d_state.cpu().numpy().view(np.uint32)}
            placed = gpu.probe_positions(grid, d_o).cpu().numpy().view(rc.SURFEL_DTYPE).reshape(-1)
            positions = placed["position"][:, :3].copy()  # (NaN for a probe without a valid offset: none comes from a step)
            st = placement["state"]
            print(f"relocation: min_front {min_front:.4g}, moved per step {moved}, {int((st & rc.RT_PROBE_INSIDE != 0).sum())} probes "
                  f"inside, {int((st & rc.RT_PROBE_IDLE != 0).sum())} idle")
        if a.tol is None:
            L, ns, ms, rays = bake_probes(gpu, positions, a.spp, amb, a.seed)
            taken = None
        else:
            L, ns, ms, rays, taken = bake_probes_tol(gpu, positions, a.tol, a.min_spp, max_spp, a.batch, amb, a.seed)
        k = min(a.show, len(positions))
        rows = []
        for i in range(k):
            s, cn, cm, _ = gpu.render_surfels(np.repeat(positions[i:i + 1], 6, axis=0), AXES, a.spp, a.seed, rc.RT_GATHER_COSINE,
                                              stream_base=i * 6)
            rows.append((rc.sh_irradiance(L[i], AXES), np.pi * rc.gather_mean(s, cn, cm, amb)))
    finally:
        gpu.close()
    extra = dict(placement, **({} if taken is None else {"spp": taken}))
    np.savez(a.out, positions=positions, L=L, samples=ns, misses=ms, grid=np.array(a.grid), bounds=np.array(bounds), **extra)
    if taken is None:
        how = f"{a.spp} spp"
    else:
        cap = -(-max_spp // a.batch) * a.batch
        how = (f"rel_tol {a.tol}: {int(taken.sum())} samples of {len(positions)} x {cap} = {len(positions) * cap} "
               f"({int((taken < cap).sum())} probes stopped early, {int(taken.min())} .. {int(taken.max())} spp)")
    print(f"{os.path.basename(path)}: {a.grid[0]}x{a.grid[1]}x{a.grid[2]} = {len(positions)} probes over "
          f"{np.round(bounds, 4).tolist()}, {how}, {rays} rays, {int(ms.sum())} of {int((ns + ms).sum())} samples met "
          f"nothing -> {a.out}")
    names = ("+x", "-x", "+y", "-y", "+z", "-z")
    for i, (e_sh, e_cos) in enumerate(rows):
        print(f"probe {i} at {np.round(positions[i], 4).tolist()}: irradiance r g b, L2 probe | pi x COSINE gather ({a.spp} spp each)")
        for name, u, v in zip(names, e_sh, e_cos):
            print(f"  {name}  {u[0]:9.5f} {u[1]:9.5f} {u[2]:9.5f} | {v[0]:9.5f} {v[1]:9.5f} {v[2]:9.5f}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
