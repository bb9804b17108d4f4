"""A primitive lit from a grid of light probes, from the bake to the irradiance on the device.

usage: python tools/shade_probes.py SCENE --grid NX NY NZ --spp N [--prim P] --size W H [--offset E] [--flip]
                                    [--seed S] [--traversal MODE] [--out PREFIX] [--depth]
                                    [--relocate STEPS [--min-front X]]
       python tools/shade_probes.py --mesh --grid ...

SCENE is a scene file (or the name of one shipped in tests/golden/scenes; --mesh: the procedural 1 M-triangle
mesh of raytracercore_amd/scenes.py).  The probes are the cell centres of an NX x NY x NZ grid over the scene's
bound shrunk by 5 % (tools/bake_probes.py): render_probes_device takes N RT_GATHER_SPHERE samples at each,
probe_radiance_device closes the sums with the scene's ambient colour, and shade_probes_device reads the grid
at the texel centres of triangle primitive P (texel_surfels, default the scene's first), once leaving out
the probes a texel cannot see and once without that test.  Nothing leaves the device until the results do.
Writes PREFIX.npy / PREFIX_flat.npy (float32 [H, W, 3], with and without visibility), PREFIX_weight.npy
([H, W]) and PREFIX.ppm / PREFIX_flat.ppm (luminance, grey).

Prints, over the texels, the mean and the largest relative difference (of the luminance, relative to the mean
luminance of the gather) to pi x gather_mean of a COSINE render_surfels of the same N samples at the same
points -- the irradiance by its own estimator -- and the share of texels with weight < 1 and with weight 0.
The difference is Monte Carlo noise on both sides plus what nine coefficients and a trilinear blend cannot
hold.  Information, not a test.

--depth: also bakes the probes' depth maps (render_probe_depth, the same N samples in the same directions, d_max
twice the grid's diagonal step, sharpness 5) and shades the texels a third way, rt_shade_probes_depth_device, into
PREFIX_depth.npy / PREFIX_depth_weight.npy; prints its difference to the gather as for the other two, and how the
depth test agrees with the rays over the (texel, corner) pairs that have a segment: the share of ray-hidden
corners whose Chebyshev weight c is below 0.5, and the share of ray-visible corners with c >= 0.5.

--relocate STEPS [--min-front X] (implies --depth): probe relocation (rtcore.h, "probe relocation").  STEPS steps of
N samples each and a classification (relocate_probes; min_front X, default a fifth of the smallest step), then the
radiance and the depth maps are baked again at the relocated positions (probe_positions) and the texels shaded
through the placed entries, with rays (rt_shade_probes_placed_device) and with the maps
(rt_shade_probes_depth_placed_device), into PREFIX_relocated.npy / PREFIX_relocated_weight.npy.  Prints both
differences to the gather, the probes moved per step, the state counts, and the agreement table above before and
after relocation (after: the segments end at the relocated probes).
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

LUM = np.array([0.2126, 0.7152, 0.0722])


def load_scene(rc, scene, mesh: bool):
    if mesh:
        from raytracercore_amd.scenes import mesh_scene_text

        return rc.SceneLoader.from_text(mesh_scene_text()), "mesh"
    path = scene if os.path.exists(scene) else rc.scene_path(scene)
    return rc.SceneLoader.from_file(path), os.path.basename(path)


def scene_grid(rc, scene, dims, visibility=True, bias=0.0):
    """(rt_probe_grid, probe positions [n, 3]) of the cell centres of dims cells over the scene's bound shrunk by 5 %."""
    from bake_probes import probe_grid

    b = rc.scene_bound(list(scene.prims))
    lo, hi = np.array(b["lo"], np.float64), np.array(b["hi"], np.float64)
    pad = 0.05 * (hi - lo)
    lo, hi = lo + pad, hi - pad
    positions = probe_grid(list(lo) + list(hi), dims)
    return rc.probe_grid(positions[0], (hi - lo) / np.array(dims), dims, visibility, bias), positions


def first_triangle(rc, scene) -> int:
    return next(i for i, p in enumerate(scene.prims) if p.kind == rc.RT_PRIM_TRIANGLE)


def texel_surfels(prim, width: int, height: int, offset: float, flip: bool = False):
    """The texel centres of the parallelogram a triangle primitive spans, v0 + (i + 1/2) / width (v1 - v0) +
    (j + 1/2) / height (v2 - v0), pushed `offset` along the unit normal (v1 - v0) x (v2 - v0) (negated with flip);
    (positions, normals), both (width, height, 3).  rt_prim.p holds the three vertices (include/rtcore.h);
    rc.prim_surfels adds p[1] and p[2] to p[0] as if they were edges, so its points leave the primitive, and a
    grid is not read where nothing is lit: hence this function (DESIGN.md section 8 has the lead)."""
    v0, v1, v2 = (np.array([v.x, v.y, v.z], np.float64) for v in prim.p)
    e01, e02 = v1 - v0, v2 - v0
    nrm = np.cross(e01, e02)
    nrm = nrm / np.sqrt(nrm @ nrm) * (-1.0 if flip else 1.0)
    u = ((np.arange(width) + 0.5) / width)[:, None, None]
    v = ((np.arange(height) + 0.5) / height)[None, :, None]
    positions = v0 + u * e01 + v * e02 + offset * nrm
    return positions, np.broadcast_to(nrm, positions.shape).copy()


def bake_grid_device(rc, torch, gpu, positions, spp: int, seed: int, ambient):
    """L of the probes at `positions` as a device tensor [n, 9, 3], and the rays spent."""
    n = len(positions)
    d_probes = torch.from_numpy(rc._pack_surfels(positions, np.tile([0.0, 0.0, 1.0], (n, 1))).view(np.uint8)).cuda()
    d_sh = torch.zeros((n, 9, 4), dtype=torch.float64, device="cuda")
    d_ns, d_nm = (torch.zeros(n, dtype=torch.int32, device="cuda") for _ in range(2))
    d_count = torch.zeros(1, dtype=torch.int64, device="cuda")
    d_L = torch.empty((n, 9, 3), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    gpu.render_probes_device(d_probes, n, spp, seed, 0, 0, d_sh, d_ns, d_nm, d_count)
    rc.probe_radiance_device(d_sh, d_ns, d_nm, n, ambient, d_L)
    torch.cuda.synchronize()
    return d_L, int(d_count.item())


def corner_chebyshev(rc, grid, D, rays, t_max, d_max: float, var_floor: float):
    """The Chebyshev weight c of every (point, corner) pair with a segment (t_max > 0; 1 elsewhere), from the
    segments rt_debug_probe_segments_device reports: the probe is the segment's end, v = -direction * t_max its
    vector to the point (numpy, not the kernels' rounding: information)."""
    d, t = rays["direction"][..., :3], t_max[..., None]
    q = rays["origin"][..., :3] + d * t
    idx = np.rint((q - np.array(grid.origin)) / np.array(grid.step)).astype(np.int64)
    idx = np.clip(idx, 0, np.array(grid.dims) - 1)
    probe = (idx[..., 2] * grid.dims[1] + idx[..., 1]) * grid.dims[0] + idx[..., 0]
    has = t_max > 0
    v = np.where(has[..., None], -d * t, [0.0, 0.0, 1.0])
    m = D[probe, rc.oct_texel(v)]
    mu, m2 = m[..., 0], m[..., 1]
    r = np.minimum(t_max, d_max)
    with np.errstate(invalid="ignore"):
        var = np.maximum(m2 - mu * mu, var_floor)
        c = (var / (var + (r - mu) ** 2)) ** 3
        return np.where(has & np.isfinite(mu) & np.isfinite(m2) & (r > mu), c, 1.0)


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--depth", action="store_true")
    ap.add_argument("scene", nargs="?", default="bounce.txt")
    ap.add_argument("--mesh", action="store_true")
    ap.add_argument("--grid", type=int, nargs=3, required=True, metavar=("NX", "NY", "NZ"))
    ap.add_argument("--spp", type=int, required=True)
    ap.add_argument("--prim", type=int)
    ap.add_argument("--size", type=int, nargs=2, required=True, metavar=("W", "H"))
    ap.add_argument("--offset", type=float, default=1e-3)
    ap.add_argument("--flip", action="store_true")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--traversal", default="AUTO", choices=["AUTO", "BRUTE", "GROUPED", "BVH"])
    ap.add_argument("--out", default="shade_probes")
    ap.add_argument("--relocate", type=int, default=0, metavar="STEPS")
    ap.add_argument("--min-front", type=float, default=None, metavar="X")
    a = ap.parse_args(argv)
    if min(a.grid) < 1 or a.spp < 1 or min(a.size) < 1 or a.relocate < 0:
        ap.error("--grid, --spp and --size must be >= 1, --relocate >= 0")
    a.depth = a.depth or a.relocate > 0

    import torch

    import raytracercore_amd as rc
    from bake_ao import write_ppm

    scene, name = load_scene(rc, a.scene, a.mesh)
    p = first_triangle(rc, scene) if a.prim is None else a.prim
    if not 0 <= p < scene.n_prims or scene.prims[p].kind != rc.RT_PRIM_TRIANGLE:
        ap.error(f"--prim must name a triangle primitive (0 .. {scene.n_prims - 1})")
    W, H = a.size
    amb = scene.params.ambient
    grid, positions = scene_grid(rc, scene, a.grid)
    flat, _ = scene_grid(rc, scene, a.grid, visibility=False)
    pos, nrm = texel_surfels(scene.prims[p], W, H, a.offset, a.flip)
    n = W * H
    gpu = rc.GpuRaytracer(scene, 0, traversal=getattr(rc, "RT_TRAVERSAL_" + a.traversal))
    try:
        d_L, rays = bake_grid_device(rc, torch, gpu, positions, a.spp, a.seed, amb)
        d_pts = torch.from_numpy(rc._pack_surfels(pos.reshape(-1, 3), nrm.reshape(-1, 3)).view(np.uint8)).cuda()
        d_E, d_E0 = (torch.empty((n, 3), dtype=torch.float64, device="cuda") for _ in range(2))
        d_W, d_W0 = (torch.empty(n, dtype=torch.float64, device="cuda") for _ in range(2))
        d_sum = torch.zeros(3 * n, dtype=torch.float64, device="cuda")
        d_ns, d_nm = (torch.zeros(n, dtype=torch.int32, device="cuda") for _ in range(2))
        torch.cuda.synchronize()
        gpu.shade_probes_device(grid, d_L, d_pts, n, d_E, d_W)
        gpu.shade_probes_device(flat, d_L, d_pts, n, d_E0, d_W0)
        gpu.render_surfels_device(d_pts, n, a.spp, a.seed, rc.RT_GATHER_COSINE, 0, 0, d_sum, d_ns, d_nm)
        torch.cuda.synchronize()
        E, E0, Wt = d_E.cpu().numpy(), d_E0.cpu().numpy(), d_W.cpu().numpy()
        gather = np.pi * rc.gather_mean(d_sum.cpu().numpy().reshape(3, n).T, d_ns.cpu().numpy().view(np.uint32),
                                        d_nm.cpu().numpy().view(np.uint32), amb)
        absent = int(torch.isnan(d_L).any(dim=2).any(dim=1).sum().item())
        if a.depth:
            d_max = 2.0 * float(np.linalg.norm(np.array(flat.step)))
            P = rc.probe_depth_params(d_max, 5)
            acc = gpu.render_probe_depth(positions, a.spp, a.seed, d_max, sharpness=5)
            d_Ed = torch.empty((n, 3), dtype=torch.float64, device="cuda")
            d_Wd = torch.empty(n, dtype=torch.float64, device="cuda")
            rc.shade_probes_depth_device(flat, P, d_L, acc["D"], d_pts, n, d_Ed, d_Wd)
            torch.cuda.synchronize()
            Ed, Wd = d_Ed.cpu().numpy(), d_Wd.cpu().numpy()
            seg, t_max = gpu.probe_segments_device(grid, pos.reshape(-1, 3), nrm.reshape(-1, 3))
            occ = np.asarray(gpu.occluded_rays(seg.reshape(-1), None, t_max.reshape(-1))).reshape(n, 8) != 0
            cheb = corner_chebyshev(rc, grid, acc["D"].cpu().numpy(), seg, t_max, d_max, P.var_floor)
            counts = acc["counts"].cpu().numpy().view(np.uint32).astype(np.int64)
        if a.relocate:
            min_front = a.min_front if a.min_front is not None else 0.2 * float(min(flat.step))
            R = rc.probe_relocate_params(min_front)
            d_o, d_state, d_info, moved = gpu.relocate_probes(flat, R, a.spp, a.relocate, a.seed)
            placed = gpu.probe_positions(flat, d_o).cpu().numpy().view(rc.SURFEL_DTYPE).reshape(-1)
            d_Lr, _ = bake_grid_device(rc, torch, gpu, placed["position"][:, :3], a.spp, a.seed, amb)
            acc_r = gpu.render_probe_depth(placed, a.spp, a.seed, d_max, sharpness=5)
            d_Er, d_Ev = (torch.empty((n, 3), dtype=torch.float64, device="cuda") for _ in range(2))
            d_Wr, d_Wv = (torch.empty(n, dtype=torch.float64, device="cuda") for _ in range(2))
            rc.shade_probes_depth_placed_device(flat, d_o, d_state, P, d_Lr, acc_r["D"], d_pts, n, d_Er, d_Wr)
            gpu.shade_probes_placed_device(grid, d_o, d_state, d_Lr, d_pts, n, d_Ev, d_Wv)
            torch.cuda.synchronize()
            Er, Wr, Ev, Wv = d_Er.cpu().numpy(), d_Wr.cpu().numpy(), d_Ev.cpu().numpy(), d_Wv.cpu().numpy()
            seg_r, t_max_r = gpu.probe_segments_placed_device(grid, d_o, d_state, pos.reshape(-1, 3), nrm.reshape(-1, 3))
            occ_r = np.asarray(gpu.occluded_rays(seg_r.reshape(-1), None, t_max_r.reshape(-1))).reshape(n, 8) != 0
            cheb_r = corner_chebyshev(rc, grid, acc_r["D"].cpu().numpy(), seg_r, t_max_r, d_max, P.var_floor)
            counts_r = acc_r["counts"].cpu().numpy().view(np.uint32).astype(np.int64)
            state = d_state.cpu().numpy().view(np.uint32)
            offsets = d_o.cpu().numpy()
    finally:
        gpu.close()

    def image(v):
        return np.ascontiguousarray(v.reshape(W, H, -1).transpose(1, 0, 2).astype(np.float32))

    np.save(a.out + ".npy", image(E))
    np.save(a.out + "_flat.npy", image(E0))
    np.save(a.out + "_weight.npy", image(Wt)[..., 0])
    write_ppm(a.out + ".ppm", np.nan_to_num(image(E) @ LUM.astype(np.float32)))
    write_ppm(a.out + "_flat.ppm", np.nan_to_num(image(E0) @ LUM.astype(np.float32)))
    ref = gather @ LUM
    scale = max(float(np.nanmean(ref)), 1e-300)
    print(f"{name} primitive {p}, {W}x{H} texels lit from {a.grid[0]}x{a.grid[1]}x{a.grid[2]} = {len(positions)} probes "
          f"({absent} absent), {a.spp} spp, {rays} rays in the bake; mean luminance of pi x COSINE gather {scale:.5f}")
    ways = [("visibility", E, Wt > 0), ("no visibility", E0, np.ones(n, bool))]
    if a.depth:
        ways.append(("depth maps", Ed, Wd > 0))
        np.save(a.out + "_depth.npy", image(Ed))
        np.save(a.out + "_depth_weight.npy", image(Wd)[..., 0])
    if a.relocate:
        ways += [("relocated, rays", Ev, Wv > 0), ("relocated, maps", Er, Wr > 0)]
        np.save(a.out + "_relocated.npy", image(Er))
        np.save(a.out + "_relocated_weight.npy", image(Wr)[..., 0])
    for label, e, lit in ways:
        d = np.abs(e @ LUM - ref)[lit] / scale
        print(f"  {label:14s} mean |difference| {float(np.nanmean(d)) if d.size else float('nan'):.4f}, max "
              f"{float(np.nanmax(d)) if d.size else float('nan'):.4f} of that mean, over {int(lit.sum())} texels with a probe")
    print(f"  weight < 1 at {float((Wt < 1 - 1e-12).mean()):.4f} of the texels, weight 0 at {float((Wt == 0).mean()):.4f}"
          f" -> {a.out}.npy, {a.out}_flat.npy, {a.out}_weight.npy, {a.out}.ppm, {a.out}_flat.ppm")
    share = lambda sel, ok: float((ok & sel).sum()) / max(int(sel.sum()), 1)  # noqa: E731
    if a.relocate:
        steps = np.linalg.norm(offsets / np.array(flat.step), axis=1)
        print(f"  relocation: min_front {min_front:.4g}, {a.relocate} steps of {a.spp} spp moved {moved} probes; states: "
              f"{int((state == 0).sum())} plain, {int((state & rc.RT_PROBE_INSIDE != 0).sum())} inside, "
              f"{int((state & rc.RT_PROBE_IDLE != 0).sum())} idle; offsets up to {float(np.nanmax(steps)):.3f} steps, "
              f"{int((steps > 0).sum())} of {len(steps)} probes off their grid position")
        for label, tm, oc, ch, cn in (("before", t_max, occ, cheb, counts), ("after", t_max_r, occ_r, cheb_r, counts_r)):
            has = tm > 0
            hidden, visible = has & oc, has & ~oc
            print(f"  {label:6s} relocation: {int(has.sum())} (texel, corner) pairs, {int(hidden.sum())} ray-hidden, of them c < 0.5 at "
                  f"{share(hidden, ch < 0.5):.4f}; {int(visible.sum())} ray-visible, of them c >= 0.5 at {share(visible, ch >= 0.5):.4f}; "
                  f"inside hits {int(cn[:, 1].sum())} of {int(cn[:, 0].sum())}, "
                  f"{int((rc.probe_backface_share(cn) > 0.5).sum())} probes with a backface share above 0.5")
    if a.depth:
        has = t_max > 0
        hidden, visible = has & occ, has & ~occ
        print(f"  depth against rays over {int(has.sum())} (texel, corner) pairs: {int(hidden.sum())} ray-hidden, of them c < 0.5 at "
              f"{share(hidden, cheb < 0.5):.4f}; {int(visible.sum())} ray-visible, of them c >= 0.5 at {share(visible, cheb >= 0.5):.4f}; "
              f"depth weight < 1 at {float((Wd < 1 - 1e-12).mean()):.4f} of the texels, 0 at {float((Wd == 0).mean()):.4f}; "
              f"d_max {d_max:.4g}, inside hits {int(counts[:, 1].sum())} of {int(counts[:, 0].sum())} hits, "
              f"{int((rc.probe_backface_share(counts) > 0.5).sum())} probes with a backface share above 0.5")
    return 0


if __name__ == "__main__":
    sys.exit(main())
