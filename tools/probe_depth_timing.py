"""What probe depth maps cost: the depth bake against rt_render_probes_device, and the depth-weighted shading
against rt_shade_probes_device with and without RT_PROBE_GRID_VISIBILITY.

usage: python tools/probe_depth_timing.py [--scene bounce.txt | --mesh] [--mode BRUTE] [--grid 8,32] [--n 4096,1048576]
                                          [--spp 64] [--prim P] [--flip] [--reps 3]

The method is tools/shade_probes_timing.py's: one process per scene, G x G x G probes over the scene's bound shrunk
by 5 %, the points the texel centres of triangle primitive P, device events on one stream round every timed
window, after warming each, the windows alternating, medians.  Per G:
  bake_sh     rt_render_probes_device, --spp samples per probe (the path kernels: whole paths, not one hit)
  bake_depth  rt_render_probe_depth_device at the same n and spp: per chunk the sample rays, the closest-hit launch
              and the fold
  close       rt_probe_depth_close_device
and per (G, n):
  blend       rt_shade_probes_device without the flag: the blend kernel alone
  rays        rt_shade_probes_device with RT_PROBE_GRID_VISIBILITY: the yardstick
  depth       rt_shade_probes_depth_device
  depth_wrap  the same with RT_PROBE_DEPTH_WRAP
One JSON line per G and one per (G, n).  d_max is twice the grid's diagonal step.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def stats(ms):
    return {"min": round(min(ms), 3), "max": round(max(ms), 3), "median": round(float(np.median(ms)), 3)}


def timed(torch, st, runs, order, reps):
    """Median-ready lists of milliseconds per window: every window warmed once, then reps rounds in `order`."""
    ms = {key: [] for key in order}
    with torch.cuda.stream(st):
        for key in order:
            runs[key]()
        st.synchronize()
        for _ in range(reps):
            for key in order:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(st)
                runs[key]()
                e1.record(st)
                e1.synchronize()
                ms[key].append(e0.elapsed_time(e1))
    return ms


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scene", default="bounce.txt")
    ap.add_argument("--mesh", action="store_true")
    ap.add_argument("--mode", default="BRUTE", choices=["BRUTE", "GROUPED", "BVH"])
    ap.add_argument("--grid", default="8,32")
    ap.add_argument("--n", default="4096,1048576")
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--prim", type=int)
    ap.add_argument("--flip", action="store_true")
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args(argv)

    import torch

    import raytracercore_amd as rc
    from shade_probes import first_triangle, load_scene, scene_grid, texel_surfels

    if rc.device_count() < 1:
        raise RuntimeError("probe_depth_timing: no HIP device (a timing needs the GPU)")
    scene, name = load_scene(rc, a.scene, a.mesh)
    p = first_triangle(rc, scene) if a.prim is None else a.prim
    amb = scene.params.ambient
    gpu = rc.GpuRaytracer(scene, 0, traversal=getattr(rc, "RT_TRAVERSAL_" + a.mode))
    assert gpu.info().traversal == getattr(rc, "RT_TRAVERSAL_" + a.mode)
    st = torch.cuda.Stream()
    s = st.cuda_stream
    for G in (int(v) for v in a.grid.split(",")):
        vis, positions = scene_grid(rc, scene, (G, G, G), bias=0.0)
        flat, _ = scene_grid(rc, scene, (G, G, G), visibility=False)
        n_p = len(positions)
        d_max = 2.0 * float(np.linalg.norm(np.array(flat.step)))
        P, Pw = rc.probe_depth_params(d_max, 5), rc.probe_depth_params(d_max, 5, wrap=True)
        d_probes = torch.from_numpy(rc._pack_surfels(positions, np.tile([0.0, 0.0, 1.0], (n_p, 1))).view(np.uint8)).cuda()
        d_sh = torch.zeros((n_p, 9, 4), dtype=torch.float64, device="cuda")
        d_ns, d_nm = (torch.zeros(n_p, dtype=torch.int32, device="cuda") for _ in range(2))
        d_L = torch.empty((n_p, 9, 3), dtype=torch.float64, device="cuda")
        d_depth = torch.zeros((n_p, 3, 64), dtype=torch.float64, device="cuda")
        d_counts = torch.zeros((n_p, 4), dtype=torch.int32, device="cuda")
        d_D = torch.empty((n_p, 64, 2), dtype=torch.float64, device="cuda")
        bake = {
            "bake_sh": lambda: gpu.render_probes_device(d_probes, n_p, a.spp, 0, 0, 0, d_sh, d_ns, d_nm, stream=s),
            "bake_depth": lambda: gpu.render_probe_depth_device(d_probes, n_p, a.spp, 0, 0, 0, P, d_depth, d_counts, stream=s),
            "close": lambda: rc.probe_depth_close_device(d_depth, n_p, d_D, stream=s),
        }
        ms = timed(torch, st, bake, ("bake_sh", "bake_depth", "close"), a.reps)
        rc.probe_radiance_device(d_sh, d_ns, d_nm, n_p, amb, d_L, stream=s)
        st.synchronize()
        counts = d_counts.cpu().numpy().view(np.uint32).astype(np.int64).sum(axis=0)
        med = {key: float(np.median(v)) for key, v in ms.items()}
        print(json.dumps({"scene": name, "mode": a.mode, "grid": G, "probes": n_p, "spp": a.spp, "reps": a.reps, "d_max": round(d_max, 4),
                          "ms": {key: stats(v) for key, v in ms.items()},
                          "depth_over_sh": round(med["bake_depth"] / med["bake_sh"], 4),
                          "inside_share_of_hits": round(float(counts[1]) / max(float(counts[0]), 1.0), 4),
                          "absent_texels": int(torch.isnan(d_D[:, :, 0]).sum().item())}), flush=True)
        for n in (int(v) for v in a.n.split(",")):
            w = 1 << ((n.bit_length() - 1) // 2)
            h = n // w
            pos, nrm = texel_surfels(scene.prims[p], w, h, 1e-3, a.flip)
            n = w * h
            d_pts = torch.from_numpy(rc._pack_surfels(pos.reshape(-1, 3), nrm.reshape(-1, 3)).view(np.uint8)).cuda()
            d_E = torch.empty((n, 3), dtype=torch.float64, device="cuda")
            d_W = {key: torch.empty(n, dtype=torch.float64, device="cuda") for key in ("blend", "rays", "depth", "depth_wrap")}
            runs = {
                "blend": lambda: gpu.shade_probes_device(flat, d_L, d_pts, n, d_E, d_W["blend"], stream=s),
                "rays": lambda: gpu.shade_probes_device(vis, d_L, d_pts, n, d_E, d_W["rays"], stream=s),
                "depth": lambda: rc.shade_probes_depth_device(flat, P, d_L, d_D, d_pts, n, d_E, d_W["depth"], stream=s),
                "depth_wrap": lambda: rc.shade_probes_depth_device(flat, Pw, d_L, d_D, d_pts, n, d_E, d_W["depth_wrap"], stream=s),
            }
            ms = timed(torch, st, runs, ("blend", "rays", "depth", "depth_wrap"), a.reps)
            st.synchronize()
            med = {key: float(np.median(v)) for key, v in ms.items()}
            print(json.dumps({"scene": name, "mode": a.mode, "grid": G, "n": n, "reps": a.reps, "prim": p,
                              "ms": {key: stats(v) for key, v in ms.items()},
                              "depth_over_rays": round(med["depth"] / med["rays"], 4),
                              "depth_over_blend": round(med["depth"] / med["blend"], 4),
                              "mean_weight": {key: round(float(v.mean().item()), 4) for key, v in d_W.items()}}), flush=True)
            del d_pts, d_E, d_W
    gpu.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
