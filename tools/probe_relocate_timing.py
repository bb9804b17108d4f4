"""What probe relocation costs: a relocation step against rt_render_probe_depth_device at the same n and spp, and the
placed shading entries against the unplaced ones.

usage: python tools/probe_relocate_timing.py [--scene bounce.txt | --mesh] [--mode BRUTE] [--grid 8,32] [--n 4096,1048576]
                                             [--spp 64] [--prim P] [--flip] [--reps 3]

The method is tools/probe_depth_timing.py's: one process per scene, G x G x G probes over the scene's bound shrunk by
5 %, the points the texel centres of triangle primitive P, device events on one stream round every timed window,
after warming each, the windows alternating, medians.  Per G:
  bake_depth  rt_render_probe_depth_device, --spp samples per probe: the sample rays, the closest-hit launch and the
              depth fold per chunk (the yardstick)
  classify    rt_relocate_probes_device with RT_PROBE_RELOCATE_CLASSIFY_ONLY from the relocated offsets: the positions,
              the same rays and launch, and the relocation fold
  step        rt_relocate_probes_device from zero offsets (the offsets are set to zero outside the window)
  positions   rt_probe_positions_device
and per (G, n), with the offsets and states two steps and a classification leave:
  blend / blend_placed    rt_shade_probes_device / rt_shade_probes_placed_device without the visibility flag
  rays / rays_placed      the same with RT_PROBE_GRID_VISIBILITY
  depth / depth_placed    rt_shade_probes_depth_device / rt_shade_probes_depth_placed_device
One JSON line per G and one per (G, n).  d_max is twice the grid's diagonal step, min_front a fifth of the smallest
step.
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
    from probe_depth_timing import stats, timed
    from shade_probes import first_triangle, load_scene, scene_grid, texel_surfels

    if rc.device_count() < 1:
        raise RuntimeError("probe_relocate_timing: no HIP device (a timing needs the GPU)")
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
        P = rc.probe_depth_params(d_max, 5)
        R = rc.probe_relocate_params(0.2 * float(min(flat.step)))
        Rc = rc.probe_relocate_params(R.min_front, classify_only=True)
        d_o, d_state, d_info, moved = gpu.relocate_probes(flat, R, a.spp, 2, 0)
        d_zero = torch.zeros_like(d_o)
        d_probes = gpu.probe_positions(flat, d_o)
        d_sh = torch.zeros((n_p, 9, 4), dtype=torch.float64, device="cuda")
        d_ns, d_nm = (torch.zeros(n_p, dtype=torch.int32, device="cuda") for _ in range(2))
        d_L = torch.empty((n_p, 9, 3), dtype=torch.float64, device="cuda")
        d_depth = torch.zeros((n_p, 3, 64), dtype=torch.float64, device="cuda")
        d_counts = torch.zeros((n_p, 4), dtype=torch.int32, device="cuda")
        d_D = torch.empty((n_p, 64, 2), dtype=torch.float64, device="cuda")
        d_info2 = torch.zeros_like(d_info)

        def step():
            gpu.relocate_probes_device(flat, R, a.spp, 0, 0, 0, d_zero, d_info2, stream=s)

        runs = {
            "bake_depth": lambda: gpu.render_probe_depth_device(d_probes, n_p, a.spp, 0, 0, 0, P, d_depth, d_counts, stream=s),
            "classify": lambda: gpu.relocate_probes_device(flat, Rc, a.spp, 0, 0, 0, d_o, d_info2, stream=s),
            "positions": lambda: rc.probe_positions_device(flat, d_o, d_probes, stream=s),
        }
        ms = timed(torch, st, runs, ("bake_depth", "classify", "positions"), a.reps)
        ms["step"] = []
        with torch.cuda.stream(st):
            for k in range(a.reps + 1):  # (the first one warms)
                d_zero.zero_()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(st)
                step()
                e1.record(st)
                e1.synchronize()
                if k:
                    ms["step"].append(e0.elapsed_time(e1))
        gpu.render_probes_device(d_probes, n_p, a.spp, 0, 0, 0, d_sh, d_ns, d_nm, stream=s)
        rc.probe_radiance_device(d_sh, d_ns, d_nm, n_p, amb, d_L, stream=s)
        rc.probe_depth_close_device(d_depth, n_p, d_D, stream=s)
        st.synchronize()
        state = d_state.cpu().numpy().view(np.uint32)
        med = {key: float(np.median(v)) for key, v in ms.items()}
        print(json.dumps({"scene": name, "mode": a.mode, "grid": G, "probes": n_p, "spp": a.spp, "reps": a.reps,
                          "min_front": round(R.min_front, 4), "ms": {key: stats(v) for key, v in ms.items()},
                          "classify_over_bake_depth": round(med["classify"] / med["bake_depth"], 4),
                          "step_over_bake_depth": round(med["step"] / med["bake_depth"], 4),
                          "moved_per_step": moved, "inside": int((state & rc.RT_PROBE_INSIDE != 0).sum()),
                          "idle": int((state & rc.RT_PROBE_IDLE != 0).sum())}), flush=True)
        for n in (int(v) for v in a.n.split(",")):
            w = 1 << ((n.bit_length() - 1) // 2)
            h = n // w
            pos, nrm = texel_surfels(scene.prims[p], w, h, 1e-3, a.flip)
            n = w * h
            d_pts = torch.from_numpy(rc._pack_surfels(pos.reshape(-1, 3), nrm.reshape(-1, 3)).view(np.uint8)).cuda()
            d_E = torch.empty((n, 3), dtype=torch.float64, device="cuda")
            keys = ("blend", "blend_placed", "rays", "rays_placed", "depth", "depth_placed")
            d_W = {key: torch.empty(n, dtype=torch.float64, device="cuda") for key in keys}
            runs = {
                "blend": lambda: gpu.shade_probes_device(flat, d_L, d_pts, n, d_E, d_W["blend"], stream=s),
                "blend_placed": lambda: gpu.shade_probes_placed_device(flat, d_o, d_state, d_L, d_pts, n, d_E, d_W["blend_placed"], stream=s),
                "rays": lambda: gpu.shade_probes_device(vis, d_L, d_pts, n, d_E, d_W["rays"], stream=s),
                "rays_placed": lambda: gpu.shade_probes_placed_device(vis, d_o, d_state, d_L, d_pts, n, d_E, d_W["rays_placed"], stream=s),
                "depth": lambda: rc.shade_probes_depth_device(flat, P, d_L, d_D, d_pts, n, d_E, d_W["depth"], stream=s),
                "depth_placed": lambda: rc.shade_probes_depth_placed_device(flat, d_o, d_state, P, d_L, d_D, d_pts, n, d_E,
                                                                            d_W["depth_placed"], stream=s),
            }
            ms = timed(torch, st, runs, keys, a.reps)
            st.synchronize()
            med = {key: float(np.median(v)) for key, v in ms.items()}
            print(json.dumps({"scene": name, "mode": a.mode, "grid": G, "n": n, "reps": a.reps, "prim": p,
                              "ms": {key: stats(v) for key, v in ms.items()},
                              "placed_over_unplaced": {k: round(med[k + "_placed"] / med[k], 4) for k in ("blend", "rays", "depth")},
                              "mean_weight": {key: round(float(v.mean().item()), 4) for key, v in d_W.items()}}), flush=True)
            del d_pts, d_E, d_W
    gpu.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
