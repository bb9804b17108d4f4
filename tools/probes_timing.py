"""What a probe costs: rt_render_probes_device against the scalar SPHERE gather and against the long way round.

usage: python tools/probes_timing.py [--scene bounce.txt | --mesh] [--mode BRUTE] [--n 4096,65536] [--spp 64,1024]
                                     [--reps 3] [--only a,b,c]

The probes are the cell centres of a cubic grid over the scene's bound (tools/bake_probes.py), the first n of
them, x fastest.  --mesh: the procedural mesh config (raytracercore_amd/scenes.py) in place of a scene file.
Per (n, spp), on one stream, device events round every timed window, after warming each:
  (a) rt_render_probes_device: n probes, spp samples, one sample per work item, folded to 36 sums per probe.
  (b) rt_render_surfels_device in RT_GATHER_SPHERE at the same n and spp: the same paths in longer items and no
      directional result -- the floor.
  (c) the way without the entry: rt_debug_surfel_rays_device into an n x spp ray buffer (64 B per sample),
      rt_render_rays_device at spp = 1 over it (32 B of accumulators per sample), and a torch fold of the basis
      and the weighted sums in fp64.
A call is split by sample_base wherever 64 ceil(n / 64) x (spp rounded up to a power of two) passes 2^26 (the
split is printed); the sizes of the defaults need none.  Every window's results are compared.  (b) against (a):
the counts and the ray count equal, and band 0 (c[0] / K0 is the scalar sum) as a relative difference, which the
scalar gather's several fp32 samples per item leave near 1e-6.  (c) against (a): ray i spp + k of the buffer
is sample k of probe i's first segment, but in one call over the buffer its path draws from stream i spp + k,
not from (i, k): the counts and the misses' projection c[.][3], which depend on first segments alone, are
compared (relative, the torch fold sums in another order); the colours agree only as estimates.  Inside a
closed room no sample meets nothing, and the comparison of c[.][3] is then one of zeros.
One JSON line per (n, spp).  The fold kernel's own time is not in these windows: read it from a kernel trace
of `--only a` (rocprofv3 --kernel-trace --stats -- python tools/probes_timing.py --only a ...),
accumulate_probes_kernel's row.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

K = (0.28209479177387814, 0.48860251190291992, 1.0925484305920792, 0.31539156525252005, 0.54627421529603959)


def stats(ms):
    return {"min": round(min(ms), 3), "max": round(max(ms), 3), "median": round(float(np.median(ms)), 3)}


def torch_fold(torch, d_rays, d_sum, d_ns, d_ms, n, spp):
    """(c)'s last step: sh [n, 9, 4] from the n x spp rays and their per-sample accumulators."""
    m = n * spp
    d = d_rays.view(torch.float64).view(m, 8)
    x, y, z = d[:, 4], d[:, 5], d[:, 6]
    Y = torch.stack([torch.full_like(x, K[0]), K[1] * y, K[1] * z, K[1] * x, (K[2] * x) * y, (K[2] * y) * z,
                     K[3] * ((3.0 * z) * z - 1.0), (K[2] * x) * z, K[4] * (x * x - y * y)], dim=1)
    Y = Y * ((x != 0) | (y != 0) | (z != 0)).to(torch.float64)[:, None]  # (an invalid probe's rays are zeros)
    w = torch.cat([d_sum.view(3, m).t(), d_ms.to(torch.float64)[:, None]], dim=1)  # colour of a hit (0 for a miss), 1 for a miss
    sh = torch.bmm(Y.view(n, spp, 9).transpose(1, 2), w.view(n, spp, 4))
    return sh, d_ns.view(n, spp).sum(dim=1), d_ms.view(n, spp).sum(dim=1)


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scene", default="bounce.txt")
    ap.add_argument("--mesh", action="store_true")
    ap.add_argument("--mode", default="BRUTE", choices=["BRUTE", "GROUPED", "BVH"])
    ap.add_argument("--n", default="4096,65536")
    ap.add_argument("--spp", default="64,1024")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--only", default="a,b,c")
    a = ap.parse_args(argv)

    import torch

    import raytracercore_amd as rc
    from bake_probes import probe_grid

    if rc.device_count() < 1:
        raise RuntimeError("probes_timing: no HIP device (a timing needs the GPU)")
    if a.mesh:
        from raytracercore_amd.scenes import mesh_scene_text

        scene, name = rc.SceneLoader.from_text(mesh_scene_text()), "mesh"
    else:
        path = a.scene if os.path.exists(a.scene) else rc.scene_path(a.scene)
        scene, name = rc.SceneLoader.from_file(path), os.path.basename(path)
    b = rc.scene_bound(list(scene.prims))
    lo, hi = np.array(b["lo"], np.float64), np.array(b["hi"], np.float64)
    pad = 0.05 * (hi - lo)
    sizes = [int(v) for v in a.n.split(",")]
    side = int(np.ceil(max(sizes) ** (1.0 / 3.0)))
    grid = probe_grid(list(lo + pad) + list(hi - pad), (side, side, side))
    which = a.only.split(",")
    lib = rc.load_library()
    gpu = rc.GpuRaytracer(scene, 0, traversal=getattr(rc, "RT_TRAVERSAL_" + a.mode))
    assert gpu.info().traversal == getattr(rc, "RT_TRAVERSAL_" + a.mode)
    st = torch.cuda.Stream()
    for n in sizes:
        probes = rc._pack_surfels(grid[:n], np.tile([0.0, 0.0, 1.0], (n, 1)))
        d_probes = torch.from_numpy(probes.view(np.uint8)).cuda()
        for spp in (int(v) for v in a.spp.split(",")):
            pow2 = 1 << (spp - 1).bit_length()
            fit = (1 << 26) // (64 * ((n + 63) // 64))  # sample slots per call
            step = spp if pow2 <= fit else 1 << (fit.bit_length() - 1)
            pieces = [(s0, min(step, spp - s0)) for s0 in range(0, spp, step)]
            m = n * spp
            d_sh = torch.zeros((n, 9, 4), dtype=torch.float64, device="cuda")
            d_ns, d_ms = (torch.zeros(n, dtype=torch.int32, device="cuda") for _ in range(2))
            d_sum_b = torch.zeros(3 * n, dtype=torch.float64, device="cuda")
            d_ns_b, d_ms_b = (torch.zeros(n, dtype=torch.int32, device="cuda") for _ in range(2))
            d_count = torch.zeros(1, dtype=torch.int64, device="cuda")
            if "c" in which:
                d_rays = torch.empty(m * 64, dtype=torch.uint8, device="cuda")
                d_sum_c = torch.zeros(3 * m, dtype=torch.float64, device="cuda")
                d_ns_c, d_ms_c = (torch.zeros(m, dtype=torch.int32, device="cuda") for _ in range(2))
            res = {}

            def run_a():
                for t in (d_sh, d_ns, d_ms):
                    t.zero_()
                for s0, k in pieces:
                    gpu.render_probes_device(d_probes, n, k, 0, s0, 0, d_sh, d_ns, d_ms, d_count, stream=st.cuda_stream)

            def run_b():
                for t in (d_sum_b, d_ns_b, d_ms_b):
                    t.zero_()
                gpu.render_surfels_device(d_probes, n, spp, 0, rc.RT_GATHER_SPHERE, 0, 0, d_sum_b, d_ns_b, d_ms_b, d_count,
                                          stream=st.cuda_stream)

            def run_c():
                for t in (d_sum_c, d_ns_c, d_ms_c):
                    t.zero_()
                rc._check(lib.rt_debug_surfel_rays_device(rc.RT_GATHER_SPHERE, C.c_void_p(d_probes.data_ptr()), n, spp, 0, 0, 0,
                                                          C.c_void_p(d_rays.data_ptr()), C.c_void_p(st.cuda_stream)))
                # ray i * spp + k must draw from (stream i, sample k): one call per sample over a strided view is
                # the only exact way, and n x spp rays in one call the only fair one; the paths' later draws then
                # come from other streams, so (c) is compared in its counts' totals and its first segments only
                gpu.render_rays_device(d_rays.data_ptr(), m, 1, 0, 0, 0, d_sum_c.data_ptr(), d_ns_c.data_ptr(), d_ms_c.data_ptr(),
                                       d_count.data_ptr(), stream=st.cuda_stream)
                res["c"] = torch_fold(torch, d_rays, d_sum_c, d_ns_c, d_ms_c, n, spp)

            runs = {"a": run_a, "b": run_b, "c": run_c}
            ms, traced = {}, {}
            with torch.cuda.stream(st):
                for key in which:  # warm, and the calls' ray counts
                    d_count.zero_()
                    runs[key]()
                    st.synchronize()
                    traced[key] = int(d_count.item())
                    ms[key] = []
                for _ in range(a.reps):
                    for key in which:
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record(st)
                        runs[key]()
                        e1.record(st)
                        e1.synchronize()
                        ms[key].append(e0.elapsed_time(e1))
            checks = {}
            if "a" in which and "b" in which:
                checks["b_counts_equal"] = bool(torch.equal(d_ns, d_ns_b) and torch.equal(d_ms, d_ms_b)) and traced["a"] == traced["b"]
                band0 = d_sh[:, 0, :3] / K[0]
                checks["b_band0_rel"] = float(((band0 - d_sum_b.view(3, n).t()).abs().max() / band0.abs().max().clamp(min=1e-300)).item())
            if "a" in which and "c" in which:
                sh_c, ns_c, ms_c = res["c"]
                # the misses' projection depends on the first segments alone, which (c) shares with (a) exactly
                checks["c_sky_rel"] = float(((sh_c[..., 3] - d_sh[..., 3]).abs().max() / d_sh[..., 3].abs().max().clamp(min=1e-300)).item())
                checks["c_counts_equal"] = bool(torch.equal(ns_c.to(torch.int32), d_ns) and torch.equal(ms_c.to(torch.int32), d_ms))
            rec = {"scene": name, "mode": a.mode, "n": n, "spp": spp, "reps": a.reps, "split": pieces if len(pieces) > 1 else None,
                   "ms": {key: stats(v) for key, v in ms.items()}, "rays_traced": traced, "checks": checks}
            if "a" in ms and "b" in ms:
                rec["a_over_b"] = round(float(np.median(ms["a"]) / np.median(ms["b"])), 4)
            if "a" in ms and "c" in ms:
                rec["c_over_a"] = round(float(np.median(ms["c"]) / np.median(ms["a"])), 4)
            print(json.dumps(rec), flush=True)
            if "c" in which:
                del d_rays, d_sum_c, d_ns_c, d_ms_c
            res.clear()
    gpu.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
