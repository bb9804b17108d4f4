"""Why does this pixel have its colour?  The command-line stand-in for the RayInspector's list
(RayInspector.RunTraces -> Raytracer.GetDebugTrace): the library's own samples of one pixel, one
line per sample and one per bounce, from rt_trace_paths.

usage: python tools/inspect_pixel.py SCENE X Y [--samples N] [--seed S] [--sample-base B]
                                     [--camera C] [--size WxH] [--traversal MODE]

SCENE is a scene file (or the name of one shipped in tests/golden/scenes).  To look at samples that
are in a rendered image, pass the seed and the sample indices that render used.
"""
from __future__ import annotations

import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def _v(a) -> str:
    return "(" + " ".join(f"{float(c):.6g}" for c in a) + ")"


def format_sample(rc, k: int, records, n_rays: int, color) -> list[str]:
    """The lines of one sample: its colour, then one line per bounce record."""
    miss = all(float(c) == -1.0 for c in color)
    lines = [f"sample {k}: {'miss' if miss else 'colour ' + _v(color)}, {n_rays} ray{'s' if n_rays != 1 else ''}"]
    for r in records[:n_rays]:
        head = f"  [{int(r['bounce'])}] {rc.BOUNCE_TYPE_NAMES[int(r['type'])]:<17}"
        ray = f"ray {_v(r['origin'])} -> {_v(r['direction'])} tint {_v(r['tint'])}"
        if int(r["prim_id"]) < 0:
            lines.append(f"{head} no hit; {ray}")
            continue
        lines.append(f"{head} prim {int(r['prim_id'])}{' inside' if int(r['inside']) else ''} t {float(r['distance']):.6g} "
                     f"at {_v(r['position'])} n {_v(r['normal'])} cos {float(r['cos_in']):.6g} "
                     f"fresnel {float(r['fresnel']):.6g}; {ray}")
    return lines


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("scene")
    ap.add_argument("x", type=int)
    ap.add_argument("y", type=int)
    ap.add_argument("--samples", type=int, default=8)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--sample-base", type=int, default=0)
    ap.add_argument("--camera", type=int, default=0)
    ap.add_argument("--size", default="", help="WxH (default: the scene's own size)")
    ap.add_argument("--traversal", default="AUTO", choices=["AUTO", "BRUTE", "GROUPED", "BVH", "BVH2"])
    a = ap.parse_args(argv)

    import raytracercore_amd as rc

    path = a.scene if os.path.exists(a.scene) else rc.scene_path(a.scene)
    scene = rc.SceneLoader.from_file(path)
    size = tuple(int(v) for v in a.size.lower().split("x")) if a.size else None
    gpu = rc.GpuRaytracer(scene, a.camera, size=size, traversal=getattr(rc, "RT_TRAVERSAL_" + a.traversal))
    try:
        records, n_rays, colors = gpu.trace_paths(a.x, a.y, 1, 1, a.samples, seed=a.seed, sample_base=a.sample_base)
        print(f"{os.path.basename(path)} {gpu.width}x{gpu.height} camera {a.camera} pixel ({a.x}, {a.y}) seed {a.seed} "
              f"samples {a.sample_base}..{a.sample_base + a.samples - 1} traversal "
              f"{('AUTO', 'BRUTE', 'BVH', 'BVH2', 'GROUPED')[gpu.info().traversal]}")
        for k in range(a.samples):
            print("\n".join(format_sample(rc, a.sample_base + k, records[0, 0, k], int(n_rays[0, 0, k]), colors[0, 0, k])))
    finally:
        gpu.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
