"""The analytic reference (tests/analytic_hits.py) and the CPU oracle held to each other, ray by ray.

Both are fp64, written apart: plain numpy formulas over the ABI's rt_prim records on one side, the oracle's
restatement of the reference's AVX paths with its BVH query on the other.  Scenes: the zoo of
tests/test_hit_records_gpu.py, bounce.txt, die.txt, the 300-primitive soup and the vertex-normal scene.
Rays: the 4096 line-of-sight rays of tests/test_query_rays_gpu.py and the targeted rays of
tests/test_hit_records_gpu.py (128 per primitive, fewer on a large scene: about 4096 in all).

ID: compared on every ray.  A mismatch is excused only where the reference's two smallest distances over
the primitives differ by no more than 1e-9 max(t, 1) (a tie: either answer is right), and the share of rays
excluded that way must stay below 0.1 %.  A tie on which the IDs agree is not excluded: its distance is
compared like any other.  Distance: |t_oracle - t| / max(t, 1) on every hit with equal IDs, within 16 times
the reference's own rounding on the same rays, measured by running it again in np.longdouble.

Measured (x86-64, 80-bit long double).  Per scene: rays, ties, rays excluded, the reference against
itself in long double, the oracle against the reference (the bar is 16 times the column before it):
    zoo       8508   0   0   1.557e-14   1.245e-14
    bounce    6912   8   0   1.265e-14   3.448e-15
    die       7808   0   0   6.454e-15   0
    soup300   7996   0   0   9.157e-13   3.231e-14
    vn        5504   0   0   6.327e-14   1.163e-15
No ID mismatch anywhere.  bounce.txt's 8 ties are exact: the cubes' bottom faces lie in the floor's plane, and
rays aimed at them from below meet both at once (0.12 % of the rays; both sides name the same primitive).
"""
import functools

import numpy as np
import pytest

import test_query_rays_gpu as Q
from analytic_hits import HASNORMALS, INVERT, MIRROR, PLANE, SPHERE, TRANSFORMED, TRIANGLE, TWOSIDED, closest_hit
from oracle.oracle import OracleScene
from test_hit_records_gpu import reference_rounding, targeted_rays, zoo_scene

SCENES = ("zoo", "bounce", "die", "soup300", "vn")
TIE = 1e-9
MAX_TIE_SHARE = 1e-3  # of the rays, excluded


def _scene(name):
    return zoo_scene() if name == "zoo" else Q._scene(name)


@functools.lru_cache(maxsize=None)
def _answers(name):
    import raytracercore_amd as rc

    scene = _scene(name)
    prims = scene.prims
    o1, d1 = Q._line_of_sight_rays(scene.cameras[0])
    o2, d2, _ = targeted_rays(prims, per=max(8, min(128, 4096 // len(prims))))
    o, d = np.concatenate([o1, o2]), np.concatenate([d1, d2])
    ref = closest_hit(prims, o, d)
    orc = OracleScene.from_abi(rc.rt_scene_params.from_buffer_copy(scene.params), list(prims), list(scene.cameras))
    ids, ts = Q._trace(orc, o, d)
    return prims, o, d, ref, ids, ts


@pytest.mark.parametrize("name", SCENES)
def test_reference_and_oracle_agree(name):
    prims, o, d, ref, ids, ts = _answers(name)
    hit = ref["id"] >= 0
    tie = hit & (ref["t2"] - ref["t"] <= TIE * np.maximum(ref["t"], 1.0))
    excluded = tie & (ids != ref["id"])
    wrong = np.flatnonzero(~tie & (ids != ref["id"]))
    same = hit & (ids == ref["id"])
    own = reference_rounding(prims, o, d, ref, same)
    err = float((np.abs(ts[same] - ref["t"][same]) / np.maximum(ref["t"][same], 1.0)).max())
    print(f"{name}: rays {len(o)} hits {hit.sum()} ties {tie.sum()} excluded {excluded.sum()} id mismatches {wrong.size} "
          f"reference against long double {own:.3e} oracle against reference {err:.3e} bar {16 * own:.3e}")
    assert hit.sum() > len(o) // 4
    assert excluded.mean() <= MAX_TIE_SHARE
    assert wrong.size == 0, (wrong[:8], ids[wrong[:8]], ref["id"][wrong[:8]])
    assert err <= 16 * own


def test_the_zoo_holds_every_form(rc):
    """One-sided, two-sided and inverted on every kind; plain spheres and ellipsoids of both sidedness;
    flat, mirrored and vertex-normal triangles; and the record forms the brute-force orders make of them
    (rt_debug_brute_layout): a single world rectangle (the axis-aligned mirrored triangle), world boxes
    (the axis-aligned cube, the room with a side missing), rectangles in frames (the rotated cube, the
    other mirrored triangle), plain triangles, spheres and planes."""
    prims = zoo_scene().prims
    forms = {(p.kind, p.flags) for p in prims}
    print("zoo (kind, flags):", sorted(forms))
    for kind in (TRIANGLE, SPHERE, PLANE):
        flags = [f for k, f in forms if k == kind]
        assert any(not f & (TWOSIDED | INVERT) for f in flags), kind
        assert any(f & TWOSIDED for f in flags), kind
        assert any(f & INVERT for f in flags), kind
    for want in ((SPHERE, TRANSFORMED), (SPHERE, TRANSFORMED | TWOSIDED), (SPHERE, TWOSIDED), (SPHERE, 0),
                 (TRIANGLE, MIRROR), (TRIANGLE, MIRROR | INVERT), (TRIANGLE, HASNORMALS | TWOSIDED), (TRIANGLE, TWOSIDED),
                 (TRIANGLE, 0)):
        assert want in forms, want
    layout = rc.brute_layout(list(prims))
    print("zoo layout:", layout)
    assert layout["rects"] == 1 and layout["boxes"] == 2 and layout["frames"] == 2 and layout["frame_rects"] == 7
    assert layout["tris"] == 4 and layout["spheres"] == 7 and layout["planes"] == 3
