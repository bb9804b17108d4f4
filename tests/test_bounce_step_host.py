"""The oracle's bounce step against the oracle's own paths (no GPU).

orc_shade_steps and orc_camera_sample_ray run the code get_color and camera_ray run, so a replay along the
oracle's own samples (orc_sample_path: per bounce the direction as traced, normal, inside, tint) must give
back the oracle's types, directions, tints and final colours bit for bit, with the draw cursor advanced by
the rule tests/bounce_cases.py states (`draws_of`).  That proves the factoring of get_color's loop and the
draw accounting the GPU test (tests/test_bounce_step_gpu.py) relies on.

Coverage: on the oracle's own paths every case keeps its excluded decisions (a margin under THRESHOLD)
at or under half the GPU test's cap, and the cases built for it (MATERIALS, MATERIALS_AIR) hold the
per-class counts of bounce_cases.CLASS_MIN among the bounces that are not excluded.  The other cases
cannot hold all of them by construction (recursion 0 and 2 never reach bounce 3, the shipped scenes
have no glass thinner than air) and are held to the exclusion share only.
"""
import numpy as np
import pytest

import bounce_cases as bc
from bounce_cases import EXCLUDED_CAP, THRESHOLD


@pytest.fixture(scope="module")
def replays(rc):
    """Every case's oracle paths and their replay, computed once."""
    out = {}
    for case in bc.CASES:
        scene = bc.parse(rc, case)
        orc = bc.oracle_of(rc, case, scene)
        paths = bc.paths_of_oracle(case, orc, scene.params.recursion)
        out[case.name] = (scene, paths, bc.compare(case, scene, orc, paths, THRESHOLD))
    return out


def test_cases_fit_one_trace_call(rc):
    for case in bc.CASES:
        scene = bc.parse(rc, case)
        w, h = case.tile[2:]
        assert w * h * case.spp * (scene.params.recursion + 1) <= 34000, case.name
        assert case.tile[0] + w <= case.size[0] and case.tile[1] + h <= case.size[1]


def test_materials_scene_is_what_the_rows_say(rc):
    scene = bc.parse(rc, bc.CASE["MATERIALS"])
    shin = sorted({p.shininess for p in scene.prims})
    assert set(bc.SHININESS) <= set(shin) and np.isposinf(shin[-1])
    assert {p.refractive_index for p in scene.prims} >= {0.0, 0.8, 1.5, 2.4}
    lum = lambda c: c.r + c.g + c.b
    assert any(lum(p.emission) + lum(p.diffuse) + lum(p.specular) + lum(p.refraction) == 0 for p in scene.prims)
    assert any(lum(p.refraction) > 0 and lum(p.specular) == 0 for p in scene.prims)
    assert bc.parse(rc, bc.CASE["MATERIALS_AIR"]).params.air_ior == 1.33
    cams = {c.name: bc.parse(rc, c).cameras[0] for c in bc.CASES if c.name.startswith(("MATERIALS", "CAMERA"))}
    assert cams["CAMERA_DOF"].dof_amount == 1000 and cams["CAMERA_DOF"].focal_length == 3
    assert cams["MATERIALS"].dof_amount == 0 and cams["CAMERA_ORTHO"].kind == rc.RT_CAMERA_ORTHO


@pytest.mark.parametrize("name", [c.name for c in bc.CASES])
def test_replay_is_exact(replays, name):
    """Same code, same inputs: types, directions, tints and colours bit-equal, draws as `draws_of` says."""
    _, paths, r = replays[name]
    assert (r["nan_normals"] > 100) == (name == "VERTEX_NORMALS")  # the one case that has them
    assert r["type_mismatch"] == 0 and r["type_mismatch_excluded"] == 0, r["first_mismatches"]
    assert r["draws_agree"] and r["next_missing"] == 0 and r["bad_end_type"] == 0
    assert r["camera_draws"] == ([4] if name in ("CAMERA_DOF", "die.txt") else [2])
    assert r["err"] == {"camera_direction": 0.0, "direction": 0.0, "length_renormalised": 0.0, "length_kept": 0.0,
                        "tint": 0.0, "colour": 0.0}, r["err"]
    assert r["shaded"] == r["compared"] + r["excluded"]
    if bc.CASE[name].unshaded:  # recursion 0, debug geom: every path is its camera ray's hit
        assert r["shaded"] == 0 and (paths.n == 1).all()
    else:
        assert r["shaded"] > 1000


@pytest.mark.parametrize("name", [c.name for c in bc.CASES])
def test_coverage_on_the_oracles_own_paths(replays, name):
    _, paths, r = replays[name]
    print(name, "excluded", r["excluded"], "of", r["shaded"], "classes", r["classes"], "ends", r["end_types"])
    assert r["excluded"] <= 0.5 * EXCLUDED_CAP * max(1, r["shaded"])
    if bc.CASE[name].classes:
        short = {k: (v, bc.CLASS_MIN[k]) for k, v in r["classes"].items() if v < bc.CLASS_MIN[k]}
        assert not short, short
    if name == "die.txt":  # the window sees the die
        assert (paths.type[:, 0] == bc.MISSED).mean() < 0.5
    if name.startswith("SHALLOW"):
        assert all(r["classes"][f"out_at_{b}"] == 0 for b in (3, 6, 9))
