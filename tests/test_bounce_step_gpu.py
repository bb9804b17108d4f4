"""shade() of the path kernels, bounce by bounce, against an fp64 replay of the shading.

rt_trace_paths records, per bounce, the ray that was traced, the hit normal and `inside` the shading used,
the tint before the bounce and the resulting type, cos_in and Fresnel ratio; the next record holds the ray
and the tint that shade() made.  Each record's own inputs, widened to fp64, go to the oracle's bounce step
(orc_shade_steps: the function the oracle's get_color runs) with the uniforms shade() consumed there: the
stream is keyed by (seed, pixel, sample) and the cursor follows from the recorded types.  So the kernel
answers for every bounce of every path, whether or not an earlier bounce of the path took another branch
than the oracle's own path did.  tests/bounce_cases.py holds the cases and the comparison,
tests/test_bounce_step_host.py proves the replay exact on the oracle's own paths.

A decision (lobe choice, total internal reflection, cos >= 0, the side of a specular ray) whose margin in
fp64 is under THRESHOLD = 8 x the cos_in bound can fall either way in fp32: such bounces are counted, not
compared, and may be at most 2 % of a case's bounces.  Fresnel ratios at sin_out > 0.995 are left out as
in test_paths_against_oracle (at most 10 % of the ones kept).

Bounds (bounce_cases.BOUNDS): 4 x the largest error measured on an MI355X over all cases and modes,
rounded up to one digit.  Measured maximum -> bound:
    cos_in, absolute                         4.79e-7 (MATERIALS, BRUTE)     -> 2e-6   (THRESHOLD 1.6e-5)
    fresnel, absolute                        9.81e-6 (bounce.txt, BRUTE)    -> 4e-5
    direction, max-norm of the difference    5.75e-6 (MATERIALS, BVH)       -> 3e-5
    length, rays renormalised for the next   1.22e-7 (CAMERA_ORTHO, BVH)    -> 5e-7
    length, rays kept as they are            1.32e-6 (MATERIALS, BRUTE)     -> 6e-6
    tint, relative                           1.17e-7 (bounce.txt, BRUTE)    -> 5e-7
    colour, relative to max(1, |c|)          5.91e-8 (MATERIALS, BRUTE)     -> 3e-7
    camera origin, absolute                  2.18e-7 (CAMERA_ORTHO, BRUTE)  -> 9e-7
    camera direction, absolute               2.09e-7 (die.txt, BRUTE)       -> 9e-7
No type differed from the oracle's in any case or mode, even with no exclusion at all; the excluded
share was at most 0.05 % of a case's bounces.  The length of the next direction is held apart for the
rays shade() renormalises (next bounce index a multiple of 3: the step's vector has length 1) and for
the others, which carry a drift of about 1e-6 on both sides: a kernel that renormalises one bounce
early reaches bounces 3, 6 and 9 with that drift (measured 1.4e-6 on MATERIALS, 5.5e-7 on MATERIALS_AIR)
and fails the first bound.  VERTEX_NORMALS is the case with NaN normals (smooth triangles hit from
behind): there the type and the cursor are checked, nothing else.

The first run found one thing.  Before shade() brought a sphere's normal back to unit length the
maxima were cos_in 8.07e-5, fresnel 1.98e-4 and direction 2.79e-4, all on the glass spheres (ior 1.5,
hits from inside, bounces 2 to 5, CAMERA_ORTHO and MATERIALS in the BVH modes worst): an fp32 direction
drifts from unit length by up to 5e-6 between the renormalising bounces, the sphere test takes |d| = 1,
so the hit point lay off the sphere and p/r - c/r was off unit length by up to 2e-5; the Fresnel ratio
and the refracted ray magnify that near the critical angle.
"""
import numpy as np
import pytest

import bounce_cases as bc
from bounce_cases import BOUNDS, CLASS_MIN, EXCLUDED_CAP, FRESNEL_LEFT_OUT_CAP, THRESHOLD
from test_trace_paths_gpu import _check_rules, _colors_equal_1spp

pytestmark = pytest.mark.gpu

PARAMS = [(c.name, m) for c in bc.CASES for m in c.modes]


def trace_and_compare(rc, case, mode, link_renders=False):
    """One rt_trace_paths call of the case in this mode, and its comparison (bounce_cases.compare)."""
    scene = bc.parse(rc, case)
    gpu = rc.GpuRaytracer(scene, 0, size=case.size, traversal=getattr(rc, "RT_TRAVERSAL_" + mode))
    try:
        assert gpu.info().traversal == getattr(rc, "RT_TRAVERSAL_" + mode)
        rec, n, col = gpu.trace_paths(*case.tile, case.spp, seed=case.seed)
        _check_rules(rc, rec, n, gpu.params.recursion)
        if link_renders:  # the traced samples are the rendered ones (scene-specialised kernels on)
            _colors_equal_1spp(gpu, col, case.tile, case.seed, 0)
    finally:
        gpu.close()
    orc = bc.oracle_of(rc, case, scene)
    return bc.compare(case, scene, orc, bc.paths_of_records(case, rec, n, col), THRESHOLD)


@pytest.mark.parametrize("name,mode", PARAMS)
def test_every_bounce_against_the_fp64_step(rc, name, mode):
    case = bc.CASE[name]
    r = trace_and_compare(rc, case, mode, link_renders=name == "MATERIALS")
    print(f"{name} {mode}: " + ", ".join(f"{k} {v:.3g}" for k, v in r["err"].items()))
    print(f"  shaded {r['shaded']}, excluded {r['excluded']} ({r['excluded'] / max(1, r['shaded']):.4%}), NaN normals "
          f"{r['nan_normals']}, Fresnel kept {r.get('fresnel_kept')} left out {r.get('fresnel_left_out')}, "
          f"ends {r['end_types']}, classes {r['classes']}")
    # the bookkeeping: every path ends on an ending type, every continuing bounce has its next record
    assert r["bad_end_type"] == 0 and r["next_missing"] == 0 and r["draws_agree"] and r["origin_mismatch"] == 0
    assert r["camera_draws"] == ([4] if name in ("CAMERA_DOF", "die.txt") else [2])
    # types: equal wherever no decision is marginal (also under a NaN normal, whose step decides without it)
    assert r["type_mismatch"] == 0 and r["type_mismatch_nan"] == 0, r["first_mismatches"]
    assert r["fresnel_nan_mismatch"] == 0 and r["fresnel_tir_mismatch"] == 0
    for k, v in r["err"].items():
        assert v <= BOUNDS[k], (k, v, BOUNDS[k])
    # the caps (conditions, not measurements)
    assert r["excluded"] <= EXCLUDED_CAP * max(1, r["compared"])
    assert r["fresnel_left_out"] <= FRESNEL_LEFT_OUT_CAP * max(1, r["fresnel_kept"])
    assert (r["nan_normals"] > 100) == (name == "VERTEX_NORMALS")  # the one case that has them
    if case.classes:
        short = {k: (v, CLASS_MIN[k] // 2) for k, v in r["classes"].items() if v < CLASS_MIN[k] // 2}
        assert not short, short
    if case.unshaded:
        assert r["shaded"] == 0 and r["end_types"].keys() <= {bc.RECURSION_COMPLETE, bc.MISSED, bc.DEBUG}
    else:
        assert r["compared"] > 1000
