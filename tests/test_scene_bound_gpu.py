"""The scene bound on the device: the skip changes no result.

A wave of camera rays of which none meets the scene bound skips its closest-hit query (path_body,
kernels_path.hip).  RTCORE_SCENE_BOUND=0 turns the skip off for the launches that follow; sums, samples,
misses and the ray count must be bit-identical with it and without, on the scene-specialised build and
on the generic one (rt_set_jit(0)), in the flat and the grouped order, for tiles and for caller-supplied
rays.
"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# a lit plane behind a sphere: every camera ray that misses the sphere (and so the bound) meets the plane
PLANE_BEHIND = ("size 64 48\ncamera 0 -6 0, 0 0 0, 0 0 1, 60\ntwosided true\nemission 1 1 1\ndiffuse .5 .5 .5\n"
                "plane 3 0 1 0\nemission 0 0 0\nsphere 0 0 0 .5\n")
PLANES_ONLY = "size 40 24\nambient color .2 .3 .4\ncamera 0 -4 3, 0 0 0, 0 0 1, 60\ndiffuse .5 .5 .5\nplane 0 0 0 1\n"
EMPTY = "size 40 24\ncamera 0 -4 3, 0 0 0, 0 0 1, 60\n"


def _bounce_ortho(rc):
    src = open(rc.scene_path("bounce.txt")).read()
    cam = "camera 2.8 -2.8 -1, 0 0 -1, 0 0 -1, 90"
    assert cam in src
    return src.replace(cam, "orthographic 2.8 -2.8 -1, 0 0 -1, 0 0 -1, 4", 1)


def _with_bound(on, fn):
    """fn() with the skip on (the default) or off."""
    old = os.environ.pop("RTCORE_SCENE_BOUND", None)
    try:
        if not on:
            os.environ["RTCORE_SCENE_BOUND"] = "0"
        return fn()
    finally:
        os.environ.pop("RTCORE_SCENE_BOUND", None)
        if old is not None:
            os.environ["RTCORE_SCENE_BOUND"] = old


def _same(a, b):
    (sa, na, ma, ra), (sb, nb, mb, rb) = a, b
    return ra == rb and np.array_equal(na, nb) and np.array_equal(ma, mb) and sa.tobytes() == sb.tobytes()


# (case, scene, camera, frame size, spp, traversal)
TILE_CASES = [
    # 24 x 13.5 blocks of 8x8: by the oracle 220 all-miss, 55 all-hit and 37 mixed ones, and a ragged last row
    ("bounce_cam0", "bounce.txt", 0, (192, 108), 8, "BRUTE"),
    ("bounce_cam0_grouped", "bounce.txt", 0, (192, 108), 8, "GROUPED"),
    ("bounce_cam1_inside", "bounce.txt", 1, (96, 96), 4, "BRUTE"),  # inside the room: no miss
    ("die_cam0", "die.txt", 0, (96, 96), 8, "GROUPED"),             # depth-of-field rays
    ("die_cam0_flat", "die.txt", 0, (96, 96), 8, "BRUTE"),
    ("plane_behind", PLANE_BEHIND, 0, (64, 48), 8, "BRUTE"),
    ("ortho", "ortho", 0, (96, 64), 8, "BRUTE"),
    ("planes_only", PLANES_ONLY, 0, (40, 24), 8, "BRUTE"),
    ("empty", EMPTY, 0, (40, 24), 4, "BRUTE"),
]


def _load(rc, scene):
    if scene == "ortho":
        return rc.SceneLoader.from_text(_bounce_ortho(rc))
    if scene.endswith(".txt"):
        return rc.SceneLoader.from_file(rc.scene_path(scene))
    return rc.SceneLoader.from_text(scene)


@pytest.mark.parametrize("jit", [True, False], ids=["specialised", "generic"])
@pytest.mark.parametrize("case,scene,cam,size,spp,mode", TILE_CASES, ids=[c[0] for c in TILE_CASES])
def test_skip_changes_nothing(rc, case, scene, cam, size, spp, mode, jit):
    parsed = _load(rc, scene)
    rc.set_jit(jit)
    try:
        g = rc.GpuRaytracer(parsed, cam, size=size, traversal=getattr(rc, "RT_TRAVERSAL_" + mode))
        on = _with_bound(True, lambda: g.render_tile(0, 0, size[0], size[1], spp, seed=5, sample_base=3))
        off = _with_bound(False, lambda: g.render_tile(0, 0, size[0], size[1], spp, seed=5, sample_base=3))
        if jit and case not in ("planes_only", "empty"):
            assert g.build_stats()["jit_status"] == 1.0
        g.close()
    finally:
        rc.set_jit(True)
    assert _same(on, off)
    s, n, m, rays = on
    npix = size[0] * size[1]
    assert (n + m == spp).all() and rays >= npix * spp
    if case.startswith("bounce_cam0") or case in ("die_cam0", "die_cam0_flat", "ortho"):
        # by the oracle's primary_ids 77 % (bounce.txt camera 0), 55 % (die.txt) and 73 % (orthographic) of
        # these frames' pixels look past the scene
        assert 0.4 * npix * spp < m.sum() < npix * spp
        if not case.startswith("die"):  # and whole blocks do: the frame's corner (die.txt's lens moves the origins)
            assert (m[:8, :8] == spp).all()
    if case == "bounce_cam1_inside":
        assert m.sum() == 0
    if case == "plane_behind":  # the rays that miss the bound still meet the plane
        assert m.sum() == 0 and rays > npix * spp
        assert (s.reshape(npix, 3)[0] > 0).all()  # a corner pixel: the lit plane, not the sphere
    if case == "planes_only":
        assert 0 < n.sum()
    if case == "empty":
        assert n.sum() == 0 and rays == npix * spp


def _caller_rays(rc, parsed):
    """Rays that start outside the bound and point away, start outside and cross it, start inside, and
    sit past the origin limit (the far-origin fallback), 64 of each in turn so that whole waves are of one
    kind and others are mixed; then all kinds interleaved."""
    b = rc.scene_bound(parsed.prims)
    lo, hi = b["lo"].astype(np.float64), b["hi"].astype(np.float64)
    ctr, rad = (lo + hi) / 2, float(np.linalg.norm(hi - lo)) / 2
    r = np.random.default_rng(9)

    def unit(m):
        v = r.normal(size=(m, 3))
        return v / np.linalg.norm(v, axis=1, keepdims=True)

    n = 64
    v = unit(n)
    o_out = ctr + v * (rad * r.uniform(1.5, 6, (n, 1)))
    away = (o_out, v)
    aim = r.uniform(lo, hi, (n, 3)) - o_out
    cross = (o_out, aim / np.linalg.norm(aim, axis=1, keepdims=True))
    inside = (r.uniform(lo, hi, (n, 3)), unit(n))
    o_far = ctr + unit(n) * (4.0 * float(b["limit"]))
    aim = ctr - o_far
    d_far = aim / np.linalg.norm(aim, axis=1, keepdims=True)
    d_far[::2] = unit(n)[::2]
    far = (o_far, d_far)
    kinds = [away, cross, inside, far]
    o = np.concatenate([k[0] for k in kinds])
    d = np.concatenate([k[1] for k in kinds])
    mix = r.permutation(len(o))
    assert (np.abs(o_far).sum(axis=1) > float(b["limit"])).all()
    return np.concatenate([o, o[mix]]), np.concatenate([d, d[mix]])


@pytest.mark.parametrize("jit", [True, False], ids=["specialised", "generic"])
@pytest.mark.parametrize("scene,mode", [("bounce.txt", "BRUTE"), ("die.txt", "GROUPED"), (PLANE_BEHIND, "BRUTE")],
                         ids=["bounce", "die_grouped", "plane_behind"])
def test_render_rays_skip_changes_nothing(rc, scene, mode, jit):
    parsed = _load(rc, scene)
    o, d = _caller_rays(rc, parsed)
    rc.set_jit(jit)
    try:
        g = rc.GpuRaytracer(parsed, 0, size=(64, 48), traversal=getattr(rc, "RT_TRAVERSAL_" + mode))
        on = _with_bound(True, lambda: g.render_rays(o, d, 4, 21))
        off = _with_bound(False, lambda: g.render_rays(o, d, 4, 21))
        g.close()
    finally:
        rc.set_jit(True)
    assert _same(on, off)
    s, n, m, rays = on
    assert (n + m == 4).all() and rays >= 4 * len(o)
    if scene != PLANE_BEHIND:
        assert (m[:64] == 4).all()  # pointing away from a scene without planes: primary misses, a whole wave of them
        assert n[64:192].sum() > 0  # crossing the bound, or from inside it: some meet a primitive
    else:
        assert n[:64].sum() > 0     # pointing away from the sphere, some of them towards the plane
