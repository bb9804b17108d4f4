"""The scene bound on the host: rt_debug_scene_bound's box and the kernels' slab predicate, restated here.

The brute-force path kernels skip the closest-hit query of a wave of camera rays when no lane's ray
meets the padded box over every primitive but the planes (path_body / scene_meets, kernels_path.hip).
That is sound only if (a) the box holds every bounded primitive and (b) the fp32 predicate never
rejects a ray that meets one.  (a): every triangle and parallelogram vertex, and a dense sample of every
ellipsoid's surface, lies inside the box; planes do not widen it.  (b): the predicate in numpy float32
(the fma as a float64 product rounded once, the reciprocal clamped to +-2^64 as slab_rcp_lean does),
over seeded rays whose origins lie inside the bound, 1-100 x the scene extent away and 2^20 x away: every
ray for which the fp64 oracle's closest-hit query reports a bounded primitive passes, without exception,
and the far origins pass by the fallback (the origin limit), not by the pad.  (c): rays that point away
from the box, or pass it at more than the pad, are rejected, so a predicate that never rejects fails.
(d): the scene-specialised build's generated header carries the bound word for word.
"""
import numpy as np
import pytest

from oracle.oracle import OracleScene

F32 = np.float32


def _seeded_scene(seed):
    """Boxes (rotated and sheared into parallelograms), spheres, rotated and anisotropically scaled
    spheres, off the origin; every other scene gets a plane under it."""
    r = np.random.default_rng(seed)
    t = ["size 32 32", "camera 0 -9 2, 0 0 0, 0 0 1, 60", "diffuse .5 .5 .5", "twosided true"]
    off = r.uniform(-3, 3, 3) * (seed % 3)
    for _ in range(3):
        c = off + r.uniform(-2, 2, 3)
        t += ["pushtransform", "translate %g %g %g" % tuple(c), "rotate %g %g %g %g" % (*r.uniform(-1, 1, 3), r.uniform(0, 180)),
              "scale %g %g %g" % tuple(r.uniform(.3, 1.5, 3)), "cube 0 0 0 1 1 1 all", "poptransform"]
    for _ in range(2):
        t.append("sphere %g %g %g %g" % (*(off + r.uniform(-2, 2, 3)), r.uniform(.2, .8)))
    for _ in range(3):
        c = off + r.uniform(-2, 2, 3)
        t += ["pushtransform", "translate %g %g %g" % tuple(c), "rotate %g %g %g %g" % (*r.uniform(-1, 1, 3), r.uniform(0, 180)),
              "scale %g %g %g" % tuple(r.uniform(.2, 2.0, 3)), "sphere %g %g %g %g" % (*r.uniform(-.3, .3, 3), r.uniform(.3, .7)),
              "poptransform"]
    if seed % 2:
        t.append("plane 0 0 1 %g" % (off[2] - 4.0))
    return "\n".join(t) + "\n"


SCENE_NAMES = ("bounce", "die", "seeded1", "seeded2", "seeded3", "seeded4")
_cache = {}


def _scene(rc, name):
    if name not in _cache:
        if name.startswith("seeded"):
            scene = rc.SceneLoader.from_text(_seeded_scene(int(name[6:])))
        else:
            scene = rc.SceneLoader.from_file(rc.scene_path(name + ".txt"))
        _cache[name] = (scene, rc.scene_bound(scene.prims))
    return _cache[name]


def _surface_points(rc, scene):
    """World points on every bounded primitive: vertices (a parallelogram's fourth too), sphere and
    ellipsoid surfaces sampled densely (a Fibonacci lattice of 4000 directions and the six axis poles)."""
    k = np.arange(4000) + .5
    phi, z = np.pi * (1 + 5 ** .5) * k, 1 - 2 * k / 4000
    u = np.stack([np.cos(phi) * np.sqrt(1 - z * z), np.sin(phi) * np.sqrt(1 - z * z), z], 1)
    u = np.concatenate([u, np.eye(3), -np.eye(3)])
    pts = []
    for p in scene.prims:
        if p.kind == rc.RT_PRIM_TRIANGLE:
            v = np.array([[q.x, q.y, q.z] for q in p.p])
            pts.append(v)
            if p.flags & rc.RT_FLAG_MIRROR:
                pts.append((v[1] + v[2] - v[0])[None])
        elif p.kind == rc.RT_PRIM_SPHERE:
            q = np.array([p.p[0].x, p.p[0].y, p.p[0].z]) + p.radius * u
            if p.flags & rc.RT_FLAG_TRANSFORMED:  # object -> world is MatrixToObject (the reference's names)
                m = np.array(p.to_obj).reshape(4, 4)
                q = q @ m[:3, :3].T + m[:3, 3]
            pts.append(q)
    return np.concatenate(pts)


def _meets(b, o, d):
    """scene_meets (kernels_path.hip) in float32; returns (meets, by_slab, by_fallback)."""
    lo, hi, limit = b["lo"].astype(F32), b["hi"].astype(F32), F32(b["limit"])
    o, d = o.astype(F32), d.astype(F32)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        idv = np.clip(F32(1) / d, F32(-2.0 ** 64), F32(2.0 ** 64))
        oi = (o * idv).astype(F32)
        fma = lambda a, x, c: (a.astype(np.float64) * x.astype(np.float64) - c.astype(np.float64)).astype(F32)
        t0, t1 = fma(np.broadcast_to(lo, o.shape), idv, oi), fma(np.broadcast_to(hi, o.shape), idv, oi)
        tmin = np.maximum(np.fmax.reduce(np.fmin(t0, t1), axis=1), F32(0))
        tmx = np.fmin.reduce(np.fmax(t0, t1), axis=1)
        slab = ~(tmin > tmx)
        near = (np.abs(o[:, 0]) + np.abs(o[:, 1]) + np.abs(o[:, 2])).astype(F32) <= limit
        finite = np.abs((d[:, 0] + d[:, 1] + d[:, 2]).astype(F32)) < F32(np.inf)
    meets = (slab | ~near | ~finite) & (b["state"] != 1)
    return meets, slab, ~near | ~finite


@pytest.mark.parametrize("name", SCENE_NAMES)
def test_bound_contains_every_bounded_primitive(rc, name):
    scene, b = _scene(rc, name)
    assert b["state"] == 0 and b["pad"] > 0 and b["limit"] > 0
    pts = _surface_points(rc, scene)
    assert (pts >= b["lo"].astype(np.float64)).all() and (pts <= b["hi"].astype(np.float64)).all()
    # and no looser than the pad (with the ellipsoids' exact boxes): each face within pad of some point,
    # up to the lattice's resolution on a curved surface (0.2 % of a radius)
    slack = float(b["pad"]) * 1.001 + 0.004 * float(np.ptp(pts, axis=0).max())
    assert (pts.min(0) - b["lo"] <= slack).all() and (b["hi"] - pts.max(0) <= slack).all()
    # the pad as documented: 2^-18 (limit + M), limit = 1024 M
    M = float(np.abs(pts).max())
    assert float(b["limit"]) == pytest.approx(1024 * M, rel=2e-3)
    assert float(b["pad"]) == pytest.approx((1025 * M) * 2.0 ** -18, rel=2e-3)


def test_planes_do_not_widen_the_bound(rc):
    scene, b = _scene(rc, "seeded1")
    assert any(p.kind == rc.RT_PRIM_PLANE for p in scene.prims)
    without = [p for p in scene.prims if p.kind != rc.RT_PRIM_PLANE]
    b2 = rc.scene_bound(without)
    assert np.array_equal(b["lo"], b2["lo"]) and np.array_equal(b["hi"], b2["hi"]) and b["limit"] == b2["limit"]


def test_empty_and_unbounded_scenes(rc):
    planes = rc.SceneLoader.from_text("size 8 8\ncamera 0 -4 3, 0 0 0, 0 0 1, 60\nplane 0 0 0 1\n")
    for prims in (planes.prims, []):
        b = rc.scene_bound(prims)
        assert b["state"] == 1
        o = np.array([[0, 0, 1], [0, 0, 0], [5, 5, 5]], F32)
        d = np.array([[0, 0, -1], [1, 0, 0], [-1, -1, -1]], F32)
        assert not _meets(b, o, d)[0].any()  # an empty bound: no ray meets it
    scene, _ = _scene(rc, "bounce")
    prims = list((rc.rt_prim * scene.n_prims).from_buffer_copy(scene.prims))
    sph = next(p for p in prims if p.kind == rc.RT_PRIM_SPHERE)
    for bad in (float("inf"), float("nan")):
        sph.radius = bad
        b = rc.scene_bound(prims)
        assert b["state"] == 2 and b["limit"] < 0
        assert _meets(b, np.array([[50, 50, 50]], F32), np.array([[1, 1, 1]], F32))[0].all()  # no skip


def _rays(b, pts, seed, n):
    """Seeded rays: origins inside the bound, 1-100 x the extent away, and 2^20 x away; aimed at points
    of the primitives' surfaces (pts) or a little beside them, and one in five uniformly random."""
    r = np.random.default_rng(seed)
    lo, hi = b["lo"].astype(np.float64), b["hi"].astype(np.float64)
    ctr, ext = (lo + hi) / 2, float(np.linalg.norm(hi - lo))

    def unit(m):
        v = r.normal(size=(m, 3))
        return v / np.linalg.norm(v, axis=1, keepdims=True)

    o_in = r.uniform(lo, hi, (n, 3))
    o_mid = ctr + unit(n) * (ext * 10 ** r.uniform(0, 2, (n, 1)))
    o_far = ctr + unit(n) * (ext * 2.0 ** 20)
    o = np.concatenate([o_in, o_mid, o_far])
    aim = pts[r.integers(0, len(pts), 3 * n)] + r.normal(size=(3 * n, 3)) * (.02 * ext) - o
    d = aim / np.linalg.norm(aim, axis=1, keepdims=True)
    rnd = r.random(3 * n) < .2
    d[rnd] = unit(int(rnd.sum()))
    o, d = o.astype(F32), d.astype(F32)  # the kernels' rays are fp32; the oracle gets the same values
    return o, d, np.repeat(np.arange(3), n)


@pytest.mark.parametrize("name", SCENE_NAMES)
def test_no_ray_that_hits_a_bounded_primitive_is_rejected(rc, name):
    scene, b = _scene(rc, name)
    orc = OracleScene.from_abi(rc.rt_scene_params.from_buffer_copy(scene.params), list(scene.prims), list(scene.cameras))
    o, d, cls = _rays(b, _surface_points(rc, scene), 1000 + SCENE_NAMES.index(name), 400)
    meets, slab, fallback = _meets(b, o, d)
    bounded = np.array([p.kind != rc.RT_PRIM_PLANE for p in scene.prims])
    hit = np.zeros(len(o), bool)
    for i in range(len(o)):
        pid, _ = orc.raytrace((float(o[i, 0]), float(o[i, 1]), float(o[i, 2]), 1.0),
                              (float(d[i, 0]), float(d[i, 1]), float(d[i, 2]), 0.0))
        hit[i] = pid >= 0 and bounded[pid]
    for c in range(3):  # the generator does aim at the scene from every class of origin
        assert hit[cls == c].sum() >= 50, (c, int(hit[cls == c].sum()))
    assert not (hit & ~meets).any(), np.flatnonzero(hit & ~meets)[:8]
    assert not fallback[cls < 2].any()  # origins up to 100 x the extent away are served by the pad
    assert fallback[cls == 2].all()     # 2^20 x away: the fallback, whatever the slab test says


@pytest.mark.parametrize("name", SCENE_NAMES)
def test_rays_that_pass_the_box_are_rejected(rc, name):
    _, b = _scene(rc, name)
    r = np.random.default_rng(77)
    lo, hi = b["lo"].astype(np.float64), b["hi"].astype(np.float64)
    ctr, half = (lo + hi) / 2, (hi - lo) / 2
    rad = float(np.linalg.norm(half))
    v = r.normal(size=(500, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    dist = rad * 10 ** r.uniform(.1, 1.5, (500, 1))
    o = ctr + v * dist
    # pointing away from the box
    away = _meets(b, o, v)[0]
    assert not away.any()
    # towards it, but past its bounding sphere by more than the pad: aimed at a point 1.5 rad + 4 pad
    # from the centre, at right angles to the line of sight; kept where the line clears the sphere
    w = np.cross(v, r.normal(size=(500, 3)))
    w /= np.linalg.norm(w, axis=1, keepdims=True)
    aim = ctr + w * (1.5 * rad + 4 * float(b["pad"])) - o
    dd = aim / np.linalg.norm(aim, axis=1, keepdims=True)
    closest = np.linalg.norm(np.cross(ctr - o, dd), axis=1)  # the line's distance from the centre
    clear = closest > rad + 4 * float(b["pad"])
    assert clear.sum() >= 100
    assert not _meets(b, o, dd)[0][clear].any()
    # and the rays aimed at the centre are kept: the predicate is not one that rejects everything
    assert _meets(b, o, -v)[0].all()


@pytest.mark.parametrize("name,grouped", [("bounce", False), ("die", True)])
def test_specialised_header_carries_the_bound(rc, name, grouped):
    """The scene-specialised build gets the bound as literals: kSceneW of the generated header (which the
    JIT cache key hashes) holds lo | limit | hi | empty, word for word."""
    import re

    scene, b = _scene(rc, name)
    header = rc.jit_header(scene, 0, (96, 64), grouped)
    words = [int(w, 16) for w in re.search(r"kSceneW\[\d+\][^=]*= \{([^}]*)\}", header).group(1).split(",")]
    want = list(np.concatenate([b["lo"], [b["limit"]], b["hi"]]).astype(F32).view(np.uint32)) + [0]
    assert any(words[i:i + 8] == want for i in range(len(words) - 7))
