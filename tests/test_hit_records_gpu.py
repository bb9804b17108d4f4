"""Hit position, normal and Inside of the fp32 kernels against an analytic reference (tests/analytic_hits.py).

H1 holds RT_QUERY_FAST's full record -- prim_id, inside, distance, position, normal -- to the reference in
every traversal mode and with both BVH builders, H2 RT_QUERY_EXACT's inside and distance, H3 every bounce
of rt_trace_paths (the real shade(), hits after a bounce included).  The reference is held to the CPU
oracle in tests/test_analytic_hits_host.py.

The scene is a zoo of every form the geometric head of shade() / query_hit distinguishes: planes, spheres,
ellipsoids, flat and mirrored triangles, an axis-aligned and a rotated cube, an inverted room with a side
missing, a vertex-normal quad; one-sided, two-sided and inverted on every kind (the loader leaves the first
primitives two-sided, so a one-sided and an inverted sphere and two more planes follow the quad, and a small
ellipsoid beside the glass sphere for H3's tile).  Three cameras: the first sees the room from outside, the
second the glass sphere and that ellipsoid from 2 away, the third the vertex-normal quad.

The rays (`targeted_rays`): per primitive 128 rays toward a random point of it from an origin 0.3 - 2.5
away in a random direction (a quarter of a two-sided sphere's origins inside it); behind each
vertex-normal triangle 64 more, and 96 from 0.02 - 0.25 behind it: the quad lies at most 0.3 above the
two-sided floor, and only rays that start between the two reach its back.  4544 rays in all.  Origin and
direction are rounded to fp32 component by component and exactly those values, widened, go to the library.
The reference gets the same origin and d / |d| computed in fp64: the same line.  Its formulas are the
reference's, written for unit directions (Ray.Directional normalises), and the fp32 rounding leaves |d| - 1
at up to 1e-7, which a plain sphere's discriminant b^2 - 4c multiplies by |o - c|^2 / (r cos)^2: given the
direction as it is, the formulas move a hit at t = 3 by 1.5e-5, which is no arithmetic of the kernels'.  The
library's distance is a ray parameter, so it is compared as t |d|.

With the reference alone (`conditions`): a ray is *robust* if the reference returns the same ID and the same
Inside for it and for the four rays normalize(d +- 1e-3 a), normalize(d +- 1e-3 b), a and b orthonormal
to d.  A robust hit is *well-conditioned* if across those four the reference's distance moves by less
than 1 % of max(t, 1), and *normal-conditioned* if the reference's normal moves by less than 0.05 (a NaN
normal counts as unmoved when all four are NaN too).  Asserted for the reference alone: robust >= 0.95 of
the rays (0.990), well-conditioned >= 0.90 of the robust hits (0.964), per primitive >= 16 well-conditioned
hits (35 at least), per two-sided primitive >= 16 of them inside (38 at least), per vertex-normal triangle
>= 8 robust NaN-normal hits (111 and 72).

Measured on the MI355X (the tests print these), maxima over robust / well-conditioned / normal-conditioned
hits as each assertion takes them, no ID or Inside mismatch and every NaN normal in place in all cases:
                    distance   position   | |n| - 1 |   angle (rad)
    H1 BRUTE        3.636e-06  1.465e-05  4.471e-07     2.795e-06
    H1 GROUPED      3.636e-06  1.465e-05  4.471e-07     2.795e-06
    H1 BVH, HOST    1.977e-06  1.465e-05  4.471e-07     2.795e-06
    H1 BVH, GPU     1.977e-06  1.465e-05  4.471e-07     2.795e-06
    H3 glass tile   1.113e-06  7.854e-07  1.520e-06     2.411e-06   (BRUTE, GROUPED, BVH, BRUTE without the
    H3 quad tile    4.817e-07  5.134e-07  8.146e-07     3.129e-06    scene-specialised kernels: the same)
The position figure of H1 is taken on every robust hit as the issue sets it (a grazing ray on the two-sided
flat triangle; on well-conditioned hits it is 8.3e-07).  The bars are four times the largest H1 figure:
position 5.860e-05, | |n| - 1 | 1.788e-06, angle 1.118e-05 rad, each below 1e-4; the distance keeps
G3_DISTANCE_BAR.  H3 compares 91.4 % (glass tile: 310 Inside hits after a bounce, 294 on an ellipsoid) and
96.1 % (quad tile: 432 smooth normals) of its records under the same bars; `_record_references` says which
and why.  H2: 4500 robust rays, 1441 of them Inside hits, distance error 3.084e-15 against a bar of 5.233e-14.

What catches what (restated on the CPU on recorded answers, not run broken on a device): a far-root sphere
normal left un-negated turns 246 of H1's normal-conditioned hits and 237 of H3's compared records by pi; vn[0]
and vn[1] swapped in the vertex-normal blend turn 113 of H1's hits and 432 of H3's quad-tile records by up to
0.32 rad.  Both fail `assert ang.max() < ANGLE_BAR` in `_compare`, in H1 and in H3.
"""
import functools

import numpy as np
import pytest

from analytic_hits import HASNORMALS, MIRROR, SPHERE, TRANSFORMED, TRIANGLE, TWOSIDED, allowed, closest_hit, prim_hits
from test_query_rays_gpu import G3_DISTANCE_BAR

pytestmark = pytest.mark.gpu

# The bars of H1 and H3: four times the largest value measured on the MI355X over all H1 cases (the
# convention of G3_DISTANCE_BAR; the module's header has the table), each below the project's 1e-4.
POSITION_MEASURED_MAX = 1.465e-5
UNIT_MEASURED_MAX = 4.471e-7
ANGLE_MEASURED_MAX = 2.795e-6  # radians
POSITION_BAR = 4 * POSITION_MEASURED_MAX
UNIT_BAR = 4 * UNIT_MEASURED_MAX
ANGLE_BAR = 4 * ANGLE_MEASURED_MAX

ZOO = """size 64 48
camera 0 -6 2.5, 0 0 1, 0 0 1, 60
camera 2.2 -2.8 1.1, 2.3 -.6 .95, 0 0 1, 40
camera 1.5 1.6 .9, 0 3.5 .15, 0 0 1, 40
ambient color .2 .2 .2
diffuse .5 .5 .5
plane 0 0 0 1
sphere -2 0 1 .7
twosided true
refraction .9 .9 .9 1.5
sphere 2 0 1 .6
refraction off
twosided false
pushtransform
translate 0 1 1.5
rotate 1 2 3 40
scale 1.2 .5 .8
sphere 0 0 0 1
poptransform
pushtransform
translate 0 -2 .8
rotate 0 1 1 25
scale .4 .9 .3
twosided true
sphere .1 .2 .1 1
twosided false
poptransform
vertex -3 2 .2
vertex -1 2 .2
vertex -2 2.5 2
vertex 3 2 .2
vertex 1 2 .2
vertex 2 2.5 2
tri 0 1 2
twosided true
tri 3 4 5
twosided false
vertex -3.5 -1 .1
vertex -2.5 -1.4 .1
vertex -3.5 -1 1.3
tri 6 7 8 mirrored
vertex 3 -1 .5
vertex 4 -1 .5
vertex 3 0 .5
tri 9 10 11 mirrored
cube 0 -3.5 .5 .4 .4 .4 all
pushtransform
translate 1.5 -3 .6
rotate 0 0 1 30
cube 0 0 0 .3 .5 .3 all
poptransform
invert true
cube 0 0 4 8 8 4.5 not -y
invert false
twosided true
vertexnormal -1 3 0  -.3 -.3 1
vertexnormal 1 3 .3   0 -.3 1
vertexnormal 1 4 .3   0 .3 1
vertexnormal -1 4 0 -.3 .3 1
trinormal 0 1 2
trinormal 0 2 3
twosided false
sphere -3 -2.5 .6 .4
invert true
sphere 3 -2.5 .8 .5
plane 9 0 0 1
invert false
plane -3 0 0 1
pushtransform
translate 2.5 -.9 .9
rotate 1 0 1 35
scale .3 .2 .25
sphere 0 0 0 1
poptransform
"""

PER_PRIM, PER_VN_BEHIND, PER_VN_CLOSE = 128, 64, 96


@functools.lru_cache(maxsize=None)
def zoo_scene():
    import raytracercore_amd as rc

    return rc.SceneLoader.from_text(ZOO)


def _v3(v):
    return np.array([v.x, v.y, v.z])


def _m4(m):
    return np.array(list(m)).reshape(4, 4)


def _unit_vectors(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _basis(d):
    """a, b orthonormal to each d: a from the coordinate axis d is least aligned with."""
    e = np.eye(3)[np.argmin(np.abs(d), axis=1)]
    a = np.cross(d, e)
    a /= np.linalg.norm(a, axis=1, keepdims=True)
    return a, np.cross(d, a)


def targeted_rays(prims, per=PER_PRIM, per_behind=PER_VN_BEHIND, per_close=PER_VN_CLOSE, seed=11):
    """Rays aimed at every primitive in turn (the module's header).  Returns (o, d, target): fp32 values
    widened to fp64, and the primitive each ray was aimed at."""
    rng = np.random.default_rng(seed)
    os_, ds, targets = [], [], []
    for k, prim in enumerate(prims):
        n = per
        behind = 0
        if prim.kind == TRIANGLE:
            v0, v1, v2 = (_v3(prim.p[i]) for i in range(3))
            if prim.flags & HASNORMALS:
                behind = per_behind + per_close
                n += behind
            u, v = rng.uniform(size=n), rng.uniform(size=n)
            if not prim.flags & MIRROR:
                fold = u + v > 1
                u, v = np.where(fold, 1 - u, u), np.where(fold, 1 - v, v)
            point = v0 + u[:, None] * (v1 - v0) + v[:, None] * (v2 - v0)
        elif prim.kind == SPHERE:
            point = _v3(prim.p[0]) + prim.radius * _unit_vectors(rng, n) * rng.uniform(0.2, 1.0, (n, 1))
            if prim.flags & TRANSFORMED:
                m = _m4(prim.to_obj)
                point = point @ m[:3, :3].T + m[:3, 3]
        else:
            normal = _v3(prim.p[0])
            a, b = _basis(normal[None, :])
            point = normal * prim.radius + rng.uniform(-3.5, 3.5, (n, 1)) * a + rng.uniform(-3.5, 3.5, (n, 1)) * b
        away = _unit_vectors(rng, n)
        if behind:  # the last `behind` origins on the side the face normal e01 x e02 points away from
            face = np.cross(v1 - v0, v2 - v0)
            flip = (away[-behind:] @ face) > 0
            away[-behind:][flip] *= -1
        reach = rng.uniform(0.3, 2.5, (n, 1))
        if behind:  # the quad lies at most 0.3 above the two-sided floor: these start between the two
            reach[-per_close:] = rng.uniform(0.02, 0.25, (per_close, 1))
        origin = point + away * reach
        if prim.kind == SPHERE and prim.flags & TWOSIDED:  # a quarter of the origins inside the sphere
            q = n // 4
            inner = _v3(prim.p[0]) + prim.radius * _unit_vectors(rng, q) * rng.uniform(0.0, 0.9, (q, 1))
            if prim.flags & TRANSFORMED:
                inner = inner @ m[:3, :3].T + m[:3, 3]
            origin[:q] = inner
        d = point - origin
        os_.append(origin)
        ds.append(d / np.linalg.norm(d, axis=1, keepdims=True))
        targets.append(np.full(n, k, np.int32))
    o = np.concatenate(os_).astype(np.float32).astype(np.float64)
    d = np.concatenate(ds).astype(np.float32).astype(np.float64)
    return o, d, np.concatenate(targets)


def perturbed(d):
    """The four directions normalize(d +- 1e-3 a), normalize(d +- 1e-3 b)."""
    a, b = _basis(d)
    out = []
    for v in (a, -a, b, -b):
        dp = d + 1e-3 * v
        out.append(dp / np.linalg.norm(dp, axis=1, keepdims=True))
    return out


def _normal_moved(n0, n1):
    """|n1 - n0| per ray; 0 where both are NaN, inf where only one is."""
    nan0, nan1 = np.isnan(n0).any(axis=1), np.isnan(n1).any(axis=1)
    with np.errstate(invalid="ignore"):
        moved = np.linalg.norm(n1 - n0, axis=1)
    return np.where(nan0 & nan1, 0.0, np.where(nan0 | nan1, np.inf, moved))


def conditions(prims, o, d):
    """The reference's answers for the rays and which of them are robust, well-conditioned and
    normal-conditioned (the module's header): a dict of read-only arrays.  `length` is |d|: the reference
    gets d / |d|, so its t times 1 / length is the ray parameter the library reports."""
    length = np.linalg.norm(d, axis=1)
    d = d / length[:, None]
    ref = closest_hit(prims, o, d)
    robust = np.ones(len(o), bool)
    t_moved, n_moved = np.zeros(len(o)), np.zeros(len(o))
    for dp in perturbed(d):
        p = closest_hit(prims, o, dp)
        robust &= (p["id"] == ref["id"]) & (p["inside"] == ref["inside"])
        t_moved = np.maximum(t_moved, np.abs(p["t"] - ref["t"]))
        n_moved = np.maximum(n_moved, _normal_moved(ref["normal"], p["normal"]))
    hit = ref["id"] >= 0
    out = dict(ref, length=length, robust=robust, well=robust & hit & (t_moved < 0.01 * np.maximum(ref["t"], 1.0)),
               ncond=robust & hit & (n_moved < 0.05))
    for arr in out.values():
        arr.setflags(write=False)
    return out


def reference_rounding(prims, o, d, ref, keep):
    """The reference's own rounding on the rays `keep`: the largest |t - t_longdouble| / max(t, 1) between
    its fp64 answers `ref` and a run of the same formulas in np.longdouble (hits of the same primitive)."""
    assert np.finfo(np.longdouble).eps < np.finfo(np.float64).eps, "np.longdouble is no wider than fp64 here"
    wide = closest_hit(prims, o, d, np.longdouble)
    both = keep & (ref["id"] >= 0) & (wide["id"] == ref["id"])
    return float((np.abs(wide["t"][both] - ref["t"][both]) / np.maximum(ref["t"][both], 1.0)).max())


@functools.lru_cache(maxsize=None)
def _zoo_rays():
    """The zoo's rays and the reference's answers, computed once and shared (read-only).  The conditions
    below hold for the reference alone, so the test set cannot hollow itself out."""
    prims = zoo_scene().prims
    o, d, target = targeted_rays(prims)
    R = conditions(prims, o, d)
    nan = np.isnan(R["normal"]).all(axis=1)
    assert R["robust"].mean() >= 0.95, R["robust"].mean()
    assert R["well"].sum() >= 0.90 * (R["robust"] & (R["id"] >= 0)).sum()
    for k, prim in enumerate(prims):
        mine = R["well"] & (R["id"] == k)
        assert mine.sum() >= 16, (k, mine.sum())
        if prim.flags & TWOSIDED:
            assert (mine & R["inside"]).sum() >= 16, (k, (mine & R["inside"]).sum())
        if prim.flags & HASNORMALS:
            assert (R["robust"] & (R["id"] == k) & nan).sum() >= 8, (k, (R["robust"] & (R["id"] == k) & nan).sum())
    return dict(R, o=o, d=d, target=target, nan=nan)


def _angle(a, b):
    """The angle between unit vectors in radians, accurate near 0: 2 asin(|a - b| / 2)."""
    return 2 * np.arcsin(np.minimum(np.linalg.norm(a - b, axis=1) / 2, 1.0))


def _compare(tag, got_id, got_inside, got_t, got_pos, got_nrm, R, rob, well, ncond):
    """The assertions H1 and H3 share, on records already matched ray by ray to reference answers `R`
    (id, inside, t, position, normal; got_t is the distance, the ray parameter times |d|).  Prints the
    maxima before it asserts."""
    wrong = np.flatnonzero(rob & ((got_id != R["id"]) | (got_inside != R["inside"])))
    t_err = np.abs(got_t[well] - R["t"][well]) / np.maximum(R["t"][well], 1.0)
    hit = rob & (R["id"] >= 0)
    scale = np.maximum(np.abs(R["position"][hit]).max(axis=1), 1.0)
    p_err = np.abs(got_pos[hit] - R["position"][hit]).max(axis=1) / scale
    ref_nan = np.isnan(R["normal"]).all(axis=1)
    got_nan = np.isnan(got_nrm)
    plain = ncond & ~ref_nan
    unit_err = np.abs(np.linalg.norm(got_nrm[plain].astype(np.float64), axis=1) - 1.0)
    ang = _angle(got_nrm[plain].astype(np.float64), R["normal"][plain])
    p_well = p_err[well[hit]]
    print(f"{tag}: robust {rob.mean():.4f} well {well.sum()} ncond {ncond.sum()} id/inside mismatches {wrong.size} "
          f"max distance {t_err.max():.3e} position {p_err.max():.3e} (well-conditioned {p_well.max():.3e}) "
          f"unit {unit_err.max():.3e} angle {ang.max():.3e} nan normals {int((ref_nan & hit).sum())}")
    worst = {int(k): f"{p_err[R['id'][hit] == k].max():.1e} {unit_err[R['id'][plain] == k].max(initial=0):.1e} "
                     f"{ang[R['id'][plain] == k].max(initial=0):.1e}" for k in np.unique(R["id"][hit])}
    print(f"{tag}: max position, unit, angle per primitive {worst}")
    assert wrong.size == 0, (wrong[:8], got_id[wrong[:8]], R["id"][wrong[:8]], got_inside[wrong[:8]])
    assert t_err.max() < G3_DISTANCE_BAR
    assert p_err.max() < POSITION_BAR < 1e-4
    assert unit_err.max() < UNIT_BAR < 1e-4
    assert ang.max() < ANGLE_BAR < 1e-4
    # a NaN normal exactly where the reference's is NaN, in all three components
    assert np.array_equal(got_nan[hit].all(axis=1), ref_nan[hit]) and np.array_equal(got_nan[hit].any(axis=1), ref_nan[hit])


def _gpu(rc, mode, builder=None, camera=0):
    return rc.GpuRaytracer(zoo_scene(), camera, traversal=getattr(rc, "RT_TRAVERSAL_" + mode),
                           builder=None if builder is None else getattr(rc, "RT_BVH_BUILDER_" + builder))


# ---------------------------------------------------------------- H1: FAST against the reference
@pytest.mark.parametrize("mode,builder", [("BRUTE", None), ("GROUPED", None), ("BVH", "HOST"), ("BVH", "GPU")])
def test_h1_fast_records_against_the_reference(rc, mode, builder):
    """On robust rays prim_id and inside are the reference's; distance on well-conditioned hits within
    G3_DISTANCE_BAR; position within POSITION_BAR; on normal-conditioned hits |normal| = 1 within UNIT_BAR
    and the normal within ANGLE_BAR of the reference's; NaN normals exactly where the reference has them;
    misses and `reserved` as G3 has them."""
    R = _zoo_rays()
    gpu = _gpu(rc, mode, builder)
    info, stats = gpu.info(), gpu.build_stats()
    assert info.traversal == getattr(rc, "RT_TRAVERSAL_" + mode)
    layout = rc.brute_layout(list(zoo_scene().prims))
    print(f"H1 {mode} {builder}: build stats {stats}")
    if mode == "BVH":  # the planes stay outside the tree: tested when a query ends, after the leaves
        assert info.bvh_builder == getattr(rc, "RT_BVH_BUILDER_" + builder)
        assert layout["planes"] == 3 and stats["wide_leaves"] >= 1 and stats["wide_nodes"] >= 1
        gpu.check_bvh()
    else:  # the brute-force orders' record forms are the ones the host's layout announces
        for stat, form in (("flat_rects", "rects"), ("flat_boxes", "boxes"), ("flat_frames", "frames"),
                           ("flat_frame_boxes", "frame_boxes"), ("flat_frame_rects", "frame_rects"),
                           ("flat_tris", "tris"), ("flat_spheres", "spheres")):
            assert stats[stat] == layout[form], (stat, stats[stat], layout[form])
    hits = gpu.query_rays(R["o"], R["d"])
    gpu.close()
    _compare(f"H1 {mode} {builder}", hits["prim_id"], hits["inside"].astype(bool), hits["distance"] * R["length"],
             hits["position"], hits["normal"], R, R["robust"], R["well"], R["ncond"])
    assert np.array_equal(hits["distance"], hits["distance"].astype(np.float32).astype(np.float64))
    miss = hits["prim_id"] < 0
    assert (hits["prim_id"][miss] == -1).all() and not hits["distance"][miss].any() and not hits["inside"][miss].any()
    assert not hits["position"][miss].view(np.uint32).any() and not hits["normal"][miss].view(np.uint32).any()
    assert not hits["reserved"].any() and np.isin(hits["inside"], (0, 1)).all()


# ---------------------------------------------------------------- H2: EXACT against the reference
def test_h2_exact_inside_and_distance(rc):
    """RT_QUERY_EXACT (one case: the exact kernel ignores the traversal mode) restates the reference's
    formulas in fp64 on the direction as given, so here the analytic reference gets the direction as given
    too: prim_id and inside equal on every robust ray, the distance within the CPU test's bar, 16 times the
    reference's own rounding on these rays; position and normal stay zero."""
    R = _zoo_rays()
    prims = zoo_scene().prims
    ref = closest_hit(prims, R["o"], R["d"])
    gpu = _gpu(rc, "BRUTE")
    hits = gpu.query_rays(R["o"], R["d"], exact=True)
    gpu.close()
    rob = R["robust"] & (ref["id"] == R["id"]) & (ref["inside"] == R["inside"])
    assert rob.sum() >= R["robust"].sum() - 4  # (rays on which |d| - 1 of 1e-7 decides, if any)
    assert np.array_equal(hits["prim_id"][rob], ref["id"][rob])
    assert np.array_equal(hits["inside"][rob].astype(bool), ref["inside"][rob])
    hit = rob & (ref["id"] >= 0)
    err = np.abs(hits["distance"][hit] - ref["t"][hit]) / np.maximum(ref["t"][hit], 1.0)
    bar = 16 * reference_rounding(prims, R["o"], R["d"], ref, hit)
    print(f"H2: robust hits {hit.sum()} inside {int(ref['inside'][hit].sum())} max distance error {err.max():.3e} bar {bar:.3e}")
    assert ref["inside"][hit].sum() >= 16 * sum(1 for p in prims if p.flags & TWOSIDED)
    assert err.max() <= bar
    assert not hits["position"].view(np.uint32).any() and not hits["normal"].view(np.uint32).any()
    assert not hits["reserved"].any()


# ---------------------------------------------------------------- H3: every bounce of rt_trace_paths
H3_VIEWS = {"glass": (1, (27, 20, 8, 8)), "quad": (2, (28, 20, 8, 8))}  # camera index, tile
H3_SPP, H3_SEED = 8, 5
CLEAN = 2.0 ** -21  # four fp32 ulps at 1


def _nearest(prim, o, d, t_near):
    """Of the candidates of `prim` that Invert / TwoSided allow, the one nearest in t to t_near, per ray:
    (found, t, position, normal, inside)."""
    n = len(o)
    out = [np.zeros(n, bool), np.full(n, np.nan), np.full((n, 3), np.nan), np.full((n, 3), np.nan), np.zeros(n, bool)]
    gap = np.full(n, np.inf)
    for cand in prim_hits(prim, o, d):
        ok, inside = allowed(prim, cand)
        with np.errstate(invalid="ignore"):
            g = np.where(ok, np.abs(cand[0] - t_near), np.inf)
        take = g < gap
        gap = np.where(take, g, gap)
        out = [out[0] | take, np.where(take, cand[0], out[1]), np.where(take[:, None], cand[1], out[2]),
               np.where(take[:, None], cand[2], out[3]), np.where(take, inside, out[4])]
    return out


def _record_references(prims, rec):
    """For every record (a flat array, prim_id >= 0) the reference's candidate on the record's own primitive
    nearest in t to the recorded distance, for the record's own fp32 origin and direction (the direction
    normalised in fp64).  Conditioning, by the reference alone: the candidate is *robust* if it is still there,
    with the same Inside, for the four perturbed directions of `perturbed` and for the origin moved by
    +-1e-3 max(|o|, 1) along a, b and d (a thousand times its fp32 rounding, as for the direction: a path's
    ray starts on a surface, and where it starts there decides what it meets next); *well-conditioned* if
    across those ten t moves by less than 1 % of max(t, 1); *normal-conditioned* if, besides, the normal
    moves by less than 0.05 and the ray is *clean*: one the reference's formulas, written for unit directions
    and for a ray that leaves a sphere from a point on it, cover to fp32 rounding.  That is | |d| - 1 | <=
    CLEAN (the kernels renormalise a path's direction every third bounce, as the reference does; in between it
    drifts in fp32, here by up to 7e-7, and the sphere tests, derived for unit directions, put the hit
    2 (|d| - 1) t further along the ray), and, where the ray starts on the record's own plain sphere (within
    1e-3 r of it: a re-hit), the origin within CLEAN r of that sphere (the kernels' self-hit rule takes such
    an origin to lie on the sphere -- the far root is -2 oc.d -- so the next hit inherits its distance from
    the sphere).  DESIGN.md 4.2 has the measurements."""
    n = len(rec)
    o, d = rec["origin"].astype(np.float64), rec["direction"].astype(np.float64)
    length = np.linalg.norm(d, axis=1)
    d = d / length[:, None]
    a, b = _basis(d)
    step = 1e-3 * np.maximum(np.abs(o).max(axis=1), 1.0)[:, None]
    variants = [(o, dp) for dp in perturbed(d)] + [(o + s * step * v, d) for v in (a, b, d) for s in (1, -1)]
    R = dict(id=rec["prim_id"].copy(), t=np.full(n, np.nan), position=np.full((n, 3), np.nan),
             normal=np.full((n, 3), np.nan), inside=np.zeros(n, bool), length=length)
    found, robust = np.zeros(n, bool), np.ones(n, bool)
    t_moved, n_moved = np.zeros(n), np.zeros(n)
    for k in np.unique(rec["prim_id"]):
        sel = np.flatnonzero(rec["prim_id"] == k)
        prim = prims[k]
        found[sel], R["t"][sel], R["position"][sel], R["normal"][sel], R["inside"][sel] = \
            _nearest(prim, o[sel], d[sel], rec["distance"][sel] * length[sel])
        for ov, dv in variants:
            f, t, _, nrm, inside = _nearest(prim, ov[sel], dv[sel], R["t"][sel])
            robust[sel] &= f & (inside == R["inside"][sel])
            with np.errstate(invalid="ignore"):
                t_moved[sel] = np.maximum(t_moved[sel], np.where(f, np.abs(t - R["t"][sel]), np.inf))
            n_moved[sel] = np.maximum(n_moved[sel], _normal_moved(R["normal"][sel], nrm))
    robust &= found
    well = robust & (t_moved < 0.01 * np.maximum(R["t"], 1.0))
    clean = np.abs(length - 1.0) <= CLEAN
    for k in np.unique(rec["prim_id"]):
        prim = prims[k]
        if prim.kind == SPHERE and not prim.flags & TRANSFORMED:
            sel = np.flatnonzero(rec["prim_id"] == k)
            off = np.abs(np.linalg.norm(o[sel] - _v3(prim.p[0]), axis=1) - prim.radius) / prim.radius
            clean[sel] &= (off >= 1e-3) | (off <= CLEAN)
    return R, found, robust, well, well & clean & (n_moved < 0.05)


def _h3(rc, mode, tag):
    prims = zoo_scene().prims
    kind_of, flags_of = np.array([p.kind for p in prims]), np.array([p.flags for p in prims])
    for view, (camera, tile) in H3_VIEWS.items():
        gpu = _gpu(rc, mode, camera=camera)
        assert gpu.info().traversal == getattr(rc, "RT_TRAVERSAL_" + mode)
        rec, n_rays, _ = gpu.trace_paths(*tile, H3_SPP, seed=H3_SEED)
        gpu.close()
        per = rec.shape[-1]
        flat = rec.reshape(-1, per)
        live = np.arange(per)[None, :] < n_rays.reshape(-1)[:, None]
        r = flat[live & (flat["prim_id"] >= 0)]
        R, found, robust, well, ncond = _record_references(prims, r)
        share = ncond.mean()
        kinds, flags = kind_of[r["prim_id"]], flags_of[r["prim_id"]]
        inside_later = int((ncond & R["inside"] & (r["bounce"] >= 1)).sum())
        ellipsoid = int((ncond & (kinds == SPHERE) & ((flags & TRANSFORMED) != 0)).sum())
        smooth = int((ncond & ((flags & HASNORMALS) != 0) & ~np.isnan(R["normal"]).any(axis=1)).sum())
        print(f"{tag} {view}: records {len(r)} found {found.mean():.4f} robust {robust.mean():.4f} compared share "
              f"{share:.4f} inside at bounce >= 1 {inside_later} on an ellipsoid {ellipsoid} smooth normals {smooth} "
              f"primitives {np.unique(r['prim_id'][ncond]).tolist()}")
        # the reference has a candidate for every record but the re-hits of a vertex-normal triangle by the
        # ray that leaves it (distance 0; a rounding residual of the reference's fp64 decides them)
        lost = ~found
        assert not r["distance"][lost].any() and (flags[lost] & HASNORMALS).all() and lost.mean() < 0.01
        # only records whose candidate is normal-conditioned are compared: all of H1's assertions on those
        _compare(f"{tag} {view}", r["prim_id"], r["inside"].astype(bool), r["distance"].astype(np.float64) * R["length"],
                 r["position"], r["normal"], R, ncond, ncond, ncond)
        assert share >= 0.80
        if view == "glass":
            assert inside_later >= 16 and ellipsoid >= 16
        else:
            assert smooth >= 64
        assert np.isin(r["inside"], (0, 1)).all()


@pytest.mark.parametrize("mode", ["BRUTE", "GROUPED", "BVH"])
def test_h3_every_bounce_of_trace_paths(rc, mode):
    """Two 8x8 tiles of the zoo, 8 spp: one of its second camera, which sees the glass sphere and an ellipsoid
    from 2 away, one of its third, on the vertex-normal quad.  Every live record that hit something against
    the reference's candidate on the record's primitive nearest the recorded distance (which picks the far
    root when a path leaves the glass sphere, without restating the skip of the previous hit): distance,
    position, normal with the NaN rule, Inside."""
    _h3(rc, mode, f"H3 {mode}")


def test_h3_brute_without_scene_specialised_kernels(rc):
    rc.set_jit(False)
    try:
        _h3(rc, "BRUTE", "H3 BRUTE jit off")
    finally:
        rc.set_jit(True)
