"""An analytic closest hit in numpy: the independent reference of the hit-record tests.

Written from the semantics of the reference's primitives (Triangle.RayTraceAVXFaster and GetNormal,
Sphere.RayTraceAVX, Plane.DoRayTrace, Primitive.RayTrace) and the ABI's `rt_prim` records alone: plain
textbook formulas vectorised over rays, no library call, no oracle, none of the library's derived
records.  Every function takes `dtype` (np.float64 or np.longdouble), so the reference's own rounding can
be bounded by running it twice.

A candidate hit is (t, position, normal, inside): t (n,), position (n, 3), normal (n, 3), inside (n,) bool.
Where a ray has no such candidate t is NaN (and the other fields mean nothing).  A NaN *normal* beside a
finite t is a value: Triangle.GetNormal's answer inside a vertex-normal triangle.
"""
import numpy as np

TRIANGLE, SPHERE, PLANE = 0, 1, 2
MIRROR, TWOSIDED, INVERT, HASNORMALS, TRANSFORMED = 1, 2, 4, 8, 16


def _v3(v, dtype):
    return np.array([v.x, v.y, v.z], dtype)


def _m4(m, dtype):
    return np.array(list(m), dtype).reshape(4, 4)


def _dot(a, b):
    return (a * b).sum(axis=-1)


def _unit(v):
    with np.errstate(invalid="ignore", divide="ignore"):
        return v / np.sqrt(_dot(v, v))[..., None]


def _point(m, p):  # affine map of points, w = 1
    return p @ m[:3, :3].T + m[:3, 3]


def _vector(m, v):  # its linear part, w = 0
    return v @ m[:3, :3].T


def _triangle(prim, o, d, dtype):
    """Moller-Trumbore.  Mirror (a parallelogram) accepts u, v in [0, 1], else u + v <= 1; inside = det < 0;
    the hit point is v0 + u e01 + v e02.  Flat normal normalize(e01 x e02), negated inside; with vertex
    normals normalize(n0 u + n1 v + n2 (u + v)) -- the reference's own weights -- and NaN inside (the
    reflection about a face normal that such a triangle never computes: 0 / 0)."""
    v0, v1, v2 = (_v3(prim.p[k], dtype) for k in range(3))
    e01, e02 = v1 - v0, v2 - v0
    off = o - v0
    s1, s2 = np.cross(off, e01), np.cross(d, e02)
    det = _dot(s2, e01)
    with np.errstate(invalid="ignore", divide="ignore"):
        inv = 1 / det
        inv = np.where(np.isnan(inv), 0, inv)
        u, v, t = _dot(off, s2) * inv, _dot(d, s1) * inv, _dot(e02, s1) * inv
        reject = (u < 0) | (v < 0) | (t < 0)
        reject |= ((u > 1) | (v > 1)) if prim.flags & MIRROR else (u + v > 1)
    inside = inv < 0
    pos = v0 + u[:, None] * e01 + v[:, None] * e02
    if prim.flags & HASNORMALS:
        n0, n1, n2 = (_v3(prim.n[k], dtype) for k in range(3))
        nrm = _unit(n0 * u[:, None] + n1 * v[:, None] + n2 * (u + v)[:, None])
        nrm = np.where(inside[:, None], np.nan, nrm)
    else:
        face = _unit(np.cross(e01, e02))
        nrm = np.where(inside[:, None], -face, face)
    return [(np.where(reject, np.nan, t), pos, nrm, inside & ~reject)]


def _sphere(prim, o, d, dtype):
    """Both roots of |o' + t d' - c|^2 = r^2 in object space: the close root (outside, normal (p - c) / r),
    then the far root (inside, normal negated); only the far one when the close one lies behind the
    origin.  Transformed: the ray mapped by to_world with the direction renormalised, the point mapped
    back by to_obj, the normal normalize(to_normal n), the distance d . (p - o) in world space."""
    c, r = _v3(prim.p[0], dtype), dtype(prim.radius)
    xf = bool(prim.flags & TRANSFORMED)
    oo, od = o, d
    if xf:
        to_world, to_obj, to_normal = (_m4(m, dtype) for m in (prim.to_world, prim.to_obj, prim.to_normal))
        oo, od = _point(to_world, o), _unit(_vector(to_world, d))
    off = oo - c
    b = -2 * _dot(off, od)
    cc = _dot(off, off) - r * r
    with np.errstate(invalid="ignore"):
        radix = np.sqrt(b * b - 4 * cc)
    roots = []
    for t, sign in (((b - radix) / 2, 1), ((b + radix) / 2, -1)):
        p = oo + t[:, None] * od
        n = (p - c) / r
        if xf:
            p = _point(to_obj, p)
            n = _unit(_vector(to_normal, n))
            t = _dot(d, p - o)
        roots.append((t, p, sign * n))
    (tc, pc, nc), (tf, pf, nf) = roots
    with np.errstate(invalid="ignore"):
        far_ok = tf >= 0  # (false for NaN)
        close_ok = far_ok & (tc >= 0)
    first = close_ok[:, None]
    return [(np.where(close_ok, tc, np.where(far_ok, tf, np.nan)), np.where(first, pc, pf), np.where(first, nc, nf),
             far_ok & ~close_ok),
            (np.where(close_ok, tf, np.nan), pf, nf, close_ok)]


def _plane(prim, o, d, dtype):
    """n . p = origin distance.  t = (D - n . o) / (n . d), accepted from -1e-24 on; the point is o + t d,
    the distance |p - o|; inside, with the normal negated, when n . d > 0.  A ray that lies in the plane
    hits at its origin, distance 0, inside, with the normal as it is."""
    n, dist = _v3(prim.p[0], dtype), dtype(prim.radius)
    ray_dist, denom = _dot(o, n), _dot(d, n)
    with np.errstate(invalid="ignore", divide="ignore"):
        t = (dist - ray_dist) / denom
    along = (denom == 0) & (ray_dist == dist)
    ok = ~along & (denom != 0) & (t >= -1e-24)
    pos = np.where(along[:, None], o, o + t[:, None] * d)
    inside = (ok & (denom > 0)) | along
    nrm = np.where((inside & ~along)[:, None], -n, np.broadcast_to(n, pos.shape))
    length = np.sqrt(_dot(pos - o, pos - o))
    return [(np.where(ok | along, length, np.nan), pos, nrm, inside)]


def prim_hits(prim, o, d, dtype=np.float64):
    """The candidate hits of one `rt_prim` for the rays (o, d), (n, 3) each, in the reference's order."""
    o, d = np.asarray(o, dtype).reshape(-1, 3), np.asarray(d, dtype).reshape(-1, 3)
    return {TRIANGLE: _triangle, SPHERE: _sphere, PLANE: _plane}[prim.kind](prim, o, d, dtype)


def allowed(prim, cand):
    """Primitive.RayTrace's culling of one candidate: Invert flips `inside`, and an inside hit counts only
    on a two-sided primitive.  Returns (ok, inside after Invert)."""
    t, _, _, inside = cand
    if prim.flags & INVERT:
        inside = ~inside
    ok = ~np.isnan(t)
    if not prim.flags & TWOSIDED:
        ok &= ~inside
    return ok, inside & ok


def first_hit(prim, o, d, dtype=np.float64):
    """Primitive.RayTrace(ray, null): the first candidate that survives the culling."""
    out = None
    for cand in prim_hits(prim, o, d, dtype):
        ok, inside = allowed(prim, cand)
        t, pos, nrm, _ = cand
        if out is None:
            out = [np.where(ok, t, np.nan), pos, nrm, inside]
        else:
            take = np.isnan(out[0]) & ok
            out = [np.where(take, t, out[0]), np.where(take[:, None], pos, out[1]), np.where(take[:, None], nrm, out[2]),
                   np.where(take, inside, out[3])]
    return out


def closest_hit(prims, o, d, dtype=np.float64):
    """Scene.RayTrace(ray, null) by brute force: per primitive the first surviving candidate, over the
    primitives the smallest t (the lower ID of two equal ones).  Returns a dict: id (-1: miss), t, position,
    normal, inside (0 where missed) and t2, the second smallest of the primitives' distances (inf if none)."""
    o, d = np.asarray(o, dtype).reshape(-1, 3), np.asarray(d, dtype).reshape(-1, 3)
    n = len(o)
    best = dict(id=np.full(n, -1, np.int32), t=np.full(n, np.inf, dtype), position=np.zeros((n, 3), dtype),
                normal=np.zeros((n, 3), dtype), inside=np.zeros(n, bool), t2=np.full(n, np.inf, dtype))
    for k, prim in enumerate(prims):
        t, pos, nrm, inside = first_hit(prim, o, d, dtype)
        t = np.where(np.isnan(t), np.inf, t)
        win = t < best["t"]
        best["t2"] = np.where(win, best["t"], np.minimum(best["t2"], t))
        best["id"] = np.where(win, k, best["id"])
        best["t"] = np.where(win, t, best["t"])
        best["position"] = np.where(win[:, None], pos, best["position"])
        best["normal"] = np.where(win[:, None], nrm, best["normal"])
        best["inside"] = np.where(win, inside, best["inside"])
    best["t"] = np.where(best["id"] < 0, 0, best["t"])
    return best
