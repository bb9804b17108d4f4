"""Shared inputs of the temporal reprojection's tests (rt_reproject_device and its host twin
rt_debug_reproject; tests/test_reproject_host.py, tests/test_reproject_gpu.py): first hits of the shipped
scenes traced analytically over rt_camera_rays' rays, random accumulators, an independent numpy fp64
projection written from Camera.cs, FrustumCamera.cs and OrthoCamera.cs, and a numpy restatement of the
history cap (step 5 of include/rtcore.h, "temporal reprojection")."""
import functools

import numpy as np

from analytic_hits import closest_hit

FRAMES = ((8, 8), (37, 19), (130, 70))
PADS = (0, 37)
FRUSTUM, ORTHO = 0, 1
KEYS = ("sum", "samples", "misses", "q", "batches")
LOOSE = dict(sigma_z=0.05, normal_cos_min=0.9, max_history=1 << 30, flags=1)  # a max_history above every N


def bits(a):
    """An array's bytes as unsigned integers of its item size, so that NaN and -0 compare by bit pattern."""
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same(a, b):
    return np.array_equal(bits(a), bits(b))


@functools.lru_cache(maxsize=None)
def _scene(name):
    import raytracercore_amd as rc

    return rc.SceneLoader.from_file(rc.scene_path(name + ".txt"))


def camera(rc, name, index=0, **fields):
    """A copy of the scene's camera `index` with fields replaced; position, look_at and up as 3-tuples."""
    cam = rc.rt_camera.from_buffer_copy(_scene(name).cameras[index])
    return change(rc, cam, **fields)


def change(rc, cam, **fields):
    cam = rc.rt_camera.from_buffer_copy(cam)
    for k, v in fields.items():
        if k in ("position", "look_at", "up"):
            setattr(cam, k, rc.rt_vec4d(float(v[0]), float(v[1]), float(v[2]), getattr(cam, k).w))
        else:
            setattr(cam, k, v)
    return cam


def vec(v):
    return np.array([v.x, v.y, v.z], np.float64)


def _key(cam):
    return bytes(cam)


_HITS = {}


def analytic_hits(rc, name, cam, width, height):
    """The first hits of scene `name` under `cam` as a HIT_DTYPE array (height, width): rt_camera_rays' rays
    (host code) traced by tests/analytic_hits.py over the scene's rt_prim records and rounded to rt_hit's
    fp32 fields.  Read-only and cached: no device and no oracle."""
    key = (name, _key(cam), width, height)
    if key not in _HITS:
        rays = rc.camera_rays(cam, (width, height))         # [x, y]
        o = rays["origin"][..., :3].reshape(-1, 3)
        d = rays["direction"][..., :3].reshape(-1, 3)
        with np.errstate(invalid="ignore"):  # (NaN marks "no candidate" in analytic_hits)
            best = closest_hit(list(_scene(name).prims), o, d)
        hits = np.zeros(width * height, rc.HIT_DTYPE)
        hit = best["id"] >= 0
        hits["prim_id"] = best["id"]
        hits["inside"] = np.where(hit, best["inside"], 0)
        hits["distance"] = np.where(hit, best["t"], 0.0)
        with np.errstate(invalid="ignore"):
            hits["position"] = np.where(hit[:, None], best["position"], 0.0)
            hits["normal"] = np.where(hit[:, None], best["normal"], 0.0)
        out = np.ascontiguousarray(hits.reshape(width, height).T)
        out.setflags(write=False)
        _HITS[key] = out
    return _HITS[key]


def random_acc(width, height, seed, pad=0, n_max=40):
    """Random accumulators in the device layout: N = samples + misses in 0 .. n_max (about one pixel in 16
    has N == 0, one in 8 no samples), 0 .. N batches, sums and moments of any value; the elements between
    the planes hold -7."""
    rng = np.random.default_rng(seed)
    npix = width * height
    pl = npix + pad
    N = rng.integers(1, n_max + 1, npix)
    N[rng.integers(0, 16, npix) == 0] = 0
    ns = rng.integers(0, N + 1)
    ns[rng.integers(0, 8, npix) == 0] = 0
    nm = N - ns
    nb = rng.integers(0, N + 1)
    s = np.full(2 * pl + npix, -7.0)
    for c in range(3):
        s[c * pl:c * pl + npix] = rng.uniform(0.0, 3.0, npix) * ns
    return {"sum": s, "samples": ns.astype(np.uint32), "misses": nm.astype(np.uint32), "q": rng.uniform(0.0, 50.0, npix),
            "batches": nb.astype(np.uint32), "plane": pl if pad else 0, "width": width, "height": height}


def planes(flat, acc):
    npix = acc["width"] * acc["height"]
    pl = acc["plane"] or npix
    return np.stack([flat[c * pl:c * pl + npix] for c in range(3)])


def run_host(rc, acc, prev_cam, prev_hits, hits, **params):
    """reproject_host on random_acc-style accumulators with LOOSE parameters unless named; the outputs as
    flat arrays of npix (sum: (3, npix), `flat` the whole array with -7 wherever nothing was written)."""
    p = dict(LOOSE)
    p.update(params)
    W, H = acc["width"], acc["height"]
    out = rc.reproject_host(rc.reproject_params(**p), prev_cam, prev_hits, hits, acc["sum"], acc["samples"], acc["misses"],
                            acc["q"], acc["batches"], W, H, plane=acc["plane"], fill=-7.0)
    res = {k: out[k].reshape(-1) for k in ("samples", "misses", "q", "batches", "src")}
    res["flat"] = out["sum"]
    res["sum"] = planes(out["sum"], acc)
    return res


def gathered(acc, src):
    """The inputs' accumulators at the source pixels `src` (all >= 0): what an uncapped accepted pixel holds."""
    return {"sum": planes(acc["sum"], acc)[:, src], "samples": acc["samples"][src], "misses": acc["misses"][src],
            "q": acc["q"][src], "batches": acc["batches"][src]}


def padding_untouched(res, acc):
    """Nothing was written between the planes or past the frame of run_host's flat sum."""
    npix = acc["width"] * acc["height"]
    pl = acc["plane"] or npix
    flat = res["flat"]
    return all((flat[c * pl + npix:(c + 1) * pl] == -7.0).all() for c in range(2)) and (flat[2 * pl + npix:] == -7.0).all()


# ---- an independent projection (Camera.InitRender, FrustumCamera / OrthoCamera.InitRender and GetRay) ----

def _unit(v):
    return v / np.sqrt((v * v).sum())


def init_render(cam, width, height):
    """Camera.InitRender and the derived classes' in numpy fp64."""
    pos, look_at, up = vec(cam.position), vec(cam.look_at), vec(cam.up)
    look = _unit(look_at - pos)
    side = _unit(np.cross(look, -up))
    up2 = _unit(np.cross(look, side))
    side = -side
    st = dict(kind=cam.kind, position=pos, look=look, side=side, up=up2, w2=width / 2.0, h2=height / 2.0)
    if cam.kind == FRUSTUM:
        ty = np.tan(cam.fov_y / 2)
        st.update(tan_x=ty * (width / float(height)), tan_y=-ty)
    else:
        st.update(h_mult=(1 / st["w2"]) * cam.size_mult, v_mult=-(1 / st["h2"]) * (height / float(width)) * cam.size_mult)
    return st


def project(st, points):
    """Continuous pixel coordinates (fx, fy) and the depth along `look` of world points (n, 3): the inverse
    of GetRay, pixel centres at the integers."""
    v = np.asarray(points, np.float64) - st["position"]
    z, a, b = v @ st["look"], v @ st["side"], v @ st["up"]
    with np.errstate(all="ignore"):
        if st["kind"] == FRUSTUM:
            fx = st["w2"] * (1 + a / z / st["tan_x"])
            fy = st["h2"] * (1 + b / z / st["tan_y"])
        else:
            fx = st["w2"] + a / st["h_mult"]
            fy = st["h2"] + b / st["v_mult"]
    return fx, fy, z


# ---- step 5 restated ----

def luminance3(s):
    return 0.299 * s[0] + 0.587 * s[1] + 0.114 * s[2]


def restate_cap(g, max_history):
    """Step 5 of the header in vectorised numpy over gathered() accumulators whose N is above max_history."""
    ns, nm, J = (g[k].astype(np.int64) for k in ("samples", "misses", "batches"))
    N = ns + nm
    assert (N > max_history).all()
    N1 = np.full_like(N, max_history)
    ns1 = ns * N1 // N
    with np.errstate(all="ignore"):
        f = np.where(ns > 0, ns1 / np.maximum(ns, 1).astype(np.float64), 1.0)
        s1 = np.where(ns > 0, g["sum"] * f, g["sum"])
        Y, Y1 = luminance3(g["sum"]), luminance3(s1)
        J1 = np.where(J >= 2, np.minimum(J, N1), J)
        D = g["q"] - Y * Y / N
        q1 = np.where(J >= 2, D * ((J1 - 1) / np.maximum(J - 1, 1).astype(np.float64)) + Y1 * Y1 / N1, g["q"] * (N1 / N.astype(np.float64)))
    return {"sum": s1, "samples": ns1.astype(np.uint32), "misses": (N1 - ns1).astype(np.uint32), "q": q1,
            "batches": J1.astype(np.uint32)}


def ulps(a, b):
    """The distance of two finite float64 arrays in units of the last place."""
    def order(x):
        i = np.ascontiguousarray(x, np.float64).view(np.int64)
        return np.where(i < 0, np.int64(-2 ** 63) - i, i)
    return np.abs(order(a) - order(b))


# ---- the inputs tests/test_reproject_host.py's H3 and H5 and tests/test_reproject_gpu.py's G1 share ----

def moved_cameras(rc, name="bounce"):
    """(previous, current) cameras of H3: the scene's first camera, then translated and turned a little."""
    c0 = camera(rc, name)
    c1 = change(rc, c0, position=vec(c0.position) + (0.11, 0.07, -0.05), look_at=vec(c0.look_at) + (0.02, -0.03, 0.01))
    return c0, c1


def h3_inputs(rc, width, height, pad=0):
    """A frustum move over bounce: analytic hits under both cameras, random accumulators with N up to 40 and
    a cap of 24, so that copies and capped pixels both occur."""
    c0, c1 = moved_cameras(rc)
    return dict(prev_cam=c0, prev_hits=analytic_hits(rc, "bounce", c0, width, height),
                hits=analytic_hits(rc, "bounce", c1, width, height), acc=random_acc(width, height, 7 * width + height, pad),
                params=dict(LOOSE, max_history=24))


def cap_acc(width, height, seed, pad, max_history):
    """Accumulators for the cap: N in 1 .. 4 max_history, one pixel in 8 without samples (an eighth of those with
    sums of 0), one in 16 with a single sample among many misses (samples' rounds to 0), batches in
    0 .. N (so J < 2 and J > N' both occur), and moments with D = Q - Y Y / N between 0.2 Q and 0.9 Q, but one
    pixel in 50 with Q = Y Y / N as the division rounds it (D is 0 or a rounding error: no variance to keep)."""
    rng = np.random.default_rng(seed)
    npix = width * height
    pl = npix + pad
    N = rng.integers(1, 4 * max_history + 1, npix)
    ns = rng.integers(1, N + 1)
    ns[rng.integers(0, 8, npix) == 0] = 0
    one = rng.integers(0, 16, npix) == 0
    N[one], ns[one] = 4 * max_history, 1
    nb = rng.integers(0, N + 1)
    nb[rng.integers(0, 10, npix) == 0] = 1
    rgb = rng.uniform(0.1, 3.0, (3, npix)) * np.where(ns > 0, ns, (rng.integers(0, 8, npix) > 0) * 5)
    Y = luminance3(rgb)
    f = rng.uniform(0.2, 0.9, npix)
    f[rng.integers(0, 50, npix) == 0] = 0.0
    q = (Y * Y / N) / (1.0 - f)
    s = np.full(2 * pl + npix, -7.0)
    for c in range(3):
        s[c * pl:c * pl + npix] = rgb[c]
    return {"sum": s, "samples": ns.astype(np.uint32), "misses": (N - ns).astype(np.uint32), "q": q, "batches": nb.astype(np.uint32),
            "plane": pl if pad else 0, "width": width, "height": height}


def h5_inputs(rc, width, height, pad=0, max_history=32):
    """The identity move over bounce with cap_acc's accumulators."""
    c0 = camera(rc, "bounce")
    hits = analytic_hits(rc, "bounce", c0, width, height)
    return dict(prev_cam=c0, prev_hits=hits, hits=hits, acc=cap_acc(width, height, 3 * width + height, pad, max_history),
                params=dict(LOOSE, max_history=max_history))
