"""rt_reproject_device's host twin (rt_debug_reproject, no GPU) through reproject_host: the definition in
include/rtcore.h ("temporal reprojection") on first hits traced analytically over the shipped scenes --
the identity (H1), a whole-pixel ortho shift (H2), a frustum move against an independent numpy projection
(H3) --, each rejection on its own (H4), the history cap against a numpy restatement (H5), the argument
errors and the struct's layout (H6), and the twin under sanitizers in a stand-alone program."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from reproject_cases import (FRAMES, KEYS, ORTHO, PADS, analytic_hits, camera, change, gathered, h3_inputs, h5_inputs,
                             init_render, luminance3, moved_cameras, padding_untouched, project, random_acc, restate_cap,
                             run_host, same, ulps, vec)
from test_render_pixels_host import SCALARS, header_prototype

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("rt_reproject_device", "rt_debug_reproject")
SIZES = {"rt_reproject_params": 32, "rt_camera": 144, "rt_hit": 48, "void": None, "double": 8, "uint32_t": 4, "int32_t": 4}


def check_prototype(fn, name, n_params):
    """Every parameter of the header's prototype against the bound argtypes: the scalar widths exactly, a
    pointer for a pointer (c_void_p, or POINTER of an element of the size the header names)."""
    ret, params = header_prototype(name)
    assert ret == "int" and fn.restype is C.c_int
    assert len(params) == len(fn.argtypes) == n_params
    for ctype, bound in zip(params, fn.argtypes):
        if ctype.endswith("*"):
            assert bound is C.c_void_p or issubclass(bound, C._Pointer), (ctype, bound)
            if bound is not C.c_void_p:
                assert C.sizeof(bound._type_) == SIZES[ctype.rstrip("*").replace("const", "").strip()], (ctype, bound)
        else:
            assert bound is SCALARS[ctype], (ctype, bound)


def _equal_to_source(res, acc, ok, src):
    """The accepted pixels `ok` hold the accumulators of their source pixels bit for bit."""
    g = gathered(acc, src[ok])
    return same(res["sum"][:, ok], g["sum"]) and all(same(res[k][ok], g[k]) for k in KEYS[1:])


def _empty(res, mask):
    return ((res["src"][mask] == -1).all() and all((bits_zero(res[k][mask]) for k in KEYS[1:])) and
            bits_zero(res["sum"][:, mask]))


def bits_zero(a):
    return not np.ascontiguousarray(a).view(np.uint8).any()


def test_exported_bound_and_sized(rc):
    lib = rc.load_library()
    out = subprocess.run(["nm", "-D", "--defined-only", rc.LIB_PATH], capture_output=True, text=True).stdout
    for name in NAMES:
        assert f" T {name}\n" in out
        assert getattr(lib, name).argtypes is not None
    assert rc.ABI_VERSION == 6 == lib.rt_abi_version()
    check_prototype(lib.rt_reproject_device, "rt_reproject_device", 19)
    check_prototype(lib.rt_debug_reproject, "rt_debug_reproject", 18)
    for name in ("primary_hits", "reproject", "denoise", "render_adaptive"):
        assert callable(getattr(rc.GpuRaytracer, name))
    assert callable(rc.reproject_device) and callable(rc.reproject_host) and callable(rc.reproject_params)
    assert rc.REPROJECT_DEFAULTS == dict(sigma_z=0.05, normal_cos_min=0.9, max_history=32, flags=rc.RT_REPROJECT_SAME_PRIM)
    with pytest.raises(TypeError):
        rc.reproject_params(sigma_l=1.0)


# ---------------------------------------------------------------- H1
@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("width,height", FRAMES)
@pytest.mark.parametrize("name", ["bounce", "die"])
def test_h1_identity(rc, name, width, height, pad):
    """H1: the previous camera is the current one and max_history is above every N.  Every pixel with a hit
    maps to itself, src == p, and keeps its five accumulators bit for bit unless its N is 0 -- a hit whose
    normal is NaN (rt_debug_ray.normal's quirk inside a vertex-normal triangle) excepted, which step 3
    rejects; every miss pixel is empty; nothing is written between the planes or past the frame."""
    cam = camera(rc, name)
    hits = analytic_hits(rc, name, cam, width, height)
    acc = random_acc(width, height, width + height, pad)
    res = run_host(rc, acc, cam, hits, hits)
    flat = hits.reshape(-1)
    hit = flat["prim_id"] >= 0
    usable = hit & np.isfinite(flat["normal"]).all(-1)
    assert hit.sum() >= 0.2 * hit.size and (~hit).any() and (hit & ~usable).sum() <= 0.02 * hit.size
    N = acc["samples"].astype(np.int64) + acc["misses"]
    ok = usable & (N > 0)
    p = np.arange(width * height)
    assert np.array_equal(res["src"][ok], p[ok])
    assert _equal_to_source(res, acc, ok, res["src"])
    assert _empty(res, ~ok)
    assert padding_untouched(res, acc)


# ---------------------------------------------------------------- H2
def ortho_camera(rc, size_mult=2.5):
    """An ortho camera of the test's own on bounce: its first camera's position and orientation."""
    return camera(rc, "bounce", kind=ORTHO, size_mult=size_mult)


@pytest.mark.parametrize("k", [1, 5])
@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("width,height", FRAMES)
def test_h2_whole_pixel_ortho_shift(rc, width, height, pad, k):
    """H2: the current ortho camera is the previous one moved by +k * h_mult along `side`, that is k pixels.
    The world point under the current pixel (x, y) lay under (x + k, y) before, so every accepted pixel has
    src == p + k exactly, columns x >= width - k have no source in the frame and are empty, and the outputs
    equal the source's accumulators bit for bit."""
    c0 = ortho_camera(rc)
    st = init_render(c0, width, height)
    step = k * st["h_mult"] * st["side"]
    c1 = change(rc, c0, position=vec(c0.position) + step, look_at=vec(c0.look_at) + step)
    prev_hits, hits = analytic_hits(rc, "bounce", c0, width, height), analytic_hits(rc, "bounce", c1, width, height)
    acc = random_acc(width, height, width * k + height, pad)
    res = run_host(rc, acc, c0, prev_hits, hits)
    src = res["src"]
    ok = src >= 0
    y, x = np.divmod(np.arange(width * height), width)
    assert ok.sum() >= 0.1 * ok.size
    assert np.array_equal(src[ok], (y * width + x + k)[ok]) and (x[ok] + k < width).all()
    assert _equal_to_source(res, acc, ok, src) and _empty(res, ~ok)
    assert padding_untouched(res, acc)


# ---------------------------------------------------------------- H3
@pytest.mark.parametrize("kind", ["frustum", "ortho"])
@pytest.mark.parametrize("width,height", FRAMES)
def test_h3_the_projection_inverts_camera_rays(rc, width, height, kind):
    """The test's own projection against rt_camera_rays: origin + t * direction of pixel (x, y) projects to
    (x, y), to 1e-9 of a pixel, at several t."""
    for cam in moved_cameras(rc) if kind == "frustum" else (ortho_camera(rc), ortho_camera(rc, 0.7)):
        rays = rc.camera_rays(cam, (width, height))
        st = init_render(cam, width, height)
        x, y = np.mgrid[0:width, 0:height]
        for t in (0.5, 3.0, 40.0):
            pts = rays["origin"][..., :3] + t * rays["direction"][..., :3]
            fx, fy, z = project(st, pts.reshape(-1, 3))
            assert np.abs(fx - x.reshape(-1)).max() < 1e-9 and np.abs(fy - y.reshape(-1)).max() < 1e-9 and (z > 0).all()


@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("width,height", FRAMES)
def test_h3_frustum_move_against_the_projection(rc, width, height, pad):
    """H3: a translation plus a small change of look_at.  src of every non-empty pixel is numpy's nearest
    pixel of the projected hit position; pixels whose numpy fx or fy lies within 1e-6 of a half-integer are
    left out (at most 0.1 % of the frame); and no pixel numpy puts outside the frame or behind the camera
    is accepted."""
    I = h3_inputs(rc, width, height, pad)
    res = run_host(rc, I["acc"], I["prev_cam"], I["prev_hits"], I["hits"], **I["params"])
    flat = I["hits"].reshape(-1)
    fx, fy, z = project(init_render(I["prev_cam"], width, height), flat["position"].astype(np.float64))
    with np.errstate(invalid="ignore"):
        near_half = (np.abs(fx - np.floor(fx) - 0.5) < 1e-6) | (np.abs(fy - np.floor(fy) - 0.5) < 1e-6)
    near_half &= flat["prim_id"] >= 0  # (a miss has no position: it is empty whatever it projects to)
    assert near_half.sum() <= 0.001 * near_half.size
    qx, qy = np.floor(fx + 0.5), np.floor(fy + 0.5)
    inside = (flat["prim_id"] >= 0) & (z > 0) & (qx >= 0) & (qx < width) & (qy >= 0) & (qy < height)
    src = res["src"]
    ok = (src >= 0) & ~near_half
    assert ok.sum() >= 0.1 * ok.size
    assert inside[ok].all() and np.array_equal(src[ok], (qy * width + qx).astype(np.int64)[ok])
    assert not (src[~inside & ~near_half] >= 0).any()
    assert _empty(res, src < 0) and padding_untouched(res, I["acc"])


# ---------------------------------------------------------------- H4
def _h4_frames(rc):
    """An 8 x 8 pair of hit arrays under an axis-aligned ortho camera with h_mult = 1 and v_mult = -1, so
    that fx = 4 + a and fy = 4 - b are exact: both frames show the plane z = 5 (prim 0, normal (0, 0, -1),
    distance 5) with every pixel's position at its own centre; every pixel maps to itself."""
    cam = rc.rt_camera(ORTHO, 0, rc.rt_vec4d(0, 0, 0, 1), rc.rt_vec4d(0, 0, 1, 1), rc.rt_vec4d(0, 1, 0, 0), 0.0, 4.0, 0.0, 0.0, 0.0)
    st = init_render(cam, 8, 8)
    assert st["h_mult"] == 1.0 and st["v_mult"] == -1.0
    assert all(np.abs(st[k]).max() == 1.0 and np.abs(st[k]).sum() == 1.0 for k in ("look", "side", "up"))
    y, x = np.mgrid[0:8, 0:8]
    hits = np.zeros((8, 8), rc.HIT_DTYPE)
    hits["position"] = ((x - 4.0)[..., None] * st["side"] + (4.0 - y)[..., None] * st["up"] + 5.0 * st["look"])
    hits["normal"] = (0.0, 0.0, -1.0)
    hits["distance"] = 5.0
    return cam, st, hits


def _at(st, a, b, z=5.0):
    """The fp32 world position a * side + b * up + z * look, which the H4 camera projects to (4 + a, 4 - b)
    exactly at depth z; a and b are fp32 numbers."""
    p = np.float64(np.float32(a)) * st["side"] + np.float64(np.float32(b)) * st["up"] + z * st["look"]
    assert np.array_equal(p.astype(np.float32).astype(np.float64), p)
    return p.astype(np.float32)


def test_h4_each_rejection_on_its_own(rc):
    """H4: one pixel per reason on the hand-made frames; each is decided as the header says and every other
    pixel still maps to itself."""
    cam, st, base = _h4_frames(rc)
    cur, prev = base.copy(), base.copy()
    acc = random_acc(8, 8, 5)
    acc["samples"][:] = np.maximum(acc["samples"], 1)  # N > 0 everywhere but where the test says
    F = np.float32
    thr = F(0.05) * F(5.0)
    up = lambda v: np.nextafter(F(v), F(np.inf))  # noqa: E731
    down = lambda v: np.nextafter(F(v), F(-np.inf))  # noqa: E731
    want = {}          # (x, y) -> expected source (x, y) or None

    def pix(x, y, expect):
        want[(x, y)] = expect

    cur["prim_id"][0, 0] = -1; pix(0, 0, None)                                   # current miss
    cur["position"][0, 1, 1] = np.inf; pix(1, 0, None)                           # non-finite position
    cur["position"][0, 2, 0] = np.nan; pix(2, 0, None)
    cur["position"][0, 3] = _at(st, -1, 4, 0.0); pix(3, 0, None)                 # z == 0
    cur["position"][0, 4] = _at(st, 0, 4, -5.0); pix(4, 0, None)                 # z < 0
    # off-frame at the four sides and the exact edges: fx = -0.5 is pixel 0, fx = width - 0.5 is outside
    cur["position"][1, 0] = _at(st, -4.5, 3); pix(0, 1, (0, 1))                  # fx = -0.5
    cur["position"][1, 1] = _at(st, down(-4.5), 3); pix(1, 1, None)              # fx just below -0.5
    cur["position"][1, 2] = _at(st, 3.5, 3); pix(2, 1, None)                     # fx = 7.5
    cur["position"][1, 3] = _at(st, down(3.5), 3); pix(3, 1, (7, 1))             # fx just below 7.5
    cur["position"][1, 4] = _at(st, 0, 4.5); pix(4, 1, (4, 0))                   # fy = -0.5
    cur["position"][1, 5] = _at(st, 0, up(4.5)); pix(5, 1, None)                 # fy just below -0.5
    cur["position"][1, 6] = _at(st, 0, -3.5); pix(6, 1, None)                    # fy = 7.5
    cur["position"][1, 7] = _at(st, 0, up(-3.5)); pix(7, 1, (4, 7))              # fy just below 7.5
    prev["prim_id"][2, 0] = -1; pix(0, 2, None)                                  # source miss
    prev["prim_id"][2, 1] = 3; pix(1, 2, None)                                   # other prim (flag set)
    prev["inside"][2, 2] = 1; pix(2, 2, None)                                    # other inside
    cur["normal"][2, 3] = (np.sqrt(1 - 0.89 ** 2), 0.0, -0.89); pix(3, 2, None)  # normal below the stop
    cur["normal"][2, 4] = (np.sqrt(1 - 0.91 ** 2), 0.0, -0.91); pix(4, 2, (4, 2))
    cur["normal"][2, 5] = (np.nan, 0.0, -1.0); pix(5, 2, None)                   # NaN normal, either side
    prev["normal"][2, 6] = (0.0, np.nan, -1.0); pix(6, 2, None)
    prev["position"][3, 0, 2] = F(5) + thr; pix(0, 3, (0, 3))                    # plane distance just inside
    prev["position"][3, 1, 2] = up(F(5) + thr); pix(1, 3, None)                  # ... and just outside
    prev["position"][3, 2, 2] = F(5) - thr; pix(2, 3, (2, 3))
    prev["position"][3, 3, 2] = down(F(5) - thr); pix(3, 3, None)
    acc["samples"][4 * 8 + 0] = acc["misses"][4 * 8 + 0] = 0; pix(0, 4, None)    # N == 0
    assert F(5) + thr - F(5) == thr and up(F(5) + thr) - F(5) > thr

    def check(res, expect):
        src = res["src"].reshape(8, 8)
        for yy in range(8):
            for xx in range(8):
                e = expect.get((xx, yy), (xx, yy))
                assert src[yy, xx] == (-1 if e is None else e[1] * 8 + e[0]), (xx, yy, src[yy, xx], e)
        ok = res["src"] >= 0
        assert _equal_to_source(res, acc, ok, res["src"]) and _empty(res, ~ok)

    check(run_host(rc, acc, cam, prev, cur), want)
    # without RT_REPROJECT_SAME_PRIM another prim_id is accepted
    check(run_host(rc, acc, cam, prev, cur, flags=0), {**want, **{(1, 2): (1, 2)}})
    # the stops are the parameters': a wider normal stop and a wider plane stop accept their pixels
    check(run_host(rc, acc, cam, prev, cur, normal_cos_min=0.85), {**want, **{(3, 2): (3, 2)}})
    check(run_host(rc, acc, cam, prev, cur, sigma_z=0.06), {**want, **{(1, 3): (1, 3), (3, 3): (3, 3)}})


# ---------------------------------------------------------------- H5
@pytest.mark.parametrize("max_history", [32, 5])
@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("width,height", FRAMES)
def test_h5_the_cap(rc, width, height, pad, max_history):
    """H5: N up to 4 max_history.  Pixels at or below the cap are copies; above it samples' + misses' ==
    max_history, the integers equal the numpy restatement of step 5 and the doubles lie within 4 ulp of it
    (its operation order may differ); the per-sample variance s2 derived from the outputs equals the
    inputs' within 1e-12 relative wherever J >= 2 and D > 1e-9 Q, and at most 5 % of those pixels are left
    out by that condition."""
    I = h5_inputs(rc, width, height, pad, max_history)
    acc = I["acc"]
    res = run_host(rc, acc, I["prev_cam"], I["prev_hits"], I["hits"], **I["params"])
    src = res["src"]
    ok = src >= 0
    assert ok.sum() >= 0.2 * ok.size and np.array_equal(src[ok], np.arange(ok.size)[ok])
    N = acc["samples"].astype(np.int64) + acc["misses"]
    capped = ok & (N > max_history)
    assert capped.sum() >= 0.3 * ok.sum() and (ok & ~capped).any()
    assert _equal_to_source(res, acc, ok & ~capped, src) and _empty(res, ~ok) and padding_untouched(res, acc)
    g = gathered(acc, np.flatnonzero(capped))
    want = restate_cap(g, max_history)
    got = {k: (res[k][:, capped] if k == "sum" else res[k][capped]) for k in KEYS}
    assert (got["samples"].astype(np.int64) + got["misses"] == max_history).all()
    for k in ("samples", "misses", "batches"):
        assert np.array_equal(got[k], want[k]), k
    assert np.isfinite(got["sum"]).all() and np.isfinite(got["q"]).all()
    assert ulps(got["sum"], want["sum"]).max() <= 4 and ulps(got["q"], want["q"]).max() <= 4
    if pad == 0:  # the cases the inputs are meant to hold
        J, ns = g["batches"], g["samples"]
        assert (ns == 0).any() and ((ns > 0) & (got["samples"] == 0)).any() and (J < 2).any() and (J > max_history).any()
    # the variance estimate is kept
    J, J1 = g["batches"].astype(np.float64), got["batches"].astype(np.float64)
    est = g["batches"] >= 2
    Y, Y1 = luminance3(g["sum"]), luminance3(got["sum"])
    Ng = N[capped].astype(np.float64)
    D = g["q"] - Y * Y / Ng
    keep = est & (D > 1e-9 * g["q"])
    left_out = 1.0 - keep.sum() / est.sum()
    print(f"H5 {width}x{height} max_history {max_history}: {est.sum()} capped pixels with J >= 2, {100 * left_out:.2f} % left out")
    assert left_out <= 0.05
    s2_in = D[keep] / (J[keep] - 1)
    s2_out = (got["q"][keep] - Y1[keep] * Y1[keep] / max_history) / (J1[keep] - 1)
    assert (np.abs(s2_out - s2_in) <= 1e-12 * s2_in).all(), float(np.max(np.abs(s2_out - s2_in) / s2_in))


# ---------------------------------------------------------------- H6
def test_h6_bad_arguments(rc):
    lib = rc.load_library()
    W = H = 8
    z, zo = np.zeros(64, np.uint32), np.zeros(64, np.uint32)
    d, q, out, oq = np.zeros(192), np.zeros(64), np.zeros(192), np.zeros(64)
    hits = np.zeros(64, rc.HIT_DTYPE)
    src = np.zeros(64, np.int32)
    cam = camera(rc, "bounce")
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    par = lambda **kw: C.byref(rc.reproject_params(**dict(rc.REPROJECT_DEFAULTS, **kw)))  # noqa: E731
    good = [par(), C.byref(cam), ptr(hits), ptr(hits), ptr(d), ptr(z), ptr(z), ptr(q), ptr(z), 0, W, H, ptr(out), ptr(zo), ptr(zo),
            ptr(oq), ptr(zo), ptr(src)]
    assert lib.rt_debug_reproject(*good) == 0
    no_src = list(good)
    no_src[17] = None
    assert lib.rt_debug_reproject(*no_src) == 0
    nulls = [(k, None) for k in (0, 1, 2, 3, 4, 5, 6, 7, 8, 12, 13, 14, 15, 16)]
    for k, v in nulls + [(10, 0), (11, -1), (9, 63), (12, ptr(d)), (12, ptr(d[100:]))]:
        bad = list(good)
        bad[k] = v
        assert lib.rt_debug_reproject(*bad) == -1, k
    nan = float("nan")
    for kw in (dict(sigma_z=0.0), dict(sigma_z=-1.0), dict(sigma_z=nan), dict(normal_cos_min=1.5), dict(normal_cos_min=-1.01),
               dict(normal_cos_min=nan), dict(max_history=0), dict(flags=2), dict(flags=0x80000001)):
        bad = list(good)
        bad[0] = par(**kw)
        assert lib.rt_debug_reproject(*bad) == -1, kw
    for kw in (dict(normal_cos_min=-1.0), dict(normal_cos_min=1.0), dict(max_history=1), dict(flags=0)):
        assert lib.rt_debug_reproject(*([par(**kw)] + good[1:])) == 0, kw
    for k in range(4):
        p = rc.reproject_params()
        p.reserved[k] = 1
        assert lib.rt_debug_reproject(*([C.byref(p)] + good[1:])) == -1
    for kind in (2, -1):
        assert lib.rt_debug_reproject(*([good[0], C.byref(change(rc, cam, kind=kind))] + good[2:])) == -1
    assert lib.rt_debug_reproject(*([good[0], C.byref(change(rc, cam, kind=ORTHO, size_mult=2.0))] + good[2:])) == 0
    dof = change(rc, cam, dof_amount=0.2, focal_length=3.0)  # a depth-of-field camera is accepted
    assert lib.rt_debug_reproject(*([good[0], C.byref(dof)] + good[2:])) == 0
    big = list(good)
    big[10], big[11] = 1 << 16, 1 << 16  # 2^32 pixels: refused before anything is read
    assert lib.rt_debug_reproject(*big) == -1
    # the device entry refuses the same before it touches a device
    assert lib.rt_reproject_device(*([None] * 9 + [0, 8, 8] + [None] * 7)) == -1
    assert lib.rt_reproject_device(*([par(max_history=0)] + good[1:] + [None])) == -1
    with pytest.raises(rc.RtError, match="max_history"):
        rc.reproject_host(rc.reproject_params(max_history=0), cam, hits, hits, d, z, z, q, z, W, H)


def test_h6_params_layout(rc, tmp_path):
    """tests/host/reproject_layout.c compiled as C99 against include/rtcore.h: 32 B and every offset, as the
    ctypes structure has them."""
    exe = str(tmp_path / "reproject_layout")
    subprocess.run(["cc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", exe,
                    os.path.join(ROOT, "tests", "host", "reproject_layout.c")], check=True)
    lines = [ln.split() for ln in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split("\n") if ln]
    assert lines[0] == ["sizeof", "32"] and C.sizeof(rc.rt_reproject_params) == 32
    want = [("sigma_z", 0, 4), ("normal_cos_min", 4, 4), ("max_history", 8, 4), ("flags", 12, 4), ("reserved", 16, 16)]
    assert [(n, int(o), int(s)) for n, o, s in lines[1:6]] == want
    assert [n for n, _ in rc.rt_reproject_params._fields_] == [n for n, _, _ in want]
    for name, off, size in want:
        cf = getattr(rc.rt_reproject_params, name)
        assert (cf.offset, cf.size) == (off, size), name
    assert lines[6] == ["same_prim", "1", "abi", "6"] and rc.RT_REPROJECT_SAME_PRIM == 1


def test_host_twin_under_sanitizers():
    """The twin in a stand-alone program built with AddressSanitizer and UndefinedBehaviorSanitizer over the
    library's host code (`make reproject_host_check_asan`, tests/host/reproject_host_check.cpp): the
    identity, the rejections and the argument errors over frames 8 x 8, 37 x 19 and 130 x 70, each also with
    a padded plane, every array allocated at its exact size; the sanitizers report nothing, leaks included."""
    csrc = os.path.join(ROOT, "raytracercore_amd", "csrc")
    subprocess.run(["make", "-s", "-C", csrc, "-j8", "reproject_host_check_asan"], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    out = subprocess.run([os.path.join(csrc, "_obj_asan", "reproject_host_check")], capture_output=True, text=True, env=env,
                         timeout=300)
    assert out.returncode == 0 and "ok reproject 3 frames" in out.stdout and "ok rejections" in out.stdout and \
        "ok arguments" in out.stdout, out.stdout + out.stderr
    assert "Sanitizer" not in out.stderr and "runtime error" not in out.stderr, out.stderr
