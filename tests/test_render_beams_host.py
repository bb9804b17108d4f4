"""rt_render_beams, host side (no GPU): the twin rt_debug_beam_rays against a scalar numpy restatement
of rtcore.h's definition (H1) and against the formula in fp64 (H2), rt_camera_beams against
rt_camera_rays (H3), the binding, the record's layout and the panorama tool's beams (H4), and the
stand-alone sanitizer program (H5)."""
import ctypes as C
import functools
import importlib.util
import os
import subprocess

import numpy as np
import pytest

from test_render_rays_host import SCALARS, _header_prototype, _last_error

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "raytracercore_amd", "csrc")
NAMES = ("rt_render_beams", "rt_render_beams_device", "rt_debug_beam_rays", "rt_camera_beams")
FIELDS = ("origin", "direction", "origin_du", "origin_dv", "direction_du", "direction_dv")
N, SPP = 64, 5
BAD_NAN, BAD_ZERO, BAD_OVERFLOW = 9, 20, 33
M32 = 0xFFFFFFFF


# ---------------------------------------------------------------- rtcore_rng.h in Python integers
def _lowbias32(x):
    x ^= x >> 16
    x = (x * 0x7FEB352D) & M32
    x ^= x >> 15
    x = (x * 0x846CA68B) & M32
    x ^= x >> 16
    return x


def _rng_init(seed, pixel, sample):
    s0 = _lowbias32((seed + 0x9E3779B9) & M32)
    s1 = _lowbias32(((seed >> 32) & M32) ^ 0x85EBCA6B ^ s0)
    p0 = _lowbias32((pixel & M32) ^ s0)
    p1 = _lowbias32((((pixel >> 32) & M32) + p0 + s1) & M32)
    return (_lowbias32((sample & M32) ^ p0) ^ ((p1 + ((sample >> 32) & M32) * 0x9E3779B9) & M32)) | 1


def _next24(x):
    x ^= (x << 13) & M32
    x ^= x >> 17
    x ^= (x << 5) & M32
    return x, x >> 8


def _beams():
    """64 beams: base directions of length 0.2 .. 5, origins of a few units, direction footprints from
    1e-3 of the direction up to its own size, origin footprints up to 0.5; one with a NaN, one with all
    three direction vectors zero, one whose origin_du overflows fp32."""
    rng = np.random.default_rng(2024)
    b = {f: np.zeros((N, 4)) for f in FIELDS}
    b["origin"][:, :3] = rng.normal(size=(N, 3)) * 3.0
    b["origin"][:, 3] = 1.0
    d = rng.normal(size=(N, 3))
    d *= (rng.uniform(0.2, 5.0, (N, 1)) / np.linalg.norm(d, axis=1, keepdims=True))
    b["direction"][:, :3] = d
    size = np.linalg.norm(d, axis=1, keepdims=True) * 10.0 ** rng.uniform(-3, 0, (N, 1))
    for f in ("direction_du", "direction_dv"):
        v = rng.normal(size=(N, 3))
        b[f][:, :3] = v / np.linalg.norm(v, axis=1, keepdims=True) * size * rng.uniform(0.5, 1.0, (N, 1))
    for f in ("origin_du", "origin_dv"):
        b[f][:, :3] = rng.normal(size=(N, 3)) * rng.uniform(0, 0.5, (N, 1))
    b["direction_dv"][BAD_NAN, 1] = np.nan
    for f in ("direction", "direction_du", "direction_dv"):
        b[f][BAD_ZERO] = 0.0
    b["origin_du"][BAD_OVERFLOW, 2] = 1e39
    return b


def _restate(b, spp, seed, sample_base, stream_base):
    """rtcore.h's definition in scalar np.float32 operations, each rounded on its own.  Returns rays
    [n, spp, 2, 3] f32 (origin, direction; zero where there is none), uv [n, spp, 2], kind [n, spp]:
    0 a ray, 1 degenerate, 2 invalid."""
    f32 = np.float32
    n = b["origin"].shape[0]
    rays = np.zeros((n, spp, 2, 3), f32)
    uv = np.zeros((n, spp, 2))
    kind = np.zeros((n, spp), np.int32)
    with np.errstate(all="ignore"):
        for i in range(n):
            F = {f: [f32(b[f][i, c]) for c in range(3)] for f in FIELDS}
            invalid = not all(np.isfinite(b[f][i]).all() for f in FIELDS) or \
                not all(np.isfinite(x) for f in FIELDS for x in F[f])
            for k in range(spp):
                x = _rng_init(seed, stream_base + i, sample_base + k)
                x, a = _next24(x)
                x, c2 = _next24(x)
                u, v = f32(a) * f32(2.0 ** -24), f32(c2) * f32(2.0 ** -24)
                uv[i, k] = (u, v)
                if invalid:
                    kind[i, k] = 2
                    continue
                o = [(F["origin"][c] + u * F["origin_du"][c]) + v * F["origin_dv"][c] for c in range(3)]
                w = [(F["direction"][c] + u * F["direction_du"][c]) + v * F["direction_dv"][c] for c in range(3)]
                n2 = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]
                if not (np.isfinite(n2) and n2 > 0 and all(np.isfinite(x) for x in o)):
                    kind[i, k] = 1
                    continue
                ln = np.sqrt(n2)
                assert type(ln) is f32 and all(type(x) is f32 for x in o + w)
                rays[i, k, 0] = o
                rays[i, k, 1] = [x / ln for x in w]
    return rays, uv, kind


CASES = ((5, 3, 1000003), (0xDEADBEEF12345678, 2 ** 33 + 7, 2 ** 40 + 11))


@functools.lru_cache(maxsize=None)
def _twin_and_restatement(case):
    import raytracercore_amd as rc

    seed, sample_base, stream_base = CASES[case]
    b = _beams()
    rays, uv = rc.beam_rays_host(*[b[f] for f in FIELDS], SPP, seed, sample_base=sample_base, stream_base=stream_base)
    return b, rays, uv, _restate(b, SPP, seed, sample_base, stream_base)


@pytest.mark.parametrize("case", range(len(CASES)))
def test_h1_twin_equals_the_numpy_restatement(rc, case):
    """Bit for bit: origins, directions, (u, v); the all-zero ray for the invalid beams' and the
    degenerate samples; w = 1 / 0 on a ray."""
    b, rays, uv, (want, want_uv, kind) = _twin_and_restatement(case)
    assert rays.shape == (N, SPP) and rays.dtype == rc.RAY_DTYPE and uv.shape == (N, SPP, 2)
    assert (kind[BAD_NAN] == 2).all() and (kind[BAD_OVERFLOW] == 2).all() and (kind[BAD_ZERO] == 1).all()
    assert (kind == 0).sum() == (N - 3) * SPP
    assert uv.tobytes() == want_uv.tobytes()
    assert ((uv >= 0) & (uv < 1)).all() and (uv * 2.0 ** 24 == np.round(uv * 2.0 ** 24)).all()
    assert len(np.unique(uv)) > N * SPP  # (draws, not a constant)
    got_o, got_d = rays["origin"], rays["direction"]
    assert got_o[..., :3].tobytes() == want[:, :, 0].astype(np.float64).tobytes()
    assert got_d[..., :3].tobytes() == want[:, :, 1].astype(np.float64).tobytes()
    ok = kind == 0
    assert (got_o[ok][:, 3] == 1.0).all() and (got_d[..., 3] == 0.0).all() and (got_o[~ok] == 0.0).all()
    # fp32 values, widened
    assert (got_d.astype(np.float32).astype(np.float64) == got_d).all()


@pytest.mark.parametrize("case", range(len(CASES)))
def test_h2_twin_is_close_to_the_formula_in_fp64(rc, case):
    """On the valid samples of beams with |direction_du|, |direction_dv| <= |direction| (all of H1's by
    construction: nothing cancels beyond a factor the bound carries), every component of the unit
    direction is within 16 * 2^-24 of the formula evaluated in fp64 from the F-rounded inputs: at most 4
    roundings per w_c, 5 for n2, one square root, one division."""
    b, rays, uv, (_, _, kind) = _twin_and_restatement(case)
    with np.errstate(all="ignore"):
        F = {f: b[f][:, :3].astype(np.float32).astype(np.float64) for f in FIELDS}
    norm = lambda a: np.linalg.norm(a, axis=1)
    with np.errstate(all="ignore"):
        small = (norm(F["direction_du"]) <= norm(F["direction"])) & (norm(F["direction_dv"]) <= norm(F["direction"]))
    use = (kind == 0) & small[:, None]
    assert use.sum() == (N - 3) * SPP
    u, v = uv[..., 0, None], uv[..., 1, None]
    with np.errstate(all="ignore"):
        w = F["direction"][:, None] + u * F["direction_du"][:, None] + v * F["direction_dv"][:, None]
        d = w / np.linalg.norm(w, axis=2, keepdims=True)
        o = F["origin"][:, None] + u * F["origin_du"][:, None] + v * F["origin_dv"][:, None]
    err = np.abs(rays["direction"][..., :3] - d)[use]
    err_o = (np.abs(rays["origin"][..., :3] - o)[use] / np.maximum(np.abs(o[use]), 1.0))
    print(f"H2 case {case}: max |d - d64| = {err.max():.3e} = {err.max() * 2 ** 24:.2f} * 2^-24; "
          f"origin {err_o.max() * 2 ** 24:.2f} * 2^-24")
    assert err.max() <= 16 * 2.0 ** -24
    assert err_o.max() <= 16 * 2.0 ** -24


# ---------------------------------------------------------------- H3: the library's cameras
def _ortho_camera(rc, cam):
    c = rc.rt_camera.from_buffer_copy(cam)
    c.kind = rc.RT_CAMERA_ORTHO
    c.size_mult = 2.5
    return c


@pytest.mark.parametrize("kind", ["frustum", "ortho"])
def test_h3_camera_beams_against_camera_rays(rc, kind):
    """fp64, bounce camera 0 and an orthographic copy of it, a 16 x 8 tile of a 128 x 128 frame (and the
    17 x 9 one for the neighbours): at (0, 0) a beam is GetRay(x, y), at (1, 1) it is the beam of pixel
    (x + 1, y + 1) at (0, 0); normalised directions within 4 * 2^-52, origins equal (image_plane = 0)."""
    from test_query_rays_gpu import _scene

    cam = rc.rt_camera.from_buffer_copy(_scene("bounce").cameras[0])
    if kind == "ortho":
        cam = _ortho_camera(rc, cam)
    cam.image_plane = 0.0
    size, x0, y0, w, h = (128, 128), 16, 72, 16, 8
    beams = rc.camera_beams(cam, size, x0, y0, w + 1, h + 1)
    rays = rc.camera_rays(cam, size, x0, y0, w + 1, h + 1)
    assert beams.shape == (w + 1, h + 1) and beams.dtype == rc.BEAM_DTYPE and beams.itemsize == 192

    def at(b, u, v):
        o = b["origin"] + u * b["origin_du"] + v * b["origin_dv"]
        d = b["direction"] + u * b["direction_du"] + v * b["direction_dv"]
        return o[..., :3], d[..., :3] / np.linalg.norm(d[..., :3], axis=-1, keepdims=True)

    o0, d0 = at(beams, 0.0, 0.0)
    bound = 4 * 2.0 ** -52
    err = np.abs(d0 - rays["direction"][..., :3]).max()
    assert err <= bound, err
    assert np.array_equal(o0, rays["origin"][..., :3])
    assert (beams["origin"][..., 3] == 1.0).all() and not any(beams[f][..., 3].any() for f in FIELDS[1:])
    o1, d1 = at(beams[:-1, :-1], 1.0, 1.0)
    err1 = np.abs(d1 - d0[1:, 1:]).max()
    scale = max(1.0, np.abs(o0).max())
    err_o = np.abs(o1 - o0[1:, 1:]).max() / scale
    print(f"H3 {kind}: (0,0) vs GetRay {err:.2e}, (1,1) vs the neighbour {err1:.2e}, origins {err_o:.2e}")
    assert err1 <= bound and err_o <= bound
    if kind == "frustum":
        assert not beams["origin_du"].any() and not beams["origin_dv"].any() and beams["direction_du"].any()
        assert np.ptp(beams["origin"].reshape(-1, 4), axis=0).max() == 0
    else:
        assert not beams["direction_du"].any() and not beams["direction_dv"].any() and beams["origin_du"].any()
    # the tile is indexed [x, y]: u moves along x
    assert np.abs(at(beams[:-1], 1.0, 0.0)[1] - d0[1:]).max() <= bound
    assert np.abs(at(beams[:-1], 1.0, 0.0)[0] - o0[1:]).max() / scale <= bound


def test_h3_camera_beams_errors(rc):
    from test_query_rays_gpu import _scene

    lib = rc.load_library()
    cam = rc.rt_camera.from_buffer_copy(_scene("bounce").cameras[0])
    out = np.full(4, 7.0).view(np.float64)
    buf = np.zeros(16, rc.BEAM_DTYPE)
    p = buf.ctypes.data_as(C.c_void_p)
    for args in ((64, 48, 0, 0, 0, 4), (64, 48, 0, 0, 4, -1), (64, 48, 61, 0, 4, 4), (64, 48, 0, 45, 4, 4),
                 (64, 48, -1, 0, 4, 4), (0, 48, 0, 0, 4, 4)):
        assert lib.rt_camera_beams(C.byref(cam), *args, p) == -1, args
        assert "rt_camera_beams" in _last_error(lib)
    assert lib.rt_camera_beams(None, 64, 48, 0, 0, 4, 4, p) == -1
    assert lib.rt_camera_beams(C.byref(cam), 64, 48, 0, 0, 4, 4, None) == -1
    bad = rc.rt_camera.from_buffer_copy(cam)
    bad.kind = 77
    assert lib.rt_camera_beams(C.byref(bad), 64, 48, 0, 0, 4, 4, p) == -1
    assert not buf.view(np.uint8).any() and (out == 7.0).all()
    with pytest.raises(rc.RtError):
        rc.camera_beams(cam, (64, 48), 60, 0, 8, 4)


# ---------------------------------------------------------------- H4: binding and layout
def test_h4_exported_and_bound(rc):
    lib = rc.load_library()
    out = subprocess.run(["nm", "-D", "--defined-only", rc.LIB_PATH], capture_output=True, text=True).stdout
    for name in NAMES:
        assert f" T {name}\n" in out
        assert getattr(lib, name).argtypes is not None
    for name in ("render_beams", "render_beams_device"):
        assert hasattr(rc.GpuRaytracer, name)
    assert callable(rc.beam_rays_host) and callable(rc.camera_beams)
    assert C.sizeof(rc.rt_beam) == 192 == rc.BEAM_DTYPE.itemsize
    assert [f for f, _ in rc.rt_beam._fields_] == list(rc.BEAM_DTYPE.names) == list(FIELDS)
    assert [getattr(rc.rt_beam, f).offset for f in FIELDS] == [rc.BEAM_DTYPE.fields[f][1] for f in FIELDS] == \
        [0, 32, 64, 96, 128, 160]
    assert rc.ABI_VERSION == 6 == lib.rt_abi_version()  # additive: detected by symbol


@pytest.mark.parametrize("name", NAMES)
def test_h4_ctypes_prototype_matches_the_header(rc, name):
    fn = getattr(rc.load_library(), name)
    ret, params = _header_prototype(name)
    assert ret == "int" and fn.restype is C.c_int
    assert len(params) == len(fn.argtypes) == {"rt_render_beams": 11, "rt_render_beams_device": 12,
                                               "rt_debug_beam_rays": 8, "rt_camera_beams": 8}[name]
    sizes = {"rt_color": 24, "uint32_t": 4, "uint64_t": 8, "rt_camera": C.sizeof(rc.rt_camera)}
    for ctype, bound in zip(params, fn.argtypes):
        if ctype.endswith("*"):
            assert bound is C.c_void_p or issubclass(bound, C._Pointer), (ctype, bound)
            if bound is not C.c_void_p:
                assert C.sizeof(bound._type_) == sizes[ctype.rstrip("*").replace("const", "").strip()], (ctype, bound)
        else:
            assert bound is SCALARS[ctype], (ctype, bound)
    if name != "rt_camera_beams":
        at = 1 if name == "rt_debug_beam_rays" else 2
        assert params[at:at + 5] == ["int64_t", "int32_t", "uint64_t", "uint64_t", "uint64_t"]
    # the same parameter list as the entry point it mirrors
    twin = {"rt_render_beams": "rt_render_rays", "rt_render_beams_device": "rt_render_rays_device",
            "rt_camera_beams": "rt_camera_rays"}.get(name)
    if twin:
        want = [p.replace("rt_ray", "rt_beam") for p in _header_prototype(twin)[1]]
        assert params == want


def test_h4_null_scene_is_refused_without_a_device(rc):
    lib = rc.load_library()
    beams = np.zeros(2, rc.BEAM_DTYPE)
    s, ns, ms = np.full((2, 3), 7.0), np.full(2, 7, np.uint32), np.full(2, 7, np.uint32)
    count = C.c_uint64(5)
    args = (s.ctypes.data_as(C.POINTER(rc.rt_color)), ns.ctypes.data_as(C.POINTER(C.c_uint32)),
            ms.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(count))
    pb = beams.ctypes.data_as(C.c_void_p)
    for n, spp in ((2, 1), (-1, 1), (2, 0), (0, 1)):
        assert lib.rt_render_beams(None, pb, n, spp, 1, 0, 0, *args) == -1, (n, spp)
        assert "rt_render_beams" in _last_error(lib) and "null scene" in _last_error(lib)
    assert lib.rt_render_beams_device(None, pb, 2, 1, 1, 0, 0, None, None, None, None, None) == -1
    assert "rt_render_beams_device" in _last_error(lib)
    assert (s == 7.0).all() and (ns == 7).all() and (ms == 7).all() and count.value == 5
    # the twin's own argument errors
    rays = np.zeros(2, rc.RAY_DTYPE)
    pr = rays.ctypes.data_as(C.c_void_p)
    assert lib.rt_debug_beam_rays(pb, -1, 1, 0, 0, 0, pr, None) == -1
    assert lib.rt_debug_beam_rays(pb, 2, 0, 0, 0, 0, pr, None) == -1
    assert lib.rt_debug_beam_rays(None, 2, 1, 0, 0, 0, pr, None) == -1
    assert lib.rt_debug_beam_rays(pb, 2, 1, 0, 0, 0, None, None) == -1
    assert "rt_debug_beam_rays" in _last_error(lib)
    assert lib.rt_debug_beam_rays(None, 0, 1, 0, 0, 0, None, None) == 0
    assert lib.rt_debug_beam_rays(pb, 2, 1, 0, 0, 0, pr, None) == 0  # uv_out may be NULL


def test_h4_render_beams_rejects_mismatched_shapes(rc):
    """The wrapper's checks come before the library is called (no scene behind `self` here)."""
    a = [np.zeros((4, 3)) for _ in range(6)]
    a[1] = np.tile([0.0, 0.0, 1.0], (4, 1))
    call = rc.GpuRaytracer.render_beams
    for k in range(1, 6):
        bad = list(a)
        bad[k] = bad[k][:3]
        with pytest.raises(ValueError):
            call(None, *bad, 1, 0)
        bad[k] = None
        with pytest.raises(ValueError):
            call(None, *bad, 1, 0)
    with pytest.raises(ValueError):
        call(None, a[0][:, :2], *a[1:], 1, 0)
    with pytest.raises(ValueError):
        call(None, *[x.reshape(2, 2, 3) for x in a], 1, 0)
    with pytest.raises(ValueError):
        rc.beam_rays_host(a[0], a[1][:2], *a[2:], 1, 0)
    good = (np.zeros((4, 3)), np.zeros(4, np.uint32), np.zeros(4, np.uint32))
    for k, bad in ((0, np.zeros((3, 4))), (0, np.zeros((4, 3), np.float32)), (1, np.zeros(5, np.uint32)),
                   (2, np.zeros(4, np.int32)), (0, np.zeros((4, 6))[:, ::2])):
        out = list(good)
        out[k] = bad
        with pytest.raises(ValueError):
            call(None, *a, 1, 0, out=tuple(out))
    # the six arrays land in the record's rows; (n, 4) arrays keep their w
    packed = rc._pack_beams(*[np.full((2, 3), float(k)) for k in range(6)])
    assert packed.dtype == rc.BEAM_DTYPE and packed.shape == (2,)
    for k, f in enumerate(FIELDS):
        assert (packed[f][:, :3] == k).all() and (packed[f][:, 3] == (1.0 if k == 0 else 0.0)).all()
    assert rc._pack_beams(packed, None, None, None, None, None).tobytes() == packed.tobytes()


def test_h4_layout_as_a_c_compiler_sees_it(tmp_path):
    exe = str(tmp_path / "beam_layout")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "host", "beam_layout.c"), "-o", exe], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    assert out.strip() == "192 0 32 64 96 128 160"


def test_h4_panorama_beams_tile(rc):
    """tools/render_panorama.py's beams: beam (i, j) at (1, 0) is beam (i + 1, j) at (0, 0) and at (0, 1)
    beam (i, j + 1) at (0, 0), exactly; the last column closes on the first; the direction at the
    pixel's centre is panorama_rays' to first order."""
    spec = importlib.util.spec_from_file_location("render_panorama", os.path.join(ROOT, "tools", "render_panorama.py"))
    pano = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(pano)
    W, H = 64, 32
    eye, fwd = (1.0, 2.0, 3.0), np.array([0.3, 2.0, -5.0])
    o, d, du, dv = (a.reshape(H, W, 3) for a in pano.panorama_beams(eye, fwd, W))
    assert (o == eye).all()
    assert np.array_equal(d[:, :-1] + 1.0 * du[:, :-1], d[:, 1:])
    assert np.array_equal(d[:, -1] + 1.0 * du[:, -1], d[:, 0])
    assert np.array_equal(d[:-1] + 1.0 * dv[:-1], d[1:])
    assert np.abs(np.linalg.norm(d, axis=2) - 1.0).max() < 2e-9  # (snapped to 2^-30, not renormalised)
    centre = d + 0.5 * du + 0.5 * dv
    centre /= np.linalg.norm(centre, axis=2, keepdims=True)
    rays = pano.panorama_rays(eye, fwd, W)[1].reshape(H, W, 3)
    # bilinear against spherical interpolation across one pixel: second order in the pixel's angle
    assert np.abs(centre - rays).max() < 0.5 * (2 * np.pi / W) ** 2
    assert (d[0, :, 2] == 1.0).all() and not du[0].any()  # the pole: a row of corners is one point


# ---------------------------------------------------------------- H5: memory
def test_h5_host_check_under_sanitizers(rc):
    """tests/host/beam_host_check.cpp, a stand-alone program built with AddressSanitizer and UBSan over
    the library's host code (the Makefile's HOST_SAN pattern), run on the CPU: the twin and
    rt_camera_beams on exact-size heap arrays."""
    subprocess.run(["make", "-s", "-C", CSRC, "-j" + str(min(16, os.cpu_count() or 8)), "beam_host_check_asan"], check=True)
    out = subprocess.run([os.path.join(CSRC, "_obj_asan", "beam_host_check")], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "beam_host_check: ok" in out.stdout
