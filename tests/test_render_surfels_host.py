"""rt_render_surfels, host side (no GPU): the record's layout, the direction formula restated in fp64
numpy and held to analysis (its moments, unit length, d . n = z), the binding and its argument errors,
and prim_surfels.  tests/test_render_surfels_gpu.py holds the device's rays to the restatement here."""
import ctypes as C
import functools
import math
import os
import subprocess

import numpy as np
import pytest

from oracle.oracle import rng_draws
from test_render_rays_host import SCALARS, _header_prototype, _last_error

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("rt_render_surfels", "rt_render_surfels_device", "rt_debug_surfel_rays_device")
DIFFUSE, COSINE, SPHERE = 0, 1, 2
MODES = (DIFFUSE, COSINE, SPHERE)


# ---------------------------------------------------------------- the restatement
def draws(seed, streams, samples):
    """U1, U2 [len(streams), len(samples)]: the first two draws of rt_rng_init(seed, stream, sample)."""
    u = np.array([[rng_draws(seed, int(i), int(k), 2) for k in samples] for i in streams])
    return u[..., 0], u[..., 1]


def cosine_of(mode, u1):
    if mode == DIFFUSE:
        return 2.0 * np.arccos(u1) / math.pi
    if mode == COSINE:
        return np.sqrt(1.0 - u1)
    assert mode == SPHERE
    return 1.0 - 2.0 * u1


def directions(normals, mode, u1, u2):
    """include/rtcore.h, "Sample k of surfel i", in fp64: normals [n, 3] (not unit), u1 and u2 [n, spp] ->
    d [n, spp, 3] and z [n, spp].  In exact arithmetic d is unit, so the Newton step of the normalisation
    is the identity and is left out."""
    nh = normals / np.sqrt((normals[:, 0] * normals[:, 0] + normals[:, 1] * normals[:, 1]) + normals[:, 2] * normals[:, 2])[:, None]
    c = np.stack([nh[:, 1], -nh[:, 0], np.zeros(len(nh))], axis=1)
    cl = np.sqrt(c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1])
    flat = cl == 0.0
    c = np.where(flat[:, None], np.array([1.0, 0.0, 0.0]), c / np.where(flat, 1.0, cl)[:, None])
    bn = np.cross(nh, c)
    z = cosine_of(mode, u1)
    s = np.sqrt(np.maximum(0.0, 1.0 - z * z))
    turn = 2.0 * math.pi * u2
    d = nh[:, None, :] * z[..., None] + s[..., None] * (c[:, None, :] * np.cos(turn)[..., None] + bn[:, None, :] * np.sin(turn)[..., None])
    return d, z


# ---------------------------------------------------------------- H1: layout
def test_h1_layout_as_a_c_compiler_sees_it(rc, tmp_path):
    exe = str(tmp_path / "surfel_layout")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "host", "surfel_layout.c"), "-o", exe], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    assert out.strip() == "64 0 32 0 1 2"
    assert C.sizeof(rc.rt_surfel) == 64 == rc.SURFEL_DTYPE.itemsize == C.sizeof(rc.rt_ray)
    assert rc.rt_surfel.normal.offset == 32 == rc.SURFEL_DTYPE.fields["normal"][1]
    assert (rc.RT_GATHER_DIFFUSE, rc.RT_GATHER_COSINE, rc.RT_GATHER_SPHERE) == MODES


# ---------------------------------------------------------------- H2: the moments
@functools.lru_cache(maxsize=None)
def _h2_draws():
    return draws(1, range(1000, 1016), range(4096))


MOMENTS = {DIFFUSE: (2.0 / math.pi, 4.0 * (math.pi - 2.0) / math.pi ** 2), COSINE: (2.0 / 3.0, 0.5), SPHERE: (0.0, 1.0 / 3.0)}


@pytest.mark.parametrize("mode", MODES)
def test_h2_moments_of_the_restatement(mode):
    """Seed 1, streams 1000 .. 1015, samples 0 .. 4095 (65,536 directions), normal (0, 0, 1): E[z], E[z^2]
    and the means of cos 2 pi U2, sin 2 pi U2 and z cos 2 pi U2 within 0.014 of analysis: five standard
    errors of the widest of them (sd 1 / sqrt 2 over sqrt 65536)."""
    u1, u2 = _h2_draws()
    assert u1.size == 65536
    normals = np.tile([0.0, 0.0, 1.0], (u1.shape[0], 1))
    d, z = directions(normals, mode, u1, u2)
    assert np.abs(d[..., 2] - z).max() <= 1e-15
    cs, sn = np.cos(2.0 * math.pi * u2), np.sin(2.0 * math.pi * u2)
    ez, ez2 = MOMENTS[mode]
    got = {"E[z]": z.mean() - ez, "E[z^2]": (z * z).mean() - ez2, "E[cos]": cs.mean(), "E[sin]": sn.mean(),
           "E[z cos]": (z * cs).mean()}
    print(f"H2 mode {mode}: " + ", ".join(f"{k} off by {v:+.4f}" for k, v in got.items()))
    for k, v in got.items():
        assert abs(v) <= 0.014, (k, v)
    # with the normal +z the frame is c = (1, 0, 0), n x c = (0, 1, 0): d = (s cos, s sin, z)
    s = np.sqrt(np.maximum(0.0, 1.0 - z * z))
    assert np.abs(d[..., 0] - s * cs).max() <= 1e-15 and np.abs(d[..., 1] - s * sn).max() <= 1e-15


# ---------------------------------------------------------------- H3: unit, and d . n = z
def h3_normals():
    rng = np.random.default_rng(17)
    g = rng.normal(size=(60, 3))
    g /= np.linalg.norm(g, axis=1, keepdims=True)
    scaled = g[:30] * rng.uniform(0.5, 2.0, (30, 1))
    poles = np.array([[0.0, 0.0, 1.0], [0.0, 0.0, -1.0], [0.0, 0.0, 0.5], [0.0, 0.0, -2.0]])
    return np.concatenate([g[30:], scaled, poles])


@pytest.mark.parametrize("mode", MODES)
def test_h3_directions_are_unit_and_keep_their_cosine(mode):
    """General, non-unit (length 0.5 .. 2) and exactly +-z normals (the c = (1, 0, 0) branch)."""
    normals = h3_normals()
    u1, u2 = draws(3, range(len(normals)), range(64))
    d, z = directions(normals, mode, u1, u2)
    nh = normals / np.linalg.norm(normals, axis=1, keepdims=True)
    length = np.sqrt((d * d).sum(axis=2))
    cosine = (d * nh[:, None, :]).sum(axis=2)
    print(f"H3 mode {mode}: max | |d| - 1 | = {np.abs(length - 1.0).max():.2e}, max |d . n - z| = {np.abs(cosine - z).max():.2e}")
    assert np.abs(length - 1.0).max() <= 1e-15
    assert np.abs(cosine - z).max() <= 1e-15
    assert (np.abs(d[-4:, :, 2]) == np.abs(z[-4:])).all()  # the pole's own branch: d.z = +-z exactly


# ---------------------------------------------------------------- H4: the binding
def test_h4_exported_and_bound(rc):
    lib = rc.load_library()
    out = subprocess.run(["nm", "-D", "--defined-only", rc.LIB_PATH], capture_output=True, text=True).stdout
    for name in NAMES:
        assert f" T {name}\n" in out
        assert getattr(lib, name).argtypes is not None
    for name in ("render_surfels", "render_surfels_device", "surfel_rays"):
        assert hasattr(rc.GpuRaytracer, name)
    assert callable(rc.gather_mean) and callable(rc.prim_surfels)
    assert rc.ABI_VERSION == 6 == lib.rt_abi_version()  # additive: detected by symbol


@pytest.mark.parametrize("name", NAMES)
def test_h4_ctypes_prototype_matches_the_header(rc, name):
    fn = getattr(rc.load_library(), name)
    ret, params = _header_prototype(name)
    assert ret == "int" and fn.restype is C.c_int
    assert len(params) == len(fn.argtypes) == {"rt_render_surfels": 12, "rt_render_surfels_device": 13,
                                               "rt_debug_surfel_rays_device": 9}[name]
    sizes = {"rt_color": 24, "uint32_t": 4, "uint64_t": 8}
    for ctype, bound in zip(params, fn.argtypes):
        if ctype.endswith("*"):
            assert bound is C.c_void_p or issubclass(bound, C._Pointer), (ctype, bound)
            if bound is not C.c_void_p:
                assert C.sizeof(bound._type_) == sizes[ctype.rstrip("*").replace("const", "").strip()], (ctype, bound)
        else:
            assert bound is SCALARS[ctype], (ctype, bound)
    # the rays' parameter list with the mode before the list
    if name == "rt_debug_surfel_rays_device":
        assert params == ["int32_t", "const rt_surfel*", "int64_t", "int32_t", "uint64_t", "uint64_t", "uint64_t", "rt_ray*", "void*"]
    else:
        want = [p.replace("rt_ray", "rt_surfel") for p in _header_prototype(name.replace("surfels", "rays"))[1]]
        assert params == want[:1] + ["int32_t"] + want[1:]


def test_h4_argument_errors_without_a_device(rc):
    """RT_ERR_ARG before anything is launched, the buffers untouched: a null scene, n < 0, spp <= 0, and an
    unknown mode, which is checked first; the debug entry's own.  No device is touched."""
    lib = rc.load_library()
    surfels = np.zeros(2, rc.SURFEL_DTYPE)
    s, ns, ms = np.full((2, 3), 7.0), np.full(2, 7, np.uint32), np.full(2, 7, np.uint32)
    count = C.c_uint64(5)
    args = (s.ctypes.data_as(C.POINTER(rc.rt_color)), ns.ctypes.data_as(C.POINTER(C.c_uint32)),
            ms.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(count))
    ps = surfels.ctypes.data_as(C.c_void_p)
    for mode in MODES:
        for n, spp in ((2, 1), (-1, 1), (2, 0), (0, 1)):
            assert lib.rt_render_surfels(None, mode, ps, n, spp, 1, 0, 0, *args) == -1, (mode, n, spp)
            assert "rt_render_surfels" in _last_error(lib) and "null scene" in _last_error(lib)
        assert lib.rt_render_surfels_device(None, mode, ps, 2, 1, 1, 0, 0, None, None, None, None, None) == -1
        assert "rt_render_surfels_device" in _last_error(lib)
    for mode in (-1, 3, 1 << 20):
        assert lib.rt_render_surfels(None, mode, ps, 2, 1, 1, 0, 0, *args) == -1
        assert "rt_render_surfels" in _last_error(lib) and "gather mode" in _last_error(lib)
        assert lib.rt_render_surfels_device(None, mode, ps, 0, 1, 1, 0, 0, None, None, None, None, None) == -1
        assert "rt_render_surfels_device" in _last_error(lib) and "gather mode" in _last_error(lib)
        assert lib.rt_debug_surfel_rays_device(mode, None, 0, 1, 0, 0, 0, None, None) == -1
        assert "rt_debug_surfel_rays_device" in _last_error(lib) and "gather mode" in _last_error(lib)
    assert (s == 7.0).all() and (ns == 7).all() and (ms == 7).all() and count.value == 5
    # the debug entry (device pointers: none is read before the checks are through)
    p = C.c_void_p(64)
    assert lib.rt_debug_surfel_rays_device(0, p, -1, 1, 0, 0, 0, p, None) == -1
    assert lib.rt_debug_surfel_rays_device(0, p, 2, 0, 0, 0, 0, p, None) == -1
    assert lib.rt_debug_surfel_rays_device(0, None, 2, 1, 0, 0, 0, p, None) == -1
    assert lib.rt_debug_surfel_rays_device(0, p, 2, 1, 0, 0, 0, None, None) == -1
    assert lib.rt_debug_surfel_rays_device(0, p, 2 ** 57, 2, 0, 0, 0, p, None) == -1
    assert "rt_debug_surfel_rays_device" in _last_error(lib)
    assert lib.rt_debug_surfel_rays_device(2, None, 0, 1, 0, 0, 0, None, None) == 0


def test_h4_wrappers_reject_mismatched_shapes(rc):
    """The wrappers' checks come before the library is called (no scene behind `self` here)."""
    call = rc.GpuRaytracer.render_surfels
    p, n = np.zeros((4, 3)), np.tile([0.0, 0.0, 1.0], (4, 1))
    for bad in ((p[:3], n), (p, n[:, :2]), (p.reshape(2, 2, 3), n.reshape(2, 2, 3)), (np.zeros((4, 4)), n)):
        with pytest.raises(ValueError):
            call(None, *bad, 1, 0)
    good = (np.zeros((4, 3)), np.zeros(4, np.uint32), np.zeros(4, np.uint32))
    for k, bad in ((0, np.zeros((3, 4))), (0, np.zeros((4, 3), np.float32)), (1, np.zeros(5, np.uint32)), (2, np.zeros(4, np.int32))):
        out = list(good)
        out[k] = bad
        with pytest.raises(ValueError):
            call(None, p, n, 1, 0, out=tuple(out))
    packed = rc._pack_surfels(np.full((2, 3), 1.0), np.full((2, 3), 2.0))
    assert packed.dtype == rc.SURFEL_DTYPE and packed.shape == (2,)
    assert (packed["position"] == [1.0, 1.0, 1.0, 1.0]).all() and (packed["normal"] == [2.0, 2.0, 2.0, 0.0]).all()
    assert rc._pack_surfels(packed, None).tobytes() == packed.tobytes()
    # gather_mean: (sum + misses * ambient) / (samples + misses)
    mean = rc.gather_mean(np.array([[3.0, 6.0, 9.0], [0.0, 0.0, 0.0]]), np.array([3, 0], np.uint32), np.array([1, 4], np.uint32),
                          (0.2, 0.4, 0.8))
    assert np.allclose(mean, [[0.8, 1.6, 2.45], [0.2, 0.4, 0.8]], rtol=1e-15, atol=0)
    assert np.array_equal(rc.gather_mean(np.ones((1, 3)), [1], [1], rc.rt_color(1.0, 2.0, 3.0)), [[1.0, 1.5, 2.0]])


# ---------------------------------------------------------------- H5: prim_surfels
def test_h5_prim_surfels_of_a_triangle_of_bounce(rc):
    scene = rc.SceneLoader.from_file(rc.scene_path("bounce.txt"))
    prims = list(scene.prims)
    tri = next(p for p in prims if p.kind == rc.RT_PRIM_TRIANGLE)
    v0, e01, e02 = (np.array([v.x, v.y, v.z]) for v in tri.p)
    W, H, offset = 5, 3, 1e-3
    pos, nrm = rc.prim_surfels(tri, W, H, offset)
    assert pos.shape == nrm.shape == (W, H, 3)
    n = nrm[0, 0]
    assert (nrm == n).all()
    scale = max(np.linalg.norm(e01), np.linalg.norm(e02))
    assert abs(n @ n - 1.0) <= 4e-16 and abs(n @ e01) <= 1e-15 * scale and abs(n @ e02) <= 1e-15 * scale
    assert n @ np.cross(e01, e02) > 0.0
    # on the plane and inside the parallelogram: the coordinates (a, b) in the basis (e01, e02)
    on = pos - offset * n - v0
    assert np.abs(on @ n).max() <= 1e-14 * max(1.0, scale)
    ab = np.linalg.lstsq(np.stack([e01, e02], axis=1), on.reshape(-1, 3).T, rcond=None)[0].T.reshape(W, H, 2)
    assert np.abs(ab[..., 0] - ((np.arange(W) + 0.5) / W)[:, None]).max() <= 1e-12
    assert np.abs(ab[..., 1] - ((np.arange(H) + 0.5) / H)[None, :]).max() <= 1e-12
    assert (ab > 0.0).all() and (ab < 1.0).all()
    pos_f, nrm_f = rc.prim_surfels(tri, W, H, offset, flip=True)
    assert np.array_equal(nrm_f, -nrm) and np.allclose(pos_f, pos - 2 * offset * n, rtol=0, atol=1e-15 * max(1.0, np.abs(pos).max()))
    sphere = next(p for p in prims if p.kind == rc.RT_PRIM_SPHERE)
    with pytest.raises(ValueError):
        rc.prim_surfels(sphere, W, H, offset)
    with pytest.raises(ValueError):
        rc.prim_surfels(tri, 0, H, offset)
