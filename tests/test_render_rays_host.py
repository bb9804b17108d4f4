"""rt_render_rays / rt_render_rays_device, host side (no GPU): the symbols, their ctypes prototypes
against the header's, render_rays' argument checks and what the library refuses without a device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("rt_render_rays", "rt_render_rays_device")
SCALARS = {"int32_t": C.c_int32, "int64_t": C.c_int64, "uint64_t": C.c_uint64, "int": C.c_int}


def _header_prototype(name):
    """(return type, [parameter types]) of `name` as include/rtcore.h declares it, each type a string
    without the parameter's name."""
    text = open(os.path.join(ROOT, "include", "rtcore.h")).read()
    m = re.search(r"^(\w+)\s+" + name + r"\(([^;]*?)\);", text, re.M | re.S)
    assert m, name
    params = [" ".join(p.split()) for p in m.group(2).split(",")]
    return m.group(1), [re.sub(r"\s*\w+$", "", p) for p in params]


def test_exported_and_bound(rc):
    lib = rc.load_library()
    out = subprocess.run(["nm", "-D", "--defined-only", rc.LIB_PATH], capture_output=True, text=True).stdout
    for name in NAMES:
        assert f" T {name}\n" in out
        assert getattr(lib, name).argtypes is not None
    for name in ("render_rays", "render_rays_device"):
        assert hasattr(rc.GpuRaytracer, name)
    assert rc.ABI_VERSION == 6 == lib.rt_abi_version()  # additive: detected by symbol


@pytest.mark.parametrize("name", NAMES)
def test_ctypes_prototype_matches_the_header(rc, name):
    """Every parameter of the header's prototype against the bound argtypes: the scalar widths exactly,
    a pointer for a pointer (c_void_p, or POINTER of the 4- / 8- / 24-byte element the header names)."""
    fn = getattr(rc.load_library(), name)
    ret, params = _header_prototype(name)
    assert ret == "int" and fn.restype is C.c_int
    assert len(params) == len(fn.argtypes) == (11 if name == "rt_render_rays" else 12)
    sizes = {"rt_color": 24, "uint32_t": 4, "uint64_t": 8}
    for ctype, bound in zip(params, fn.argtypes):
        if ctype.endswith("*"):
            assert bound is C.c_void_p or issubclass(bound, C._Pointer), (ctype, bound)
            if bound is not C.c_void_p:
                assert C.sizeof(bound._type_) == sizes[ctype.rstrip("*").replace("const", "").strip()], (ctype, bound)
        else:
            assert bound is SCALARS[ctype], (ctype, bound)
    # n is 64-bit, spp 32-bit, then seed, sample_base, stream_base
    assert params[2:7] == ["int64_t", "int32_t", "uint64_t", "uint64_t", "uint64_t"]


def _last_error(lib):
    buf = C.create_string_buffer(512)
    lib.rt_last_error(buf, 512)
    return buf.value.decode()


def test_null_scene_is_refused_without_a_device(rc):
    """RT_ERR_ARG for a null scene (and n < 0, spp <= 0 with it) before anything is launched; the
    buffers are untouched.  No device is touched: this runs on a machine without one."""
    lib = rc.load_library()
    rays = np.zeros(2, rc.RAY_DTYPE)
    s, ns, ms = np.full((2, 3), 7.0), np.full(2, 7, np.uint32), np.full(2, 7, np.uint32)
    count = C.c_uint64(5)
    args = (s.ctypes.data_as(C.POINTER(rc.rt_color)), ns.ctypes.data_as(C.POINTER(C.c_uint32)),
            ms.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(count))
    pr = rays.ctypes.data_as(C.c_void_p)
    for n, spp in ((2, 1), (-1, 1), (2, 0), (0, 1)):
        assert lib.rt_render_rays(None, pr, n, spp, 1, 0, 0, *args) == -1, (n, spp)
        assert "rt_render_rays" in _last_error(lib) and "null scene" in _last_error(lib)
    assert lib.rt_render_rays_device(None, pr, 2, 1, 1, 0, 0, None, None, None, None, None) == -1
    assert "rt_render_rays_device" in _last_error(lib)
    assert (s == 7.0).all() and (ns == 7).all() and (ms == 7).all() and count.value == 5


def test_render_rays_rejects_mismatched_shapes(rc):
    """The wrapper's checks come before the library is called (no scene behind `self` here)."""
    o, d = np.zeros((4, 3)), np.tile([0.0, 0.0, 1.0], (4, 1))
    call = rc.GpuRaytracer.render_rays
    with pytest.raises(ValueError):
        call(None, o, d[:3], 1, 0)
    with pytest.raises(ValueError):
        call(None, o[:, :2], d, 1, 0)
    with pytest.raises(ValueError):
        call(None, o.reshape(2, 2, 3), d.reshape(2, 2, 3), 1, 0)
    good = (np.zeros((4, 3)), np.zeros(4, np.uint32), np.zeros(4, np.uint32))
    for k, bad in ((0, np.zeros((3, 4))), (0, np.zeros((4, 3), np.float32)), (1, np.zeros(5, np.uint32)),
                   (2, np.zeros(4, np.int32)), (0, np.zeros((4, 6))[:, ::2])):
        out = list(good)
        out[k] = bad
        with pytest.raises(ValueError):
            call(None, o, d, 1, 0, out=tuple(out))


def test_normalize_is_fp64_and_leaves_the_input_alone(rc):
    """normalize=True divides by the fp64 norm on the host, on a copy: seen by a stand-in for the
    library that records the rays the wrapper hands it (no scene, no device)."""
    class Probe:
        handle = None

        class lib:
            @staticmethod
            def rt_render_rays(handle, rays, n, *rest):
                Probe.seen = np.ctypeslib.as_array(C.cast(rays, C.POINTER(C.c_double)), (n, 8)).copy()
                return 0

    d = np.array([[3.0, 0.0, 4.0], [1e-3, 2e-3, 2e-3]])
    rays = rc._pack_rays(np.zeros((2, 3)), d)
    s, ns, ms, count = rc.GpuRaytracer.render_rays(Probe, rays, None, 1, 0, normalize=True)
    assert np.array_equal(Probe.seen[:, 4:7], d / np.sqrt((d * d).sum(axis=1))[:, None])
    assert np.array_equal(rays["direction"][:, :3], d)  # the caller's array is not written
    assert s.shape == (2, 3) and ns.shape == ms.shape == (2,) and count == 0
    rc.GpuRaytracer.render_rays(Probe, np.zeros((2, 3)), d, 1, 0)
    assert np.array_equal(Probe.seen[:, 4:7], d)  # taken as given without it


def test_panorama_rays_and_ppm(tmp_path):
    """tools/render_panorama.py's host parts: unit directions covering the sphere row by row, the
    centre column along the line of sight, the poles at the first and last row; the PPM's bytes."""
    import importlib.util

    spec = importlib.util.spec_from_file_location("render_panorama", os.path.join(ROOT, "tools", "render_panorama.py"))
    pano = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(pano)
    o, d = pano.panorama_rays((1.0, 2.0, 3.0), np.array([0.0, 2.0, -5.0]), 64)
    assert o.shape == d.shape == (64 * 32, 3) and (o == (1.0, 2.0, 3.0)).all()
    assert np.abs(np.linalg.norm(d, axis=1) - 1.0).max() < 1e-15
    d = d.reshape(32, 64, 3)
    mid = 0.5 * (d[15, 31] + d[16, 32])  # the image centre: forward, flattened to the horizon
    assert np.allclose(mid / np.linalg.norm(mid), (0.0, 1.0, 0.0), atol=1e-12)
    assert d[0, :, 2].min() > 0.99 and d[-1, :, 2].max() < -0.99
    assert np.abs(d.reshape(-1, 3).mean(axis=0)).max() < 0.05  # all around
    argb = np.array([[0x7F010203, -1], [0, 0x00FF8000]], np.int64).astype(np.int32)
    pano.write_ppm(str(tmp_path / "p.ppm"), argb)
    assert open(tmp_path / "p.ppm", "rb").read() == b"P6\n2 2\n255\n" + bytes([1, 2, 3, 255, 255, 255, 0, 0, 0, 255, 128, 0])
