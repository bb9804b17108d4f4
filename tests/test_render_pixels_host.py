"""rt_render_pixels / rt_render_pixels_device, host side (no GPU): the symbols, their ctypes prototypes
against the header's, what the library refuses without a device, and the plan of a list launch."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("rt_render_pixels", "rt_render_pixels_device")
SCALARS = {"int32_t": C.c_int32, "int64_t": C.c_int64, "uint64_t": C.c_uint64, "uint32_t": C.c_uint32, "int": C.c_int}
SIZES = {"rt_color": 24, "uint32_t": 4, "uint64_t": 8, "double": 8, "unsigned long long": 8, "rt_adaptive_params": 32}


def header_prototype(name):
    """(return type, [parameter types]) of `name` as include/rtcore.h declares it, each type a string
    without the parameter's name."""
    text = open(os.path.join(ROOT, "include", "rtcore.h")).read()
    m = re.search(r"^(\w+)\s+" + name + r"\(([^;]*?)\);", text, re.M | re.S)
    assert m, name
    params = [" ".join(p.split()) for p in m.group(2).split(",")]
    return m.group(1), [re.sub(r"\s*\w+$", "", p) for p in params]


def check_prototype(fn, name, n_params, ret_type=("int", C.c_int)):
    """Every parameter of the header's prototype against the bound argtypes: the scalar widths exactly, a
    pointer for a pointer (c_void_p, or POINTER of an element of the size the header names)."""
    ret, params = header_prototype(name)
    assert ret == ret_type[0] and fn.restype is ret_type[1]
    assert len(params) == len(fn.argtypes) == n_params
    for ctype, bound in zip(params, fn.argtypes):
        if ctype.endswith("*"):
            assert bound is C.c_void_p or issubclass(bound, C._Pointer), (ctype, bound)
            if bound is not C.c_void_p:
                assert C.sizeof(bound._type_) == SIZES[ctype.rstrip("*").replace("const", "").strip()], (ctype, bound)
        else:
            assert bound is SCALARS[ctype], (ctype, bound)
    return params


def test_exported_and_bound(rc):
    lib = rc.load_library()
    out = subprocess.run(["nm", "-D", "--defined-only", rc.LIB_PATH], capture_output=True, text=True).stdout
    for name in NAMES + ("rt_debug_pixels_plan",):
        assert f" T {name}\n" in out
        assert getattr(lib, name).argtypes is not None
    for name in ("render_pixels", "render_pixels_device", "render_adaptive"):
        assert hasattr(rc.GpuRaytracer, name)
    assert rc.ABI_VERSION == 6 == lib.rt_abi_version()  # additive: detected by symbol


@pytest.mark.parametrize("name", NAMES)
def test_ctypes_prototype_matches_the_header(rc, name):
    params = check_prototype(getattr(rc.load_library(), name), name, 12 if name == "rt_render_pixels" else 14)
    # n is 64-bit, spp 32-bit, then seed and sample_base
    assert params[2:6] == ["int64_t", "int32_t", "uint64_t", "uint64_t"]
    if name == "rt_render_pixels_device":
        assert params[11] == "uint64_t"  # plane


def _last_error(lib):
    buf = C.create_string_buffer(512)
    lib.rt_last_error(buf, 512)
    return buf.value.decode()


def test_null_scene_is_refused_without_a_device(rc):
    """RT_ERR_ARG for a null scene (whatever n and spp are) before anything is launched; the buffers are
    untouched.  No device is touched: this runs on a machine without one."""
    lib = rc.load_library()
    px = np.arange(2, dtype=np.uint32)
    s, ns, ms = np.full((2, 2, 3), 7.0), np.full((2, 2), 7, np.uint32), np.full((2, 2), 7, np.uint32)
    count = C.c_uint64(5)
    args = (s.ctypes.data_as(C.POINTER(rc.rt_color)), ns.ctypes.data_as(C.POINTER(C.c_uint32)),
            ms.ctypes.data_as(C.POINTER(C.c_uint32)), None, None, C.byref(count))
    pp = px.ctypes.data_as(C.c_void_p)
    for n, spp in ((2, 1), (-1, 1), (2, 0), (0, 1)):
        assert lib.rt_render_pixels(None, pp, n, spp, 1, 0, *args) == -1, (n, spp)
        assert "rt_render_pixels" in _last_error(lib) and "null scene" in _last_error(lib)
    assert lib.rt_render_pixels_device(None, pp, 2, 1, 1, 0, None, None, None, None, None, 0, None, None) == -1
    assert "rt_render_pixels_device" in _last_error(lib)
    assert (s == 7.0).all() and (ns == 7).all() and (ms == 7).all() and count.value == 5


def test_render_pixels_checks_its_arrays_first(rc):
    """The wrapper's checks come before the library is called (a stand-in without a scene behind it)."""
    class Probe:
        handle = None
        width, height = 4, 3
        _pixel_list = staticmethod(lambda pixels: rc.GpuRaytracer._pixel_list(Probe, pixels))

        class lib:
            @staticmethod
            def rt_render_pixels(handle, pixels, n, *rest):
                Probe.seen = np.ctypeslib.as_array(C.cast(pixels, C.POINTER(C.c_uint32)), (n,)).copy()
                Probe.moments = rest[6] is not None and rest[7] is not None
                return 0

    call = rc.GpuRaytracer.render_pixels
    out = call(Probe, np.array([[1, 2], [3, 0]]), 1)  # (x, y) pairs -> y * width + x
    assert Probe.seen.tolist() == [9, 3] and not Probe.moments
    assert [a.shape for a in out[:3]] == [(4, 3, 3), (4, 3), (4, 3)] and out[3] == 0 and len(out) == 4
    out = call(Probe, [5, 0, 11], 2, moments=True)
    assert Probe.seen.tolist() == [5, 0, 11] and Probe.moments and len(out) == 6
    assert out[4].shape == out[5].shape == (4, 3) and out[4].dtype == np.float64 and out[5].dtype == np.uint32
    with pytest.raises(ValueError):
        call(Probe, [-1], 1)
    with pytest.raises(ValueError):
        call(Probe, [0], 1, out=(np.zeros((3, 4, 3)), np.zeros((4, 3), np.uint32), np.zeros((4, 3), np.uint32)))
    with pytest.raises(ValueError):  # moments want five arrays
        call(Probe, [0], 1, moments=True, out=(np.zeros((4, 3, 3)), np.zeros((4, 3), np.uint32), np.zeros((4, 3), np.uint32)))


@pytest.mark.parametrize("kernel,B", [(0, 24), (1, 24), (3, 64)])
def test_samples_per_item_are_a_function_of_spp_alone(rc, kernel, B):
    """make_params_pixels: s = min(64, ceil(spp / B)) samples per work item whatever the list's length
    is, ceil(spp / s) items per entry in a power-of-two number of chunk slots, blocks of 64 entries."""
    for spp in (1, 24, 25, 64, 100, 1024):
        s = min(64, -(-spp // B))
        for n in (1, 37, 4096, 1 << 19):
            plan = rc.pixels_plan(kernel, n, spp)
            assert plan["samples_per_item"] == s, (spp, n, plan)
            assert plan["used_chunks"] == -(-spp // s)
            assert plan["n_chunks"] >= plan["used_chunks"] > plan["n_chunks"] // 2 or plan["n_chunks"] == 1
            assert plan["n_chunks"] & (plan["n_chunks"] - 1) == 0
            assert plan["blocks"] == -(-n // 64)
    assert rc.pixels_plan(0, 64, 100)["samples_per_item"] == 5 and rc.pixels_plan(3, 64, 100)["samples_per_item"] == 2
    lib = rc.load_library()
    info = (C.c_int32 * 4)()
    for bad in ((2, 64, 1), (0, 0, 1), (0, 64, 0), (4, 64, 1)):
        assert lib.rt_debug_pixels_plan(*bad, info) == -1


def test_the_kernel_source_still_compiles_under_hiprtc(rc):
    """kernels_path.hip is also the run-time compiler's source: the item-source switch and the list
    fields must build there (a scene-specialised build of either brute-force order, no device needed)."""
    assert rc.jit_compile_check("gfx950", grouped=False) > 0
    assert rc.jit_compile_check("gfx950", grouped=True) > 0
