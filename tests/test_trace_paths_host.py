"""rt_trace_paths, host side (no GPU): the record's layout in C, ctypes and numpy, the export and
the ABI version, and the arguments refused before anything touches a device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def c_layout(tmp_path_factory):
    """tests/host/debug_ray_layout.c compiled as C against include/rtcore.h, and what it prints."""
    exe = str(tmp_path_factory.mktemp("layout") / "debug_ray_layout")
    subprocess.run(["cc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", exe,
                    os.path.join(ROOT, "tests", "host", "debug_ray_layout.c")], check=True)
    lines = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split("\n")
    return [ln.split() for ln in lines if ln]


def test_debug_ray_layout_agrees(rc, c_layout):
    """sizeof and every offsetof of rt_debug_ray in C equal the ctypes structure's and the numpy
    dtype's; the size is a multiple of 16 (the kernel stores whole float4 rows)."""
    assert c_layout[0][0] == "sizeof"
    size = int(c_layout[0][1])
    fields = [(n, int(o), int(sz)) for n, o, sz in c_layout[1:15]]
    assert size % 16 == 0 and size == 96
    assert C.sizeof(rc.rt_debug_ray) == size == rc.DEBUG_RAY_DTYPE.itemsize
    assert [n for n, _, _ in fields] == [n for n, _ in rc.rt_debug_ray._fields_] == list(rc.DEBUG_RAY_DTYPE.names)
    for name, off, sz in fields:
        cf = getattr(rc.rt_debug_ray, name)
        assert (cf.offset, cf.size) == (off, sz), name
        dt, doff = rc.DEBUG_RAY_DTYPE.fields[name][:2]
        assert (doff, dt.itemsize) == (off, sz), name
    # float fields are fp32, the others int32, in all three
    for name, ctype in rc.rt_debug_ray._fields_:
        base = rc.DEBUG_RAY_DTYPE.fields[name][0].base
        elem = getattr(ctype, "_type_", ctype)
        assert base == (np.float32 if elem in (C.c_float, "f") else np.int32), name


def test_constants_agree(rc, c_layout):
    abi = c_layout[15]
    assert abi[0] == "abi" and int(abi[1]) == rc.ABI_VERSION == 6
    assert int(abi[3]) == rc.RT_TRACE_MAX_RECORDS
    assert [int(v) for v in c_layout[16][1:]] == list(range(10)) == [
        rc.RT_BOUNCE_SKIPPED, rc.RT_BOUNCE_DIFFUSE, rc.RT_BOUNCE_SPECULAR, rc.RT_BOUNCE_SPECULAR_FAIL,
        rc.RT_BOUNCE_TRANSMITTED, rc.RT_BOUNCE_EMISSION, rc.RT_BOUNCE_PURE_BLACK, rc.RT_BOUNCE_RECURSION_COMPLETE,
        rc.RT_BOUNCE_MISSED, rc.RT_BOUNCE_DEBUG]
    assert len(rc.BOUNCE_TYPE_NAMES) == 10


def test_exported_with_abi_6(rc):
    lib = rc.load_library()
    assert lib.rt_abi_version() == 6 == rc.ABI_VERSION
    out = subprocess.run(["nm", "-D", "--defined-only", rc.LIB_PATH], capture_output=True, text=True).stdout
    assert " T rt_trace_paths" in out
    assert hasattr(rc.GpuRaytracer, "trace_paths")


def _last_error(lib):
    buf = C.create_string_buffer(512)
    lib.rt_last_error(buf, 512)
    return buf.value.decode()


def test_arguments_refused_without_a_device(rc):
    """RT_ERR_ARG (-1) before anything is launched: null rays_out, spp <= 0, an empty tile, more
    records than the cap (a path has at least one record, so w*h*spp alone can exceed it), and a
    null scene -- the last as every tile entry point refuses it (check_tile)."""
    lib = rc.load_library()
    rays = (rc.rt_debug_ray * 4)()

    def call(scene, x0, y0, w, h, spp, out):
        return lib.rt_trace_paths(scene, x0, y0, w, h, spp, 0, 0, out, None, None)

    assert call(None, 0, 0, 1, 1, 1, None) == -1 and "rays_out" in _last_error(lib)
    assert call(None, 0, 0, 1, 1, 0, rays) == -1 and "spp" in _last_error(lib)
    assert call(None, 0, 0, 1, 1, -3, rays) == -1 and "spp" in _last_error(lib)
    assert call(None, 0, 0, 0, 1, 1, rays) == -1
    assert call(None, 0, 0, 1024, 1024, 2, rays) == -1 and "RT_TRACE_MAX_RECORDS" in _last_error(lib)
    assert call(None, 0, 0, 1 << 15, 1 << 15, 1 << 15, rays) == -1 and "RT_TRACE_MAX_RECORDS" in _last_error(lib)
    assert call(None, 0, 0, 1, 1, 1, rays) == -1 and "null scene" in _last_error(lib)
    assert bytes(rays) == bytes(C.sizeof(rays))  # nothing was written


def test_inspect_pixel_formats_records(rc):
    """tools/inspect_pixel.py: one line per sample and one per bounce record (no device needed)."""
    import importlib.util

    spec = importlib.util.spec_from_file_location("inspect_pixel", os.path.join(ROOT, "tools", "inspect_pixel.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    rec = np.zeros(4, rc.DEBUG_RAY_DTYPE)
    rec[0] = (7, rc.RT_BOUNCE_TRANSMITTED, 0, 1.5, 0.25, 0.9, 0, 0, (1, 2, 3), (0, 0, 1), (0, 0, 5), (0, 0, -1), (1, 1, 1), 0)
    rec[1] = (-1, rc.RT_BOUNCE_MISSED, 0, 0, np.nan, np.nan, 1, 0, (0, 0, 0), (0, 0, 0), (1, 2, 3), (0, 1, 0), (.5, .5, .5), 0)
    lines = mod.format_sample(rc, 3, rec, 2, np.array([0.1, 0.2, 0.3]))
    assert len(lines) == 3 and lines[0].startswith("sample 3: colour (0.1 0.2 0.3), 2 rays")
    assert "Transmitted" in lines[1] and "prim 7" in lines[1] and "fresnel 0.25" in lines[1]
    assert "Missed" in lines[2] and "no hit" in lines[2]
    assert mod.format_sample(rc, 0, rec[1:], 1, np.array([-1.0, -1.0, -1.0]))[0] == "sample 0: miss, 1 ray"
