"""rt_occluded_surfels, host side (no GPU): the exported symbols and their bindings, the arguments refused
before anything touches a device, the wrappers' shape checks, ambient_occlusion, and the shared surfel
set (tests/occluded_surfels_cases.py) held to the conditions that keep tests/test_occluded_surfels_gpu.py
from hollowing itself out."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from occluded_surfels_cases import INF, N, assert_not_hollow, oracle_distances, surfel_set, valid_surfels
from test_render_rays_host import SCALARS, _header_prototype, _last_error
from test_render_surfels_host import MODES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("rt_occluded_surfels", "rt_occluded_surfels_device")


def test_exported_and_bound(rc):
    lib = rc.load_library()
    out = subprocess.run(["nm", "-D", "--defined-only", rc.LIB_PATH], capture_output=True, text=True).stdout
    for name in NAMES:
        assert f" T {name}\n" in out
        assert getattr(lib, name).argtypes is not None
        assert name in rc._OPTIONAL
    for name in ("occluded_surfels", "occluded_surfels_device"):
        assert callable(getattr(rc.GpuRaytracer, name))
    assert callable(rc.ambient_occlusion)
    assert rc.ABI_VERSION == 6 == lib.rt_abi_version()  # additive: detected by symbol


@pytest.mark.parametrize("name", NAMES)
def test_ctypes_prototype_matches_the_header(rc, name):
    """Every parameter of the header's prototype against the bound argtypes: the scalar widths exactly, a
    pointer for a pointer (c_void_p, or POINTER of the 4-byte element the header names)."""
    fn = getattr(rc.load_library(), name)
    ret, params = _header_prototype(name)
    assert ret == "int" and fn.restype is C.c_int
    assert len(params) == len(fn.argtypes) == (11 if name == "rt_occluded_surfels" else 14)
    for ctype, bound in zip(params, fn.argtypes):
        if ctype.endswith("*"):
            assert bound is C.c_void_p or issubclass(bound, C._Pointer), (ctype, bound)
            if bound is not C.c_void_p:
                assert ctype == "uint32_t*" and C.sizeof(bound._type_) == 4, (ctype, bound)
        else:
            assert bound is SCALARS[ctype], (ctype, bound)
    if name == "rt_occluded_surfels":
        assert params == ["rt_scene*", "int32_t", "const struct rt_surfel*", "int64_t", "const double*", "int32_t", "uint64_t",
                          "uint64_t", "uint64_t", "uint32_t*", "uint32_t*"]
    else:
        assert params == ["rt_scene*", "int32_t", "const struct rt_surfel*", "int64_t", "const uint32_t*", "int64_t",
                          "const double*", "int32_t", "uint64_t", "uint64_t", "uint64_t", "uint32_t*", "uint32_t*", "void*"]


def test_the_header_compiles_as_c99(tmp_path):
    """The prototypes stand in the "occlusion queries" section, before rt_surfel is defined: the forward
    declaration must be one a C compiler takes without a warning."""
    src = tmp_path / "use.c"
    src.write_text('#include "rtcore.h"\nint use(rt_scene* s, const rt_surfel* p, uint32_t* o)\n'
                   "{ return rt_occluded_surfels(s, RT_GATHER_COSINE, p, 1, 0, 4, 0, 0, 0, o, 0); }\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c",
                    str(src), "-o", str(tmp_path / "use.o")], check=True)


def test_arguments_refused_without_a_device(rc):
    """Both entry points refuse an unknown gather mode (first), a null scene, n < 0, spp <= 0, and for
    n > 0 a null surfels or occluded pointer, n_records out of range and a null index with n != n_records,
    before anything is launched (no device is touched: this runs on a machine without one), and leave the
    outputs alone; n == 0 is RT_OK with null pointers and touches nothing, the scene included (the handle
    here is not a scene)."""
    lib = rc.load_library()
    surfels, tm = (rc.rt_surfel * 2)(), (C.c_double * 2)(1.0, 1.0)
    occ, ns = (C.c_uint32 * 2)(0xABABABAB, 0xABABABAB), (C.c_uint32 * 2)(0xCDCDCDCD, 0xCDCDCDCD)
    index = (C.c_uint32 * 2)(0, 1)
    not_a_scene = C.create_string_buffer(64)

    def host(scene, mode, sf, n, t, spp, o):
        return lib.rt_occluded_surfels(scene, mode, sf, n, t, spp, 1, 0, 0, o, ns)

    def device(scene, mode, sf, n, t, spp, o, n_records=None, idx=None):
        return lib.rt_occluded_surfels_device(scene, mode, sf, n if n_records is None else n_records, idx, n, t, spp, 1, 0, 0, o,
                                              ns, None)

    for fn, name in ((host, "rt_occluded_surfels"), (device, "rt_occluded_surfels_device")):
        for mode in (3, -1, 7):  # the unknown mode first: before the null scene, n < 0 and spp <= 0
            for scene, n, spp in ((None, 2, 4), (not_a_scene, -1, 4), (not_a_scene, 2, 0), (not_a_scene, 0, 4)):
                assert fn(scene, mode, surfels, n, tm, spp, occ) == -1
                assert "gather mode" in _last_error(lib) and name + ":" in _last_error(lib)
        assert fn(None, 1, surfels, 2, tm, 4, occ) == -1 and "null scene" in _last_error(lib)
        assert fn(None, 1, None, 0, None, 4, None) == -1  # a null scene, even for n == 0
        assert fn(not_a_scene, 1, surfels, -1, tm, 4, occ) == -1 and "n < 0" in _last_error(lib)
        for spp in (0, -3):
            assert fn(not_a_scene, 1, surfels, 2, tm, spp, occ) == -1 and "spp" in _last_error(lib)
            assert fn(not_a_scene, 1, None, 0, None, spp, None) == -1  # spp is checked before n == 0
        assert fn(not_a_scene, 1, None, 2, tm, 4, occ) == -1 and "null pointer" in _last_error(lib)
        assert fn(not_a_scene, 1, surfels, 2, tm, 4, None) == -1 and "null pointer" in _last_error(lib)
        for mode in MODES:
            assert fn(not_a_scene, mode, None, 0, None, 4, None) == 0
    for n_records in (0, -5, 1 << 32, 1 << 40):
        assert device(not_a_scene, 1, surfels, 2, tm, 4, occ, n_records=n_records, idx=index) == -1
        assert "n_records" in _last_error(lib)
    assert device(not_a_scene, 1, surfels, 2, tm, 4, occ, n_records=3) == -1 and "n != n_records" in _last_error(lib)
    assert device(not_a_scene, 1, None, 0, None, 4, None, n_records=0) == 0  # n == 0 comes before n_records
    assert bytes(occ) == b"\xab" * 8 and bytes(ns) == b"\xcd" * 8
    assert bytes(not_a_scene) == bytes(64)


class _NoLibrary:
    def __getattr__(self, name):
        raise AssertionError(f"the library was called ({name})")


def test_wrappers_reject_mismatched_shapes_before_the_library(rc):
    gpu = rc.GpuRaytracer.__new__(rc.GpuRaytracer)
    gpu.lib, gpu.handle = _NoLibrary(), None
    p, nrm = np.zeros((5, 3)), np.ones((5, 3))
    with pytest.raises(ValueError):
        gpu.occluded_surfels(p, np.ones((4, 3)), 4, 1)
    with pytest.raises(ValueError):
        gpu.occluded_surfels(np.zeros((5, 2)), np.ones((5, 2)), 4, 1)
    with pytest.raises(ValueError):
        gpu.occluded_surfels(p, nrm, 4, 1, t_max=np.ones(4))
    with pytest.raises(ValueError):
        gpu.occluded_surfels(p, nrm, 4, 1, t_max=np.ones((5, 1)))
    for out in ((np.zeros(4, np.uint32), np.zeros(5, np.uint32)), (np.zeros(5, np.uint32), np.zeros(5, np.int64)),
                (np.zeros(5, np.uint32),), (np.zeros(10, np.uint32)[::2], np.zeros(5, np.uint32))):
        with pytest.raises(ValueError):
            gpu.occluded_surfels(p, nrm, 4, 1, out=out)
    with pytest.raises(AssertionError, match="rt_occluded_surfels"):  # well-shaped input does reach it
        gpu.occluded_surfels(p, nrm, 4, 1, t_max=2.0)


def test_ambient_occlusion(rc):
    ao = rc.ambient_occlusion(np.array([0, 4, 1, 0], np.uint32), np.array([4, 4, 8, 0], np.uint32))
    assert ao.dtype == np.float64 and np.array_equal(ao[:3], [1.0, 0.0, 0.875]) and np.isnan(ao[3])
    assert rc.ambient_occlusion(np.zeros((2, 3), np.uint32), np.full((2, 3), 5, np.uint32)).shape == (2, 3)


def test_bake_ao_device_stands_beside_bake_ao():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import bake_ao
    finally:
        sys.path.pop(0)
    assert callable(bake_ao.bake_ao_device) and callable(bake_ao.bake_ao) and callable(bake_ao.ao_rays)
    hits = np.zeros((3, 2), np.dtype([("prim_id", np.int32), ("position", np.float32, (3,)), ("normal", np.float32, (3,))]))
    hits["prim_id"] = [[0, -1], [4, 2], [1, 7]]
    hits["normal"][..., 2] = 2.0
    hits["normal"][1, 1] = np.nan
    hits["position"] = np.random.default_rng(5).normal(size=(3, 2, 3)) * 50
    mask, pos, nrm = bake_ao.ao_surfels(hits)
    mask_r, o, _ = bake_ao.ao_rays(hits, 1, 0)
    assert np.array_equal(mask, mask_r) and np.array_equal(pos, o)  # the rays' own origins
    assert np.array_equal(nrm, np.tile([0.0, 0.0, 1.0], (4, 1)))


@pytest.mark.parametrize("name", ["bounce", "die", "mesh41"])
@pytest.mark.parametrize("mode", MODES)
def test_the_set_cannot_hollow_itself_out(name, mode):
    """The shared set at spp 5 by the reference alone (the fp64 restatement's directions, the oracle's
    distances): at t_max = 1 and at +inf the occluded share of the valid surfels' samples lies in [5 %, 95 %]
    and at least 10 % of the surfels have both outcomes among their five samples."""
    pos, nrm = surfel_set(name)
    assert pos.shape == nrm.shape == (N, 3) and len(valid_surfels()) == N - 3
    t = oracle_distances(name, mode)
    assert t.shape == (N - 3, 5)
    for t_max in (1.0, INF):
        assert_not_hollow(t < t_max, f"{name} mode {mode} t_max {t_max}")
