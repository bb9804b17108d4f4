"""rt_occluded_rays, host side (no GPU): the exported symbols and their bindings, the arguments refused
before anything touches a device, GpuRaytracer.visible's ray construction and the ray generator of
tools/bake_ao.py."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _last_error(lib):
    buf = C.create_string_buffer(512)
    lib.rt_last_error(buf, 512)
    return buf.value.decode()


@pytest.fixture(scope="module")
def bake_ao():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import bake_ao as mod
    finally:
        sys.path.pop(0)
    return mod


def test_exported_and_bound(rc):
    lib = rc.load_library()
    out = subprocess.run(["nm", "-D", "--defined-only", rc.LIB_PATH], capture_output=True, text=True).stdout
    for name in ("rt_occluded_rays", "rt_occluded_rays_device"):
        assert f" T {name}\n" in out
        assert getattr(lib, name).argtypes is not None
    for name in ("occluded_rays", "occluded_rays_device", "visible"):
        assert callable(getattr(rc.GpuRaytracer, name))
    assert rc.ABI_VERSION == 6 == lib.rt_abi_version()  # additive: detected by symbol


def test_arguments_refused_without_a_device(rc):
    """Both entry points refuse a null scene, n < 0 and an unknown mode before anything is launched (no
    device is touched: this runs on a machine without one) and leave the output alone; n == 0 is RT_OK
    with null pointers and touches nothing, the scene included (the handle here is not a scene)."""
    lib = rc.load_library()
    rays, t_max, out = (rc.rt_ray * 2)(), (C.c_double * 2)(1.0, 1.0), (C.c_uint8 * 2)(0xAB, 0xAB)
    not_a_scene = C.create_string_buffer(64)
    for fn, extra, name in ((lib.rt_occluded_rays, (), "rt_occluded_rays"),
                            (lib.rt_occluded_rays_device, (None,), "rt_occluded_rays_device")):
        assert fn(None, 0, rays, t_max, 2, out, *extra) == -1
        assert "null scene" in _last_error(lib) and name + ":" in _last_error(lib)
        assert fn(None, 0, rays, None, 2, out, *extra) == -1
        assert fn(None, 0, None, None, 0, None, *extra) == -1  # a null scene, even for n == 0
        assert fn(not_a_scene, 1, rays, t_max, -1, out, *extra) == -1 and "n < 0" in _last_error(lib)
        for mode in (2, 5, -1):
            assert fn(not_a_scene, mode, rays, t_max, 2, out, *extra) == -1 and "mode" in _last_error(lib)
        for mode in (0, 1):
            assert fn(not_a_scene, mode, None, None, 0, None, *extra) == 0
    assert bytes(out) == b"\xab\xab"
    assert bytes(not_a_scene) == bytes(64)


def test_visible_ray_construction(rc):
    """segment_rays (GpuRaytracer.visible): origin a (w = 1), direction normalize(b - a) (w = 0) unit to
    1e-15, t_max = |b - a|; coincident points give a zero direction and t_max 0, the empty segment that
    nothing occludes; tiny and huge separations keep their precision."""
    rng = np.random.default_rng(3)
    a = rng.normal(size=(5, 40, 3)) * 10.0
    b = a + rng.normal(size=(5, 40, 3)) * np.exp(rng.uniform(-30, 30, (5, 40, 1)))
    b[1, 7] = a[1, 7]
    b[4, 39] = a[4, 39]
    rays, t_max = rc.segment_rays(a, b)
    assert rays.shape == (5, 40) and rays.dtype == rc.RAY_DTYPE and t_max.shape == (5, 40) and t_max.dtype == np.float64
    same = np.zeros((5, 40), bool)
    same[1, 7] = same[4, 39] = True
    assert np.array_equal(rays["origin"][..., :3], a) and (rays["origin"][..., 3] == 1.0).all()
    assert (rays["direction"][..., 3] == 0.0).all()
    d = rays["direction"][..., :3]
    assert np.abs(np.linalg.norm(d[~same], axis=-1) - 1.0).max() <= 1e-15
    assert (d[same] == 0.0).all() and (t_max[same] == 0.0).all()
    v = (b - a)[~same]
    dist = np.sqrt((v.astype(np.longdouble) ** 2).sum(axis=-1)).astype(np.float64)
    assert np.allclose(t_max[~same], dist, rtol=1e-15, atol=0)  # a few fp64 roundings
    assert (t_max[~same] > 0).all() and np.isfinite(t_max).all()
    # the direction is b - a's: d * t_max walks from a to b
    assert np.allclose(d[~same] * t_max[~same][:, None], v, rtol=2e-15, atol=1e-15 * dist[:, None])
    far = rc.segment_rays(np.zeros((1, 3)), np.array([[3e200, 4e200, 0.0]]))
    assert np.isclose(far[1][0], 5e200, rtol=1e-15, atol=0) and np.allclose(far[0]["direction"][0, :3], [0.6, 0.8, 0.0], rtol=1e-15)
    with pytest.raises(ValueError):
        rc.segment_rays(np.zeros((4, 3)), np.zeros((5, 3)))
    with pytest.raises(ValueError):
        rc.segment_rays(np.zeros((4, 2)), np.zeros((4, 2)))


def test_bake_ao_ray_generator(rc, bake_ao):
    """ao_directions is reproducible for a seed and differs between seeds; every direction is unit and lies
    strictly in the hemisphere of its normal; the mean of cos(theta) is that of the cosine distribution
    (2/3).  ao_rays gives rays to hits with a finite normal only, offset off the surface along it."""
    rng = np.random.default_rng(5)
    n = rng.normal(size=(500, 3))
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    n[:3] = np.eye(3)
    n[3:6] = -np.eye(3)
    d = bake_ao.ao_directions(n, 16, 9)
    assert d.shape == (500, 16, 3) and d.dtype == np.float64
    assert np.array_equal(d, bake_ao.ao_directions(n, 16, 9))
    assert not np.array_equal(d, bake_ao.ao_directions(n, 16, 10))
    assert np.abs(np.linalg.norm(d, axis=-1) - 1.0).max() <= 1e-15
    cos = np.einsum("nkc,nc->nk", d, n)
    assert (cos > 0).all()
    # E[cos] = 2/3, Var[cos] = 1/18: 8000 samples put the mean within 5 sigma = 0.0132 of it
    assert abs(cos.mean() - 2.0 / 3.0) < 5 * np.sqrt(1.0 / 18.0 / cos.size)
    hits = np.zeros((3, 2), rc.HIT_DTYPE)
    hits["prim_id"] = [[0, -1], [4, 2], [1, 7]]
    hits["normal"][..., 2] = 1.0
    hits["normal"][1, 1] = np.nan  # Triangle.GetNormal's quirk
    hits["position"] = rng.normal(size=(3, 2, 3)) * 50
    mask, o, dd = bake_ao.ao_rays(hits, 4, 1)
    assert np.array_equal(mask, [[True, False], [True, False], [True, True]])
    assert o.shape == dd.shape == (16, 3)
    pos = hits["position"][mask].astype(np.float64)
    off = (o.reshape(4, 4, 3) - pos[:, None, :])
    assert (off[..., :2] == 0).all() and (off[..., 2] > 0).all()
    assert np.allclose(off[..., 2], bake_ao.AO_EPSILON * np.maximum(1.0, np.abs(pos).max(axis=1))[:, None], rtol=1e-6)
    assert (dd[:, 2] > 0).all()
