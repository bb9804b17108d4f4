"""rt_query_rays / rt_camera_rays, host side (no GPU): the layout of rt_ray and rt_hit in C, ctypes and
numpy, the camera's rays against the oracle, and the arguments refused before anything touches a device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from oracle.oracle import OracleScene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# one sphere under an orthographic camera (tests/test_gpu_parity.py EDGE_SCENES["sphere"])
ORTHO_SCENE = "size 16 12\northographic 0 -4 0 0 0 0 0 0 1 1.5\nemission 1 .5 .25\nsphere 0 0 0 1\n"


@pytest.fixture(scope="module")
def c_layout(tmp_path_factory):
    """tests/host/query_layout.c compiled as C against include/rtcore.h, and what it prints."""
    exe = str(tmp_path_factory.mktemp("layout") / "query_layout")
    subprocess.run(["cc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", exe,
                    os.path.join(ROOT, "tests", "host", "query_layout.c")], check=True)
    lines = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split("\n")
    return [ln.split() for ln in lines if ln]


def test_ray_and_hit_layout_agree(rc, c_layout):
    """H1: sizeof rt_ray == 64, sizeof rt_hit == 48, the offsets 0 / 4 / 8 / 16 / 28 / 40, in C, in the
    ctypes mirror and in the numpy dtypes; the modes are 0 / 1 under ABI version 6."""
    assert c_layout[0] == ["sizeof", "64", "48"]
    assert C.sizeof(rc.rt_ray) == 64 == rc.RAY_DTYPE.itemsize
    assert C.sizeof(rc.rt_hit) == 48 == rc.HIT_DTYPE.itemsize
    fields = [(n, int(o), int(sz)) for n, o, sz in c_layout[1:7]]
    assert [o for _, o, _ in fields] == [0, 4, 8, 16, 28, 40]
    assert [n for n, _, _ in fields] == [n for n, _ in rc.rt_hit._fields_] == list(rc.HIT_DTYPE.names)
    for name, off, sz in fields:
        cf = getattr(rc.rt_hit, name)
        assert (cf.offset, cf.size) == (off, sz), name
        dt, doff = rc.HIT_DTYPE.fields[name][:2]
        assert (doff, dt.itemsize) == (off, sz), name
    assert c_layout[7] == ["ray", "0", "32"]
    assert (rc.rt_ray.origin.offset, rc.rt_ray.direction.offset) == (0, 32)
    assert [rc.RAY_DTYPE.fields[k][1] for k in ("origin", "direction")] == [0, 32]
    assert c_layout[8] == ["modes", "0", "1", "abi", "6"]
    assert (rc.RT_QUERY_FAST, rc.RT_QUERY_EXACT) == (0, 1) == (int(rc.rt_query_mode.RT_QUERY_FAST),
                                                                 int(rc.rt_query_mode.RT_QUERY_EXACT))
    assert rc.ABI_VERSION == 6


def test_exported_and_bound(rc):
    lib = rc.load_library()
    out = subprocess.run(["nm", "-D", "--defined-only", rc.LIB_PATH], capture_output=True, text=True).stdout
    for name in ("rt_query_rays", "rt_query_rays_device", "rt_camera_rays"):
        assert f" T {name}\n" in out
        assert getattr(lib, name).argtypes is not None
    for name in ("query_rays", "query_rays_device", "camera_rays"):
        assert hasattr(rc.GpuRaytracer, name)


def _camera_case(rc, scenes, name):
    if name == "ortho":
        scene, size = rc.SceneLoader.from_text(ORTHO_SCENE), (16, 12)
    else:
        scene, size = scenes[name], (64, 48)
    params = rc.rt_scene_params.from_buffer_copy(scene.params)
    params.width, params.height = size
    return scene, size, OracleScene.from_abi(params, list(scene.prims), list(scene.cameras))


@pytest.mark.parametrize("name", ["bounce.txt", "die.txt", "ortho"])
def test_camera_rays_are_the_primary_rays(rc, scenes, name):
    """H2: every ray of camera_rays, fed to the oracle's Scene.RayTrace, gives the oracle's own
    primary ID of that pixel; directions are unit to 1e-15, w is 1 / 0; every ragged tile equals
    the slice of the full frame bit for bit."""
    scene, (W, H), orc = _camera_case(rc, scenes, name)
    rays = rc.camera_rays(scene.cameras[0], (W, H))
    assert rays.shape == (W, H) and rays.dtype == rc.RAY_DTYPE
    ids = orc.primary_ids()
    got = np.array([[orc.raytrace(rays[x, y]["origin"], rays[x, y]["direction"])[0] for y in range(H)]
                    for x in range(W)], np.int32)
    assert np.array_equal(got, ids)
    assert (ids >= 0).any() and (ids < 0).any()
    assert np.abs(np.linalg.norm(rays["direction"][..., :3], axis=-1) - 1.0).max() <= 1e-15
    assert (rays["origin"][..., 3] == 1.0).all() and (rays["direction"][..., 3] == 0.0).all()
    for x0, y0, w, h in [(0, 0, 1, 1), (W - 1, H - 1, 1, 1), (3, 5, 7, 4), (W - 9, 0, 9, H), (0, H - 5, W, 5)]:
        tile = rc.camera_rays(scene.cameras[0], (W, H), x0, y0, w, h)
        assert tile.shape == (w, h)
        assert tile.tobytes() == np.ascontiguousarray(rays[x0:x0 + w, y0:y0 + h]).tobytes(), (x0, y0, w, h)


def _last_error(lib):
    buf = C.create_string_buffer(512)
    lib.rt_last_error(buf, 512)
    return buf.value.decode()


def test_camera_rays_arguments(rc, scenes):
    """H3: null pointers, a tile outside the frame, w or h <= 0, a bad frame or camera kind: RT_ERR_ARG,
    nothing written."""
    lib = rc.load_library()
    cam = rc.rt_camera.from_buffer_copy(scenes["bounce.txt"].cameras[0])
    out = (rc.rt_ray * 16)()

    def call(c, W, H, x0, y0, w, h, o):
        return lib.rt_camera_rays(C.byref(c) if c is not None else None, W, H, x0, y0, w, h, o)

    assert call(cam, 8, 8, 0, 0, 4, 4, out) == 0
    assert bytes(out) != bytes(C.sizeof(out))
    out = (rc.rt_ray * 16)()
    assert call(None, 8, 8, 0, 0, 4, 4, out) == -1 and "rt_camera_rays" in _last_error(lib)
    assert call(cam, 8, 8, 0, 0, 4, 4, None) == -1
    for x0, y0, w, h in [(5, 0, 4, 4), (0, 5, 4, 4), (-1, 0, 4, 4), (0, -1, 4, 4), (0, 0, 0, 4), (0, 0, 4, 0),
                         (0, 0, -2, 4), (0, 0, 4, -2), (2 ** 31 - 2, 0, 4, 4)]:
        assert call(cam, 8, 8, x0, y0, w, h, out) == -1, (x0, y0, w, h)
    assert call(cam, 0, 8, 0, 0, 4, 4, out) == -1 and call(cam, 8, -1, 0, 0, 4, 4, out) == -1
    bad = rc.rt_camera.from_buffer_copy(cam)
    bad.kind = 7
    assert call(bad, 8, 8, 0, 0, 4, 4, out) == -1
    assert bytes(out) == bytes(C.sizeof(out))  # nothing was written
    with pytest.raises(rc.RtError):
        rc.camera_rays(cam, (8, 8), 6, 0, 4, 4)


def test_query_arguments_refused_without_a_device(rc):
    """rt_query_rays and rt_query_rays_device refuse a null scene, n < 0 and an unknown mode before
    anything is launched (no device is touched: this runs on a machine without one)."""
    lib = rc.load_library()
    rays, hits = (rc.rt_ray * 2)(), (rc.rt_hit * 2)()
    for fn, extra in ((lib.rt_query_rays, ()), (lib.rt_query_rays_device, (None,))):
        assert fn(None, 0, rays, 2, hits, *extra) == -1 and "null scene" in _last_error(lib)
        assert fn(None, 1, rays, -1, hits, *extra) == -1
        assert fn(None, 5, rays, 2, hits, *extra) == -1
    assert bytes(hits) == bytes(C.sizeof(hits))


def test_pack_rays(rc):
    """query_rays' input form: (n, 3) or (n, 4) arrays, w filled with 1 / 0."""
    o = np.arange(6, dtype=np.float32).reshape(2, 3)
    d4 = np.array([[0, 0, 1, 0], [1, 0, 0, 0]], np.float64)
    r = rc._pack_rays(o, d4)
    assert r.dtype == rc.RAY_DTYPE and r.shape == (2,)
    assert np.array_equal(r["origin"], [[0, 1, 2, 1], [3, 4, 5, 1]])
    assert np.array_equal(r["direction"], d4)
    with pytest.raises(ValueError):
        rc._pack_rays(o, d4[:1])
    with pytest.raises(ValueError):
        rc._pack_rays(o[:, :2], d4)
