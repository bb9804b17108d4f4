"""The block cull on the host: rt_debug_block_cull's flags against the kernels' own camera rays and the oracle.

A brute-force launch is not dealt the 8x8 blocks whose pixels cannot see the scene (block_cull.cpp);
their samples are counted as primary misses.  That is sound only if no camera ray of a dead block can
meet the scene bound.  Conservative: for every dead block of every case, the rays of all four corners of
every pixel and seeded jittered rays (the jitter's extremes among them), formed in numpy float32 as
camera_ray (kernels_path.hip) forms them, fail the float32 scene_meets predicate as
test_scene_bound_host restates it, and the fp64 oracle's primary_ids reports a miss for every pixel.
Tight: the cull follows the diagonal silhouette of bounce.txt's room.  It gives up where the proof is
not available, and an empty scene is all dead.
"""
import ctypes as C

import numpy as np
import pytest

from oracle.oracle import OracleScene
from test_scene_bound_host import _meets

F32 = np.float32


def _fma(a, b, c):
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(F32)


def _camera_f32(cam, W, H):
    """camera_init (scene_prep.cpp): Camera.InitRender in fp64, rounded to the kernel's fp32 record."""
    v = lambda q: np.array([q.x, q.y, q.z], np.float64)
    unit = lambda a: a / np.sqrt((a * a).sum())
    pos, look_at, up = v(cam.position), v(cam.look_at), v(cam.up)
    look = unit(look_at - pos)
    side = unit(np.cross(look, -up))
    up2 = unit(np.cross(look, side))
    side = -side
    w2, h2 = W / 2.0, H / 2.0
    c = {"kind": cam.kind, "pos": pos.astype(F32), "look": look.astype(F32), "side": side.astype(F32),
         "up": up2.astype(F32), "w2": F32(w2), "h2": F32(h2), "image_plane": F32(cam.image_plane)}
    if cam.kind == 0:
        ty = np.tan(cam.fov_y / 2)
        tan_x, tan_y = ty * (W / float(H)), -ty
        c.update(tan_x=F32(tan_x), tan_y=F32(tan_y), txpp=F32(tan_x / w2), typp=F32(tan_y / h2))
    else:
        c.update(h_mult=F32((1 / w2) * cam.size_mult), v_mult=F32(-(1 / h2) * (H / float(W)) * cam.size_mult))
    return c


def _camera_rays(c, sx, sy):
    """camera_ray (kernels_path.hip) in float32 for the sample positions (sx, sy)."""
    sx, sy = sx.astype(F32), sy.astype(F32)
    n = len(sx)
    if c["kind"] == 0:
        ox, oy = _fma(sx, c["txpp"], -c["tan_x"]), _fma(sy, c["typp"], -c["tan_y"])
        d = _fma(c["up"][None], oy[:, None], _fma(c["side"][None], ox[:, None], np.broadcast_to(c["look"], (n, 3))))
        o = np.broadcast_to(c["pos"], (n, 3))
    else:
        ax = ((sx - c["w2"]).astype(F32) * c["h_mult"]).astype(F32)
        ay = ((sy - c["h2"]).astype(F32) * c["v_mult"]).astype(F32)
        o = _fma(c["up"][None], ay[:, None], _fma(c["side"][None], ax[:, None], np.broadcast_to(c["pos"], (n, 3))))
        d = np.broadcast_to(c["look"], (n, 3))
    d = (d / np.sqrt((d.astype(np.float64) ** 2).sum(1, keepdims=True)).astype(F32)).astype(F32)
    return _fma(d, c["image_plane"], o), d


def _frame_rows(h, y0, bands):
    py = np.arange(h)
    if not bands:
        return y0 + py
    band, stride, offset = bands
    return y0 + ((py // band) * stride + offset) * band + py % band


def _ortho(rc, cam):
    o = rc.rt_camera.from_buffer_copy(cam)
    o.kind = rc.RT_CAMERA_ORTHO
    o.size_mult = 4.0
    return o


_state = {}


def _bounce(rc):
    if "scene" not in _state:
        _state["scene"] = rc.SceneLoader.from_file(rc.scene_path("bounce.txt"))
        _state["bound"] = rc.scene_bound(_state["scene"].prims)
    return _state["scene"], _state["bound"]


def _oracle_ids(rc, scene, cam, size):
    """The oracle's primary IDs [x, y] of the whole frame, once per camera and size."""
    key = ("ids", C.string_at(C.addressof(cam), C.sizeof(cam)), size)
    if key not in _state:
        params = rc.rt_scene_params.from_buffer_copy(scene.params)
        params.width, params.height = size
        _state[key] = OracleScene.from_abi(params, list(scene.prims), [cam]).primary_ids()
    return _state[key]


# (case, camera index or "ortho", frame size, window or None, band set or None)
CASES = [("cam%d_%dx%d" % (k, w, h), k, (w, h), None, None) for k in range(8) for (w, h) in ((160, 90), (203, 77))]
CASES += [
    ("ortho_160x90", "ortho", (160, 90), None, None),
    ("ortho_203x77", "ortho", (203, 77), None, None),
    ("cam0_window", 0, (256, 144), (3, 5, 203, 77), None),
    ("cam2_window", 2, (256, 144), (16, 8, 100, 121), None),
    ("cam0_band8", 0, (160, 90), None, (8, 2, 1)),
    ("cam0_band5", 0, (160, 90), None, (5, 2, 1)),
    ("cam0_band5_203x77", 0, (203, 77), None, (5, 2, 1)),
]


@pytest.mark.parametrize("case,cam,size,window,bands", CASES, ids=[c[0] for c in CASES])
def test_dead_blocks_see_nothing(rc, case, cam, size, window, bands):
    scene, bound = _bounce(rc)
    camera = _ortho(rc, scene.cameras[0]) if cam == "ortho" else scene.cameras[cam]
    W, H = size
    dead, live = rc.block_cull(scene.prims, camera, size, window, bands)
    assert live == int((~dead).sum())
    rows = rc.load_library().rt_band_rows(H, *bands) if bands else H
    x0, y0, w, h = window or (0, 0, W, rows)
    assert dead.shape == ((h + 7) // 8, (w + 7) // 8)
    if cam in (1, 5):  # inside the room
        assert live == dead.size
        return
    assert dead.any() and not dead.all()  # (every other camera of bounce.txt looks at the room from outside)
    # the real pixels of every dead block, in frame coordinates
    py, px = np.nonzero(np.kron(dead.astype(np.uint8), np.ones((8, 8), np.uint8))[:h, :w])
    fx, fy = x0 + px, _frame_rows(h, y0, bands)[py]
    assert fy.max() < H and fx.max() < W
    ids = _oracle_ids(rc, scene, camera, size)
    assert (ids[fx, fy] < 0).all(), "the oracle sees a primitive in a dead block"
    assert (ids >= 0).any()
    # rays: the four corners of every pixel (x + 1 is what the jitter can round up to), and seeded
    # jitter drawn as the kernel draws it, a 24-bit integer scaled by 2^-24
    r = np.random.default_rng(len(case))
    sx = [fx, fx + 1, fx, fx + 1]
    sy = [fy, fy, fy + 1, fy + 1]
    for _ in range(4):
        sx.append(_fma(r.integers(0, 1 << 24, len(fx)).astype(F32), F32(2.0 ** -24), fx.astype(F32)))
        sy.append(_fma(r.integers(0, 1 << 24, len(fy)).astype(F32), F32(2.0 ** -24), fy.astype(F32)))
    o, d = _camera_rays(_camera_f32(camera, W, H), np.concatenate(sx).astype(F32), np.concatenate(sy).astype(F32))
    meets = _meets(bound, o, d)[0]
    assert not meets.any(), (int(meets.sum()), len(meets))


def test_tight_against_the_silhouette(rc):
    """bounce.txt camera 0 at 1080p: the room's image is a hexagon.  Its bounding rectangle alone would
    cull 62.8 % of the 32,400 blocks, the exact silhouette 76.0 %; one ring of blocks along a perimeter of
    about 440 blocks is the allowance."""
    scene, _ = _bounce(rc)
    dead, live = rc.block_cull(scene.prims, scene.cameras[0], (1920, 1080))
    assert dead.size == 32400 and live == 32400 - int(dead.sum())
    assert dead.sum() >= 0.74 * 32400, int(dead.sum())
    # the live blocks are a convex shape: no dead block between two live ones of a row
    for row in ~dead:
        k = np.flatnonzero(row)
        assert len(k) == 0 or row[k[0]:k[-1] + 1].all()


def test_gives_up_where_the_proof_is_not_available(rc, scenes):
    scene, _ = _bounce(rc)
    size = (160, 90)
    n = 20 * 12
    assert rc.block_cull(scene.prims, scene.cameras[1], size)[1] == n  # inside the room
    with_plane = rc.SceneLoader.from_text(open(rc.scene_path("bounce.txt")).read() + "\nplane 0 0 1 -9\n")
    assert sum(p.kind == rc.RT_PRIM_PLANE for p in with_plane.prims) == 1
    assert rc.block_cull(with_plane.prims, with_plane.cameras[0], size)[1] == n
    die = scenes["die.txt"]
    assert die.cameras[0].dof_amount != 0
    assert rc.block_cull(die.prims, die.cameras[0], size)[1] == n  # depth of field
    for field in ("position", "look_at", "up"):
        cam = rc.rt_camera.from_buffer_copy(scene.cameras[0])
        getattr(cam, field).x = float("nan")
        assert rc.block_cull(scene.prims, cam, size)[1] == n
    cam = rc.rt_camera.from_buffer_copy(scene.cameras[0])
    cam.image_plane = float("inf")
    assert rc.block_cull(scene.prims, cam, size)[1] == n
    # a sphere whose radius is not finite: the bound's state is "no skip"
    prims = list((rc.rt_prim * scene.n_prims).from_buffer_copy(scene.prims))
    next(p for p in prims if p.kind == rc.RT_PRIM_SPHERE).radius = float("inf")
    assert rc.block_cull(prims, scene.cameras[0], size)[1] == n
    # and the camera it does serve is culled at this size
    assert rc.block_cull(scene.prims, scene.cameras[0], size)[1] < n // 2


def test_empty_scene_is_all_dead(rc):
    scene, _ = _bounce(rc)
    dead, live = rc.block_cull([], scene.cameras[0], (160, 90))
    assert live == 0 and dead.all()
    dead, live = rc.block_cull([], scene.cameras[0], (203, 77), (3, 5, 100, 50))
    assert live == 0 and dead.shape == (7, 13) and dead.all()
