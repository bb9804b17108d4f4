"""rt_query_rays on the device: closest-hit queries for caller-supplied rays, ray by ray.

G1 / G2 hold RT_QUERY_EXACT to the CPU oracle's Scene.RayTrace (orc_raytrace) and to rt_primary_ids bit
for bit.  G3 holds RT_QUERY_FAST -- the path kernels' own fp32 closest hit in every traversal mode and
with both BVH builders -- to the oracle on every ray whose answer the fp32 rounding of the ray cannot
change.  G4 holds it to the path kernels themselves: the bounce-0 records of rt_trace_paths, bit for
bit.  G5 / G6: order, sizes, chunks, streams, errors, and what a query must leave alone.

The rays (the generator of the issue): 4096 unit directions drawn from a normal distribution, origins
along camera 0's line of sight.  A ray is *robust* if the oracle returns the same ID for it and for the
four rays normalize(d +- 1e-3 a), normalize(d +- 1e-3 b), a and b orthonormal to d: a thousand times the
fp32 rounding of the direction.  A robust hit is *well-conditioned* if across those four the oracle's
distance moves by less than 1 % of max(t, 1).
"""
import ctypes as C
import functools
import os

import numpy as np
import pytest

from oracle.oracle import OracleScene

pytestmark = pytest.mark.gpu

N_RAYS = 4096

# Distance bar of G3 on well-conditioned robust hits, |t_fast - t_oracle| / max(t_oracle, 1).  Measured on
# the MI355X over all the (scene, mode, builder) cases of G3: the largest value is G3_MEASURED_MAX =
# 1.319e-5 (soup300, BRUTE and BVH alike; every other case stays below 1.1e-6).  The bar
# is four times that, 5.276e-5, which leaves room for other seeds and stays below the project's colour
# tolerance of 1e-4.
G3_MEASURED_MAX = 1.319e-5
G3_DISTANCE_BAR = 4 * G3_MEASURED_MAX

PLANE_SPHERE = ("size 16 12\nambient color .2 .3 .4\ncamera 0 -4 3, 0 0 0, 0 0 1, 60\ndiffuse .5 .5 .5\nplane 0 0 0 1\n"
                "sphere 0 0 1 .5\n")  # tests/test_gpu_parity.py EDGE_SCENES["plane"] with a sphere appended

# tests/test_gpu_oracle_paths.py VN_SCENE: two vertex-normal quads of opposite winding over a floor plane
VN_SCENE = """size 64 48
camera 0 -1.2 3.2, 0 0 0, 0 0 1, 70
ambient color .3 .3 .35
emission 4 4 4
sphere 0 0 4 .8
emission 0 0 0
diffuse .6 .5 .4
specular .3 .3 .3
shininess 10 2
twosided true
vertexnormal -2 -1 0  -.3 -.3 1
vertexnormal 0 -1 .3   0 -.3 1
vertexnormal 0 1 .3   0 .3 1
vertexnormal -2 1 0 -.3 .3 1
trinormal 0 1 2
trinormal 0 2 3
vertexnormal 0 -1 .3   0 -.3 1
vertexnormal 2 -1 0  .3 -.3 1
vertexnormal 2 1 0 .3 .3 1
vertexnormal 0 1 .3   0 .3 1
trinormal 4 6 5
trinormal 4 7 6
diffuse .3 .3 .3
specular 0 0 0
shininess 4 .5
plane -1 0 0 1
"""

SCENE_NAMES = ("bounce", "die", "mesh41", "mesh71", "plane_sphere", "soup300")


@functools.lru_cache(maxsize=None)
def _scene(name):
    import raytracercore_amd as rc
    from raytracercore_amd.scenes import mesh_scene_text, soup_scene_text

    if name in ("bounce", "die"):
        return rc.SceneLoader.from_file(rc.scene_path(name + ".txt"))
    text = {"mesh41": lambda: mesh_scene_text(41, 41), "mesh71": lambda: mesh_scene_text(71, 41),
            "plane_sphere": lambda: PLANE_SPHERE, "soup300": lambda: soup_scene_text(300, 3), "vn": lambda: VN_SCENE}[name]()
    return rc.SceneLoader.from_text(text)


def _oracle(name):
    import raytracercore_amd as rc

    scene = _scene(name)
    return OracleScene.from_abi(rc.rt_scene_params.from_buffer_copy(scene.params), list(scene.prims), list(scene.cameras))


def _trace(orc, o, d):
    ids, ts = np.empty(len(o), np.int32), np.empty(len(o), np.float64)
    for i in range(len(o)):
        ids[i], ts[i] = orc.raytrace((o[i, 0], o[i, 1], o[i, 2], 1.0), (d[i, 0], d[i, 1], d[i, 2], 0.0))
    return ids, ts


def _line_of_sight_rays(cam, n=N_RAYS):
    """The generator: n unit directions from a normal distribution, origins along the camera's line of sight."""
    rng = np.random.default_rng(7)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    pos = np.array([cam.position.x, cam.position.y, cam.position.z])
    look = np.array([cam.look_at.x, cam.look_at.y, cam.look_at.z])
    o = pos + rng.uniform(0, .75, (n, 1)) * (look - pos)
    return o, d


@functools.lru_cache(maxsize=None)
def _rays(name):
    """The scene's rays and the oracle's answers, computed once and shared (read-only)."""
    n = N_RAYS
    o, d = _line_of_sight_rays(_scene(name).cameras[0], n)
    orc = _oracle(name)
    ids, ts = _trace(orc, o, d)
    # a, b orthonormal to d: a from the coordinate axis d is least aligned with
    e = np.eye(3)[np.argmin(np.abs(d), axis=1)]
    a = np.cross(d, e)
    a /= np.linalg.norm(a, axis=1, keepdims=True)
    b = np.cross(d, a)
    robust = np.ones(n, bool)
    moved = np.zeros(n)
    for v in (a, -a, b, -b):
        dp = d + 1e-3 * v
        dp /= np.linalg.norm(dp, axis=1, keepdims=True)
        ids_p, ts_p = _trace(orc, o, dp)
        robust &= ids_p == ids
        moved = np.maximum(moved, np.abs(ts_p - ts))
    hit = ids >= 0
    well = robust & hit & (moved < 0.01 * np.maximum(ts, 1.0))
    # the test set cannot hollow itself out
    assert robust.mean() >= 0.95, (name, robust.mean())
    assert well.sum() >= 0.85 * (robust & hit).sum(), (name, well.sum(), (robust & hit).sum())
    for arr in (o, d, ids, ts, robust, well):
        arr.setflags(write=False)
    return dict(o=o, d=d, ids=ids, t=ts, robust=robust, well=well)


def _gpu(rc, name, mode="AUTO", builder=None, size=None):
    return rc.GpuRaytracer(_scene(name), 0, size=size, traversal=getattr(rc, "RT_TRAVERSAL_" + mode),
                           builder=None if builder is None else getattr(rc, "RT_BVH_BUILDER_" + builder))


def _same_bits(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


# ---------------------------------------------------------------- G1: EXACT against the oracle
@pytest.mark.parametrize("name", SCENE_NAMES)
def test_g1_exact_equals_the_oracle(rc, name):
    """prim_id equal on every ray, robust or not; distance equal bit for bit wherever there is a hit;
    position, normal and reserved zero."""
    R = _rays(name)
    gpu = _gpu(rc, name)
    hits = gpu.query_rays(R["o"], R["d"], exact=True)
    gpu.close()
    assert hits.shape == (N_RAYS,) and hits.dtype == rc.HIT_DTYPE
    assert np.array_equal(hits["prim_id"], R["ids"])
    hit = R["ids"] >= 0
    assert hit.sum() > N_RAYS // 4
    assert _same_bits(hits["distance"][hit], R["t"][hit])
    assert (hits["distance"][~hit] == 0).all() and (hits["inside"][~hit] == 0).all()
    assert np.isin(hits["inside"], (0, 1)).all()
    assert not hits["position"].view(np.uint32).any() and not hits["normal"].view(np.uint32).any()
    assert not hits["reserved"].any()


# ---------------------------------------------------------------- G2: EXACT on camera_rays
@pytest.mark.parametrize("name", ["bounce", "die"])
def test_g2_exact_on_camera_rays_equals_primary_ids(rc, name):
    """The host's camera arithmetic (rt_camera_rays) is the device's (rt_primary_ids): the full 64x48
    frame and one offset ragged tile."""
    gpu = _gpu(rc, name, size=(64, 48))
    for x0, y0, w, h in [(0, 0, 64, 48), (37, 5, 19, 13)]:
        rays = gpu.camera_rays(x0, y0, w, h)
        hits = gpu.query_rays(rays, exact=True)
        assert hits.shape == (w, h)
        ids = gpu.primary_ids(x0, y0, w, h)
        assert np.array_equal(hits["prim_id"], ids)
        assert (ids >= 0).any() and (w < 64 or (ids < 0).any())
        assert (hits["distance"][ids >= 0] > 0).all()
    gpu.close()


# ---------------------------------------------------------------- G3: FAST against the oracle
G3_CASES = [
    ("bounce", "BRUTE", None), ("bounce", "GROUPED", None), ("bounce", "BVH", None),
    ("die", "BRUTE", None), ("die", "GROUPED", None), ("die", "BVH", None),
    ("mesh41", "GROUPED", None), ("mesh41", "BVH", "HOST"),
    ("mesh71", "BVH", "HOST"), ("mesh71", "BVH", "GPU"),
    ("plane_sphere", "BRUTE", None), ("plane_sphere", "BVH", None),
    ("soup300", "BRUTE", None), ("soup300", "BVH", None),
]


@pytest.mark.parametrize("name,mode,builder", G3_CASES)
def test_g3_fast_against_the_oracle(rc, name, mode, builder):
    """On every robust ray the fp32 kernels' prim_id is the oracle's; on well-conditioned robust hits
    the distance agrees within G3_DISTANCE_BAR.  Planes sit outside the tree, and mesh71's host-built
    tree leaves 11 outer records to the end of the query."""
    R = _rays(name)
    gpu = _gpu(rc, name, mode, builder)
    assert gpu.info().traversal == getattr(rc, "RT_TRAVERSAL_" + mode)
    if name == "mesh71":
        assert gpu.info().bvh_builder == getattr(rc, "RT_BVH_BUILDER_" + builder)
        if builder == "HOST":
            assert gpu.build_stats()["outer_prims"] == 11
    hits = gpu.query_rays(R["o"], R["d"])
    gpu.close()
    rob, well = R["robust"], R["well"]
    wrong = np.flatnonzero(rob & (hits["prim_id"] != R["ids"]))
    err = np.abs(hits["distance"][well] - R["t"][well]) / np.maximum(R["t"][well], 1.0)
    print(f"G3 {name} {mode} {builder}: robust {rob.mean():.4f} well {well.sum()} id mismatches {wrong.size} "
          f"max distance error {err.max():.3e}")
    assert wrong.size == 0, (wrong[:8], hits["prim_id"][wrong[:8]], R["ids"][wrong[:8]])
    assert err.max() < G3_DISTANCE_BAR < 1e-4
    # the fp32 distance widened exactly; misses are all zero but the ID
    assert np.array_equal(hits["distance"], hits["distance"].astype(np.float32).astype(np.float64))
    miss = hits["prim_id"] < 0
    assert (hits["prim_id"][miss] == -1).all() and not hits["distance"][miss].any() and not hits["inside"][miss].any()
    assert not hits["position"][miss].view(np.uint32).any() and not hits["normal"][miss].view(np.uint32).any()
    assert not hits["reserved"].any()


# ---------------------------------------------------------------- G4: FAST reproduces the path kernels
G4_TILES = {"bounce": ((128, 128), (16, 72, 16, 16)), "die": ((128, 128), (96, 64, 16, 16)), "vn": ((64, 48), (24, 16, 16, 16))}


@pytest.mark.parametrize("mode", ["BRUTE", "GROUPED", "BVH"])
@pytest.mark.parametrize("name", ["bounce", "die", "vn"])
def test_g4_fast_reproduces_the_path_kernels(rc, name, mode):
    """The bounce-0 records of rt_trace_paths (camera rays with jitter, die.txt's with depth of field),
    queried again by their (origin, direction): prim_id, inside, distance, position and normal are the
    record's bits, NaNs compared as bit patterns, misses included.  This holds query_hit to shade()."""
    size, tile = G4_TILES[name]
    gpu = _gpu(rc, name, mode, size=size)
    assert gpu.info().traversal == getattr(rc, "RT_TRAVERSAL_" + mode)
    rec, n_rays, _ = gpu.trace_paths(*tile, 4, seed=11)
    r0 = np.ascontiguousarray(rec[..., 0]).reshape(-1)
    hits = gpu.query_rays(r0["origin"], r0["direction"])
    gpu.close()
    assert hits.shape == r0.shape == (16 * 16 * 4,)
    assert np.array_equal(hits["prim_id"], r0["prim_id"])
    assert np.array_equal(hits["inside"], r0["inside"])
    assert np.array_equal(hits["distance"], r0["distance"].astype(np.float64))
    assert _same_bits(hits["distance"].astype(np.float32), r0["distance"])
    assert _same_bits(hits["position"], r0["position"])
    assert _same_bits(hits["normal"], r0["normal"])
    assert (r0["prim_id"] >= 0).any()
    if name != "vn":
        assert (r0["prim_id"] < 0).any()  # misses are part of the tile
    else:  # both sides of the vertex-normal quads: smooth normals, and GetNormal's NaN from behind
        nan = np.isnan(r0["normal"]).all(axis=1)
        assert nan.any() and (r0["inside"][nan] == 1).all()
        ids = np.unique(r0["prim_id"][~nan])
        assert len(np.unique(r0["prim_id"])) >= 3 and len(ids) >= 2


# ---------------------------------------------------------------- G5: plumbing
@pytest.fixture(scope="module")
def mesh_bvh(rc):
    gpu = _gpu(rc, "mesh41", "BVH")
    yield gpu
    gpu.close()


def test_g5_order_sizes_and_chunks(rc, mesh_bvh):
    """The BVH kernel deals rays to lanes dynamically: the answers still follow the rays' order, for
    every n, and do not depend on how the host entry cuts the rays into chunks."""
    R = _rays("mesh41")
    o, d = R["o"], R["d"]
    full = mesh_bvh.query_rays(o, d)
    perm = np.random.default_rng(1).permutation(N_RAYS)
    assert _same_bits(mesh_bvh.query_rays(o[perm], d[perm]), full[perm])
    for n in (1, 257, 1000):
        assert _same_bits(mesh_bvh.query_rays(o[:n], d[:n]), full[:n]), n
    os.environ["RTCORE_QUERY_CHUNK"] = "256"
    try:
        assert _same_bits(mesh_bvh.query_rays(o[:1000], d[:1000]), full[:1000])
        chunked_exact = mesh_bvh.query_rays(o[:1000], d[:1000], exact=True)
    finally:
        del os.environ["RTCORE_QUERY_CHUNK"]
    assert np.array_equal(chunked_exact["prim_id"], R["ids"][:1000])
    assert _same_bits(chunked_exact, mesh_bvh.query_rays(o[:1000], d[:1000], exact=True))
    # n == 0: RT_OK, nothing touched
    empty = mesh_bvh.query_rays(np.zeros((0, 3)), np.zeros((0, 3)))
    assert empty.shape == (0,)
    assert mesh_bvh.lib.rt_query_rays(mesh_bvh.handle, rc.RT_QUERY_FAST, None, 0, None) == 0
    assert mesh_bvh.lib.rt_query_rays_device(mesh_bvh.handle, rc.RT_QUERY_EXACT, None, 0, None, None) == 0


def test_g5_device_entry_on_a_side_stream(rc, mesh_bvh):
    """rt_query_rays_device on a torch side stream, given as its raw pointer, equals the host entry."""
    import torch

    R = _rays("mesh41")
    n = 1000
    rays = rc._pack_rays(R["o"][:n], R["d"][:n])
    d_rays = torch.from_numpy(rays.view(np.uint8).copy()).cuda()
    side = torch.cuda.Stream()
    for exact in (False, True):
        d_hits = torch.full((n * rc.HIT_DTYPE.itemsize,), 0xAB, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        mesh_bvh.query_rays_device(d_rays.data_ptr(), n, d_hits.data_ptr(), exact=exact, stream=side.cuda_stream)
        side.synchronize()
        got = d_hits.cpu().numpy().view(rc.HIT_DTYPE)
        assert _same_bits(got, mesh_bvh.query_rays(R["o"][:n], R["d"][:n], exact=exact)), exact


# ---------------------------------------------------------------- G6: manners
def _rc_of(lib, *args):
    rc_ = lib.rt_query_rays(*args)
    buf = C.create_string_buffer(512)
    lib.rt_last_error(buf, 512)
    return rc_, buf.value.decode()


def test_g6_argument_and_state_errors(rc, mesh_bvh):
    lib, h = mesh_bvh.lib, mesh_bvh.handle
    rays, hits = np.zeros(4, rc.RAY_DTYPE), np.zeros(4, rc.HIT_DTYPE)
    pr, ph = rays.ctypes.data_as(C.c_void_p), hits.ctypes.data_as(C.c_void_p)
    assert _rc_of(lib, h, 0, None, 4, ph)[0] == -1
    assert _rc_of(lib, h, 0, pr, 4, None)[0] == -1
    assert _rc_of(lib, h, 0, pr, -1, ph)[0] == -1
    code, msg = _rc_of(lib, h, 2, pr, 4, ph)
    assert code == -1 and "mode" in msg
    assert lib.rt_query_rays_device(h, 0, None, 4, None, None) == -1
    assert lib.rt_query_rays_device(h, -1, pr, 4, ph, None) == -1
    assert not hits.view(np.uint8).any()
    # FAST on a BVH2 scene: RT_ERR_STATE, the message names BVH; EXACT works there
    gpu = _gpu(rc, "bounce", "BVH2")
    code, msg = _rc_of(gpu.lib, gpu.handle, 0, pr, 4, ph)
    assert code == -7 and "BVH" in msg
    assert not hits.view(np.uint8).any()
    R = _rays("bounce")
    assert np.array_equal(gpu.query_rays(R["o"][:64], R["d"][:64], exact=True)["prim_id"], R["ids"][:64])
    gpu.close()


@pytest.mark.parametrize("mode", ["BRUTE", "GROUPED", "BVH"])
def test_g6_degenerate_rays_are_misses(rc, mode):
    """NaN origin, infinite direction, zero direction, NaN direction: misses in both query modes, and the
    rays around them are answered as if they were not there."""
    R = _rays("bounce")
    gpu = _gpu(rc, "bounce", mode)
    o, d = R["o"][:70].copy(), R["d"][:70].copy()
    ref_fast, ref_exact = gpu.query_rays(o, d), gpu.query_rays(o, d, exact=True)
    bad = [3, 17, 64, 69]
    o[3, 1] = np.nan
    d[17, 0] = np.inf
    d[64] = 0.0
    d[69, 2] = np.nan
    for exact, ref in ((False, ref_fast), (True, ref_exact)):
        hits = gpu.query_rays(o, d, exact=exact)
        assert (hits["prim_id"][bad] == -1).all()
        assert not hits[bad]["distance"].any() and not hits[bad]["inside"].any()
        assert not hits[bad]["position"].view(np.uint32).any() and not hits[bad]["normal"].view(np.uint32).any()
        keep = np.setdiff1d(np.arange(70), bad)
        assert _same_bits(hits[keep], ref[keep])
        assert (ref["prim_id"][bad] >= 0).any()  # some of them were hits before
    gpu.close()


# which of 300 rays get a NaN origin: the first 200 (the wave that draws rays 0-255 refills three times
# over without starting a walk), all of them (no wave ever walks), the last 130 (its last rounds)
G6_SPOILED = {"head": slice(0, 200), "all": slice(0, 300), "tail": slice(170, 300)}


@pytest.mark.parametrize("case", list(G6_SPOILED))
def test_g6_refill_rounds_of_invalid_rays_only(rc, mesh_bvh, case):
    """The BVH kernel's refill rounds in which every ray a wave draws is invalid, so that no lane starts a
    walk: each invalid ray is a miss record, and the valid rays' records are, bit for bit, those of the
    same rays queried alone."""
    R = _rays("mesh41")
    o, d = R["o"][:300].copy(), R["d"][:300].copy()
    bad = np.zeros(300, bool)
    bad[G6_SPOILED[case]] = True
    o[bad, 0] = np.nan
    hits = mesh_bvh.query_rays(o, d)
    assert hits.shape == (300,)
    assert (hits["prim_id"][bad] == -1).all()
    assert not hits["distance"][bad].any() and not hits["inside"][bad].any() and not hits["reserved"][bad].any()
    assert not hits["position"][bad].view(np.uint32).any() and not hits["normal"][bad].view(np.uint32).any()
    alone = mesh_bvh.query_rays(o[~bad], d[~bad])
    assert _same_bits(hits[~bad], alone)
    assert case == "all" or ((alone["prim_id"] >= 0).any() and (alone["prim_id"] < 0).any())
    assert (R["ids"][:300][bad] >= 0).any()  # some of the spoiled rays were hits


def test_g6_a_query_leaves_the_renderer_alone(rc):
    """A render after queries equals the same render before them bit for bit; the counters of
    rt_scene_get_stats and the rt_kernel_times ring are what they were."""
    R = _rays("bounce")
    gpu = _gpu(rc, "bounce", "BVH", size=(128, 128))
    before = gpu.render_tile(40, 40, 24, 16, 8, seed=3)
    gpu.render_tile(0, 0, 16, 16, 2, seed=4)
    times = gpu.kernel_times(2)
    gpu.set_stats(True)
    gpu.render_tile(0, 0, 16, 16, 2, seed=4)
    assert sum(gpu.get_stats().values()) > 0  # (read and zeroed)
    launches = gpu.kernel_times(3)
    for exact in (False, True):
        gpu.query_rays(R["o"], R["d"], exact=exact)
    assert gpu.kernel_times(3) == launches
    assert sum(gpu.get_stats().values()) == 0
    gpu.set_stats(False)
    assert launches[:2] == times
    after = gpu.render_tile(40, 40, 24, 16, 8, seed=3)
    for a, b in zip(before[:3], after[:3]):
        assert _same_bits(a, b)
    assert before[3] == after[3]
    gpu.close()
