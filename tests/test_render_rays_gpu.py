"""rt_render_rays on the device: path-traced radiance for caller-supplied rays.

R1 brings the library's own samples back ray by ray (the bounce-0 rays of rt_trace_paths) and gets
their colours bit for bit.  R2 holds the colours to the CPU oracle's Scene.RayTrace through DebugGeom
scenes, with no random draw involved.  R3 / R4: a ray's result does not depend on where it stands in the
list, and a call of spp samples is spp calls of one.  R5 / R6: sizes, chunks, streams, errors, and what
a call must leave alone.

The rays of R2 - R5 are the generator of tests/test_query_rays_gpu.py (4096 unit directions, origins
along camera 0's line of sight) and its notion of a *robust* ray.  The share of rays it leaves out as
not robust, computed by the oracle on the CPU: bounce 0.27 % (11 of 4096), soup300 0.27 % (11 of 4096).
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from test_query_rays_gpu import N_RAYS, _gpu, _rays, _same_bits, _scene

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 11


# ---------------------------------------------------------------- R1: the library's own samples
# (scene, traversal, builder, frame size, tile x0, y0); the tile is 16 x 8 at 4 spp.  bounce and mesh41
# share a camera whose tile at (16, 72) straddles the silhouette: primary misses.  PLANE_SPHERE's camera
# sees the plane in every pixel, so it brings no primary miss but paths that end in the ambient colour.
R1_CASES = [
    ("bounce", "BRUTE", None, (128, 128), 16, 72), ("bounce", "GROUPED", None, (128, 128), 16, 72),
    ("bounce", "BVH", None, (128, 128), 16, 72),
    ("mesh41", "BVH", "HOST", (128, 128), 16, 72), ("mesh41", "BVH", "GPU", (128, 128), 16, 72),
    ("vn", "BRUTE", None, (64, 48), 24, 16), ("vn", "BVH", None, (64, 48), 24, 16),
    ("plane_sphere", "BRUTE", None, (64, 48), 24, 16), ("plane_sphere", "BVH", None, (64, 48), 24, 16),
]


@pytest.mark.parametrize("name,mode,builder,size,x0,y0", R1_CASES)
def test_r1_own_samples_bit_for_bit(rc, name, mode, builder, size, x0, y0):
    """Each row y and sample k of the tile in a call of its own: the row's 16 bounce-0 rays,
    stream_base = y * W + x0, sample_base = k, spp = 1 -- 32 calls of n = 16.  sum is the sample's
    colour exactly, samples / misses 1 / 0, or 0 / 1 on a primary miss with sum 0; the rays of all the
    calls add up to rt_render_tile's for the tile."""
    w, h, spp = 16, 8, 4
    gpu = _gpu(rc, name, mode, builder, size=size)
    assert gpu.info().traversal == getattr(rc, "RT_TRAVERSAL_" + mode)
    if builder:
        assert gpu.info().bvh_builder == getattr(rc, "RT_BVH_BUILDER_" + builder)
    assert gpu.camera.dof_amount == 0.0
    rec, n_rec, colors = gpu.trace_paths(x0, y0, w, h, spp, seed=SEED)
    total = 0
    n_miss = 0
    for j in range(h):
        for k in range(spp):
            r0 = np.ascontiguousarray(rec[:, j, k, 0])
            s, ns, ms, rays = gpu.render_rays(r0["origin"], r0["direction"], 1, SEED, sample_base=k,
                                              stream_base=(y0 + j) * size[0] + x0)
            total += rays
            c = colors[:, j, k]
            miss = (c == -1.0).all(axis=1)
            n_miss += int(miss.sum())
            assert np.array_equal(ns, (~miss).astype(np.uint32)) and np.array_equal(ms, miss.astype(np.uint32)), (j, k)
            assert _same_bits(s[~miss], c[~miss]), (j, k)
            assert not s[miss].any()
    assert total == gpu.render_tile(x0, y0, w, h, spp, seed=SEED)[3]
    if name in ("bounce", "mesh41"):
        assert 0 < n_miss < w * h * spp
    if name == "vn":  # a vertex-normal triangle hit at bounce 0 and left again: the re-hit test ran
        vn_ids = [i for i, p in enumerate(_scene("vn").prims) if p.flags & rc.RT_FLAG_HASNORMALS]
        assert (np.isin(rec[..., 0]["prim_id"], vn_ids) & (n_rec > 1)).any()
    if name == "plane_sphere":  # paths that leave the scene after a bounce: the ambient colour
        later = rec[..., 1:]
        assert ((later["type"] == rc.RT_BOUNCE_MISSED) & (np.arange(1, rec.shape[-1]) < n_rec[..., None])).any()
    gpu.close()


# ---------------------------------------------------------------- R2: against the oracle, DebugGeom
def _debug_geom_scene(rc, name):
    scene = _scene(name)
    params = rc.rt_scene_params.from_buffer_copy(scene.params)
    params.debug_geom = 1
    prims = (rc.rt_prim * scene.n_prims).from_buffer_copy(scene.prims)
    if name == "soup300":  # its primitives all carry the default (black) material: give each its own, so
        for i, p in enumerate(prims):  # that the colour names the primitive; every third is not reflective
            p.diffuse = rc.rt_color(0.1 + (i * 0.37) % 1.0, 0.1 + (i * 0.61) % 1.0, 0.1 + (i * 0.13) % 1.0)
            p.specular = rc.rt_color(0.05 * (i % 7), 0.03 * (i % 5), 0.07 * (i % 3))
            p.emission = rc.rt_color(0.01 * (i % 5), 0.0, 0.02 * (i % 4))
            p.shininess = -1.0 if i % 3 == 0 else 10.0
    return rc.ParsedScene(params, prims, scene.cameras)


@pytest.mark.parametrize("name,mode", [("bounce", "BRUTE"), ("bounce", "GROUPED"), ("bounce", "BVH"),
                                       ("soup300", "BRUTE"), ("soup300", "BVH")])
def test_r2_debug_geom_colours_of_the_oracles_hits(rc, name, mode):
    """params.debug_geom = 1 (Raytracer.cs:93-98): a sample's colour is specular + diffuse + emission
    of the primitive hit, specular after Primitive.Specular's Shininess <= 0 gating (Primitive.cs:111-
    129), and no number is drawn.  On the robust rays the primitive is the one orc_raytrace names, the
    colour agrees within 4 * 2^-24 relative per component (three fp32 roundings of the materials and
    two adds) and the misses are the oracle's.  Fewer than 5 % of the rays are left out as not robust.
    (soup300's copy also gets a material per primitive: the scene's own are all the black default.)"""
    R = _rays(name)
    rob = R["robust"]
    assert 1.0 - rob.mean() < 0.05
    scene = _debug_geom_scene(rc, name)
    gpu = rc.GpuRaytracer(scene, 0, traversal=getattr(rc, "RT_TRAVERSAL_" + mode))
    spp = 2
    s, ns, ms, rays = gpu.render_rays(R["o"], R["d"], spp, seed=5)
    gpu.close()
    assert rays == N_RAYS * spp  # every sample is one query
    want = np.zeros((N_RAYS, 3))
    for i in np.flatnonzero(R["ids"] >= 0):
        p = scene.prims[int(R["ids"][i])]
        spec = (p.specular.r, p.specular.g, p.specular.b) if p.shininess > 0 else (0.0, 0.0, 0.0)
        want[i] = np.add(np.add(spec, (p.diffuse.r, p.diffuse.g, p.diffuse.b)), (p.emission.r, p.emission.g, p.emission.b))
    hit = R["ids"] >= 0
    assert (hit & rob).sum() > N_RAYS // 4 and (~hit & rob).sum() > N_RAYS // 8
    assert np.array_equal(ns[rob], np.where(hit, spp, 0)[rob]) and np.array_equal(ms[rob], np.where(hit, 0, spp)[rob])
    assert ((ns + ms) == spp).all()
    got = s[rob & hit] / spp
    err = np.abs(got - want[rob & hit])
    print(f"R2 {name} {mode}: non-robust {1 - rob.mean():.4%}, max relative colour error "
          f"{(err / np.maximum(want[rob & hit], 1e-300)).max():.3e}")
    assert (err <= 4 * 2.0 ** -24 * want[rob & hit]).all()
    assert not s[rob & ~hit].any()
    assert len(np.unique(want[rob & hit], axis=0)) >= 3


# ---------------------------------------------------------------- R3: position independence
@pytest.mark.parametrize("mode", ["BRUTE", "GROUPED", "BVH"])
def test_r3_a_rays_result_does_not_depend_on_its_position(rc, mode):
    """Ray i of a call (stream_base = b, n = 200) is the single-ray call (stream_base = b + i, n = 1),
    bit for bit, for rays in the first, second and last wave of the call."""
    R = _rays("bounce")
    o, d = R["o"][:200], R["d"][:200]
    gpu = _gpu(rc, "bounce", mode)
    b, spp = 123457, 3
    s, ns, ms, _ = gpu.render_rays(o, d, spp, SEED, sample_base=2, stream_base=b)
    assert (ns > 0).any() and s.any()
    for i in (0, 1, 63, 64, 65, 199):
        s1, ns1, ms1, _ = gpu.render_rays(o[i:i + 1], d[i:i + 1], spp, SEED, sample_base=2, stream_base=b + i)
        assert _same_bits(s1[0], s[i]) and ns1[0] == ns[i] and ms1[0] == ms[i], i
    # and it does depend on the stream: the same ray under another key takes other paths
    s2 = gpu.render_rays(o, d, spp, SEED, sample_base=2, stream_base=b + 1)[0]
    assert not _same_bits(s2, s)
    gpu.close()


# ---------------------------------------------------------------- R4: several samples per ray
@pytest.mark.parametrize("mode", ["BRUTE", "BVH"])
def test_r4_one_call_of_16_spp_is_16_calls_of_one(rc, mode):
    """Counts and ray totals exact; each sum within 15 * 2^-24 * sum |c| of the 16 single samples added
    in fp64: the fp32 partial-sum bound of the kernels' per-item accumulation (at 16 spp an item is one
    sample and the fold adds them in sample order in fp64, so the sums are in fact equal; the bound is
    what holds at every spp)."""
    R = _rays("bounce")
    o, d = R["o"][:300], R["d"][:300]
    gpu = _gpu(rc, "bounce", mode)
    s, ns, ms, rays = gpu.render_rays(o, d, 16, SEED, stream_base=77)
    acc = (np.zeros((300, 3)), np.zeros(300, np.uint32), np.zeros(300, np.uint32))
    mag = np.zeros((300, 3))
    total = 0
    for k in range(16):
        sk, _, _, rk = gpu.render_rays(o, d, 1, SEED, sample_base=k, stream_base=77)
        mag += np.abs(sk)
        total += rk
        gpu.render_rays(o, d, 1, SEED, sample_base=k, stream_base=77, out=acc)
    gpu.close()
    assert np.array_equal(ns, acc[1]) and np.array_equal(ms, acc[2]) and ((ns + ms) == 16).all()
    assert rays == total
    assert (np.abs(s - acc[0]) <= 15 * 2.0 ** -24 * mag).all()
    assert (ns > 0).any() and (ms > 0).any()


# ---------------------------------------------------------------- R5: sizes and plumbing
@pytest.fixture(scope="module")
def mesh_bvh(rc):
    gpu = _gpu(rc, "mesh41", "BVH")
    yield gpu
    gpu.close()


def _rays4097():
    R = _rays("mesh41")
    return np.concatenate([R["o"], R["o"][:1]]), np.concatenate([R["d"], -R["d"][:1]])


CHILD = """
import sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import raytracercore_amd as rc
from test_query_rays_gpu import _gpu
z = np.load(sys.argv[2])
gpu = _gpu(rc, "mesh41", "BVH")
s, ns, ms, rays = gpu.render_rays(z["o"], z["d"], 2, 11, stream_base=9)
gpu.close()
np.savez(sys.argv[3], s=s, ns=ns, ms=ms, rays=rays)
"""


def test_r5_sizes_and_chunks(rc, mesh_bvh, tmp_path):
    """n = 1, 63, 64, 65 and 4097 are prefixes of one another; a host call cut into chunks of 1024 rays
    (RTCORE_QUERY_CHUNK, set for a fresh child process) is the uncut call bit for bit."""
    o, d = _rays4097()
    full = mesh_bvh.render_rays(o, d, 2, SEED, stream_base=9)
    assert ((full[1] + full[2]) == 2).all() and (full[1] > 0).any() and (full[2] > 0).any()
    for n in (1, 63, 64, 65):
        part = mesh_bvh.render_rays(o[:n], d[:n], 2, SEED, stream_base=9)
        for a, b in zip(part[:3], full[:3]):
            assert _same_bits(a, b[:n]), n
    np.savez(tmp_path / "rays.npz", o=o, d=d)
    env = dict(os.environ, RTCORE_QUERY_CHUNK="1024")
    subprocess.run([sys.executable, "-c", CHILD, ROOT, str(tmp_path / "rays.npz"), str(tmp_path / "out.npz")],
                   check=True, env=env, timeout=300)
    z = np.load(tmp_path / "out.npz")
    assert _same_bits(z["s"], full[0]) and _same_bits(z["ns"], full[1]) and _same_bits(z["ms"], full[2])
    assert int(z["rays"]) == full[3]


def test_r5_device_entry_on_a_side_stream_and_accumulation(rc, mesh_bvh):
    """rt_render_rays_device on a torch side stream equals the host entry (planes R | G | B), its ray
    counter included; a second call into the same buffers, host or device, adds."""
    import torch

    o, d = _rays4097()
    n = 1000
    host = mesh_bvh.render_rays(o[:n], d[:n], 4, SEED, stream_base=3)
    rays = rc._pack_rays(o[:n], d[:n])
    d_list = torch.from_numpy(rays.view(np.uint8).copy()).cuda()
    d_sum = torch.zeros(3 * n, dtype=torch.float64, device="cuda")
    d_ns = torch.zeros(n, dtype=torch.int32, device="cuda")
    d_ms = torch.zeros(n, dtype=torch.int32, device="cuda")
    d_count = torch.zeros(1, dtype=torch.int64, device="cuda")
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    for rep in (1, 2):
        mesh_bvh.render_rays_device(d_list.data_ptr(), n, 4, SEED, 0, 3, d_sum.data_ptr(), d_ns.data_ptr(),
                                    d_ms.data_ptr(), d_count.data_ptr(), stream=side.cuda_stream)
        side.synchronize()
        assert _same_bits(d_sum.cpu().numpy().reshape(3, n).T, rep * host[0])
        assert np.array_equal(d_ns.cpu().numpy().view(np.uint32), rep * host[1])
        assert np.array_equal(d_ms.cpu().numpy().view(np.uint32), rep * host[2])
        assert int(d_count.item()) == rep * host[3]
    # a null counter is allowed
    mesh_bvh.render_rays_device(d_list.data_ptr(), n, 4, SEED, 0, 3, d_sum.data_ptr(), d_ns.data_ptr(),
                                d_ms.data_ptr(), 0, stream=side.cuda_stream)
    side.synchronize()
    assert _same_bits(d_sum.cpu().numpy().reshape(3, n).T, 3 * host[0])
    # the host entry adds into `out` as well
    acc = tuple(a.copy() for a in host[:3])
    again = mesh_bvh.render_rays(o[:n], d[:n], 4, SEED, stream_base=3, out=acc)
    assert again[0] is acc[0] and _same_bits(acc[0], 2 * host[0]) and np.array_equal(acc[1], 2 * host[1])
    assert np.array_equal(acc[2], 2 * host[2]) and again[3] == host[3]
    # the device entry's size bound (include/rtcore.h): 64 spp on the BVH kernel, 62,914,560 rays
    lib, h = mesh_bvh.lib, mesh_bvh.handle
    args = (SEED, 0, 0, C.c_void_p(d_sum.data_ptr()), C.c_void_p(d_ns.data_ptr()), C.c_void_p(d_ms.data_ptr()), None, None)
    assert lib.rt_render_rays_device(h, C.c_void_p(d_list.data_ptr()), 62914560 + 1, 64, *args) == -1
    assert lib.rt_render_rays_device(h, C.c_void_p(d_list.data_ptr()), 2 ** 30 + 1, 1, *args) == -1
    torch.cuda.synchronize()
    assert _same_bits(d_sum.cpu().numpy().reshape(3, n).T, 3 * host[0])


def _sentinels(n):
    return np.full((n, 3), 7.5), np.full(n, 7, np.uint32), np.full(n, 9, np.uint32)


def _raw(rc, gpu, rays, n, spp, bufs, count=None, null=()):
    p = [rays.ctypes.data_as(C.c_void_p), bufs[0].ctypes.data_as(C.POINTER(rc.rt_color)),
         bufs[1].ctypes.data_as(C.POINTER(C.c_uint32)), bufs[2].ctypes.data_as(C.POINTER(C.c_uint32))]
    for k in null:
        p[k] = None
    return gpu.lib.rt_render_rays(gpu.handle, p[0], n, spp, SEED, 0, 0, p[1], p[2], p[3],
                                  C.byref(count) if count is not None else None)


def test_r5_empty_calls_and_errors_touch_nothing(rc, mesh_bvh):
    """n == 0: RT_OK, the sentinel-filled buffers unchanged.  Every RT_ERR_ARG case and the BVH2 scene's
    RT_ERR_STATE: the same."""
    rays = rc._pack_rays(*[a[:8] for a in _rays4097()])
    bufs = _sentinels(8)
    count = C.c_uint64(41)
    assert _raw(rc, mesh_bvh, rays, 0, 4, bufs, count) == 0
    assert mesh_bvh.lib.rt_render_rays_device(mesh_bvh.handle, None, 0, 1, 0, 0, 0, None, None, None, None, None) == 0
    for n, spp, null in ((8, 4, (0,)), (8, 4, (1,)), (8, 4, (2,)), (8, 4, (3,)), (-1, 4, ()), (8, 0, ()), (8, -3, ())):
        assert _raw(rc, mesh_bvh, rays, n, spp, bufs, count, null) == -1, (n, spp, null)
    gpu2 = _gpu(rc, "bounce", "BVH2")
    assert _raw(rc, gpu2, rays, 8, 4, bufs, count) == -7
    buf = C.create_string_buffer(512)
    gpu2.lib.rt_last_error(buf, 512)
    assert "BVH" in buf.value.decode()
    gpu2.close()
    want = _sentinels(8)
    assert all(_same_bits(a, b) for a, b in zip(bufs, want)) and count.value == 41
    # and the same call with nothing wrong works, adding to the sentinels
    assert _raw(rc, mesh_bvh, rays, 8, 4, bufs, count) == 0
    assert ((bufs[1] - 7) + (bufs[2] - 9) == 4).all() and count.value > 41


@pytest.mark.parametrize("mode", ["BRUTE", "GROUPED", "BVH"])
def test_r5_invalid_rays_are_primary_misses(rc, mode):
    """NaN origin, infinite component, zero direction, NaN direction: misses += spp, nothing else, no
    ray counted; the rays around them get what they get without them."""
    R = _rays("bounce")
    gpu = _gpu(rc, "bounce", mode)
    o, d = R["o"][:70].copy(), R["d"][:70].copy()
    spp = 5
    ref = gpu.render_rays(o, d, spp, SEED)
    bad = [3, 17, 64, 69]
    o[3, 1] = np.nan
    d[17, 0] = np.inf
    d[64] = 0.0
    d[69, 2] = np.nan
    s, ns, ms, rays = gpu.render_rays(o, d, spp, SEED)
    assert (ms[bad] == spp).all() and not ns[bad].any() and not s[bad].any()
    keep = np.setdiff1d(np.arange(70), bad)
    for a, b in zip((s, ns, ms), ref[:3]):
        assert _same_bits(a[keep], b[keep])
    assert (ref[1][bad] > 0).any()  # some of them were hits before
    # the four rays alone, under the keys they had in the list, trace what the list lost
    lost = sum(gpu.render_rays(R["o"][i:i + 1], R["d"][i:i + 1], spp, SEED, stream_base=i)[3] for i in bad)
    assert rays == ref[3] - lost and lost > 0
    assert gpu.render_rays(o[bad], d[bad], spp, SEED)[3] == 0
    gpu.close()


# ---------------------------------------------------------------- R6: what it leaves alone
@pytest.mark.parametrize("mode", ["AUTO", "BVH"])
def test_r6_render_rays_leaves_the_renderer_alone(rc, mode):
    """Before and after render_rays calls: the counters of rt_scene_get_stats (enabled), the
    rt_kernel_times ring, build statistic [15] (the scene-specialised kernel's state) and a
    rt_render_tile_1spp pass are what they were.  The ring is held by its length, exactly: three timed
    launches before and after, so rt_kernel_times(4) is refused.  A launch's duration is derived from
    its event pair again at every read, and two reads of one launch were seen to differ in the seventh
    digit with no render_rays call between them; so the durations are compared to 1e-4 relative (a
    render_rays launch recorded in the ring would be another launch's duration altogether)."""
    R = _rays("bounce")
    gpu = _gpu(rc, "bounce", mode, size=(128, 128))
    before = gpu.render_tile_1spp(40, 40, 24, 16, seed=3, sample_index=2)
    tile = gpu.render_tile(40, 40, 24, 16, 8, seed=3)
    assert rc.BUILD_STAT_NAMES[15] == "jit_status"
    jit = gpu.build_stats()["jit_status"]
    gpu.set_stats(True)
    gpu.render_tile(0, 0, 16, 16, 2, seed=4)
    assert sum(gpu.get_stats().values()) > 0  # (read and zeroed)
    launches = gpu.kernel_times(3)
    with pytest.raises(rc.RtError):
        gpu.kernel_times(4)
    jit_now = gpu.build_stats()["jit_status"]  # (0 after the instrumented launch, which runs the generic kernel)
    gpu.render_rays(R["o"], R["d"], 2, SEED)
    gpu.render_rays(R["o"][:100], R["d"][:100], 40, SEED, stream_base=5)
    with pytest.raises(rc.RtError):
        gpu.kernel_times(4)
    assert np.allclose(gpu.kernel_times(3), launches, rtol=1e-4, atol=0)
    assert np.allclose(gpu.kernel_times(1), launches[2:], rtol=1e-4, atol=0)
    assert sum(gpu.get_stats().values()) == 0
    assert gpu.build_stats()["jit_status"] == jit_now
    gpu.set_stats(False)
    assert _same_bits(gpu.render_tile_1spp(40, 40, 24, 16, seed=3, sample_index=2), before)
    after = gpu.render_tile(40, 40, 24, 16, 8, seed=3)
    assert all(_same_bits(a, b) for a, b in zip(tile[:3], after[:3])) and tile[3] == after[3]
    assert gpu.build_stats()["jit_status"] == jit
    # and with the scene-specialised kernel in use (AUTO): its state and the other build figures stay
    stats = gpu.build_stats()
    gpu.render_rays(R["o"][:64], R["d"][:64], 2, SEED)
    assert gpu.build_stats() == stats
    assert _same_bits(gpu.render_tile_1spp(40, 40, 24, 16, seed=3, sample_index=2), before)
    gpu.close()
