"""rt_render_surfels on the device: gathered radiance at caller-supplied surface points.

Promise (a), G1 and G2: sample k of surfel i is, bit for bit, what render_rays returns at spp = 1,
sample_base + k and stream_base + i for the ray surfel_rays (rt_debug_surfel_rays_device) reports for it.
Promise (b), G3: that ray is the fp64 restatement of tests/test_render_surfels_host.py to within the bounds
the bounce directions are held to (tests/bounce_cases.py).  G4 and G5: two scenes whose answer is known
exactly.  G6: position independence, plumbing, and what a call leaves alone.

The surfels of G1, G2, G3 and G6: the first 200 generator rays of tests/test_query_rays_gpu.py (three full
waves and a short fourth) traced with query_rays; a hit gives position + 1e-3 normal and the normal scaled
by 0.5 .. 2, a miss (or a NaN normal) the ray's origin and minus its direction.  Surfels 7 and 130 are
invalid, surfel 64 has a zero normal, surfels 10 and 11 the normals (0, 0, +-1) exactly."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from bounce_cases import BOUNDS
from test_query_rays_gpu import _gpu, _line_of_sight_rays, _same_bits, _scene
from test_render_beams_gpu import G1_CASES
from test_render_surfels_host import COSINE, DIFFUSE, MODES, SPHERE, directions, draws

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 11
N = 200
BASE = 123457
BAD = [7, 130, 64]  # a NaN position component, an infinite normal component, a zero normal
POLES = (10, 11)


@functools.lru_cache(maxsize=None)
def _surfels(name):
    """(positions, normals), both (N, 3) f64 (read-only, shared)."""
    import raytracercore_amd as rc

    o, d = (a[:N] for a in _line_of_sight_rays(_scene(name).cameras[0]))
    gpu = _gpu(rc, name)
    hits = gpu.query_rays(o, d)
    gpu.close()
    hit = (hits["prim_id"] >= 0) & np.isfinite(hits["normal"]).all(axis=1)
    rng = np.random.default_rng(41)
    scale = rng.uniform(0.5, 2.0, (N, 1))
    hp, hn = hits["position"].astype(np.float64), hits["normal"].astype(np.float64)
    pos = np.where(hit[:, None], hp + 1e-3 * hn, o)
    nrm = np.where(hit[:, None], hn * scale, -d)
    pos[BAD[0], 1] = np.nan
    nrm[BAD[1], 2] = np.inf
    nrm[BAD[2]] = 0.0
    nrm[POLES[0]] = (0.0, 0.0, 1.0)
    nrm[POLES[1]] = (0.0, 0.0, -1.0)
    assert hit.sum() > N // 4
    pos.setflags(write=False)
    nrm.setflags(write=False)
    return pos, nrm


def _single_samples(gpu, rays, count):
    """render_rays of rays[:, k] at spp 1 for k < count: the yardstick's per-sample results."""
    return [gpu.render_rays(np.ascontiguousarray(rays[:, k]), None, 1, SEED, sample_base=k, stream_base=BASE) for k in range(count)]


# ---------------------------------------------------------------- G1: promise (a)
CASES = [c + (DIFFUSE,) for c in G1_CASES] + [("bounce", m, None, (128, 128), g) for m in ("BRUTE", "BVH") for g in (COSINE, SPHERE)]


@pytest.mark.parametrize("name,mode,builder,size,gather", CASES)
def test_g1_each_sample_is_render_rays_of_the_reported_ray(rc, name, mode, builder, size, gather):
    """For k in 0..4, render_surfels(spp = 1, sample_base = k) equals render_rays of surfel_rays(...)[:, k]:
    sum bits, samples, misses and the ray count.  One call at spp = 5 is the five added in fp64 in sample
    order (5 <= B: every item is one sample)."""
    pos, nrm = _surfels(name)
    gpu = _gpu(rc, name, mode, builder, size=size)
    assert gpu.info().traversal == getattr(rc, "RT_TRAVERSAL_" + mode)
    rays = gpu.surfel_rays(pos, nrm, 5, SEED, gather, stream_base=BASE)
    assert rays.shape == (N, 5)
    want = _single_samples(gpu, rays, 5)
    acc = (np.zeros((N, 3)), np.zeros(N, np.uint32), np.zeros(N, np.uint32))
    total = 0
    for k in range(5):
        s, ns, ms, count = gpu.render_surfels(pos, nrm, 1, SEED, gather, sample_base=k, stream_base=BASE)
        ws, wns, wms, wcount = want[k]
        assert _same_bits(s, ws) and np.array_equal(ns, wns) and np.array_equal(ms, wms) and count == wcount, k
        assert ((ns + ms) == 1).all() and (ms[BAD] == 1).all()
        acc[0][:] += ws
        acc[1][:] += wns
        acc[2][:] += wms
        total += wcount
    s, ns, ms, count = gpu.render_surfels(pos, nrm, 5, SEED, gather, stream_base=BASE)
    gpu.close()
    assert _same_bits(s, acc[0]) and np.array_equal(ns, acc[1]) and np.array_equal(ms, acc[2]) and count == total
    assert (ms[BAD] == 5).all() and not ns[BAD].any() and not s[BAD].any()
    assert not rays[BAD].view(np.float64).any()  # (an invalid surfel's rays are all zeros)
    assert (ns > 0).sum() > N // 4 and total > 0
    # the five samples of a surfel are not one ray five times
    good = np.setdiff1d(np.arange(N), BAD)
    d = rays["direction"][good]
    assert (np.abs(d[:, 1:] - d[:, :1]).max(axis=(1, 2)) > 1e-3).all()
    assert not _same_bits(s, 5 * want[0][0])


# ---------------------------------------------------------------- G2: several samples per item
@pytest.mark.parametrize("mode,spp", [("BRUTE", 50), ("BVH", 130)])
def test_g2_several_samples_per_item(rc, mode, spp):
    """Counts and rays exact; each sum within (s - 1) * 2^-24 * sum |c_k| of the fp64 sum of the
    per-sample render_rays results, s the samples per item (the fp32 partial-sum bound)."""
    pos, nrm = _surfels("bounce")
    gpu = _gpu(rc, "bounce", mode, size=(128, 128))
    kernel = {"BRUTE": 0, "BVH": 3}[mode]
    per_item = rc.pixels_plan(kernel, N, spp)["samples_per_item"]
    assert per_item > 1
    rays = gpu.surfel_rays(pos, nrm, spp, SEED, DIFFUSE, stream_base=BASE)
    acc = (np.zeros((N, 3)), np.zeros(N, np.uint32), np.zeros(N, np.uint32))
    mag = np.zeros((N, 3))
    total = 0
    for sk, nk, mk, rk in _single_samples(gpu, rays, spp):
        acc[0][:] += sk
        acc[1][:] += nk
        acc[2][:] += mk
        mag += np.abs(sk)
        total += rk
    s, ns, ms, count = gpu.render_surfels(pos, nrm, spp, SEED, DIFFUSE, stream_base=BASE)
    gpu.close()
    assert np.array_equal(ns, acc[1]) and np.array_equal(ms, acc[2]) and ((ns + ms) == spp).all()
    assert count == total
    err = np.abs(s - acc[0])
    bound = (per_item - 1) * 2.0 ** -24 * mag
    print(f"G2 {mode} spp {spp}: {per_item} samples per item, max error / bound = {(err / np.maximum(bound, 1e-300)).max():.3f}")
    assert (err <= bound).all()
    assert (ms[BAD] == spp).all() and (ns > 0).any()


# ---------------------------------------------------------------- G3: promise (b)
@pytest.mark.parametrize("gather", MODES)
def test_g3_reported_rays_against_the_fp64_restatement(rc, gather):
    """surfel_rays at 8 spp: the origin is F(position) exactly, the direction within BOUNDS["direction"]
    (max-norm) of the restatement on F(normal) and the oracle's draws, its length within
    BOUNDS["length_renormalised"] of 1.
    Measured on an MI355X over the 197 valid surfels x 8 samples: direction 1.41e-6 (DIFFUSE), 5.0e-7
    (COSINE), 1.3e-7 (SPHERE); length 9.0e-8, 8.7e-8, 8.4e-8."""
    spp = 8
    pos, nrm = _surfels("bounce")
    gpu = _gpu(rc, "bounce", "BRUTE", size=(128, 128))
    rays = gpu.surfel_rays(pos, nrm, spp, SEED, gather, stream_base=BASE)
    gpu.close()
    good = np.setdiff1d(np.arange(N), BAD)
    assert not rays[BAD].view(np.float64).any()
    o, d = rays["origin"][good], rays["direction"][good]
    assert (o[..., 3] == 1.0).all() and (d[..., 3] == 0.0).all()
    assert np.array_equal(o[..., :3], np.broadcast_to(pos[good].astype(np.float32).astype(np.float64)[:, None, :], (len(good), spp, 3)))
    assert np.array_equal(d, d.astype(np.float32).astype(np.float64))  # (fp32 values, widened)
    u1, u2 = draws(SEED, BASE + good, range(spp))
    want, _ = directions(nrm[good].astype(np.float32).astype(np.float64), gather, u1, u2)
    err = float(np.abs(d[..., :3] - want).max())
    length = float(np.abs(np.sqrt((d[..., :3] ** 2).sum(axis=2)) - 1.0).max())
    print(f"G3 mode {gather}: max |d - d64| = {err:.3e} (bound {BOUNDS['direction']:.0e}), "
          f"max | |d| - 1 | = {length:.3e} (bound {BOUNDS['length_renormalised']:.0e})")
    assert err <= BOUNDS["direction"]
    assert length <= BOUNDS["length_renormalised"]
    # the poles' frame is c = (1, 0, 0): their samples are among the compared ones
    assert all(p in good for p in POLES)


# ---------------------------------------------------------------- G4: furnace
FURNACE = ("size 16 12\ncamera 0 -4 0, 0 0 0, 0 0 1, 60\ntwosided false\ninvert true\nemission .5 .5 .5\ndiffuse 0 0 0\n"
           "specular 0 0 0\nsphere 0 0 0 5\n")


@pytest.mark.parametrize("mode", ["BRUTE", "BVH"])
def test_g4_furnace(rc, mode):
    """Inside an inverted sphere of radius 5 that only emits (.5, .5, .5), every sample of every surfel ends
    at its first hit with exactly 0.5: 32 spp sum to exactly 16 in every channel, in all three modes."""
    scene = rc.SceneLoader.from_text(FURNACE)
    gpu = rc.GpuRaytracer(scene, 0, traversal=getattr(rc, "RT_TRAVERSAL_" + mode))
    rng = np.random.default_rng(3)
    g = rng.normal(size=(64, 3))
    pos = g / np.linalg.norm(g, axis=1, keepdims=True) * (2.0 * rng.uniform(0, 1, (64, 1)) ** (1 / 3))
    nrm = rng.normal(size=(64, 3))
    for gather in MODES:
        s, ns, ms, count = gpu.render_surfels(pos, nrm, 32, SEED, gather, stream_base=5)
        assert (ns == 32).all() and not ms.any() and count == 64 * 32, gather
        assert (s == 16.0).all(), gather
        assert np.array_equal(rc.gather_mean(s, ns, ms, (0.1, 0.2, 0.3)), np.full((64, 3), 0.5))
    gpu.close()


# ---------------------------------------------------------------- G5: open sky
OPEN_SKY = "size 16 12\nambient color .2 .3 .4\ncamera 0 -4 3, 0 0 0, 0 0 1, 60\ntwosided true\ndiffuse .5 .5 .5\nplane 0 0 0 1\n"


def test_g5_open_sky(rc):
    """One two-sided plane z = 0, one surfel at (0, 0, 1) with the normal (0, 0, 1), 256 spp.  DIFFUSE and
    COSINE never leave the upper hemisphere: every sample is a primary miss.  SPHERE: the primary misses are
    the reported rays that do not go down, about half of them."""
    scene = rc.SceneLoader.from_text(OPEN_SKY)
    gpu = rc.GpuRaytracer(scene, 0)
    pos, nrm = np.array([[0.0, 0.0, 1.0]]), np.array([[0.0, 0.0, 1.0]])
    for gather in (DIFFUSE, COSINE):
        s, ns, ms, count = gpu.render_surfels(pos, nrm, 256, SEED, gather)
        assert ms[0] == 256 and ns[0] == 0 and count == 256 and not s.any(), gather
        amb = scene.params.ambient
        assert np.array_equal(rc.gather_mean(s, ns, ms, amb), [[amb.r, amb.g, amb.b]])
    rays = gpu.surfel_rays(pos, nrm, 256, SEED, SPHERE)
    up = int((rays["direction"][0, :, 2] >= 0.0).sum())
    s, ns, ms, count = gpu.render_surfels(pos, nrm, 256, SEED, SPHERE)
    gpu.close()
    print(f"G5 SPHERE: {up} of 256 rays do not go down")
    assert 64 < up < 192
    assert ms[0] == up and ns[0] == 256 - up and count >= 256


# ---------------------------------------------------------------- G6: plumbing
@pytest.mark.parametrize("mode", ["BRUTE", "GROUPED", "BVH"])
def test_g6_a_surfels_result_does_not_depend_on_its_position(rc, mode):
    """Entries of the list in separate calls, each with its own stream_base: every result is the full
    call's for that surfel."""
    pos, nrm = _surfels("bounce")
    gpu = _gpu(rc, "bounce", mode, size=(128, 128))
    spp = 3
    s, ns, ms, _ = gpu.render_surfels(pos, nrm, spp, SEED, DIFFUSE, sample_base=2, stream_base=BASE)
    assert (ns > 0).any() and s.any()
    for i in (0, 1, 63, 64, 65, 199):
        s1, ns1, ms1, _ = gpu.render_surfels(pos[i:i + 1], nrm[i:i + 1], spp, SEED, DIFFUSE, sample_base=2, stream_base=BASE + i)
        assert _same_bits(s1[0], s[i]) and ns1[0] == ns[i] and ms1[0] == ms[i], i
    # the list's tail under the stream base that keeps every surfel's stream: another n, other positions
    # and other waves, the same results
    s2, ns2, ms2, _ = gpu.render_surfels(pos[37:], nrm[37:], spp, SEED, DIFFUSE, sample_base=2, stream_base=BASE + 37)
    assert _same_bits(s2, s[37:]) and np.array_equal(ns2, ns[37:]) and np.array_equal(ms2, ms[37:])
    s3 = gpu.render_surfels(pos, nrm, spp, SEED, DIFFUSE, sample_base=2, stream_base=BASE + 1)[0]
    assert not _same_bits(s3, s)
    gpu.close()


@pytest.fixture(scope="module")
def bounce_bvh(rc):
    gpu = _gpu(rc, "bounce", "BVH", size=(128, 128))
    yield gpu
    gpu.close()


CHILD = """
import sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import raytracercore_amd as rc
from test_query_rays_gpu import _gpu
z = np.load(sys.argv[2])
gpu = _gpu(rc, "bounce", "BVH", size=(128, 128))
s, ns, ms, rays = gpu.render_surfels(z["pos"], z["nrm"], 2, 11, rc.RT_GATHER_COSINE, stream_base=9)
gpu.close()
np.savez(sys.argv[3], s=s, ns=ns, ms=ms, rays=rays)
"""


def test_g6_chunks(rc, bounce_bvh, tmp_path):
    """n = 200 cut into chunks of 64 surfels (RTCORE_QUERY_CHUNK, set for a fresh child process) is the
    one-chunk call bit for bit."""
    pos, nrm = _surfels("bounce")
    full = bounce_bvh.render_surfels(pos, nrm, 2, SEED, COSINE, stream_base=9)
    assert ((full[1] + full[2]) == 2).all() and (full[1] > 0).any() and (full[2] > 0).any()
    np.savez(tmp_path / "surfels.npz", pos=pos, nrm=nrm)
    env = dict(os.environ, RTCORE_QUERY_CHUNK="64")
    subprocess.run([sys.executable, "-c", CHILD, ROOT, str(tmp_path / "surfels.npz"), str(tmp_path / "out.npz")],
                   check=True, env=env, timeout=300)
    z = np.load(tmp_path / "out.npz")
    assert _same_bits(z["s"], full[0]) and _same_bits(z["ns"], full[1]) and _same_bits(z["ms"], full[2])
    assert int(z["rays"]) == full[3]


def test_g6_device_entry_on_a_side_stream(rc, bounce_bvh):
    """rt_render_surfels_device on a torch side stream adds to non-zero accumulators what the host entry
    returns (planes R | G | B), its ray counter included, and leaves the sentinels round the arrays intact."""
    import torch

    n, pad = N, 64
    pos, nrm = _surfels("bounce")
    surfels = rc._pack_surfels(pos, nrm)
    host = bounce_bvh.render_surfels(surfels, None, 4, SEED, SPHERE, stream_base=3)
    d_list = torch.from_numpy(surfels.view(np.uint8).copy()).cuda()
    d_sum = torch.full((pad + 3 * n + pad,), 2.5, dtype=torch.float64, device="cuda")
    d_ns = torch.full((pad + n + pad,), 7, dtype=torch.int32, device="cuda")
    d_ms = torch.full((pad + n + pad,), 9, dtype=torch.int32, device="cuda")
    d_count = torch.full((3,), 41, dtype=torch.int64, device="cuda")
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    for rep in (1, 2):
        bounce_bvh.render_surfels_device(d_list, n, 4, SEED, SPHERE, 0, 3, d_sum[pad:], d_ns[pad:], d_ms[pad:],
                                         d_count[1:].data_ptr(), stream=side.cuda_stream)
        side.synchronize()
        got = d_sum.cpu().numpy()
        want = 2.5 + host[0] if rep == 1 else (2.5 + host[0]) + host[0]
        assert _same_bits(got[pad:pad + 3 * n].reshape(3, n).T, want)
        assert (got[:pad] == 2.5).all() and (got[pad + 3 * n:] == 2.5).all()
        ns, ms = d_ns.cpu().numpy(), d_ms.cpu().numpy()
        assert np.array_equal(ns[pad:pad + n].view(np.uint32), 7 + rep * host[1])
        assert np.array_equal(ms[pad:pad + n].view(np.uint32), 9 + rep * host[2])
        assert (ns[:pad] == 7).all() and (ns[pad + n:] == 7).all() and (ms[:pad] == 9).all() and (ms[pad + n:] == 9).all()
        assert d_count.cpu().tolist() == [41, 41 + rep * host[3], 41]
    # the device entry's size bound is rt_render_rays_device's
    lib, h = bounce_bvh.lib, bounce_bvh.handle
    args = (SEED, 0, 0, C.c_void_p(d_sum.data_ptr()), C.c_void_p(d_ns.data_ptr()), C.c_void_p(d_ms.data_ptr()), None, None)
    assert lib.rt_render_surfels_device(h, 0, C.c_void_p(d_list.data_ptr()), 62914560 + 1, 64, *args) == -1
    assert lib.rt_render_surfels_device(h, 0, C.c_void_p(d_list.data_ptr()), 2 ** 30 + 1, 1, *args) == -1
    torch.cuda.synchronize()
    assert (d_sum.cpu().numpy()[:pad] == 2.5).all()


def _sentinels(n):
    return np.full((n, 3), 7.5), np.full(n, 7, np.uint32), np.full(n, 9, np.uint32)


def _raw(rc, gpu, surfels, n, spp, bufs, count=None, null=(), gather=DIFFUSE):
    p = [surfels.ctypes.data_as(C.c_void_p), bufs[0].ctypes.data_as(C.POINTER(rc.rt_color)),
         bufs[1].ctypes.data_as(C.POINTER(C.c_uint32)), bufs[2].ctypes.data_as(C.POINTER(C.c_uint32))]
    for k in null:
        p[k] = None
    return gpu.lib.rt_render_surfels(gpu.handle, gather, p[0], n, spp, SEED, 0, 0, p[1], p[2], p[3],
                                     C.byref(count) if count is not None else None)


def _last_error(lib):
    buf = C.create_string_buffer(512)
    lib.rt_last_error(buf, 512)
    return buf.value.decode()


def test_g6_empty_calls_and_errors_touch_nothing(rc, bounce_bvh):
    """n == 0: RT_OK, the sentinel-filled buffers unchanged.  Every RT_ERR_ARG case, an unknown mode among
    them, and the BVH2 scene's RT_ERR_STATE with rt_render_rays' message: the same."""
    pos, nrm = _surfels("bounce")
    surfels = rc._pack_surfels(pos[20:28], nrm[20:28])
    bufs = _sentinels(8)
    count = C.c_uint64(41)
    assert _raw(rc, bounce_bvh, surfels, 0, 4, bufs, count) == 0
    assert bounce_bvh.lib.rt_render_surfels_device(bounce_bvh.handle, 2, None, 0, 1, 0, 0, 0, None, None, None, None, None) == 0
    for n, spp, null in ((8, 4, (0,)), (8, 4, (1,)), (8, 4, (2,)), (8, 4, (3,)), (-1, 4, ()), (8, 0, ()), (8, -3, ())):
        assert _raw(rc, bounce_bvh, surfels, n, spp, bufs, count, null) == -1, (n, spp, null)
    for gather in (-1, 3, 7):
        assert _raw(rc, bounce_bvh, surfels, 8, 4, bufs, count, gather=gather) == -1
        assert "gather mode" in _last_error(bounce_bvh.lib)
        assert bounce_bvh.lib.rt_render_surfels_device(bounce_bvh.handle, gather, C.c_void_p(64), 8, 4, 0, 0, 0, C.c_void_p(64),
                                                       C.c_void_p(64), C.c_void_p(64), None, None) == -1
    gpu2 = _gpu(rc, "bounce", "BVH2")
    assert _raw(rc, gpu2, surfels, 8, 4, bufs, count) == -7
    msg = _last_error(gpu2.lib)
    rays = rc._pack_rays(surfels["position"], surfels["normal"])
    assert gpu2.lib.rt_render_rays(gpu2.handle, rays.ctypes.data_as(C.c_void_p), 8, 4, SEED, 0, 0,
                                   bufs[0].ctypes.data_as(C.POINTER(rc.rt_color)), bufs[1].ctypes.data_as(C.POINTER(C.c_uint32)),
                                   bufs[2].ctypes.data_as(C.POINTER(C.c_uint32)), None) == -7
    assert msg == _last_error(gpu2.lib).replace("rt_render_rays", "rt_render_surfels") and "BVH2" in msg
    assert gpu2.lib.rt_render_surfels_device(gpu2.handle, 0, C.c_void_p(64), 8, 4, 0, 0, 0, C.c_void_p(64), C.c_void_p(64),
                                             C.c_void_p(64), None, None) == -7
    gpu2.close()
    want = _sentinels(8)
    assert all(_same_bits(a, b) for a, b in zip(bufs, want)) and count.value == 41
    # and the same call with nothing wrong works, adding to the sentinels
    assert _raw(rc, bounce_bvh, surfels, 8, 4, bufs, count) == 0
    assert ((bufs[1] - 7) + (bufs[2] - 9) == 4).all() and count.value > 41


@pytest.mark.parametrize("jit", [True, False])
@pytest.mark.parametrize("mode", ["AUTO", "BVH"])
def test_g6_render_surfels_leaves_the_renderer_alone(rc, mode, jit):
    """A render_tile before and after surfel calls is bit-identical, with rt_set_jit on and off; the
    counters of rt_scene_get_stats, the rt_kernel_times ring and the build statistics (the scene-specialised
    kernel's state among them) are what they were."""
    pos, nrm = _surfels("bounce")
    rc.set_jit(jit)
    try:
        gpu = _gpu(rc, "bounce", mode, size=(128, 128))
        before = gpu.render_tile_1spp(40, 40, 24, 16, seed=3, sample_index=2)
        tile = gpu.render_tile(40, 40, 24, 16, 8, seed=3)
        gpu.set_stats(True)
        gpu.render_tile(0, 0, 16, 16, 2, seed=4)
        assert sum(gpu.get_stats().values()) > 0  # (read and zeroed)
        launches = gpu.kernel_times(3)
        with pytest.raises(rc.RtError):
            gpu.kernel_times(4)
        stats = gpu.build_stats()
        gpu.render_surfels(pos, nrm, 2, SEED)
        gpu.render_surfels(pos[:100], nrm[:100], 40, SEED, COSINE, stream_base=5)
        gpu.surfel_rays(pos[:64], nrm[:64], 2, SEED, SPHERE)
        with pytest.raises(rc.RtError):
            gpu.kernel_times(4)
        assert np.allclose(gpu.kernel_times(3), launches, rtol=1e-4, atol=0)
        assert sum(gpu.get_stats().values()) == 0
        assert gpu.build_stats() == stats
        gpu.set_stats(False)
        assert _same_bits(gpu.render_tile_1spp(40, 40, 24, 16, seed=3, sample_index=2), before)
        after = gpu.render_tile(40, 40, 24, 16, 8, seed=3)
        assert all(_same_bits(a, b) for a, b in zip(tile[:3], after[:3])) and tile[3] == after[3]
        gpu.close()
    finally:
        rc.set_jit(True)
