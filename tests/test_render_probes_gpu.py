"""rt_render_probes on the device: L2 spherical-harmonic sums of a point's RT_GATHER_SPHERE gather samples.

Promise 1, G1: the result is, bit for bit, probe_fold_host (rt_debug_probe_fold) and the numpy replay of
tests/test_render_probes_host.py over the rays surfel_rays reports and what render_rays returns for each at
spp = 1.  Promise 3, G2: a + b samples are a, then b at sample_base + a.  Promise 2, G3: position and chunk
independence.  G4 and G5: two scenes whose answer is known.  G6: plumbing, errors, what a call leaves alone.

The probes are the surfels of tests/test_render_surfels_gpu.py (N = 200: three full waves and a short fourth;
BAD lists the three invalid ones), their normals kept: a probe's normal fixes the frame of its directions."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from test_query_rays_gpu import _gpu, _same_bits
from test_render_probes_host import K0, basis, replay
from test_render_surfels_gpu import BAD, BASE, FURNACE, N, OPEN_SKY, SEED, _last_error, _surfels
from test_render_surfels_host import SPHERE

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOOD = np.setdiff1d(np.arange(N), BAD)


def _yardstick(gpu, pos, nrm, spp, sample_base=0, stream_base=BASE):
    """(rays [n, spp], rgb [n, spp, 3] f32, miss [n, spp] bool, ray count): the reported rays and render_rays
    of each at spp = 1."""
    rays = gpu.surfel_rays(pos, nrm, spp, SEED, SPHERE, sample_base=sample_base, stream_base=stream_base)
    singles = [gpu.render_rays(np.ascontiguousarray(rays[:, k]), None, 1, SEED, sample_base=sample_base + k, stream_base=stream_base)
               for k in range(spp)]
    rgb = np.stack([s for s, _, _, _ in singles], axis=1).astype(np.float32)
    miss = np.stack([ms for _, _, ms, _ in singles], axis=1) == 1
    assert all(((ns + ms) == 1).all() for _, ns, ms, _ in singles)
    return rays, rgb, miss, sum(c for _, _, _, c in singles)


# ---------------------------------------------------------------- G1: promise 1
@pytest.mark.parametrize("name,mode,spp", [("bounce", "BRUTE", 5), ("bounce", "BRUTE", 50), ("bounce", "BVH", 130), ("die", "GROUPED", 7)])
def test_g1_result_is_the_fold_of_the_per_sample_results(rc, name, mode, spp):
    """Every bit of sh, samples, misses and the ray count, against the host twin and against the numpy replay.
    50 spp: the scalar gather runs 3 samples per item there; 130: not a power of two, above a wave."""
    pos, nrm = _surfels(name)
    gpu = _gpu(rc, name, mode, size=(128, 128))
    assert gpu.info().traversal == getattr(rc, "RT_TRAVERSAL_" + mode)
    rays, rgb, miss, total = _yardstick(gpu, pos, nrm, spp)
    sh, ns, nm, count = gpu.render_probes(pos, spp, SEED, normals=nrm, stream_base=BASE)
    gpu.close()
    assert sh.shape == (N, 9, 4) and sh.dtype == np.float64
    twin = rc.probe_fold_host(rays, rgb, miss)
    rep = replay(rays, rgb, miss)
    for want in (twin, rep):
        assert _same_bits(sh, want[0]) and np.array_equal(ns, want[1]) and np.array_equal(nm, want[2])
    assert count == total and ((ns + nm) == spp).all()
    assert (nm[BAD] == spp).all() and not ns[BAD].any() and not sh[BAD].any()
    assert not rays[BAD].view(np.float64).any()
    hits, skies = int((ns[GOOD] > 0).sum()), int((nm[GOOD] > 0).sum())
    print(f"G1 {name} {mode} spp {spp}: {hits} probes with hits, {skies} with misses, {count} rays")
    assert hits > N // 4 and skies > 0 and sh[GOOD][..., :3].any() and sh[GOOD][..., 3].any()


# ---------------------------------------------------------------- G2: promise 3
@pytest.mark.parametrize("mode", ["BRUTE", "BVH"])
def test_g2_samples_in_two_calls_are_one_call(rc, mode):
    """50 spp in one call == 20 spp, then 30 at sample_base + 20 into the same arrays: bit for bit."""
    pos, nrm = _surfels("bounce")
    gpu = _gpu(rc, "bounce", mode, size=(128, 128))
    one = gpu.render_probes(pos, 50, SEED, normals=nrm, sample_base=3, stream_base=BASE)
    out = gpu.render_probes(pos, 20, SEED, normals=nrm, sample_base=3, stream_base=BASE)
    first = out[0].copy()
    two = gpu.render_probes(pos, 30, SEED, normals=nrm, sample_base=23, stream_base=BASE, out=out[:3])
    gpu.close()
    assert two[0] is out[0]
    assert _same_bits(two[0], one[0]) and np.array_equal(two[1], one[1]) and np.array_equal(two[2], one[2])
    assert out[3] + two[3] == one[3]
    assert first.any() and not _same_bits(first, one[0]) and (one[1] > 0).any() and (one[2][GOOD] > 0).any()


# ---------------------------------------------------------------- G3: promise 2
@pytest.mark.parametrize("mode", ["BRUTE", "BVH"])
def test_g3_a_probes_result_does_not_depend_on_its_position(rc, mode):
    pos, nrm = _surfels("bounce")
    gpu = _gpu(rc, "bounce", mode, size=(128, 128))
    spp = 6
    sh, ns, nm, _ = gpu.render_probes(pos, spp, SEED, normals=nrm, sample_base=2, stream_base=BASE)
    assert sh.any() and (ns > 0).any()
    for i in (0, 1, 63, 64, 65, 199):
        s1, ns1, nm1, _ = gpu.render_probes(pos[i:i + 1], spp, SEED, normals=nrm[i:i + 1], sample_base=2, stream_base=BASE + i)
        assert _same_bits(s1[0], sh[i]) and ns1[0] == ns[i] and nm1[0] == nm[i], i
    s2, ns2, nm2, _ = gpu.render_probes(pos[37:], spp, SEED, normals=nrm[37:], sample_base=2, stream_base=BASE + 37)
    assert _same_bits(s2, sh[37:]) and np.array_equal(ns2, ns[37:]) and np.array_equal(nm2, nm[37:])
    s3 = gpu.render_probes(pos, spp, SEED, normals=nrm, sample_base=2, stream_base=BASE + 1)[0]
    assert not _same_bits(s3, sh)
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
out = (z["sh0"].copy(), z["ns0"].copy(), z["nm0"].copy())
sh, ns, nm, rays = gpu.render_probes(z["pos"], 3, 11, normals=z["nrm"], stream_base=9, out=out)
gpu.close()
np.savez(sys.argv[3], sh=sh, ns=ns, nm=nm, rays=rays)
"""


def test_g3_chunks(rc, bounce_bvh, tmp_path):
    """n = 200 cut into chunks of 64 probes (RTCORE_QUERY_CHUNK, set for a fresh child process) is the one-chunk
    call bit for bit, into arrays that were not zero."""
    pos, nrm = _surfels("bounce")
    rng = np.random.default_rng(5)
    start = (rng.normal(size=(N, 9, 4)), np.full(N, 3, np.uint32), np.full(N, 4, np.uint32))
    full = bounce_bvh.render_probes(pos, 3, SEED, normals=nrm, stream_base=9, out=tuple(a.copy() for a in start))
    assert ((full[1] + full[2]) == 3 + 7).all() and (full[1] > 3).any() and (full[2][GOOD] > 4).any()
    np.savez(tmp_path / "probes.npz", pos=pos, nrm=nrm, sh0=start[0], ns0=start[1], nm0=start[2])
    env = dict(os.environ, RTCORE_QUERY_CHUNK="64")
    subprocess.run([sys.executable, "-c", CHILD, ROOT, str(tmp_path / "probes.npz"), str(tmp_path / "out.npz")],
                   check=True, env=env, timeout=300)
    z = np.load(tmp_path / "out.npz")
    assert _same_bits(z["sh"], full[0]) and _same_bits(z["ns"], full[1]) and _same_bits(z["nm"], full[2])
    assert int(z["rays"]) == full[3]


# ---------------------------------------------------------------- G4: furnace
@pytest.mark.parametrize("mode", ["BRUTE", "BVH"])
def test_g4_furnace(rc, mode):
    """Inside an inverted sphere that only emits (.5, .5, .5) every sample is a hit of exactly 0.5: c[l][j] is the
    replay of sum 0.5 Y_l(d_k) bit for bit, no misses, and the band-0 radiance is 0.5 sqrt(4 pi)."""
    scene = rc.SceneLoader.from_text(FURNACE)
    gpu = rc.GpuRaytracer(scene, 0, traversal=getattr(rc, "RT_TRAVERSAL_" + mode))
    rng = np.random.default_rng(3)
    g = rng.normal(size=(64, 3))
    pos = g / np.linalg.norm(g, axis=1, keepdims=True) * (2.0 * rng.uniform(0, 1, (64, 1)) ** (1 / 3))
    nrm = rng.normal(size=(64, 3))
    rays = gpu.surfel_rays(pos, nrm, 32, SEED, SPHERE, stream_base=5)
    sh, ns, nm, count = gpu.render_probes(pos, 32, SEED, normals=nrm, stream_base=5)
    gpu.close()
    assert (ns == 32).all() and not nm.any() and count == 64 * 32
    want = replay(rays, np.full((64, 32, 3), 0.5, np.float32), np.zeros((64, 32), bool))
    assert _same_bits(sh, want[0]) and not sh[..., 3].any()
    Y = basis(rays["direction"][..., :3])
    acc = np.zeros((64, 9))
    for k in range(32):
        acc = acc + 0.5 * Y[:, k]
    assert _same_bits(sh[..., 0], acc) and _same_bits(sh[..., 1], acc) and _same_bits(sh[..., 2], acc)
    L = rc.probe_radiance_sh(sh, ns, nm, (0.1, 0.2, 0.3))
    assert np.abs(L[:, 0, :] - 0.5 * math.sqrt(4.0 * math.pi)).max() <= 1e-12
    # the higher bands of a constant are Monte Carlo noise about zero: 32 samples, sd of L_l = 0.5 sqrt(4 pi / 32)
    assert np.abs(L[:, 1:, :]).max() < 5 * 0.5 * math.sqrt(4.0 * math.pi / 32.0)


# ---------------------------------------------------------------- G5: open sky
def test_g5_open_sky(rc):
    """One two-sided plane z = 0, one probe at (0, 0, 1), 256 spp: the misses are exactly the reported rays that
    do not go down, c[.][3] is the replay over those, and the sky is above (c[2][3] > 0: Y2 is z's)."""
    scene = rc.SceneLoader.from_text(OPEN_SKY)
    gpu = rc.GpuRaytracer(scene, 0)
    pos = np.array([[0.0, 0.0, 1.0]])
    rays = gpu.surfel_rays(pos, np.array([[0.0, 0.0, 1.0]]), 256, SEED, SPHERE)
    sh, ns, nm, count = gpu.render_probes(pos, 256, SEED)  # (the default normal is +z)
    gpu.close()
    up = rays["direction"][:, :, 2] >= 0.0
    assert 64 < up.sum() < 192 and nm[0] == up.sum() and ns[0] == 256 - up.sum() and count >= 256
    Y = basis(rays["direction"][0, :, :3])
    acc = np.zeros(9)
    for k in np.flatnonzero(up[0]):
        acc = acc + Y[k]
    assert _same_bits(sh[0, :, 3], acc)
    assert sh[0, 2, 3] > 0.0 and sh[0, 0, 3] == np.cumsum(np.full(256, K0))[nm[0] - 1]
    assert abs(sh[0, 1, 3]) < sh[0, 2, 3] and abs(sh[0, 3, 3]) < sh[0, 2, 3]  # (an axis mix-up would put z's weight there)
    assert sh[0, :, :3].any()  # the plane below is lit by the sky: the hits carry colour


# ---------------------------------------------------------------- G6: plumbing
def test_g6_device_entry_on_a_side_stream(rc, bounce_bvh):
    """rt_render_probes_device on a torch side stream continues non-zero accumulators exactly as the host entry
    continues copies of them, its ray counter included, and leaves the sentinels round the arrays intact."""
    import torch

    n, pad, spp = N, 64, 4
    pos, nrm = _surfels("bounce")
    probes = rc._pack_surfels(pos, nrm)
    rng = np.random.default_rng(9)
    start = rng.normal(size=(n, 9, 4))
    host = bounce_bvh.render_probes(probes, spp, SEED, stream_base=3, out=(start.copy(), np.full(n, 7, np.uint32), np.full(n, 9, np.uint32)))
    host2 = bounce_bvh.render_probes(probes, spp, SEED, stream_base=3, out=tuple(a.copy() for a in host[:3]))
    d_list = torch.from_numpy(probes.view(np.uint8).copy()).cuda()
    sh0 = np.full(pad + 36 * n + pad, 2.5)
    sh0[pad:pad + 36 * n] = start.reshape(-1)
    d_sh = torch.from_numpy(sh0).cuda()
    d_ns = torch.full((pad + n + pad,), 7, dtype=torch.int32, device="cuda")
    d_ms = torch.full((pad + n + pad,), 9, dtype=torch.int32, device="cuda")
    d_count = torch.full((3,), 41, dtype=torch.int64, device="cuda")
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    for rep, want in ((1, host), (2, host2)):
        bounce_bvh.render_probes_device(d_list, n, spp, SEED, 0, 3, d_sh[pad:], d_ns[pad:], d_ms[pad:], d_count[1:].data_ptr(),
                                        stream=side.cuda_stream)
        side.synchronize()
        got = d_sh.cpu().numpy()
        assert _same_bits(got[pad:pad + 36 * n].reshape(n, 9, 4), want[0])
        assert (got[:pad] == 2.5).all() and (got[pad + 36 * n:] == 2.5).all()
        ns, ms = d_ns.cpu().numpy(), d_ms.cpu().numpy()
        assert np.array_equal(ns[pad:pad + n].view(np.uint32), want[1]) and np.array_equal(ms[pad:pad + n].view(np.uint32), want[2])
        assert (ns[:pad] == 7).all() and (ns[pad + n:] == 7).all() and (ms[:pad] == 9).all() and (ms[pad + n:] == 9).all()
        assert d_count.cpu().tolist() == [41, 41 + rep * host[3], 41]
    assert host[3] == host2[3] > 0 and ((host[1] - 7) + (host[2] - 9) == spp).all()


def _sentinels(n):
    return np.full((n, 9, 4), 7.5), np.full(n, 7, np.uint32), np.full(n, 9, np.uint32)


def _raw(rc, gpu, probes, n, spp, bufs, count=None, null=()):
    p = [probes.ctypes.data_as(C.c_void_p), bufs[0].ctypes.data_as(C.POINTER(rc.rt_probe_sh)),
         bufs[1].ctypes.data_as(C.POINTER(C.c_uint32)), bufs[2].ctypes.data_as(C.POINTER(C.c_uint32))]
    for k in null:
        p[k] = None
    return gpu.lib.rt_render_probes(gpu.handle, p[0], n, spp, SEED, 0, 0, p[1], p[2], p[3], C.byref(count) if count is not None else None)


def test_g6_empty_calls_and_errors_touch_nothing(rc, bounce_bvh):
    """n == 0: RT_OK, the sentinel-filled buffers unchanged.  Every RT_ERR_ARG case, the 2^26 bound at n = 64 and
    spp = 2^21 among them, and the BVH2 scene's RT_ERR_STATE with rt_render_rays' message: the same."""
    import torch

    pos, nrm = _surfels("bounce")
    probes = rc._pack_surfels(pos[20:28], nrm[20:28])
    bufs = _sentinels(8)
    count = C.c_uint64(41)
    lib, h = bounce_bvh.lib, bounce_bvh.handle
    assert _raw(rc, bounce_bvh, probes, 0, 4, bufs, count) == 0
    assert lib.rt_render_probes_device(h, None, 0, 1, 0, 0, 0, None, None, None, None, None) == 0
    for n, spp, null in ((8, 4, (0,)), (8, 4, (1,)), (8, 4, (2,)), (8, 4, (3,)), (-1, 4, ()), (8, 0, ()), (8, -3, ())):
        assert _raw(rc, bounce_bvh, probes, n, spp, bufs, count, null) == -1, (n, spp, null)
    assert _raw(rc, bounce_bvh, probes, 8, 1 << 21, bufs, count) == -1  # (not even 64 probes fit one launch)
    assert "sample_base" in _last_error(lib)
    # the device entry's bound: 64 * ceil(n / 64) * pow2ceil(spp) <= 2^26
    d_list = torch.from_numpy(rc._pack_surfels(pos[:64], nrm[:64]).view(np.uint8).copy()).cuda()
    d_sh = torch.full((64 * 36,), 2.5, dtype=torch.float64, device="cuda")
    d_ns = torch.full((64,), 7, dtype=torch.int32, device="cuda")
    d_ms = torch.full((64,), 9, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ptrs = (C.c_void_p(d_sh.data_ptr()), C.c_void_p(d_ns.data_ptr()), C.c_void_p(d_ms.data_ptr()), None, None)
    for n, spp in ((64, 1 << 21), (65, 1 << 20), (64, (1 << 20) + 1), ((1 << 26) + 1, 1), ((1 << 20) + 1, 33), (64, 2 ** 31 - 1)):
        assert lib.rt_render_probes_device(h, C.c_void_p(d_list.data_ptr()), n, spp, SEED, 0, 0, *ptrs) == -1, (n, spp)
        msg = _last_error(lib)
        assert "rt_render_probes_device" in msg and "2^26" in msg and "sample_base" in msg
    torch.cuda.synchronize()
    assert (d_sh.cpu().numpy() == 2.5).all() and (d_ns.cpu().numpy() == 7).all() and (d_ms.cpu().numpy() == 9).all()
    gpu2 = _gpu(rc, "bounce", "BVH2")
    assert _raw(rc, gpu2, probes, 8, 4, bufs, count) == -7
    msg = _last_error(gpu2.lib)
    rays = rc._pack_rays(probes["position"], probes["normal"])
    s3 = np.zeros((8, 3))
    assert gpu2.lib.rt_render_rays(gpu2.handle, rays.ctypes.data_as(C.c_void_p), 8, 4, SEED, 0, 0, s3.ctypes.data_as(C.POINTER(rc.rt_color)),
                                   bufs[1].ctypes.data_as(C.POINTER(C.c_uint32)), bufs[2].ctypes.data_as(C.POINTER(C.c_uint32)), None) == -7
    assert msg == _last_error(gpu2.lib).replace("rt_render_rays", "rt_render_probes") and "BVH2" in msg
    assert gpu2.lib.rt_render_probes_device(gpu2.handle, C.c_void_p(64), 8, 4, 0, 0, 0, C.c_void_p(64), C.c_void_p(64), C.c_void_p(64),
                                            None, None) == -7
    gpu2.close()
    want = _sentinels(8)
    assert all(_same_bits(a, b) for a, b in zip(bufs, want)) and count.value == 41 and not s3.any()
    # and the same call with nothing wrong works, continuing from the sentinels
    assert _raw(rc, bounce_bvh, probes, 8, 4, bufs, count) == 0
    assert ((bufs[1] - 7) + (bufs[2] - 9) == 4).all() and count.value > 41 and not _same_bits(bufs[0], want[0])


@pytest.mark.parametrize("mode", ["AUTO", "BVH"])
def test_g6_render_probes_leaves_the_renderer_alone(rc, mode):
    """A render_tile_1spp, a render_tile and a render_surfels before and after probe calls are bit-identical; the
    counters of rt_scene_get_stats, the rt_kernel_times ring and the build statistics are what they were."""
    pos, nrm = _surfels("bounce")
    gpu = _gpu(rc, "bounce", mode, size=(128, 128))
    before = gpu.render_tile_1spp(40, 40, 24, 16, seed=3, sample_index=2)
    tile = gpu.render_tile(40, 40, 24, 16, 8, seed=3)
    gather = gpu.render_surfels(pos, nrm, 30, SEED, SPHERE, stream_base=5)
    gpu.set_stats(True)
    gpu.render_tile(0, 0, 16, 16, 2, seed=4)
    assert sum(gpu.get_stats().values()) > 0  # (read and zeroed)
    launches = gpu.kernel_times(3)
    with pytest.raises(rc.RtError):
        gpu.kernel_times(4)
    stats = gpu.build_stats()
    gpu.render_probes(pos, 2, SEED, normals=nrm)
    gpu.render_probes(pos[:100], 40, SEED, normals=nrm[:100], stream_base=5)
    with pytest.raises(rc.RtError):
        gpu.kernel_times(4)
    assert np.allclose(gpu.kernel_times(3), launches, rtol=1e-4, atol=0)
    assert sum(gpu.get_stats().values()) == 0
    assert gpu.build_stats() == stats
    gpu.set_stats(False)
    assert _same_bits(gpu.render_tile_1spp(40, 40, 24, 16, seed=3, sample_index=2), before)
    after = gpu.render_tile(40, 40, 24, 16, 8, seed=3)
    assert all(_same_bits(a, b) for a, b in zip(tile[:3], after[:3])) and tile[3] == after[3]
    again = gpu.render_surfels(pos, nrm, 30, SEED, SPHERE, stream_base=5)
    assert all(_same_bits(a, b) for a, b in zip(gather[:3], again[:3])) and gather[3] == again[3]
    gpu.close()
