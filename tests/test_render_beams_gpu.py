"""rt_render_beams on the device: footprint-sampled radiance for caller-supplied rays.

The yardstick is rt_render_rays: sample k of beam i is, bit for bit, what render_rays returns at spp = 1,
sample_base + k and stream_base + i for the ray the host twin (beam_rays_host) reports for it (G1, G2).
G3 holds the draws to the library's own camera: the beams of camera_beams give the bounce-0 rays
rt_trace_paths records.  G4 - G6: position independence, plumbing, and what a call leaves alone.

The beams of G1, G2 and G4: the first 200 generator rays of tests/test_query_rays_gpu.py (the o and d of
its _rays; three full waves and a short fourth) with random footprints of about 1e-2; beams 7 and 130 are
invalid, beam 64 has an all-zero direction triple (every sample degenerate)."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from test_query_rays_gpu import _gpu, _line_of_sight_rays, _same_bits, _scene

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 11
N = 200
BASE = 123457
INVALID, ZERO = (7, 130), 64


@functools.lru_cache(maxsize=None)
def _beams(name):
    """The six (N, 3) arrays of the scene's beams (read-only, shared)."""
    o, d = (a[:N] for a in _line_of_sight_rays(_scene(name).cameras[0]))  # (_rays' o and d, without its oracle pass)
    rng = np.random.default_rng(31)
    o, d = o.copy(), d * rng.uniform(0.5, 2.0, (N, 1))  # (need not be unit)
    ou, ov, du, dv = (rng.normal(size=(N, 3)) * 1e-2 for _ in range(4))
    ou[INVALID[0], 1] = np.nan
    dv[INVALID[1], 2] = np.inf
    d[ZERO] = du[ZERO] = dv[ZERO] = 0.0
    out = (o, d, ou, ov, du, dv)
    for a in out:
        a.setflags(write=False)
    return out


def _five_single_samples(rc, gpu, beams):
    """render_rays of the twin's rays [:, k] at spp 1 for k in 0..4: the yardstick's five results."""
    rays, _ = rc.beam_rays_host(*beams, 5, SEED, stream_base=BASE)
    return [gpu.render_rays(np.ascontiguousarray(rays[:, k]), None, 1, SEED, sample_base=k, stream_base=BASE) for k in range(5)]


# ---------------------------------------------------------------- G1: the yardstick
G1_CASES = [("bounce", "BRUTE", None, (128, 128)), ("bounce", "GROUPED", None, (128, 128)), ("bounce", "BVH", None, (128, 128)),
            ("mesh41", "BVH", "HOST", None), ("mesh41", "BVH", "GPU", None), ("vn", "BRUTE", None, None), ("vn", "BVH", None, None)]


@pytest.mark.parametrize("name,mode,builder,size", G1_CASES)
def test_g1_each_sample_is_render_rays_of_the_twins_ray(rc, name, mode, builder, size):
    """For k in 0..4, render_beams(spp = 1, sample_base = k) equals render_rays of the twin's rays: sum
    bits, samples, misses and the ray count.  One call at spp = 5 is the five added in fp64 in sample
    order (5 <= B: every item is one sample)."""
    beams = _beams(name)
    gpu = _gpu(rc, name, mode, builder, size=size)
    assert gpu.info().traversal == getattr(rc, "RT_TRAVERSAL_" + mode)
    want = _five_single_samples(rc, gpu, beams)
    acc = (np.zeros((N, 3)), np.zeros(N, np.uint32), np.zeros(N, np.uint32))
    total = 0
    for k in range(5):
        s, ns, ms, rays = gpu.render_beams(*beams, 1, SEED, sample_base=k, stream_base=BASE)
        ws, wns, wms, wrays = want[k]
        assert _same_bits(s, ws) and np.array_equal(ns, wns) and np.array_equal(ms, wms) and rays == wrays, k
        assert ((ns + ms) == 1).all() and (ms[list(INVALID) + [ZERO]] == 1).all()
        acc[0][:] += ws
        acc[1][:] += wns
        acc[2][:] += wms
        total += wrays
    s, ns, ms, rays = gpu.render_beams(*beams, 5, SEED, stream_base=BASE)
    gpu.close()
    assert _same_bits(s, acc[0]) and np.array_equal(ns, acc[1]) and np.array_equal(ms, acc[2]) and rays == total
    bad = list(INVALID) + [ZERO]
    assert (ms[bad] == 5).all() and not ns[bad].any() and not s[bad].any()
    assert (ns > 0).sum() > N // 4 and total > 0
    # the footprint matters: the five samples of a beam are not one ray five times
    one = want[0][0]
    assert not _same_bits(s, 5 * one)


# ---------------------------------------------------------------- G2: several samples per item
@pytest.mark.parametrize("mode,spp", [("BRUTE", 50), ("BVH", 130)])
def test_g2_several_samples_per_item(rc, mode, spp):
    """Counts and rays exact; each sum within (s - 1) * 2^-24 * sum |c_k| of the fp64 sum of the
    per-sample render_rays results, s the samples per item (the fp32 partial-sum bound)."""
    beams = _beams("bounce")
    gpu = _gpu(rc, "bounce", mode, size=(128, 128))
    kernel = {"BRUTE": 0, "BVH": 3}[mode]
    plan = rc.pixels_plan(kernel, N, spp)
    per_item = plan["samples_per_item"]
    assert per_item > 1
    rays, _ = rc.beam_rays_host(*beams, spp, SEED, stream_base=BASE)
    acc = (np.zeros((N, 3)), np.zeros(N, np.uint32), np.zeros(N, np.uint32))
    mag = np.zeros((N, 3))
    total = 0
    for k in range(spp):
        sk, nk, mk, rk = gpu.render_rays(np.ascontiguousarray(rays[:, k]), None, 1, SEED, sample_base=k, stream_base=BASE)
        acc[0][:] += sk
        acc[1][:] += nk
        acc[2][:] += mk
        mag += np.abs(sk)
        total += rk
    s, ns, ms, count = gpu.render_beams(*beams, spp, SEED, stream_base=BASE)
    gpu.close()
    assert np.array_equal(ns, acc[1]) and np.array_equal(ms, acc[2]) and ((ns + ms) == spp).all()
    assert count == total
    err = np.abs(s - acc[0])
    bound = (per_item - 1) * 2.0 ** -24 * mag
    print(f"G2 {mode} spp {spp}: {per_item} samples per item, max error / bound = {(err / np.maximum(bound, 1e-300)).max():.3f}")
    assert (err <= bound).all()
    assert (ms[list(INVALID) + [ZERO]] == spp).all() and (ns > 0).any()


# ---------------------------------------------------------------- G3: the draws are the camera's
def test_g3_camera_beams_give_the_cameras_own_rays(rc):
    """bounce camera 0 (no depth of field, image_plane 0) at 128 x 128, the tile 16 x 8 at (16, 72), 4 spp,
    BRUTE: the twin's rays of camera_beams, row by row under stream_base = y * W + x0, against the
    record-0 rays rt_trace_paths reports for the same seed and samples.  Every direction component within
    32 * 2^-24 (two fp32 chains of about ten roundings; 1e-4 of a pixel, which subtends 1.5e-2), origins equal."""
    W, x0, y0, w, h, spp = 128, 16, 72, 16, 8, 4
    gpu = _gpu(rc, "bounce", "BRUTE", size=(W, W))
    cam = gpu.camera
    assert cam.dof_amount == 0.0 and cam.image_plane == 0.0 and cam.kind == rc.RT_CAMERA_FRUSTUM
    rec = gpu.trace_paths(x0, y0, w, h, spp, seed=SEED)[0]
    beams = rc.camera_beams(cam, (W, W), x0, y0, w, h)
    worst = 0.0
    for j in range(h):
        row = np.ascontiguousarray(beams[:, j])
        rays, uv = rc.beam_rays_host(row, None, None, None, None, None, spp, SEED, stream_base=(y0 + j) * W + x0)
        got_d, got_o = rays["direction"][..., :3], rays["origin"][..., :3]
        want_d, want_o = rec[:, j, :, 0]["direction"][..., :3], rec[:, j, :, 0]["origin"][..., :3]
        worst = max(worst, float(np.abs(got_d - want_d).max()))
        assert np.array_equal(got_o, want_o), j
    gpu.close()
    print(f"G3: max |d_beam - d_camera| = {worst:.3e} = {worst * 2 ** 24:.2f} * 2^-24")
    assert worst <= 32 * 2.0 ** -24


# ---------------------------------------------------------------- G4: position independence
@pytest.mark.parametrize("mode", ["BRUTE", "GROUPED", "BVH"])
def test_g4_a_beams_result_does_not_depend_on_its_position(rc, mode):
    beams = _beams("bounce")
    gpu = _gpu(rc, "bounce", mode, size=(128, 128))
    spp = 3
    s, ns, ms, _ = gpu.render_beams(*beams, spp, SEED, sample_base=2, stream_base=BASE)
    assert (ns > 0).any() and s.any()
    for i in (0, 1, 63, 64, 65, 199):
        s1, ns1, ms1, _ = gpu.render_beams(*[a[i:i + 1] for a in beams], spp, SEED, sample_base=2, stream_base=BASE + i)
        assert _same_bits(s1[0], s[i]) and ns1[0] == ns[i] and ms1[0] == ms[i], i
    s2 = gpu.render_beams(*beams, spp, SEED, sample_base=2, stream_base=BASE + 1)[0]
    assert not _same_bits(s2, s)
    gpu.close()


# ---------------------------------------------------------------- G5: plumbing
@pytest.fixture(scope="module")
def mesh_bvh(rc):
    gpu = _gpu(rc, "mesh41", "BVH")
    yield gpu
    gpu.close()


def _beams4097(rc):
    go, gd = _line_of_sight_rays(_scene("mesh41").cameras[0])
    o = np.concatenate([go, go[:1]])
    d = np.concatenate([gd, -gd[:1]])
    rng = np.random.default_rng(5)
    z = np.zeros_like(o)
    return rc._pack_beams(o, d, z, z, rng.normal(size=o.shape) * 1e-2, rng.normal(size=o.shape) * 1e-2)


CHILD = """
import sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import raytracercore_amd as rc
from test_query_rays_gpu import _gpu
beams = np.load(sys.argv[2])
gpu = _gpu(rc, "mesh41", "BVH")
s, ns, ms, rays = gpu.render_beams(beams, None, None, None, None, None, 2, 11, stream_base=9)
gpu.close()
np.savez(sys.argv[3], s=s, ns=ns, ms=ms, rays=rays)
"""


def test_g5_chunks(rc, mesh_bvh, tmp_path):
    """n = 4097 cut into chunks of 1000 beams (RTCORE_QUERY_CHUNK, set for a fresh child process) is the
    one-chunk call bit for bit."""
    beams = _beams4097(rc)
    full = mesh_bvh.render_beams(beams, None, None, None, None, None, 2, SEED, stream_base=9)
    assert ((full[1] + full[2]) == 2).all() and (full[1] > 0).any() and (full[2] > 0).any()
    np.save(tmp_path / "beams.npy", beams)
    env = dict(os.environ, RTCORE_QUERY_CHUNK="1000")
    subprocess.run([sys.executable, "-c", CHILD, ROOT, str(tmp_path / "beams.npy"), str(tmp_path / "out.npz")],
                   check=True, env=env, timeout=300)
    z = np.load(tmp_path / "out.npz")
    assert _same_bits(z["s"], full[0]) and _same_bits(z["ns"], full[1]) and _same_bits(z["ms"], full[2])
    assert int(z["rays"]) == full[3]


def test_g5_device_entry_on_a_side_stream(rc, mesh_bvh):
    """rt_render_beams_device on a torch side stream adds to non-zero accumulators what the host entry
    returns (planes R | G | B), its ray counter included, and leaves the sentinels round the arrays intact."""
    import torch

    n, pad = 1000, 64
    beams = _beams4097(rc)[:n]
    host = mesh_bvh.render_beams(beams, None, None, None, None, None, 4, SEED, stream_base=3)
    d_list = torch.from_numpy(beams.view(np.uint8).copy()).cuda()
    d_sum = torch.full((pad + 3 * n + pad,), 2.5, dtype=torch.float64, device="cuda")
    d_ns = torch.full((pad + n + pad,), 7, dtype=torch.int32, device="cuda")
    d_ms = torch.full((pad + n + pad,), 9, dtype=torch.int32, device="cuda")
    d_count = torch.full((3,), 41, dtype=torch.int64, device="cuda")
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    for rep in (1, 2):
        mesh_bvh.render_beams_device(d_list.data_ptr(), n, 4, SEED, 0, 3, d_sum[pad:].data_ptr(), d_ns[pad:].data_ptr(),
                                     d_ms[pad:].data_ptr(), d_count[1:].data_ptr(), stream=side.cuda_stream)
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
    lib, h = mesh_bvh.lib, mesh_bvh.handle
    args = (SEED, 0, 0, C.c_void_p(d_sum.data_ptr()), C.c_void_p(d_ns.data_ptr()), C.c_void_p(d_ms.data_ptr()), None, None)
    assert lib.rt_render_beams_device(h, C.c_void_p(d_list.data_ptr()), 62914560 + 1, 64, *args) == -1
    assert lib.rt_render_beams_device(h, C.c_void_p(d_list.data_ptr()), 2 ** 30 + 1, 1, *args) == -1
    torch.cuda.synchronize()
    assert (d_sum.cpu().numpy()[:pad] == 2.5).all()


def _sentinels(n):
    return np.full((n, 3), 7.5), np.full(n, 7, np.uint32), np.full(n, 9, np.uint32)


def _raw(rc, gpu, beams, n, spp, bufs, count=None, null=()):
    p = [beams.ctypes.data_as(C.c_void_p), bufs[0].ctypes.data_as(C.POINTER(rc.rt_color)),
         bufs[1].ctypes.data_as(C.POINTER(C.c_uint32)), bufs[2].ctypes.data_as(C.POINTER(C.c_uint32))]
    for k in null:
        p[k] = None
    return gpu.lib.rt_render_beams(gpu.handle, p[0], n, spp, SEED, 0, 0, p[1], p[2], p[3],
                                   C.byref(count) if count is not None else None)


def _last_error(lib):
    buf = C.create_string_buffer(512)
    lib.rt_last_error(buf, 512)
    return buf.value.decode()


def test_g5_empty_calls_and_errors_touch_nothing(rc, mesh_bvh):
    """n == 0: RT_OK, the sentinel-filled buffers unchanged.  Every RT_ERR_ARG case and the BVH2 scene's
    RT_ERR_STATE, with rt_render_rays' message: the same."""
    beams = _beams4097(rc)[:8]
    bufs = _sentinels(8)
    count = C.c_uint64(41)
    assert _raw(rc, mesh_bvh, beams, 0, 4, bufs, count) == 0
    assert mesh_bvh.lib.rt_render_beams_device(mesh_bvh.handle, None, 0, 1, 0, 0, 0, None, None, None, None, None) == 0
    for n, spp, null in ((8, 4, (0,)), (8, 4, (1,)), (8, 4, (2,)), (8, 4, (3,)), (-1, 4, ()), (8, 0, ()), (8, -3, ())):
        assert _raw(rc, mesh_bvh, beams, n, spp, bufs, count, null) == -1, (n, spp, null)
    gpu2 = _gpu(rc, "bounce", "BVH2")
    assert _raw(rc, gpu2, beams, 8, 4, bufs, count) == -7
    msg = _last_error(gpu2.lib)
    rays = rc._pack_rays(beams["origin"], beams["direction"])
    assert gpu2.lib.rt_render_rays(gpu2.handle, rays.ctypes.data_as(C.c_void_p), 8, 4, SEED, 0, 0,
                                   bufs[0].ctypes.data_as(C.POINTER(rc.rt_color)), bufs[1].ctypes.data_as(C.POINTER(C.c_uint32)),
                                   bufs[2].ctypes.data_as(C.POINTER(C.c_uint32)), None) == -7
    assert msg == _last_error(gpu2.lib).replace("rt_render_rays", "rt_render_beams") and "BVH2" in msg
    assert gpu2.lib.rt_render_beams_device(gpu2.handle, C.c_void_p(64), 8, 4, 0, 0, 0, C.c_void_p(64), C.c_void_p(64),
                                           C.c_void_p(64), None, None) == -7
    gpu2.close()
    want = _sentinels(8)
    assert all(_same_bits(a, b) for a, b in zip(bufs, want)) and count.value == 41
    # and the same call with nothing wrong works, adding to the sentinels
    assert _raw(rc, mesh_bvh, beams, 8, 4, bufs, count) == 0
    assert ((bufs[1] - 7) + (bufs[2] - 9) == 4).all() and count.value > 41


# ---------------------------------------------------------------- G6: what it leaves alone
@pytest.mark.parametrize("mode", ["AUTO", "BVH"])
def test_g6_render_beams_leaves_the_renderer_alone(rc, mode):
    """The checks of test_r6_render_rays_leaves_the_renderer_alone with render_beams calls in the middle:
    the counters of rt_scene_get_stats, the rt_kernel_times ring, the build statistics (the
    scene-specialised kernel's state, [15..17], among them) and the next renders are what they were."""
    beams = _beams("bounce")
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
    jit_now = gpu.build_stats()["jit_status"]
    gpu.render_beams(*beams, 2, SEED)
    gpu.render_beams(*[a[:100] for a in beams], 40, SEED, stream_base=5)
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
    stats = gpu.build_stats()
    gpu.render_beams(*[a[:64] for a in beams], 2, SEED)
    assert gpu.build_stats() == stats
    assert _same_bits(gpu.render_tile_1spp(40, 40, 24, 16, seed=3, sample_index=2), before)
    gpu.close()
