"""rt_render_pixels / rt_render_pixels_device on the device: the camera's own samples for a list of frame
pixels, added into whole-frame accumulators, with the moments of the error estimate.

P1 holds a list of a window's pixels to rt_render_tile / rt_render_device of that window, bit for bit.
P2 holds single samples to rt_render_tile_1spp.  P3: a pixel's record does not depend on the list it
comes in, on the entry point or on the host entry's chunking.  P4 / P5: several samples per work item
against the fp64 sums of the single samples, and the moments against numpy.  P6: errors, and what a
call must leave alone.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from test_query_rays_gpu import _gpu, _same_bits, _scene

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 11
W0, H0 = 32, 24  # P1's window


def _lum(c):
    """DoubleColor.GetLuminance in fp64, left to right, every operation rounded on its own (numpy fuses nothing)."""
    return (0.299 * c[..., 0] + 0.587 * c[..., 1]) + 0.114 * c[..., 2]


def _window_pixels(W, x0, y0, w, h):
    y, x = np.mgrid[y0:y0 + h, x0:x0 + w]
    return (y * W + x).reshape(-1).astype(np.uint32)


def _silhouette_window(gpu, w, h):
    """The first window on the 8-pixel grid (row-major) in which between a quarter and three quarters of the
    pixels see a primitive."""
    hit = gpu.primary_ids() >= 0  # [x, y]
    for y0 in range(0, gpu.height - h + 1, 8):
        for x0 in range(0, gpu.width - w + 1, 8):
            share = hit[x0:x0 + w, y0:y0 + h].mean()
            if 0.25 <= share <= 0.75:
                return x0, y0
    raise AssertionError("no window across the silhouette")


# ---------------------------------------------------------------- P1: a window's pixels as a list
# (scene, traversal, builder, frame size, window x0, y0 or None: found across the silhouette)
P1_CASES = [
    ("bounce", "BRUTE", None, (128, 128), None), ("bounce", "GROUPED", None, (128, 128), None),
    ("bounce", "BVH", None, (128, 128), None),
    ("mesh41", "BVH", "HOST", (128, 128), None), ("mesh41", "BVH", "GPU", (128, 128), None),
    ("vn", "BRUTE", None, (64, 48), (24, 16)), ("vn", "BVH", None, (64, 48), (24, 16)),
    ("plane_sphere", "BRUTE", None, (64, 48), (16, 8)),
    ("die", "AUTO", None, (128, 128), None),
]


@pytest.mark.parametrize("name,mode,builder,size,at", P1_CASES)
def test_p1_a_windows_pixels_equal_the_tile_render(rc, name, mode, builder, size, at):
    """Every pixel of a 32 x 24 window, shuffled, at 16 spp (one sample per work item in both launches):
    sums, samples, misses and rays are rt_render_tile's of that window from zero buffers, bit for bit, and
    every pixel outside the window stays zero.  Device entry: whole-frame accumulators prefilled with
    non-zero values equal rt_render_device's window accumulators prefilled with the same, bit for bit."""
    import torch

    gpu = _gpu(rc, name, mode, builder, size=size)
    if mode != "AUTO":
        assert gpu.info().traversal == getattr(rc, "RT_TRAVERSAL_" + mode)
    if builder:
        assert gpu.info().bvh_builder == getattr(rc, "RT_BVH_BUILDER_" + builder)
    if name == "die":
        assert gpu.camera.dof_amount > 0.0
    W, H = size
    x0, y0 = at if at else _silhouette_window(gpu, W0, H0)
    spp = 16
    tile = gpu.render_tile(x0, y0, W0, H0, spp, seed=SEED, sample_base=3)
    px = np.random.default_rng(1).permutation(_window_pixels(W, x0, y0, W0, H0))
    s, ns, ms, rays = gpu.render_pixels(px, spp, seed=SEED, sample_base=3)
    win = (slice(x0, x0 + W0), slice(y0, y0 + H0))
    assert _same_bits(s[win], tile[0]) and _same_bits(ns[win], tile[1]) and _same_bits(ms[win], tile[2])
    assert rays == tile[3] and ((tile[1] + tile[2]) == spp).all()
    for a in (s, ns, ms):
        rest = a.copy()
        rest[win] = 0
        assert not rest.any()
    if at is None:
        assert (tile[2] > 0).any() and (tile[1] > 0).any()
    # the device entry against rt_render_device, from equal non-zero accumulator contents
    rng = np.random.default_rng(2)
    pre_s = rng.uniform(0.5, 9.0, (3, H0, W0))
    pre_n = rng.integers(1, 50, (H0, W0)).astype(np.int32)
    pre_m = rng.integers(1, 50, (H0, W0)).astype(np.int32)
    t_s, t_n, t_m = (torch.from_numpy(a.copy()).cuda() for a in (pre_s, pre_n, pre_m))
    t_rays = torch.zeros(2, dtype=torch.int64, device="cuda")
    gpu.render_device(x0, y0, W0, H0, spp, SEED, 3, t_s.data_ptr(), t_n.data_ptr(), t_m.data_ptr(), t_rays.data_ptr())
    f_s = torch.zeros((3, H, W), dtype=torch.float64, device="cuda")
    f_n = torch.zeros((H, W), dtype=torch.int32, device="cuda")
    f_m = torch.zeros((H, W), dtype=torch.int32, device="cuda")
    f_s[:, y0:y0 + H0, x0:x0 + W0] = torch.from_numpy(pre_s).cuda()
    f_n[y0:y0 + H0, x0:x0 + W0] = torch.from_numpy(pre_n).cuda()
    f_m[y0:y0 + H0, x0:x0 + W0] = torch.from_numpy(pre_m).cuda()
    before = (f_s.cpu().numpy(), f_n.cpu().numpy(), f_m.cpu().numpy())
    d_px = torch.from_numpy(px.view(np.int32).copy()).cuda()
    torch.cuda.synchronize()
    gpu.render_pixels_device(d_px.data_ptr(), px.size, spp, SEED, 3, f_s.data_ptr(), f_n.data_ptr(), f_m.data_ptr(),
                             d_rays=t_rays[1:].data_ptr())
    torch.cuda.synchronize()
    assert _same_bits(f_s[:, y0:y0 + H0, x0:x0 + W0].cpu().numpy(), t_s.cpu().numpy())
    assert _same_bits(f_n[y0:y0 + H0, x0:x0 + W0].cpu().numpy(), t_n.cpu().numpy())
    assert _same_bits(f_m[y0:y0 + H0, x0:x0 + W0].cpu().numpy(), t_m.cpu().numpy())
    assert int(t_rays[0]) == int(t_rays[1]) == rays
    for a, b in zip((f_s, f_n, f_m), before):  # nothing outside the window is written
        a[..., y0:y0 + H0, x0:x0 + W0] = 0
        b[..., y0:y0 + H0, x0:x0 + W0] = 0
        assert _same_bits(a.cpu().numpy(), b)
    gpu.close()


# ---------------------------------------------------------------- P2: single samples
@pytest.mark.parametrize("name,mode,at", [("bounce", "BRUTE", None), ("bounce", "BVH", None), ("plane_sphere", "BVH", (16, 8))])
def test_p2_single_samples_equal_render_tile_1spp(rc, name, mode, at):
    """spp 1 at sample_base k: every listed pixel holds the sample rt_render_tile_1spp(seed, k) returns
    for it; Placeholder there <=> misses == 1 with sum 0 here.  bounce's window brings primary misses,
    plane_sphere's none."""
    size = (128, 128) if name == "bounce" else (64, 48)
    gpu = _gpu(rc, name, mode, size=size)
    x0, y0 = at if at else _silhouette_window(gpu, W0, H0)
    px = _window_pixels(size[0], x0, y0, W0, H0)[::-1].copy()
    win = (slice(x0, x0 + W0), slice(y0, y0 + H0))
    n_miss = 0
    for k in range(4):
        one = gpu.render_tile_1spp(x0, y0, W0, H0, seed=SEED, sample_index=k)
        s, ns, ms, _ = gpu.render_pixels(px, 1, seed=SEED, sample_base=k)
        miss = (one == -1.0).all(axis=2)
        n_miss += int(miss.sum())
        assert np.array_equal(ms[win] == 1, miss) and np.array_equal(ns[win] == 1, ~miss)
        assert ((ns + ms)[win] == 1).all()
        assert _same_bits(s[win][~miss], one[~miss]) and not s[win][miss].any()
    assert (n_miss > 0) == (name == "bounce") and n_miss < 4 * W0 * H0
    gpu.close()


# ---------------------------------------------------------------- P3: independence of the list
CHILD = """
import sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import raytracercore_amd as rc
from test_query_rays_gpu import _gpu
px = np.load(sys.argv[2])
gpu = _gpu(rc, "bounce", sys.argv[4], size=(128, 128))
s, ns, ms, rays, q, nb = gpu.render_pixels(px, 100, seed=11, sample_base=5, moments=True)
gpu.close()
np.savez(sys.argv[3], s=s, ns=ns, ms=ms, rays=rays, q=q, nb=nb)
"""


def _records(out, px, W):
    """The accumulators of the listed pixels, from whole-frame [x, y] arrays."""
    x, y = px % W, px // W
    return tuple(a[x, y] for a in (out[0], out[1], out[2], out[4], out[5]))


@pytest.mark.parametrize("mode", ["BRUTE", "BVH"])
def test_p3_a_pixels_record_does_not_depend_on_the_list(rc, mode, tmp_path):
    """spp 100 (5 samples per item brute force, 2 on the BVH kernel).  37 pixels of a 64 x 64 window have
    the same bits -- sums, counts, q, batches -- in the list of all 4096, in a list of the 37, in another
    order, in the host entry cut into chunks of 64 entries (RTCORE_QUERY_CHUNK, a fresh child process) and
    in the device entry on a side stream."""
    import torch

    W = H = 128
    gpu = _gpu(rc, "bounce", mode, size=(W, H))
    assert rc.pixels_plan(0 if mode == "BRUTE" else 3, 4096, 100)["samples_per_item"] == (5 if mode == "BRUTE" else 2)
    x0, y0 = _silhouette_window(gpu, 64, 64)
    all_px = _window_pixels(W, x0, y0, 64, 64)
    rng = np.random.default_rng(3)
    some = rng.choice(all_px, 37, replace=False)
    full = gpu.render_pixels(all_px, 100, seed=SEED, sample_base=5, moments=True)
    want = _records(full, some, W)
    assert ((want[1] + want[2]) == 100).all() and (want[1] > 0).any() and want[3].any()
    for lst in (some, some[::-1].copy(), rng.permutation(all_px)):
        got = gpu.render_pixels(lst, 100, seed=SEED, sample_base=5, moments=True)
        assert all(_same_bits(a, b) for a, b in zip(_records(got, some, W), want))
    np.save(tmp_path / "px.npy", all_px)
    env = dict(os.environ, RTCORE_QUERY_CHUNK="64")
    subprocess.run([sys.executable, "-c", CHILD, ROOT, str(tmp_path / "px.npy"), str(tmp_path / "out.npz"), mode],
                   check=True, env=env, timeout=300)
    z = np.load(tmp_path / "out.npz")
    for a, b in zip((z["s"], z["ns"], z["ms"], z["q"], z["nb"]), (full[0], full[1], full[2], full[4], full[5])):
        assert _same_bits(a, b)
    assert int(z["rays"]) == full[3]
    # the device entry on a side stream (accumulators row-major, planes R | G | B)
    d_px = torch.from_numpy(some.view(np.int32).copy()).cuda()
    acc = [torch.zeros(sh, dtype=dt, device="cuda") for sh, dt in (((3, H, W), torch.float64), ((H, W), torch.int32),
           ((H, W), torch.int32), ((H, W), torch.float64), ((H, W), torch.int32))]
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    gpu.render_pixels_device(d_px.data_ptr(), 37, 100, SEED, 5, *[a.data_ptr() for a in acc], stream=side.cuda_stream)
    side.synchronize()
    x, y = some % W, some // W
    host = [a.cpu().numpy() for a in acc]
    assert _same_bits(host[0][:, y, x].T, want[0])
    for k in (1, 2, 3, 4):
        assert _same_bits(host[k][y, x], want[k].view(host[k].dtype) if k != 3 else want[k])
    assert int(host[1].sum() + host[2].sum()) == 37 * 100
    gpu.close()


# ---------------------------------------------------------------- P4 / P5: several samples per item, moments
@pytest.fixture(scope="module", params=["BRUTE", "BVH"])
def hundred(rc, request):
    """bounce 128 x 128, a 32 x 24 window across the silhouette: the 200 one-sample passes of sample
    indices 0 .. 199 (computed once, read only) and the scene."""
    mode = request.param
    gpu = _gpu(rc, "bounce", mode, size=(128, 128))
    x0, y0 = _silhouette_window(gpu, W0, H0)
    ones = np.stack([gpu.render_tile_1spp(x0, y0, W0, H0, seed=SEED, sample_index=k) for k in range(200)])
    ones.setflags(write=False)
    yield {"gpu": gpu, "mode": mode, "x0": x0, "y0": y0, "ones": ones, "s": 5 if mode == "BRUTE" else 2,
           "px": _window_pixels(128, x0, y0, W0, H0)}
    gpu.close()


def _batch_reference(ones, s):
    """From one-sample passes [k, w, h, 3] (Placeholder -1 on a miss) and s samples per item: the fp64
    colour sums, hit and miss counts, the magnitude sums, and q, J by the chunk rule with each item's
    colour sum taken in fp64."""
    miss = (ones == -1.0).all(axis=3)
    col = np.where(miss[..., None], 0.0, ones)
    q = np.zeros(ones.shape[1:3])
    for j in range(0, ones.shape[0], s):
        y = _lum(col[j:j + s].sum(axis=0))
        q = q + y * y / float(min(s, ones.shape[0] - j))
    return col.sum(axis=0), (~miss).sum(axis=0), miss.sum(axis=0), np.abs(col).sum(axis=0), q, -(-ones.shape[0] // s)


def test_p4_100_spp_against_the_sum_of_the_single_samples(hundred):
    """Counts exact.  Each channel within (s - 1) * 2^-24 * S + 200 * 2^-53 * S of the fp64 sum of the 100
    single samples, S the sum of their magnitudes.  Derivation: an item's sum is the plain fp32 running
    sum of its s samples' colours (bounce(): L.ar += col.x from 0, so the first add is exact and each of
    the s - 1 others rounds once, by at most 2^-24 of a partial sum that does not exceed the item's
    magnitude sum times 1 + (s - 1) * 2^-24; that second-order factor is the 1 + 2^-20 below); the items
    are exact as doubles, and the fold and the reference each add 100 or fewer terms in fp64, at most
    99 * 2^-53 * S each."""
    gpu, s = hundred["gpu"], hundred["s"]
    win = (slice(hundred["x0"], hundred["x0"] + W0), slice(hundred["y0"], hundred["y0"] + H0))
    want, n_hit, n_miss, mag, _, _ = _batch_reference(hundred["ones"][:100], s)
    got = gpu.render_pixels(hundred["px"], 100, seed=SEED)
    assert np.array_equal(got[1][win], n_hit) and np.array_equal(got[2][win], n_miss)
    assert (n_hit > 0).any() and (n_miss > 0).any()
    err = np.abs(got[0][win] - want)
    bound = ((s - 1) * 2.0 ** -24 * (1 + 2.0 ** -20) + 200 * 2.0 ** -53) * mag
    print(f"P4 {hundred['mode']}: max error / bound {np.max(err / np.maximum(bound, 1e-300)):.3f}, "
          f"max relative error {np.max(err / np.maximum(mag, 1e-300)):.3e}")
    assert (err <= bound).all()
    assert err.any()  # several samples per item: the fp32 partial sums do round


def test_p5_moments(hundred):
    """spp 16, one sample per batch: J = 16 and Q = the sum of the 16 squared luminances.  Every operation
    is the same IEEE fp64 operation on both sides (the products by the three weights, two adds, a square,
    a division by 1, the running sum from zero), so Q is held to 16 * 2^-52 relative: the bound of a
    16-term fp64 sum in any order, above one in the same order.
    spp 100: J = ceil(100 / s); Q within (2 e + e^2) * Qm + 64 * 2^-53 * Qm, where e is P4's relative
    bound of an item's fp32 sums, so of its luminance Y_j (the weights are positive and the colours not
    negative), 2 e + e^2 that of Y_j^2, and Qm the sum of Y_j^2 / t_j taken over the magnitude sums.  A
    second call with sample_base = 100 adds to both: q by one fp64 add, batches by J."""
    gpu, s = hundred["gpu"], hundred["s"]
    win = (slice(hundred["x0"], hundred["x0"] + W0), slice(hundred["y0"], hundred["y0"] + H0))
    px = hundred["px"]
    _, n_hit, n_miss, _, q16, j16 = _batch_reference(hundred["ones"][:16], 1)
    got = gpu.render_pixels(px, 16, seed=SEED, moments=True)
    assert j16 == 16 and (got[5][win] == 16).all() and np.array_equal(got[1][win], n_hit)
    err = np.abs(got[4][win] - q16)
    print(f"P5 {hundred['mode']} spp 16: q equal in bits: {_same_bits(got[4][win], q16)}, max relative error "
          f"{np.max(err / np.maximum(q16, 1e-300)):.3e}")
    assert (err <= 16 * 2.0 ** -52 * q16).all() and q16.any()
    assert not (got[4][win][n_hit == 0]).any()  # an all-miss pixel: luminance 0 in every batch
    for a in (got[4], got[5]):  # nothing outside the list
        rest = a.copy()
        rest[win] = 0
        assert not rest.any()

    ones = hundred["ones"]
    _, _, _, mag, q100, j100 = _batch_reference(ones[:100], s)
    miss = (ones[:100] == -1.0).all(axis=3)
    col = np.where(miss[..., None], 0.0, np.abs(ones[:100]))
    qm = sum(_lum(col[j:j + s].sum(axis=0)) ** 2 / s for j in range(0, 100, s))
    first = gpu.render_pixels(px, 100, seed=SEED, moments=True)
    assert j100 == -(-100 // s) and (first[5][win] == j100).all()
    e = (s - 1) * 2.0 ** -24 * (1 + 2.0 ** -20)
    err = np.abs(first[4][win] - q100)
    bound = (2 * e + e * e + 64 * 2.0 ** -53) * qm
    print(f"P5 {hundred['mode']} spp 100: max error / bound {np.max(err / np.maximum(bound, 1e-300)):.3f}")
    assert (err <= bound).all()
    second = gpu.render_pixels(px, 100, seed=SEED, sample_base=100, moments=True)
    assert not _same_bits(second[4], first[4])
    both = tuple(a.copy() for a in (first[0], first[1], first[2], first[4], first[5]))
    gpu.render_pixels(px, 100, seed=SEED, sample_base=100, moments=True, out=both)
    assert _same_bits(both[3], first[4] + second[4]) and (both[4][win] == 2 * j100).all()
    assert _same_bits(both[0], first[0] + second[0]) and ((both[1] + both[2])[win] == 200).all()
    # the standard error the header defines, from these accumulators: finite, and smaller with more samples
    se1 = rc_se(first[0], first[1], first[2], first[4], first[5])[win]
    se2 = rc_se(both[0], both[1], both[2], both[3], both[4])[win]
    lit = first[1][win] > 50
    assert np.isfinite(se1).all() and np.isfinite(se2).all() and np.median(se2[lit]) < np.median(se1[lit])


def rc_se(*acc):
    import raytracercore_amd as rc

    return rc.pixel_standard_error(*acc)


# ---------------------------------------------------------------- P6: errors and state
def _raw(rc, gpu, px, n, spp, bufs, count=None, null=(), q=None, nb=None):
    p = [px.ctypes.data_as(C.c_void_p), bufs[0].ctypes.data_as(C.POINTER(rc.rt_color)),
         bufs[1].ctypes.data_as(C.POINTER(C.c_uint32)), bufs[2].ctypes.data_as(C.POINTER(C.c_uint32))]
    for k in null:
        p[k] = None
    return gpu.lib.rt_render_pixels(gpu.handle, p[0], n, spp, SEED, 0, p[1], p[2], p[3],
                                    q.ctypes.data_as(C.POINTER(C.c_double)) if q is not None else None,
                                    nb.ctypes.data_as(C.POINTER(C.c_uint32)) if nb is not None else None,
                                    C.byref(count) if count is not None else None)


def _sentinels(W, H):
    return np.full((W, H, 3), 7.5), np.full((W, H), 7, np.uint32), np.full((W, H), 9, np.uint32)


def test_p6_errors_touch_nothing(rc):
    import torch

    W, H = 64, 48
    gpu = _gpu(rc, "plane_sphere", "BRUTE", size=(W, H))
    px = np.arange(8, dtype=np.uint32) * 5
    bufs = _sentinels(W, H)
    q, nb = np.full((W, H), 2.5), np.full((W, H), 3, np.uint32)
    count = C.c_uint64(41)
    assert _raw(rc, gpu, px, 0, 4, bufs, count) == 0
    assert gpu.lib.rt_render_pixels(gpu.handle, None, 0, 1, 0, 0, None, None, None, None, None, None) == 0
    assert gpu.lib.rt_render_pixels_device(gpu.handle, None, 0, 1, 0, 0, None, None, None, None, None, 0, None, None) == 0
    for n, spp, null in ((8, 4, (0,)), (8, 4, (1,)), (8, 4, (2,)), (8, 4, (3,)), (-1, 4, ()), (8, 0, ()), (8, -3, ())):
        assert _raw(rc, gpu, px, n, spp, bufs, count, null) == -1, (n, spp, null)
    assert _raw(rc, gpu, px, 8, 4, bufs, count, q=q) == -1 and _raw(rc, gpu, px, 8, 4, bufs, count, nb=nb) == -1
    outside = px.copy()
    outside[5] = W * H
    assert _raw(rc, gpu, outside, 8, 4, bufs, count, q=q, nb=nb) == -1
    twice = px.copy()
    twice[7] = twice[2]
    assert _raw(rc, gpu, twice, 8, 4, bufs, count, q=q, nb=nb) == -1
    err = C.create_string_buffer(512)
    gpu.lib.rt_last_error(err, 512)
    assert "twice" in err.value.decode() and "entry 7" in err.value.decode()
    gpu2 = _gpu(rc, "bounce", "BVH2", size=(W, H))
    assert _raw(rc, gpu2, px, 8, 4, bufs, count) == -7
    gpu2.lib.rt_last_error(err, 512)
    assert "BVH" in err.value.decode()
    gpu2.close()
    # no camera: a scene made through the C ABI and never given one
    scene = _scene("plane_sphere")
    params = rc.rt_scene_params.from_buffer_copy(scene.params)
    params.width, params.height = W, H
    handle = C.c_void_p()
    prims = (rc.rt_prim * scene.n_prims)(*scene.prims)
    assert gpu.lib.rt_scene_create(C.byref(params), prims, scene.n_prims, 0, C.byref(handle)) == 0
    p = [px.ctypes.data_as(C.c_void_p), bufs[0].ctypes.data_as(C.POINTER(rc.rt_color)),
         bufs[1].ctypes.data_as(C.POINTER(C.c_uint32)), bufs[2].ctypes.data_as(C.POINTER(C.c_uint32))]
    assert gpu.lib.rt_render_pixels(handle, p[0], 8, 4, SEED, 0, p[1], p[2], p[3], None, None, None) == -7
    gpu.lib.rt_scene_destroy(handle)
    want = _sentinels(W, H)
    assert all(_same_bits(a, b) for a, b in zip(bufs, want)) and count.value == 41
    assert (q == 2.5).all() and (nb == 3).all()
    # and the same call with nothing wrong works, adding to the sentinels at the listed pixels only
    assert _raw(rc, gpu, px, 8, 4, bufs, count, q=q, nb=nb) == 0
    x, y = px % W, px // W
    assert ((bufs[1][x, y] - 7) + (bufs[2][x, y] - 9) == 4).all() and count.value > 41 and (nb[x, y] == 7).all()
    bufs[1][x, y] = 7
    bufs[2][x, y] = 9
    assert (bufs[1] == 7).all() and (bufs[2] == 9).all()
    # the device entry skips entries outside the frame: it traces the others, and only them
    lst = np.array([3, W * H, 70, 0xFFFFFFFF, W * H - 1], np.uint32)
    ok = lst[lst < W * H]
    ref = gpu.render_pixels(ok, 4, seed=SEED, moments=True)
    d_px = torch.from_numpy(lst.view(np.int32).copy()).cuda()
    acc = [torch.zeros(sh, dtype=dt, device="cuda") for sh, dt in (((3, H, W), torch.float64), ((H, W), torch.int32),
           ((H, W), torch.int32), ((H, W), torch.float64), ((H, W), torch.int32))]
    d_rays = torch.zeros(1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    gpu.render_pixels_device(d_px.data_ptr(), lst.size, 4, SEED, 0, *[a.data_ptr() for a in acc], d_rays=d_rays.data_ptr())
    torch.cuda.synchronize()
    assert int(d_rays.item()) == ref[3]
    assert _same_bits(acc[0].cpu().numpy().transpose(2, 1, 0), ref[0])
    assert _same_bits(acc[1].cpu().numpy().T.view(np.uint32), ref[1]) and _same_bits(acc[2].cpu().numpy().T.view(np.uint32), ref[2])
    assert _same_bits(acc[3].cpu().numpy().T, ref[4]) and int(acc[4].sum()) == 4 * ok.size
    # the device entry's size bound is rt_render_rays_device's
    h = gpu.handle
    args = (SEED, 0, C.c_void_p(acc[0].data_ptr()), C.c_void_p(acc[1].data_ptr()), C.c_void_p(acc[2].data_ptr()), None, None,
            0, None, None)
    assert gpu.lib.rt_render_pixels_device(h, C.c_void_p(d_px.data_ptr()), 125829120 + 1, 64, *args) == -1
    assert gpu.lib.rt_render_pixels_device(h, C.c_void_p(d_px.data_ptr()), 2 ** 30 + 1, 1, *args) == -1
    gpu.close()


@pytest.mark.parametrize("mode", ["AUTO", "BVH"])
def test_p6_render_pixels_leaves_the_renderer_alone(rc, mode):
    """Before and after render_pixels calls: the counters of rt_scene_get_stats (enabled), the
    rt_kernel_times ring (held by its length: three timed launches before and after), build statistic
    [15] (the scene-specialised kernel's state) and a rt_render_tile_1spp pass are what they were (the
    pattern of test_r6_render_rays_leaves_the_renderer_alone, durations compared to 1e-4 relative)."""
    gpu = _gpu(rc, "bounce", mode, size=(128, 128))
    px = _window_pixels(128, 40, 40, 24, 16)
    before = gpu.render_tile_1spp(40, 40, 24, 16, seed=3, sample_index=2)
    tile = gpu.render_tile(40, 40, 24, 16, 8, seed=3)
    jit = gpu.build_stats()["jit_status"]
    gpu.set_stats(True)
    gpu.render_tile(0, 0, 16, 16, 2, seed=4)
    assert sum(gpu.get_stats().values()) > 0  # (read and zeroed)
    launches = gpu.kernel_times(3)
    with pytest.raises(rc.RtError):
        gpu.kernel_times(4)
    jit_now = gpu.build_stats()["jit_status"]
    gpu.render_pixels(px, 2, seed=SEED)
    gpu.render_pixels(px[:100], 40, seed=SEED, sample_base=5, moments=True)
    with pytest.raises(rc.RtError):
        gpu.kernel_times(4)
    assert np.allclose(gpu.kernel_times(3), launches, rtol=1e-4, atol=0)
    assert sum(gpu.get_stats().values()) == 0
    assert gpu.build_stats()["jit_status"] == jit_now
    gpu.set_stats(False)
    assert _same_bits(gpu.render_tile_1spp(40, 40, 24, 16, seed=3, sample_index=2), before)
    after = gpu.render_tile(40, 40, 24, 16, 8, seed=3)
    assert all(_same_bits(a, b) for a, b in zip(tile[:3], after[:3])) and tile[3] == after[3]
    assert gpu.build_stats()["jit_status"] == jit
    stats = gpu.build_stats()
    got = gpu.render_pixels(px, 8, seed=3)  # with the scene-specialised kernel in use (AUTO): the generic one ran
    assert gpu.build_stats() == stats
    assert _same_bits(got[0][40:64, 40:56], tile[0]) and got[3] == tile[3]
    gpu.close()
