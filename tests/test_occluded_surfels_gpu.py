"""rt_occluded_surfels on the device: any-hit occlusion counts at caller-supplied surface points.

The yardstick everywhere is the per-sample way to the same numbers: surfel_rays
(rt_debug_surfel_rays_device) reports the fp32 ray of every sample and occluded_rays (rt_occluded_rays,
RT_QUERY_FAST) answers each with its entry's t_max; the counts must equal the sum of those answers exactly.
S1: promise 1 in every traversal mode, with both builders and in the three gather modes.  S2: shapes, and
the brute-force kernels' sample blocks.  S3: promise 2 (lists, sample ranges, chunks, streams).  S4:
degenerate input.  S5: two scenes whose answer is known.  S6: errors and what a call leaves alone.  S7:
tools/bake_ao.py --device.  The surfel set: tests/occluded_surfels_cases.py."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from occluded_surfels_cases import BAD, BASE, INF, N, SEED, assert_not_hollow, surfel_set, t_cycle, valid_surfels
from test_occluded_rays_gpu import PLANE_SPHERE
from test_query_rays_gpu import _gpu
from test_render_surfels_gpu import FURNACE
from test_render_surfels_host import COSINE, DIFFUSE, MODES, SPHERE, draws

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _yardstick(gpu, pos, nrm, spp, gather, t_max, sample_base=0, stream_base=BASE):
    """occluded_rays' answer for every reported sample ray, bool [n, spp]."""
    rays = gpu.surfel_rays(pos, nrm, spp, SEED, gather, sample_base=sample_base, stream_base=stream_base)
    assert rays.shape == (len(pos), spp)
    tm = None if t_max is None else np.broadcast_to(np.asarray(t_max, np.float64).reshape(-1, 1), rays.shape)
    return gpu.occluded_rays(rays, None, tm)


def _last_error(lib):
    buf = C.create_string_buffer(512)
    lib.rt_last_error(buf, 512)
    return buf.value.decode()


# ---------------------------------------------------------------- S1: promise 1
S1_CASES = ([("bounce", m, None, (128, 128), DIFFUSE) for m in ("BRUTE", "GROUPED", "BVH")] +
            [("bounce", m, None, (128, 128), g) for m in ("BRUTE", "BVH") for g in (COSINE, SPHERE)] +
            [("mesh41", "BVH", "HOST", None, DIFFUSE), ("mesh41", "BVH", "GPU", None, DIFFUSE),
             ("vn", "BRUTE", None, None, DIFFUSE), ("vn", "BVH", None, None, DIFFUSE), ("die", "GROUPED", None, None, DIFFUSE),
             ("plane_sphere", "BRUTE", None, None, DIFFUSE), ("plane_sphere", "BVH", None, None, DIFFUSE)])


@pytest.mark.parametrize("name,mode,builder,size,gather", S1_CASES)
def test_s1_counts_are_occluded_rays_of_the_reported_rays(rc, name, mode, builder, size, gather):
    """spp 5, t_max cycling over 0.25 / 1 / +inf by entry: occluded equals, exactly, the sum over k of
    occluded_rays(surfel_rays(...)[:, k], t_max), and samples is 5 everywhere.  The yardstick's own answers
    meet the two conditions that keep the comparison from being vacuous."""
    pos, nrm = surfel_set(name)
    gpu = _gpu(rc, name, mode, builder, size=size)
    assert gpu.info().traversal == getattr(rc, "RT_TRAVERSAL_" + mode)
    if builder:
        assert gpu.info().bvh_builder == getattr(rc, "RT_BVH_BUILDER_" + builder)
    tm = t_cycle()
    want = _yardstick(gpu, pos, nrm, 5, gather, tm)
    occ, ns = gpu.occluded_surfels(pos, nrm, 5, SEED, gather, t_max=tm, stream_base=BASE)
    gpu.close()
    assert occ.dtype == ns.dtype == np.uint32 and occ.shape == ns.shape == (N,)
    wrong = np.flatnonzero(occ != want.sum(axis=1))
    assert wrong.size == 0, (wrong[:8], occ[wrong[:8]], want.sum(axis=1)[wrong[:8]])
    assert (ns == 5).all()
    assert not want[BAD].any()
    assert_not_hollow(want[valid_surfels()], f"S1 {name} {mode} {builder} gather {gather}")


# ---------------------------------------------------------------- S2: shapes
@pytest.fixture(scope="module", params=["BRUTE", "BVH"])
def bounce(rc, request):
    """bounce in one traversal mode with the yardstick of the whole set at 130 samples (t_max cycling):
    sample k of entry e does not depend on n or spp, so every smaller shape reads its corner of it."""
    pos, nrm = surfel_set("bounce")
    gpu = _gpu(rc, "bounce", request.param, size=(128, 128))
    want = _yardstick(gpu, pos, nrm, 130, DIFFUSE, t_cycle())
    want.setflags(write=False)
    yield gpu, request.param, want
    gpu.close()


def test_s2_shapes(rc, bounce):
    """n in {1, 63, 64, 65, 200} x spp in {1, 5, 50, 130}: part waves, one wave and a lane more, several
    blocks; one sample, fewer samples than lanes, more than a wave's worth per entry."""
    gpu, mode, want = bounce
    pos, nrm = surfel_set("bounce")
    tm = t_cycle()
    for n in (1, 63, 64, 65, 200):
        for spp in (1, 5, 50, 130):
            occ, ns = gpu.occluded_surfels(pos[:n], nrm[:n], spp, SEED, DIFFUSE, t_max=tm[:n], stream_base=BASE)
            assert np.array_equal(occ, want[:n, :spp].sum(axis=1)), (n, spp)
            assert (ns == spp).all(), (n, spp)
    assert 0 < want.sum() < want.size


def test_s2_few_entries_many_samples(rc, bounce):
    """n = 3 at spp 700: several work units add to one entry."""
    gpu, mode, _ = bounce
    pos, nrm = surfel_set("bounce")
    pos, nrm, tm = pos[20:23], nrm[20:23], np.array([1.0, INF, 0.25])
    want = _yardstick(gpu, pos, nrm, 700, COSINE, tm, stream_base=BASE + 20)
    occ, ns = gpu.occluded_surfels(pos, nrm, 700, SEED, COSINE, t_max=tm, stream_base=BASE + 20)
    assert np.array_equal(occ, want.sum(axis=1)) and (ns == 700).all()
    assert 0 < want.sum() < want.size


@pytest.mark.parametrize("switches", ["BLOCK=1", "BLOCK=7", "BLOCK=50", "BLOCK=1000", "LANES=1", "LANES=64", "LANES=1 BLOCK=7",
                                      "LANES=1 BLOCK=50", "LANES=8 BLOCK=20", "LANES=5", "REFILL=16", "REFILL=64"])
def test_s2_the_work_split_changes_nothing(rc, bounce, switches):
    """The brute-force kernels' unit is (64 / lanes) positions x a block of samples and the BVH kernel
    refills at a threshold, all three the host's choice; the counts do not depend on them.  The planning
    switches RTCORE_OCCLUDED_SURFELS_LANES / _BLOCK / _REFILL set them: a block of 1 (a unit per sample, atomic
    adds), 7 (a short last block), all 50 samples (the position's lanes own its entry: the plain
    read-modify-write); 1 lane per position (a lane walks its surfel's samples alone), 64 (a wave per
    position), 5 (taken as 4); 20 samples over 8 lanes (rounded up to 24); a refill only when 16 or all 64
    lanes wait."""
    gpu, mode, want = bounce
    pos, nrm = surfel_set("bounce")
    names = ["RTCORE_OCCLUDED_SURFELS_" + s.split("=")[0] for s in switches.split()]
    for s, name in zip(switches.split(), names):
        os.environ[name] = s.split("=")[1]
    try:
        out = (np.full(N, 3, np.uint32), np.full(N, 4, np.uint32))
        gpu.occluded_surfels(pos, nrm, 50, SEED, DIFFUSE, t_max=t_cycle(), stream_base=BASE, out=out)
    finally:
        for name in names:
            del os.environ[name]
    assert np.array_equal(out[0], 3 + want[:, :50].sum(axis=1)) and (out[1] == 54).all()


# ---------------------------------------------------------------- S3: promise 2
def _device_call(rc, gpu, surfels, index, t_max, spp, occ0, ns0, n_records=None, pad=16, stream=0, sample_base=0,
                 stream_base=BASE, gather=DIFFUSE):
    """rt_occluded_surfels_device over device copies; the accumulators start as occ0 / ns0 (scalars or
    arrays) between `pad` sentinels.  Returns (occluded, samples) with the pads checked."""
    import torch

    n_records = len(surfels) if n_records is None else n_records
    d_surfels = torch.from_numpy(surfels.view(np.uint8).copy()).cuda()
    d_tm = None if t_max is None else torch.from_numpy(np.ascontiguousarray(t_max, np.float64)).cuda()
    d_index = None if index is None else torch.from_numpy(np.ascontiguousarray(index, np.uint32).view(np.int32)).cuda()
    acc = []
    for start, sentinel in ((occ0, 0x5A5A5A5A), (ns0, 0x3C3C3C3C)):
        a = np.full(pad + n_records + pad, sentinel, np.uint32)
        a[pad:pad + n_records] = start
        acc.append(torch.from_numpy(a.view(np.int32)).cuda())
    torch.cuda.synchronize()
    gpu.occluded_surfels_device(gather, d_surfels, n_records, d_index, n_records if index is None else len(index), d_tm, spp,
                                SEED, sample_base, stream_base, acc[0][pad:], acc[1][pad:], stream=stream)
    torch.cuda.synchronize()
    out = []
    for a, sentinel in zip(acc, (0x5A5A5A5A, 0x3C3C3C3C)):
        h = a.cpu().numpy().view(np.uint32)
        assert (h[:pad] == sentinel).all() and (h[pad + n_records:] == sentinel).all()
        out.append(h[pad:pad + n_records].copy())
    return out


def test_s3_lists(rc, bounce):
    """A reversed and a strided list, a prefix, and more records than entries listed: each listed entry gets
    the identity call's counts, every other entry and the sentinels round the arrays stay as they were.  An
    entry at or past n_records writes nothing."""
    gpu, mode, want = bounce
    pos, nrm = surfel_set("bounce")
    surfels, tm = rc._pack_surfels(pos, nrm), t_cycle()
    counts = want[:, :5].sum(axis=1).astype(np.uint32)
    full = _device_call(rc, gpu, surfels, None, tm, 5, 100, 200)
    assert np.array_equal(full[0], 100 + counts) and (full[1] == 205).all()
    lists = {"reversed": np.arange(N)[::-1], "strided": np.arange(3, N, 7), "prefix": np.arange(70),
             "shuffled third": np.random.default_rng(2).permutation(N)[:N // 3]}
    for what, index in lists.items():
        occ, ns = _device_call(rc, gpu, surfels, index, tm, 5, 100, 200)
        rest = np.setdiff1d(np.arange(N), index)
        assert np.array_equal(occ[index], full[0][index]) and (ns[index] == 205).all(), what
        assert (occ[rest] == 100).all() and (ns[rest] == 200).all(), what
    # fewer records than the arrays hold: entries 150 .. 199, 2^32 - 1 and n_records itself are skipped
    index = np.concatenate([np.arange(140, N), [0xFFFFFFFF, 150], np.arange(5)]).astype(np.uint32)
    occ, ns = _device_call(rc, gpu, surfels[:150], index, tm[:150], 5, 100, 200, n_records=150)
    listed = np.concatenate([np.arange(140, 150), np.arange(5)])
    rest = np.setdiff1d(np.arange(150), listed)
    assert np.array_equal(occ[listed], full[0][listed]) and (ns[listed] == 205).all()
    assert (occ[rest] == 100).all() and (ns[rest] == 200).all()
    # samples may be null
    import torch

    d_surfels = torch.from_numpy(surfels.view(np.uint8).copy()).cuda()
    d_occ = torch.zeros(N, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    gpu.occluded_surfels_device(DIFFUSE, d_surfels, N, None, N, None, 5, SEED, 0, BASE, d_occ)
    torch.cuda.synchronize()
    inf = gpu.occluded_surfels(pos, nrm, 5, SEED, DIFFUSE, stream_base=BASE)[0]
    assert np.array_equal(d_occ.cpu().numpy().view(np.uint32), inf)
    assert np.array_equal(inf, gpu.occluded_surfels(pos, nrm, 5, SEED, DIFFUSE, t_max=INF, stream_base=BASE)[0])
    assert (inf >= counts).all() and (inf > counts).any()  # a longer segment hides no less


def test_s3_sample_ranges_add_up(rc, bounce):
    """Samples 0 .. 4 and 5 .. 9 into one pair of accumulators equal one call at spp 10."""
    gpu, mode, want = bounce
    pos, nrm = surfel_set("bounce")
    tm = t_cycle()
    out = (np.zeros(N, np.uint32), np.zeros(N, np.uint32))
    gpu.occluded_surfels(pos, nrm, 5, SEED, DIFFUSE, t_max=tm, sample_base=0, stream_base=BASE, out=out)
    first = out[0].copy()
    gpu.occluded_surfels(pos, nrm, 5, SEED, DIFFUSE, t_max=tm, sample_base=5, stream_base=BASE, out=out)
    one = gpu.occluded_surfels(pos, nrm, 10, SEED, DIFFUSE, t_max=tm, stream_base=BASE)
    assert np.array_equal(out[0], one[0]) and np.array_equal(out[1], one[1]) and (one[1] == 10).all()
    assert np.array_equal(one[0], want[:, :10].sum(axis=1)) and np.array_equal(first, want[:, :5].sum(axis=1))
    assert (out[0] != 2 * first).any()  # (the second five are not the first five again)


def test_s3_chunks_and_streams(rc, bounce):
    """The host entry cut into chunks of 64 surfels (RTCORE_QUERY_CHUNK) equals the one-chunk call; the
    device entry on a torch side stream equals the host entry."""
    import torch

    gpu, mode, want = bounce
    pos, nrm = surfel_set("bounce")
    tm = t_cycle()
    full = gpu.occluded_surfels(pos, nrm, 7, SEED, SPHERE, t_max=tm, stream_base=BASE)
    assert 0 < full[0].sum() < 7 * N and (full[1] == 7).all()
    os.environ["RTCORE_QUERY_CHUNK"] = "64"
    try:
        cut = gpu.occluded_surfels(pos, nrm, 7, SEED, SPHERE, t_max=tm, stream_base=BASE)
        cut_inf = gpu.occluded_surfels(pos, nrm, 7, SEED, SPHERE, stream_base=BASE)
    finally:
        del os.environ["RTCORE_QUERY_CHUNK"]
    assert np.array_equal(cut[0], full[0]) and np.array_equal(cut[1], full[1])
    assert np.array_equal(cut_inf[0], gpu.occluded_surfels(pos, nrm, 7, SEED, SPHERE, stream_base=BASE)[0])
    side = torch.cuda.Stream()
    occ, ns = _device_call(rc, gpu, rc._pack_surfels(pos, nrm), None, tm, 7, 0, 0, stream=side.cuda_stream, gather=SPHERE)
    assert np.array_equal(occ, full[0]) and np.array_equal(ns, full[1])
    # an entry's counts do not depend on where the call starts: the tail of the set, keyed as in the whole
    tail = gpu.occluded_surfels(pos[37:], nrm[37:], 7, SEED, SPHERE, t_max=tm[37:], stream_base=BASE + 37)
    assert np.array_equal(tail[0], full[0][37:])


# ---------------------------------------------------------------- S4: degenerate input
@pytest.mark.parametrize("mode", ["BRUTE", "GROUPED", "BVH"])
def test_s4_degenerate_surfels_and_segments(rc, mode):
    """The three invalid surfels give occluded 0 and samples += spp; t_max NaN, 0, -1, -0.0 and 1e-60 give 0;
    +inf is valid; the entries around them are answered as if they were not there."""
    pos, nrm = surfel_set("bounce")
    gpu = _gpu(rc, "bounce", mode, size=(128, 128))
    good_pos = pos.copy()
    good_nrm = nrm.copy()
    good_pos[BAD[0]] = pos[BAD[0] + 1]
    good_nrm[BAD[1]] = nrm[BAD[1] + 1]
    good_nrm[BAD[2]] = nrm[BAD[2] + 1]
    tm = np.full(N, INF)
    ref = gpu.occluded_surfels(good_pos, good_nrm, 6, SEED, COSINE, t_max=tm, stream_base=BASE)[0]
    bad_t = {5: np.nan, 20: 0.0, 33: -1.0, 40: -0.0, 66: 1e-60, 190: -INF}
    for i, v in bad_t.items():
        tm[i] = v
    out = (np.full(N, 9, np.uint32), np.full(N, 2, np.uint32))
    gpu.occluded_surfels(pos, nrm, 6, SEED, COSINE, t_max=tm, stream_base=BASE, out=out)
    gpu.close()
    bad = BAD + list(bad_t)
    keep = np.setdiff1d(np.arange(N), bad)
    assert (out[0][bad] == 9).all() and (out[1] == 8).all()
    assert np.array_equal(out[0][keep], 9 + ref[keep])
    assert ref[bad].any() and ref[keep].any() and (ref[keep] < 6).any()  # some of them were occluded before


# ---------------------------------------------------------------- S5: known answers
@pytest.mark.parametrize("mode", ["BRUTE", "BVH"])
def test_s5_inside_a_closed_box(rc, mode):
    """In the middle of the closed emitting sphere of radius 5 every sample is occluded at t_max = +inf and
    none at a t_max below the distance to the wall, in all three gather modes."""
    scene = rc.SceneLoader.from_text(FURNACE)
    gpu = rc.GpuRaytracer(scene, 0, traversal=getattr(rc, "RT_TRAVERSAL_" + mode))
    rng = np.random.default_rng(3)
    pos = rng.uniform(-1.0, 1.0, (70, 3))  # within sqrt 3 of the centre: the wall is more than 3.2 away
    nrm = rng.normal(size=(70, 3))
    for gather in MODES:
        occ, ns = gpu.occluded_surfels(pos, nrm, 32, SEED, gather, stream_base=5)
        assert (occ == 32).all() and (ns == 32).all(), gather
        occ, ns = gpu.occluded_surfels(pos, nrm, 32, SEED, gather, t_max=3.2, stream_base=5)
        assert not occ.any() and (ns == 32).all(), gather
    gpu.close()


PLANE = "size 16 12\nambient color .2 .3 .4\ncamera 0 -4 3, 0 0 0, 0 0 1, 60\ndiffuse .5 .5 .5\nplane 0 0 0 1\n"


@pytest.mark.parametrize("mode", ["BRUTE", "BVH"])
def test_s5_sphere_mode_over_a_plane(rc, mode):
    """One plane z = 0 and a surfel at (0, 0, 1) with normal (0, 0, 1), SPHERE mode, t_max = 2: a sample is
    occluded exactly when its direction's z = 1 - 2 U1 is below -1/2, so the count is #{k: U1_k > 0.75} from
    the oracle's draws; the claim is skipped only for draws within 1e-5 of 0.75, of which there is at most one."""
    u1, _ = draws(SEED, [77], range(256))
    u1 = u1[0]
    near = np.abs(u1 - 0.75) <= 1e-5
    assert near.sum() <= 1
    sure = int(((u1 > 0.75) & ~near).sum())
    assert 32 <= sure <= 96  # (a quarter of 256, give or take)
    gpu = rc.GpuRaytracer(rc.SceneLoader.from_text(PLANE), 0, traversal=getattr(rc, "RT_TRAVERSAL_" + mode))
    occ, ns = gpu.occluded_surfels([[0.0, 0.0, 1.0]], [[0.0, 0.0, 1.0]], 256, SEED, SPHERE, t_max=2.0, stream_base=77)
    free = gpu.occluded_surfels([[0.0, 0.0, 1.0]], [[0.0, 0.0, 1.0]], 256, SEED, SPHERE, t_max=0.99, stream_base=77)[0]
    gpu.close()
    assert ns[0] == 256 and sure <= occ[0] <= sure + int(near.sum())
    assert free[0] == 0  # (the plane is 1 away)


# ---------------------------------------------------------------- S6: manners
def test_s6_state_error_on_a_bvh2_scene(rc):
    pos, nrm = surfel_set("bounce")
    surfels = rc._pack_surfels(pos[20:24], nrm[20:24])
    occ, ns = np.full(4, 0xAB, np.uint32), np.full(4, 0xCD, np.uint32)
    ps, po, pn = surfels.ctypes.data_as(C.c_void_p), occ.ctypes.data_as(C.POINTER(C.c_uint32)), ns.ctypes.data_as(C.POINTER(C.c_uint32))
    gpu = _gpu(rc, "bounce", "BVH2")
    assert gpu.lib.rt_occluded_surfels(gpu.handle, 1, ps, 4, None, 4, SEED, 0, 0, po, pn) == -7
    msg = _last_error(gpu.lib)
    rays, hits = np.zeros(4, rc.RAY_DTYPE), np.zeros(4, rc.HIT_DTYPE)
    assert gpu.lib.rt_query_rays(gpu.handle, rc.RT_QUERY_FAST, rays.ctypes.data_as(C.c_void_p), 4, hits.ctypes.data_as(C.c_void_p)) == -7
    assert msg == _last_error(gpu.lib).replace("rt_query_rays", "rt_occluded_surfels") and "BVH2" in msg
    assert gpu.lib.rt_occluded_surfels_device(gpu.handle, 1, C.c_void_p(64), 4, None, 4, None, 4, SEED, 0, 0, C.c_void_p(64), None,
                                              None) == -7
    assert gpu.lib.rt_occluded_surfels(gpu.handle, 5, ps, 4, None, 4, SEED, 0, 0, po, pn) == -1  # the mode comes first
    assert gpu.lib.rt_occluded_surfels(gpu.handle, 1, None, 0, None, 4, SEED, 0, 0, None, None) == 0
    gpu.close()
    assert (occ == 0xAB).all() and (ns == 0xCD).all()


def test_s6_a_call_leaves_the_renderer_alone(rc):
    """A render after occlusion calls equals the same render before them bit for bit; the counters of
    rt_scene_get_stats and the rt_kernel_times ring are what they were."""
    pos, nrm = surfel_set("bounce")
    gpu = _gpu(rc, "bounce", "BVH", size=(128, 128))
    before = gpu.render_tile(40, 40, 24, 16, 8, seed=3)
    gpu.render_tile(0, 0, 16, 16, 2, seed=4)
    times = gpu.kernel_times(2)
    gpu.set_stats(True)
    gpu.render_tile(0, 0, 16, 16, 2, seed=4)
    assert sum(gpu.get_stats().values()) > 0  # (read and zeroed)
    launches = gpu.kernel_times(3)
    stats = gpu.build_stats()
    for gather in MODES:
        for tm in (None, 1.0):
            assert gpu.occluded_surfels(pos, nrm, 9, SEED, gather, t_max=tm)[1].sum() == 9 * N
    assert gpu.kernel_times(3) == launches
    assert sum(gpu.get_stats().values()) == 0
    assert gpu.build_stats() == stats
    gpu.set_stats(False)
    assert launches[:2] == times
    after = gpu.render_tile(40, 40, 24, 16, 8, seed=3)
    for a, b in zip(before[:3], after[:3]):
        assert np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()
    assert before[3] == after[3]
    gpu.close()


# ---------------------------------------------------------------- S7: the tool
def test_s7_bake_ao_device_equals_the_per_ray_image(rc):
    """tools/bake_ao.py's bake_ao_device on bounce at width 64, K = 8, R = 1: value for value 1 - counts / K
    of occluded_rays for surfel_rays of the same surfels; neither all 0 nor all 1."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import bake_ao
    finally:
        sys.path.pop(0)
    gpu = _gpu(rc, "bounce", size=(64, 48))
    ao = bake_ao.bake_ao_device(gpu, 8, 1.0, seed=5)
    hits = gpu.query_rays(gpu.camera_rays())  # [x, y]
    mask, pos, nrm = bake_ao.ao_surfels(hits)
    rays = gpu.surfel_rays(pos, nrm, 8, 5, COSINE)
    counts = gpu.occluded_rays(rays, None, 1.0).sum(axis=1)
    gpu.close()
    ref = np.ones(hits.shape, np.float32)
    ref[mask] = (1.0 - counts / 8.0).astype(np.float32)
    assert ao.shape == (48, 64) and ao.dtype == np.float32
    assert np.array_equal(ao, ref.T)
    assert (ao[~mask.T] == 1).all() and (~mask).any()
    assert ao.min() >= 0 and ao.max() == 1 and 0 < (ao < 1).sum() < ao.size
    assert np.array_equal(ao * 8, np.rint(ao * 8))  # multiples of 1 / K
