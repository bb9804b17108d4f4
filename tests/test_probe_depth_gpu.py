"""Probe depth maps on the device: the bake against the fold's host twin over the reported rays and the query's
answers (G1, promise 1); a probe's result alone, in sub-ranges called in any order, on a side stream and chunked
(G2, promise 2); a + b samples (G3, promise 3); a probe at the centre of a sphere (G4); the shading against its
twin (G5, promise 1), a point's result alone and the tie to rt_shade_probes_device (G6, promises 2 and 3); the
device pipeline bake -> close -> shade (G7); errors and empty calls (G8); the existing shading and the renderer
left alone (G9).  The replay is tests/probe_depth_cases.py's."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from probe_depth_cases import replay_corner, same_bits
from test_query_rays_gpu import _gpu
from test_render_surfels_gpu import _last_error, _surfels
from test_render_surfels_host import SPHERE
from test_shade_probes_gpu import DIMS, _scene_grid
from test_shade_probes_host import BAD, N, n_probes, random_L

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED, STREAM_BASE, SAMPLE_BASE = 13, 1000, 3


def _bake(rc, gpu, pos, nrm, spp, params, sample_base=SAMPLE_BASE, stream_base=STREAM_BASE, stream=None, acc=None, sentinels=True):
    """rt_render_probe_depth_device over torch tensors, added into acc = (d_depth, d_counts) (new zeroed ones for
    None, with sentinels behind each, checked unless told otherwise); (depth (n, 3, 64), counts (n, 4) uint32, acc)."""
    import torch

    n = len(pos)
    d_probes = torch.from_numpy(rc._pack_surfels(pos, nrm).view(np.uint8).copy()).cuda()
    if acc is None:
        acc = (torch.zeros(n * 192 + 8, dtype=torch.float64, device="cuda"), torch.zeros(n * 4 + 8, dtype=torch.int32, device="cuda"))
        acc[0][n * 192:] = 2.5
        acc[1][n * 4:] = 77
    torch.cuda.synchronize()
    gpu.render_probe_depth_device(d_probes, n, spp, SEED, sample_base, stream_base, params, acc[0], acc[1],
                                  stream=stream.cuda_stream if stream is not None else 0)
    if stream is not None:
        stream.synchronize()
    torch.cuda.synchronize()
    depth, counts = acc[0].cpu().numpy(), acc[1].cpu().numpy()
    assert not sentinels or ((depth[n * 192:] == 2.5).all() and (counts[n * 4:] == 77).all())
    return depth[:n * 192].reshape(n, 3, 64), counts[:n * 4].reshape(n, 4).view(np.uint32), acc


def _samples(gpu, pos, nrm, spp, sample_base=SAMPLE_BASE, stream_base=STREAM_BASE):
    """The rays rt_debug_surfel_rays_device reports and rt_query_rays' RT_QUERY_FAST answers for them, (n, spp)."""
    rays = gpu.surfel_rays(pos, nrm, spp, SEED, SPHERE, sample_base=sample_base, stream_base=stream_base)
    return rays, gpu.query_rays(rays)


# ---------------------------------------------------------------- G1: promise 1
@pytest.mark.parametrize("name,mode", [("bounce", "BRUTE"), ("bounce", "BVH"), ("die", "GROUPED")])
def test_g1_bake_is_the_twin_over_the_reported_rays_and_the_querys_answers(rc, name, mode):
    """n = 1, 5, 63, 65 (a wave, a block of four waves and one past it) x spp = 1, 63, 64, 65, 130, an invalid
    probe in every case but the first; d_max is the median hit distance, so half the hits are held to it."""
    pos, nrm = _surfels(name)
    assert BAD[0] == 7 and BAD[2] == 64
    gpu = _gpu(rc, name, mode)
    rays, hits = _samples(gpu, pos[:65], nrm[:65], 130)
    hit = hits["prim_id"] >= 0
    d_max = float(np.median(hits["distance"][hit]))
    seen = np.zeros(4, np.int64)
    for sharpness in (5, 0):
        P = rc.probe_depth_params(d_max, sharpness)
        for n, first in ((1, 0), (1, 7), (5, 3), (63, 0), (65, 0)):
            for spp in (1, 63, 64, 65, 130) if sharpness else (65,):
                sl = slice(first, first + n)
                depth, counts, _ = _bake(rc, gpu, pos[sl], nrm[sl], spp, P, stream_base=STREAM_BASE + first)
                # (sample k of a probe is the same ray whatever spp is: the first spp columns of the 130)
                want_d, want_c = rc.probe_depth_fold_host(P, rays[sl, :spp], hits[sl, :spp])
                assert same_bits(depth, want_d) and same_bits(counts, want_c), (sharpness, n, first, spp)
                bad = [i - first for i in (7, 64) if first <= i < first + n]
                assert (counts[bad] == [0, 0, 0, spp]).all() and not depth[bad].any()
                assert (counts[:, 0] + counts[:, 2] + counts[:, 3] == spp).all() and (counts[:, 1] <= counts[:, 0]).all()
                seen += counts.sum(axis=0).astype(np.int64)
    gpu.close()
    print(f"G1 {name} {mode}: d_max {d_max:.4g}, hits {seen[0]}, inside {seen[1]}, misses {seen[2]}, skipped {seen[3]}, "
          f"{int((hits['distance'][hit] > d_max).sum())} of {int(hit.sum())} hits past d_max")
    assert seen[0] > 0 and seen[3] > 0 and np.isfinite(d_max) and d_max > 0


# ---------------------------------------------------------------- G2: promise 2
@pytest.fixture(scope="module")
def bounce_bvh(rc):
    gpu = _gpu(rc, "bounce", "BVH", size=(128, 128))
    yield gpu
    gpu.close()


G2_N, G2_SPP, G2_DMAX = 65, 70, 1.5


@pytest.fixture(scope="module")
def bake_case(rc, bounce_bvh):
    pos, nrm = _surfels("bounce")
    P = rc.probe_depth_params(G2_DMAX, 5)
    depth, counts, _ = _bake(rc, bounce_bvh, pos[:G2_N], nrm[:G2_N], G2_SPP, P)
    return pos[:G2_N], nrm[:G2_N], P, depth, counts


def test_g2_a_probes_result_does_not_depend_on_its_place(rc, bounce_bvh, bake_case):
    import torch

    pos, nrm, P, depth, counts = bake_case
    for i in (0, 7, 63, 64):
        d1, c1, _ = _bake(rc, bounce_bvh, pos[i:i + 1], nrm[i:i + 1], G2_SPP, P, stream_base=STREAM_BASE + i)
        assert same_bits(d1[0], depth[i]) and same_bits(c1[0], counts[i]), i
    # sub-ranges called in a shuffled order into slices of one pair of arrays
    whole = (torch.zeros(G2_N * 192 + 8, dtype=torch.float64, device="cuda"), torch.zeros(G2_N * 4 + 8, dtype=torch.int32, device="cuda"))
    whole[0][G2_N * 192:] = 2.5
    whole[1][G2_N * 4:] = 77
    cuts = [0, 1, 6, 40, 64, 65]
    for k in np.random.default_rng(4).permutation(len(cuts) - 1):
        a, b = cuts[k], cuts[k + 1]
        _bake(rc, bounce_bvh, pos[a:b], nrm[a:b], G2_SPP, P, stream_base=STREAM_BASE + a, acc=(whole[0][a * 192:], whole[1][a * 4:]),
              sentinels=False)
    got_d, got_c = whole[0].cpu().numpy(), whole[1].cpu().numpy()
    assert (got_d[G2_N * 192:] == 2.5).all() and (got_c[G2_N * 4:] == 77).all()
    assert same_bits(got_d[:G2_N * 192].reshape(G2_N, 3, 64), depth) and same_bits(got_c[:G2_N * 4].reshape(G2_N, 4).view(np.uint32), counts)
    assert len(np.unique(counts[:, 0])) > 3 and counts[:, 2].sum() + counts[:, 0].sum() == (G2_N - 2) * G2_SPP


def test_g2_a_side_stream_gives_the_same_bits(rc, bounce_bvh, bake_case):
    import torch

    pos, nrm, P, depth, counts = bake_case
    d1, c1, _ = _bake(rc, bounce_bvh, pos, nrm, G2_SPP, P, stream=torch.cuda.Stream())
    assert same_bits(d1, depth) and same_bits(c1, counts)


CHILD = """
import sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import raytracercore_amd as rc
from test_query_rays_gpu import _gpu
from test_probe_depth_gpu import _bake, G2_SPP, G2_DMAX
z = np.load(sys.argv[2])
gpu = _gpu(rc, "bounce", "BVH", size=(128, 128))
P = rc.probe_depth_params(G2_DMAX, 5)
d70, c70, _ = _bake(rc, gpu, z["pos"], z["nrm"], G2_SPP, P)
d5, c5, _ = _bake(rc, gpu, z["pos"], z["nrm"], 5, P)
gpu.close()
np.savez(sys.argv[3], d70=d70, c70=c70, d5=d5, c5=c5)
"""


def test_g2_chunks(rc, bounce_bvh, bake_case, tmp_path):
    """RTCORE_QUERY_CHUNK = 96 samples, set for a fresh child process: at 70 spp a chunk is one probe, at 5 spp it
    is 19; both are the one-chunk call bit for bit."""
    pos, nrm, P, depth, counts = bake_case
    d5, c5, _ = _bake(rc, bounce_bvh, pos, nrm, 5, P)
    np.savez(tmp_path / "case.npz", pos=pos, nrm=nrm)
    env = dict(os.environ, RTCORE_QUERY_CHUNK="96")
    subprocess.run([sys.executable, "-c", CHILD, ROOT, str(tmp_path / "case.npz"), str(tmp_path / "out.npz")],
                   check=True, env=env, timeout=300)
    z = np.load(tmp_path / "out.npz")
    assert same_bits(z["d70"], depth) and same_bits(z["c70"], counts)
    assert same_bits(z["d5"], d5) and same_bits(z["c5"], c5)


# ---------------------------------------------------------------- G3: promise 3
def test_g3_64_and_66_samples_are_130(rc, bounce_bvh):
    pos, nrm = _surfels("bounce")
    P = rc.probe_depth_params(G2_DMAX, 5)
    whole = _bake(rc, bounce_bvh, pos[:9], nrm[:9], 130, P)
    first = _bake(rc, bounce_bvh, pos[:9], nrm[:9], 64, P)
    both = _bake(rc, bounce_bvh, pos[:9], nrm[:9], 66, P, sample_base=SAMPLE_BASE + 64, acc=first[2])
    assert same_bits(both[0], whole[0]) and same_bits(both[1], whole[1])
    assert not same_bits(first[0], whole[0]) and (whole[1][7] == [0, 0, 0, 130]).all()


# ---------------------------------------------------------------- G4: a sphere round the probe
UNIT_SPHERE = "size 16 12\ncamera 0 -4 0, 0 0 0, 0 0 1, 60\ntwosided true\ndiffuse .5 .5 .5\nspecular 0 0 0\nsphere 0 0 0 1\n"


def test_g4_a_probe_at_the_centre_of_a_unit_sphere(rc):
    """One two-sided unit sphere, the probe at its centre, d_max = 4, 64 samples.  Every sample hits at distance 1
    from inside, so every texel has mu = 1 and no variance, to the fast hit's distance error: the project's bar
    on it is 1e-4 (tests/test_hit_records_gpu.py; measured 3.6e-6), which bounds |mu - 1| directly and
    m2 - mu^2 by about 2e-4 + 1e-8, under the 1e-3 asked.  Shading: a point at distance 0.5 is nearer than every
    mean (W = 1); a point at distance 2 gets the Chebyshev weight, computed here from the baked D by the replay."""
    import torch

    gpu = rc.GpuRaytracer(rc.SceneLoader.from_text(UNIT_SPHERE), 0)
    acc = gpu.render_probe_depth(np.zeros((1, 3)), 64, SEED, 4.0, sharpness=5)
    counts = acc["counts"].cpu().numpy().view(np.uint32)
    D = acc["D"].cpu().numpy()
    assert isinstance(acc["D"], torch.Tensor) and acc["D"].is_cuda and D.shape == (1, 64, 2)
    print(f"G4: counts {counts[0].tolist()}, |mu - 1| max {np.abs(D[0, :, 0] - 1).max():.3g}, "
          f"m2 - mu^2 in [{(D[0, :, 1] - D[0, :, 0] ** 2).min():.3g}, {(D[0, :, 1] - D[0, :, 0] ** 2).max():.3g}]")
    assert counts[0].tolist() == [64, 64, 0, 0] and rc.probe_backface_share(counts)[0] == 1.0
    assert np.isfinite(D).all()
    assert np.abs(D[0, :, 0] - 1).max() < 1e-4 and (np.abs(D[0, :, 1] - D[0, :, 0] ** 2) < 1e-3).all()
    grid = rc.probe_grid((0, 0, 0), (1, 1, 1), (1, 1, 1), False, 0.0)
    L = random_L((1, 1, 1), seed=12)
    u = np.random.default_rng(3).normal(size=(32, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    f = 1e-2
    P = rc.probe_depth_params(4.0, 5, f)
    E_near, W_near = gpu.shade_probes_depth(grid, L, acc["D"], P, 0.5 * u, u)
    E_far, W_far = gpu.shade_probes_depth(grid, L, D, P, 2.0 * u, u)
    gpu.close()
    assert (W_near == 1.0).all() and E_near.any()
    want = np.array([replay_corner(4.0, f, False, D[0], [float(x) for x in 2.0 * row], [float(x) for x in row])[0] for row in u])
    print(f"G4: W at distance 2 in [{W_far.min():.6g}, {W_far.max():.6g}], (f / (f + 1))^3 = {(f / (f + 1)) ** 3:.6g}")
    assert np.abs(W_far / want - 1).max() < 1e-3
    assert np.abs(want / (f / (f + 1)) ** 3 - 1).max() < 1e-3  # (delta = 2 - mu is 1 to 1e-4: c moves by 6e-4 at the most)


# ---------------------------------------------------------------- G5 .. G7: the shading
@pytest.fixture(scope="module")
def shade_case(rc, bounce_bvh):
    """A 4 x 3 x 2 grid over the room, its depth maps baked at 64 spp, random L with an absent probe, and the 200
    points of the surfel tests tiled to 257."""
    grid = _scene_grid(rc, "bounce", visibility=False)
    iz, iy, ix = np.meshgrid(*(np.arange(d) for d in DIMS[::-1]), indexing="ij")
    probe_pos = np.array(grid.origin) + np.stack([ix, iy, iz], axis=-1).reshape(-1, 3) * np.array(grid.step)
    d_max = float(2 * np.linalg.norm(np.array(grid.step)))
    acc = bounce_bvh.render_probe_depth(probe_pos, 64, SEED, d_max)
    L = random_L(DIMS, seed=17, absent=(5,))
    pos, nrm = _surfels("bounce")
    pos, nrm = np.concatenate([pos, pos[:57] + 0.01]), np.concatenate([nrm, nrm[:57]])
    return grid, probe_pos, d_max, acc, L, pos, nrm


@pytest.mark.parametrize("wrap", [False, True])
def test_g5_shading_is_the_twin(rc, bounce_bvh, shade_case, wrap):
    grid, _, d_max, acc, L, pos, nrm = shade_case
    D = acc["D"].cpu().numpy()
    P = rc.probe_depth_params(d_max, 5, 1e-3, wrap)
    for n in (1, 255, 257):
        E, W = bounce_bvh.shade_probes_depth(grid, L, acc["D"], P, pos[:n], nrm[:n])
        want_E, want_W = rc.shade_probes_depth_host(grid, L, D, P, pos[:n], nrm[:n])
        assert same_bits(E, want_E) and same_bits(W, want_W), n
    flat = rc.shade_probes_host(grid, L, pos, nrm)
    lower = (W < flat[1]).sum()
    print(f"G5 wrap={wrap}: {int((W > 0).sum())} of {len(W)} points lit, {int(lower)} with a weight below the plain blend's, "
          f"{int(np.isnan(D[:, :, 0]).sum())} of {D[:, :, 0].size} texels absent")
    assert not E[BAD].any() and not W[BAD].any() and E.any() and lower > 0


def test_g6_a_points_result_alone_and_the_tie_to_shade_probes(rc, bounce_bvh, shade_case):
    import torch

    grid, _, d_max, acc, L, pos, nrm = shade_case
    P = rc.probe_depth_params(d_max, 5, 1e-3, True)
    E, W = bounce_bvh.shade_probes_depth(grid, L, acc["D"], P, pos, nrm)
    for i in (0, 63, 64, 199, 256):
        E1, W1 = bounce_bvh.shade_probes_depth(grid, L, acc["D"], P, pos[i:i + 1], nrm[i:i + 1])
        assert same_bits(E1[0], E[i]) and W1[0] == W[i], i
    order = np.random.default_rng(4).permutation(len(pos))
    E2, W2 = bounce_bvh.shade_probes_depth(grid, L, acc["D"], P, pos[order], nrm[order])
    assert same_bits(E2, E[order]) and same_bits(W2, W[order])
    # a side stream, sentinels round the outputs, and no weight array
    n, pad = len(pos), 16
    d_L = torch.from_numpy(L.reshape(-1).copy()).cuda()
    d_pts = torch.from_numpy(rc._pack_surfels(pos, nrm).view(np.uint8).copy()).cuda()
    d_E = torch.full((pad + 3 * n + pad,), 2.5, dtype=torch.float64, device="cuda")
    d_W = torch.full((pad + n + pad,), 3.5, dtype=torch.float64, device="cuda")
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    rc.shade_probes_depth_device(grid, P, d_L, acc["D"], d_pts, n, d_E[pad:], d_W[pad:], stream=side.cuda_stream)
    side.synchronize()
    got_E, got_W = d_E.cpu().numpy(), d_W.cpu().numpy()
    assert same_bits(got_E[pad:-pad].reshape(n, 3), E) and same_bits(got_W[pad:-pad], W)
    assert (got_E[:pad] == 2.5).all() and (got_E[-pad:] == 2.5).all() and (got_W[:pad] == 3.5).all() and (got_W[-pad:] == 3.5).all()
    d_W[:] = 3.5
    rc.shade_probes_depth_device(grid, P, d_L, acc["D"], d_pts, n, d_E[pad:], 0)
    torch.cuda.synchronize()
    assert same_bits(d_E.cpu().numpy()[pad:-pad].reshape(n, 3), E) and (d_W.cpu().numpy() == 3.5).all()
    # promise 3: every texel absent, no wrap: rt_shade_probes_device without the visibility flag, bit for bit
    absent = torch.full((n_probes(DIMS), 64, 2), float("nan"), dtype=torch.float64, device="cuda")
    E3, W3 = bounce_bvh.shade_probes_depth(grid, L, absent, rc.probe_depth_params(d_max, 5, 1e-3), pos, nrm)
    want = bounce_bvh.shade_probes(grid, L, pos, nrm)
    assert same_bits(E3, want[0]) and same_bits(W3, want[1]) and not same_bits(W3, W)


def test_g7_device_pipeline_bake_close_shade(rc, bounce_bvh, shade_case):
    """Bake, close and shade with nothing leaving the device until the result, against the three host twins fed
    with the reported rays and the query's answers."""
    import torch

    grid, probe_pos, d_max, _, L, pos, nrm = shade_case
    n_p, spp, n = n_probes(DIMS), 33, N
    probe_nrm = np.tile([0.0, 0.0, 1.0], (n_p, 1))
    P = rc.probe_depth_params(d_max, 3, 1e-3, True)
    rays, hits = _samples(bounce_bvh, probe_pos, probe_nrm, spp, 0, 0)
    want_depth, want_counts = rc.probe_depth_fold_host(P, rays, hits)
    want_D = rc.probe_depth_close_host(want_depth)
    want_E, want_W = rc.shade_probes_depth_host(grid, L, want_D, P, pos[:n], nrm[:n])
    d_probes = torch.from_numpy(rc._pack_surfels(probe_pos, probe_nrm).view(np.uint8).copy()).cuda()
    d_depth = torch.zeros((n_p, 3, 64), dtype=torch.float64, device="cuda")
    d_counts = torch.zeros((n_p, 4), dtype=torch.int32, device="cuda")
    d_D = torch.full((n_p * 128 + 8,), 2.5, dtype=torch.float64, device="cuda")
    d_L = torch.from_numpy(L.reshape(-1).copy()).cuda()
    d_pts = torch.from_numpy(rc._pack_surfels(pos[:n], nrm[:n]).view(np.uint8).copy()).cuda()
    d_E = torch.full((3 * n,), 2.5, dtype=torch.float64, device="cuda")
    d_W = torch.full((n,), 2.5, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    bounce_bvh.render_probe_depth_device(d_probes, n_p, spp, SEED, 0, 0, P, d_depth, d_counts)
    rc.probe_depth_close_device(d_depth, n_p, d_D)
    rc.shade_probes_depth_device(grid, P, d_L, d_D, d_pts, n, d_E, d_W)
    torch.cuda.synchronize()
    got_D = d_D.cpu().numpy()
    assert same_bits(d_depth.cpu().numpy(), want_depth) and same_bits(d_counts.cpu().numpy().view(np.uint32), want_counts)
    assert same_bits(got_D[:n_p * 128].reshape(n_p, 64, 2), want_D) and (got_D[n_p * 128:] == 2.5).all()
    assert same_bits(d_E.cpu().numpy().reshape(n, 3), want_E) and same_bits(d_W.cpu().numpy(), want_W)
    assert (want_W > 0).sum() > n // 2 and (want_counts[:, 0] > 0).all()
    # a texel without weight is absent on the device as on the host
    d_depth[2, 0, 11] = 0.0
    rc.probe_depth_close_device(d_depth, n_p, d_D)
    torch.cuda.synchronize()
    want_depth[2, 0, 11] = 0.0
    got = d_D.cpu().numpy()[:n_p * 128].reshape(n_p, 64, 2)
    assert np.isnan(got[2, 11]).all() and same_bits(got, rc.probe_depth_close_host(want_depth))


# ---------------------------------------------------------------- G8: plumbing
def test_g8_empty_calls_and_errors_touch_nothing(rc, bounce_bvh, shade_case):
    import torch

    grid, probe_pos, d_max, acc, L, pos, nrm = shade_case
    lib, h = bounce_bvh.lib, bounce_bvh.handle
    P = rc.probe_depth_params(d_max, 5)
    d_probes = torch.from_numpy(rc._pack_surfels(pos[20:28], nrm[20:28]).view(np.uint8).copy()).cuda()
    d_depth = torch.full((8 * 192,), 2.5, dtype=torch.float64, device="cuda")
    d_counts = torch.full((8 * 4,), 77, dtype=torch.int32, device="cuda")
    d_L = torch.from_numpy(L.reshape(-1).copy()).cuda()
    d_E = torch.full((24,), 2.5, dtype=torch.float64, device="cuda")
    d_W = torch.full((8,), 2.5, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    p = lambda t: C.c_void_p(t.data_ptr())

    def bake(handle, n, spp, par=P, null=()):
        a = [p(d_probes), p(d_depth), p(d_counts)]
        for k in null:
            a[k] = None
        return lib.rt_render_probe_depth_device(handle, a[0], n, spp, 0, 0, 0, C.byref(par) if par is not None else None, a[1], a[2], None)

    assert bake(h, 0, 4) == 0 and bake(h, 0, 4, None, (0, 1, 2)) == 0
    for n, spp, par, null in ((8, 4, P, (0,)), (8, 4, P, (1,)), (8, 4, P, (2,)), (8, 4, None, ()), (-1, 4, P, ()), (8, 0, P, ()),
                              (8, -3, P, ()), (8, (1 << 19) + 1, P, ())):
        assert bake(h, n, spp, par, null) == -1, (n, spp, null)
        assert "rt_render_probe_depth_device" in _last_error(lib)
    assert "2^19" in _last_error(lib)
    for field, value in (("d_max", 0.0), ("var_floor", float("nan")), ("sharpness", 9), ("flags", 2)):
        bad = rc.rt_probe_depth_params.from_buffer_copy(bytes(P))
        setattr(bad, field, value)
        assert bake(h, 8, 4, bad) == -1, field
    assert bake(None, 8, 4) == -1 and "null scene" in _last_error(lib)
    # BVH2: RT_ERR_STATE for the bake; the shading needs no scene
    gpu2 = _gpu(rc, "bounce", "BVH2")
    assert bake(gpu2.handle, 8, 4) == -7 and "BVH2" in _last_error(lib)
    assert bake(gpu2.handle, 0, 4) == 0
    gpu2.close()
    # the visibility flag is refused by the depth entry
    vis = _scene_grid(rc, "bounce", visibility=True)
    shade = lambda g, n: lib.rt_shade_probes_depth_device(C.byref(g), C.byref(P), p(d_L), p(acc["D"]), p(d_probes), n, p(d_E), p(d_W), None)
    assert shade(vis, 8) == -1 and "RT_PROBE_GRID_VISIBILITY" in _last_error(lib) and shade(vis, 0) == -1
    assert shade(grid, 0) == 0 and shade(grid, -1) == -1
    assert lib.rt_probe_depth_close_device(p(d_depth), 0, None, None) == 0 and lib.rt_probe_depth_close_device(p(d_depth), 8, None, None) == -1
    torch.cuda.synchronize()
    assert (d_depth.cpu().numpy() == 2.5).all() and (d_counts.cpu().numpy() == 77).all()
    assert (d_E.cpu().numpy() == 2.5).all() and (d_W.cpu().numpy() == 2.5).all()
    # and the same calls with nothing wrong work
    d_depth[:] = 0
    d_counts[:] = 0
    assert bake(h, 8, 4) == 0 and shade(grid, 8) == 0
    torch.cuda.synchronize()
    assert (d_counts.cpu().numpy().reshape(8, 4)[:, [0, 2]].sum(axis=1) == 4).all() and d_depth.cpu().numpy().any()
    assert not (d_E.cpu().numpy() == 2.5).any() and not (d_W.cpu().numpy() == 2.5).any()


@pytest.mark.parametrize("mode", ["AUTO", "BVH"])
def test_g9_the_existing_shading_and_the_renderer_are_left_alone(rc, mode):
    """rt_shade_probes_device with flags 0 and 1, a render_tile_1spp, a render_tile and a render_surfels before and
    after the new calls are bit-identical; the counters of rt_scene_get_stats, the rt_kernel_times ring and the
    build statistics are what they were."""
    pos, nrm = _surfels("bounce")
    grid, flat = _scene_grid(rc, "bounce"), _scene_grid(rc, "bounce", visibility=False)
    L = random_L(DIMS, seed=19)
    gpu = _gpu(rc, "bounce", mode, size=(128, 128))
    shaded = [gpu.shade_probes(g, L, pos, nrm) for g in (flat, grid)]
    before = gpu.render_tile_1spp(40, 40, 24, 16, seed=3, sample_index=2)
    tile = gpu.render_tile(40, 40, 24, 16, 8, seed=3)
    gather = gpu.render_surfels(pos, nrm, 30, 11, SPHERE, stream_base=5)
    gpu.set_stats(True)
    gpu.render_tile(0, 0, 16, 16, 2, seed=4)
    assert sum(gpu.get_stats().values()) > 0  # (read and zeroed)
    launches = gpu.kernel_times(3)
    with pytest.raises(rc.RtError):
        gpu.kernel_times(4)
    stats = gpu.build_stats()
    acc = gpu.render_probe_depth(pos[:n_probes(DIMS)], 40, SEED, 1.5, normals=nrm[:n_probes(DIMS)])
    acc = gpu.render_probe_depth(pos[:n_probes(DIMS)], 24, SEED, 1.5, normals=nrm[:n_probes(DIMS)], sample_base=40, out=acc)
    E, W = gpu.shade_probes_depth(flat, L, acc["D"], rc.probe_depth_params(1.5, 5, 1e-3, True), pos, nrm)
    assert W.any() and int(acc["counts"][:, [0, 2, 3]].sum()) == n_probes(DIMS) * 64
    with pytest.raises(rc.RtError):
        gpu.kernel_times(4)
    assert np.allclose(gpu.kernel_times(3), launches, rtol=1e-4, atol=0)
    assert sum(gpu.get_stats().values()) == 0
    assert gpu.build_stats() == stats
    gpu.set_stats(False)
    for g, want in zip((flat, grid), shaded):
        assert all(same_bits(a, b) for a, b in zip(gpu.shade_probes(g, L, pos, nrm), want))
    assert same_bits(gpu.render_tile_1spp(40, 40, 24, 16, seed=3, sample_index=2), before)
    after = gpu.render_tile(40, 40, 24, 16, 8, seed=3)
    assert all(same_bits(a, b) for a, b in zip(tile[:3], after[:3])) and tile[3] == after[3]
    again = gpu.render_surfels(pos, nrm, 30, 11, SPHERE, stream_base=5)
    assert all(same_bits(a, b) for a, b in zip(gather[:3], again[:3])) and gather[3] == again[3]
    gpu.close()
