"""rt_shade_probes on the device: the segments against their host twin (G1); the result against the blend's
host twin fed with the reported segments' any-hit answers (G2, promise 1); a point's result alone, permuted,
chunked, through the host and the device entry and on a side stream (G3, promise 3); a wall between two probes
(G4); the device pipeline from the bake to the irradiance (G5); errors, empty calls and the renderer left
alone (G6).  The replay and the point sets are tests/test_shade_probes_host.py's."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from test_query_rays_gpu import _gpu, _same_bits, _scene
from test_render_surfels_gpu import _last_error, _surfels
from test_render_surfels_host import SPHERE
from test_shade_probes_host import BAD, GRIDS, N, make_grid, n_probes, points, random_L

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIMS = (4, 3, 2)


def _scene_grid(rc, name, visibility=True, bias=1e-3, dims=DIMS, z0=None):
    """dims probes over the scene's bound (rc.scene_bound) shrunk by 5 % on every side, corner to corner; z0:
    the grid's lowest plane instead of the shrunk bound's."""
    b = rc.scene_bound(list(_scene(name).prims))
    lo, hi = np.array(b["lo"], np.float64), np.array(b["hi"], np.float64)
    pad = 0.05 * (hi - lo)
    lo, hi = lo + pad, hi - pad
    if z0 is not None:
        lo[2] = z0
    return rc.probe_grid(lo, (hi - lo) / (np.array(dims) - 1), dims, visibility, bias)


def _occluded_device(gpu, rays, t_max):
    """rt_occluded_rays_device's answers (RT_QUERY_FAST) for (n, 8) segments."""
    import torch

    d_rays = torch.from_numpy(np.ascontiguousarray(rays).view(np.uint8).reshape(-1).copy()).cuda()
    d_t = torch.from_numpy(np.ascontiguousarray(t_max).reshape(-1).copy()).cuda()
    d_out = torch.full((rays.size,), 7, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    gpu.occluded_rays_device(d_rays.data_ptr(), d_t.data_ptr(), rays.size, d_out.data_ptr())
    torch.cuda.synchronize()
    occ = d_out.cpu().numpy().reshape(rays.shape)
    assert np.isin(occ, (0, 1)).all()
    return occ


def _host_path(rc, gpu, grid, L, pos, nrm):
    """Promise 1's right-hand side, and the segments' answers."""
    rays, t_max = gpu.probe_segments_device(grid, pos, nrm)
    occ = _occluded_device(gpu, rays, t_max)
    return rc.shade_probes_host(grid, L, pos, nrm, occ), occ, t_max


# ---------------------------------------------------------------- G1: the segments
@pytest.mark.parametrize("dims", GRIDS)
def test_g1_device_segments_are_the_host_twins(rc, dims):
    pos, nrm = points(dims)
    gpu = _gpu(rc, "bounce")
    for grid in (make_grid(rc, dims), make_grid(rc, dims, visibility=False), make_grid(rc, dims, bias=0.0)):
        rays, t_max = gpu.probe_segments_device(grid, pos, nrm)
        want_rays, want_t = rc.probe_segments_host(grid, pos, nrm)
        assert _same_bits(rays, want_rays) and _same_bits(t_max, want_t)
    assert t_max.any() and not t_max[BAD].any()
    one = gpu.probe_segments_device(make_grid(rc, dims, bias=0.0), pos[5:6], nrm[5:6])
    assert _same_bits(one[0], want_rays[5:6]) and _same_bits(one[1], want_t[5:6])
    gpu.close()


# ---------------------------------------------------------------- G2: promise 1
# The grids.  bounce: the room's bound shrunk by 5 %; its probes hang in the air of the room, and the light box
# and the room's furniture hide some from some points.  die: the same box puts every cell across the solid cube
# (all 197 valid points had a hidden corner), so its grid keeps the shrunk bound in x and y and starts at
# z = 1.2, in the air above the cube's +z face: points on that face see all their probes, points on the -x and
# -y faces do not.  G2_COUNTS: per case, the valid points with a hidden corner and those with segments and none
# hidden, of 200, as an MI355X gave them (133 of 770 segments occluded on bounce, 249 of 674 on die).  The test
# asks only that neither is 0, so that neither branch is vacuous: one answer of the any-hit kernels moving is
# not this test's business.
G2_GRIDS = {"bounce": None, "die": 1.2}
G2_COUNTS = {("bounce", "BRUTE"): (47, 150), ("bounce", "BVH"): (47, 150), ("die", "GROUPED"): (77, 120)}


@pytest.mark.parametrize("name,mode", list(G2_COUNTS))
def test_g2_result_is_the_twin_fed_with_the_any_hit_answers(rc, name, mode):
    pos, nrm = _surfels(name)
    grid = _scene_grid(rc, name, z0=G2_GRIDS[name])
    L = random_L(DIMS, seed=17, absent=(5,))
    gpu = _gpu(rc, name, mode)
    E, W = gpu.shade_probes(grid, L, pos, nrm)
    (want_E, want_W), occ, t_max = _host_path(rc, gpu, grid, L, pos, nrm)
    gpu.close()
    hidden = (occ != 0).any(axis=1)
    clear = (t_max > 0).any(axis=1) & ~hidden
    print(f"G2 {name} {mode}: {int(hidden.sum())} points with a hidden corner, {int(clear.sum())} with segments and none hidden, "
          f"{int((occ != 0).sum())} of {int((t_max > 0).sum())} segments occluded, {int((W == 0).sum())} points of weight 0")
    assert _same_bits(E, want_E) and _same_bits(W, want_W)
    assert hidden.sum() >= 1 and clear.sum() >= 1
    assert not E[BAD].any() and not W[BAD].any() and E.any()
    assert ((W >= 0) & (W <= 1 + 1e-15)).all() and (W[hidden] < 1).any()


# ---------------------------------------------------------------- G3: promise 3
@pytest.fixture(scope="module")
def bounce_bvh(rc):
    gpu = _gpu(rc, "bounce", "BVH", size=(128, 128))
    yield gpu
    gpu.close()


@pytest.fixture(scope="module")
def bounce_case(rc, bounce_bvh):
    pos, nrm = _surfels("bounce")
    grid = _scene_grid(rc, "bounce")
    L = random_L(DIMS, seed=18)
    return grid, L, pos, nrm, bounce_bvh.shade_probes(grid, L, pos, nrm)


def test_g3_a_points_result_does_not_depend_on_its_place(rc, bounce_bvh, bounce_case):
    grid, L, pos, nrm, (E, W) = bounce_case
    for i in (0, 1, 63, 64, 65, 199):
        E1, W1 = bounce_bvh.shade_probes(grid, L, pos[i:i + 1], nrm[i:i + 1])
        assert _same_bits(E1[0], E[i]) and W1[0] == W[i], i
    order = np.random.default_rng(4).permutation(N)
    E2, W2 = bounce_bvh.shade_probes(grid, L, pos[order], nrm[order])
    assert _same_bits(E2, E[order]) and _same_bits(W2, W[order])
    assert len(np.unique(W)) > 3


CHILD = """
import sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import raytracercore_amd as rc
from test_query_rays_gpu import _gpu
z = np.load(sys.argv[2])
gpu = _gpu(rc, "bounce", "BVH", size=(128, 128))
grid = rc.rt_probe_grid.from_buffer_copy(z["grid"].tobytes())
E, W = gpu.shade_probes(grid, z["L"], z["pos"], z["nrm"])
gpu.close()
np.savez(sys.argv[3], E=E, W=W)
"""


def test_g3_chunks(rc, bounce_case, tmp_path):
    """n = 200 cut into chunks of 8 points (RTCORE_QUERY_CHUNK = 64 segments, set for a fresh child process) is
    the one-chunk call bit for bit."""
    grid, L, pos, nrm, (E, W) = bounce_case
    np.savez(tmp_path / "case.npz", grid=np.frombuffer(bytes(grid), np.uint8), L=L, pos=pos, nrm=nrm)
    env = dict(os.environ, RTCORE_QUERY_CHUNK="64")
    subprocess.run([sys.executable, "-c", CHILD, ROOT, str(tmp_path / "case.npz"), str(tmp_path / "out.npz")],
                   check=True, env=env, timeout=300)
    z = np.load(tmp_path / "out.npz")
    assert _same_bits(z["E"], E) and _same_bits(z["W"], W)


def _device_call(rc, gpu, grid, L, pos, nrm, stream=None, weight=True):
    """shade_probes_device over torch tensors with sentinels round the outputs; (E, W)."""
    import torch

    n, pad = len(pos), 16
    d_L = torch.from_numpy(np.ascontiguousarray(L, np.float64).reshape(-1).copy()).cuda()
    d_pts = torch.from_numpy(rc._pack_surfels(pos, nrm).view(np.uint8).copy()).cuda()
    d_E = torch.full((pad + 3 * n + pad,), 2.5, dtype=torch.float64, device="cuda")
    d_W = torch.full((pad + n + pad,), 3.5, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    gpu.shade_probes_device(grid, d_L, d_pts, n, d_E[pad:], d_W[pad:] if weight else 0,
                            stream=stream.cuda_stream if stream is not None else 0)
    if stream is not None:
        stream.synchronize()
    torch.cuda.synchronize()
    E, W = d_E.cpu().numpy(), d_W.cpu().numpy()
    assert (E[:pad] == 2.5).all() and (E[pad + 3 * n:] == 2.5).all() and (W[:pad] == 3.5).all() and (W[pad + n:] == 3.5).all()
    assert weight or (W == 3.5).all()
    return E[pad:pad + 3 * n].reshape(n, 3), W[pad:pad + n]


def test_g3_host_entry_device_entry_and_a_side_stream_agree(rc, bounce_bvh, bounce_case):
    import torch

    grid, L, pos, nrm, (E, W) = bounce_case
    E1, W1 = _device_call(rc, bounce_bvh, grid, L, pos, nrm)
    assert _same_bits(E1, E) and _same_bits(W1, W)
    E2, W2 = _device_call(rc, bounce_bvh, grid, L, pos, nrm, stream=torch.cuda.Stream())
    assert _same_bits(E2, E) and _same_bits(W2, W)
    E3, _ = _device_call(rc, bounce_bvh, grid, L, pos, nrm, weight=False)
    assert _same_bits(E3, E)
    # the outputs are written, not added to: a second call into the same arrays (the host entry's are new
    # each time; here the blend without visibility, twice)
    flat = _scene_grid(rc, "bounce", visibility=False)
    E4, W4 = _device_call(rc, bounce_bvh, flat, L, pos, nrm)
    want = rc.shade_probes_host(flat, L, pos, nrm)
    assert _same_bits(E4, want[0]) and _same_bits(W4, want[1]) and not _same_bits(E4, E)


# ---------------------------------------------------------------- G4: the wall
WALL = ("size 16 12\ncamera -4 0 0, 0 0 0, 0 0 1, 60\ntwosided true\ndiffuse .5 .5 .5\nspecular 0 0 0\n"
        "vertex 0 -2 -2\nvertex 0 2 -2\nvertex 0 2 2\nvertex 0 -2 2\ntri 0 1 2\ntri 0 2 3\n")


@pytest.mark.parametrize("mode", ["BRUTE", "BVH"])
def test_g4_a_probe_behind_a_wall_does_not_light_the_point(rc, mode):
    """A two-sided wall in the plane x = 0, |y|, |z| <= 2, a red probe at x = -1 and a blue one at x = +1 (band 0
    only), points at x = -+0.25: with visibility each point is lit by its own side's probe alone, with the
    weight 0.625 that probe has in the blend; without, by both."""
    rng = np.random.default_rng(8)
    n = 64
    pos = np.concatenate([np.full((n, 1), -0.25), rng.uniform(-1, 1, (n, 2))], axis=1)
    pos[n // 2:, 0] = 0.25
    nrm = np.zeros((n, 3))
    nrm[:, 0] = np.sign(pos[:, 0])
    left = pos[:, 0] < 0
    L = np.zeros((2, 9, 3))
    L[0, 0, 0] = L[1, 0, 2] = 1.0
    grid = rc.probe_grid((-1, 0, 0), (2, 1, 1), (2, 1, 1), True, 0.0)
    # every segment crosses x = 0 at least 0.5 inside the wall's edges, or does not reach x = 0 (fp64)
    for q in ((-1.0, 0.0, 0.0), (1.0, 0.0, 0.0)):
        v = np.array(q) - pos
        crosses = np.sign(q[0]) != np.sign(pos[:, 0])
        s = -pos[:, 0] / v[:, 0]
        at = pos + s[:, None] * v
        assert (np.abs(at[crosses, 1:]) <= 1.5).all() and ((s[crosses] > 0) & (s[crosses] < 1)).all()
        assert ((s[~crosses] < 0) | (s[~crosses] > 1)).all()
    scene = rc.SceneLoader.from_text(WALL)
    gpu = rc.GpuRaytracer(scene, 0, traversal=getattr(rc, "RT_TRAVERSAL_" + mode))
    E, W = gpu.shade_probes(grid, L, pos, nrm)
    flat = rc.probe_grid((-1, 0, 0), (2, 1, 1), (2, 1, 1), False, 0.0)
    E0, W0 = gpu.shade_probes(flat, L, pos, nrm)
    gpu.close()
    assert (W == 0.625).all()
    assert (E[left, 2] == 0).all() and (E[left, 0] > 0).all() and (E[~left, 0] == 0).all() and (E[~left, 2] > 0).all()
    assert not E[:, 1].any()
    # band 0 alone: E = A_0 Y_0 L = pi * 0.28209479177387814, the blend's weight divided out again
    assert np.abs(E[left, 0] - np.pi * 0.28209479177387814).max() < 1e-15
    assert (W0 == 1.0).all() and (E0[:, 0] > 0).all() and (E0[:, 2] > 0).all()
    assert np.abs(E0[left, 0] / E0[left, 2] - 0.625 / 0.375).max() < 1e-14


# ---------------------------------------------------------------- G5: from the bake to the irradiance on the device
def test_g5_device_pipeline_end_to_end(rc, bounce_bvh):
    import torch

    grid = _scene_grid(rc, "bounce")
    n_p, spp, seed = n_probes(DIMS), 8, 5
    iz, iy, ix = np.meshgrid(*(np.arange(d) for d in DIMS[::-1]), indexing="ij")
    index = np.stack([ix, iy, iz], axis=-1).reshape(-1, 3)
    probe_pos = np.array(grid.origin) + index * np.array(grid.step)
    probe_nrm = np.tile([0.0, 0.0, 1.0], (n_p, 1))
    pos, nrm = _surfels("bounce")
    ambient = _scene("bounce").params.ambient
    # the host's way
    sh, ns, nm, _ = bounce_bvh.render_probes(probe_pos, spp, seed, normals=probe_nrm)
    L = rc.probe_radiance_sh(sh, ns, nm, ambient)
    assert np.isfinite(L).all() and (ns > 0).all()
    (want_E, want_W), occ, _ = _host_path(rc, bounce_bvh, grid, L, pos, nrm)
    # the device's, nothing leaving it until the result
    d_probes = torch.from_numpy(rc._pack_surfels(probe_pos, probe_nrm).view(np.uint8).copy()).cuda()
    d_sh = torch.zeros(n_p * 36, dtype=torch.float64, device="cuda")
    d_ns = torch.zeros(n_p, dtype=torch.int32, device="cuda")
    d_nm = torch.zeros(n_p, dtype=torch.int32, device="cuda")
    d_L = torch.full((n_p * 27 + 8,), 2.5, dtype=torch.float64, device="cuda")
    d_pts = torch.from_numpy(rc._pack_surfels(pos, nrm).view(np.uint8).copy()).cuda()
    d_E = torch.full((3 * N,), 2.5, dtype=torch.float64, device="cuda")
    d_W = torch.full((N,), 2.5, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    bounce_bvh.render_probes_device(d_probes, n_p, spp, seed, 0, 0, d_sh, d_ns, d_nm)
    rc.probe_radiance_device(d_sh, d_ns, d_nm, n_p, ambient, d_L)
    bounce_bvh.shade_probes_device(grid, d_L, d_pts, N, d_E, d_W)
    torch.cuda.synchronize()
    got_L = d_L.cpu().numpy()
    assert _same_bits(d_sh.cpu().numpy().reshape(n_p, 9, 4), sh)
    assert _same_bits(got_L[:n_p * 27].reshape(n_p, 9, 3), L) and (got_L[n_p * 27:] == 2.5).all()
    assert _same_bits(got_L[:n_p * 27].reshape(n_p, 9, 3), rc.probe_radiance_host(sh, ns, nm, ambient))
    assert _same_bits(d_E.cpu().numpy().reshape(N, 3), want_E) and _same_bits(d_W.cpu().numpy(), want_W)
    assert (want_W > 0).sum() > N // 2 and occ.any()
    # a probe without a sample is absent on the device as on the host
    d_ns[3] = 0
    d_nm[3] = 0
    rc.probe_radiance_device(d_sh, d_ns, d_nm, n_p, ambient, d_L)
    torch.cuda.synchronize()
    ns0, nm0 = ns.copy(), nm.copy()
    ns0[3] = nm0[3] = 0
    got = d_L.cpu().numpy()[:n_p * 27].reshape(n_p, 9, 3)
    assert np.isnan(got[3]).all() and _same_bits(got, rc.probe_radiance_host(sh, ns0, nm0, ambient))


# ---------------------------------------------------------------- G6: plumbing
def test_g6_empty_calls_and_errors_touch_nothing(rc, bounce_bvh, bounce_case):
    import torch

    grid, L, pos, nrm, _ = bounce_case
    lib, h = bounce_bvh.lib, bounce_bvh.handle
    pts = rc._pack_surfels(pos[20:28], nrm[20:28])
    E, W = np.full((8, 3), 7.5), np.full(8, 7.5)
    pL, pp = L.ctypes.data_as(C.POINTER(C.c_double)), pts.ctypes.data_as(C.c_void_p)
    pE, pW = E.ctypes.data_as(C.POINTER(rc.rt_color)), W.ctypes.data_as(C.POINTER(C.c_double))
    d_L = torch.from_numpy(L.reshape(-1).copy()).cuda()
    d_pts = torch.from_numpy(pts.view(np.uint8).copy()).cuda()
    d_E = torch.full((24,), 2.5, dtype=torch.float64, device="cuda")
    d_W = torch.full((8,), 2.5, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    dev = [C.c_void_p(t.data_ptr()) for t in (d_L, d_pts, d_E, d_W)]

    def host(g, n, null=()):
        p = [pL, pp, pE, pW]
        for k in null:
            p[k] = None
        return lib.rt_shade_probes(h, C.byref(g) if g is not None else None, p[0], p[1], n, p[2], p[3])

    def device(g, n, null=()):
        p = list(dev)
        for k in null:
            p[k] = None
        return lib.rt_shade_probes_device(h, C.byref(g) if g is not None else None, p[0], p[1], n, p[2], p[3], None)

    for call in (host, device):
        assert call(grid, 0) == 0 and call(grid, 0, (0, 1, 2, 3)) == 0
        for n, null in ((8, (0,)), (8, (1,)), (8, (2,)), (-1, ())):
            assert call(grid, n, null) == -1, (call.__name__, n, null)
            assert "rt_shade_probes" in _last_error(lib)
        assert call(None, 8) == -1 and "null grid" in _last_error(lib)
        for what, value in (("step", 0.0), ("origin", np.inf), ("dims", 0)):
            bad = rc.rt_probe_grid.from_buffer_copy(bytes(grid))
            getattr(bad, what)[1] = type(getattr(bad, what)[1])(value)
            assert call(bad, 8) == -1 and call(bad, 0) == -1, what
        for what, value in (("bias", -1.0), ("bias", float("nan")), ("flags", 2), ("flags", 3)):
            bad = rc.rt_probe_grid.from_buffer_copy(bytes(grid))
            setattr(bad, what, value)
            assert call(bad, 8) == -1, what
        bad = rc.rt_probe_grid.from_buffer_copy(bytes(grid))
        bad.reserved[0] = 1
        assert call(bad, 8) == -1
    # BVH2: RT_ERR_STATE with the flag, and only with it
    flat = _scene_grid(rc, "bounce", visibility=False)
    gpu2 = _gpu(rc, "bounce", "BVH2")
    h2 = gpu2.handle
    assert lib.rt_shade_probes(h2, C.byref(grid), pL, pp, 8, pE, pW) == -7 and "BVH2" in _last_error(lib)
    assert lib.rt_shade_probes_device(h2, C.byref(grid), *dev[:2], 8, *dev[2:], None) == -7
    assert lib.rt_shade_probes(h2, C.byref(grid), pL, pp, 0, pE, pW) == 0
    torch.cuda.synchronize()
    assert (E == 7.5).all() and (W == 7.5).all() and (d_E.cpu().numpy() == 2.5).all() and (d_W.cpu().numpy() == 2.5).all()
    E2, W2 = gpu2.shade_probes(flat, L, pos[20:28], nrm[20:28])
    gpu2.close()
    want = rc.shade_probes_host(flat, L, pos[20:28], nrm[20:28])
    assert _same_bits(E2, want[0]) and _same_bits(W2, want[1])
    # and the same call with nothing wrong works; without a weight array too
    assert host(grid, 8) == 0 and not (E == 7.5).any() and not (W == 7.5).any()
    E1 = E.copy()
    E[:] = 7.5
    W[:] = 7.5
    assert host(grid, 8, (3,)) == 0 and _same_bits(E, E1) and (W == 7.5).all()


@pytest.mark.parametrize("mode", ["AUTO", "BVH"])
def test_g6_shade_probes_leaves_the_renderer_alone(rc, mode):
    """A render_tile_1spp, a render_tile and a render_surfels before and after shade_probes calls are
    bit-identical; the counters of rt_scene_get_stats, the rt_kernel_times ring and the build statistics are
    what they were.  No camera is needed: the scene of G4 has none set before its call."""
    pos, nrm = _surfels("bounce")
    grid = _scene_grid(rc, "bounce")
    L = random_L(DIMS, seed=19)
    gpu = _gpu(rc, "bounce", mode, size=(128, 128))
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
    E, W = gpu.shade_probes(grid, L, pos, nrm)
    gpu.shade_probes(_scene_grid(rc, "bounce", visibility=False), L, pos[:100], nrm[:100])
    assert W.any()
    with pytest.raises(rc.RtError):
        gpu.kernel_times(4)
    assert np.allclose(gpu.kernel_times(3), launches, rtol=1e-4, atol=0)
    assert sum(gpu.get_stats().values()) == 0
    assert gpu.build_stats() == stats
    gpu.set_stats(False)
    assert _same_bits(gpu.render_tile_1spp(40, 40, 24, 16, seed=3, sample_index=2), before)
    after = gpu.render_tile(40, 40, 24, 16, 8, seed=3)
    assert all(_same_bits(a, b) for a, b in zip(tile[:3], after[:3])) and tile[3] == after[3]
    again = gpu.render_surfels(pos, nrm, 30, 11, SPHERE, stream_base=5)
    assert all(_same_bits(a, b) for a, b in zip(gather[:3], again[:3])) and gather[3] == again[3]
    assert all(_same_bits(a, b) for a, b in zip(gpu.shade_probes(grid, L, pos, nrm), (E, W)))
    gpu.close()
