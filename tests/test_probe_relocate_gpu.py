"""Probe relocation on the device: a step against the host twin over the reported rays and the query's answers
(G1, promise 1); a sphere round the probe (G2); a probe's result alone, in sub-ranges called in any order, on a
side stream and chunked, and CLASSIFY_ONLY (G3, promises 2 and 3); the placed shading against its twins and
against the unplaced entries (G4, G5); the device pipeline relocate -> positions -> bakes -> close -> placed shade
(G6); errors (G7); the existing shading and the renderer left alone (G8).  The replay is
tests/probe_relocate_cases.py's."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from probe_relocate_cases import IDLE, INSIDE, random_placement, replay_rule, same_bits
from test_probe_depth_gpu import SEED, UNIT_SPHERE
from test_query_rays_gpu import _gpu
from test_render_surfels_gpu import _last_error, _surfels
from test_render_surfels_host import SPHERE
from test_shade_probes_gpu import DIMS, _occluded_device, _scene_grid
from test_shade_probes_host import BAD, n_probes, random_L

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STREAM_BASE, SAMPLE_BASE = 1000, 3
BACK_SHARE, MAX_OFFSET = 0.25, 0.45


def _line_grid(rc, name, n, first=0, n_all=65):
    """n probes on a line along x through the scene's surfels, probe i of it being probe first + i of the line of
    n_all; the y and z steps are the surfels' extent, so offsets inside the bound scatter the probes over it."""
    pos, _ = _surfels(name)
    ok = np.isfinite(pos).all(axis=1)
    lo, hi = pos[ok].min(axis=0), pos[ok].max(axis=0)
    span = np.maximum(hi - lo, 1e-3)
    step = np.array([1.2 * span[0] / (n_all - 1), span[1], span[2]])
    origin = np.array([lo[0] - 0.1 * span[0], 0.5 * (lo[1] + hi[1]), 0.5 * (lo[2] + hi[2])])
    origin[0] = origin[0] + float(first) * step[0]  # (origin + (double)i * step of the whole line, the same double)
    return rc.probe_grid(origin, step, (n, 1, 1), False)


def _line_offsets(rc, name, n_all=65, invalid=7):
    grid = _line_grid(rc, name, n_all)
    offsets, _ = random_placement((n_all, 1, 1), tuple(grid.step), seed=51, nan_probe=invalid)
    return offsets


def _samples(rc, gpu, grid, offsets, spp, sample_base=SAMPLE_BASE, stream_base=STREAM_BASE):
    """The rays rt_debug_surfel_rays_device reports at rt_debug_probe_positions' records, and rt_query_rays' answers."""
    probes = rc.probe_positions_host(grid, offsets)
    rays = gpu.surfel_rays(probes["position"][:, :3], probes["normal"][:, :3], spp, SEED, SPHERE, sample_base=sample_base,
                           stream_base=stream_base)
    return rays, gpu.query_rays(rays)


def _step(rc, gpu, grid, params, spp, offsets, sample_base=SAMPLE_BASE, stream_base=STREAM_BASE, stream=None, out=None):
    """rt_relocate_probes_device over torch tensors with sentinels behind the arrays: (offsets after, info)."""
    import torch

    n = n_probes(tuple(grid.dims))
    if out is None:
        d_o = torch.full((n * 3 + 8,), 2.5, dtype=torch.float64, device="cuda")
        d_i = torch.full((n * 16 + 8,), 77, dtype=torch.int32, device="cuda")
    else:
        d_o, d_i = out
    d_o[:n * 3] = torch.from_numpy(np.ascontiguousarray(offsets, np.float64).reshape(-1).copy()).cuda()
    torch.cuda.synchronize()
    gpu.relocate_probes_device(grid, params, spp, SEED, sample_base, stream_base, d_o, d_i,
                               stream=stream.cuda_stream if stream is not None else 0)
    if stream is not None:
        stream.synchronize()
    torch.cuda.synchronize()
    got_o, got_i = d_o.cpu().numpy(), d_i.cpu().numpy()
    if out is None:
        assert (got_o[n * 3:] == 2.5).all() and (got_i[n * 16:] == 77).all()
    return got_o[:n * 3].reshape(n, 3), got_i[:n * 16].copy().view(rc.RELOCATION_DTYPE)


def _branches(rc, grid, params, info, offsets, rays, spp):
    """The branch each probe took and the refusals, by the replay's rule over the device's fold."""
    out = []
    for i, rec in enumerate(info):
        f = {name: (float(rec[name]) if name.startswith("d_") else int(rec[name])) for name in rec.dtype.names}
        with np.errstate(all="ignore"):
            c, state, moved, branch, refused = replay_rule(tuple(grid.step), params.back_share, params.min_front, params.max_offset, f,
                                                           spp, offsets[i], rays[i])
        assert (state, moved) == (int(rec["state"]), int(rec["moved"])), i
        out.append("refused" if refused else branch)
    return out


# ---------------------------------------------------------------- G1: promise 1
G1_CASES = [("bounce", "BRUTE"), ("bounce", "BVH"), ("die", "GROUPED")]
G1_SEEN = {}


def _g1_case(rc, name, mode):
    """One scene and mode of G1, checked once however many tests ask: the branches its probes took."""
    if (name, mode) in G1_SEEN:
        return G1_SEEN[name, mode]
    gpu = _gpu(rc, name, mode)
    offsets = _line_offsets(rc, name)
    rays, hits = _samples(rc, gpu, _line_grid(rc, name, 65), offsets, 130)
    front = (hits["prim_id"] >= 0) & (hits["inside"] == 0)
    min_front = float(np.median(hits["distance"][front]))
    P = rc.probe_relocate_params(min_front, BACK_SHARE, MAX_OFFSET)
    seen = {}
    for n, first in ((1, 0), (1, 7), (5, 3), (63, 0), (65, 0)):
        grid = _line_grid(rc, name, n, first)
        sl = slice(first, first + n)
        for spp in (1, 63, 64, 65, 130):
            got_o, info = _step(rc, gpu, grid, P, spp, offsets[sl], stream_base=STREAM_BASE + first)
            # (sample k of a probe is the same ray whatever spp is: the first spp columns of the 130)
            want_o, want = rc.probe_relocate_host(grid, P, rays[sl, :spp], hits[sl, :spp], offsets[sl])
            assert same_bits(got_o, want_o) and info.tobytes() == want.tobytes(), (n, first, spp)
            if first <= 7 < first + n:
                bad = info[7 - first]
                assert bad["state"] == INSIDE | IDLE and bad["skipped"] == spp and bad["moved"] == 0 and np.isnan(got_o[7 - first, 1])
            assert (info["front"] + info["back"] + info["misses"] + info["skipped"] == spp).all()
            for b in _branches(rc, grid, P, info, offsets[sl], rays[sl, :spp], spp):
                seen[b] = seen.get(b, 0) + 1
    gpu.close()
    print(f"G1 {name} {mode}: min_front {min_front:.4g}, branches {seen}, inside hits {int((hits['inside'] != 0).sum())} of {hits.size}")
    assert min_front > 0
    G1_SEEN[name, mode] = seen
    return seen


@pytest.mark.parametrize("name,mode", G1_CASES)
def test_g1_step_is_the_twin_over_the_reported_rays_and_the_querys_answers(rc, name, mode):
    """n = 1, 5, 63, 65 (a wave, a block of four waves and one past it) x spp = 1, 63, 64, 65, 130 (below, at and
    past one sample per lane), an invalid probe (a NaN offset) in every case but the first; min_front is the median
    front distance of the reported hits, so that probes with and without a front face inside it both occur."""
    seen = _g1_case(rc, name, mode)
    assert seen.get("b", 0) > 0 and seen.get("c", 0) > 0 and seen.get("s", 0) > 0


def test_g1_every_branch_and_the_refusal_occurred_over_the_case_set(rc):
    """Over the three cases (each is run once in a session): (a), (b), (c) and a refused candidate each occurred."""
    total = {}
    for name, mode in G1_CASES:
        for k, v in _g1_case(rc, name, mode).items():
            total[k] = total.get(k, 0) + v
    print(f"G1 branches over the case set: {total}")
    assert all(total.get(b, 0) > 0 for b in ("a", "b", "c", "refused")), total


# ---------------------------------------------------------------- G2: a sphere round the probe
def test_g2_a_probe_at_the_centre_of_a_unit_sphere(rc):
    """Every sample hits the two-sided unit sphere from inside, and, from its centre, at the distance 1.0f exactly
    (the depth tests' G4 scene): the fold keeps sample 0, the rule moves the probe along D_0 by 1 + min_front / 2
    where the step lets it (step 4: (1.125 / 4)^2 < 0.45^2) and leaves it where the step does not (step 1)."""
    gpu = rc.GpuRaytracer(rc.SceneLoader.from_text(UNIT_SPHERE), 0)
    P = rc.probe_relocate_params(0.25, BACK_SHARE, MAX_OFFSET)
    for step, moves in ((4.0, True), (1.0, False)):
        grid = rc.probe_grid((0, 0, 0), (step,) * 3, (1, 1, 1), False)
        rays, hits = _samples(rc, gpu, grid, None, 64)
        assert (hits["inside"] == 1).all() and (hits["distance"] == 1.0).all()
        got_o, info = _step(rc, gpu, grid, P, 64, np.zeros((1, 3)))
        rec = info[0]
        assert (rec["k_back"], rec["k_near"], rec["k_far"], rec["back"], rec["front"]) == (0, -1, -1, 64, 0)
        assert rec["state"] == INSIDE | IDLE and rec["d_back"] == 1.0 and rec["moved"] == int(moves)
        want = rays["direction"][0, 0, :3] * (1.0 + 0.25 * 0.5) if moves else np.zeros(3)
        assert same_bits(got_o[0], want), (step, got_o, want)
    gpu.close()


# ---------------------------------------------------------------- G3: promises 2 and 3
@pytest.fixture(scope="module")
def bounce_bvh(rc):
    gpu = _gpu(rc, "bounce", "BVH", size=(128, 128))
    yield gpu
    gpu.close()


G3_N, G3_SPP, G3_FRONT = 65, 70, 0.3


@pytest.fixture(scope="module")
def step_case(rc, bounce_bvh):
    offsets = _line_offsets(rc, "bounce")
    P = rc.probe_relocate_params(G3_FRONT, BACK_SHARE, MAX_OFFSET)
    got_o, info = _step(rc, bounce_bvh, _line_grid(rc, "bounce", G3_N), P, G3_SPP, offsets)
    assert info["moved"].sum() > 5
    return offsets, P, got_o, info


def test_g3_a_probes_result_does_not_depend_on_its_place(rc, bounce_bvh, step_case):
    import torch

    offsets, P, got_o, info = step_case
    for i in (0, 7, 63, 64):
        o1, i1 = _step(rc, bounce_bvh, _line_grid(rc, "bounce", 1, i), P, G3_SPP, offsets[i:i + 1], stream_base=STREAM_BASE + i)
        assert same_bits(o1[0], got_o[i]) and i1.tobytes() == info[i:i + 1].tobytes(), i
    # sub-ranges called in a shuffled order into slices of one pair of arrays
    whole = (torch.full((G3_N * 3 + 8,), 2.5, dtype=torch.float64, device="cuda"), torch.full((G3_N * 16 + 8,), 77, dtype=torch.int32, device="cuda"))
    cuts = [0, 1, 6, 40, 64, 65]
    for k in np.random.default_rng(4).permutation(len(cuts) - 1):
        a, b = cuts[k], cuts[k + 1]
        _step(rc, bounce_bvh, _line_grid(rc, "bounce", b - a, a), P, G3_SPP, offsets[a:b], stream_base=STREAM_BASE + a,
              out=(whole[0][a * 3:], whole[1][a * 16:]))
    w_o, w_i = whole[0].cpu().numpy(), whole[1].cpu().numpy()
    assert (w_o[G3_N * 3:] == 2.5).all() and (w_i[G3_N * 16:] == 77).all()
    assert same_bits(w_o[:G3_N * 3].reshape(G3_N, 3), got_o) and w_i[:G3_N * 16].tobytes() == info.tobytes()


def test_g3_a_side_stream_gives_the_same_bits(rc, bounce_bvh, step_case):
    import torch

    offsets, P, got_o, info = step_case
    o1, i1 = _step(rc, bounce_bvh, _line_grid(rc, "bounce", G3_N), P, G3_SPP, offsets, stream=torch.cuda.Stream())
    assert same_bits(o1, got_o) and i1.tobytes() == info.tobytes()


def test_g3_classify_only_leaves_the_offsets_bits(rc, bounce_bvh, step_case):
    offsets, P, got_o, info = step_case
    o1, i1 = _step(rc, bounce_bvh, _line_grid(rc, "bounce", G3_N), rc.probe_relocate_params(G3_FRONT, BACK_SHARE, MAX_OFFSET, True),
                   G3_SPP, offsets)
    assert same_bits(o1, offsets) and i1.tobytes() == info.tobytes() and not same_bits(got_o, offsets)


CHILD = """
import sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import raytracercore_amd as rc
from test_query_rays_gpu import _gpu
from test_probe_relocate_gpu import _line_grid, _step, G3_N, G3_SPP, G3_FRONT, BACK_SHARE, MAX_OFFSET
offsets = np.load(sys.argv[2])["offsets"]
gpu = _gpu(rc, "bounce", "BVH", size=(128, 128))
P = rc.probe_relocate_params(G3_FRONT, BACK_SHARE, MAX_OFFSET)
o70, i70 = _step(rc, gpu, _line_grid(rc, "bounce", G3_N), P, G3_SPP, offsets)
o5, i5 = _step(rc, gpu, _line_grid(rc, "bounce", G3_N), P, 5, offsets)
gpu.close()
np.savez(sys.argv[3], o70=o70, i70=i70.view(np.uint8), o5=o5, i5=i5.view(np.uint8))
"""


def test_g3_chunks(rc, bounce_bvh, step_case, tmp_path):
    """RTCORE_QUERY_CHUNK = 96 samples, set for a fresh child process: at 70 spp a chunk is one probe, at 5 spp it
    is 19; both are the one-chunk call bit for bit."""
    offsets, P, got_o, info = step_case
    o5, i5 = _step(rc, bounce_bvh, _line_grid(rc, "bounce", G3_N), P, 5, offsets)
    np.savez(tmp_path / "case.npz", offsets=offsets)
    env = dict(os.environ, RTCORE_QUERY_CHUNK="96")
    subprocess.run([sys.executable, "-c", CHILD, ROOT, str(tmp_path / "case.npz"), str(tmp_path / "out.npz")],
                   check=True, env=env, timeout=300)
    z = np.load(tmp_path / "out.npz")
    assert same_bits(z["o70"], got_o) and z["i70"].tobytes() == info.tobytes()
    assert same_bits(z["o5"], o5) and z["i5"].tobytes() == i5.tobytes()


# ---------------------------------------------------------------- G4, G5: the placed shading
@pytest.fixture(scope="module")
def shade_case(rc, bounce_bvh):
    """The 4 x 3 x 2 grid over the room, depth maps baked at 64 spp at the placed positions, random L with an absent
    probe, random offsets with 15 % RT_PROBE_INSIDE states and a NaN offset, and the 200 surfels tiled to 257."""
    grid = _scene_grid(rc, "bounce", visibility=False)
    offsets, state = random_placement(DIMS, tuple(grid.step), seed=53, nan_probe=9)
    probes = bounce_bvh.probe_positions(grid, offsets)
    host = rc.probe_positions_host(grid, offsets)
    assert probes.cpu().numpy().tobytes() == host.tobytes() and np.isnan(host["position"][9]).all()
    d_max = float(2 * np.linalg.norm(np.array(grid.step)))
    acc = bounce_bvh.render_probe_depth(host, 64, SEED, d_max)
    L = random_L(DIMS, seed=17, absent=(5,))
    pos, nrm = _surfels("bounce")
    pos, nrm = np.concatenate([pos, pos[:57] + 0.01]), np.concatenate([nrm, nrm[:57]])
    return grid, offsets, state, d_max, acc, L, pos, nrm


@pytest.mark.parametrize("visibility", [False, True])
def test_g4_placed_blend_is_the_twin(rc, bounce_bvh, shade_case, visibility):
    import torch

    _, offsets, state, _, _, L, pos, nrm = shade_case
    grid = _scene_grid(rc, "bounce", visibility=visibility)
    for n in (1, 255, 257):
        rays, t_max = bounce_bvh.probe_segments_placed_device(grid, offsets, state, pos[:n], nrm[:n])
        want_rays, want_t = rc.probe_segments_placed_host(grid, offsets, state, pos[:n], nrm[:n])
        assert same_bits(rays, want_rays) and same_bits(t_max, want_t), n
        occ = _occluded_device(bounce_bvh, rays, t_max)
        want_E, want_W = rc.shade_probes_placed_host(grid, offsets, state, L, pos[:n], nrm[:n], occ)
        E, W = bounce_bvh.shade_probes(grid, L, pos[:n], nrm[:n], offsets=offsets, state=state)  # (the host-buffer entry)
        assert same_bits(E, want_E) and same_bits(W, want_W), n
        d_o, d_s = bounce_bvh._device_placement(grid, offsets, state, torch.device("cuda"))
        d_L = torch.from_numpy(L.reshape(-1).copy()).cuda()
        d_pts = torch.from_numpy(rc._pack_surfels(pos[:n], nrm[:n]).view(np.uint8).copy()).cuda()
        d_E = torch.full((3 * n + 8,), 2.5, dtype=torch.float64, device="cuda")
        d_W = torch.full((n + 8,), 2.5, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        bounce_bvh.shade_probes_placed_device(grid, d_o, d_s, d_L, d_pts, n, d_E, d_W)
        torch.cuda.synchronize()
        got_E, got_W = d_E.cpu().numpy(), d_W.cpu().numpy()
        assert same_bits(got_E[:3 * n].reshape(n, 3), want_E) and same_bits(got_W[:n], want_W), n
        assert (got_E[3 * n:] == 2.5).all() and (got_W[n:] == 2.5).all()
    plain = bounce_bvh.shade_probes(grid, L, pos, nrm)
    print(f"G4 visibility={visibility}: {int((W > 0).sum())} of {len(W)} points lit, {int((W != plain[1]).sum())} weights differ "
          f"from the unplaced blend's, {int(occ.sum())} of {occ.size} segments hidden")
    assert not E[BAD].any() and not W[BAD].any() and E.any() and (W != plain[1]).any()
    assert t_max.any() == visibility


@pytest.mark.parametrize("wrap", [False, True])
def test_g4_placed_depth_shading_is_the_twin(rc, bounce_bvh, shade_case, wrap):
    grid, offsets, state, d_max, acc, L, pos, nrm = shade_case
    D = acc["D"].cpu().numpy()
    P = rc.probe_depth_params(d_max, 5, 1e-3, wrap)
    for n in (1, 255, 257):
        E, W = bounce_bvh.shade_probes_depth(grid, L, acc["D"], P, pos[:n], nrm[:n], offsets=offsets, state=state)
        want_E, want_W = rc.shade_probes_depth_placed_host(grid, offsets, state, L, D, P, pos[:n], nrm[:n])
        assert same_bits(E, want_E) and same_bits(W, want_W), n
    plain = bounce_bvh.shade_probes_depth(grid, L, acc["D"], P, pos, nrm)
    assert not E[BAD].any() and not W[BAD].any() and E.any() and (W != plain[1]).any()
    only_o = bounce_bvh.shade_probes_depth(grid, L, acc["D"], P, pos, nrm, offsets=offsets)
    want = rc.shade_probes_depth_placed_host(grid, offsets, None, L, D, P, pos, nrm)
    assert same_bits(only_o[0], want[0]) and same_bits(only_o[1], want[1]) and not same_bits(only_o[1], W)


def test_g5_no_placement_is_the_unplaced_entry(rc, bounce_bvh, shade_case):
    """Promise 2 of the placed entries: NULL arrays and all-zero arrays against the existing entries, bit for bit."""
    grid, _, _, d_max, acc, L, pos, nrm = shade_case
    vis = _scene_grid(rc, "bounce", visibility=True)
    n = n_probes(DIMS)
    P = rc.probe_depth_params(d_max, 5, 1e-3, True)
    depth = bounce_bvh.shade_probes_depth(grid, L, acc["D"], P, pos, nrm)
    seg = bounce_bvh.probe_segments_device(vis, pos, nrm)
    for o, s in ((np.zeros((n, 3)), np.zeros(n, np.uint32)), (np.zeros((n, 3)), None), (None, np.full(n, IDLE, np.uint32))):
        for g in (grid, vis):
            want = bounce_bvh.shade_probes(g, L, pos, nrm)
            got = bounce_bvh.shade_probes(g, L, pos, nrm, offsets=o, state=s)
            assert same_bits(got[0], want[0]) and same_bits(got[1], want[1])
        got = bounce_bvh.shade_probes_depth(grid, L, acc["D"], P, pos, nrm, offsets=o, state=s)
        assert same_bits(got[0], depth[0]) and same_bits(got[1], depth[1])
        got = bounce_bvh.probe_segments_placed_device(vis, o, s, pos, nrm)
        assert same_bits(got[0], seg[0]) and same_bits(got[1], seg[1])
    got = bounce_bvh.probe_segments_placed_device(vis, None, None, pos, nrm)
    assert same_bits(got[0], seg[0]) and same_bits(got[1], seg[1]) and seg[1].any() and depth[1].any()


# ---------------------------------------------------------------- G6: the device pipeline
def test_g6_device_pipeline_relocate_positions_bakes_close_placed_shade(rc, bounce_bvh, shade_case):
    """Two steps and a classification, the positions, the radiance and the depth bake there, the close and the
    placed depth shading with nothing leaving the device until the result, against the twins fed with the reported
    rays and the query's answers."""
    import torch

    grid, _, _, d_max, _, _, pos, nrm = shade_case
    n_p, spp, n = n_probes(DIMS), 33, 200
    R = rc.probe_relocate_params(0.6 * float(min(grid.step)), BACK_SHARE, MAX_OFFSET)
    P = rc.probe_depth_params(d_max, 3, 1e-3, True)
    d_o, d_state, d_info, moved = bounce_bvh.relocate_probes(grid, R, spp, 2, SEED)
    # the twins, step by step
    want_o = np.zeros((n_p, 3))
    want_moved = []
    for j in range(3):
        rays, hits = _samples(rc, bounce_bvh, grid, want_o, spp, j * spp, 0)
        par = R if j < 2 else rc.probe_relocate_params(R.min_front, BACK_SHARE, MAX_OFFSET, True)
        want_o, want_info = rc.probe_relocate_host(grid, par, rays, hits, want_o)
        want_moved.append(int(want_info["moved"].sum()))
    assert same_bits(d_o.cpu().numpy(), want_o) and d_info.cpu().numpy().tobytes() == want_info.tobytes()
    assert same_bits(d_state.cpu().numpy().view(np.uint32), want_info["state"]) and moved == want_moved[:2] and moved[0] > 0
    print(f"G6: moved per step {moved}, then {want_moved[2]} would; states {np.bincount(want_info['state'], minlength=4).tolist()}")
    d_probes = bounce_bvh.probe_positions(grid, d_o)
    want_probes = rc.probe_positions_host(grid, want_o)
    assert d_probes.cpu().numpy().tobytes() == want_probes.tobytes()
    d_depth = torch.zeros((n_p, 3, 64), dtype=torch.float64, device="cuda")
    d_counts = torch.zeros((n_p, 4), dtype=torch.int32, device="cuda")
    d_D = torch.empty((n_p, 64, 2), dtype=torch.float64, device="cuda")
    d_pts = torch.from_numpy(rc._pack_surfels(pos[:n], nrm[:n]).view(np.uint8).copy()).cuda()
    d_E = torch.full((3 * n,), 2.5, dtype=torch.float64, device="cuda")
    d_W = torch.full((n,), 2.5, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    d_sh = torch.zeros((n_p, 9, 4), dtype=torch.float64, device="cuda")
    d_ns, d_nm = (torch.zeros(n_p, dtype=torch.int32, device="cuda") for _ in range(2))
    d_L = torch.empty((n_p, 9, 3), dtype=torch.float64, device="cuda")
    bounce_bvh.render_probes_device(d_probes, n_p, spp, SEED, 0, 0, d_sh, d_ns, d_nm)
    rc.probe_radiance_device(d_sh, d_ns, d_nm, n_p, (0.1, 0.1, 0.1), d_L)
    bounce_bvh.render_probe_depth_device(d_probes, n_p, spp, SEED, 0, 0, P, d_depth, d_counts)
    rc.probe_depth_close_device(d_depth, n_p, d_D)
    rc.shade_probes_depth_placed_device(grid, d_o, d_state, P, d_L, d_D, d_pts, n, d_E, d_W)
    torch.cuda.synchronize()
    # the radiance bake at the relocated records is the bake at the twin's records (the bake has its own tests)
    L = d_L.cpu().numpy()
    sh, ns, nm, _ = bounce_bvh.render_probes(want_probes, spp, SEED)
    assert same_bits(d_sh.cpu().numpy(), sh) and np.array_equal(d_ns.cpu().numpy().view(np.uint32), ns)
    assert same_bits(L, rc.probe_radiance_host(sh, ns, nm, (0.1, 0.1, 0.1))) and np.isfinite(L[want_info["state"] & INSIDE == 0]).all()
    rays, hits = _samples(rc, bounce_bvh, grid, want_o, spp, 0, 0)
    want_depth, want_counts = rc.probe_depth_fold_host(P, rays, hits)
    want_D = rc.probe_depth_close_host(want_depth)
    want_E, want_W = rc.shade_probes_depth_placed_host(grid, want_o, want_info["state"], L, want_D, P, pos[:n], nrm[:n])
    assert same_bits(d_depth.cpu().numpy(), want_depth) and same_bits(d_counts.cpu().numpy().view(np.uint32), want_counts)
    assert same_bits(d_D.cpu().numpy(), want_D)
    assert same_bits(d_E.cpu().numpy().reshape(n, 3), want_E) and same_bits(d_W.cpu().numpy(), want_W) and (want_W > 0).sum() > n // 2


# ---------------------------------------------------------------- G7: errors
def test_g7_errors_touch_nothing(rc, bounce_bvh, shade_case):
    import torch

    grid = shade_case[0]
    lib, h = bounce_bvh.lib, bounce_bvh.handle
    n = n_probes(DIMS)
    P = rc.probe_relocate_params(0.3)
    d_o = torch.full((n * 3,), 2.5, dtype=torch.float64, device="cuda")
    d_i = torch.full((n * 16,), 77, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731

    def step(handle, spp, par=P, g=grid, null=()):
        a = [p(d_o), p(d_i)]
        for k in null:
            a[k] = None
        return lib.rt_relocate_probes_device(handle, C.byref(g) if g is not None else None, C.byref(par) if par is not None else None, spp, 0, 0,
                                             0, a[0], a[1], None)

    for spp, par, g, null in ((4, P, grid, (0,)), (4, P, grid, (1,)), (4, None, grid, ()), (4, P, None, ()), (0, P, grid, ()),
                              (-3, P, grid, ()), ((1 << 19) + 1, P, grid, ())):
        assert step(h, spp, par, g, null) == -1, (spp, null)
        assert "rt_relocate_probes_device" in _last_error(lib)
    assert "2^19" in _last_error(lib)
    for field, value in (("back_share", 1.0), ("min_front", 0.0), ("max_offset", 0.5), ("flags", 2), ("reserved", 1)):
        bad = rc.rt_probe_relocate_params.from_buffer_copy(bytes(P))
        setattr(bad, field, value)
        assert step(h, 4, bad) == -1, field
    assert step(None, 4) == -1 and "null scene" in _last_error(lib)
    gpu2 = _gpu(rc, "bounce", "BVH2")
    assert step(gpu2.handle, 4) == -7 and "BVH2" in _last_error(lib)
    vis = _scene_grid(rc, "bounce", visibility=True)
    d_pts = torch.zeros((4, 64), dtype=torch.uint8, device="cuda")
    assert lib.rt_shade_probes_placed_device(gpu2.handle, C.byref(vis), None, None, p(d_o), p(d_pts), 4, p(d_o), None, None) == -7
    gpu2.close()
    torch.cuda.synchronize()
    assert (d_o.cpu().numpy() == 2.5).all() and (d_i.cpu().numpy() == 77).all()
    # and the same call with nothing wrong works
    d_o[:] = 0
    assert step(h, 4) == 0
    torch.cuda.synchronize()
    info = d_i.cpu().numpy().view(rc.RELOCATION_DTYPE)
    assert (info["front"] + info["back"] + info["misses"] == 4).all() and (info["reserved"] == 0).all()


# ---------------------------------------------------------------- G8: everything else left alone
@pytest.mark.parametrize("mode", ["AUTO", "BVH"])
def test_g8_the_existing_shading_and_the_renderer_are_left_alone(rc, mode):
    """rt_shade_probes_device with flags 0 and 1, rt_shade_probes_depth_device, a render_tile_1spp, a render_tile and
    a render_surfels before and after the new calls are bit-identical; the counters of rt_scene_get_stats, the
    rt_kernel_times ring and the build statistics are what they were."""
    pos, nrm = _surfels("bounce")
    grid, flat = _scene_grid(rc, "bounce"), _scene_grid(rc, "bounce", visibility=False)
    L = random_L(DIMS, seed=19)
    gpu = _gpu(rc, "bounce", mode, size=(128, 128))
    shaded = [gpu.shade_probes(g, L, pos, nrm) for g in (flat, grid)]
    DP = rc.probe_depth_params(1.5, 5, 1e-3, True)
    acc = gpu.render_probe_depth(rc.probe_positions_host(flat), 32, SEED, 1.5)
    depth = gpu.shade_probes_depth(flat, L, acc["D"], DP, pos, nrm)
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
    d_o, d_state, d_info, moved = gpu.relocate_probes(flat, rc.probe_relocate_params(0.5 * float(min(flat.step))), 40, 2, SEED)
    E, W = gpu.shade_probes(grid, L, pos, nrm, offsets=d_o, state=d_state)
    E2, W2 = gpu.shade_probes_depth(flat, L, acc["D"], DP, pos, nrm, offsets=d_o, state=d_state)
    gpu.probe_positions(flat, d_o)
    assert W.any() and W2.any() and len(moved) == 2
    with pytest.raises(rc.RtError):
        gpu.kernel_times(4)
    assert np.allclose(gpu.kernel_times(3), launches, rtol=1e-4, atol=0)
    assert sum(gpu.get_stats().values()) == 0
    assert gpu.build_stats() == stats
    gpu.set_stats(False)
    for g, want in zip((flat, grid), shaded):
        assert all(same_bits(a, b) for a, b in zip(gpu.shade_probes(g, L, pos, nrm), want))
    assert all(same_bits(a, b) for a, b in zip(gpu.shade_probes_depth(flat, L, acc["D"], DP, pos, nrm), depth))
    assert same_bits(gpu.render_tile_1spp(40, 40, 24, 16, seed=3, sample_index=2), before)
    after = gpu.render_tile(40, 40, 24, 16, 8, seed=3)
    assert all(same_bits(a, b) for a, b in zip(tile[:3], after[:3])) and tile[3] == after[3]
    again = gpu.render_surfels(pos, nrm, 30, 11, SPHERE, stream_base=5)
    assert all(same_bits(a, b) for a, b in zip(gather[:3], again[:3])) and gather[3] == again[3]
    gpu.close()
