"""Probe relocation, host side (no GPU): include/rtcore.h's "probe relocation" restated in plain Python
(tests/probe_relocate_cases.py) and held to the host twins bit for bit: the fold and the rule over forced cases
(H1), the positions (H2), the placed segment, blend and depth twins and their promise 2 (H3), the argument
errors (H4), the records' layout and the twins under sanitizers (H5), the binding.
tests/test_probe_relocate_gpu.py holds the device to the twins."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

from probe_depth_cases import random_D
from probe_relocate_cases import (BACK_SHARE, CLASSIFY_ONLY, FORCED, IDLE, INSIDE, MAX_OFFSET, MIN_FRONT, SPP, STEP as R_STEP,
                                  WANT_BRANCH, forced_samples, info_matches, random_placement, replay_absent_mask,
                                  replay_positions, replay_relocate, replay_segments_placed, replay_shade_depth_placed, same_bits)
from test_render_rays_host import SCALARS, _header_prototype, _last_error
from test_shade_probes_host import BIAS, GRIDS, ORIGIN, STEP, make_grid, n_probes, points, random_L, replay_blend

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "raytracercore_amd", "csrc")
NAMES = {"rt_probe_positions_device": 4, "rt_debug_probe_positions": 3, "rt_relocate_probes_device": 10,
         "rt_debug_probe_relocate": 7, "rt_shade_probes_placed_device": 10, "rt_shade_probes_placed": 9,
         "rt_debug_probe_segments_placed_device": 8, "rt_debug_probe_segments_placed": 7, "rt_debug_shade_probes_placed": 9,
         "rt_shade_probes_depth_placed_device": 11, "rt_debug_shade_probes_depth_placed": 10}
R_ORIGIN = (0.5, -1.0, 2.0)
D_MAX, FLOOR = 1.0, 1e-3


def _params(rc, classify_only=False, min_front=MIN_FRONT, back_share=BACK_SHARE, max_offset=MAX_OFFSET):
    return rc.probe_relocate_params(min_front, back_share, max_offset, classify_only)


def _forced(rc):
    names, dims, rays, hits, offsets = forced_samples(rc)
    return names, rc.probe_grid(R_ORIGIN, R_STEP, dims, False), rays, hits, offsets


# ---------------------------------------------------------------- H1: the fold and the rule
def test_h1_twin_against_the_replay_on_the_forced_cases(rc):
    names, grid, rays, hits, offsets = _forced(rc)
    got_o, info = rc.probe_relocate_host(grid, _params(rc), rays, hits, offsets)
    want_o, want, branches, refused = replay_relocate(R_STEP, BACK_SHARE, MIN_FRONT, MAX_OFFSET, 0, rays, hits, offsets)
    assert same_bits(got_o, want_o) and info_matches(info, want)
    assert dict(zip(names, branches)) == WANT_BRANCH
    rec, at = dict(zip(names, info)), dict(zip(names, got_o))
    was = dict(zip(names, offsets))
    assert [n for n, r in zip(names, refused) if r] == ["refused_outside", "refused_not_finite"]
    # (a): the nearest back face is sample 2 along +x at 0.2: 0.2 + 0.125 along it
    assert rec["a_taken"]["state"] == INSIDE and rec["a_taken"]["k_back"] == 2 and at["a_taken"].tolist() == [0.2 + 0.125, 0.0, 0.0]
    assert rec["a_exact_share"]["state"] == 0 and rec["a_exact_share"]["back"] == 2 and rec["a_exact_share"]["moved"] == 0
    assert rec["b_p_positive"]["moved"] == 0 and same_bits(at["b_p_positive"], was["b_p_positive"])
    assert at["b_p_zero_h_above"].tolist() == [0.0, 0.05 + MIN_FRONT, 0.0]
    assert at["b_p_negative_h_below"].tolist() == [-0.15, 0.0, 0.0]  # half the far distance, below min_front
    assert at["b_p_negative_h_above"].tolist() == [-MIN_FRONT, 0.0, 0.1]
    assert rec["c_len_zero"]["moved"] == 0 and rec["c_len_zero"]["state"] == 0
    # home exactly: three +0.0, also where the offset held -0.0 (its bits change: moved)
    assert at["c_home_exactly"].tobytes() == np.zeros(3).tobytes() and rec["c_home_exactly"]["moved"] == 1
    part = at["c_part_way"]
    assert rec["c_part_way"]["moved"] == 1 and 0 < np.linalg.norm(part) < np.linalg.norm(was["c_part_way"])
    assert abs(np.linalg.norm(was["c_part_way"]) - np.linalg.norm(part) - (0.35 - MIN_FRONT)) < 1e-15
    assert at["c_no_front"].tobytes() == np.zeros(3).tobytes() and rec["c_no_front"]["state"] == IDLE
    for name in ("refused_outside", "refused_not_finite"):
        assert rec[name]["moved"] == 0 and rec[name]["state"] & INSIDE and same_bits(at[name], was[name])
    assert rec["refused_not_finite"]["k_back"] == -1 and rec["refused_not_finite"]["d_back"] == math.inf
    t = rec["ties_keep_lowest_k"]
    assert (t["k_back"], t["k_near"], t["k_far"]) == (0, 1, 2) and (t["d_back"], t["d_near"], t["d_far"]) == (0.5, 0.1, 2.0)
    z = rec["zeros_of_both_signs_tie"]
    assert z["k_near"] == 1 and not np.signbit(z["d_near"])
    nn = rec["nan_counted_never_chosen"]
    assert (nn["front"], nn["back"], nn["k_near"], nn["k_far"], nn["k_back"]) == (4, 1, 1, 4, -1)
    ms = rec["misses_and_skipped"]
    assert (ms["skipped"], ms["misses"], ms["front"]) == (2, SPP - 4, 2)
    for name in ("all_skipped", "offset_not_finite"):
        assert rec[name]["state"] == INSIDE | IDLE and rec[name]["moved"] == 0 and rec[name]["skipped"] == SPP
        assert same_bits(at[name], was[name])
    assert (info["reserved"] == 0).all() and (info["front"] + info["back"] + info["misses"] + info["skipped"] == SPP).all()


def test_h1_classify_only_reports_and_leaves_the_offsets(rc):
    names, grid, rays, hits, offsets = _forced(rc)
    start = offsets.copy()
    step_o, step_info = rc.probe_relocate_host(grid, _params(rc), rays, hits, offsets)
    got_o, info = rc.probe_relocate_host(grid, _params(rc, classify_only=True), rays, hits, offsets)
    assert same_bits(got_o, start) and same_bits(offsets, start)
    assert info.tobytes() == step_info.tobytes() and info["moved"].sum() >= 8  # (moved: what a step would do)
    want_o, want, _, _ = replay_relocate(R_STEP, BACK_SHARE, MIN_FRONT, MAX_OFFSET, CLASSIFY_ONLY, rays, hits, offsets)
    assert same_bits(want_o, start) and info_matches(info, want)


def test_h1_random_samples_and_a_second_step(rc):
    """Random directions, kinds and distances (ties by construction: distances from a set of eight values), from
    random offsets; then a second step from the first one's offsets."""
    rng = np.random.default_rng(71)
    dims, spp = (5, 4, 3), 24
    n = n_probes(dims)
    grid = rc.probe_grid(R_ORIGIN, R_STEP, dims, False)
    d = rng.normal(size=(n, spp, 3))
    d = (d / np.linalg.norm(d, axis=-1, keepdims=True)).astype(np.float32).astype(np.float64)
    rays, hits = np.zeros((n, spp), rc.RAY_DTYPE), np.zeros((n, spp), rc.HIT_DTYPE)
    rays["direction"][..., :3] = d
    rays["direction"][rng.random((n, spp)) < 0.05] = 0.0
    hits["prim_id"] = np.where(rng.random((n, spp)) < 0.3, -1, 5)
    hits["inside"] = rng.random((n, spp)) < np.linspace(0, 0.6, n)[:, None]
    hits["distance"] = rng.choice([0.05, 0.1, 0.2, 0.3, 0.6, 1.0, 2.5, np.nan], (n, spp))
    hits["distance"] *= np.where(np.arange(n) % 3 == 0, 8.0, 1.0)[:, None]  # (every third probe has nothing within min_front)
    offsets, _ = random_placement(dims, R_STEP, seed=72)
    seen = set()
    for _ in range(2):
        got_o, info = rc.probe_relocate_host(grid, _params(rc), rays, hits, offsets)
        want_o, want, branches, refused = replay_relocate(R_STEP, BACK_SHARE, MIN_FRONT, MAX_OFFSET, 0, rays, hits, offsets)
        assert same_bits(got_o, want_o) and info_matches(info, want)
        seen |= set(branches) | ({"refused"} if any(refused) else set())
        offsets = got_o
    assert seen >= {"a", "b", "c", "refused"}


# ---------------------------------------------------------------- H2: positions
@pytest.mark.parametrize("dims", GRIDS)
def test_h2_positions_twin(rc, dims):
    grid = make_grid(rc, dims)
    offsets, _ = random_placement(dims, STEP, nan_probe=n_probes(dims) - 1)
    offsets[0] = (-0.0, 0.0, math.inf) if n_probes(dims) > 2 else offsets[0]
    got = rc.probe_positions_host(grid, offsets)
    want = replay_positions(ORIGIN, STEP, dims, offsets)
    assert same_bits(got["position"], want[:, 0]) and same_bits(got["normal"], want[:, 1])
    assert np.isnan(got["position"][-1]).all() and (got["normal"] == [0, 0, 1, 0]).all()
    if n_probes(dims) > 2:
        assert np.isnan(got["position"][0]).all() and np.isfinite(got["position"][1:-1]).all()
    plain = rc.probe_positions_host(grid)
    assert same_bits(plain["position"], replay_positions(ORIGIN, STEP, dims, None)[:, 0])
    assert same_bits(plain, rc.probe_positions_host(grid, np.zeros((n_probes(dims), 3))))
    ix = np.arange(n_probes(dims)) % dims[0]
    assert same_bits(plain["position"][:, 0], ORIGIN[0] + ix * STEP[0])


# ---------------------------------------------------------------- H3: the placed twins
def _placement(dims):
    return random_placement(dims, STEP, nan_probe=1 if n_probes(dims) > 1 else None)


@pytest.mark.parametrize("dims", GRIDS)
def test_h3_placed_segments_twin_against_the_replay(rc, dims):
    pos, nrm = points(dims)
    offsets, state = _placement(dims)
    rays, t_max = rc.probe_segments_placed_host(make_grid(rc, dims), offsets, state, pos, nrm)
    want_rays, want_t = replay_segments_placed(ORIGIN, STEP, dims, BIAS, offsets, state, pos, nrm)
    assert same_bits(rays["origin"], want_rays[:, :, 0]) and same_bits(rays["direction"], want_rays[:, :, 1])
    assert same_bits(t_max, want_t)
    plain = rc.probe_segments_host(make_grid(rc, dims), pos, nrm)
    absent = replay_absent_mask(ORIGIN, STEP, dims, offsets, state, pos, nrm)
    assert (t_max[absent] == 0).all() and not same_bits(t_max, plain[1])
    if n_probes(dims) > 1:
        assert absent.any() and (plain[1][absent] > 0).any()
    # without visibility every segment is the empty one
    none = rc.probe_segments_placed_host(make_grid(rc, dims, visibility=False), offsets, state, pos, nrm)
    assert not none[1].any() and not none[0]["origin"].any()


@pytest.mark.parametrize("dims", GRIDS)
def test_h3_placed_blend_twin_against_the_replay(rc, dims):
    """The placed blend is the plain blend without the absent probes: the replay of "probe grids" with those
    corners given as hidden."""
    pos, nrm = points(dims)
    offsets, state = _placement(dims)
    L = random_L(dims, absent=(n_probes(dims) - 1,) if n_probes(dims) > 1 else ())
    occ = np.random.default_rng(8).random((len(pos), 8)) < 0.2
    absent = replay_absent_mask(ORIGIN, STEP, dims, offsets, state, pos, nrm)
    grid = make_grid(rc, dims)
    for occluded in (None, occ):
        E, W = rc.shade_probes_placed_host(grid, offsets, state, L, pos, nrm, occluded)
        want = replay_blend(dims, L, pos, nrm, absent if occluded is None else absent | occluded)
        assert same_bits(E, want[0]) and same_bits(W, want[1])
    if n_probes(dims) > 1:
        assert not same_bits(W, rc.shade_probes_host(grid, L, pos, nrm, occ)[1])
    # the offsets alone do not show in the blend; RT_PROBE_IDLE does not either
    E2, W2 = rc.shade_probes_placed_host(grid, None, state & INSIDE, L, pos, nrm, occ)
    finite = np.where(np.isfinite(offsets).all(axis=1, keepdims=True), offsets, 0.0)
    E3, W3 = rc.shade_probes_placed_host(grid, finite, state, L, pos, nrm, occ)
    assert same_bits(E2, E3) and same_bits(W2, W3)


@pytest.mark.parametrize("wrap", [False, True])
@pytest.mark.parametrize("dims", GRIDS)
def test_h3_placed_depth_twin_against_the_replay(rc, dims, wrap):
    pos, nrm = points(dims)
    offsets, state = _placement(dims)
    L = random_L(dims, absent=(n_probes(dims) - 1,) if n_probes(dims) > 1 else ())
    D = random_D(n_probes(dims))
    grid = make_grid(rc, dims, visibility=False)
    P = rc.probe_depth_params(D_MAX, 5, FLOOR, wrap)
    E, W = rc.shade_probes_depth_placed_host(grid, offsets, state, L, D, P, pos, nrm)
    want = replay_shade_depth_placed(ORIGIN, STEP, dims, BIAS, D_MAX, FLOOR, wrap, offsets, state, L, D, pos, nrm)
    assert same_bits(E, want[0]) and same_bits(W, want[1])
    plain = rc.shade_probes_depth_host(grid, L, D, P, pos, nrm)
    assert (W > 0).sum() > 50 and not same_bits(W, plain[1])  # (the offsets move distances and texels)
    for o, s in ((offsets, None), (None, state)):
        E1, W1 = rc.shade_probes_depth_placed_host(grid, o, s, L, D, P, pos, nrm)
        want = replay_shade_depth_placed(ORIGIN, STEP, dims, BIAS, D_MAX, FLOOR, wrap, o, s, L, D, pos, nrm)
        assert same_bits(E1, want[0]) and same_bits(W1, want[1])


@pytest.mark.parametrize("dims", GRIDS)
def test_h3_promise_2_no_placement_is_the_unplaced_entry(rc, dims):
    pos, nrm = points(dims)
    L = random_L(dims, absent=(0,) if n_probes(dims) > 1 else ())
    D = random_D(n_probes(dims))
    occ = np.random.default_rng(8).random((len(pos), 8)) < 0.2
    n = n_probes(dims)
    vis, flat = make_grid(rc, dims), make_grid(rc, dims, visibility=False)
    P = rc.probe_depth_params(D_MAX, 5, FLOOR, True)
    seg = rc.probe_segments_host(vis, pos, nrm)
    blend = rc.shade_probes_host(vis, L, pos, nrm, occ)
    depth = rc.shade_probes_depth_host(flat, L, D, P, pos, nrm)
    for o, s in ((None, None), (np.zeros((n, 3)), np.zeros(n, np.uint32)), (np.zeros((n, 3)), None), (None, np.full(n, IDLE, np.uint32))):
        got = rc.probe_segments_placed_host(vis, o, s, pos, nrm)
        assert same_bits(got[0], seg[0]) and same_bits(got[1], seg[1])
        got = rc.shade_probes_placed_host(vis, o, s, L, pos, nrm, occ)
        assert same_bits(got[0], blend[0]) and same_bits(got[1], blend[1])
        got = rc.shade_probes_depth_placed_host(flat, o, s, L, D, P, pos, nrm)
        assert same_bits(got[0], depth[0]) and same_bits(got[1], depth[1])
    assert blend[1].any() and depth[1].any() and seg[1].any()


# ---------------------------------------------------------------- H4: argument errors
def test_h4_argument_errors_touch_nothing(rc):
    lib = rc.load_library()
    names, grid, rays, hits, offsets = _forced(rc)
    n = len(names)
    v = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None  # noqa: E731
    o, info = np.full((n, 3), 7.0), np.full(n * 16, 7, np.uint32)
    good = _params(rc)

    def relocate(g, p, spp=SPP, r_=rays, h_=hits, o_=o, i_=info):
        g, p = (C.byref(x) if x is not None else None for x in (g, p))
        yield "rt_debug_probe_relocate", lib.rt_debug_probe_relocate(g, p, v(r_), v(h_), spp, v(o_), v(i_))

    def bad(**kw):
        par = _params(rc)
        for name, value in kw.items():
            setattr(par, name, value)
        return par

    bad_params = {"share negative": bad(back_share=-0.01), "share 1": bad(back_share=1.0), "share NaN": bad(back_share=math.nan),
                  "front 0": bad(min_front=0.0), "front negative": bad(min_front=-1.0), "front inf": bad(min_front=math.inf),
                  "front NaN": bad(min_front=math.nan), "max 0": bad(max_offset=0.0), "max 0.5": bad(max_offset=0.5),
                  "max NaN": bad(max_offset=math.nan), "flag bits": bad(flags=2), "reserved": bad(reserved=1), "null": None}
    for what, par in bad_params.items():
        for name, status in relocate(grid, par):
            assert status == -1 and name + ":" in _last_error(lib), what
        # a null scene is refused first, before the params are looked at
        assert lib.rt_relocate_probes_device(None, C.byref(grid), C.byref(par) if par is not None else None, SPP, 1, 0, 0, v(o), v(info),
                                             None) == -1 and "null scene" in _last_error(lib)
    bad_grids = {"null grid": None}
    for what, (field, at, value) in {"step 0": ("step", 1, 0.0), "origin inf": ("origin", 0, math.inf), "dims 0": ("dims", 2, 0),
                                     "reserved": ("reserved", 1, 1)}.items():
        g = rc.probe_grid(R_ORIGIN, R_STEP, (n, 1, 1), False)
        getattr(g, field)[at] = value
        bad_grids[what] = g
    g = rc.probe_grid(R_ORIGIN, R_STEP, (n, 1, 1), False)
    g.flags = 2
    bad_grids["flags 2"] = g
    pos, nrm = points(GRIDS[0])
    pts = rc._pack_surfels(pos[:4], nrm[:4])
    L, D = random_L(GRIDS[0]), random_D(n_probes(GRIDS[0]))
    E, W = np.full((4, 3), 7.0), np.full(4, 7.0)
    seg_r, seg_t = np.full((4, 8, 8), 7.0), np.full((4, 8), 7.0)
    probes = np.full((n_probes(GRIDS[0]), 8), 7.0)
    P = rc.probe_depth_params(D_MAX, 5, FLOOR)

    def shade(g, p=P, n=4, L_=L, D_=D, pts_=pts, E_=E, r_=seg_r, flat=None):
        gd = g if flat is None else flat  # (the depth entries take a grid without flags)
        g, gd, p = (C.byref(x) if x is not None else None for x in (g, gd, p))
        yield "rt_debug_probe_segments_placed", lib.rt_debug_probe_segments_placed(g, None, None, v(pts_), n, v(r_), v(seg_t))
        yield "rt_debug_probe_segments_placed_device", lib.rt_debug_probe_segments_placed_device(g, None, None, v(pts_), n, v(r_), v(seg_t), None)
        yield "rt_debug_shade_probes_placed", lib.rt_debug_shade_probes_placed(g, None, None, v(L_), v(pts_), n, None, v(E_), v(W))
        yield "rt_debug_shade_probes_depth_placed", lib.rt_debug_shade_probes_depth_placed(gd, None, None, p, v(L_), v(D_), v(pts_), n, v(E_), v(W))
        # (these end in the argument checks: the device entries are never given host memory to launch over)
        yield "rt_shade_probes_depth_placed_device", lib.rt_shade_probes_depth_placed_device(gd, None, None, p, v(L_), v(D_), v(pts_), n, v(E_), v(W), None)

    for what, g in bad_grids.items():
        for name, status in relocate(g, good):
            assert status == -1 and name + ":" in _last_error(lib), what
        for count in (4, 0):
            for name, status in shade(g, n=count):
                assert status == -1 and name + ":" in _last_error(lib), (what, name)
        for status in (lib.rt_debug_probe_positions(C.byref(g) if g is not None else None, None, v(probes)),
                       lib.rt_probe_positions_device(C.byref(g) if g is not None else None, None, v(probes), None)):
            assert status == -1 and "rt_" in _last_error(lib), what
    vis, flat = make_grid(rc, GRIDS[0]), make_grid(rc, GRIDS[0], visibility=False)
    assert lib.rt_debug_shade_probes_depth_placed(C.byref(vis), None, None, C.byref(P), v(L), v(D), v(pts), 4, v(E), v(W)) == -1
    assert "RT_PROBE_GRID_VISIBILITY" in _last_error(lib)
    for par in (None, rc.probe_depth_params(0.0), rc.probe_depth_params(1.0, 9)):
        par = C.byref(par) if par is not None else None
        assert lib.rt_debug_shade_probes_depth_placed(C.byref(flat), None, None, par, v(L), v(D), v(pts), 4, v(E), v(W)) == -1
        assert "rt_debug_shade_probes_depth_placed:" in _last_error(lib)
        assert lib.rt_shade_probes_depth_placed_device(C.byref(flat), None, None, par, v(L), v(D), v(pts), 4, v(E), v(W), None) == -1
        assert "rt_shade_probes_depth_placed_device:" in _last_error(lib)
    for kw in (dict(n=-1), dict(pts_=None), dict(E_=None, r_=None), dict(L_=None, D_=None, r_=None)):
        for name, status in shade(vis, flat=flat, **kw):
            assert status == -1 and ("n < 0" if "n" in kw else "null pointer") in _last_error(lib), (kw, name)
    for name, status in shade(vis, n=0, L_=None, D_=None, pts_=None, E_=None, r_=None, flat=flat):
        assert status == 0, name
    for kw in (dict(spp=0), dict(spp=-3), dict(spp=(1 << 19) + 1), dict(r_=None), dict(h_=None), dict(o_=None), dict(i_=None)):
        for name, status in relocate(grid, good, **kw):
            assert status == -1 and name + ":" in _last_error(lib), kw
    assert "2^19" in [_last_error(lib) for _ in relocate(grid, good, spp=(1 << 19) + 1)][0]
    assert lib.rt_debug_probe_positions(C.byref(flat), None, None) == -1 and lib.rt_probe_positions_device(C.byref(flat), None, None, None) == -1
    for status in (lib.rt_shade_probes_placed(None, C.byref(vis), None, None, v(L), v(pts), 4, v(E), v(W)),
                   lib.rt_shade_probes_placed_device(None, C.byref(vis), None, None, v(L), v(pts), 4, v(E), v(W), None)):
        assert status == -1 and "null scene" in _last_error(lib)
    for a in (o, E, W, seg_r, seg_t, probes):
        assert (a == 7.0).all()
    assert (info == 7).all()
    # the wrappers' own checks
    with pytest.raises(ValueError):
        rc.probe_relocate_host(grid, good, rays[:-1], hits[:-1], offsets)
    with pytest.raises(ValueError):
        rc.probe_relocate_host(grid, good, rays, hits, offsets[:-1])
    with pytest.raises(ValueError):
        rc.shade_probes_placed_host(vis, np.zeros((3, 3)), None, L, pos[:4], nrm[:4])
    with pytest.raises(ValueError):
        rc.shade_probes_depth_placed_host(flat, None, np.zeros(3, np.uint32), L, D, P, pos[:4], nrm[:4])


# ---------------------------------------------------------------- H5: layout and memory
def test_h5_layout_as_a_c_compiler_sees_it(rc, tmp_path):
    exe = str(tmp_path / "probe_relocate_layout")
    subprocess.run(["cc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "host", "probe_relocate_layout.c"), "-o", exe], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    assert out.split("\n")[:3] == ["32 0 8 16 24 28", "64 0 4 20 24 36 40 56", "1 2 1"]
    assert C.sizeof(rc.rt_probe_relocate_params) == 32
    assert [getattr(rc.rt_probe_relocate_params, f).offset for f in ("back_share", "min_front", "max_offset", "flags", "reserved")] == [0, 8, 16, 24, 28]
    dt = rc.RELOCATION_DTYPE
    assert dt.itemsize == 64 and [dt.fields[f][1] for f in ("state", "moved", "skipped", "k_near", "reserved", "d_near", "d_far")] == [0, 4, 20, 24, 36, 40, 56]
    assert (rc.RT_PROBE_INSIDE, rc.RT_PROBE_IDLE, rc.RT_PROBE_RELOCATE_CLASSIFY_ONLY) == (1, 2, 1) == (INSIDE, IDLE, CLASSIFY_ONLY)
    assert rc.ABI_VERSION == 6 == rc.load_library().rt_abi_version()  # additive: detected by symbol


def test_h5_host_check_under_sanitizers(rc):
    """tests/host/probe_relocate_host_check.cpp, a stand-alone program built with AddressSanitizer and UBSan over
    the library's host code, run on the CPU: the five twins on exact-size heap arrays, and their argument errors."""
    subprocess.run(["make", "-s", "-C", CSRC, "-j" + str(min(16, os.cpu_count() or 8)), "probe_relocate_host_check_asan"], check=True)
    out = subprocess.run([os.path.join(CSRC, "_obj_asan", "probe_relocate_host_check")], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "probe_relocate_host_check: ok" in out.stdout


# ---------------------------------------------------------------- the binding
def test_exported_and_bound(rc):
    lib = rc.load_library()
    out = subprocess.run(["nm", "-D", "--defined-only", rc.LIB_PATH], capture_output=True, text=True).stdout
    for name in NAMES:
        assert f" T {name}\n" in out
        assert getattr(lib, name).argtypes is not None
    for name in ("relocate_probes", "relocate_probes_device", "probe_positions", "shade_probes_placed_device",
                 "probe_segments_placed_device"):
        assert hasattr(rc.GpuRaytracer, name)
    for name in ("probe_relocate_params", "probe_positions_host", "probe_positions_device", "probe_relocate_host",
                 "probe_segments_placed_host", "shade_probes_placed_host", "shade_probes_depth_placed_host",
                 "shade_probes_depth_placed_device"):
        assert callable(getattr(rc, name))
    par = rc.probe_relocate_params(0.2)
    assert (par.back_share, par.min_front, par.max_offset, par.flags, par.reserved) == (0.25, 0.2, 0.45, 0, 0)
    assert rc.probe_relocate_params(0.2, classify_only=True).flags == 1
    header = open(os.path.join(ROOT, "include", "rtcore.h")).read()
    top = header[:header.index("typedef enum rt_status")]
    for name in list(NAMES) + ["rt_probe_relocate_params", "rt_probe_relocation"]:
        assert name in top, name  # the list of what version 6 gained


@pytest.mark.parametrize("name", list(NAMES))
def test_ctypes_prototype_matches_the_header(rc, name):
    fn = getattr(rc.load_library(), name)
    ret, params = _header_prototype(name)
    assert ret == "int" and fn.restype is C.c_int
    assert len(params) == len(fn.argtypes) == NAMES[name]
    sizes = {"rt_probe_depth_params": 32, "rt_probe_grid": 80, "rt_probe_relocate_params": 32}
    for ctype, bound in zip(params, fn.argtypes):
        if ctype.endswith("*"):
            assert bound is C.c_void_p or issubclass(bound, C._Pointer), (ctype, bound)
            if bound is not C.c_void_p:
                assert C.sizeof(bound._type_) == sizes[ctype.rstrip("*").replace("const", "").strip()], (ctype, bound)
        else:
            assert bound is SCALARS[ctype], (ctype, bound)
