"""Probe depth maps, host side (no GPU): include/rtcore.h's "probe depth maps" restated in plain Python loops
(tests/probe_depth_cases.py) and held to the host twins bit for bit: the texel rules (H1), the fold and its
a + b promise (H2), the close (H3), the shading against the replay and against rt_debug_shade_probes (H4),
known answers (H5), the argument errors (H6), the records' layout and the twins under sanitizers (H7), the
binding.  tests/test_probe_depth_gpu.py holds the device to the twins."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

from probe_depth_cases import (random_D, replay_close, replay_fold, replay_shade, replay_texel, replay_texel_dir, same_bits,
                               synthetic_samples)
from test_render_rays_host import SCALARS, _header_prototype, _last_error
from test_shade_probes_host import BIAS, GRIDS, N, ORIGIN, STEP, make_grid, n_probes, points, random_L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "raytracercore_amd", "csrc")
NAMES = {"rt_render_probe_depth_device": 11, "rt_debug_probe_depth_fold": 7, "rt_probe_depth_close_device": 4,
         "rt_debug_probe_depth_close": 3, "rt_shade_probes_depth_device": 9, "rt_debug_shade_probes_depth": 8,
         "rt_debug_oct_texel_dirs": 1, "rt_debug_oct_texel": 3}
D_MAX, FLOOR = 1.0, 1e-3  # (the grids' probes are 0.5 .. 1.25 apart: distances on both sides of d_max)


def _params(rc, d_max=D_MAX, sharpness=5, var_floor=FLOOR, wrap=False):
    return rc.probe_depth_params(d_max, sharpness, var_floor, wrap)


# ---------------------------------------------------------------- H1: the texel rules
def test_h1_every_texel_direction_maps_back_to_its_texel(rc):
    T = rc.oct_texel_dirs()
    assert T.shape == (64, 3) and np.abs(np.linalg.norm(T, axis=1) - 1).max() < 1e-15
    assert np.array_equal(rc.oct_texel(T), np.arange(64))
    twin = rc.oct_texel_dirs_host()
    assert same_bits(twin, T)
    assert same_bits(twin, np.array([replay_texel_dir(t) for t in range(64)]))
    assert np.array_equal(rc.oct_texel_host(twin), np.arange(64))
    # a texel's direction lies strictly inside it: scaled, it is still the texel's
    assert np.array_equal(rc.oct_texel_host(twin * 1e-200), np.arange(64)) and np.array_equal(rc.oct_texel_host(twin * 3e150), np.arange(64))
    assert (T[[27, 28, 35, 36], 2] > 0).all() and (T[[0, 7, 56, 63], 2] < 0).all()  # (the square's middle looks up, its corners down)


def test_h1_axes_and_negative_zero_follow_the_sgn_rule(rc):
    nz = -0.0
    cases = {(0, 0, 1): 36, (1, 0, 0): 39, (-1, 0, 0): 32, (0, 1, 0): 60, (0, -1, 0): 4,
             (0, 0, -1): 63, (nz, nz, -1): 63, (nz, 0, -1): 63,  # sgn(-0.0) = 1: the (+, +) corner
             (-1e-300, 0, -1): 56, (0, -1e-300, -1): 7,       # a negative component, however small, picks its own corner
             (1, nz, 0): 39, (nz, 1, nz): 60, (1, 1, nz): 54, (-1, -1, -0.0): 18, (2, 2, -4): 63, (3, -1, -4): 15}
    v = np.array([list(map(float, k)) for k in cases])
    want = np.array(list(cases.values()), np.int32)
    assert np.array_equal(np.array([replay_texel(*row) for row in v]), want)
    assert np.array_equal(rc.oct_texel_host(v), want)
    assert np.array_equal(rc.oct_texel(v), want)


def test_h1_twin_matches_the_replay_on_random_vectors(rc):
    rng = np.random.default_rng(2)
    v = rng.normal(size=(2000, 3)) * np.exp(rng.normal(size=(2000, 1)) * 20)
    v[::7, 2] = -np.abs(v[::7, 2])
    v[::11, 0] = 0.0
    v[::13, 1] = -0.0
    # on texel borders: multiples of 1/4 in (u, v) with a 1-norm of 1
    u = rng.integers(-4, 5, 400) / 4.0
    w = (1 - np.abs(u)) * rng.choice([-1.0, 1.0], 400) * rng.integers(0, 5, 400) / 4.0
    border = np.stack([u, w, (1 - np.abs(u) - np.abs(w)) * rng.choice([-1.0, 1.0], 400)], axis=1)
    border = border[np.abs(border).sum(axis=1) > 0]
    v = np.concatenate([v, border])
    got = rc.oct_texel_host(v)
    assert np.array_equal(got, np.array([replay_texel(*(float(x) for x in row)) for row in v]))
    assert np.array_equal(got, rc.oct_texel(v))
    assert len(np.unique(got)) == 64
    assert np.array_equal(rc.oct_texel_host(np.array([[0.0, 0.0, 0.0], [np.nan, 1, 0], [1, np.inf, 0], [0, -0.0, 0]])), [-1] * 4)


# ---------------------------------------------------------------- H2: the fold
@pytest.mark.parametrize("sharpness", [0, 5, 8])
def test_h2_fold_twin_against_the_replay(rc, sharpness):
    d_max = 1.5
    rays, hits = synthetic_samples(rc, d_max=d_max)
    assert rays.shape == (3, 5)
    start = np.random.default_rng(6).uniform(0, 2, (3, 3, 64))  # (added to what the arrays hold)
    depth, counts = start.copy(), np.array([[1, 0, 2, 3]] * 3, np.uint32)
    want_d, want_c = start.copy(), counts.copy()
    got = rc.probe_depth_fold_host(_params(rc, d_max, sharpness), rays, hits, out=(depth, counts))
    replay_fold(d_max, sharpness, rays, hits, want_d, want_c)
    assert got[0] is depth and same_bits(depth, want_d) and same_bits(counts, want_c)
    assert np.array_equal(counts - np.array([1, 0, 2, 3], np.uint32), [[4, 0, 1, 0], [4, 1, 0, 1], [5, 0, 0, 0]])
    assert not same_bits(depth, start) and np.isfinite(depth).all()
    if sharpness == 0:  # w = c: the lower half-space of a texel adds nothing, the upper adds its cosine
        fresh, _ = rc.probe_depth_fold_host(_params(rc, d_max, 0), rays[:1, :1], hits[:1, :1])
        cs = rc.oct_texel_dirs() @ rays["direction"][0, 0, :3]
        assert np.array_equal(fresh[0, 0] > 0, cs > 0) and np.abs(fresh[0, 0] - np.maximum(cs, 0)).max() < 1e-15


def test_h2_fold_of_a_plus_b_samples_is_a_then_b(rc):
    rays, hits = synthetic_samples(rc, n=3, spp=5)
    P = _params(rc, 1.5, 5)
    whole = rc.probe_depth_fold_host(P, rays, hits)
    for a in (1, 2, 4):
        acc = rc.probe_depth_fold_host(P, rays[:, :a], hits[:, :a])
        acc = rc.probe_depth_fold_host(P, rays[:, a:], hits[:, a:], out=acc)
        assert same_bits(acc[0], whole[0]) and same_bits(acc[1], whole[1]), a
    # a probe's sums do not depend on its neighbours
    one = rc.probe_depth_fold_host(P, rays[1:2], hits[1:2])
    assert same_bits(one[0][0], whole[0][1]) and same_bits(one[1][0], whole[1][1])


def test_h2_distances_are_held_to_d_max(rc):
    rays, hits = (a[2:] for a in synthetic_samples(rc))  # (the probe with five plain hits)
    far = hits.copy()
    far["distance"] = 100.0
    missed = hits.copy()
    missed["prim_id"] = -1
    P = _params(rc, 1.5, 2)
    a, ca = rc.probe_depth_fold_host(P, rays, far)
    b, cb = rc.probe_depth_fold_host(P, rays, missed)
    assert same_bits(a, b) and ca[0, 0] == 5 and cb[0, 2] == 5
    D = rc.probe_depth_close_host(a)
    has = a[0, 0] > 0
    assert has.any() and np.abs(D[0, has, 0] - 1.5).max() < 1e-14 and np.abs(D[0, has, 1] - 2.25).max() < 1e-14


# ---------------------------------------------------------------- H3: the close
def test_h3_close_twin_and_absent_texels(rc):
    rng = np.random.default_rng(9)
    depth = rng.uniform(0.1, 5, (4, 3, 64))
    depth[0, 0, 5] = 0.0
    depth[1, 0, :] = 0.0
    depth[2, 0, 7] = -1.0
    depth[3, 0, 9] = np.nan
    D = rc.probe_depth_close_host(depth)
    assert same_bits(D, replay_close(depth))
    gone = np.zeros((4, 64), bool)
    gone[0, 5] = gone[1, :] = gone[2, 7] = gone[3, 9] = True
    assert np.isnan(D[gone]).all() and np.isfinite(D[~gone]).all()
    assert same_bits(D[~gone][:, 0], depth[:, 1][~gone] / depth[:, 0][~gone])
    assert rc.probe_depth_close_host(np.zeros((0, 3, 64))).shape == (0, 64, 2)


# ---------------------------------------------------------------- H4: the shading
@pytest.mark.parametrize("wrap", [False, True])
@pytest.mark.parametrize("dims", GRIDS)
def test_h4_shade_twin_against_the_replay(rc, dims, wrap):
    pos, nrm = points(dims)
    assert len(pos) == N == 200
    L = random_L(dims, absent=(n_probes(dims) - 1,) if n_probes(dims) > 1 else ())
    D = random_D(n_probes(dims))
    assert np.isnan(D).any() and np.isfinite(D).any()
    grid = make_grid(rc, dims, visibility=False)
    E, W = rc.shade_probes_depth_host(grid, L, D, _params(rc, wrap=wrap), pos, nrm)
    want_E, want_W = replay_shade(ORIGIN, STEP, dims, BIAS, D_MAX, FLOOR, wrap, L, D, pos, nrm)
    assert same_bits(E, want_E) and same_bits(W, want_W)
    flat = rc.shade_probes_host(grid, L, pos, nrm)
    assert (W > 0).sum() > 100 and not same_bits(W, flat[1])  # (the test weighs something down)
    if not wrap:
        assert (W <= flat[1]).all() and (W[flat[1] > 0] > 0).all()  # a Chebyshev weight is in (0, 1]


@pytest.mark.parametrize("dims", GRIDS)
def test_h4_absent_maps_without_wrap_are_the_plain_blend(rc, dims):
    """Promise 3: with every texel absent and no wrap flag the result is rt_debug_shade_probes with occluded =
    NULL on the same grid, bit for bit."""
    pos, nrm = points(dims)
    L = random_L(dims, absent=(0,) if n_probes(dims) > 1 else ())
    grid = make_grid(rc, dims, visibility=False)
    D = np.full((n_probes(dims), 64, 2), np.nan)
    E, W = rc.shade_probes_depth_host(grid, L, D, _params(rc), pos, nrm)
    want = rc.shade_probes_host(grid, L, pos, nrm, None)
    assert same_bits(E, want[0]) and same_bits(W, want[1]) and W.any()
    # a texel one of whose values is not finite is absent too; and a mean no point reaches changes nothing
    for D2 in (np.stack([np.full((n_probes(dims), 64), 0.3), np.full((n_probes(dims), 64), np.inf)], axis=-1),
               np.full((n_probes(dims), 64, 2), 1e6)):
        E2, W2 = rc.shade_probes_depth_host(grid, L, D2, _params(rc), pos, nrm)
        assert same_bits(E2, want[0]) and same_bits(W2, want[1])


# ---------------------------------------------------------------- H5: known answers
def test_h5_one_probe_a_point_beyond_and_a_point_before_the_mean(rc):
    """A 1 x 1 x 1 grid, mu = 1 and m2 = 1 in every texel (variance 0: the floor f works), d_max = 4.  A point at
    distance 2: c = (f / (f + 1))^3, and W = c since the one corner has t_c = 1; E is the plain blend's, the
    weight divided out again.  A point at distance 0.5 is nearer than the mean: W = 1 exactly."""
    grid = make_grid(rc, (1, 1, 1), visibility=False, bias=0.0)
    L = random_L((1, 1, 1), seed=12)
    D = np.ones((1, 64, 2))
    rng = np.random.default_rng(14)
    u = rng.normal(size=(40, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    nrm = rng.normal(size=(40, 3))
    for f in (1e-3, 0.25, 7.0):
        P = _params(rc, 4.0, 5, f)
        # (2 u and u / 2 are exact; the distance is 2 or 0.5 to within an ulp, far from the mean either way)
        E, W = rc.shade_probes_depth_host(grid, L, D, P, np.array(ORIGIN) + 2.0 * u, nrm)
        q = f / (f + 1.0 * 1.0)
        c = (q * q) * q
        assert np.abs(W / c - 1).max() < 1e-14, f
        axis = np.array(ORIGIN) + np.array([[2.0, 0, 0], [0, -2.0, 0], [0, 0, 2.0]])  # (exactly 2 away)
        Ea, Wa = rc.shade_probes_depth_host(grid, L, D, P, axis, nrm[:3])
        assert (Wa == c).all(), f
        flat = rc.shade_probes_host(grid, L, np.array(ORIGIN) + 2.0 * u, nrm)
        # (nine terms of at most 1.03 |L| each, two more roundings per term and one for the division: 4e-15 |L|)
        assert (flat[1] == 1.0).all() and np.abs(E - flat[0]).max() <= 1e-13 * np.abs(L).max()
        E1, W1 = rc.shade_probes_depth_host(grid, L, D, P, np.array(ORIGIN) + 0.5 * u, nrm)
        assert (W1 == 1.0).all() and same_bits(E1, rc.shade_probes_host(grid, L, np.array(ORIGIN) + 0.5 * u, nrm)[0])
    # d_max holds the point's distance too: at d_max = 1 a point at 2 is not beyond a mean of 1
    assert (rc.shade_probes_depth_host(grid, L, D, _params(rc, 1.0), np.array(ORIGIN) + 2.0 * u, nrm)[1] == 1.0).all()


def test_h5_wrap_weight_for_three_normals(rc):
    """The wrap weight alone (absent maps): 1.2 for a normal that faces the probe, 0.2 for one that faces away,
    0.45 sideways; and 1 for a point on the probe."""
    grid = make_grid(rc, (1, 1, 1), visibility=False, bias=0.0)
    L = random_L((1, 1, 1), seed=12)
    D = np.full((1, 64, 2), np.nan)
    at = np.array(ORIGIN) + np.array([1.0, 0.0, 0.0])
    pos = np.array([at, at, at, at, np.array(ORIGIN)])
    nrm = np.array([[-3.0, 0, 0], [0.5, 0, 0], [0, 2.0, 0], [0, 0, -1.0], [0, 0, 1.0]])
    E, W = rc.shade_probes_depth_host(grid, L, D, _params(rc, wrap=True), pos, nrm)
    assert W.tolist() == [1.0 * 1.0 + 0.2, 0.0 * 0.0 + 0.2, 0.5 * 0.5 + 0.2, 0.5 * 0.5 + 0.2, 1.0]
    assert np.abs(W - [1.2, 0.2, 0.45, 0.45, 1.0]).max() < 1e-15
    flat = rc.shade_probes_host(grid, L, pos, nrm)
    assert np.abs(E - flat[0]).max() <= 1e-13 * np.abs(L).max()  # one corner: the weight divides out (H5's bound)
    assert (rc.shade_probes_depth_host(grid, L, D, _params(rc), pos, nrm)[1] == 1.0).all()


# ---------------------------------------------------------------- H6: argument errors
def _bad_params(rc):
    def p(**kw):
        par = _params(rc)
        for name, value in kw.items():
            if name == "reserved":
                par.reserved[value] = 1
            else:
                setattr(par, name, value)
        return par

    return {"d_max 0": p(d_max=0.0), "d_max negative": p(d_max=-1.0), "d_max NaN": p(d_max=math.nan), "d_max inf": p(d_max=math.inf),
            "floor 0": p(var_floor=0.0), "floor NaN": p(var_floor=math.nan), "floor inf": p(var_floor=math.inf),
            "sharpness -1": p(sharpness=-1), "sharpness 9": p(sharpness=9), "flag bits": p(flags=2), "flag bits 3": p(flags=3),
            "reserved 0": p(reserved=0), "reserved 1": p(reserved=1)}


def test_h6_argument_errors_touch_nothing(rc):
    lib = rc.load_library()
    dims = GRIDS[0]
    pos, nrm = points(dims)
    pts = rc._pack_surfels(pos[:4], nrm[:4])
    L, D = random_L(dims), random_D(n_probes(dims))
    E, W = np.full((4, 3), 7.0), np.full(4, 7.0)
    rays, hits = synthetic_samples(rc)
    depth, counts, closed = np.full((3, 3, 64), 7.0), np.full((3, 4), 7, np.uint32), np.full((3, 64, 2), 7.0)
    v = lambda a: a.ctypes.data_as(C.c_void_p)
    good_g, good_p = make_grid(rc, dims, visibility=False), _params(rc)

    def shade(g, p, n=4, L_=v(L), D_=v(D), pts_=v(pts), E_=v(E)):
        g, p = (C.byref(x) if x is not None else None for x in (g, p))
        yield "rt_debug_shade_probes_depth", lib.rt_debug_shade_probes_depth(g, p, L_, D_, pts_, n, E_, v(W))
        # (ends in the argument checks: the device entry is never given host memory to launch over)
        yield "rt_shade_probes_depth_device", lib.rt_shade_probes_depth_device(g, p, L_, D_, pts_, n, E_, v(W), None)

    def fold(p, n=3, spp=5, r_=v(rays), h_=v(hits), d_=v(depth), c_=v(counts)):
        return lib.rt_debug_probe_depth_fold(C.byref(p) if p is not None else None, r_, h_, n, spp, d_, c_)

    for what, par in list(_bad_params(rc).items()) + [("null params", None)]:
        for name, status in shade(good_g, par):
            assert status == -1 and name + ":" in _last_error(lib), (what, name)
        assert fold(par) == -1 and "rt_debug_probe_depth_fold:" in _last_error(lib), what
        assert lib.rt_render_probe_depth_device(None, v(pts), 4, 5, 0, 0, 0, C.byref(par) if par is not None else None, v(depth),
                                                v(counts), None) == -1 and "null scene" in _last_error(lib)
    bad_grids = {"visibility flag": make_grid(rc, dims, visibility=True), "null grid": None}
    for what, (field, at, value) in {"step 0": ("step", 1, 0.0), "origin inf": ("origin", 0, math.inf), "dims 0": ("dims", 2, 0),
                                     "reserved": ("reserved", 1, 1)}.items():
        g = make_grid(rc, dims, visibility=False)
        getattr(g, field)[at] = value
        bad_grids[what] = g
    for field, value in (("bias", -1.0), ("bias", math.nan), ("flags", 2)):
        g = make_grid(rc, dims, visibility=False)
        setattr(g, field, value)
        bad_grids[f"{field} {value}"] = g
    for what, g in bad_grids.items():
        for n in (4, 0):  # (a bad grid is an error at n == 0 too: it is checked first)
            for name, status in shade(g, good_p, n):
                assert status == -1 and name + ":" in _last_error(lib), (what, name)
    for name, status in shade(bad_grids["visibility flag"], good_p):
        assert "RT_PROBE_GRID_VISIBILITY" in _last_error(lib)
    for kw in (dict(n=-1), dict(L_=None), dict(D_=None), dict(pts_=None), dict(E_=None)):
        for name, status in shade(good_g, good_p, **kw):
            assert status == -1 and ("n < 0" if "n" in kw else "null pointer") in _last_error(lib), (kw, name)
    for name, status in shade(good_g, good_p, 0, None, None, None, None):
        assert status == 0, name
    for kw in (dict(n=-1), dict(spp=0), dict(spp=-2), dict(r_=None), dict(h_=None), dict(d_=None), dict(c_=None)):
        assert fold(good_p, **kw) == -1, kw
    assert fold(good_p, 0, 5, None, None, None, None) == 0
    assert lib.rt_debug_probe_depth_close(None, 3, v(closed)) == -1 and lib.rt_debug_probe_depth_close(v(depth), 3, None) == -1
    assert lib.rt_debug_probe_depth_close(v(depth), -1, v(closed)) == -1 and "rt_debug_probe_depth_close:" in _last_error(lib)
    assert lib.rt_probe_depth_close_device(None, 3, None, None) == -1 and lib.rt_probe_depth_close_device(v(depth), -1, v(closed), None) == -1
    assert lib.rt_probe_depth_close_device(v(depth), 1 << 25, v(closed), None) == -1
    assert lib.rt_debug_probe_depth_close(None, 0, None) == 0 and lib.rt_probe_depth_close_device(None, 0, None, None) == 0
    assert (E == 7.0).all() and (W == 7.0).all() and (depth == 7.0).all() and (counts == 7).all() and (closed == 7.0).all()
    # the wrappers' own checks
    with pytest.raises(ValueError):
        rc.shade_probes_depth_host(good_g, L, D[:-1], good_p, pos[:4], nrm[:4])
    with pytest.raises(ValueError):
        rc.shade_probes_depth_host(good_g, L[:-1], D, good_p, pos[:4], nrm[:4])
    with pytest.raises(ValueError):
        rc.probe_depth_fold_host(good_p, rays, hits[:, :4])
    with pytest.raises(ValueError):
        rc.probe_depth_close_host(np.zeros((2, 3, 63)))


# ---------------------------------------------------------------- H7: layout and memory
def test_h7_layout_as_a_c_compiler_sees_it(rc, tmp_path):
    exe = str(tmp_path / "probe_depth_layout")
    subprocess.run(["cc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "host", "probe_depth_layout.c"), "-o", exe], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    assert out.strip() == "32 0 8 16 20 24 1536 512 1"
    assert C.sizeof(rc.rt_probe_depth_params) == 32
    assert [getattr(rc.rt_probe_depth_params, f).offset for f in ("d_max", "var_floor", "sharpness", "flags", "reserved")] == [0, 8, 16, 20, 24]
    assert rc.RT_PROBE_DEPTH_WRAP == 1
    assert rc.ABI_VERSION == 6 == rc.load_library().rt_abi_version()  # additive: detected by symbol


def test_h7_host_check_under_sanitizers(rc):
    """tests/host/probe_depth_host_check.cpp, a stand-alone program built with AddressSanitizer and UBSan over
    the library's host code, run on the CPU: the five twins on exact-size heap arrays, and their argument
    errors."""
    subprocess.run(["make", "-s", "-C", CSRC, "-j" + str(min(16, os.cpu_count() or 8)), "probe_depth_host_check_asan"], check=True)
    out = subprocess.run([os.path.join(CSRC, "_obj_asan", "probe_depth_host_check")], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "probe_depth_host_check: ok" in out.stdout


# ---------------------------------------------------------------- the binding
def test_exported_and_bound(rc):
    lib = rc.load_library()
    out = subprocess.run(["nm", "-D", "--defined-only", rc.LIB_PATH], capture_output=True, text=True).stdout
    for name in NAMES:
        assert f" T {name}\n" in out
        assert getattr(lib, name).argtypes is not None
    for name in ("render_probe_depth", "render_probe_depth_device", "shade_probes_depth"):
        assert hasattr(rc.GpuRaytracer, name)
    for name in ("probe_depth_params", "probe_depth_close_device", "probe_depth_close_host", "probe_depth_fold_host",
                 "shade_probes_depth_device", "shade_probes_depth_host", "oct_texel_dirs", "oct_texel", "probe_backface_share"):
        assert callable(getattr(rc, name))
    share = rc.probe_backface_share(np.array([[64, 64, 0, 0], [10, 0, 54, 0], [0, 0, 64, 0], [8, 2, 0, 56]], np.uint32))
    assert share[:2].tolist() == [1.0, 0.0] and np.isnan(share[2]) and share[3] == 0.25


@pytest.mark.parametrize("name", list(NAMES))
def test_ctypes_prototype_matches_the_header(rc, name):
    fn = getattr(rc.load_library(), name)
    ret, params = _header_prototype(name)
    assert ret == "int" and fn.restype is C.c_int
    assert len(params) == len(fn.argtypes) == NAMES[name]
    sizes = {"rt_probe_depth_params": 32, "rt_probe_grid": 80}
    for ctype, bound in zip(params, fn.argtypes):
        if ctype.endswith("*"):
            assert bound is C.c_void_p or issubclass(bound, C._Pointer), (ctype, bound)
            if bound is not C.c_void_p:
                assert C.sizeof(bound._type_) == sizes[ctype.rstrip("*").replace("const", "").strip()], (ctype, bound)
        else:
            assert bound is SCALARS[ctype], (ctype, bound)
