"""rt_shade_probes, host side (no GPU): include/rtcore.h's "probe grids" restated in plain Python loops, one
rounding per operation and in the stated order, and held to the three host twins bit for bit (H1 radiance,
H2 segments, H3 blend); the blend's properties on known answers (H4); the argument errors (H5); the record's
layout and the twins under sanitizers (H6); the binding.  tests/test_shade_probes_gpu.py holds the device to
the twins."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

from test_render_probes_host import basis
from test_render_rays_host import SCALARS, _header_prototype, _last_error

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "raytracercore_amd", "csrc")
NAMES = ("rt_probe_radiance_device", "rt_debug_probe_radiance", "rt_shade_probes_device", "rt_shade_probes",
         "rt_debug_probe_segments_device", "rt_debug_probe_segments", "rt_debug_shade_probes")
A_LOBE = [3.141592653589793] + [2.0943951023931953] * 3 + [0.7853981633974483] * 5
# origin, step and the bias are sums of a few powers of two, so probe positions, and the grid coordinate of a
# point placed on one, are exact
ORIGIN, STEP, BIAS = (-1.0, 0.5, 2.0), (0.5, 0.75, 1.25), 0.25
GRIDS = ((4, 3, 2), (1, 1, 1), (1, 3, 1))
N = 200
BAD = [7, 130, 64]  # test_render_surfels_gpu.BAD: a NaN position component, an infinite normal component, a zero normal
ON_PROBE = 150      # the point that the bias puts exactly on a probe


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def make_grid(rc, dims, visibility=True, bias=BIAS):
    return rc.probe_grid(ORIGIN, STEP, dims, visibility, bias)


def probe_position(dims, index):
    return np.array([ORIGIN[a] + index[a] * STEP[a] for a in range(3)])


def points(dims, seed=3):
    """The 200 points of H2: random ones, a third of them outside the grid on every side; [100, 120) at probe
    positions; [120, 150) on cell faces; ON_PROBE put on a probe by the bias; the three invalid ones."""
    rng = np.random.default_rng(seed)
    lo = np.array(ORIGIN)
    hi = probe_position(dims, [d - 1 for d in dims])
    span = np.maximum(hi - lo, np.array(STEP))
    pos = lo - 0.4 * span + rng.random((N, 3)) * 1.8 * span
    nrm = rng.normal(size=(N, 3)) * np.exp(rng.normal(size=(N, 1)))  # not unit
    for i in range(100, 150):
        index = [int(rng.integers(0, d)) for d in dims]
        at = probe_position(dims, index)
        if i < 120:
            pos[i] = at
        else:
            pos[i, (i - 120) % 3] = at[(i - 120) % 3]
    pos[ON_PROBE] = probe_position(dims, [d - 1 for d in dims]) - np.array([0.0, 0.0, BIAS])
    nrm[ON_PROBE] = (0.0, 0.0, 1.0)
    pos[BAD[0], 1] = np.nan
    nrm[BAD[1], 0] = np.inf
    nrm[BAD[2]] = 0.0
    return pos, nrm


# ---------------------------------------------------------------- the restatement (Python floats are IEEE doubles)
def replay_cell(dims, p, n):
    """rtcore.h, "Point", "Cell" and "Corners": None for an invalid point, else (n^, i, t[8])."""
    vals = [float(v) for v in p] + [1.0] + [float(v) for v in n] + [0.0]
    n2 = (vals[4] * vals[4] + vals[5] * vals[5]) + vals[6] * vals[6]
    if not all(math.isfinite(v) for v in vals) or n2 == 0.0 or not math.isfinite(n2):
        return None
    ln = math.sqrt(n2)
    nh = [vals[4] / ln, vals[5] / ln, vals[6] / ln]
    i, f = [0, 0, 0], [0.0, 0.0, 0.0]
    for a in range(3):
        if dims[a] == 1:
            continue
        g = (vals[a] - ORIGIN[a]) / STEP[a]
        g = 0.0 if g < 0.0 else float(dims[a] - 1) if g > dims[a] - 1 else g
        i[a] = min(int(g), dims[a] - 2)
        f[a] = g - float(i[a])
    t = []
    for c in range(8):
        w = [f[a] if (c >> a) & 1 else 1.0 - f[a] for a in range(3)]
        t.append((w[0] * w[1]) * w[2])
    return nh, i, t


def replay_segments(dims, pos, nrm, visibility=True, bias=BIAS):
    """rtcore.h, "Segment": (rays (n, 8, 2, 4), t_max (n, 8))."""
    n = len(pos)
    rays, t_max = np.zeros((n, 8, 2, 4)), np.zeros((n, 8))
    for k in range(n):
        cell = replay_cell(dims, pos[k], nrm[k])
        if cell is None or not visibility:
            continue
        nh, i, t = cell
        for c in range(8):
            if t[c] == 0.0:
                continue
            o = [float(pos[k][a]) + bias * nh[a] for a in range(3)]
            q = [ORIGIN[a] + float(i[a] + ((c >> a) & 1)) * STEP[a] for a in range(3)]
            v = [q[a] - o[a] for a in range(3)]
            dist = math.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
            if not dist > 0.0 or not math.isfinite(dist):
                continue
            rays[k, c, 0] = o + [1.0]
            rays[k, c, 1] = [v[0] / dist, v[1] / dist, v[2] / dist, 0.0]
            t_max[k, c] = dist
    return rays, t_max


def replay_blend(dims, L, pos, nrm, occluded=None):
    """rtcore.h, "Blend": (irradiance (n, 3), weight (n,)); L (n_probes, 9, 3), occluded (n, 8) or None."""
    n = len(pos)
    E, Wout = np.zeros((n, 3)), np.zeros(n)
    Lp = np.asarray(L, np.float64).reshape(-1, 27)
    for k in range(n):
        cell = replay_cell(dims, pos[k], nrm[k])
        if cell is None:
            continue
        nh, i, t = cell
        W, B = 0.0, [0.0] * 27
        for c in range(8):
            if t[c] == 0.0 or (occluded is not None and occluded[k][c]):
                continue
            ix, iy, iz = (i[a] + ((c >> a) & 1) for a in range(3))
            row = [float(v) for v in Lp[(iz * dims[1] + iy) * dims[0] + ix]]
            if not all(math.isfinite(v) for v in row):
                continue
            W = W + t[c]
            for j in range(27):
                B[j] = B[j] + t[c] * row[j]
        if not W > 0.0:
            continue
        Y = [float(v) for v in basis(np.array(nh))]
        a = [A_LOBE[l] * Y[l] for l in range(9)]
        for ch in range(3):
            e = a[0] * B[ch]
            for l in range(1, 9):
                e = e + a[l] * B[3 * l + ch]
            E[k, ch] = e / W
        Wout[k] = W
    return E, Wout


def n_probes(dims):
    return dims[0] * dims[1] * dims[2]


def random_L(dims, seed=5, absent=()):
    L = np.random.default_rng(seed).normal(size=(n_probes(dims), 9, 3))
    for p in absent:
        L[p, 4, 1] = np.nan
    return L


def light_like_L(rng, shape=()):
    """Coefficients of a radiance that is positive in every direction (band 0 in 1 .. 2, the others within
    0.1): the irradiance is a sum without cancellation, so a relative bound per component means something."""
    L = rng.uniform(-0.1, 0.1, size=shape + (9, 3))
    L[..., 0, :] = rng.uniform(1.0, 2.0, size=shape + (3,))
    return L


def unit(nrm):
    n2 = (nrm[:, 0] * nrm[:, 0] + nrm[:, 1] * nrm[:, 1]) + nrm[:, 2] * nrm[:, 2]
    return nrm / np.sqrt(n2)[:, None]


# ---------------------------------------------------------------- H1: the radiance twin
def test_h1_radiance_twin_is_probe_radiance_sh_bit_for_bit(rc):
    rng = np.random.default_rng(11)
    n = 300
    sh = rng.normal(size=(n, 9, 4)) * 50.0
    ns = rng.integers(0, 1000, n).astype(np.uint32)
    nm = rng.integers(0, 1000, n).astype(np.uint32)
    ns[:4] = (0, 0, 2 ** 32 - 1, 2 ** 32 - 1)
    nm[:4] = (0, 5, 2 ** 32 - 1, 0)  # (N == 0; misses only; N past 32 bits)
    ambient = (0.2, 0.3, 0.4)
    L = rc.probe_radiance_host(sh, ns, nm, ambient)
    want = rc.probe_radiance_sh(sh, ns, nm, ambient)
    has = (ns.astype(np.uint64) + nm) > 0
    assert has.sum() == n - 1
    assert _same_bits(L[has], want[has])
    assert np.isnan(L[~has]).all() and L[~has].size == 27
    assert _same_bits(rc.probe_radiance_host(sh, ns, nm, rc.rt_color(*ambient)), L)


# ---------------------------------------------------------------- H2: the segments twin
@pytest.mark.parametrize("dims", GRIDS)
def test_h2_segments_twin_against_the_replay(rc, dims):
    pos, nrm = points(dims)
    rays, t_max = rc.probe_segments_host(make_grid(rc, dims), pos, nrm)
    want_rays, want_t = replay_segments(dims, pos, nrm)
    assert _same_bits(rays["origin"], want_rays[:, :, 0]) and _same_bits(rays["direction"], want_rays[:, :, 1])
    assert _same_bits(t_max, want_t)
    # what the point set is there for
    cells = [replay_cell(dims, pos[k], nrm[k]) for k in range(N)]
    assert [k for k in range(N) if cells[k] is None] == sorted(BAD)
    assert not rays[BAD].view(np.uint8).any() and not t_max[BAD].any()
    for k in range(100, 120):  # at a probe's position: that probe alone, and the segment to itself is empty (bias != 0: not)
        assert sorted(cells[k][2]) == [0.0] * 7 + [1.0]
    visited = np.array([[t != 0.0 for t in c[2]] if c else [False] * 8 for c in cells])
    assert ((t_max > 0) <= visited).all()
    gone = visited[ON_PROBE] & (t_max[ON_PROBE] == 0)  # dist == 0: a visited corner with an empty segment
    assert gone.sum() == 1 and not rays[ON_PROBE][gone].view(np.uint8).any()
    if dims == (4, 3, 2):
        lo, hi = np.array(ORIGIN), probe_position(dims, [d - 1 for d in dims])
        for a in range(3):
            assert (pos[:100, a] < lo[a]).any() and (pos[:100, a] > hi[a]).any()
        assert (visited.sum(axis=1) == 8).sum() > 20
    length = np.sqrt((rays["direction"][..., :3] ** 2).sum(axis=-1))
    assert np.abs(length[t_max > 0] - 1.0).max() < 1e-15
    # without the flag: all zeros
    rays0, t0 = rc.probe_segments_host(make_grid(rc, dims, visibility=False), pos, nrm)
    assert not rays0.view(np.uint8).any() and not t0.any()
    # bias 0 at a probe's position: no segment at all
    rays1, t1 = rc.probe_segments_host(make_grid(rc, dims, bias=0.0), pos[100:120], nrm[100:120])
    assert not rays1.view(np.uint8).any() and not t1.any()
    want_rays, want_t = replay_segments(dims, pos, nrm, bias=0.0)
    rays1, t1 = rc.probe_segments_host(make_grid(rc, dims, bias=0.0), pos, nrm)
    assert _same_bits(rays1["direction"], want_rays[:, :, 1]) and _same_bits(t1, want_t)


# ---------------------------------------------------------------- H3: the blend twin
@pytest.mark.parametrize("dims", GRIDS)
def test_h3_blend_twin_against_the_replay(rc, dims):
    pos, nrm = points(dims)
    L = random_L(dims, absent=(0, n_probes(dims) - 1) if n_probes(dims) > 1 else ())
    grid = make_grid(rc, dims)
    occluded = np.random.default_rng(9).integers(0, 2, (N, 8)).astype(np.uint8)
    for occ in (occluded, None):
        E, W = rc.shade_probes_host(grid, L, pos, nrm, occ)
        want_E, want_W = replay_blend(dims, L, pos, nrm, occ)
        assert _same_bits(E, want_E) and _same_bits(W, want_W)
        assert not E[BAD].any() and not W[BAD].any()
    # the flag and the bias play no part in the blend
    E0, W0 = rc.shade_probes_host(make_grid(rc, dims, False, 0.0), L, pos, nrm)
    assert _same_bits(E0, E) and _same_bits(W0, W)


# ---------------------------------------------------------------- H4: properties
DIMS = GRIDS[0]


def test_h4_the_same_radiance_at_every_probe(rc):
    pos, nrm = points(DIMS)
    good = np.setdiff1d(np.arange(N), BAD)
    one = light_like_L(np.random.default_rng(21))
    L = np.broadcast_to(one, (n_probes(DIMS), 9, 3))
    E, W = rc.shade_probes_host(make_grid(rc, DIMS), L, pos[good], nrm[good])
    want = rc.sh_irradiance(one, unit(nrm[good]))
    assert (want > 0).all()
    assert (np.abs(E - want) <= 1e-14 * np.abs(want)).all()
    assert (np.abs(W - 1.0) <= 1e-15).all()


def test_h4_radiance_affine_in_the_probe_position(rc):
    rng = np.random.default_rng(22)
    base, slope = light_like_L(rng), rng.uniform(-0.02, 0.02, size=(3, 9, 3))
    at = np.array([probe_position(DIMS, (ix, iy, iz)) for iz in range(DIMS[2]) for iy in range(DIMS[1]) for ix in range(DIMS[0])])
    L = base + np.einsum("pa,alc->plc", at, slope)
    lo, hi = np.array(ORIGIN), probe_position(DIMS, [d - 1 for d in DIMS])
    pos = lo + rng.random((N, 3)) * (hi - lo)  # inside the grid
    nrm = rng.normal(size=(N, 3))
    E, W = rc.shade_probes_host(make_grid(rc, DIMS), L, pos, nrm)
    want = rc.sh_irradiance(base + np.einsum("pa,alc->plc", pos, slope), unit(nrm))
    assert (want > 0).all()
    assert (np.abs(E - want) <= 1e-12 * np.abs(want)).all()


def test_h4_a_point_at_a_probe_reads_that_probe_alone(rc):
    L = light_like_L(np.random.default_rng(23), (n_probes(DIMS),))
    index = [(ix, iy, iz) for iz in range(DIMS[2]) for iy in range(DIMS[1]) for ix in range(DIMS[0])]
    pos = np.array([probe_position(DIMS, i) for i in index])
    nrm = np.random.default_rng(24).normal(size=pos.shape)
    L_others_absent = L.copy()
    E, W = rc.shade_probes_host(make_grid(rc, DIMS), L, pos, nrm)
    assert (W == 1.0).all()
    want = rc.sh_irradiance(L, unit(nrm))
    assert (np.abs(E - want) <= 1e-14 * np.abs(want)).all()
    for p in range(len(index)):  # ... alone: every other probe made absent changes nothing
        L_others_absent[:] = np.nan
        L_others_absent[p] = L[p]
        E1, W1 = rc.shade_probes_host(make_grid(rc, DIMS), L_others_absent, pos[p:p + 1], nrm[p:p + 1])
        assert _same_bits(E1, E[p:p + 1]) and W1[0] == 1.0


def test_h4_hidden_and_absent_corners(rc):
    pos, nrm = points(DIMS)
    L = random_L(DIMS)
    grid = make_grid(rc, DIMS)
    E, W = rc.shade_probes_host(grid, L, pos, nrm, np.ones((N, 8), np.uint8))
    assert not E.any() and not W.any()
    E, W = rc.shade_probes_host(grid, np.full_like(L, np.nan), pos, nrm)
    assert not E.any() and not W.any()
    # one corner hidden, or its probe absent: the renormalised blend of the other seven
    inside = [k for k in range(N) if k not in BAD and all(t != 0.0 for t in replay_cell(DIMS, pos[k], nrm[k])[2])][:24]
    assert len(inside) == 24
    for j, k in enumerate(inside):
        c = j % 8
        occ = np.zeros((1, 8), np.uint8)
        occ[0, c] = 1
        _, i, t = replay_cell(DIMS, pos[k], nrm[k])
        E_hid, W_hid = rc.shade_probes_host(grid, L, pos[k:k + 1], nrm[k:k + 1], occ)
        want_E, want_W = replay_blend(DIMS, L, pos[k:k + 1], nrm[k:k + 1], occ)
        assert _same_bits(E_hid, want_E) and _same_bits(W_hid, want_W)
        ix, iy, iz = (i[a] + ((c >> a) & 1) for a in range(3))
        L_abs = L.copy()
        L_abs[(iz * DIMS[1] + iy) * DIMS[0] + ix, 8, 2] = np.inf
        E_abs, W_abs = rc.shade_probes_host(grid, L_abs, pos[k:k + 1], nrm[k:k + 1])
        assert _same_bits(E_abs, E_hid) and _same_bits(W_abs, W_hid)
        assert abs(W_hid[0] - (1.0 - t[c])) <= 1e-15 and 0.0 < W_hid[0] < 1.0
        E_all, W_all = rc.shade_probes_host(grid, L, pos[k:k + 1], nrm[k:k + 1])
        assert not _same_bits(E_all, E_hid)


def test_h4_a_point_outside_takes_the_boundarys_value(rc):
    pos, nrm = points(DIMS)
    good = np.setdiff1d(np.arange(N), BAD)
    lo, hi = np.array(ORIGIN), probe_position(DIMS, [d - 1 for d in DIMS])
    clamped = np.clip(pos[good], lo, hi)
    assert (clamped != pos[good]).any(axis=1).sum() > 50
    L = random_L(DIMS)
    grid = make_grid(rc, DIMS)
    E, W = rc.shade_probes_host(grid, L, pos[good], nrm[good])
    E1, W1 = rc.shade_probes_host(grid, L, clamped, nrm[good])
    assert _same_bits(E, E1) and _same_bits(W, W1)


# ---------------------------------------------------------------- H5: argument errors
def _bad_grids(rc):
    def g(**kw):
        grid = make_grid(rc, DIMS)
        for name, (at, value) in kw.items():
            if at is None:
                setattr(grid, name, value)
            else:
                getattr(grid, name)[at] = value
        return grid

    return {
        "step 0": g(step=(1, 0.0)), "step negative": g(step=(0, -1.0)), "step NaN": g(step=(2, math.nan)),
        "step inf": g(step=(0, math.inf)), "origin inf": g(origin=(1, -math.inf)), "origin NaN": g(origin=(2, math.nan)),
        "dims 0": g(dims=(1, 0)), "dims negative": g(dims=(2, -3)), "bias NaN": g(bias=(None, math.nan)),
        "bias negative": g(bias=(None, -1e-9)), "bias inf": g(bias=(None, math.inf)), "flag bits": g(flags=(None, 3)),
        "reserved": g(reserved=(1, 1)),
        "2^31 probes": rc.probe_grid(ORIGIN, STEP, (2048, 1024, 1024)),
        "2^31 probes in a plane": rc.probe_grid(ORIGIN, STEP, (65536, 65536, 1)),
    }


def test_h5_argument_errors_touch_nothing(rc):
    lib = rc.load_library()
    pos, nrm = points(DIMS)
    pts = rc._pack_surfels(pos[:4], nrm[:4])
    L = random_L(DIMS)
    E, W = np.full((4, 3), 7.0), np.full(4, 7.0)
    rays, t_max = np.full((4, 8, 8), 7.0), np.full((4, 8), 7.0)
    pp, pL = pts.ctypes.data_as(C.c_void_p), L.ctypes.data_as(C.POINTER(C.c_double))
    pE, pW = E.ctypes.data_as(C.POINTER(rc.rt_color)), W.ctypes.data_as(C.POINTER(C.c_double))
    pr, pt = rays.ctypes.data_as(C.c_void_p), t_max.ctypes.data_as(C.POINTER(C.c_double))
    good = make_grid(rc, DIMS)

    def calls(grid, n, L_=pL, pts_=pp, E_=pE, r_=pr, t_=pt, only=""):
        """(name, status) of the entries without a scene whose name holds `only`.  Every call made here ends in
        the argument checks: the device entry is never given host memory to launch over."""
        g = C.byref(grid) if grid is not None else None
        if only in "rt_debug_shade_probes":
            yield "rt_debug_shade_probes", lib.rt_debug_shade_probes(g, L_, pts_, n, None, E_, pW)
        if only in "rt_debug_probe_segments":
            yield "rt_debug_probe_segments", lib.rt_debug_probe_segments(g, pts_, n, r_, t_)
        if only in "rt_debug_probe_segments_device":
            yield "rt_debug_probe_segments_device", lib.rt_debug_probe_segments_device(g, pts_, n, r_, t_, None)

    for what, grid in list(_bad_grids(rc).items()) + [("null grid", None)]:
        for n in (4, 0):  # (a bad grid is an error at n == 0 too: it is checked first)
            for name, rc_ in calls(grid, n):
                assert rc_ == -1, (what, name)
                assert name + ":" in _last_error(lib), (what, name)
    for name, rc_ in calls(good, -1):
        assert rc_ == -1 and "n < 0" in _last_error(lib), name
    for kw in (dict(L_=None, only="shade"), dict(E_=None, only="shade"), dict(pts_=None), dict(r_=None, only="segments"),
               dict(t_=None, only="segments")):
        seen = [(name, rc_, _last_error(lib)) for name, rc_ in calls(good, 4, **kw)]
        assert len(seen) == {"shade": 1, "segments": 2, "": 3}[kw.get("only", "")]
        for name, rc_, message in seen:
            assert rc_ == -1 and "null pointer" in message, (kw, name)
    for name, rc_ in calls(good, 0, None, None, None, None, None):
        assert rc_ == 0, name
    # the scene entries: a null scene comes first, whatever else is wrong or empty
    for n in (4, 0, -1):
        assert lib.rt_shade_probes(None, C.byref(good), pL, pp, n, pE, pW) == -1 and "null scene" in _last_error(lib)
        assert lib.rt_shade_probes_device(None, C.byref(good), pL, pp, n, pE, pW, None) == -1 and "null scene" in _last_error(lib)
    # the radiance entries
    sh, ns = np.zeros((2, 9, 4)), np.zeros(2, np.uint32)
    out = np.full((2, 9, 3), 7.0)
    psh, pns, pout = (sh.ctypes.data_as(C.POINTER(rc.rt_probe_sh)), ns.ctypes.data_as(C.POINTER(C.c_uint32)),
                      out.ctypes.data_as(C.POINTER(C.c_double)))
    amb = rc.rt_color(0.1, 0.2, 0.3)
    for args in ((psh, pns, pns, -1, amb, pout), (None, pns, pns, 2, amb, pout), (psh, None, pns, 2, amb, pout),
                 (psh, pns, None, 2, amb, pout), (psh, pns, pns, 2, amb, None)):
        assert lib.rt_debug_probe_radiance(*args) == -1 and "rt_debug_probe_radiance" in _last_error(lib)
    assert lib.rt_probe_radiance_device(None, None, None, 2, amb, None, None) == -1
    assert lib.rt_probe_radiance_device(None, None, None, -1, amb, None, None) == -1
    assert lib.rt_debug_probe_radiance(None, None, None, 0, amb, None) == 0
    assert lib.rt_probe_radiance_device(None, None, None, 0, amb, None, None) == 0
    assert (E == 7.0).all() and (W == 7.0).all() and (rays == 7.0).all() and (t_max == 7.0).all() and (out == 7.0).all()
    # the wrappers' own checks
    with pytest.raises(ValueError):
        rc.shade_probes_host(good, L[:-1], pos[:4], nrm[:4])
    with pytest.raises(ValueError):
        rc.shade_probes_host(good, L, pos[:4], nrm[:4], np.zeros((4, 7)))
    with pytest.raises(ValueError):
        rc.probe_segments_host(good, pos[:4], nrm[:3])


# ---------------------------------------------------------------- H6: layout and memory
def test_h6_layout_as_a_c_compiler_sees_it(rc, tmp_path):
    exe = str(tmp_path / "probe_grid_layout")
    subprocess.run(["cc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "host", "probe_grid_layout.c"), "-o", exe], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    assert out.strip() == "80 0 24 48 60 64 72 1"
    assert C.sizeof(rc.rt_probe_grid) == 80
    assert [getattr(rc.rt_probe_grid, f).offset for f in ("origin", "step", "dims", "flags", "bias", "reserved")] == [0, 24, 48, 60, 64, 72]
    assert rc.RT_PROBE_GRID_VISIBILITY == 1
    assert rc.ABI_VERSION == 6 == rc.load_library().rt_abi_version()  # additive: detected by symbol


def test_h6_host_check_under_sanitizers(rc):
    """tests/host/shade_probes_host_check.cpp, a stand-alone program built with AddressSanitizer and UBSan over
    the library's host code, run on the CPU: the three twins on exact-size heap arrays over H2's grids, and
    their argument errors."""
    subprocess.run(["make", "-s", "-C", CSRC, "-j" + str(min(16, os.cpu_count() or 8)), "shade_probes_host_check_asan"], check=True)
    out = subprocess.run([os.path.join(CSRC, "_obj_asan", "shade_probes_host_check")], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "shade_probes_host_check: ok" in out.stdout


# ---------------------------------------------------------------- the binding
def test_exported_and_bound(rc):
    lib = rc.load_library()
    out = subprocess.run(["nm", "-D", "--defined-only", rc.LIB_PATH], capture_output=True, text=True).stdout
    for name in NAMES:
        assert f" T {name}\n" in out
        assert getattr(lib, name).argtypes is not None
    for name in ("shade_probes", "shade_probes_device", "probe_segments_device"):
        assert hasattr(rc.GpuRaytracer, name)
    for name in ("probe_grid", "probe_radiance_host", "probe_radiance_device", "probe_segments_host", "shade_probes_host"):
        assert callable(getattr(rc, name))


@pytest.mark.parametrize("name", NAMES)
def test_ctypes_prototype_matches_the_header(rc, name):
    fn = getattr(rc.load_library(), name)
    ret, params = _header_prototype(name)
    assert ret == "int" and fn.restype is C.c_int
    assert len(params) == len(fn.argtypes) == {"rt_probe_radiance_device": 7, "rt_debug_probe_radiance": 6, "rt_shade_probes_device": 8,
                                               "rt_shade_probes": 7, "rt_debug_probe_segments_device": 6,
                                               "rt_debug_probe_segments": 5, "rt_debug_shade_probes": 7}[name]
    sizes = {"rt_probe_sh": 288, "uint32_t": 4, "double": 8, "rt_color": 24, "rt_probe_grid": 80}
    for ctype, bound in zip(params, fn.argtypes):
        if ctype.endswith("*"):
            assert bound is C.c_void_p or issubclass(bound, C._Pointer), (ctype, bound)
            if bound is not C.c_void_p:
                assert C.sizeof(bound._type_) == sizes[ctype.rstrip("*").replace("const", "").strip()], (ctype, bound)
        elif ctype == "rt_color":
            assert bound is rc.rt_color
        else:
            assert bound is SCALARS[ctype], (ctype, bound)
