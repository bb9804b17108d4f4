"""Obscurance at surfels, host side (no GPU): include/rtcore.h's "obscurance at surfels" restated in plain Python
loops (tests/obscurance_cases.py) and held to the host twins bit for bit: the fold and its a + b promise (H1),
the rule, its error figures and the selection (H2), the argument errors (H3), the records' layout and the twins
under sanitizers (H4), the binding.  tests/test_obscurance_gpu.py holds the device to the twins."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

from obscurance_cases import (random_acc, replay_error, replay_fold, replay_select, replay_weight, same_bits, start_acc,
                              synthetic_samples)
from test_render_rays_host import SCALARS, _header_prototype, _last_error

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "raytracercore_amd", "csrc")
NAMES = {"rt_obscurance_surfels_device": 13, "rt_debug_obscurance_fold": 6, "rt_obscurance_select_device": 7,
         "rt_debug_obscurance_select": 5, "rt_debug_obscurance_error": 5}
RADIUS = 1.5


# ---------------------------------------------------------------- H1: the fold
@pytest.mark.parametrize("power", [0, 1, 2, 8])
def test_h1_fold_twin_against_the_replay(rc, power):
    rays, hits = synthetic_samples(rc, RADIUS)
    assert rays.shape == (3, 6)
    start = start_acc(rc, 3)
    acc, want = start.copy(), start.copy()
    got = rc.obscurance_fold_host(rc.obscurance_params(RADIUS, power), rays, hits, out=acc)
    replay_fold(RADIUS, power, rays, hits, want)
    assert got is acc and same_bits(acc, want)
    # the named cases: the miss and the distance at the radius weigh 0, the one just inside is a hit whose weight
    # is the least the power gives, the zero direction only counts, the NaN distance is not a hit
    assert replay_weight(-1, 0.0, RADIUS, power) == (0.0, False) and replay_weight(3, RADIUS, RADIUS, power) == (0.0, False)
    w, inside = replay_weight(3, float(hits["distance"][0, 3]), RADIUS, power)
    assert inside and (w == 1.0 if power == 0 else 0.0 < w < 1e-15)
    assert replay_weight(3, math.nan, RADIUS, power) == (0.0, False)
    assert np.array_equal(acc["samples"] - start["samples"], [6, 6, 6])
    fresh = rc.obscurance_fold_host(rc.obscurance_params(RADIUS, power), rays, hits)
    in_r = (hits["prim_id"] >= 0) & (hits["distance"] < RADIUS) & (rays["direction"][..., :3] != 0).any(axis=-1)
    assert np.array_equal(fresh["hits"], in_r.sum(axis=1)) and 0 < in_r.sum() < in_r.size
    assert not in_r[0, 1] and not in_r[0, 2] and in_r[0, 3] and not in_r[1, 0] and not in_r[2, 4] and in_r[1, 3]
    if power == 0:
        assert np.array_equal(fresh["o"], fresh["hits"]) and np.array_equal(fresh["o2"], fresh["o"])
    else:
        assert (fresh["o2"] < fresh["o"]).all() and (fresh["o"] < fresh["hits"]).all()
    # the zero direction adds nothing, not even a zero: a -0.0 in the sums survives a call of such samples alone
    neg = np.zeros(1, rc.OBSCURANCE_DTYPE)
    neg["o"], neg["bent"] = -0.0, -0.0
    rc.obscurance_fold_host(rc.obscurance_params(RADIUS, power), rays[1:2, :1], hits[1:2, :1], out=neg)
    assert np.signbit(neg["o"][0]) and np.signbit(neg["bent"][0]).all() and neg["samples"][0] == 1 and neg["hits"][0] == 0


def test_h1_fold_of_a_plus_b_samples_is_a_then_b(rc):
    rays, hits = synthetic_samples(rc, RADIUS)
    for power in (0, 1, 3):
        P = rc.obscurance_params(RADIUS, power)
        whole = rc.obscurance_fold_host(P, rays, hits, out=start_acc(rc, 3))
        for a in (1, 2, 5):
            acc = rc.obscurance_fold_host(P, rays[:, :a], hits[:, :a], out=start_acc(rc, 3))
            acc = rc.obscurance_fold_host(P, rays[:, a:], hits[:, a:], out=acc)
            assert same_bits(acc, whole), (power, a)
        # an entry's sums do not depend on its neighbours
        one = rc.obscurance_fold_host(P, rays[1:2], hits[1:2], out=start_acc(rc, 3)[1:2].copy())
        assert same_bits(one[0], whole[1])


def test_h1_known_sums(rc):
    """Four samples along +z at distances 0, r / 2, r and a miss, power 2: weights 1, 1/4, 0, 0."""
    rays = np.zeros((1, 4), rc.RAY_DTYPE)
    rays["direction"][..., 2] = 1.0
    hits = np.zeros((1, 4), rc.HIT_DTYPE)
    hits["distance"][0] = (0.0, 1.0, 2.0, 0.0)
    hits["prim_id"][0, 3] = -1
    acc = rc.obscurance_fold_host(rc.obscurance_params(2.0, 2), rays, hits)[0]
    assert (acc["o"], acc["o2"], acc["samples"], acc["hits"]) == (1.25, 1.0625, 4, 2)
    assert acc["bent"].tolist() == [0.0, 0.0, 2.75]
    assert rc.ambient_access(np.array([acc]))[0] == 1 - 1.25 / 4
    assert rc.bent_normals(np.array([acc]), np.array([[0.0, 3.0, 0.0]])).tolist() == [[0.0, 0.0, 1.0]]
    none = np.zeros(2, rc.OBSCURANCE_DTYPE)
    none["bent"][1] = np.nan
    assert rc.ambient_access(none).tolist() == [1.0, 1.0]
    assert rc.bent_normals(none, np.array([[0.0, 3.0, 0.0], [2.0, 0.0, 0.0]])).tolist() == [[0.0, 1.0, 0.0], [1.0, 0.0, 0.0]]


# ---------------------------------------------------------------- H2: the rule
def _nan_or_bits(a, b):
    """Equal bit for bit, a NaN matching any NaN (a square root's NaN carries the platform's sign)."""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and same_bits(a[~np.isnan(a)], b[~np.isnan(b)])


def test_h2_error_twin_against_the_replay(rc):
    acc = random_acc(rc)
    par = rc.obscurance_select_params(0.05, 8, 32)
    se, mean = rc.obscurance_error(par, acc)
    want_se, want_mean = np.full(len(acc), np.nan), np.full(len(acc), np.nan)
    for e in range(len(acc)):
        N = int(acc["samples"][e])
        if N >= 2:
            want_se[e] = replay_error(float(acc["o"][e]), float(acc["o2"][e]), N)[0]
            with np.errstate(all="ignore"):
                want_mean[e] = acc["o"][e] / np.float64(N)
    assert _nan_or_bits(se, want_se) and _nan_or_bits(mean, want_mean)
    assert np.isnan(se[:2]).all() and np.isnan(mean[:2]).all() and np.isfinite(se[2:6]).all()  # N = 0 and 1, then 2, 2, 8, 32
    # a constant-weight entry has se == 0 exactly, whatever the rounding of its sums
    assert se[13] == 0.0 and se[14] == 0.0 and se[15] == 0.0 and se[16] == 0.0
    assert abs(mean[13] - 0.3) < 1e-15 and mean[14] == 1.0 and mean[15] == 0.0
    mixed = np.isfinite(se) & np.isfinite(acc["o"]) & np.isfinite(acc["o2"]) & (acc["hits"] > 0) & (acc["hits"] < acc["samples"])
    assert mixed.sum() > 100 and (se[mixed] > 0).all()


@pytest.mark.parametrize("tol,lo,hi", [(0.05, 8, 32), (0.0, 2, 40), (0.1, 0, 1 << 31), (0.02, 16, 16), (1.0, 1, 3)])
def test_h2_select_twin_against_the_replay(rc, tol, lo, hi):
    acc = random_acc(rc)
    par = rc.obscurance_select_params(tol, lo, hi)
    want = replay_select(tol, lo, hi, acc)
    lst, count = rc.obscurance_select_host(par, acc)
    assert count == len(want) and lst.tolist() == want
    # N at min is judged by the rule, one below it is active; N at max is inactive whatever its sums
    N = acc["samples"]
    assert set(np.nonzero(N < lo)[0]) <= set(want) and not set(np.nonzero(N >= hi)[0]) & set(want)
    # a NaN in o or o2 cannot converge: inactive once it has min_samples; constant weights stop at min_samples
    for e in (10, 11, 13, 14, 15, 16):
        assert (e in want) == (N[e] < lo), e
    # cap below the count: the list's first cap entries, the count unchanged
    for cap in (0, 1, len(want) // 2):
        short, count2 = rc.obscurance_select_host(par, acc, cap=cap)
        assert count2 == len(want) and short.tolist() == want[:cap]


def test_h2_the_rule_is_neither_always_on_nor_always_off(rc):
    acc = random_acc(rc)
    _, count = rc.obscurance_select_host(rc.obscurance_select_params(0.05, 8, 1000), acc)
    judged = int((acc["samples"] >= 8).sum())
    below = int((acc["samples"] < 8).sum())
    assert below + judged // 5 < count < below + judged - judged // 5


# ---------------------------------------------------------------- H3: argument errors
def test_h3_argument_errors_touch_nothing(rc):
    lib = rc.load_library()
    rays, hits = synthetic_samples(rc, RADIUS)
    acc = np.zeros(3, rc.OBSCURANCE_DTYPE)
    acc.view(np.uint8)[:] = 7
    lst, se, mean = np.full(4, 7, np.uint32), np.full(3, 7.0), np.full(3, 7.0)
    v = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    good = rc.obscurance_params(RADIUS, 1)

    def p(**kw):
        par = rc.obscurance_params(RADIUS, 1)
        for name, value in kw.items():
            if name == "reserved":
                par.reserved[value] = 1
            else:
                setattr(par, name, value)
        return par

    bad = {"radius 0": p(radius=0.0), "radius negative": p(radius=-1.0), "radius NaN": p(radius=math.nan),
           "radius inf": p(radius=math.inf), "power -1": p(power=-1), "power 9": p(power=9), "reserved 0": p(reserved=0),
           "reserved 1": p(reserved=1), "reserved 2": p(reserved=2)}

    def fold(par, n=3, spp=6, r_=v(rays), h_=v(hits), a_=v(acc)):
        return lib.rt_debug_obscurance_fold(C.byref(par) if par is not None else None, r_, h_, n, spp, a_)

    def device(par, mode=rc.RT_GATHER_COSINE, scene=None, n=3, spp=6):
        # (ends in the argument checks: the device entry is never given host memory to launch over)
        return lib.rt_obscurance_surfels_device(scene, mode, v(rays), 3, None, n, C.byref(par) if par is not None else None, spp,
                                                0, 0, 0, v(acc), None)

    for what, par in list(bad.items()) + [("null params", None)]:
        assert fold(par) == -1 and "rt_debug_obscurance_fold:" in _last_error(lib), what
    for kw in (dict(n=-1), dict(spp=0), dict(spp=-2), dict(r_=None), dict(h_=None), dict(a_=None)):
        assert fold(good, **kw) == -1, kw
    assert fold(good, 0, 6, None, None, None) == 0
    # the device entry's order: the mode first, then the scene
    assert device(good, mode=3) == -1 and "unknown gather mode" in _last_error(lib)
    assert device(good, mode=-1) == -1 and "unknown gather mode" in _last_error(lib)
    assert device(good) == -1 and "null scene" in _last_error(lib) and "rt_obscurance_surfels_device:" in _last_error(lib)
    assert device(bad["power 9"]) == -1 and "null scene" in _last_error(lib)

    sel = rc.obscurance_select_params(0.05, 8, 32)

    def select(par=sel, a_=v(acc), n=3, l_=v(lst), cap=4):
        par = C.byref(par) if par is not None else None
        yield "rt_debug_obscurance_select", lib.rt_debug_obscurance_select(par, a_, n, l_, cap)
        yield "rt_obscurance_select_device", lib.rt_obscurance_select_device(par, a_, n, l_, cap, v(lst), None)

    for kw in (dict(par=None), dict(a_=None), dict(l_=None), dict(n=0), dict(n=-3), dict(n=1 << 32),
               dict(par=rc.obscurance_select_params(-0.5, 8, 32)), dict(par=rc.obscurance_select_params(math.nan, 8, 32))):
        for name, status in select(**kw):
            assert status == -1 and name + ":" in _last_error(lib), (kw, name)
    assert lib.rt_obscurance_select_device(C.byref(sel), v(acc), 3, v(lst), 4, None, None) == -1  # a null count
    assert lib.rt_debug_obscurance_select(C.byref(sel), v(np.zeros(3, rc.OBSCURANCE_DTYPE)), 3, None, 0) == 3  # no list wanted
    for args in ((None, v(acc), 3, v(se), v(mean)), (C.byref(sel), None, 3, v(se), v(mean)), (C.byref(sel), v(acc), 3, None, v(mean)),
                 (C.byref(sel), v(acc), 3, v(se), None), (C.byref(sel), v(acc), -1, v(se), v(mean))):
        assert lib.rt_debug_obscurance_error(*args) == -1 and "rt_debug_obscurance_error:" in _last_error(lib)
    assert lib.rt_debug_obscurance_error(C.byref(sel), None, 0, None, None) == 0
    assert (acc.view(np.uint8) == 7).all() and (lst == 7).all() and (se == 7.0).all() and (mean == 7.0).all()
    # the wrappers' own checks
    with pytest.raises(ValueError):
        rc.obscurance_fold_host(good, rays, hits[:, :4])
    with pytest.raises(ValueError):
        rc.obscurance_fold_host(good, rays, hits, out=np.zeros(2, rc.OBSCURANCE_DTYPE))
    with pytest.raises(ValueError):
        rc.GpuRaytracer.obscurance_adaptive(None, np.zeros((2, 3)), np.ones((2, 3)), 0.1, 8, 4, 4)


# ---------------------------------------------------------------- H4: layout and memory
def test_h4_layout_as_a_c_compiler_sees_it(rc, tmp_path):
    exe = str(tmp_path / "obscurance_layout")
    subprocess.run(["cc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "host", "obscurance_layout.c"), "-o", exe], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    assert out.strip() == "24 0 8 12 | 48 0 8 16 40 44 | 16 0 8 12"
    assert C.sizeof(rc.rt_obscurance_params) == 24 and C.sizeof(rc.rt_obscurance) == 48 and C.sizeof(rc.rt_obscurance_select_params) == 16
    assert [getattr(rc.rt_obscurance_params, f).offset for f in ("radius", "power", "reserved")] == [0, 8, 12]
    assert [getattr(rc.rt_obscurance, f).offset for f in ("o", "o2", "bent", "samples", "hits")] == [0, 8, 16, 40, 44]
    assert [getattr(rc.rt_obscurance_select_params, f).offset for f in ("tol", "min_samples", "max_samples")] == [0, 8, 12]
    assert rc.OBSCURANCE_DTYPE.itemsize == 48
    assert [rc.OBSCURANCE_DTYPE.fields[f][1] for f in ("o", "o2", "bent", "samples", "hits")] == [0, 8, 16, 40, 44]
    assert rc.ABI_VERSION == 6 == rc.load_library().rt_abi_version()  # additive: detected by symbol


def test_h4_host_check_under_sanitizers(rc):
    """tests/host/obscurance_host_check.cpp, a stand-alone program built with AddressSanitizer and UBSan over the
    library's host code, run on the CPU: the three twins on exact-size heap arrays, and their argument errors."""
    subprocess.run(["make", "-s", "-C", CSRC, "-j" + str(min(16, os.cpu_count() or 8)), "obscurance_host_check_asan"], check=True)
    out = subprocess.run([os.path.join(CSRC, "_obj_asan", "obscurance_host_check")], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "obscurance_host_check: ok" in out.stdout


# ---------------------------------------------------------------- the binding
def test_exported_and_bound(rc):
    lib = rc.load_library()
    out = subprocess.run(["nm", "-D", "--defined-only", rc.LIB_PATH], capture_output=True, text=True).stdout
    for name in NAMES:
        assert f" T {name}\n" in out
        assert getattr(lib, name).argtypes is not None
    for name in ("obscurance_surfels", "obscurance_surfels_device", "obscurance_select_device", "obscurance_adaptive"):
        assert hasattr(rc.GpuRaytracer, name)
    for name in ("obscurance_params", "obscurance_select_params", "obscurance_fold_host", "obscurance_select_device",
                 "obscurance_select_host", "obscurance_error", "ambient_access", "bent_normals"):
        assert callable(getattr(rc, name))
    assert rc.obscurance_params(2.0).power == 1 and tuple(rc.obscurance_params(2.0, 3).reserved) == (0, 0, 0)


@pytest.mark.parametrize("name", list(NAMES))
def test_ctypes_prototype_matches_the_header(rc, name):
    fn = getattr(rc.load_library(), name)
    ret, params = _header_prototype(name)
    assert (ret, fn.restype) == (("int64_t", C.c_int64) if name == "rt_debug_obscurance_select" else ("int", C.c_int))
    assert len(params) == len(fn.argtypes) == NAMES[name]
    sizes = {"rt_obscurance_params": 24, "rt_obscurance_select_params": 16}
    scalars = dict(SCALARS, uint32_t=C.c_uint32)
    for ctype, bound in zip(params, fn.argtypes):
        if ctype.endswith("*"):
            assert bound is C.c_void_p or issubclass(bound, C._Pointer), (ctype, bound)
            if bound is not C.c_void_p:
                assert C.sizeof(bound._type_) == sizes[ctype.rstrip("*").replace("const", "").strip()], (ctype, bound)
        else:
            assert bound is scalars[ctype], (ctype, bound)
