"""rt_denoise_device's host twin (rt_debug_denoise, no GPU) through denoise_host: the properties the
definition in include/rtcore.h ("denoising") promises -- a constant image maps to itself, nothing leaks
across an edge the normals or prim_ids stop, invalid pixels pass through and alter no neighbour, the noise
goes down -- the twin against a scalar numpy restatement of that definition, the argument errors and the
struct's layout, and the twin under sanitizers in a stand-alone program."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from denoise_cases import FRAMES, PARAMS, bits, make_guides, make_inputs, mse_luminance, planes, restate, run_host
from test_render_pixels_host import SCALARS, header_prototype

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("rt_primary_hits_device", "rt_denoise_device", "rt_debug_denoise")
SIZES = {"rt_denoise_params": 32, "rt_hit": 48, "rt_scene": None, "void": None, "double": 8, "uint32_t": 4, "float": 4}


def check_prototype(fn, name, n_params):
    """Every parameter of the header's prototype against the bound argtypes: the scalar widths exactly, a
    pointer for a pointer (c_void_p, or POINTER of an element of the size the header names)."""
    ret, params = header_prototype(name)
    assert ret == "int" and fn.restype is C.c_int
    assert len(params) == len(fn.argtypes) == n_params
    for ctype, bound in zip(params, fn.argtypes):
        if ctype.endswith("*"):
            assert bound is C.c_void_p or issubclass(bound, C._Pointer), (ctype, bound)
            if bound is not C.c_void_p:
                assert C.sizeof(bound._type_) == SIZES[ctype.rstrip("*").replace("const", "").strip()], (ctype, bound)
        else:
            assert bound is SCALARS[ctype], (ctype, bound)


def _same(a, b):
    return np.array_equal(bits(a), bits(b))


def _random_frame(rc, W, H, seed):
    """Random accumulators over make_guides' hits: every pixel with 1 .. 40 samples, a few misses, 0 .. 12
    batches and moments to match a per-sample variance of about a quarter of the squared mean."""
    rng = np.random.default_rng(seed)
    npix = W * H
    hits = make_guides(rc, W, H)
    ns = rng.integers(1, 41, npix).astype(np.uint32)
    nm = rng.integers(0, 3, npix).astype(np.uint32)
    nb = rng.integers(0, 13, npix).astype(np.uint32)
    mean = rng.uniform(0.05, 2.0, (3, npix))
    s = mean * ns
    Y = 0.299 * s[0] + 0.587 * s[1] + 0.114 * s[2]
    N = (ns + nm).astype(np.float64)
    q = Y * Y / N + 0.25 * (Y / N) ** 2 * np.maximum(nb.astype(np.float64) - 1, 0) * rng.uniform(0.5, 1.5, npix)
    acc = {"sum": s.reshape(-1).copy(), "samples": ns, "misses": nm, "q": q, "batches": nb, "plane": 0, "width": W, "height": H}
    return acc, hits


def test_exported_bound_and_sized(rc):
    lib = rc.load_library()
    out = subprocess.run(["nm", "-D", "--defined-only", rc.LIB_PATH], capture_output=True, text=True).stdout
    for name in NAMES:
        assert f" T {name}\n" in out
        assert getattr(lib, name).argtypes is not None
    assert rc.ABI_VERSION == 6 == lib.rt_abi_version()
    check_prototype(lib.rt_primary_hits_device, "rt_primary_hits_device", 7)
    check_prototype(lib.rt_denoise_device, "rt_denoise_device", 13)
    check_prototype(lib.rt_debug_denoise, "rt_debug_denoise", 12)
    for name in ("primary_hits_device", "denoise"):
        assert callable(getattr(rc.GpuRaytracer, name))
    assert callable(rc.denoise_device) and callable(rc.denoise_host)


@pytest.mark.parametrize("iterations", [1, 2, 3, 4, 5])
def test_h1_constant_image_maps_to_itself(rc, iterations):
    """H1: sum = samples * c0 with a dyadic c0, random guides, validity and moments: every valid pixel's
    out_sum is its sum bit for bit (c_q - c_p is exactly 0 for every tap), and so is every invalid one's."""
    W, H = 37, 19
    rng = np.random.default_rng(11)
    acc, hits = _random_frame(rc, W, H, 11)
    npix = W * H
    n = rng.normal(size=(H, W, 3))
    hits["normal"] = n / np.sqrt((n * n).sum(-1, keepdims=True))  # unit vectors in any direction, as a hit's are
    hits["position"] = rng.normal(size=(H, W, 3)) * 3
    hits["distance"] = rng.uniform(0.5, 9.0, (H, W)).astype(np.float32)
    hits["prim_id"] = rng.integers(-1, 4, (H, W))
    acc["samples"] = rng.integers(0, 41, npix).astype(np.uint32)
    c0 = np.array([0.625, 1.75, 0.09375])
    acc["sum"] = (c0[:, None] * acc["samples"]).reshape(-1)
    for flags in (0, rc.RT_DENOISE_SAME_PRIM):
        out, flat, var = run_host(rc, acc, hits, iterations=iterations, flags=flags)
        assert _same(flat, acc["sum"])
        valid = (acc["samples"] > 0) & (hits["prim_id"].reshape(-1) >= 0)
        assert 0 < valid.sum() < npix
        assert (var.reshape(-1)[~valid] == 0).all() and np.isfinite(var).all()


@pytest.mark.parametrize("same_prim", [False, True])
@pytest.mark.parametrize("iterations", [1, 5])
def test_h2_nothing_leaks_across_an_edge(rc, same_prim, iterations):
    """H2: a vertical line splits the frame into two planes with perpendicular normals (w_n = 0 exactly),
    or with equal normals, different prim_ids and RT_DENOISE_SAME_PRIM.  Whatever the accumulators right
    of the line hold -- other colours, other moments, NaN, no samples -- the output left of it is the
    same bit for bit."""
    W, H, edge = 40, 24, 20
    acc, hits = _random_frame(rc, W, H, 3)
    y, x = np.mgrid[0:H, 0:W]
    right = x >= edge
    hits["prim_id"] = right.astype(np.int32)
    hits["position"] = np.stack([(x - W / 2) * 0.02, (y - H / 2) * 0.02, np.full((H, W), 5.0)], -1)
    hits["distance"] = 5.0
    hits["normal"] = np.where(right[..., None] & (not same_prim), np.array([-1.0, 0.0, 0.0]), np.array([0.0, 0.0, -1.0]))
    flags = rc.RT_DENOISE_SAME_PRIM if same_prim else 0
    a_out, _, a_var = run_host(rc, acc, hits, iterations=iterations, flags=flags)
    rng = np.random.default_rng(4)
    r = right.reshape(-1)
    npix = W * H
    other = {k: v.copy() for k, v in acc.items() if isinstance(v, np.ndarray)}
    for c in range(3):
        other["sum"][c * npix:(c + 1) * npix][r] = rng.uniform(0.0, 500.0, r.sum())
    other["q"][r] = rng.uniform(0.0, 1e4, r.sum())
    other["samples"][r] = rng.integers(0, 100, r.sum())
    other["batches"][r] = rng.integers(0, 30, r.sum())
    idx = np.flatnonzero(r)
    other["sum"][idx[::7]] = np.nan
    other["q"][idx[3::11]] = np.inf
    b_out, _, b_var = run_host(rc, dict(acc, **other), hits, iterations=iterations, flags=flags)
    assert _same(a_out[:, :, :edge], b_out[:, :, :edge]) and _same(a_var[:, :edge], b_var[:, :edge])
    assert not _same(a_out[:, :, edge:], b_out[:, :, edge:])
    # and the line matters: without it (one prim, one normal) the right side reaches the left
    hits["prim_id"] = 0
    hits["normal"] = np.array([0.0, 0.0, -1.0])
    a_out = run_host(rc, acc, hits, iterations=iterations, flags=flags)[0]
    b_out = run_host(rc, dict(acc, **other), hits, iterations=iterations, flags=flags)[0]
    assert not _same(a_out[:, :, :edge], b_out[:, :, :edge])


@pytest.mark.parametrize("iterations", [1, 5])
def test_h3_invalid_pixels_pass_through_and_alter_nobody(rc, iterations):
    """H3: a pixel with samples == 0, with prim_id < 0 or with NaN in its sum leaves as it came (out_sum =
    sum bit for bit, out_var = 0); one whose normal is NaN keeps its own colour, (float)(sum / samples)
    * samples.  None of them reaches a neighbour: changing their values changes no other pixel's output."""
    W, H = 24, 16
    acc, hits = _random_frame(rc, W, H, 8)
    hits["prim_id"] = 0
    hits["normal"] = np.array([0.0, 0.0, -1.0])  # one plane: every valid pixel reaches its neighbours
    hits["position"][..., 2] = 5.0
    npix = W * H
    at = {"no_samples": 5 * W + 4, "no_hit": 5 * W + 9, "nan_sum": 9 * W + 6, "nan_normal": 9 * W + 14, "corner": 0}
    acc["samples"][at["no_samples"]] = 0
    acc["samples"][at["corner"]] = 0
    hits["prim_id"][divmod(at["no_hit"], W)] = -1
    acc["sum"][npix + at["nan_sum"]] = np.nan
    hits["normal"][divmod(at["nan_normal"], W)] = np.nan
    out, flat, var = run_host(rc, acc, hits, iterations=iterations)
    s3 = acc["sum"].reshape(3, npix)
    o3 = out.reshape(3, npix)
    for k in ("no_samples", "no_hit", "nan_sum", "corner"):
        assert _same(o3[:, at[k]], s3[:, at[k]]) and var.reshape(-1)[at[k]] == 0, k
    a = at["nan_normal"]
    n = np.float64(acc["samples"][a])
    assert _same(o3[:, a], (s3[:, a] / n).astype(np.float32).astype(np.float64) * n)
    special = np.zeros(npix, bool)
    special[list(at.values())] = True
    assert not _same(o3[:, ~special], s3[:, ~special])  # (the filter did something)
    # other values in those pixels, still invalid (or still without a usable normal)
    other = {k: v.copy() for k, v in acc.items() if isinstance(v, np.ndarray)}
    for k, i in at.items():
        for c in range(3):
            if not (k == "nan_sum" and c == 1):
                other["sum"][c * npix + i] *= 3.5
        other["q"][i] *= 7.0
        other["batches"][i] += 2
        if k not in ("no_samples", "corner"):
            other["samples"][i] += 5
    hits2 = hits.copy()
    ys, xs = np.divmod(np.array(list(at.values())), W)
    hits2["position"][ys, xs] += 0.25
    hits2["distance"][ys, xs] *= 2.0
    out2, _, var2 = run_host(rc, dict(acc, **other), hits2, iterations=iterations)
    assert _same(out2.reshape(3, npix)[:, ~special], o3[:, ~special])
    assert _same(var2.reshape(-1)[~special], var.reshape(-1)[~special])


@pytest.mark.parametrize("width,height", FRAMES)
def test_h4_it_denoises(rc, width, height):
    """H4: on a piecewise-constant truth (two planes and a patch of varying normals) with per-sample noise
    drawn in numpy, the luminance error against the truth over the valid pixels is strictly smaller after
    the filter than before."""
    acc, hits, truth, valid = make_inputs(rc, width, height, seed=width + height)
    out, _, var = run_host(rc, acc, hits)
    before = mse_luminance(planes(acc["sum"], acc), acc["samples"], truth, valid)
    after = mse_luminance(out, acc["samples"], truth, valid)
    print(f"H4 {width}x{height}: luminance MSE {before:.5g} -> {after:.5g}, ratio {after / before:.4f}")
    assert after < before
    assert np.isfinite(var[valid]).all() and (var[valid] >= 0).all() and (var[~valid] == 0).all()


@pytest.mark.parametrize("width,height,plane_pad,iterations,flags", [(8, 8, 0, 5, 0), (37, 19, 5, 2, 0), (37, 19, 0, 1, 1)])
def test_host_twin_equals_the_restatement(rc, width, height, plane_pad, iterations, flags):
    """The twin against the definition written out in scalar numpy (tests/denoise_cases.py, restate), bit
    for bit: the same single-rounded operations in the same order."""
    acc, hits, _, _ = make_inputs(rc, width, height, seed=5, plane=width * height + plane_pad if plane_pad else 0)
    out, _, var = run_host(rc, acc, hits, iterations=iterations, flags=flags)
    want, want_var = restate(acc, hits, iterations=iterations, flags=flags)
    assert _same(out, want) and _same(var, want_var)


@pytest.mark.parametrize("width,height", FRAMES)
def test_plane_padding_changes_nothing(rc, width, height):
    acc, hits, _, _ = make_inputs(rc, width, height, seed=2)
    pad, _, _, _ = make_inputs(rc, width, height, seed=2, plane=width * height + 37)
    a, _, a_var = run_host(rc, acc, hits)
    b, flat, b_var = run_host(rc, pad, hits)
    assert _same(a, b) and _same(a_var, b_var)
    npix = width * height
    assert (flat[npix:npix + 37] == 0).all() and (flat[2 * npix + 37:2 * npix + 74] == 0).all()  # between the planes


def test_h5_bad_arguments(rc):
    lib = rc.load_library()
    W = H = 8
    z = np.zeros(64, np.uint32)
    d = np.zeros(192)
    hits = np.zeros(64, rc.HIT_DTYPE)
    out = np.zeros(192)
    var = np.zeros(64, np.float32)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    par = lambda **kw: C.byref(rc.denoise_params(**dict(PARAMS, **kw)))  # noqa: E731
    good = [par(), ptr(d), ptr(z), ptr(z), ptr(d[:64]), ptr(z), 0, ptr(hits), W, H, ptr(out), ptr(var)]
    assert lib.rt_debug_denoise(*good) == 0
    no_var = list(good)
    no_var[11] = None
    assert lib.rt_debug_denoise(*no_var) == 0
    for k, v in ((0, None), (1, None), (2, None), (3, None), (4, None), (5, None), (7, None), (10, None), (8, 0), (9, -1),
                 (6, 63), (10, ptr(d)), (10, ptr(d[100:]))):
        bad = list(good)
        bad[k] = v
        assert lib.rt_debug_denoise(*bad) == -1, k
    nan = float("nan")
    for kw in (dict(sigma_l=0.0), dict(sigma_l=nan), dict(sigma_z=-1.0), dict(sigma_z=nan), dict(lum_eps=0.0), dict(lum_eps=nan),
               dict(normal_pow_log2=-1), dict(normal_pow_log2=9), dict(iterations=0), dict(iterations=6), dict(flags=2),
               dict(flags=0x80000001)):
        bad = list(good)
        bad[0] = par(**kw)
        assert lib.rt_debug_denoise(*bad) == -1, kw
    p = rc.denoise_params(**PARAMS)
    p.reserved[1] = 1
    assert lib.rt_debug_denoise(*([C.byref(p)] + good[1:])) == -1
    big = list(good)
    big[8], big[9] = 1 << 16, 1 << 16  # 2^32 pixels: refused before anything is read
    assert lib.rt_debug_denoise(*big) == -1
    # the device entries refuse the same before they touch a device
    assert lib.rt_denoise_device(None, None, None, None, None, None, 0, None, 8, 8, None, None, None) == -1
    assert lib.rt_denoise_device(*([par(iterations=6)] + good[1:] + [None])) == -1
    assert lib.rt_primary_hits_device(None, 0, 0, 8, 8, None, None) == -1


def test_h5_params_layout(rc, tmp_path):
    """tests/host/denoise_layout.c compiled as C99 against include/rtcore.h: 32 B and every offset, as the
    ctypes structure has them."""
    exe = str(tmp_path / "denoise_layout")
    subprocess.run(["cc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", exe,
                    os.path.join(ROOT, "tests", "host", "denoise_layout.c")], check=True)
    lines = [ln.split() for ln in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split("\n") if ln]
    assert lines[0] == ["sizeof", "32"] and C.sizeof(rc.rt_denoise_params) == 32
    want = [("sigma_l", 0, 4), ("sigma_z", 4, 4), ("lum_eps", 8, 4), ("normal_pow_log2", 12, 4), ("iterations", 16, 4),
            ("flags", 20, 4), ("reserved", 24, 8)]
    assert [(n, int(o), int(s)) for n, o, s in lines[1:8]] == want
    assert [n for n, _ in rc.rt_denoise_params._fields_] == [n for n, _, _ in want]
    for name, off, size in want:
        cf = getattr(rc.rt_denoise_params, name)
        assert (cf.offset, cf.size) == (off, size), name
    assert lines[8] == ["same_prim", "1", "abi", "6"] and rc.RT_DENOISE_SAME_PRIM == 1


def test_h6_host_twin_under_sanitizers():
    """The twin in a stand-alone program built with AddressSanitizer and UndefinedBehaviorSanitizer over the
    library's host code (`make denoise_host_check_asan`, tests/host/denoise_host_check.cpp): frames 8 x 8,
    37 x 19 and 130 x 70, each also with a padded plane, every array allocated at its exact size; the
    sanitizers report nothing, leaks included."""
    csrc = os.path.join(ROOT, "raytracercore_amd", "csrc")
    subprocess.run(["make", "-s", "-C", csrc, "-j8", "denoise_host_check_asan"], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    out = subprocess.run([os.path.join(csrc, "_obj_asan", "denoise_host_check")], capture_output=True, text=True, env=env,
                         timeout=300)
    assert out.returncode == 0 and "ok denoise 3 frames" in out.stdout and "ok arguments" in out.stdout, out.stdout + out.stderr
    assert "Sanitizer" not in out.stderr and "runtime error" not in out.stderr, out.stderr
