"""rt_render_probes, host side (no GPU): the L2 basis restated in numpy from include/rtcore.h's formulas and
held to the host twin bit for bit (H1) and to orthonormality by exact quadrature (H2), the fold twin against
a numpy loop (H3), the helpers on known answers (H4), the probes' launch plan and the record's layout (H5),
the twins under sanitizers (H6) and the binding.  tests/test_render_probes_gpu.py holds the device to the
restatement here."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

from test_render_rays_host import SCALARS, _header_prototype, _last_error

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "raytracercore_amd", "csrc")
NAMES = ("rt_render_probes", "rt_render_probes_device", "rt_debug_sh_basis", "rt_debug_probe_fold")
K0, K1, K2 = 0.28209479177387814, 0.48860251190291992, 1.0925484305920792
K3, K4 = 0.31539156525252005, 0.54627421529603959


# ---------------------------------------------------------------- the restatement
def basis(d):
    """rtcore.h, "Basis (normative)": d (..., 3) f64 -> Y (..., 9); every numpy operation is one rounding."""
    x, y, z = (np.asarray(d, np.float64)[..., k] for k in range(3))
    return np.stack([np.full(x.shape, K0), K1 * y, K1 * z, K1 * x, (K2 * x) * y, (K2 * y) * z, K3 * ((3.0 * z) * z - 1.0),
                     (K2 * x) * z, K4 * (x * x - y * y)], axis=-1)


def replay(rays, rgb, miss, out=None):
    """rtcore.h, "Accumulation (normative)", sample by sample: rays (n, spp) RAY_DTYPE, rgb (n, spp, 3) fp32
    values, miss (n, spp) bool -> (sh [n, 9, 4], samples, misses), added to `out`."""
    n, spp = rays.shape
    sh, ns, nm = out if out is not None else (np.zeros((n, 9, 4)), np.zeros(n, np.uint32), np.zeros(n, np.uint32))
    d = rays["direction"][..., :3]
    Y = basis(d)
    col = np.asarray(rgb, np.float32).astype(np.float64)
    dead = ~d.any(axis=2)
    for k in range(spp):
        hit = ~dead[:, k] & ~miss[:, k]
        sky = ~dead[:, k] & miss[:, k]
        sh[hit, :, :3] = sh[hit, :, :3] + (col[hit, k][:, None, :] * Y[hit, k][:, :, None])
        sh[sky, :, 3] = sh[sky, :, 3] + Y[sky, k]
        ns += hit.astype(np.uint32)
        nm += (~hit).astype(np.uint32)
    return sh, ns, nm


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ---------------------------------------------------------------- H1: the basis twin
def test_h1_basis_twin_is_the_restatement_bit_for_bit(rc):
    rng = np.random.default_rng(7)
    g = rng.normal(size=(1000, 3))
    g /= np.linalg.norm(g, axis=1, keepdims=True)
    axes = np.concatenate([np.eye(3), -np.eye(3)])
    d = np.concatenate([g, axes, g.astype(np.float32).astype(np.float64)])
    got = rc.sh_basis(d)
    assert got.shape == (2006, 9) and _same_bits(got, basis(d))
    assert _same_bits(rc.sh_basis(d.reshape(2, 1003, 3)), basis(d).reshape(2, 1003, 9))
    # the axes: Y2 is z's, Y6 = K3 (3 z^2 - 1), Y8 = K4 (x^2 - y^2)
    z = rc.sh_basis([0.0, 0.0, 1.0])
    assert z[2] == K1 and z[6] == K3 * 2.0 and z[1] == z[3] == z[4] == z[5] == z[7] == z[8] == 0.0
    assert rc.sh_basis([1.0, 0.0, 0.0])[8] == K4 and rc.sh_basis([0.0, -1.0, 0.0])[8] == -K4
    assert rc.sh_basis(np.zeros((0, 3))).shape == (0, 9)
    with pytest.raises(ValueError):
        rc.sh_basis(np.zeros((4, 2)))


# ---------------------------------------------------------------- H2: orthonormality
def test_h2_orthonormal_by_exact_quadrature(rc):
    """8-point Gauss-Legendre in z times 16 equal steps in phi integrates every product Y_l Y_m (degree <= 4 in
    z, frequency <= 4 in phi) exactly: the Gram matrix is the identity within 1e-12."""
    zs, wz = np.polynomial.legendre.leggauss(8)
    phi = 2.0 * math.pi * np.arange(16) / 16.0
    s = np.sqrt(1.0 - zs * zs)
    d = np.stack([s[:, None] * np.cos(phi)[None, :], s[:, None] * np.sin(phi)[None, :], np.broadcast_to(zs[:, None], (8, 16))], axis=-1)
    w = (wz[:, None] * (2.0 * math.pi / 16.0) * np.ones(16)[None, :]).reshape(-1)
    Y = rc.sh_basis(d).reshape(-1, 9)
    gram = (Y * w[:, None]).T @ Y
    err = float(np.abs(gram - np.eye(9)).max())
    print(f"H2: max |gram - I| = {err:.2e}")
    assert err <= 1e-12


# ---------------------------------------------------------------- H3: the fold twin
def _fold_case(rc):
    rng = np.random.default_rng(19)
    n, spp = 5, 70
    rays = np.zeros((n, spp), rc.RAY_DTYPE)
    g = rng.normal(size=(n, spp, 3))
    g = (g / np.linalg.norm(g, axis=2, keepdims=True)).astype(np.float32).astype(np.float64)
    rays["direction"][..., :3] = g
    rays["origin"][..., :3] = rng.normal(size=(n, spp, 3))
    rays["origin"][..., 3] = 1.0
    rays[2] = np.zeros((), rays.dtype)  # an invalid probe: every ray all zeros
    rgb = rng.uniform(0.0, 2.0, (n, spp, 3)).astype(np.float32)
    miss = rng.uniform(size=(n, spp)) < 0.3
    return rays, rgb, miss


def test_h3_fold_twin_against_the_numpy_loop(rc):
    rays, rgb, miss = _fold_case(rc)
    n, spp = rays.shape
    sh, ns, nm = rc.probe_fold_host(rays, rgb, miss)
    want = replay(rays, rgb, miss)
    assert _same_bits(sh, want[0]) and np.array_equal(ns, want[1]) and np.array_equal(nm, want[2])
    assert nm[2] == spp and ns[2] == 0 and not sh[2].any()
    assert ((ns + nm) == spp).all() and (ns[[0, 1, 3, 4]] > 0).all() and (nm[[0, 1, 3, 4]] > 0).all()
    assert sh[0, :, 3].any() and sh[0, :, :3].any()
    # added to what the arrays hold, in sample order
    rng = np.random.default_rng(23)
    start = (rng.normal(size=(n, 9, 4)), np.full(n, 3, np.uint32), np.full(n, 4, np.uint32))
    got = rc.probe_fold_host(rays, rgb, miss, out=tuple(a.copy() for a in start))
    want = replay(rays, rgb, miss, out=tuple(a.copy() for a in start))
    assert _same_bits(got[0], want[0]) and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
    assert _same_bits(got[0][2], start[0][2]) and got[2][2] == 4 + spp
    assert not _same_bits(got[0], start[0] + sh)  # (not the fold from zero added on: the order is part of the result)
    # 30 samples, then 40 into the same arrays, are the 70
    out = rc.probe_fold_host(rays[:, :30], rgb[:, :30], miss[:, :30])
    out = rc.probe_fold_host(np.ascontiguousarray(rays[:, 30:]), rgb[:, 30:], miss[:, 30:], out=out)
    assert _same_bits(out[0], sh) and np.array_equal(out[1], ns) and np.array_equal(out[2], nm)
    with pytest.raises(ValueError):
        rc.probe_fold_host(rays, rgb[:, :3], miss)
    with pytest.raises(ValueError):
        rc.probe_fold_host(rays, rgb, miss, out=(np.zeros((n, 9, 3)), ns, nm))


# ---------------------------------------------------------------- H4: the helpers
def test_h4_helpers_on_a_constant_radiance(rc):
    """Radiance A from every direction: c[l] = N / (4 pi) * integral A Y_l = A N K0 for l = 0 and exactly zero
    above, so L[0] = A sqrt(4 pi), and the irradiance on any normal is pi A.  The same through the misses'
    row with ambient = A."""
    A = np.array([0.25, 0.5, 2.0])
    N = 4096
    c = np.zeros((3, 9, 4))
    c[:, 0, :3] = A * N * math.sqrt(4.0 * math.pi) / (4.0 * math.pi)
    L = rc.probe_radiance_sh(c, np.full(3, N, np.uint32), np.zeros(3, np.uint32), (9.0, 9.0, 9.0))
    assert L.shape == (3, 9, 3)
    assert np.abs(L[:, 0] - A * math.sqrt(4.0 * math.pi)).max() <= 1e-12 and not L[:, 1:].any()
    nrm = np.array([[0.0, 0.0, 1.0], [1.0, 0.0, 0.0], [0.6, 0.0, -0.8]])
    assert np.abs(rc.sh_irradiance(L, nrm) - math.pi * A).max() <= 1e-12
    assert np.abs(rc.sh_radiance(L, nrm) - A).max() <= 1e-12
    c = np.zeros((3, 9, 4))
    c[:, 0, 3] = N * K0  # every sample a miss: the sum of Y0
    L = rc.probe_radiance_sh(c, np.zeros(3, np.uint32), np.full(3, N, np.uint32), rc.rt_color(*A))
    assert np.abs(L[:, 0] - A * math.sqrt(4.0 * math.pi)).max() <= 1e-12 and not L[:, 1:].any()
    assert np.abs(rc.sh_irradiance(L, nrm) - math.pi * A).max() <= 1e-12
    # half hits of A, half misses under the ambient A: the same again
    c[:, 0, 3] = N / 2 * K0
    c[:, 0, :3] = A * (N / 2) * K0
    L = rc.probe_radiance_sh(c, np.full(3, N // 2, np.uint32), np.full(3, N // 2, np.uint32), A)
    assert np.abs(rc.sh_irradiance(L, nrm) - math.pi * A).max() <= 1e-12
    # a clamped-cosine sky about +z, L(d) = max(0, d.z): its L2 irradiance on +z is the lobe's own norm
    # pi (1/4 + 1/3 + 5/64) (bands 0, 1, 2 of max(0, cos) are sqrt(pi)/2, sqrt(pi/3), sqrt(5 pi)/8)
    L = np.zeros((1, 9, 3))
    L[0, 0], L[0, 2], L[0, 6] = math.sqrt(math.pi) / 2.0, math.sqrt(math.pi / 3.0), math.sqrt(5.0 * math.pi) / 8.0
    want = math.pi * (0.25 + 1.0 / 3.0 + 5.0 / 64.0)
    assert np.abs(rc.sh_irradiance(L, [[0.0, 0.0, 1.0]]) - want).max() <= 1e-12
    assert np.isnan(rc.probe_radiance_sh(np.zeros((1, 9, 4)), [0], [0], A)).all()


# ---------------------------------------------------------------- H5: the plan and the layout
@pytest.mark.parametrize("n,spp", [(200, 5), (200, 50), (64, 130)])
def test_h5_every_sample_is_one_item_dealt_once(rc, n, spp):
    """The probes' plan is the rays' 8-wide tile with chunks = spp: one sample per item, n_chunks the next power
    of two.  The tickets deal every (block, chunk < spp) slot once and no slot at or past spp, so each of the
    n * spp real items (probe 64 b + lane < n, sample k) is dealt exactly once; the lanes past n of the last
    block stay closed in the kernels (item_ray >= n_rays)."""
    tickets, info = rc.item_order(8, (n + 7) // 8, spp, chunks=spp)
    n_chunks = 1 << (spp - 1).bit_length()
    assert info["chunk"] == 1 and info["n_chunks"] == n_chunks
    n_blocks = (n + 63) // 64
    seen = np.zeros(n_blocks * n_chunks * 64, np.int32)
    for _, first, length in tickets:
        assert length > 0 and first % 64 == 0 and length % 64 == 0
        seen[first:first + length] += 1
    seen = seen.reshape(n_blocks, n_chunks, 64)
    assert (seen[:, :spp] == 1).all() and not seen[:, spp:].any()
    probe = (np.arange(n_blocks)[:, None] * 64 + np.arange(64)[None, :]) < n
    assert int((seen[:, :spp] * probe[:, None, :]).sum()) == n * spp


def test_h5_layout_as_a_c_compiler_sees_it(rc, tmp_path):
    exe = str(tmp_path / "probe_layout")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "host", "probe_layout.c"), "-o", exe], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    assert out.strip() == "288 0 32 256 280 32"
    assert C.sizeof(rc.rt_probe_sh) == 288 == np.zeros((9, 4)).nbytes
    assert rc.ABI_VERSION == 6 == rc.load_library().rt_abi_version()  # additive: detected by symbol


# ---------------------------------------------------------------- H6: memory
def test_h6_host_check_under_sanitizers(rc):
    """tests/host/probe_host_check.cpp, a stand-alone program built with AddressSanitizer and UBSan over the
    library's host code (the Makefile's HOST_SAN pattern), run on the CPU: both twins on exact-size heap
    arrays, n = 0 and spp = 1 among the sizes, and their argument errors."""
    subprocess.run(["make", "-s", "-C", CSRC, "-j" + str(min(16, os.cpu_count() or 8)), "probe_host_check_asan"], check=True)
    out = subprocess.run([os.path.join(CSRC, "_obj_asan", "probe_host_check")], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "probe_host_check: ok" in out.stdout


# ---------------------------------------------------------------- the binding
def test_exported_and_bound(rc):
    lib = rc.load_library()
    out = subprocess.run(["nm", "-D", "--defined-only", rc.LIB_PATH], capture_output=True, text=True).stdout
    for name in NAMES:
        assert f" T {name}\n" in out
        assert getattr(lib, name).argtypes is not None
    for name in ("render_probes", "render_probes_device"):
        assert hasattr(rc.GpuRaytracer, name)
    for name in ("sh_basis", "probe_fold_host", "probe_radiance_sh", "sh_radiance", "sh_irradiance"):
        assert callable(getattr(rc, name))


@pytest.mark.parametrize("name", NAMES)
def test_ctypes_prototype_matches_the_header(rc, name):
    fn = getattr(rc.load_library(), name)
    ret, params = _header_prototype(name)
    assert ret == "int" and fn.restype is C.c_int
    assert len(params) == len(fn.argtypes) == {"rt_render_probes": 11, "rt_render_probes_device": 12, "rt_debug_sh_basis": 3,
                                               "rt_debug_probe_fold": 8}[name]
    sizes = {"rt_probe_sh": 288, "uint32_t": 4, "uint64_t": 8}
    for ctype, bound in zip(params, fn.argtypes):
        if ctype.endswith("*"):
            assert bound is C.c_void_p or issubclass(bound, C._Pointer), (ctype, bound)
            if bound is not C.c_void_p:
                assert C.sizeof(bound._type_) == sizes[ctype.rstrip("*").replace("const", "").strip()], (ctype, bound)
        else:
            assert bound is SCALARS[ctype], (ctype, bound)
    if name.startswith("rt_render_probes"):  # the surfels' parameter list without the mode, rt_probe_sh for the sums
        want = _header_prototype(name.replace("probes", "surfels"))[1]
        want = [p.replace("rt_color*", "rt_probe_sh*").replace("double*", "rt_probe_sh*") for p in want[:1] + want[2:]]
        assert params == want


def test_argument_errors_without_a_device(rc):
    """RT_ERR_ARG before anything is launched, the buffers untouched: a null scene with n < 0, spp <= 0, n == 0."""
    lib = rc.load_library()
    probes = np.zeros(2, rc.SURFEL_DTYPE)
    sh, ns, ms = np.full((2, 9, 4), 7.0), np.full(2, 7, np.uint32), np.full(2, 7, np.uint32)
    count = C.c_uint64(5)
    args = (sh.ctypes.data_as(C.POINTER(rc.rt_probe_sh)), ns.ctypes.data_as(C.POINTER(C.c_uint32)),
            ms.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(count))
    pp = probes.ctypes.data_as(C.c_void_p)
    for n, spp in ((2, 1), (-1, 1), (2, 0), (0, 1)):
        assert lib.rt_render_probes(None, pp, n, spp, 1, 0, 0, *args) == -1, (n, spp)
        assert "rt_render_probes" in _last_error(lib) and "null scene" in _last_error(lib)
    assert lib.rt_render_probes_device(None, pp, 2, 1, 1, 0, 0, None, None, None, None, None) == -1
    assert "rt_render_probes_device" in _last_error(lib)
    assert (sh == 7.0).all() and (ns == 7).all() and (ms == 7).all() and count.value == 5
    # the wrapper's own checks come before the library is called (no scene behind `self` here)
    with pytest.raises(ValueError):
        rc.GpuRaytracer.render_probes(None, np.zeros((4, 3)), 1, 0, out=(np.zeros((4, 9, 3)), np.zeros(4, np.uint32), np.zeros(4, np.uint32)))
    with pytest.raises(ValueError):
        rc.GpuRaytracer.render_probes(None, np.zeros((4, 3)), 1, 0, normals=np.zeros((3, 3)))
