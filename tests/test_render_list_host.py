"""rt_render_list / rt_render_list_device, host side (no GPU): the symbols, their ctypes prototypes against
the header's, what the library refuses without a device, and the numpy restatement of the moments fold
(tests/list_cases.py) that tests/test_render_list_gpu.py relies on, against pixel_standard_error."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from list_cases import fold_moments, lum, standard_error
from test_render_pixels_host import _last_error, check_prototype

NAMES = ("rt_render_list", "rt_render_list_device")


def test_exported_and_bound(rc):
    lib = rc.load_library()
    out = subprocess.run(["nm", "-D", "--defined-only", rc.LIB_PATH], capture_output=True, text=True).stdout
    for name in NAMES:
        assert f" T {name}\n" in out
        assert getattr(lib, name).argtypes is not None
    for name in ("render_list", "render_list_device", "gather_adaptive"):
        assert hasattr(rc.GpuRaytracer, name)
    assert (rc.RT_LIST_RAYS, rc.RT_LIST_BEAMS, rc.RT_LIST_SURFELS) == (0, 1, 2)
    assert rc.ABI_VERSION == 6 == lib.rt_abi_version()  # additive: detected by symbol


@pytest.mark.parametrize("name", NAMES)
def test_ctypes_prototype_matches_the_header(rc, name):
    params = check_prototype(getattr(rc.load_library(), name), name, 17 if name == "rt_render_list" else 19)
    # kind, gather_mode; records, n_records; index, n; spp; seed, sample_base, stream_base
    assert params[1:11] == ["int32_t", "int32_t", "const void*", "int64_t", "const uint32_t*", "int64_t", "int32_t",
                            "uint64_t", "uint64_t", "uint64_t"]
    if name == "rt_render_list_device":
        assert params[16] == "uint64_t"  # plane


def test_refused_without_a_device(rc):
    """RT_ERR_ARG for a null scene, whatever n and spp are, before anything is launched; an unknown kind is
    reported first and a gather mode for rays second, each by name in rt_last_error.  The buffers are
    untouched.  No device is touched: this runs on a machine without one."""
    lib = rc.load_library()
    recs = np.zeros(2, rc.RAY_DTYPE)
    s, ns, ms = np.full((2, 3), 7.0), np.full(2, 7, np.uint32), np.full(2, 7, np.uint32)
    count = C.c_uint64(5)
    out = (s.ctypes.data_as(C.POINTER(rc.rt_color)), ns.ctypes.data_as(C.POINTER(C.c_uint32)),
           ms.ctypes.data_as(C.POINTER(C.c_uint32)), None, None, C.byref(count))
    rp = recs.ctypes.data_as(C.c_void_p)
    for n, spp in ((2, 1), (-1, 1), (2, 0), (0, 1)):
        assert lib.rt_render_list(None, rc.RT_LIST_RAYS, 0, rp, 2, None, n, spp, 1, 0, 0, *out) == -1, (n, spp)
        assert "rt_render_list:" in _last_error(lib) and "null scene" in _last_error(lib)
    dev = (None, None, None, None, None, 0, None, None)
    assert lib.rt_render_list_device(None, rc.RT_LIST_SURFELS, rc.RT_GATHER_COSINE, rp, 2, None, 2, 1, 1, 0, 0, *dev) == -1
    assert "rt_render_list_device" in _last_error(lib) and "null scene" in _last_error(lib)
    for kind in (-1, 3, 99):  # before the null scene
        assert lib.rt_render_list(None, kind, 0, rp, 2, None, 2, 1, 1, 0, 0, *out) == -1
        assert "unknown kind" in _last_error(lib)
        assert lib.rt_render_list_device(None, kind, 7, rp, 2, None, 2, 1, 1, 0, 0, *dev) == -1
        assert "unknown kind" in _last_error(lib)
    for kind, mode in ((rc.RT_LIST_RAYS, 1), (rc.RT_LIST_BEAMS, 2), (rc.RT_LIST_SURFELS, 3), (rc.RT_LIST_SURFELS, -1)):
        assert lib.rt_render_list(None, kind, mode, rp, 2, None, 2, 1, 1, 0, 0, *out) == -1
        assert "gather mode" in _last_error(lib)
    assert (s == 7.0).all() and (ns == 7).all() and (ms == 7).all() and count.value == 5


def test_the_wrapper_checks_its_arrays_first(rc):
    """render_list's own checks come before the library is called (a stand-in without a scene behind it)."""
    class Probe:
        handle = None
        lib = None

    recs = np.zeros(4, rc.SURFEL_DTYPE)
    with pytest.raises(ValueError):
        rc.GpuRaytracer.render_list(Probe(), 5, recs)
    with pytest.raises(ValueError):
        rc.GpuRaytracer.render_list(Probe(), rc.RT_LIST_SURFELS, recs, index=[0, -1])
    with pytest.raises(ValueError):  # moments asked, three arrays given
        rc.GpuRaytracer.render_list(Probe(), rc.RT_LIST_SURFELS, recs, moments=True,
                                    out=(np.zeros((4, 3)), np.zeros(4, np.uint32), np.zeros(4, np.uint32)))
    with pytest.raises(ValueError):  # arrays over another n
        rc.GpuRaytracer.render_list(Probe(), rc.RT_LIST_SURFELS, recs,
                                    out=(np.zeros((5, 3)), np.zeros(5, np.uint32), np.zeros(5, np.uint32)))
    with pytest.raises(ValueError):
        rc.GpuRaytracer.gather_adaptive(Probe(), rc.RT_LIST_SURFELS, recs, 0.1, 8, 32, 8, shape=(3, 2))


def test_the_fold_restatement_agrees_with_pixel_standard_error(rc):
    """Hand-made items for five entries: equal batches, unequal batch sizes, one batch only (J < 2: inf), an
    all-miss entry (Q = 0, se = 0) and an entry whose last item is empty (t_j = 0: no batch).  fold_moments'
    q and batches are the header's sums written out by hand, and pixel_standard_error of them is the
    header's estimate evaluated entry by entry in Python floats."""
    c = np.zeros((3, 5, 3))
    t = np.zeros((3, 5), np.int64)
    c[:, 0] = [[1.0, 2.0, 3.0], [0.5, 0.25, 0.125], [2.0, 0.0, 1.0]]
    t[:, 0] = 4
    c[:, 1] = [[3.0, 1.0, 0.5], [1.0, 1.0, 1.0], [0.25, 0.5, 0.75]]
    t[:, 1] = [7, 3, 1]
    c[0, 2] = [0.3, 0.6, 0.9]
    t[:, 2] = [5, 0, 0]
    t[:, 3] = [6, 6, 2]  # all misses: sums stay zero
    c[:2, 4] = [[0.125, 0.0, 4.0], [1.5, 2.5, 0.0]]
    t[:, 4] = [2, 2, 0]
    q, j = fold_moments(c, t)
    assert j.tolist() == [3, 3, 1, 3, 2]
    for e in range(5):
        want = 0.0
        for k in range(3):
            if t[k, e] > 0:
                y = (0.299 * c[k, e, 0] + 0.587 * c[k, e, 1]) + 0.114 * c[k, e, 2]
                want = want + y * y / float(t[k, e])
        assert q[e] == want
    total = c.sum(axis=0)
    n = t.sum(axis=0).astype(np.uint32)
    hits = np.where(total.any(axis=1), n, 0).astype(np.uint32)
    se = rc.pixel_standard_error(total, hits, n - hits, q, j)
    mine = standard_error(total, hits, n - hits, q, j)
    assert np.isinf(se[2]) and se[3] == 0.0 and np.isfinite(se[[0, 1, 4]]).all() and (se[[0, 1, 4]] > 0).all()
    assert np.array_equal(se, mine)
    assert lum(total[0]) == (0.299 * 3.5 + 0.587 * 2.25) + 0.114 * 4.125
