"""The host-buffer entries' chunk pipeline: a call cut into chunks is the uncut call, bit for bit.

Every host entry that takes caller's items (rt_query_rays, rt_occluded_rays, rt_render_rays, rt_render_beams,
rt_render_surfels, rt_render_pixels, rt_render_list, rt_occluded_surfels) runs them through one
double-buffered loop in chunks of RTCORE_QUERY_CHUNK items.  With chunks of 64, n = 64, 65, 128, 150 and 192
give one full chunk, two with a one-item tail, two full, three with a short tail and three full: both slot
parities are reused and the last chunk is both full and short.  The yardstick is the same entry with the
variable unset (one chunk at these sizes); there is no tolerance.

Two successive cut calls check that nothing of the first call's plans or events leaks into the second: an
overwriting entry answers the same again, an accumulating entry adds its own contribution again (the
arrays double, which is exact in fp64 and in the counts), and the ray count repeats.

The variable is set as each entry's own chunking test sets it: in the process for the queries and the
occlusion entries, for a fresh child process for the render entries (one child for all of them).

bounce.txt at 128 x 128, mode BVH; GROUPED as well for the two occlusion entries, whose launch planning
depends on n.  The items: the first 192 generator rays of tests/test_query_rays_gpu.py and the beams and
surfels made of them (tests/test_render_beams_gpu.py, tests/test_render_surfels_gpu.py, with their invalid
records at 7, 64 and 130), and 192 distinct frame pixels."""
import contextlib
import os
import subprocess
import sys

import numpy as np
import pytest

from test_query_rays_gpu import _gpu, _line_of_sight_rays, _same_bits, _scene
from test_render_beams_gpu import _beams
from test_render_surfels_gpu import _surfels

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNK = 64
NS = (64, 65, 128, 150, 192)
N_MAX = max(NS)
SEED = 11
BASE = 123457
SPP_RENDER, SPP_COUNTS = 2, 3
COSINE = 1
LIST_BEAMS = 1
SIZE = (128, 128)


@contextlib.contextmanager
def _cut():
    os.environ["RTCORE_QUERY_CHUNK"] = str(CHUNK)
    try:
        yield
    finally:
        del os.environ["RTCORE_QUERY_CHUNK"]


def _rays():
    o, d = _line_of_sight_rays(_scene("bounce").cameras[0])
    return o[:N_MAX], d[:N_MAX]


def _t_max():
    """One segment end per item: short, middling and long, a few +inf."""
    tm = np.random.default_rng(17).uniform(0.25, 12.0, N_MAX)
    tm[::13] = np.inf
    return tm


# ---------------------------------------------------------------- the queries and the occlusion entries
@pytest.fixture(scope="module")
def scene(rc):
    """The scene in a traversal mode, made once per mode."""
    made = {}

    def get(mode):
        if mode not in made:
            made[mode] = _gpu(rc, "bounce", mode, size=SIZE)
        return made[mode]

    yield get
    for gpu in made.values():
        gpu.close()


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("exact", [False, True], ids=["fast", "exact"])
def test_query_rays(scene, n, exact):
    gpu = scene("BVH")
    o, d = _rays()
    full = gpu.query_rays(o[:n], d[:n], exact=exact)
    assert (full["prim_id"] >= 0).any() and (full["prim_id"] < 0).any()
    with _cut():
        first = gpu.query_rays(o[:n], d[:n], exact=exact)
        second = gpu.query_rays(o[:n], d[:n], exact=exact)
    assert _same_bits(first, full) and _same_bits(second, full)


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("bounded", [True, False], ids=["t_max", "unbounded"])
@pytest.mark.parametrize("mode", ["BVH", "GROUPED"])
def test_occluded_rays(scene, mode, n, bounded):
    gpu = scene(mode)
    o, d = _rays()
    tm = _t_max()[:n] if bounded else None
    full = gpu.occluded_rays(o[:n], d[:n], tm)
    assert full.any() and not full.all()
    with _cut():
        first = gpu.occluded_rays(o[:n], d[:n], tm)
        second = gpu.occluded_rays(o[:n], d[:n], tm)
    assert _same_bits(first, full) and _same_bits(second, full)


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("bounded", [True, False], ids=["t_max", "unbounded"])
@pytest.mark.parametrize("mode", ["BVH", "GROUPED"])
def test_occluded_surfels(scene, mode, n, bounded):
    gpu = scene(mode)
    pos, nrm = (a[:n] for a in _surfels("bounce"))
    tm = _t_max()[:n] if bounded else None
    call = lambda out=None: gpu.occluded_surfels(pos, nrm, SPP_COUNTS, SEED, COSINE, t_max=tm, stream_base=BASE, out=out)
    full = call()
    assert 0 < full[0].sum() < SPP_COUNTS * n and (full[1] == SPP_COUNTS).all()
    with _cut():
        out = call()
        first = tuple(a.copy() for a in out)
        call(out)
    assert all(_same_bits(a, b) for a, b in zip(first, full))
    assert all(_same_bits(a, 2 * b) for a, b in zip(out, first))


# ---------------------------------------------------------------- the render entries
def _pixels():
    return np.random.default_rng(5).choice(SIZE[0] * SIZE[1], N_MAX, replace=False).astype(np.uint32)


def _list_index():
    """192 of the 200 beams in a shuffled order: rt_render_list gathers them on the host, chunk by chunk."""
    return np.random.default_rng(53).permutation(200)[:N_MAX].astype(np.uint32)


def render_cases(rc, gpu):
    """Every render entry at every n, called twice into one set of arrays: {case: the arrays after the first
    call, its ray count, the arrays after the second, its ray count}.  Runs as it stands in this process
    (uncut) and in the child (cut)."""
    o, d = _rays()
    beams = rc._pack_beams(*_beams("bounce"))
    pos, nrm = _surfels("bounce")
    px, index = _pixels(), _list_index()
    kw = dict(sample_base=1, stream_base=BASE)
    calls = {
        "rays": lambda n, out: gpu.render_rays(o[:n], d[:n], SPP_RENDER, SEED, out=out, **kw),
        "beams": lambda n, out: gpu.render_beams(beams[:n], None, None, None, None, None, SPP_RENDER, SEED, out=out, **kw),
        "surfels": lambda n, out: gpu.render_surfels(pos[:n], nrm[:n], SPP_RENDER, SEED, COSINE, out=out, **kw),
        "pixels": lambda n, out: gpu.render_pixels(px[:n], SPP_RENDER, SEED, sample_base=1, out=out, moments=True),
        "list_indexed": lambda n, out: gpu.render_list(LIST_BEAMS, beams, index[:n], SPP_RENDER, SEED, out=out, moments=True, **kw),
        "list_all": lambda n, out: gpu.render_list(LIST_BEAMS, beams[:n], None, SPP_RENDER, SEED, out=out, moments=True, **kw),
    }
    res = {}
    for name, call in calls.items():
        for n in NS:
            r = call(n, None)
            out = r[:3] + r[4:]  # (sum, samples, misses[, q, batches]); r[3] is the ray count
            first, rays_first = [a.copy() for a in out], r[3]
            r = call(n, out)
            res[name, n] = first + [np.uint64(rays_first)] + [a.copy() for a in out] + [np.uint64(r[3])]
    return res


CHILD = """
import sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import raytracercore_amd as rc
from test_chunk_pipeline_gpu import SIZE, render_cases
from test_query_rays_gpu import _gpu
gpu = _gpu(rc, "bounce", "BVH", size=SIZE)
res = render_cases(rc, gpu)
gpu.close()
np.savez(sys.argv[2], **{"%s/%d/%d" % (name, n, i): a for (name, n), arrays in res.items() for i, a in enumerate(arrays)})
"""


@pytest.fixture(scope="module")
def renders(rc, tmp_path_factory):
    """(uncut, cut): render_cases here, and in a fresh child with the variable set."""
    gpu = _gpu(rc, "bounce", "BVH", size=SIZE)
    uncut = render_cases(rc, gpu)
    gpu.close()
    path = tmp_path_factory.mktemp("chunk_pipeline") / "cut.npz"
    env = dict(os.environ, RTCORE_QUERY_CHUNK=str(CHUNK))
    subprocess.run([sys.executable, "-c", CHILD, ROOT, str(path)], check=True, env=env, timeout=300)
    z = np.load(path)
    cut = {key: [z["%s/%d/%d" % (key + (i,))] for i in range(len(arrays))] for key, arrays in uncut.items()}
    return uncut, cut


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("name", ["rays", "beams", "surfels", "pixels", "list_indexed", "list_all"])
def test_render_entries(renders, name, n):
    uncut, cut = renders
    want, got = uncut[name, n], cut[name, n]
    k = len(want) // 2 - 1  # arrays of one call; then its ray count
    s, ns, ms = want[:3]
    assert int(ns.sum()) + int(ms.sum()) == SPP_RENDER * n and ns.any() and s.any() and want[k] > 0
    for i in range(k + 1):  # the first cut call is the uncut call, ray count included
        assert _same_bits(got[i], want[i]), (name, n, i)
    for i in range(k):  # the second adds the same again
        assert _same_bits(got[k + 1 + i], 2 * got[i]), (name, n, i)
    assert got[2 * k + 1] == got[k]
