"""Obscurance at surfels on the device: the sums against the fold's host twin over the reported rays and the
query's answers (G1, promise 1); index lists (G2); an entry's result alone, in sub-ranges called in any order, on a
side stream and chunked (G3, promise 2); a + b samples (G4, promise 3); a surfel at the centre of a sphere (G5);
the selection pass against its twin (G6); the adaptive loop (G7); errors and empty calls (G8); the renderer, the
occlusion counts and the depth bake left alone (G9).  The replay is tests/obscurance_cases.py's; the surfels are
tests/occluded_surfels_cases.py's shared set."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from obscurance_cases import same_bits
from occluded_surfels_cases import BAD, BASE, N, SEED, assert_not_hollow, surfel_set, valid_surfels
from test_query_rays_gpu import _gpu
from test_render_surfels_gpu import _last_error

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIFFUSE, COSINE, SPHERE = 0, 1, 2
RADIUS = 2.0
SAMPLE_BASE = 3
PAD = 96  # sentinel bytes behind the accumulators: two records


def _run(rc, gpu, pos, nrm, spp, params, mode=COSINE, index=None, sample_base=SAMPLE_BASE, stream_base=BASE, stream=None, acc=None,
         sentinels=True):
    """rt_obscurance_surfels_device over torch tensors, added into the byte tensor acc (a new zeroed one for None,
    with sentinel bytes behind it, which are checked unless told otherwise); (the (n,) OBSCURANCE_DTYPE result, acc)."""
    import torch

    n = len(pos)
    d_surfels = torch.from_numpy(rc._pack_surfels(pos, nrm).view(np.uint8).copy()).cuda()
    d_index = None if index is None else torch.from_numpy(np.ascontiguousarray(index, np.uint32).view(np.int32)).cuda()
    if acc is None:
        acc = torch.zeros(n * 48 + PAD, dtype=torch.uint8, device="cuda")
        acc[n * 48:] = 0x5A
    torch.cuda.synchronize()
    gpu.obscurance_surfels_device(mode, d_surfels, n, d_index, n if index is None else len(index),
                                  params, spp, SEED, sample_base, stream_base, acc,
                                  stream=stream.cuda_stream if stream is not None else 0)
    if stream is not None:
        stream.synchronize()
    torch.cuda.synchronize()
    got = acc.cpu().numpy()
    assert not sentinels or (got[n * 48:n * 48 + PAD] == 0x5A).all()
    return got[:n * 48].view(rc.OBSCURANCE_DTYPE).copy(), acc


def _samples(gpu, pos, nrm, spp, mode=COSINE, sample_base=SAMPLE_BASE, stream_base=BASE):
    """The rays rt_debug_surfel_rays_device reports and rt_query_rays' RT_QUERY_FAST answers for them, (n, spp)."""
    rays = gpu.surfel_rays(pos, nrm, spp, SEED, mode, sample_base=sample_base, stream_base=stream_base)
    return rays, gpu.query_rays(rays)


def _weights(rays, hits, radius):
    """(in, w at power 1) of the twin's inputs, as numpy sees them."""
    inside = (hits["prim_id"] >= 0) & (hits["distance"] < radius) & (rays["direction"][..., :3] != 0).any(axis=-1)
    return inside, np.where(inside, np.clip(1.0 - hits["distance"] / radius, 0.0, 1.0), 0.0)


# ---------------------------------------------------------------- G1: promise 1
@pytest.mark.parametrize("name,traversal", [("bounce", "BRUTE"), ("bounce", "BVH"), ("die", "GROUPED")])
def test_g1_sums_are_the_twin_over_the_reported_rays_and_the_querys_answers(rc, name, traversal):
    """n = 1, 5, 63, 65 (a wave, a block of four waves and one past it) x spp = 1, 63, 64, 65, 130 (one batch of 64
    samples short, full and one past it, and two and a tail), an invalid surfel in every case but the first; powers
    0, 1 and 3; the three gather modes on bounce / BVH."""
    pos, nrm = surfel_set(name)
    assert BAD[0] == 7 and BAD[2] == 64
    gpu = _gpu(rc, name, traversal)
    modes = (COSINE, DIFFUSE, SPHERE) if (name, traversal) == ("bounce", "BVH") else (COSINE,)
    seen = np.zeros(2, np.int64)
    for mode in modes:
        rays, hits = _samples(gpu, pos[:65], nrm[:65], 130, mode)
        for power in (1, 0, 3):
            P = rc.obscurance_params(RADIUS, power)
            full = power == 1 and mode == COSINE
            for n, first in ((1, 0), (1, 7), (5, 3), (63, 0), (65, 0)):
                for spp in (1, 63, 64, 65, 130) if full else (65, 130) if n in (5, 65) else ():
                    sl = slice(first, first + n)
                    got, _ = _run(rc, gpu, pos[sl], nrm[sl], spp, P, mode, stream_base=BASE + first)
                    # (sample k of an entry is the same ray whatever spp is: the first spp columns of the 130)
                    want = rc.obscurance_fold_host(P, rays[sl, :spp], hits[sl, :spp])
                    assert same_bits(got, want), (mode, power, n, first, spp)
                    bad = [i - first for i in (7, 64) if first <= i < first + n]
                    assert (got["samples"] == spp).all() and not got["hits"][bad].any() and not got["o"][bad].any()
                    assert not got["bent"][bad].any() and (got["hits"] <= spp).all()
                    seen += (int(got["hits"].sum()), int(got["samples"].sum()))
    gpu.close()
    print(f"G1 {name} {traversal}: {seen[0]} of {seen[1]} samples hit inside the radius")
    assert 0 < seen[0] < seen[1]


# ---------------------------------------------------------------- the shared case: bounce / BVH, the whole set
@pytest.fixture(scope="module")
def bounce_bvh(rc):
    gpu = _gpu(rc, "bounce", "BVH", size=(128, 128))
    yield gpu
    gpu.close()


@pytest.fixture(scope="module")
def full_case(rc, bounce_bvh):
    """The 200 surfels at 5 samples, COSINE, radius 2, power 1: (pos, nrm, params, rays, hits, the identity call's
    rows); read-only."""
    pos, nrm = surfel_set("bounce")
    P = rc.obscurance_params(RADIUS, 1)
    rays, hits = _samples(bounce_bvh, pos, nrm, 5)
    acc, _ = _run(rc, bounce_bvh, pos, nrm, 5, P)
    acc.setflags(write=False)
    return pos, nrm, P, rays, hits, acc


@pytest.mark.parametrize("name,traversal,mode", [("bounce", "BVH", COSINE), ("bounce", "BVH", DIFFUSE), ("bounce", "BVH", SPHERE),
                                                 ("die", "GROUPED", COSINE)])
def test_g1_the_inputs_are_not_hollow(rc, name, traversal, mode):
    """The twin's inputs over the valid surfels at 5 samples: hits inside the radius on both sides, and at least
    10 % of the samples with a weight strictly between 0.05 and 0.95 at power 1, so that a kernel that only ever
    sees weights 0 and 1 cannot pass; the whole set against the twin with them."""
    pos, nrm = surfel_set(name)
    gpu = _gpu(rc, name, traversal)
    rays, hits = _samples(gpu, pos, nrm, 5, mode)
    got, _ = _run(rc, gpu, pos, nrm, 5, rc.obscurance_params(RADIUS, 1), mode)
    gpu.close()
    good = valid_surfels()
    inside, w = _weights(rays[good], hits[good], RADIUS)
    assert_not_hollow(inside, f"{name} {traversal} mode {mode}: hit inside the radius")
    between = float(((w > 0.05) & (w < 0.95)).mean())
    print(f"{name} {traversal} mode {mode}: {100 * between:.1f} % of the samples weigh in (0.05, 0.95)")
    assert between >= 0.10
    assert same_bits(got, rc.obscurance_fold_host(rc.obscurance_params(RADIUS, 1), rays, hits))
    assert np.array_equal(got["hits"][good], inside.sum(axis=1)) and not got["hits"][BAD].any()


# ---------------------------------------------------------------- G2: the list
def test_g2_lists(rc, bounce_bvh, full_case):
    """A shuffled list shorter than the records that also names n_records and 2^32 - 1: the listed entries get the
    identity call's rows, the others and the two out of range keep their sentinel bytes."""
    import torch

    pos, nrm, P, _, _, whole = full_case
    rng = np.random.default_rng(5)
    listed = rng.permutation(N)[:77]
    index = np.concatenate([listed[:30], [N], listed[30:60], [(1 << 32) - 1], listed[60:]]).astype(np.uint32)
    acc = torch.full((N * 48 + PAD,), 0x5A, dtype=torch.uint8, device="cuda")
    acc[:N * 48].view(N, 48)[torch.from_numpy(listed).cuda()] = 0
    got, _ = _run(rc, bounce_bvh, pos, nrm, 5, P, index=index, acc=acc)
    assert same_bits(got[listed], whole[listed])
    rest = np.setdiff1d(np.arange(N), listed)
    assert (got[rest].view(np.uint8) == 0x5A).all() and len(rest) == N - 77
    # the list of every entry, backwards, is the identity call
    back, _ = _run(rc, bounce_bvh, pos, nrm, 5, P, index=np.arange(N)[::-1].copy())
    assert same_bits(back, whole)
    # the wrapper: listed entries only, added into the caller's array
    out = bounce_bvh.obscurance_surfels(pos, nrm, 5, SEED, RADIUS, 1, COSINE, index=listed, sample_base=SAMPLE_BASE, stream_base=BASE)
    assert same_bits(out[listed], whole[listed]) and not out[rest].view(np.uint8).any()


# ---------------------------------------------------------------- G3: promise 2
G3_N, G3_SPP = 65, 70


@pytest.fixture(scope="module")
def place_case(rc, bounce_bvh):
    pos, nrm = (a[:G3_N] for a in surfel_set("bounce"))
    P = rc.obscurance_params(RADIUS, 2)
    acc, _ = _run(rc, bounce_bvh, pos, nrm, G3_SPP, P)
    acc.setflags(write=False)
    return pos, nrm, P, acc


def test_g3_an_entrys_result_does_not_depend_on_its_place(rc, bounce_bvh, place_case):
    import torch

    pos, nrm, P, whole = place_case
    for i in (0, 7, 63, 64):
        one, _ = _run(rc, bounce_bvh, pos[i:i + 1], nrm[i:i + 1], G3_SPP, P, stream_base=BASE + i)
        assert same_bits(one[0], whole[i]), i
    # sub-ranges called in a shuffled order into slices of one array
    acc = torch.zeros(G3_N * 48 + PAD, dtype=torch.uint8, device="cuda")
    acc[G3_N * 48:] = 0x5A
    cuts = [0, 1, 6, 40, 64, 65]
    for k in np.random.default_rng(4).permutation(len(cuts) - 1):
        a, b = cuts[k], cuts[k + 1]
        _run(rc, bounce_bvh, pos[a:b], nrm[a:b], G3_SPP, P, stream_base=BASE + a, acc=acc[a * 48:], sentinels=False)
    got = acc.cpu().numpy()
    assert (got[G3_N * 48:] == 0x5A).all() and same_bits(got[:G3_N * 48].view(rc.OBSCURANCE_DTYPE), whole)
    assert len(np.unique(whole["hits"])) > 3


def test_g3_a_side_stream_gives_the_same_bits(rc, bounce_bvh, place_case):
    import torch

    pos, nrm, P, whole = place_case
    got, _ = _run(rc, bounce_bvh, pos, nrm, G3_SPP, P, stream=torch.cuda.Stream())
    assert same_bits(got, whole)


def test_g3_the_two_fold_layouts_agree(rc, bounce_bvh, place_case, monkeypatch):
    """RTCORE_OBSCURANCE_FOLD=thread, read at every call: the thread-per-entry fold gives the wave-per-entry one's
    bits (both are the twin's)."""
    pos, nrm, P, whole = place_case
    monkeypatch.setenv("RTCORE_OBSCURANCE_FOLD", "thread")
    got, _ = _run(rc, bounce_bvh, pos, nrm, G3_SPP, P)
    assert same_bits(got, whole)


CHILD = """
import sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import raytracercore_amd as rc
from test_query_rays_gpu import _gpu
from test_obscurance_gpu import _run, G3_SPP, RADIUS
z = np.load(sys.argv[2])
gpu = _gpu(rc, "bounce", "BVH", size=(128, 128))
P = rc.obscurance_params(RADIUS, 2)
a70, _ = _run(rc, gpu, z["pos"], z["nrm"], G3_SPP, P)
a5, _ = _run(rc, gpu, z["pos"], z["nrm"], 5, P)
l5, _ = _run(rc, gpu, z["pos"], z["nrm"], 5, P, index=z["index"])
gpu.close()
np.savez(sys.argv[3], a70=a70.view(np.uint8), a5=a5.view(np.uint8), l5=l5.view(np.uint8))
"""


def test_g3_chunks(rc, bounce_bvh, place_case, tmp_path):
    """RTCORE_QUERY_CHUNK = 96 samples, set for a fresh child process: at 70 spp a chunk is one entry, at 5 spp it
    is 19, with and without a list; all are the one-chunk call bit for bit."""
    pos, nrm, P, whole = place_case
    a5, _ = _run(rc, bounce_bvh, pos, nrm, 5, P)
    index = np.random.default_rng(8).permutation(G3_N)[:50].astype(np.uint32)
    np.savez(tmp_path / "case.npz", pos=pos, nrm=nrm, index=index)
    env = dict(os.environ, RTCORE_QUERY_CHUNK="96")
    subprocess.run([sys.executable, "-c", CHILD, ROOT, str(tmp_path / "case.npz"), str(tmp_path / "out.npz")],
                   check=True, env=env, timeout=300)
    z = np.load(tmp_path / "out.npz")
    assert same_bits(z["a70"].view(rc.OBSCURANCE_DTYPE), whole) and same_bits(z["a5"].view(rc.OBSCURANCE_DTYPE), a5)
    l5 = z["l5"].view(rc.OBSCURANCE_DTYPE)
    rest = np.setdiff1d(np.arange(G3_N), index)
    assert same_bits(l5[index], a5[index]) and not l5[rest].view(np.uint8).any()


# ---------------------------------------------------------------- G4: promise 3
def test_g4_64_and_66_samples_are_130(rc, bounce_bvh):
    pos, nrm = surfel_set("bounce")
    P = rc.obscurance_params(RADIUS, 1)
    whole, _ = _run(rc, bounce_bvh, pos[:9], nrm[:9], 130, P)
    first, acc = _run(rc, bounce_bvh, pos[:9], nrm[:9], 64, P)
    both, _ = _run(rc, bounce_bvh, pos[:9], nrm[:9], 66, P, sample_base=SAMPLE_BASE + 64, acc=acc)
    assert same_bits(both, whole) and not same_bits(first, whole)
    assert whole["samples"].tolist() == [130] * 9 and whole["hits"][7] == 0 and whole["o"][7] == 0


# ---------------------------------------------------------------- G5: a sphere round the surfel
UNIT_SPHERE = "size 16 12\ncamera 0 -4 0, 0 0 0, 0 0 1, 60\ntwosided true\ndiffuse .5 .5 .5\nspecular 0 0 0\nsphere 0 0 0 1\n"


def _in_order(values):
    s = [0.0, 0.0, 0.0]
    for row in values:
        for a in range(3):
            s[a] = s[a] + float(row[a])
    return s


def test_g5_a_surfel_at_the_centre_of_a_unit_sphere(rc):
    """One two-sided unit sphere, one surfel at its centre, SPHERE mode, 64 samples: every fast hit is at distance
    exactly 1.0, so every weight is the same and the sums are known."""
    gpu = rc.GpuRaytracer(rc.SceneLoader.from_text(UNIT_SPHERE), 0)
    pos, nrm = np.zeros((1, 3)), np.array([[0.0, 0.0, 1.0]])
    rays, hits = _samples(gpu, pos, nrm, 64, SPHERE)
    dist = hits["distance"][0]
    print(f"G5: distances in [{dist.min()!r}, {dist.max()!r}], {int((hits['prim_id'][0] >= 0).sum())} hits")
    d = rays["direction"][0, :, :3]
    run = lambda radius, power: _run(rc, gpu, pos, nrm, 64, rc.obscurance_params(radius, power), SPHERE)[0][0]  # noqa: E731
    a = run(2.0, 1)
    print(f"G5 radius 2 power 1: o {a['o']!r} o2 {a['o2']!r} hits {a['hits']} bent {a['bent'].tolist()}")
    assert a["o"] == 32.0 and a["o2"] == 16.0 and a["hits"] == 64 and a["samples"] == 64
    se, mean = rc.obscurance_error(rc.obscurance_select_params(0.01, 8, 1000), np.array([a]))
    assert se[0] == 0.0 and mean[0] == 0.5
    assert a["bent"].tolist() == _in_order(0.5 * d) and a["bent"].tolist() == [0.5 * x for x in _in_order(d)]
    assert run(2.0, 2)["o"] == 16.0
    for radius in (1.0, 0.5):
        b = run(radius, 1)
        assert b["o"] == 0.0 and b["o2"] == 0.0 and b["hits"] == 0 and b["samples"] == 64, radius
        assert b["bent"].tolist() == _in_order(d), radius
    gpu.close()


# ---------------------------------------------------------------- G6: the selection pass
@pytest.mark.parametrize("n", [1, 63, 64, 65, 200])
def test_g6_select_is_the_twin(rc, bounce_bvh, full_case, n):
    """On accumulators the device produced: every entry at 5 samples, every second one at 10."""
    import torch

    pos, nrm, P, _, _, _ = full_case
    _, d_acc = _run(rc, bounce_bvh, pos, nrm, 5, P)
    acc, _ = _run(rc, bounce_bvh, pos, nrm, 5, P, index=np.arange(1, N, 2), sample_base=SAMPLE_BASE + 5, acc=d_acc)
    assert set(acc["samples"].tolist()) == {5, 10}
    par = rc.obscurance_select_params(0.12, 4, 10)
    want, count = rc.obscurance_select_host(par, acc[:n])
    assert count == len(want) and (n < 63 or 0 < count < (n + 1) // 2 + 1)
    for cap in sorted({n, count // 2, 0}):
        d_list = torch.full((n + 4,), -5, dtype=torch.int32, device="cuda")
        d_count = torch.full((2,), -5, dtype=torch.int32, device="cuda")
        bounce_bvh.obscurance_select_device(par, d_acc, n, d_list if cap else None, cap, d_count)
        torch.cuda.synchronize()
        got, got_count = d_list.cpu().numpy(), d_count.cpu().numpy()
        k = min(cap, count)
        assert got_count.tolist() == [count, -5], (n, cap)
        assert got[:k].view(np.uint32).tolist() == want[:k].tolist() and (got[k:] == -5).all(), (n, cap)
    if n == 200:  # a side stream
        side = torch.cuda.Stream()
        d_list = torch.full((n,), -5, dtype=torch.int32, device="cuda")
        d_count = torch.zeros(1, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        bounce_bvh.obscurance_select_device(par, d_acc, n, d_list, n, d_count, stream=side.cuda_stream)
        side.synchronize()
        assert d_count.item() == count and d_list.cpu().numpy()[:count].tolist() == want.tolist()


# ---------------------------------------------------------------- G7: the loop
def test_g7_the_adaptive_loop(rc, bounce_bvh):
    """obscurance_adaptive on bounce, COSINE, radius 1, power 1, tol 0.02, min 32, max 256, batch 16 over the shared
    set.  A model of this loop on the CPU oracle's distances gave 71 of 197 valid surfels stopping at 32 and 90
    reaching 256; asserted are only the loose conditions: at least 20 % each."""
    pos, nrm = surfel_set("bounce")
    out = bounce_bvh.obscurance_adaptive(pos, nrm, 0.02, 32, 256, 16, seed=SEED, radius=1.0, power=1, mode=COSINE, stream_base=BASE,
                                         sample_base=SAMPLE_BASE)
    acc = out["acc"].cpu().numpy().reshape(-1).view(rc.OBSCURANCE_DTYPE)
    counts = out["counts"]
    print(f"G7: {len(counts)} iterations, list lengths {counts}")
    assert 2 <= len(counts) <= 16 and counts[0] == N and all(b <= a for a, b in zip(counts, counts[1:]))
    assert [len(lst) for lst in out["lists"]] == counts
    ns = acc["samples"].astype(np.int64)
    assert (ns % 16 == 0).all() and ns.min() >= 32 and ns.max() <= 256
    se, _ = rc.obscurance_error(out["params"], acc)
    assert (se[ns < 256] <= 0.02).all() and (ns[BAD] == 32).all()
    good = valid_surfels()
    at_min, at_cap = float((ns[good] == 32).mean()), float((ns[good] == 256).mean())
    print(f"G7: {int((ns[good] == 32).sum())} of {len(good)} valid surfels stop at 32, {int((ns[good] == 256).sum())} reach 256, "
          f"{int(ns.sum())} samples against {256 * N} fixed")
    assert at_min >= 0.20 and at_cap >= 0.20
    # promises 2 and 3 together: one plain call per distinct sample count over the entries that ended there
    want = np.zeros(N, rc.OBSCURANCE_DTYPE)
    for c in np.unique(ns):
        bounce_bvh.obscurance_surfels(pos, nrm, int(c), SEED, 1.0, 1, COSINE, index=np.nonzero(ns == c)[0], sample_base=SAMPLE_BASE,
                                      stream_base=BASE, out=want)
    assert same_bits(acc, want)
    open_share = rc.ambient_access(acc)
    bent = rc.bent_normals(acc, nrm)
    assert ((open_share >= 0) & (open_share <= 1)).all() and np.abs(np.linalg.norm(bent[good], axis=1) - 1).max() < 1e-12


# ---------------------------------------------------------------- G8: plumbing
def test_g8_empty_calls_and_errors_touch_nothing(rc, bounce_bvh):
    import torch

    pos, nrm = surfel_set("bounce")
    lib, h = bounce_bvh.lib, bounce_bvh.handle
    P = rc.obscurance_params(RADIUS, 1)
    d_surfels = torch.from_numpy(rc._pack_surfels(pos[20:28], nrm[20:28]).view(np.uint8).copy()).cuda()
    d_acc = torch.full((8 * 48,), 0x5A, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731

    def call(handle, n, spp, par=P, null=(), mode=COSINE, n_records=8, index=None):
        a = [p(d_surfels), p(d_acc)]
        for k in null:
            a[k] = None
        return lib.rt_obscurance_surfels_device(handle, mode, a[0], n_records, index, n, C.byref(par) if par is not None else None, spp,
                                                0, 0, 0, a[1], None)

    assert call(h, 0, 4) == 0 and call(h, 0, 4, None, (0, 1)) == 0
    for kw in (dict(null=(0,)), dict(null=(1,)), dict(par=None), dict(n=-1), dict(spp=0), dict(spp=-3), dict(spp=(1 << 19) + 1),
               dict(mode=3), dict(mode=-1), dict(n_records=0), dict(n_records=1 << 32), dict(n=7), dict(n_records=9)):
        args = dict(dict(handle=h, n=8, spp=4), **kw)
        assert call(**args) == -1, kw
        assert "rt_obscurance_surfels_device" in _last_error(lib), kw
    assert call(h, 8, (1 << 19) + 1) == -1 and "2^19" in _last_error(lib) and "sample_base" in _last_error(lib)
    assert call(h, 8, 4, mode=3) == -1 and "gather mode" in _last_error(lib)
    for field, value in (("radius", 0.0), ("radius", float("nan")), ("radius", float("inf")), ("power", 9), ("power", -1)):
        bad = rc.rt_obscurance_params.from_buffer_copy(bytes(P))
        setattr(bad, field, value)
        assert call(h, 8, 4, bad) == -1, field
    assert call(None, 8, 4) == -1 and "null scene" in _last_error(lib)
    gpu2 = _gpu(rc, "bounce", "BVH2")
    assert call(gpu2.handle, 8, 4) == -7 and "BVH2" in _last_error(lib)
    assert call(gpu2.handle, 0, 4) == 0
    assert call(gpu2.handle, 8, 4, mode=3) == -1  # (the argument errors come first)
    gpu2.close()
    torch.cuda.synchronize()


def test_g8_errors_leave_the_accumulators_alone(rc, bounce_bvh):
    import torch

    pos, nrm = surfel_set("bounce")
    lib, h = bounce_bvh.lib, bounce_bvh.handle
    P = rc.obscurance_params(RADIUS, 1)
    d_surfels = torch.from_numpy(rc._pack_surfels(pos[20:28], nrm[20:28]).view(np.uint8).copy()).cuda()
    d_acc = torch.full((8 * 48,), 0x5A, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    call = lambda n, spp, mode=COSINE: lib.rt_obscurance_surfels_device(h, mode, p(d_surfels), 8, None, n, C.byref(P), spp, 0, 0, 0,  # noqa: E731
                                                                          p(d_acc), None)
    assert call(0, 4) == 0 and call(8, (1 << 19) + 1) == -1 and call(8, 4, 7) == -1 and call(-1, 4) == -1
    torch.cuda.synchronize()
    assert (d_acc.cpu().numpy() == 0x5A).all()
    d_acc[:] = 0
    assert call(8, 4) == 0
    torch.cuda.synchronize()
    got = d_acc.cpu().numpy().view(rc.OBSCURANCE_DTYPE)
    assert (got["samples"] == 4).all() and got["hits"].sum() > 0


# ---------------------------------------------------------------- G9: nothing else moved
@pytest.mark.parametrize("traversal", ["AUTO", "BVH"])
def test_g9_the_renderer_the_counts_and_the_depth_bake_are_left_alone(rc, traversal):
    """A render_tile, a render_tile_1spp, rt_occluded_surfels_device and a depth bake before and after the new calls
    are bit-identical; the counters of rt_scene_get_stats, the rt_kernel_times ring and the build statistics are
    what they were."""
    import torch

    pos, nrm = surfel_set("bounce")
    gpu = _gpu(rc, "bounce", traversal, size=(128, 128))
    d_surfels = torch.from_numpy(rc._pack_surfels(pos, nrm).view(np.uint8).copy()).cuda()

    def counts():
        d_occ, d_ns = torch.zeros(N, dtype=torch.int32, device="cuda"), torch.zeros(N, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        gpu.occluded_surfels_device(COSINE, d_surfels, N, None, N, None, 6, SEED, 0, BASE, d_occ, d_ns)
        torch.cuda.synchronize()
        return d_occ.cpu().numpy(), d_ns.cpu().numpy()

    def depth():
        acc = gpu.render_probe_depth(pos[:24], 40, SEED, 1.5, normals=nrm[:24])
        return acc["depth"].cpu().numpy(), acc["counts"].cpu().numpy(), acc["D"].cpu().numpy()

    before = gpu.render_tile_1spp(40, 40, 24, 16, seed=3, sample_index=2)
    tile = gpu.render_tile(40, 40, 24, 16, 8, seed=3)
    occ, baked = counts(), depth()
    gpu.set_stats(True)
    gpu.render_tile(0, 0, 16, 16, 2, seed=4)
    assert sum(gpu.get_stats().values()) > 0  # (read and zeroed)
    launches = gpu.kernel_times(3)
    with pytest.raises(rc.RtError):
        gpu.kernel_times(4)
    stats = gpu.build_stats()
    acc = gpu.obscurance_surfels(pos, nrm, 40, SEED, RADIUS, 1, COSINE, stream_base=BASE)
    acc = gpu.obscurance_surfels(pos, nrm, 24, SEED, RADIUS, 1, COSINE, sample_base=40, stream_base=BASE, out=acc)
    loop = gpu.obscurance_adaptive(pos, nrm, 0.05, 16, 64, 16, seed=SEED, radius=1.0)
    assert (acc["samples"] == 64).all() and acc["hits"].sum() > 0 and len(loop["counts"]) >= 1
    with pytest.raises(rc.RtError):
        gpu.kernel_times(4)
    assert np.allclose(gpu.kernel_times(3), launches, rtol=1e-4, atol=0)
    assert sum(gpu.get_stats().values()) == 0
    assert gpu.build_stats() == stats
    gpu.set_stats(False)
    assert same_bits(gpu.render_tile_1spp(40, 40, 24, 16, seed=3, sample_index=2), before)
    after = gpu.render_tile(40, 40, 24, 16, 8, seed=3)
    assert all(same_bits(a, b) for a, b in zip(tile[:3], after[:3])) and tile[3] == after[3]
    assert all(same_bits(a, b) for a, b in zip(counts(), occ))
    assert all(same_bits(a, b) for a, b in zip(depth(), baked))
    gpu.close()
