"""Adaptive light probes on the device: rt_render_probe_list_device, rt_probe_select_device and the loop.

G1: promises 1 and 2 (the identity list is rt_render_probes_device, with and without moments).  G2: promise 3
(the moments are the host twin's and the numpy replay's over the per-sample results).  G3: promises 4 to 6
(a list, entries skipped and untouched, a + b samples).  G4: the selection pass against its host twin.  G5: the
furnace.  G6: the loop against a replay driven by the host twin, and against direct calls.  G7: errors, empty
calls and what a call leaves alone.

The probes are the 200 surfels of tests/test_render_surfels_gpu.py (three full waves and a short fourth; BAD
lists the three invalid ones); the scenes are 128 x 128."""
import ctypes as C

import numpy as np
import pytest

from probe_list_cases import moments_replay
from test_query_rays_gpu import _gpu, _same_bits
from test_render_probes_gpu import GOOD, _yardstick
from test_render_surfels_gpu import BAD, BASE, FURNACE, N, SEED, _last_error, _surfels
from test_render_surfels_host import SPHERE

pytestmark = pytest.mark.gpu

PAD = 64  # sentinel elements on either side of every device array


class Acc:
    """Device accumulators of n probes with PAD sentinel elements round each array."""

    def __init__(self, n, sh=None, ns=None, nm=None, mom=None):
        import torch

        self.n = n
        host = [np.full(2 * PAD + 36 * n, 2.5), np.full(2 * PAD + n, 7, np.int32), np.full(2 * PAD + n, 9, np.int32),
                np.full(2 * PAD + 8 * n, 3.5)]
        for buf, a, per in zip(host, (sh, ns, nm, mom), (36, 1, 1, 8)):
            buf[PAD:PAD + per * n] = 0 if a is None else np.asarray(a).reshape(-1).view(buf.dtype)
        self.t = [torch.from_numpy(b).cuda() for b in host]
        self.rays = torch.full((3,), 41, dtype=torch.int64, device="cuda")

    @property
    def ptrs(self):
        return [t[PAD:] for t in self.t]

    def get(self):
        """(sh [n, 9, 4], samples u32, misses u32, moments [n, 4, 2], rays), the sentinels checked."""
        import torch

        torch.cuda.synchronize()
        n = self.n
        out = []
        for t, per, fill in zip(self.t, (36, 1, 1, 8), (2.5, 7, 9, 3.5)):
            a = t.cpu().numpy()
            assert (a[:PAD] == fill).all() and (a[PAD + per * n:] == fill).all()
            out.append(a[PAD:PAD + per * n])
        r = self.rays.cpu().tolist()
        assert r[0] == 41 and r[2] == 41
        return out[0].reshape(n, 9, 4), out[1].view(np.uint32), out[2].view(np.uint32), out[3].reshape(n, 4, 2), r[1] - 41

    def render(self, gpu, d_probes, index, spp, sample_base=0, moments=True, stream=0, n_records=None):
        import torch

        d_index = None if index is None else torch.from_numpy(np.asarray(index, np.uint32).view(np.int32).copy()).cuda()
        sh, ns, nm, mom = self.ptrs
        gpu.render_probe_list_device(d_probes, self.n if n_records is None else n_records, d_index,
                                     self.n if index is None else len(index), spp, SEED, sample_base, BASE, sh, ns, nm,
                                     mom if moments else 0, self.rays[1:].data_ptr(), stream)
        return self


def _probes(rc, name="bounce"):
    import torch

    pos, nrm = _surfels(name)
    return torch.from_numpy(rc._pack_surfels(pos, nrm).view(np.uint8).copy()).cuda()


def _start(n=N, seed=9):
    rng = np.random.default_rng(seed)
    return (rng.normal(size=(n, 9, 4)), np.full(n, 3, np.uint32), np.full(n, 4, np.uint32), rng.uniform(0.0, 2.0, (n, 4, 2)))


# ---------------------------------------------------------------- G1: promises 1 and 2
@pytest.mark.parametrize("name,mode,spp", [("bounce", "BRUTE", 5), ("bounce", "BVH", 130), ("die", "GROUPED", 7)])
def test_g1_identity_list_is_render_probes_device(rc, name, mode, spp):
    gpu = _gpu(rc, name, mode, size=(128, 128))
    assert gpu.info().traversal == getattr(rc, "RT_TRAVERSAL_" + mode)
    d_probes = _probes(rc, name)
    start = _start()
    ref = Acc(N, *start)
    sh, ns, nm, _ = ref.ptrs
    gpu.render_probes_device(d_probes, N, spp, SEED, 2, BASE, sh, ns, nm, ref.rays[1:].data_ptr())
    want = ref.get()
    plain = Acc(N, *start).render(gpu, d_probes, None, spp, 2, moments=False).get()
    with_m = Acc(N, *start).render(gpu, d_probes, None, spp, 2, moments=True).get()
    gpu.close()
    for got in (plain, with_m):
        assert _same_bits(got[0], want[0]) and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
        assert got[4] == want[4] > 0
    assert _same_bits(plain[3], start[3]) and not _same_bits(with_m[3], start[3])  # no moments: the array untouched
    assert not _same_bits(want[0], start[0]) and ((want[1] - 3) + (want[2] - 4) == spp).all()
    assert _same_bits(with_m[3][BAD], start[3][BAD])


# ---------------------------------------------------------------- G2: promise 3
@pytest.fixture(scope="module")
def bounce_bvh(rc):
    gpu = _gpu(rc, "bounce", "BVH", size=(128, 128))
    yield gpu
    gpu.close()


@pytest.fixture(scope="module")
def acc50(rc, bounce_bvh):
    """bounce, BVH, 50 spp from zero with moments: (sh, samples, misses, moments, rays) on the host."""
    return Acc(N).render(bounce_bvh, _probes(rc), None, 50).get()


@pytest.mark.parametrize("mode,spp", [("BRUTE", 5), ("BVH", 50)])
def test_g2_moments_are_the_host_twins(rc, mode, spp):
    pos, nrm = _surfels("bounce")
    gpu = _gpu(rc, "bounce", mode, size=(128, 128))
    rays, rgb, miss, total = _yardstick(gpu, pos, nrm, spp)
    got = Acc(N).render(gpu, _probes(rc), None, spp).get()
    start = _start()
    cont = Acc(N, *start).render(gpu, _probes(rc), None, spp).get()
    gpu.close()
    twin = rc.probe_moments_host(rays, rgb, miss)
    assert _same_bits(got[3], twin) and _same_bits(got[3], moments_replay(rays, rgb, miss))
    assert _same_bits(cont[3], rc.probe_moments_host(rays, rgb, miss, out=start[3].copy()))
    fold = rc.probe_fold_host(rays, rgb, miss)
    assert _same_bits(got[0], fold[0]) and np.array_equal(got[1], fold[1]) and np.array_equal(got[2], fold[2]) and got[4] == total
    assert not got[3][BAD].any() and (got[2][BAD] == spp).all()
    hits, skies = int((got[3][GOOD][:, :, 0] > 0).all(axis=1).sum()), int((got[3][GOOD][:, 0, 1] > 0).sum())
    print(f"G2 {mode} spp {spp}: {hits} probes with m[.][0] > 0, {skies} with m[0][1] > 0")
    assert hits > N // 4 and skies > 0


# ---------------------------------------------------------------- G3: promises 4 to 6
LIST = [199, 64, 0, 65, 63, 200, 7]


@pytest.mark.parametrize("mode", ["BRUTE", "BVH"])
def test_g3_a_list_names_entries(rc, mode):
    gpu = _gpu(rc, "bounce", mode, size=(128, 128))
    d_probes = _probes(rc)
    start = _start()
    full = Acc(N, *start).render(gpu, d_probes, None, 6, 2).get()
    got = Acc(N, *start).render(gpu, d_probes, LIST, 6, 2).get()
    named = [e for e in LIST if e < N]
    rest = np.setdiff1d(np.arange(N), named)
    for a, b, s in zip(got[:4], full[:4], start):
        assert _same_bits(a[named], b[named]) and _same_bits(a[rest], s[rest])
        assert not _same_bits(b[rest], s[rest])
    assert 0 < got[4] < full[4]
    assert got[2][7] == 4 + 6 and _same_bits(got[0][7], start[0][7]) and _same_bits(got[3][7], start[3][7])  # 7 is invalid
    # the same entries at other list positions, in a longer array of records (the first N are the same records)
    import torch

    longer = torch.cat([d_probes, d_probes[:64 * 40]])
    moved = Acc(N + 40, *[np.concatenate([s, s[:40]]) for s in start]).render(gpu, longer, named[::-1] + [N + 3], 6, 2).get()
    for a, b in zip(moved[:4], full[:4]):
        assert _same_bits(a[named], b[named])
    # 20 + 30 samples are 50, moments included
    one = Acc(N, *start).render(gpu, d_probes, LIST, 50, 3).get()
    two = Acc(N, *start).render(gpu, d_probes, LIST, 20, 3)
    mid = two.get()
    two = two.render(gpu, d_probes, LIST, 30, 23).get()
    gpu.close()
    for a, b, m in zip(two[:4], one[:4], mid[:4]):
        assert _same_bits(a, b) and not _same_bits(m, b)
    assert two[4] == one[4]


# ---------------------------------------------------------------- G4: the selection pass
def _select_device(rc, par, acc, cap=None, stream=0):
    """probe_select_device over host accumulators uploaded between sentinels: (list, count)."""
    import torch

    dev = Acc(N, *acc[:4])
    cap = N if cap is None else cap
    d_list = torch.full((PAD + cap + PAD,), -5, dtype=torch.int32, device="cuda")
    d_count = torch.full((3,), -5, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    sh, ns, nm, mom = dev.ptrs
    rc.probe_select_device(par, sh, ns, nm, mom, N, d_list[PAD:], cap, d_count[1:], stream=stream)
    torch.cuda.synchronize()
    after = dev.get()
    assert all(_same_bits(a, b) for a, b in zip(after[:4], acc[:4]))  # inputs only
    lst, cnt = d_list.cpu().numpy(), d_count.cpu().numpy()
    assert cnt[0] == -5 and cnt[2] == -5
    count = int(cnt[1]) & 0xFFFFFFFF
    k = min(count, cap)
    assert (lst[:PAD] == -5).all() and (lst[PAD + k:] == -5).all()
    return lst[PAD:PAD + k].view(np.uint32), count


# (se / max(level, irr_floor) of these accumulators has the quartiles 1.15, 1.45, 1.84: profiles/probe_list/measure.log)
@pytest.mark.parametrize("rel_tol", [0.1, 1.5, 2.0])
def test_g4_select_device_is_the_host_twin(rc, bounce_bvh, acc50, rel_tol):
    import torch

    amb = bounce_bvh.params.ambient
    par = rc.probe_select_params(rel_tol, 16, 1000, amb)
    want, count = rc.probe_select_host(par, *acc50[:4])
    got, got_count = _select_device(rc, par, acc50)
    print(f"G4 rel_tol {rel_tol}: {count} of {N} active")
    assert got_count == count and np.array_equal(got, want) and (np.diff(want.astype(np.int64)) > 0).all()
    assert not set(BAD) & set(want.tolist())
    cap = count // 2
    got, got_count = _select_device(rc, par, acc50, cap=cap)
    assert got_count == count and np.array_equal(got, want[:cap])
    side = torch.cuda.Stream()
    got, got_count = _select_device(rc, par, acc50, stream=side.cuda_stream)
    assert got_count == count and np.array_equal(got, want)
    # below min: all; at max: none
    got, got_count = _select_device(rc, rc.probe_select_params(rel_tol, 51, 1000, amb), acc50)
    assert got_count == N and np.array_equal(got, np.arange(N))
    got, got_count = _select_device(rc, rc.probe_select_params(0.0, 16, 50, amb), acc50)
    assert got_count == 0


# ---------------------------------------------------------------- G5: the furnace
def test_g5_furnace(rc):
    """Inside an inverted sphere that only emits (.5, .5, .5): level = pi / 2, se = pi / sqrt(N), so
    at rel_tol 0.25 a probe stops about N = 64; 48 .. 96 allowed (tests/test_probe_list_host.py, H4)."""
    scene = rc.SceneLoader.from_text(FURNACE)
    gpu = rc.GpuRaytracer(scene, 0)
    rng = np.random.default_rng(3)
    g = rng.normal(size=(64, 3))
    pos = g / np.linalg.norm(g, axis=1, keepdims=True) * (2.0 * rng.uniform(0, 1, (64, 1)) ** (1 / 3))
    res = gpu.bake_probes_adaptive(pos, 0.25, 16, 256, 16, seed=SEED, normals=rng.normal(size=(64, 3)))
    gpu.close()
    spp = res["spp"].cpu().numpy()
    print(f"G5: stops at N = {dict(zip(*np.unique(spp, return_counts=True)))}, counts {res['counts']}")
    assert (spp >= 48).all() and (spp <= 96).all() and not res["misses"].cpu().numpy().any()
    assert res["counts"][0] == 64 and res["rays"] == int(spp.sum())
    par = res["params"]
    se, level = rc.probe_error(par, res["sh"].cpu().numpy(), res["samples"].cpu().numpy().view(np.uint32),
                               res["misses"].cpu().numpy().view(np.uint32), res["moments"].cpu().numpy())
    assert np.abs(level - np.pi / 2.0).max() <= 1e-12 and (se <= 0.25 * level).all()


# ---------------------------------------------------------------- G6: the loop
def _host(res):
    return (res["sh"].cpu().numpy(), res["samples"].cpu().numpy().view(np.uint32), res["misses"].cpu().numpy().view(np.uint32),
            res["moments"].cpu().numpy())


def test_g6_loop_runs_every_valid_probe_to_max(rc, bounce_bvh):
    """rel_tol = 1e-6: no probe with any variance converges before max_spp; the three invalid ones have se = 0
    and the level at the floor, and leave right after min_spp: two list lengths, with no tuning.
    min_spp = 1024: bounce.txt's lights are small and its ambient colour is black, so a valid probe whose samples
    so far all came back black has c = m = 0 and se = 0 exactly, like an invalid one, and leaves at min_spp too
    ("what the rule cannot see").  Of these 197 valid probes that is 40, 22, 17, 6, 2 and 0 after 32,
    50, 64, 128, 256 and 1024 samples at this seed (profiles/probe_list/measure.log), so from 1024 samples on
    "valid" and "has seen light" are the same set here.  200 x 2048 samples are a few milliseconds."""
    pos, nrm = _surfels("bounce")
    res = bounce_bvh.bake_probes_adaptive(pos, 1e-6, 1024, 2048, 512, seed=SEED, normals=nrm, stream_base=BASE, sample_base=5)
    assert res["counts"] == [N] * 2 + [N - 3] * 2
    par = res["params"]
    assert (par.min_samples, par.max_samples) == (1024, 2048)
    amb = bounce_bvh.params.ambient
    assert (par.ambient.r, par.ambient.g, par.ambient.b) == (amb.r, amb.g, amb.b)
    # the loop again, driven by the host twin over accumulators that direct calls continue
    d_probes = _probes(rc)
    replay = Acc(N)
    for it, lst in enumerate(res["lists"]):
        want, count = rc.probe_select_host(par, *replay.get()[:4])
        assert count == res["counts"][it] and np.array_equal(lst.cpu().numpy().view(np.uint32), want), it
        replay.render(bounce_bvh, d_probes, want, 512, 5 + 512 * it)
    final = replay.get()
    assert rc.probe_select_host(par, *final[:4])[1] == 0
    got = _host(res)
    assert all(_same_bits(a, b) for a, b in zip(got, final[:4])) and res["rays"] == final[4]
    # each entry's result is one direct call at spp = N
    spp = res["spp"].cpu().numpy()
    assert (spp[BAD] == 1024).all() and (spp[GOOD] == 2048).all()
    for n_spp in (1024, 2048):
        direct = Acc(N).render(bounce_bvh, d_probes, None, n_spp, 5).get()
        at = np.flatnonzero(spp == n_spp)
        assert all(_same_bits(a[at], b[at]) for a, b in zip(got, direct[:4]))


G6_TOL = 0.5  # (profiles/probe_list/measure.log: of 0.05 .. 0.5 the one at which most probes stopped early, 70 of 197)


def test_g6_loop_at_a_moderate_tolerance(rc, bounce_bvh):
    pos, nrm = _surfels("bounce")
    res = bounce_bvh.bake_probes_adaptive(pos, G6_TOL, 16, 256, 16, seed=SEED, normals=nrm, stream_base=BASE)
    spp = res["spp"].cpu().numpy()
    early = int((spp[GOOD] < 256).sum())
    print(f"G6 rel_tol {G6_TOL}: {early} of {len(GOOD)} valid probes stopped before 256 spp, counts {res['counts']}, "
          f"{int(spp.sum())} samples of {N * 256}")
    lst, count = rc.probe_select_host(res["params"], *_host(res))
    assert count == 0 and len(lst) == 0
    assert res["counts"][0] == N and all(a >= b for a, b in zip(res["counts"], res["counts"][1:]))


# ---------------------------------------------------------------- G7: errors and what a call leaves alone
def test_g7_empty_calls_and_errors_touch_nothing(rc, bounce_bvh):
    import torch

    lib, h = bounce_bvh.lib, bounce_bvh.handle
    d_probes = _probes(rc)
    acc = Acc(N, *_start())
    before = acc.get()
    d_index = torch.arange(128, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    sh, ns, nm, mom = (C.c_void_p(t.data_ptr()) for t in acc.ptrs)
    pp, ix = C.c_void_p(d_probes.data_ptr()), C.c_void_p(d_index.data_ptr())
    call = lambda *a: lib.rt_render_probe_list_device(h, *a)  # noqa: E731
    assert call(pp, N, ix, 0, 4, SEED, 0, 0, sh, ns, nm, mom, None, None) == 0          # n == 0
    assert call(None, 0, None, 0, 1, 0, 0, 0, None, None, None, None, None, None) == 0
    for args, word in (((pp, N, ix, -1, 4), "n < 0"), ((pp, N, ix, 8, 0), "spp <= 0"), ((None, N, ix, 8, 4), "null pointer"),
                       ((pp, 0, ix, 8, 4), "n_records <= 0"), ((pp, -2, ix, 8, 4), "n_records <= 0"),
                       ((pp, 1 << 32, ix, 8, 4), "2^32"), ((pp, N, None, 8, 4), "n != n_records")):
        assert call(*args, SEED, 0, 0, sh, ns, nm, mom, None, None) == -1, args
        assert "rt_render_probe_list_device" in _last_error(lib) and word in _last_error(lib), (args, _last_error(lib))
    for null in range(3):
        out = [sh, ns, nm]
        out[null] = None
        assert call(pp, N, ix, 8, 4, SEED, 0, 0, *out, mom, None, None) == -1 and "null pointer" in _last_error(lib)
    # the bound on the list length: 64 * ceil(n / 64) * pow2ceil(spp) <= 2^26, whatever n_records is
    for n, spp in ((64, 1 << 21), (65, 1 << 20), (64, (1 << 20) + 1), ((1 << 26) + 1, 1), ((1 << 20) + 1, 33), (64, 2 ** 31 - 1)):
        assert call(pp, 1 << 30, ix, n, spp, SEED, 0, 0, sh, ns, nm, mom, None, None) == -1, (n, spp)
        assert "2^26" in _last_error(lib) and "sample_base" in _last_error(lib)
    gpu2 = _gpu(rc, "bounce", "BVH2")
    assert gpu2.lib.rt_render_probe_list_device(gpu2.handle, pp, N, ix, 8, 4, SEED, 0, 0, sh, ns, nm, mom, None, None) == -7
    assert "BVH2" in _last_error(lib) and "rt_render_probe_list_device" in _last_error(lib)
    gpu2.close()
    after = acc.get()
    assert all(_same_bits(a, b) for a, b in zip(after[:4], before[:4])) and after[4] == before[4] == 0
    # the select pass's device-side refusals
    par = rc.probe_select_params(0.1, 1, 8)
    assert lib.rt_probe_select_device(C.byref(par), sh, ns, nm, mom, N, None, 4, ix, None) == -1
    assert lib.rt_probe_select_device(C.byref(par), sh, ns, nm, None, N, ix, 4, ix, None) == -1
    assert (d_index.cpu().numpy() == np.arange(128)).all()
    # and the same call with nothing wrong works, continuing from what is there
    assert call(pp, N, ix, 8, 4, SEED, 0, 0, sh, ns, nm, mom, None, None) == 0
    now = acc.get()
    assert ((now[1][:8] - 3) + (now[2][:8] - 4) == 4).all() and _same_bits(now[0][8:], before[0][8:])


@pytest.mark.parametrize("mode", ["AUTO", "BVH"])
def test_g7_calls_leave_the_renderer_alone(rc, mode):
    pos, nrm = _surfels("bounce")
    gpu = _gpu(rc, "bounce", mode, size=(128, 128))
    before = gpu.render_tile_1spp(40, 40, 24, 16, seed=3, sample_index=2)
    tile = gpu.render_tile(40, 40, 24, 16, 8, seed=3)
    gather = gpu.render_surfels(pos, nrm, 30, SEED, SPHERE, stream_base=5)
    probes = gpu.render_probes(pos, 6, SEED, normals=nrm, stream_base=5)
    gpu.set_stats(True)
    gpu.render_tile(0, 0, 16, 16, 2, seed=4)
    assert sum(gpu.get_stats().values()) > 0  # (read and zeroed)
    launches = gpu.kernel_times(3)
    with pytest.raises(rc.RtError):
        gpu.kernel_times(4)
    stats = gpu.build_stats()
    d_probes = _probes(rc)
    Acc(N).render(gpu, d_probes, LIST, 6).render(gpu, d_probes, None, 40, moments=False).get()
    gpu.bake_probes_adaptive(pos, 0.5, 16, 32, 16, seed=SEED, normals=nrm)
    with pytest.raises(rc.RtError):
        gpu.kernel_times(4)
    assert np.allclose(gpu.kernel_times(3), launches, rtol=1e-4, atol=0)
    assert sum(gpu.get_stats().values()) == 0
    assert gpu.build_stats() == stats
    gpu.set_stats(False)
    assert _same_bits(gpu.render_tile_1spp(40, 40, 24, 16, seed=3, sample_index=2), before)
    after = gpu.render_tile(40, 40, 24, 16, 8, seed=3)
    assert all(_same_bits(a, b) for a, b in zip(tile[:3], after[:3])) and tile[3] == after[3]
    again = gpu.render_surfels(pos, nrm, 30, SEED, SPHERE, stream_base=5)
    assert all(_same_bits(a, b) for a, b in zip(gather[:3], again[:3])) and gather[3] == again[3]
    again = gpu.render_probes(pos, 6, SEED, normals=nrm, stream_base=5)
    assert all(_same_bits(a, b) for a, b in zip(probes[:3], again[:3])) and probes[3] == again[3]
    gpu.close()
