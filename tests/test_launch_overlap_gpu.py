"""Launch overlap on the device: consecutive device renders on two launch sets change no result.

rt_render_device and rt_render_bands_device run launch k's path kernel on the stream of launch set k & 1,
beside the tail of launch k - 1, and fold its partials on the caller's stream (run_path, scene_upload.hip).
What can go wrong is ordering and buffer reuse, so the launches are small and queued without a host sync,
and every comparison is bit for bit -- sums, samples, misses and the ray counts -- against the same call
sequence under RTCORE_LAUNCH_OVERLAP=0 in the same process: a path kernel that does not wait for the fold
of two launches ago, a fold out of order, a buffer or a record replaced under a kernel in flight, pixel keys
of the wrong seed, a serial launch (a host tile, an instrumented launch) among overlapped ones, two caller
streams, band sets.  RTCORE_BLOCK_CULL_MIN=1 throughout, so that these small windows have cull records.
"""
import os
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SPP = 16
COMBOS = {"flat": ("bounce.txt", "RT_TRAVERSAL_BRUTE"), "grouped": ("die.txt", "RT_TRAVERSAL_GROUPED"),
          "bvh": ("bounce.txt", "RT_TRAVERSAL_BVH")}


@pytest.fixture(scope="module")
def torch():
    return pytest.importorskip("torch")


@pytest.fixture(scope="module")
def gpus(rc, scenes):
    """One scene object per combination at 64 x 64, and the flat one again at 96 x 96."""
    made = {}

    def get(combo, size=64):
        if (combo, size) not in made:
            name, trav = COMBOS[combo]
            made[combo, size] = rc.GpuRaytracer(scenes[name], 0, size=(size, size), traversal=getattr(rc, trav))
        return made[combo, size]

    yield get
    for g in made.values():
        g.close()


class Acc:
    """Device accumulators of a w x h window and a ray counter."""

    def __init__(self, torch, w, h):
        self.sum = torch.zeros(3 * w * h, dtype=torch.float64, device="cuda")
        self.n = torch.zeros(w * h, dtype=torch.int32, device="cuda")
        self.m = torch.zeros(w * h, dtype=torch.int32, device="cuda")

    def arrays(self):
        return [self.sum.cpu().numpy(), self.n.cpu().numpy(), self.m.cpu().numpy()]


def _render(g, acc, rays, stream, window, k, seed=3, spp=SPP):
    g.render_device(*window, spp, seed, k * spp, acc.sum.data_ptr(), acc.n.data_ptr(), acc.m.data_ptr(), rays.data_ptr(),
                    stream.cuda_stream)


def _both(torch, scenario):
    """scenario() with overlap off (the reference) and on; each returns a list of arrays after its own sync."""
    old = {k: os.environ.pop(k, None) for k in ("RTCORE_LAUNCH_OVERLAP", "RTCORE_BLOCK_CULL_MIN")}
    try:
        os.environ["RTCORE_BLOCK_CULL_MIN"] = "1"
        os.environ["RTCORE_LAUNCH_OVERLAP"] = "0"
        ref = scenario()
        torch.cuda.synchronize()
        del os.environ["RTCORE_LAUNCH_OVERLAP"]
        got = scenario()
        torch.cuda.synchronize()
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
    assert len(ref) == len(got)
    for i, (a, b) in enumerate(zip(ref, got)):
        a, b = np.asarray(a), np.asarray(b)
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), f"array {i} differs"
    return ref


def _some_light(ref_arrays):
    assert any(np.asarray(a).dtype == np.float64 and np.asarray(a).sum() > 0 for a in ref_arrays)


@pytest.mark.parametrize("combo", sorted(COMBOS))
def test_six_launches_six_accumulators(rc, torch, gpus, combo):
    """Each launch set is reused three times: a kernel that overwrote partials not yet folded would show."""
    g = gpus(combo)
    win = (0, 0, 64, 64)

    def scenario():
        st = torch.cuda.Stream()
        with torch.cuda.stream(st):
            accs = [Acc(torch, 64, 64) for _ in range(6)]
            rays = torch.zeros(1, dtype=torch.int64, device="cuda")
            st.synchronize()
            for k in range(6):
                _render(g, accs[k], rays, st, win, k)
            st.synchronize()
            return [a for acc in accs for a in acc.arrays()] + [rays.cpu().numpy()]

    ref = _both(torch, scenario)
    _some_light(ref)
    assert all((ref[3 * k + 1].astype(np.int64) + ref[3 * k + 2] == SPP).all() for k in range(6))
    assert ref[0].tobytes() != ref[3].tobytes()  # (rising sample_base: the launches differ)


@pytest.mark.parametrize("combo", sorted(COMBOS))
def test_six_launches_one_accumulator(rc, torch, gpus, combo):
    """The folds keep the caller's stream order: fp64 sums added in another order would differ in bits."""
    g = gpus(combo)
    win = (0, 0, 64, 64)

    def scenario():
        st = torch.cuda.Stream()
        with torch.cuda.stream(st):
            acc = Acc(torch, 64, 64)
            rays = torch.zeros(1, dtype=torch.int64, device="cuda")
            st.synchronize()
            for k in range(6):
                _render(g, acc, rays, st, win, k)
            st.synchronize()
            return acc.arrays() + [rays.cpu().numpy()]

    ref = _both(torch, scenario)
    assert (ref[1].astype(np.int64) + ref[2] == 6 * SPP).all() and int(ref[3][0]) > 0


@pytest.mark.parametrize("combo", sorted(COMBOS))
def test_ray_counts_follow_the_stream(rc, torch, gpus, combo):
    """d_rays zeroed on the stream between calls, read on the stream after each: per-launch counts."""
    g = gpus(combo)
    win = (0, 0, 64, 64)

    def scenario():
        st = torch.cuda.Stream()
        with torch.cuda.stream(st):
            acc = Acc(torch, 64, 64)
            rays = torch.zeros(1, dtype=torch.int64, device="cuda")
            st.synchronize()
            seen = []
            for k in range(6):
                if k % 2 == 0:
                    rays.zero_()
                _render(g, acc, rays, st, win, k)
                seen.append(rays.clone())
            st.synchronize()
            return acc.arrays() + [torch.cat(seen).cpu().numpy()]

    ref = _both(torch, scenario)
    counts = ref[3]
    assert (counts > 0).all() and (counts[1::2] > counts[0::2]).all()  # zeroed before the even ones, added to by the odd


def test_work_buffers_grow_and_shrink(rc, torch, gpus):
    """32 x 32, 96 x 96, 32 x 32 ...: the sets' buffers are reallocated, and each window has its own cull record.
    A launch overlaps the one before it when it repeats its size, so each size comes again at once."""
    g = gpus("flat", 96)
    sizes = (32, 96, 32, 32, 32, 96, 96, 96, 64, 64, 32, 32)

    def scenario():
        st = torch.cuda.Stream()
        with torch.cuda.stream(st):
            accs = [Acc(torch, n, n) for n in sizes]
            rays = torch.zeros(1, dtype=torch.int64, device="cuda")
            st.synchronize()
            for k, n in enumerate(sizes):
                _render(g, accs[k], rays, st, (0, 0, n, n), k)
            st.synchronize()
            return [a for acc in accs for a in acc.arrays()] + [rays.cpu().numpy()]

    _some_light(_both(torch, scenario))
    # a scene object whose first launches are overlapped: every buffer of both sets starts empty
    scene = rc.SceneLoader.from_file(rc.scene_path("bounce.txt"))
    fresh = []

    def scenario_fresh():
        fresh.append(rc.GpuRaytracer(scene, 0, size=(96, 96), traversal=rc.RT_TRAVERSAL_BRUTE))
        g2 = fresh[-1]
        st = torch.cuda.Stream()
        with torch.cuda.stream(st):
            accs = [Acc(torch, n, n) for n in sizes]
            rays = torch.zeros(1, dtype=torch.int64, device="cuda")
            st.synchronize()
            for k, n in enumerate(sizes):
                _render(g2, accs[k], rays, st, (96 - n, 0, n, n), k)
            st.synchronize()
            return [a for acc in accs for a in acc.arrays()] + [rays.cpu().numpy()]

    try:
        _both(torch, scenario_fresh)
    finally:
        for g2 in fresh:
            g2.close()


def test_seed_changes_between_launches(rc, torch, gpus):
    """A new seed rebuilds the pixel keys, which the other set's kernel may still be reading."""
    g = gpus("flat")
    seeds = (3, 3, 9, 9, 3, 11)

    def scenario():
        st = torch.cuda.Stream()
        with torch.cuda.stream(st):
            accs = [Acc(torch, 64, 64) for _ in seeds]
            rays = torch.zeros(1, dtype=torch.int64, device="cuda")
            st.synchronize()
            for k, seed in enumerate(seeds):
                _render(g, accs[k], rays, st, (0, 0, 64, 64), k, seed=seed)
            st.synchronize()
            return [a for acc in accs for a in acc.arrays()] + [rays.cpu().numpy()]

    _some_light(_both(torch, scenario))


@pytest.mark.parametrize("between", ["tile", "stats"])
def test_serial_launch_between_device_renders(rc, torch, gpus, between):
    """rt_render_tile (host buffers, the scene's own stream) or an instrumented launch among overlapped ones."""
    g = gpus("flat")
    win = (0, 0, 64, 64)

    def scenario():
        st = torch.cuda.Stream()
        with torch.cuda.stream(st):
            accs = [Acc(torch, 64, 64) for _ in range(5)]
            rays = torch.zeros(1, dtype=torch.int64, device="cuda")
            st.synchronize()
            _render(g, accs[0], rays, st, win, 0)
            _render(g, accs[1], rays, st, win, 1)
            if between == "tile":
                extra = list(g.render_tile(8, 8, 40, 24, SPP, seed=5, sample_base=7))
                extra[3] = np.asarray([extra[3]], np.int64)
            else:
                g.set_stats(True)
                try:
                    _render(g, accs[4], rays, st, win, 9)
                finally:
                    g.set_stats(False)
                extra = []
            _render(g, accs[2], rays, st, win, 2)
            _render(g, accs[3], rays, st, win, 3)
            st.synchronize()
            return [a for acc in accs for a in acc.arrays()] + [rays.cpu().numpy()] + extra

    _some_light(_both(torch, scenario))


def test_two_caller_streams(rc, torch, gpus):
    """Launches alternate between two caller streams and add into one accumulator set: the library orders them."""
    g = gpus("flat")
    win = (0, 0, 64, 64)

    def scenario():
        sts = [torch.cuda.Stream(), torch.cuda.Stream()]
        acc = Acc(torch, 64, 64)
        own = [Acc(torch, 64, 64) for _ in range(6)]
        rays = torch.zeros(1, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        for k in range(6):
            _render(g, acc, rays, sts[k % 2], win, k)
            _render(g, own[k], rays, sts[k % 2], win, 6 + k)
        torch.cuda.synchronize()
        return acc.arrays() + [a for o in own for a in o.arrays()] + [rays.cpu().numpy()]

    ref = _both(torch, scenario)
    assert (ref[1].astype(np.int64) + ref[2] == 6 * SPP).all()


def test_band_sets_back_to_back(rc, torch, gpus):
    """rt_render_bands_device, band stride 2: both offsets queued back to back, three steps."""
    from raytracercore_amd import sharding

    g = gpus("flat", 96)
    W = H = 96
    plane = sharding.slot_rows(H, 2, sharding.BAND) * W

    def scenario():
        st = torch.cuda.Stream()
        with torch.cuda.stream(st):
            slots = [torch.zeros(4 * plane, dtype=torch.float64, device="cuda") for _ in range(2)]
            rays = torch.zeros(1, dtype=torch.int64, device="cuda")
            st.synchronize()
            for k in range(3):
                for off in range(2):
                    s_, n_, m_ = sharding.slot_views(slots[off], plane)
                    g.render_bands_device(sharding.BAND, 2, off, SPP, 3, k * SPP, s_.data_ptr(), n_.data_ptr(), m_.data_ptr(),
                                          plane, rays.data_ptr(), st.cuda_stream)
            st.synchronize()
            return [s.cpu().numpy() for s in slots] + [rays.cpu().numpy()]

    ref = _both(torch, scenario)
    assert ref[0].sum() > 0 and ref[1].sum() > 0 and int(ref[2][0]) > 0


def test_kernel_times(rc, torch, gpus):
    """n positive entries whose sum fits the host's time between the syncs around the launches; with overlap
    off they are the raw event pairs (the predecessor of every launch, the ring's 65th pair for the oldest,
    ended before it began), with overlap on never more than those."""
    g = gpus("flat", 96)
    win = (0, 0, 96, 96)
    n = 8
    st = torch.cuda.Stream()
    old = {k: os.environ.pop(k, None) for k in ("RTCORE_LAUNCH_OVERLAP", "RTCORE_BLOCK_CULL_MIN")}
    try:
        for mode in ("0", None):
            if mode is not None:
                os.environ["RTCORE_LAUNCH_OVERLAP"] = mode
            else:
                os.environ.pop("RTCORE_LAUNCH_OVERLAP", None)
            with torch.cuda.stream(st):
                acc = Acc(torch, 96, 96)
                rays = torch.zeros(1, dtype=torch.int64, device="cuda")
                _render(g, acc, rays, st, win, 0, spp=64)  # (buffers, records and keys in place)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for k in range(n):
                    _render(g, acc, rays, st, win, 1 + k, spp=64)
                torch.cuda.synchronize()
                wall_ms = (time.perf_counter() - t0) * 1e3
            ms = g.kernel_times(n)
            raw = g.kernel_times_raw(n)
            if mode == "0":
                assert ms == raw
                # the whole ring, wrapped: 70 serial launches, the oldest entry's predecessor in the 65th pair
                with torch.cuda.stream(st):
                    for k in range(70):
                        _render(g, acc, rays, st, (0, 0, 32, 32), 100 + k, spp=4)
                    torch.cuda.synchronize()
                assert g.kernel_times(64) == g.kernel_times_raw(64)
            else:
                assert all(a <= b for a, b in zip(ms, raw))
            print(f"overlap {mode or 'on'}: kernel ms {[round(v, 4) for v in ms]} sum {sum(ms):.4f} host {wall_ms:.4f}")
            assert len(ms) == n and all(v > 0 for v in ms)
            assert sum(ms) <= wall_ms * 1.001
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
