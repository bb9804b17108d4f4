"""The block cull on the device: a launch over the live blocks alone changes no result.

A brute-force launch is planned over the 8x8 blocks whose pixels can see the scene (run_path,
block_cull.cpp); the pixels of the others are counted as spp primary misses and rays.
RTCORE_BLOCK_CULL=0 turns that off for the launches that follow and RTCORE_BLOCK_CULL_MIN=1 culls
launches of any size; sums, samples, misses and the ray count must be bit-identical with the cull and
without, on the scene-specialised build and the generic one, in the flat and the grouped order, over
tiles, ragged windows, band sets, the 1-spp pass and rt_frame, with the record rebuilt and reused across
camera changes, and an instrumented launch must report the counters it always has.
"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIZE = (256, 144)


def _with_cull(on, fn):
    """fn() with every launch culled (threshold 1) or with the cull off."""
    old = {k: os.environ.pop(k, None) for k in ("RTCORE_BLOCK_CULL", "RTCORE_BLOCK_CULL_MIN")}
    try:
        os.environ["RTCORE_BLOCK_CULL_MIN"] = "1"
        if not on:
            os.environ["RTCORE_BLOCK_CULL"] = "0"
        return fn()
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def _same(a, b):
    (sa, na, ma, ra), (sb, nb, mb, rb) = a, b
    return ra == rb and np.array_equal(na, nb) and np.array_equal(ma, mb) and sa.tobytes() == sb.tobytes()


def _gpu(rc, scenes, mode, cam=0):
    return rc.GpuRaytracer(scenes["bounce.txt"], cam, size=SIZE, traversal=getattr(rc, "RT_TRAVERSAL_" + mode))


def _dead_pixels(rc, scenes, cam, window):
    """[w, h] mask of the window's pixels in dead blocks, by the host reporter."""
    dead, _ = rc.block_cull(scenes["bounce.txt"].prims, scenes["bounce.txt"].cameras[cam], SIZE, window)
    x0, y0, w, h = window
    return np.kron(dead.astype(np.uint8), np.ones((8, 8), np.uint8))[:h, :w].T.astype(bool)


@pytest.mark.parametrize("jit", [True, False], ids=["specialised", "generic"])
@pytest.mark.parametrize("mode", ["BRUTE", "GROUPED"])
def test_cull_changes_nothing(rc, scenes, mode, jit):
    """Whole frame at 5 spp (a short last chunk) and 48 spp, a ragged offset window, an all-dead window,
    two seeds."""
    rc.set_jit(jit)
    try:
        g = _gpu(rc, scenes, mode)
        for window, spp, seed in (((0, 0, 256, 144), 5, 5), ((0, 0, 256, 144), 48, 5), ((0, 0, 256, 144), 5, 11),
                                  ((3, 5, 203, 77), 5, 5), ((3, 5, 203, 77), 48, 11), ((0, 0, 64, 64), 5, 5)):
            on = _with_cull(True, lambda: g.render_tile(*window, spp, seed=seed, sample_base=3))
            off = _with_cull(False, lambda: g.render_tile(*window, spp, seed=seed, sample_base=3))
            assert _same(on, off), (window, spp, seed)
            s, n, m, rays = on
            dead = _dead_pixels(rc, scenes, 0, window)
            assert (m[dead] == spp).all() and (n[dead] == 0).all() and not s[dead].any()
            assert (n + m == spp).all()
            if window == (0, 0, 64, 64):  # the frame's top-left corner: every block dead, one ray per sample
                assert dead.all() and rays == 64 * 64 * spp
            else:
                assert 0.3 < dead.mean() < 0.9 and n.sum() > 0 and rays > window[2] * window[3] * spp
        if jit:
            assert g.build_stats()["jit_status"] == 1.0
        g.close()
    finally:
        rc.set_jit(True)


@pytest.mark.parametrize("mode", ["BRUTE", "GROUPED"])
@pytest.mark.parametrize("band", [8, 5])
def test_band_sets(rc, scenes, mode, band):
    import torch

    g = _gpu(rc, scenes, mode)
    W, H = SIZE
    plane = rc.band_slot_rows(H, band, 2) * W
    dev = torch.device("cuda", 0)

    def run():
        s_ = torch.zeros(3 * plane, dtype=torch.float64, device=dev)
        n_ = torch.zeros(plane, dtype=torch.int32, device=dev)
        m_ = torch.zeros(plane, dtype=torch.int32, device=dev)
        r_ = torch.zeros(1, dtype=torch.int64, device=dev)
        g.render_bands_device(band, 2, 1, 6, 7, 2, s_.data_ptr(), n_.data_ptr(), m_.data_ptr(), plane, r_.data_ptr(), 0)
        torch.cuda.synchronize()
        return s_.cpu().numpy(), n_.cpu().numpy(), m_.cpu().numpy(), int(r_.item())

    on, off = _with_cull(True, run), _with_cull(False, run)
    assert _same(on, off)
    rows = rc.band_rows_count(H, band, 2, 1)
    dead, live = rc.block_cull(scenes["bounce.txt"].prims, scenes["bounce.txt"].cameras[0], SIZE, None, (band, 2, 1))
    assert 0 < live < dead.size
    mask = np.kron(dead.astype(np.uint8), np.ones((8, 8), np.uint8))[:rows, :W].astype(bool).ravel()
    assert (on[2][:rows * W][mask] == 6).all() and (on[1][:rows * W][mask] == 0).all()
    assert on[1].sum() > 0
    g.close()


@pytest.mark.parametrize("jit", [True, False], ids=["specialised", "generic"])
def test_1spp_pass_writes_the_placeholder(rc, scenes, jit):
    rc.set_jit(jit)
    try:
        g = _gpu(rc, scenes, "BRUTE")
        for window in ((0, 0, 256, 144), (3, 5, 203, 77)):
            on = _with_cull(True, lambda: g.render_tile_1spp(*window, seed=4, sample_index=9))
            off = _with_cull(False, lambda: g.render_tile_1spp(*window, seed=4, sample_index=9))
            assert on.tobytes() == off.tobytes()
            dead = _dead_pixels(rc, scenes, 0, window)
            assert (on[dead] == -1.0).all() and (on[~dead] >= 0).any()
        g.close()
    finally:
        rc.set_jit(True)


def test_frame_one_gpu(rc, scenes):
    f = rc.GpuFrame(scenes["bounce.txt"], 0, n_gpus=1, size=SIZE)
    on = _with_cull(True, lambda: f.render(6, seed=3, sample_base=1))
    off = _with_cull(False, lambda: f.render(6, seed=3, sample_base=1))
    f.close()
    assert _same(on, off)
    assert (on[1] + on[2] == 6).all() and on[1].sum() > 0 and on[2].sum() > 0.5 * 6 * SIZE[0] * SIZE[1]


@pytest.mark.parametrize("mode", ["BRUTE", "GROUPED"])
def test_record_follows_the_camera(rc, scenes, mode):
    """Camera 0, camera 1 (inside the room: nothing dead), camera 0 again, camera 2: the record is
    rebuilt on a camera change and reused between, with several windows alive at once."""
    cams = scenes["bounce.txt"].cameras
    g = _gpu(rc, scenes, mode)
    windows = ((0, 0, 256, 144), (3, 5, 203, 77), (128, 0, 128, 144), (0, 72, 256, 72), (64, 16, 96, 96))

    def run():
        out = []
        for k in (0, 1, 0, 2):
            g.set_camera(cams[k])
            for rep in range(2):
                for window in windows:
                    out.append(g.render_tile(*window, 4, seed=2 + rep, sample_base=rep))
        return out

    on, off = _with_cull(True, run), _with_cull(False, run)
    assert len(on) == 40 and all(_same(a, b) for a, b in zip(on, off))
    per_cam = [sum(int(r[2].sum()) for r in on[10 * i:10 * i + 10]) for i in range(4)]
    assert per_cam[0] == per_cam[2] > 0 and per_cam[1] == 0 and per_cam[3] > 0
    g.close()


@pytest.mark.parametrize("mode", ["BRUTE", "GROUPED"])
def test_instrumented_launch_keeps_its_counters(rc, scenes, mode):
    g = _gpu(rc, scenes, mode)
    g.set_stats(True)

    def run():
        tile = g.render_tile(0, 0, 256, 144, 4, seed=6)
        return tile, g.get_stats()

    (t_on, st_on), (t_off, st_off) = _with_cull(True, run), _with_cull(False, run)
    g.set_stats(False)
    assert _same(t_on, t_off)
    for name in ("node_visits", "tri_tests", "sph_tests", "wave_iters"):  # the counters that are no clocks
        assert st_on[name] == st_off[name], name
    assert st_on["wave_iters"] > 0
    assert _same(_with_cull(True, lambda: g.render_tile(0, 0, 256, 144, 4, seed=6)), t_on)
    g.close()
