"""Start rows on the device: building an item's camera rays when the item opens changes no result.

A brute-force tile launch with a frustum camera without depth of field keeps the camera rays of every
open item in a row buffer (run_path, plan_start_rows; refill in kernels_path.hip): the wave builds them
together at the item open and a lane's sample start loads its row.  RTCORE_START_ROWS=0 turns that off
for the launches that follow; sums (byte for byte), samples, misses and the ray count must be the same
with the rows and without, on the scene-specialised build and the generic one, in the flat and the
grouped order, with multi-row items, a short last item, items over the row cap, ragged windows, band
sets, the 1-spp pass, other cameras, items opened out of step, the block cull on and off, a sample base
past 2^32, and a buffer that is reused and regrown; an instrumented launch reports the counters it
always has.
"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIZE = (256, 144)
FRAME = (0, 0, 256, 144)
RAGGED = (3, 5, 203, 77)
KEYS = ("RTCORE_START_ROWS", "RTCORE_PATH_CHUNKS", "RTCORE_ITEM_BATCH", "RTCORE_BLOCK_CULL", "RTCORE_BLOCK_CULL_MIN")


def _with_rows(on, fn, **env):
    """fn() with the start rows on (the default) or off, under the given RTCORE_* settings."""
    old = {k: os.environ.pop(k, None) for k in KEYS}
    try:
        for k, v in env.items():
            os.environ["RTCORE_" + k] = str(v)
        if not on:
            os.environ["RTCORE_START_ROWS"] = "0"
        return fn()
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def _same(a, b):
    (sa, na, ma, ra), (sb, nb, mb, rb) = a, b
    return ra == rb and np.array_equal(na, nb) and np.array_equal(ma, mb) and sa.tobytes() == sb.tobytes()


def _gpu(rc, scene, mode, cam=0):
    return rc.GpuRaytracer(scene, cam, size=SIZE, traversal=getattr(rc, "RT_TRAVERSAL_" + mode))


def _both(fn, **env):
    on, off = _with_rows(True, fn, **env), _with_rows(False, fn, **env)
    return on, off


# (RTCORE_PATH_CHUNKS, spp): items of 10 samples and a short last one of 7; one sample per item (the
# small frame's own chunks); items of 20 samples, over the row cap, so the launch does without rows
SHAPES = ((4, 37), (None, 5), (2, 40))


@pytest.mark.parametrize("jit", [True, False], ids=["specialised", "generic"])
@pytest.mark.parametrize("mode", ["BRUTE", "GROUPED"])
def test_rows_change_nothing(rc, scenes, mode, jit):
    rc.set_jit(jit)
    try:
        g = _gpu(rc, scenes["bounce.txt"], mode)
        cam = scenes["bounce.txt"].cameras[0]
        for chunks, spp in SHAPES:
            env = {} if chunks is None else {"PATH_CHUNKS": chunks}
            for window, base in ((FRAME, 3), (RAGGED, 2 ** 32 + 3)):
                on, off = _both(lambda: g.render_tile(*window, spp, seed=5, sample_base=base), **env)
                assert _same(on, off), (chunks, spp, window)
                assert (on[1] + on[2] == spp).all() and on[1].sum() > 0
            plan = _with_rows(True, lambda: rc.start_rows(0 if mode == "BRUTE" else 1, cam, 256, 144, spp), **env)
            assert plan["on"] == (chunks != 2) and plan["chunk"] == {4: 10, None: 1, 2: 20}[chunks]
        if jit:
            assert g.build_stats()["jit_status"] == 1.0
        g.close()
    finally:
        rc.set_jit(True)


@pytest.mark.parametrize("mode", ["BRUTE", "GROUPED"])
def test_band_set(rc, scenes, mode):
    import torch

    g = _gpu(rc, scenes["bounce.txt"], mode)
    W, H = SIZE
    band = 5
    plane = rc.band_slot_rows(H, band, 2) * W
    dev = torch.device("cuda", 0)

    def run():
        s_ = torch.zeros(3 * plane, dtype=torch.float64, device=dev)
        n_ = torch.zeros(plane, dtype=torch.int32, device=dev)
        m_ = torch.zeros(plane, dtype=torch.int32, device=dev)
        r_ = torch.zeros(1, dtype=torch.int64, device=dev)
        g.render_bands_device(band, 2, 1, 37, 7, 2, s_.data_ptr(), n_.data_ptr(), m_.data_ptr(), plane, r_.data_ptr(), 0)
        torch.cuda.synchronize()
        return s_.cpu().numpy(), n_.cpu().numpy(), m_.cpu().numpy(), int(r_.item())

    on, off = _both(run, PATH_CHUNKS=4)
    assert _same(on, off) and on[1].sum() > 0
    g.close()


@pytest.mark.parametrize("jit", [True, False], ids=["specialised", "generic"])
def test_1spp_pass(rc, scenes, jit):
    rc.set_jit(jit)
    try:
        g = _gpu(rc, scenes["bounce.txt"], "BRUTE")
        for window in (FRAME, RAGGED):
            on, off = _both(lambda: g.render_tile_1spp(*window, seed=4, sample_index=9))
            assert on.tobytes() == off.tobytes() and (on >= 0).any()
        g.close()
    finally:
        rc.set_jit(True)


def _ortho(rc, scenes):
    cam = rc.rt_camera.from_buffer_copy(scenes["bounce.txt"].cameras[0])
    cam.kind = rc.RT_CAMERA_ORTHO
    return cam


@pytest.mark.parametrize("mode", ["BRUTE", "GROUPED"])
def test_cameras(rc, scenes, mode):
    """Camera 1 stands inside the room (no block is culled), camera 4 has 120 degrees; an orthographic
    camera and die.txt's depth of field do not qualify: the launches run without rows either way."""
    kernel = 0 if mode == "BRUTE" else 1
    g = _gpu(rc, scenes["bounce.txt"], mode)
    cams = scenes["bounce.txt"].cameras
    for cam, qualifies in ((cams[1], True), (cams[4], True), (_ortho(rc, scenes), False), (cams[0], True)):
        g.set_camera(cam)
        on, off = _both(lambda: g.render_tile(*FRAME, 37, seed=8, sample_base=1), PATH_CHUNKS=4)
        assert _same(on, off) and (on[1] + on[2] == 37).all()
        assert _with_rows(True, lambda: rc.start_rows(kernel, cam, 256, 144, 37), PATH_CHUNKS=4)["on"] == qualifies
    g.close()
    d = _gpu(rc, scenes["die.txt"], mode)
    on, off = _both(lambda: d.render_tile(*FRAME, 37, seed=8), PATH_CHUNKS=4)
    assert _same(on, off) and on[1].sum() > 0
    assert not _with_rows(True, lambda: rc.start_rows(kernel, scenes["die.txt"].cameras[0], 256, 144, 37), PATH_CHUNKS=4)["on"]
    d.close()


@pytest.mark.parametrize("mode", ["BRUTE", "GROUPED"])
def test_items_opened_out_of_step_and_the_block_cull(rc, scenes, mode):
    g = _gpu(rc, scenes["bounce.txt"], mode)
    ref = _with_rows(False, lambda: g.render_tile(*FRAME, 37, seed=9, sample_base=2), PATH_CHUNKS=4)
    for env in ({"ITEM_BATCH": 0}, {"ITEM_BATCH": 8}, {"BLOCK_CULL_MIN": 1}, {"BLOCK_CULL": 0}):
        on, off = _both(lambda: g.render_tile(*FRAME, 37, seed=9, sample_base=2), PATH_CHUNKS=4, **env)
        assert _same(on, off) and _same(on, ref), env
    g.close()


@pytest.mark.parametrize("jit", [True, False], ids=["specialised", "generic"])
def test_buffer_is_reused_and_regrown(rc, scenes, jit):
    """One scene object: a small window first (a small grid, so a small buffer), two seeds on it, then
    the frame at more samples (a larger grid), then the small window again."""
    rc.set_jit(jit)
    try:
        launches = (((64, 40, 64, 48), 13, 1), ((64, 40, 64, 48), 13, 2), (FRAME, 37, 1), (FRAME, 150, 2),
                    ((64, 40, 64, 48), 13, 1))

        def run():
            g = _gpu(rc, scenes["bounce.txt"], "BRUTE")
            out = [g.render_tile(*w, spp, seed=seed) for w, spp, seed in launches]
            g.close()
            return out

        on, off = _both(run, PATH_CHUNKS=16)
        assert all(_same(a, b) for a, b in zip(on, off))
        assert _same(on[0], on[4]) and not _same(on[0], on[1])
    finally:
        rc.set_jit(True)


@pytest.mark.parametrize("mode", ["BRUTE", "GROUPED"])
def test_instrumented_launch_keeps_its_counters(rc, scenes, mode):
    g = _gpu(rc, scenes["bounce.txt"], mode)
    plain = _with_rows(True, lambda: g.render_tile(*FRAME, 37, seed=6), PATH_CHUNKS=4)
    g.set_stats(True)

    def run():
        tile = g.render_tile(*FRAME, 37, seed=6)
        return tile, g.get_stats()

    (t_on, st_on), (t_off, st_off) = _both(run, PATH_CHUNKS=4)
    g.set_stats(False)
    assert _same(t_on, t_off) and _same(t_on, plain)
    for name in ("node_visits", "tri_tests", "sph_tests", "wave_iters"):  # the counters that are no clocks
        assert st_on[name] == st_off[name], name
    assert st_on["wave_iters"] > 0
    g.close()
