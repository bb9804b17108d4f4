"""Sample rounds on the device: holding a wave's lanes back so that they start their samples together
changes no result.

A brute-force tile launch may run a ticket's samples in rounds (refill in kernels_path.hip,
ticket_rounds in rt_kernels.h): a lane whose sample has ended starts its next one only once no lane of
its wave is live.  RTCORE_SAMPLE_ROUNDS=0 turns that off for the launches that follow, 2 forces it on
every ticket and 1 (the default) lets each wave choose per ticket.  Only when a sample starts depends
on the setting, so sums (byte for byte), samples, misses and the ray count must be the same under all
three: on the scene-specialised build and the generic one, in the flat and the grouped order, for
bounce.txt's cameras outside and inside the room, with multi-sample items and a short last one, one
sample per item, many tickets per wave, ragged windows, items opened out of step, the block cull on
and off, no start rows, a band set, the 1-spp pass and a sample base past 2^32; die.txt gives forced
rounds the most ragged path lengths; an instrumented launch reports the counters it always has; and
rt_render_rays and rt_render_pixels, which have no rounds, return what they did.
"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIZE = (256, 144)
FRAME = (0, 0, 256, 144)
RAGGED = (3, 5, 203, 77)
KEYS = ("RTCORE_SAMPLE_ROUNDS", "RTCORE_START_ROWS", "RTCORE_PATH_CHUNKS", "RTCORE_ITEM_BATCH", "RTCORE_BLOCK_CULL",
        "RTCORE_BLOCK_CULL_MIN")
SETTINGS = (0, 1, 2)


def _with_rounds(setting, fn, **env):
    """fn() under RTCORE_SAMPLE_ROUNDS=setting and the given RTCORE_* settings."""
    old = {k: os.environ.pop(k, None) for k in KEYS}
    try:
        for k, v in env.items():
            os.environ["RTCORE_" + k] = str(v)
        os.environ["RTCORE_SAMPLE_ROUNDS"] = str(setting)
        return fn()
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def _all(fn, **env):
    return [_with_rounds(s, fn, **env) for s in SETTINGS]


def _same(a, b):
    (sa, na, ma, ra), (sb, nb, mb, rb) = a, b
    return ra == rb and np.array_equal(na, nb) and np.array_equal(ma, mb) and sa.tobytes() == sb.tobytes()


def _all_same(outs):
    return all(_same(outs[0], o) for o in outs[1:])


def _gpu(rc, scene, mode, cam=0):
    return rc.GpuRaytracer(scene, cam, size=SIZE, traversal=getattr(rc, "RT_TRAVERSAL_" + mode))


# (RTCORE_PATH_CHUNKS, spp): items of 10 samples and a short last one of 7; one sample per item (the
# small frame's own chunks); one sample per item in 64 chunks, so that a wave draws many tickets and
# the rule is asked past its first
SHAPES = ((4, 37), (None, 5), (64, 64))


@pytest.mark.parametrize("jit", [True, False], ids=["specialised", "generic"])
@pytest.mark.parametrize("mode", ["BRUTE", "GROUPED"])
@pytest.mark.parametrize("cam", [0, 1])
def test_rounds_change_nothing(rc, scenes, mode, jit, cam):
    rc.set_jit(jit)
    try:
        g = _gpu(rc, scenes["bounce.txt"], mode, cam)
        for chunks, spp in SHAPES:
            env = {} if chunks is None else {"PATH_CHUNKS": chunks}
            for window, base in ((FRAME, 3), (RAGGED, 2 ** 32 + 3)):
                outs = _all(lambda: g.render_tile(*window, spp, seed=5, sample_base=base), **env)
                assert _all_same(outs), (chunks, spp, window)
                assert (outs[0][1] + outs[0][2] == spp).all() and outs[0][1].sum() > 0
        if jit:
            assert g.build_stats()["jit_status"] == 1.0
        g.close()
    finally:
        rc.set_jit(True)


@pytest.mark.parametrize("mode", ["BRUTE", "GROUPED"])
def test_items_opened_out_of_step_cull_and_rows(rc, scenes, mode):
    g = _gpu(rc, scenes["bounce.txt"], mode)
    ref = _with_rounds(0, lambda: g.render_tile(*FRAME, 37, seed=9, sample_base=2), PATH_CHUNKS=4)
    for env in ({"ITEM_BATCH": 0}, {"ITEM_BATCH": 8}, {"BLOCK_CULL_MIN": 1}, {"BLOCK_CULL": 0}, {"START_ROWS": 0},
                {"START_ROWS": 0, "ITEM_BATCH": 8}):
        for window in (FRAME, RAGGED):
            outs = _all(lambda: g.render_tile(*window, 37, seed=9, sample_base=2), PATH_CHUNKS=4, **env)
            assert _all_same(outs), (env, window)
            assert window != FRAME or _same(outs[0], ref), env
    g.close()


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

    outs = _all(run, PATH_CHUNKS=4)
    assert _all_same(outs) and outs[0][1].sum() > 0
    g.close()


@pytest.mark.parametrize("jit", [True, False], ids=["specialised", "generic"])
def test_1spp_pass(rc, scenes, jit):
    rc.set_jit(jit)
    try:
        g = _gpu(rc, scenes["bounce.txt"], "BRUTE")
        for window in (FRAME, RAGGED):
            outs = _all(lambda: g.render_tile_1spp(*window, seed=4, sample_index=9))
            assert all(o.tobytes() == outs[0].tobytes() for o in outs) and (outs[0] >= 0).any()
        g.close()
    finally:
        rc.set_jit(True)


@pytest.mark.parametrize("jit", [True, False], ids=["specialised", "generic"])
@pytest.mark.parametrize("mode", ["BRUTE", "GROUPED"])
def test_die_ragged_paths(rc, scenes, mode, jit):
    """die.txt: depth of field, a mean of 1.2 rays per sample and a few long paths; forced rounds make
    every lane wait for those."""
    rc.set_jit(jit)
    try:
        d = _gpu(rc, scenes["die.txt"], mode)
        for env in ({"PATH_CHUNKS": 4}, {"PATH_CHUNKS": 4, "ITEM_BATCH": 8}, {"PATH_CHUNKS": 64}):
            outs = _all(lambda: d.render_tile(*FRAME, 37, seed=8), **env)
            assert _all_same(outs) and outs[0][1].sum() > 0, env
        d.close()
    finally:
        rc.set_jit(True)


@pytest.mark.parametrize("mode", ["BRUTE", "GROUPED"])
def test_instrumented_launch_keeps_its_counters(rc, scenes, mode):
    g = _gpu(rc, scenes["bounce.txt"], mode)
    plain = _with_rounds(1, lambda: g.render_tile(*FRAME, 37, seed=6), PATH_CHUNKS=4)
    g.set_stats(True)

    def run():
        tile = g.render_tile(*FRAME, 37, seed=6)
        return tile, g.get_stats()

    outs = _all(run, PATH_CHUNKS=4)
    g.set_stats(False)
    for tile, st in outs:
        assert _same(tile, outs[0][0]) and _same(tile, plain)
        for name in ("node_visits", "tri_tests", "sph_tests", "wave_iters"):  # the counters that are no clocks
            assert st[name] == outs[0][1][name], name
    assert outs[0][1]["wave_iters"] > 0
    g.close()


@pytest.mark.parametrize("mode", ["BRUTE", "GROUPED"])
def test_ray_and_pixel_lists_are_unchanged(rc, scenes, mode):
    g = _gpu(rc, scenes["bounce.txt"], mode)
    W, H = SIZE
    rays = rc.camera_rays(scenes["bounce.txt"].cameras[0], SIZE, 96, 40, 24, 16)
    pixels = (np.arange(40, 56)[:, None] * W + np.arange(96, 120)[None, :]).reshape(-1)[::-1]
    outs_r = _all(lambda: g.render_rays(rays, None, 37, 7, sample_base=2, stream_base=11))
    outs_p = _all(lambda: g.render_pixels(pixels, 37, seed=7, sample_base=2))
    assert _all_same(outs_r) and outs_r[0][1].sum() > 0
    assert _all_same(outs_p) and outs_p[0][1].sum() > 0
    # the pixel list gives what the tile gives wherever both have the same samples per item (both: 2 here)
    tile = _with_rounds(2, lambda: g.render_tile(96, 40, 24, 16, 37, seed=7, sample_base=2), PATH_CHUNKS=24)
    sp, np_, mp, _ = outs_p[0]
    assert np.array_equal(np_[96:120, 40:56], tile[1]) and np.array_equal(mp[96:120, 40:56], tile[2])
    g.close()
