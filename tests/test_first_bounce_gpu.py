"""The first bounce on the device: a camera-ray query over the units a block can see changes no result.

In the iteration of the flat brute-force tile kernel in which every live lane of a wave holds a camera
ray (in a rounds ticket: once per round), a wave whose lanes are of one 8x8 block tests only the units
of the flat order whose bit is set in the block's mask (unit_masks, block_cull.cpp; trace_units,
rt_trace.h).
RTCORE_FIRST_BOUNCE=0 turns that off for the launches that follow.  A unit that is left out could not
have been met, so sums (byte for byte), samples, misses and the ray count must be the same with and
without: on the scene-specialised build and the generic one, for bounce.txt's cameras outside the room
and the one inside it (no cull record, so no masks), with every ticket in rounds, the rule's choice and
none, with waves that open their items together and out of step (which mixes blocks in a wave), items
of eleven samples and a short last one, a window at an offset, a band set of five rows, the 1-spp pass,
die.txt (depth of field: no cull record) and an instrumented launch, whose instances do not have it.
"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIZE = (256, 144)
WINDOWS = ((0, 0, 256, 144), (64, 32, 128, 72))
KEYS = ("RTCORE_FIRST_BOUNCE", "RTCORE_SAMPLE_ROUNDS", "RTCORE_PATH_CHUNKS", "RTCORE_ITEM_BATCH", "RTCORE_BLOCK_CULL_MIN",
        "RTCORE_BLOCK_CULL")


def _with(first, fn, **env):
    """fn() under RTCORE_FIRST_BOUNCE=first, RTCORE_BLOCK_CULL_MIN=1 and the given RTCORE_* settings."""
    old = {k: os.environ.pop(k, None) for k in KEYS}
    try:
        os.environ["RTCORE_BLOCK_CULL_MIN"] = "1"
        for k, v in env.items():
            os.environ["RTCORE_" + k] = str(v)
        if first is not None:
            os.environ["RTCORE_FIRST_BOUNCE"] = str(first)
        return fn()
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def _same(a, b):
    (sa, na, ma, ra), (sb, nb, mb, rb) = a, b
    return ra == rb and np.array_equal(na, nb) and np.array_equal(ma, mb) and sa.tobytes() == sb.tobytes()


def _gpu(rc, scene, cam=0):
    return rc.GpuRaytracer(scene, cam, size=SIZE, traversal=rc.RT_TRAVERSAL_BRUTE)


@pytest.mark.parametrize("jit", [True, False], ids=["specialised", "generic"])
@pytest.mark.parametrize("cam", [0, 3, 7, 1])
def test_first_bounce_changes_nothing(rc, scenes, jit, cam):
    scene = scenes["bounce.txt"]
    for window in WINDOWS:  # the masks are in use for the cameras outside the room, and leave units out
        u = rc.block_units(scene.prims, scene.cameras[cam], SIZE, window)
        assert u["on"] == (cam != 1)
        assert cam == 1 or (u["masks"] != (1 << u["n_units"]) - 1).any()
    rc.set_jit(jit)
    try:
        g = _gpu(rc, scene, cam)
        for window in WINDOWS:
            for spp, chunks in ((22, 2), (3, None)):  # items of 11 samples; 3 samples: a short only round
                for rounds in (0, 1, 2):
                    for batch in (64, 16):
                        env = {"SAMPLE_ROUNDS": rounds, "ITEM_BATCH": batch}
                        if chunks:
                            env["PATH_CHUNKS"] = chunks
                        run = lambda: g.render_tile(*window, spp, seed=5, sample_base=3)
                        off, on = _with(0, run, **env), _with(None, run, **env)
                        assert _same(off, on), (window, spp, rounds, batch)
                        assert (on[1] + on[2] == spp).all() and on[1].sum() > 0
            # the record with the masks appended is still the cull's record: a launch without any cull agrees
            run = lambda: g.render_tile(*window, 22, seed=5, sample_base=3)
            assert _same(_with(None, run, PATH_CHUNKS=2), _with(0, run, PATH_CHUNKS=2, BLOCK_CULL=0)), window
        if jit:
            assert g.build_stats()["jit_status"] == 1.0
        g.close()
    finally:
        rc.set_jit(True)


def test_band_set(rc, scenes):
    import torch

    g = _gpu(rc, scenes["bounce.txt"])
    W, H = SIZE
    band = 5
    plane = rc.band_slot_rows(H, band, 2) * W
    dev = torch.device("cuda", 0)

    def run():
        s_ = torch.zeros(3 * plane, dtype=torch.float64, device=dev)
        n_ = torch.zeros(plane, dtype=torch.int32, device=dev)
        m_ = torch.zeros(plane, dtype=torch.int32, device=dev)
        r_ = torch.zeros(1, dtype=torch.int64, device=dev)
        g.render_bands_device(band, 2, 1, 22, 7, 2, s_.data_ptr(), n_.data_ptr(), m_.data_ptr(), plane, r_.data_ptr(), 0)
        torch.cuda.synchronize()
        return s_.cpu().numpy(), n_.cpu().numpy(), m_.cpu().numpy(), int(r_.item())

    for rounds in (1, 2):
        off = _with(0, run, PATH_CHUNKS=2, SAMPLE_ROUNDS=rounds)
        on = _with(1, run, PATH_CHUNKS=2, SAMPLE_ROUNDS=rounds)
        assert _same(off, on) and on[1].sum() > 0
    g.close()


@pytest.mark.parametrize("jit", [True, False], ids=["specialised", "generic"])
def test_1spp_pass(rc, scenes, jit):
    rc.set_jit(jit)
    try:
        g = _gpu(rc, scenes["bounce.txt"])
        for window in WINDOWS:
            for rounds in (1, 2):
                run = lambda: g.render_tile_1spp(*window, seed=4, sample_index=9)
                off, on = _with(0, run, SAMPLE_ROUNDS=rounds), _with(1, run, SAMPLE_ROUNDS=rounds)
                assert off.tobytes() == on.tobytes() and (on >= 0).any()
        g.close()
    finally:
        rc.set_jit(True)


def test_die_is_unchanged(rc, scenes):
    """die.txt's camera has depth of field: no cull record, so no masks."""
    die = scenes["die.txt"]
    assert not rc.block_units(die.prims, die.cameras[0], SIZE)["on"]
    d = _gpu(rc, die)
    for rounds in (1, 2):
        run = lambda: d.render_tile(*WINDOWS[0], 22, seed=8)
        off = _with(0, run, PATH_CHUNKS=2, SAMPLE_ROUNDS=rounds)
        on = _with(1, run, PATH_CHUNKS=2, SAMPLE_ROUNDS=rounds)
        assert _same(off, on) and on[1].sum() > 0
    d.close()


def test_instrumented_launch_keeps_its_counters(rc, scenes):
    g = _gpu(rc, scenes["bounce.txt"])
    plain = _with(1, lambda: g.render_tile(*WINDOWS[0], 22, seed=6), PATH_CHUNKS=2)
    g.set_stats(True)

    def run():
        tile = g.render_tile(*WINDOWS[0], 22, seed=6)
        return tile, g.get_stats()

    (tile0, st0), (tile1, st1) = _with(0, run, PATH_CHUNKS=2), _with(1, run, PATH_CHUNKS=2)
    g.set_stats(False)
    assert _same(tile0, tile1) and _same(tile1, plain)
    for name in ("node_visits", "tri_tests", "sph_tests", "wave_iters"):  # the counters that are no clocks
        assert st0[name] == st1[name], name
    assert st1["wave_iters"] > 0
    g.close()
