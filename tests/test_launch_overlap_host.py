"""Launch overlap's two host decisions (launch_overlaps, overlap_wait through rt_debug_launch_overlap; no GPU)."""
import itertools
import os

import pytest

NONE, STREAM, HOST = 0, 1, 2
CHANGES = ("pkeys_rebuilt", "cull_fresh", "cull_replaced", "jit_rebuilt", "buffer_grown")
FREES = {"cull_replaced", "jit_rebuilt", "buffer_grown"}


@pytest.fixture(autouse=True)
def _clean_env():
    old = os.environ.pop("RTCORE_LAUNCH_OVERLAP", None)
    yield
    os.environ.pop("RTCORE_LAUNCH_OVERLAP", None)
    if old is not None:
        os.environ["RTCORE_LAUNCH_OVERLAP"] = old


def test_which_launches_overlap(rc):
    assert rc.launch_overlap()[0]
    assert not rc.launch_overlap(device_entry=False)[0]  # rt_render_tile, the list entries, rt_frame, the probe
    assert not rc.launch_overlap(repeats=False)[0]  # another width, height or spp than the launch before it
    assert not rc.launch_overlap(bvh=True)[0]  # the BVH kernels: measured slower beside each other
    assert not rc.launch_overlap(instrumented=True)[0]
    assert not rc.launch_overlap(tracing=True)[0]
    assert not rc.launch_overlap(instrumented=True, tracing=True)[0]


def test_byte_cap(rc):
    """4 GiB of partials for the second set: every bench.py launch of the brute-force kernels is far within it."""
    assert rc.launch_overlap(partial_bytes=2_123_366_400)[0]
    assert rc.launch_overlap(partial_bytes=4 << 30)[0]
    assert not rc.launch_overlap(partial_bytes=(4 << 30) + 1)[0]


def test_switch_is_read_per_launch(rc):
    os.environ["RTCORE_LAUNCH_OVERLAP"] = "0"
    assert not rc.launch_overlap()[0]
    os.environ["RTCORE_LAUNCH_OVERLAP"] = "1"
    assert rc.launch_overlap()[0]
    del os.environ["RTCORE_LAUNCH_OVERLAP"]
    assert rc.launch_overlap()[0]


def test_what_a_launch_waits_for(rc):
    """Nothing rewritten: no wait.  Freed memory: the host.  Otherwise the other set's kernel, on the stream."""
    for bits in itertools.product((False, True), repeat=len(CHANGES)):
        change = dict(zip(CHANGES, bits))
        on = {k for k, v in change.items() if v}
        want = NONE if not on else HOST if on & FREES else STREAM
        assert rc.launch_overlap(**change)[1] == want, change
        assert rc.launch_overlap(device_entry=False, **change)[1] == want  # (the wait does not depend on the launch)


def test_bad_arguments(rc):
    import ctypes as C

    lib = rc.load_library()
    wait = C.c_int32(0)
    assert lib.rt_debug_launch_overlap(32, 0, 0, C.byref(wait)) < 0
    assert lib.rt_debug_launch_overlap(0, 0, 32, C.byref(wait)) < 0
    assert lib.rt_debug_launch_overlap(0, 0, 0, None) < 0
