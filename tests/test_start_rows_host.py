"""The planning of the start rows (plan_start_rows through rt_debug_start_rows; host code, no GPU)."""
import os

import pytest


@pytest.fixture(autouse=True)
def _clean_env():
    old = {k: os.environ.pop(k, None) for k in ("RTCORE_START_ROWS", "RTCORE_PATH_CHUNKS")}
    yield
    for k, v in old.items():
        os.environ.pop(k, None)
        if v is not None:
            os.environ[k] = v


def _cam(scenes, name="bounce.txt", k=0):
    return scenes[name].cameras[k]


def test_headline_launch(rc, scenes):
    """1080p at 256 spp: 24 chunks of 11 samples, 1,792 blocks x 4 waves x 11 rows x 1 KiB."""
    for kernel in (0, 1):
        plan = rc.start_rows(kernel, _cam(scenes), 1920, 1080, 256, grid_blocks=1792)
        assert plan == {"on": True, "rows": 11, "bytes": 1792 * 4 * 11 * 1024, "chunk": 11}


def test_rows_follow_the_chunk_up_to_16(rc, scenes):
    cam = _cam(scenes)
    for chunks, spp, chunk in ((4, 37, 10), (1, 16, 16), (1, 17, 17), (2, 40, 20), (24, 1536, 64)):
        plan = rc.start_rows(0, cam, 256, 144, spp, chunks=chunks, grid_blocks=64)
        assert plan["chunk"] == chunk
        if chunk <= 16:
            assert plan == {"on": True, "rows": chunk, "bytes": 64 * 4 * chunk * 1024, "chunk": chunk}
        else:
            assert plan == {"on": False, "rows": 0, "bytes": 0, "chunk": chunk}
    os.environ["RTCORE_PATH_CHUNKS"] = "4"  # the launch's own override, read per call
    assert rc.start_rows(0, cam, 256, 144, 37, grid_blocks=64)["rows"] == 10


def test_cap(rc, scenes):
    """256 MiB: 16 rows are 64 KiB per block, so 4,096 blocks fit and 4,097 do not."""
    cam = _cam(scenes)
    assert rc.start_rows(0, cam, 256, 144, 16, chunks=1, grid_blocks=4096) == {
        "on": True, "rows": 16, "bytes": 256 << 20, "chunk": 16}
    assert not rc.start_rows(0, cam, 256, 144, 16, chunks=1, grid_blocks=4097)["on"]
    assert rc.start_rows(0, cam, 256, 144, 8, chunks=1, grid_blocks=8192)["on"]


def test_cameras_and_kernels(rc, scenes):
    cam = _cam(scenes)
    ortho = rc.rt_camera.from_buffer_copy(cam)
    ortho.kind = rc.RT_CAMERA_ORTHO
    assert not rc.start_rows(0, ortho, 256, 144, 37, chunks=4)["on"]
    assert not rc.start_rows(0, _cam(scenes, "die.txt"), 256, 144, 37, chunks=4)["on"]  # depth of field
    for k in range(len(scenes["bounce.txt"].cameras)):
        assert rc.start_rows(1, _cam(scenes, k=k), 256, 144, 37, chunks=4)["on"]
    for kernel in (2, 3):  # the BVH kernels
        assert not rc.start_rows(kernel, cam, 256, 144, 64)["on"]
    assert not rc.start_rows(0, cam, 256, 144, 37, chunks=4, instrumented=True)["on"]
    assert not rc.start_rows(0, cam, 256, 144, 37, chunks=4, vertex_normals=True)["on"]


def test_switch(rc, scenes):
    cam = _cam(scenes)
    os.environ["RTCORE_START_ROWS"] = "0"
    assert rc.start_rows(0, cam, 1920, 1080, 256) == {"on": False, "rows": 0, "bytes": 0, "chunk": 11}
    os.environ["RTCORE_START_ROWS"] = "1"
    assert rc.start_rows(0, cam, 1920, 1080, 256)["on"]


def test_bad_arguments(rc, scenes):
    cam = _cam(scenes)
    for args in ((4, cam, 8, 8, 1), (0, cam, 0, 8, 1), (0, cam, 8, 8, 0)):
        with pytest.raises(rc.RtError):
            rc.start_rows(*args)
    with pytest.raises(rc.RtError):
        rc.start_rows(0, cam, 8, 8, 1, grid_blocks=0)
