"""Adaptive sampling on the device: rt_adaptive_select_device against its host twin (A1), and the driver
loop GpuRaytracer.render_adaptive held to the rule it is built on (A2, A3)."""
import numpy as np
import pytest

from adaptive_cases import FRAMES, LUM_FLOOR, MAX_SAMPLES, MIN_SAMPLES, REL_TOL, make_accumulators
from test_query_rays_gpu import _gpu, _same_bits

pytestmark = pytest.mark.gpu

SEED = 11


# ---------------------------------------------------------------- A1: the device pass against the host twin
@pytest.mark.parametrize("width,height", FRAMES)
@pytest.mark.parametrize("plane_pad", [0, 37])
def test_a1_device_select_equals_the_host_twin(rc, width, height, plane_pad):
    """The synthetic accumulators of tests/test_adaptive_host.py: the same list, in the same order, and
    the same count, with cap at, above and below the count and with planes further apart than the frame."""
    import torch

    npix = width * height
    acc = make_accumulators(width, height, seed=width * 1000 + height, plane=npix + plane_pad if plane_pad else 0)
    par = rc.rt_adaptive_params(REL_TOL, LUM_FLOOR, MIN_SAMPLES, MAX_SAMPLES)
    want, count = rc.adaptive_select_host(par, acc["sum"], acc["samples"], acc["misses"], acc["q"], acc["batches"], width,
                                          height, plane=acc["plane"])
    assert 0 < count == want.size < npix
    dev = [torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()
           for a in (acc["sum"], acc["samples"], acc["misses"], acc["q"], acc["batches"])]
    for cap in (npix, count, count // 2, 1, 0):
        out = torch.full((npix + 1,), -7, dtype=torch.int32, device="cuda")
        d_count = torch.full((1,), -1, dtype=torch.int32, device="cuda")
        rc.adaptive_select_device(par, *[a.data_ptr() for a in dev], width, height, out.data_ptr() if cap else 0, cap,
                                  d_count.data_ptr(), plane=acc["plane"])
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        assert int(d_count.item()) == count, cap
        k = min(cap, count)
        assert np.array_equal(got[:k].view(np.uint32), want[:k]), cap
        assert (got[k:] == -7).all(), cap  # nothing past the list, nothing past cap
    # on a side stream, twice: the pass's scratch is shared, the calls are ordered
    side = torch.cuda.Stream()
    out = torch.zeros(npix, dtype=torch.int32, device="cuda")
    d_count = torch.zeros(1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    for stream in (side.cuda_stream, 0, side.cuda_stream):
        rc.adaptive_select_device(par, *[a.data_ptr() for a in dev], width, height, out.data_ptr(), npix, d_count.data_ptr(),
                                  plane=acc["plane"], stream=stream)
    torch.cuda.synchronize()
    assert int(d_count.item()) == count and np.array_equal(out.cpu().numpy()[:count].view(np.uint32), want)


# ---------------------------------------------------------------- A2 / A3: the driver loop
TOL, MIN_SPP, MAX_SPP, BATCH = 0.3, 8, 64, 8


@pytest.fixture(scope="module")
def adaptive(rc):
    gpu = _gpu(rc, "bounce", "AUTO", size=(128, 128))
    res = gpu.render_adaptive(TOL, MIN_SPP, MAX_SPP, BATCH, seed=SEED)
    yield gpu, res
    gpu.close()


def _host_layout(res):
    """render_adaptive's device tensors as whole-frame arrays in render_pixels' [x, y] layout."""
    return (np.ascontiguousarray(res["sum"].cpu().numpy().transpose(2, 1, 0)),
            np.ascontiguousarray(res["samples"].cpu().numpy().T).view(np.uint32),
            np.ascontiguousarray(res["misses"].cpu().numpy().T).view(np.uint32),
            np.ascontiguousarray(res["q"].cpu().numpy().T),
            np.ascontiguousarray(res["batches"].cpu().numpy().T).view(np.uint32))


def _twin(rc, par, acc, W, H):
    """The host twin on [x, y] arrays."""
    return rc.adaptive_select_host(par, acc[0].transpose(2, 1, 0), acc[1].T, acc[2].T, acc[3].T, acc[4].T, W, H)


def test_a2_render_adaptive_obeys_the_rule(rc, adaptive):
    """bounce 128 x 128, min 8, max 64, batches of 8, rel_tol 0.3.  The loop ends; every N is a multiple of 8
    in [8, 64]; some pixels stop early and some reach the cap; the list sizes never grow; the total is below
    64 x pixels; background-only pixels stop at 8.  Replayed on the host from the returned lists with
    rt_render_pixels: at every iteration the host twin names exactly the list the device pass made (so every
    pixel with N >= 16 was active on the accumulators it had at N - 8, and every pixel is inactive on those it
    ended with), and the replay's accumulators are the loop's, bit for bit.  A second run gives the same bits."""
    gpu, res = adaptive
    W, H = gpu.width, gpu.height
    par = res["params"]
    assert (par.min_samples, par.max_samples) == (MIN_SPP, MAX_SPP)
    N = res["spp"].cpu().numpy()
    counts = res["counts"]
    print(f"A2: list sizes {counts}, samples {int(N.sum())} of {MAX_SPP * W * H} "
          f"({N.sum() / (MAX_SPP * W * H):.1%}), N histogram {np.bincount(N.reshape(-1) // BATCH).tolist()}")
    assert len(counts) == MAX_SPP // BATCH or counts[-1] > 0
    assert (N % BATCH == 0).all() and N.min() >= MIN_SPP and N.max() <= MAX_SPP
    assert (N < MAX_SPP).any() and (N == MAX_SPP).any()
    assert (N[N < MAX_SPP] > MIN_SPP).any()  # stopped by the tolerance, not only by all-miss pixels
    assert counts[0] == W * H and all(a >= b for a, b in zip(counts, counts[1:]))
    assert int(N.sum()) == BATCH * sum(counts) < MAX_SPP * W * H
    acc = _host_layout(res)
    background = (gpu.render_tile(0, 0, W, H, 1, seed=SEED)[1] == 0) & (acc[1] == 0)  # [x, y]: no hit ever
    assert background.any() and (N.T[background] == MIN_SPP).all()
    # the replay
    rep = (np.zeros((W, H, 3)), np.zeros((W, H), np.uint32), np.zeros((W, H), np.uint32), np.zeros((W, H)),
           np.zeros((W, H), np.uint32))
    rays = 0
    for it, lst in enumerate(res["lists"]):
        lst = lst.cpu().numpy().view(np.uint32)
        want, n = _twin(rc, par, rep, W, H)
        assert n == counts[it] and np.array_equal(lst, want), it
        rays += gpu.render_pixels(lst, BATCH, seed=SEED, sample_base=it * BATCH, out=rep, moments=True)[3]
    assert _twin(rc, par, rep, W, H)[1] == 0
    assert all(_same_bits(a, b) for a, b in zip(rep, acc)) and rays == res["rays"]
    again = gpu.render_adaptive(TOL, MIN_SPP, MAX_SPP, BATCH, seed=SEED)
    assert again["counts"] == counts and all(_same_bits(a, b) for a, b in zip(_host_layout(again), acc))


def test_a3_a_pixel_alone(rc, adaptive):
    """A pixel that ended with N samples holds what N / 8 calls of rt_render_pixels for that pixel alone
    give, 8 samples each at sample_base 0, 8, ...: one pixel for every N that occurs."""
    gpu, res = adaptive
    W, H = gpu.width, gpu.height
    acc = _host_layout(res)
    N = res["spp"].cpu().numpy()
    seen = 0
    for n in np.unique(N):
        y, x = np.argwhere(N == n)[len(np.argwhere(N == n)) // 2]
        own = None
        for k in range(int(n) // BATCH):
            out = gpu.render_pixels([y * W + x], BATCH, seed=SEED, sample_base=k * BATCH, moments=True,
                                    out=None if own is None else own)
            own = (out[0], out[1], out[2], out[4], out[5])
        assert all(_same_bits(a[x, y], b[x, y]) for a, b in zip(own, acc)), (n, x, y)
        seen += 1
    assert seen >= 3
