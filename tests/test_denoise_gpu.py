"""Denoising on the device: rt_primary_hits_device against rt_query_rays over rt_camera_rays (G1),
rt_denoise_device against its host twin on synthetic inputs (G2) and on an adaptive render of bounce, where
it must also bring the image closer to a converged one (G3)."""
import numpy as np
import pytest

from denoise_cases import FRAMES, PARAMS, luminance, make_inputs, planes, run_host
from test_query_rays_gpu import _gpu, _same_bits

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5


def _hits_device(rc, gpu, x0=0, y0=0, w=None, h=None, stream=0):
    """primary_hits_device into a sentinel-filled tensor with 4 records to spare; returns (the tensor, the
    tile's hits as a HIT_DTYPE array [h, w])."""
    import torch

    w = gpu.width - x0 if w is None else w
    h = gpu.height - y0 if h is None else h
    buf = torch.full((w * h + 4, rc.HIT_DTYPE.itemsize), SENTINEL, dtype=torch.uint8, device="cuda")
    gpu.primary_hits_device(buf.data_ptr(), x0, y0, w, h, stream=stream)
    torch.cuda.synchronize()
    raw = buf.cpu().numpy()
    assert (raw[w * h:] == SENTINEL).all()
    return buf, raw[:w * h].reshape(-1).view(rc.HIT_DTYPE).reshape(h, w)


# ---------------------------------------------------------------- G1: the guide pass
@pytest.mark.parametrize("mode", ["AUTO", "GROUPED", "BVH"])
@pytest.mark.parametrize("name", ["bounce", "die"])
def test_g1_primary_hits_are_query_rays_of_camera_rays(rc, name, mode):
    """64 x 64, and a sub-tile with x0, y0 > 0: every record equals, bit for bit, what rt_query_rays answers
    for rt_camera_rays' ray of that pixel; nothing is written past the tile."""
    gpu = _gpu(rc, name, mode, size=(64, 64))
    for tile in ((0, 0, 64, 64), (5, 9, 37, 19)):
        want = gpu.query_rays(gpu.camera_rays(*tile))       # [x, y]
        got = _hits_device(rc, gpu, *tile)[1]               # [y, x]
        assert (want["prim_id"] >= 0).any() and _same_bits(got, want.T), tile
    gpu.close()


def test_g1_rows_in_chunks_and_errors(rc):
    """A frame of more than 2^19 pixels takes two chunks of rows; a BVH2 scene and a tile outside the frame
    are refused."""
    import torch

    gpu = _gpu(rc, "bounce", "AUTO", size=(1024, 600))
    want = gpu.query_rays(gpu.camera_rays())
    side = torch.cuda.Stream()
    got = _hits_device(rc, gpu, stream=side.cuda_stream)[1]
    assert _same_bits(got, want.T)
    buf = torch.zeros((16, 48), dtype=torch.uint8, device="cuda")
    with pytest.raises(rc.RtError, match="-1"):
        gpu.primary_hits_device(buf.data_ptr(), 1020, 0, 8, 2)
    with pytest.raises(rc.RtError, match="-1"):
        gpu.primary_hits_device(0, 0, 0, 4, 4)
    gpu.close()
    gpu = _gpu(rc, "bounce", "BVH2", size=(64, 64))
    with pytest.raises(rc.RtError, match="BVH2"):
        gpu.primary_hits_device(buf.data_ptr(), 0, 0, 4, 4)
    gpu.close()


# ---------------------------------------------------------------- G2: the device pass against the host twin
def _upload(acc, hits):
    import torch

    arrs = (acc["sum"], acc["samples"], acc["misses"], acc["q"], acc["batches"])
    dev = [torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda() for a in arrs]
    d_hits = torch.from_numpy(np.ascontiguousarray(hits).reshape(-1).view(np.uint8)).cuda()
    return dev, d_hits


@pytest.mark.parametrize("iterations", [1, 5])
@pytest.mark.parametrize("plane_pad", [0, 37])
@pytest.mark.parametrize("width,height", FRAMES)
def test_g2_device_equals_the_host_twin(rc, width, height, plane_pad, iterations):
    """The synthetic noisy frames of tests/test_denoise_host.py's H4 (invalid, NaN and single-batch pixels
    included): out_sum and out_var equal the twin's bit for bit, from a side stream, the default stream and
    the side stream again; the bytes between the planes and past the frame keep their sentinel."""
    import torch

    npix = width * height
    acc, hits, _, _ = make_inputs(rc, width, height, seed=width + height, plane=npix + plane_pad if plane_pad else 0)
    want, want_flat, want_var = run_host(rc, acc, hits, iterations=iterations)
    par = rc.denoise_params(**dict(PARAMS, iterations=iterations))
    dev, d_hits = _upload(acc, hits)
    pl = acc["plane"] or npix
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    outs = []
    for stream in (side.cuda_stream, 0, side.cuda_stream):
        out = torch.full((2 * pl + npix + 8,), -7.0, dtype=torch.float64, device="cuda")
        var = torch.full((npix + 8,), -7.0, dtype=torch.float32, device="cuda")
        rc.denoise_device(par, *[a.data_ptr() for a in dev], d_hits.data_ptr(), width, height, out.data_ptr(), var.data_ptr(),
                          plane=acc["plane"], stream=stream)
        outs.append((out, var))
    torch.cuda.synchronize()
    for out, var in outs:
        out, var = out.cpu().numpy(), var.cpu().numpy()
        assert _same_bits(planes(out, acc), want) and _same_bits(var[:npix].reshape(height, width), want_var)
        assert (var[npix:] == -7.0).all() and (out[2 * pl + npix:] == -7.0).all()
        for c in range(2):
            assert (out[c * pl + npix:(c + 1) * pl] == -7.0).all()
    # without the variance output
    out = torch.full((2 * pl + npix,), -7.0, dtype=torch.float64, device="cuda")
    rc.denoise_device(par, *[a.data_ptr() for a in dev], d_hits.data_ptr(), width, height, out.data_ptr(), 0, plane=acc["plane"])
    torch.cuda.synchronize()
    assert _same_bits(planes(out.cpu().numpy(), acc), want)


# ---------------------------------------------------------------- G3: real data
TOL, MIN_SPP, MAX_SPP, BATCH, SEED, REF_SPP = 0.3, 8, 64, 8, 11, 2048


def test_g3_an_adaptive_render_of_bounce(rc):
    """bounce 128 x 128, render_adaptive(0.3, 8, 64, 8), then GpuRaytracer.denoise: the device result equals
    the twin on the downloaded accumulators and hits bit for bit; against a 2048-spp render of the frame
    the luminance error over the pixels with samples > 0 is strictly below the unfiltered result's;
    rt_tonemap_device takes the output, and background-only pixels keep their ARGB codes."""
    import torch

    gpu = _gpu(rc, "bounce", "AUTO", size=(128, 128))
    W, H = gpu.width, gpu.height
    res = gpu.render_adaptive(TOL, MIN_SPP, MAX_SPP, BATCH, seed=SEED)
    out, var = gpu.denoise(res, return_var=True)
    assert out.shape == (3, H, W) and out.dtype == torch.float64 and var.shape == (H, W)
    hits = _hits_device(rc, gpu)[1]
    acc = {"sum": res["sum"].cpu().numpy().reshape(-1), "samples": res["samples"].cpu().numpy().reshape(-1).view(np.uint32),
           "misses": res["misses"].cpu().numpy().reshape(-1).view(np.uint32), "q": res["q"].cpu().numpy().reshape(-1),
           "batches": res["batches"].cpu().numpy().reshape(-1).view(np.uint32), "plane": 0, "width": W, "height": H}
    assert rc.denoise_iterations(W, H) == 2 and rc.denoise_iterations(1920, 1080) == 5
    want, _, want_var = run_host(rc, acc, hits, **dict(rc.DENOISE_DEFAULTS, iterations=rc.denoise_iterations(W, H)))
    got = out.cpu().numpy()
    assert _same_bits(got, want) and _same_bits(var.cpu().numpy(), want_var)
    # the converged image
    ref = torch.zeros((3, H, W), dtype=torch.float64, device="cuda")
    ref_n = torch.zeros((H, W), dtype=torch.int32, device="cuda")
    ref_m = torch.zeros((H, W), dtype=torch.int32, device="cuda")
    rays = torch.zeros(1, dtype=torch.int64, device="cuda")
    gpu.render_device(0, 0, W, H, REF_SPP, SEED + 1, 0, ref.data_ptr(), ref_n.data_ptr(), ref_m.data_ptr(), rays.data_ptr())
    torch.cuda.synchronize()
    ns = acc["samples"].reshape(H, W).astype(np.float64)
    rn = ref_n.cpu().numpy().astype(np.float64)
    mask = (ns > 0) & (rn > 0)
    assert mask.sum() > 1000 and (ns > 0).sum() - mask.sum() < 0.01 * mask.sum()
    truth = luminance(np.moveaxis(ref.cpu().numpy(), 0, -1) / np.maximum(rn, 1)[..., None])
    mse = {}
    for key, s in (("before", acc["sum"].reshape(3, H, W)), ("after", got)):
        d = luminance(np.moveaxis(s, 0, -1) / np.maximum(ns, 1)[..., None]) - truth
        mse[key] = float(np.mean(d[mask] ** 2))
    print(f"G3: luminance MSE against {REF_SPP} spp over {int(mask.sum())} pixels: {mse['before']:.5g} -> {mse['after']:.5g}, "
          f"ratio {mse['after'] / mse['before']:.4f}")
    assert mse["after"] < mse["before"]
    # tone mapping takes the output as it takes the sums
    argb = [torch.zeros((H, W), dtype=torch.int32, device="cuda") for _ in range(2)]
    for s, a in zip((res["sum"], out), argb):
        rc.tonemap_device(s.data_ptr(), res["samples"].data_ptr(), res["misses"].data_ptr(), W, H, a.data_ptr(),
                          background=(0.1, 0.2, 0.3), background_alpha=1.0)
    torch.cuda.synchronize()
    a0, a1 = (a.cpu().numpy() for a in argb)
    background = ns == 0
    assert background.any() and np.array_equal(a0[background], a1[background])
    assert not np.array_equal(a0[mask], a1[mask])
    gpu.close()
