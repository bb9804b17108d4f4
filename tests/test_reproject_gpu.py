"""Temporal reprojection on the device: rt_reproject_device against its host twin on the inputs of
tests/test_reproject_host.py (G1), on real first hits and accumulators of bounce and die for the identity
and a whole-pixel ortho shift (G2), and inside the adaptive loop, where continuing from the carried
accumulators must cost fewer rays than starting again without costing accuracy (G3)."""
import numpy as np
import pytest

from reproject_cases import (FRAMES, KEYS, LOOSE, ORTHO, PADS, camera, change, gathered, h3_inputs, h5_inputs, init_render,
                             luminance3, planes, run_host, same, vec)
from test_query_rays_gpu import _gpu

pytestmark = pytest.mark.gpu

def _dev(a):
    import torch

    a = np.array(a)  # (a writable copy: the cached hits are read-only)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    elif a.dtype.fields is not None:
        a = a.reshape(-1).view(np.uint8)
    return torch.from_numpy(a).cuda()


def _run_device(rc, par, prev_cam, d_prev, d_hits, d_acc, acc, stream=0, with_src=True):
    """rt_reproject_device into sentinel-filled tensors with 8 elements to spare each; returns them."""
    import torch

    W, H = acc["width"], acc["height"]
    npix = W * H
    pl = acc["plane"] or npix
    out = {"sum": torch.full((2 * pl + npix + 8,), -7.0, dtype=torch.float64, device="cuda"),
           "q": torch.full((npix + 8,), -7.0, dtype=torch.float64, device="cuda")}
    for k in ("samples", "misses", "batches", "src"):
        out[k] = torch.full((npix + 8,), 7, dtype=torch.int32, device="cuda")
    rc.reproject_device(par, prev_cam, d_prev.data_ptr(), d_hits.data_ptr(), *[d_acc[k].data_ptr() for k in KEYS], W, H,
                        *[out[k].data_ptr() for k in KEYS], out["src"].data_ptr() if with_src else 0, plane=acc["plane"],
                        stream=stream)
    return out


def _check_device(out, want, acc, with_src=True):
    """The device's outputs equal the twin's (run_host's result) bit for bit; the sentinels stand."""
    npix = acc["width"] * acc["height"]
    pl = acc["plane"] or npix
    got = {k: v.cpu().numpy() for k, v in out.items()}
    assert same(planes(got["sum"], acc), want["sum"])
    assert (got["sum"][2 * pl + npix:] == -7.0).all()
    for c in range(2):
        assert (got["sum"][c * pl + npix:(c + 1) * pl] == -7.0).all()
    assert same(got["q"][:npix], want["q"]) and (got["q"][npix:] == -7.0).all()
    for k in ("samples", "misses", "batches"):
        assert np.array_equal(got[k][:npix].view(np.uint32), want[k]) and (got[k][npix:] == 7).all(), k
    if with_src:
        assert np.array_equal(got["src"][:npix], want["src"]) and (got["src"][npix:] == 7).all()
    else:
        assert (got["src"] == 7).all()


# ---------------------------------------------------------------- G1: the device pass against the host twin
@pytest.mark.parametrize("inputs", ["h3", "h5"])
@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("width,height", FRAMES)
def test_g1_device_equals_the_host_twin(rc, width, height, pad, inputs):
    """The H3 (frustum move, copies and capped pixels) and H5 (the cap's corner cases) inputs: all six
    outputs equal the twin's bit for bit from a side stream, the default stream and the side stream again;
    the elements between the planes and past the frame keep their sentinel; once without out_src."""
    import torch

    I = (h3_inputs if inputs == "h3" else h5_inputs)(rc, width, height, pad)
    acc = I["acc"]
    want = run_host(rc, acc, I["prev_cam"], I["prev_hits"], I["hits"], **I["params"])
    assert (want["src"] >= 0).any() and (want["src"] < 0).any()
    par = rc.reproject_params(**I["params"])
    d_acc = {k: _dev(acc[k]) for k in KEYS}
    d_prev, d_hits = _dev(I["prev_hits"]), _dev(I["hits"])
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    outs = [_run_device(rc, par, I["prev_cam"], d_prev, d_hits, d_acc, acc, stream=s) for s in (side.cuda_stream, 0, side.cuda_stream)]
    outs.append(_run_device(rc, par, I["prev_cam"], d_prev, d_hits, d_acc, acc, with_src=False))
    torch.cuda.synchronize()
    for i, out in enumerate(outs):
        _check_device(out, want, acc, with_src=i < 3)


# ---------------------------------------------------------------- G2: real hits, identity and shift
def _render_8spp(gpu, seed=3):
    """One 8-spp rt_render_pixels_device pass with moments over every pixel; the accumulators as torch
    tensors in render_adaptive's layout."""
    import torch

    W, H = gpu.width, gpu.height
    acc = {"sum": torch.zeros((3, H, W), dtype=torch.float64, device="cuda"),
           "samples": torch.zeros((H, W), dtype=torch.int32, device="cuda"),
           "misses": torch.zeros((H, W), dtype=torch.int32, device="cuda"),
           "q": torch.zeros((H, W), dtype=torch.float64, device="cuda"),
           "batches": torch.zeros((H, W), dtype=torch.int32, device="cuda")}
    lst = torch.arange(W * H, dtype=torch.int32, device="cuda")
    gpu.render_pixels_device(lst.data_ptr(), W * H, 8, seed, 0, *[acc[k].data_ptr() for k in KEYS], 0, 0, 0)
    torch.cuda.synchronize()
    return acc


def _host_acc(res, W, H):
    return {"sum": res["sum"].cpu().numpy().reshape(-1), "samples": res["samples"].cpu().numpy().reshape(-1).view(np.uint32),
            "misses": res["misses"].cpu().numpy().reshape(-1).view(np.uint32), "q": res["q"].cpu().numpy().reshape(-1),
            "batches": res["batches"].cpu().numpy().reshape(-1).view(np.uint32), "plane": 0, "width": W, "height": H}


def _host_hits(rc, t, W, H):
    return t.cpu().numpy().reshape(-1).view(rc.HIT_DTYPE).reshape(H, W)


def _equals_twin(rc, got, acc, prev_cam, prev_hits, hits, **params):
    """GpuRaytracer.reproject's result against the twin on the downloaded arrays; returns the twin's."""
    want = run_host(rc, acc, prev_cam, prev_hits, hits, **params)
    npix = acc["width"] * acc["height"]
    assert same(got["sum"].cpu().numpy().reshape(3, npix), want["sum"]) and same(got["q"].cpu().numpy().reshape(-1), want["q"])
    for k in ("samples", "misses", "batches"):
        assert np.array_equal(got[k].cpu().numpy().reshape(-1).view(np.uint32), want[k]), k
    assert np.array_equal(got["src"].cpu().numpy().reshape(-1), want["src"])
    return want


@pytest.mark.parametrize("mode", ["AUTO", "GROUPED", "BVH"])
@pytest.mark.parametrize("name", ["bounce", "die"])
def test_g2_identity_on_real_hits(rc, name, mode):
    """64 x 64, hits from rt_primary_hits_device, accumulators from one 8-spp pass with moments.  The
    previous camera is the current one: every pixel with a hit and a usable normal maps to itself and keeps
    its accumulators bit for bit, every other pixel is empty, and the device equals the twin."""
    gpu = _gpu(rc, name, mode, size=(64, 64))
    W, H = gpu.width, gpu.height
    res = _render_8spp(gpu)
    hits = gpu.primary_hits()
    got = gpu.reproject(res, gpu.camera, hits, hits, max_history=LOOSE["max_history"])
    assert got["hits"] is hits and got["src"].shape == (H, W)
    acc, hh = _host_acc(res, W, H), _host_hits(rc, hits, W, H)
    want = _equals_twin(rc, got, acc, gpu.camera, hh, hh)
    flat = hh.reshape(-1)
    usable = (flat["prim_id"] >= 0) & np.isfinite(flat["normal"]).all(-1)
    assert usable.sum() >= 0.2 * usable.size and ((flat["prim_id"] >= 0) & ~usable).sum() <= 0.02 * usable.size
    assert ((acc["samples"].astype(np.int64) + acc["misses"]) == 8).all()
    p = np.arange(W * H)
    assert np.array_equal(want["src"][usable], p[usable]) and (want["src"][~usable] == -1).all()
    g = gathered(acc, p[usable])
    assert same(want["sum"][:, usable], g["sum"]) and all(same(want[k][usable], g[k]) for k in KEYS[1:])
    assert not want["sum"][:, ~usable].any() and not any(want[k][~usable].any() for k in KEYS[1:])
    gpu.close()


@pytest.mark.parametrize("mode", ["AUTO", "GROUPED", "BVH"])
def test_g2_ortho_shift_on_real_hits(rc, mode):
    """An ortho camera of the test's own on bounce (its first camera's position and orientation, size 2.5),
    moved 3 pixels along `side`: every accepted pixel's source is (x + 3, y) exactly and its accumulators are
    the source's bit for bit; of the pixels whose shifted source is in the frame and shows the same prim_id
    in both hit arrays at most 1 % are rejected (none would be in exact arithmetic: the margin is for fp32
    hit positions at grazing angles); the device equals the twin."""
    k = 3
    gpu = _gpu(rc, "bounce", mode, size=(64, 64))
    W, H = gpu.width, gpu.height
    c0 = camera(rc, "bounce", kind=ORTHO, size_mult=2.5)
    st = init_render(c0, W, H)
    step = k * st["h_mult"] * st["side"]
    c1 = change(rc, c0, position=vec(c0.position) + step, look_at=vec(c0.look_at) + step)
    gpu.set_camera(c0)
    res = _render_8spp(gpu)
    prev_hits = gpu.primary_hits()
    gpu.set_camera(c1)
    got = gpu.reproject(res, c0, prev_hits, max_history=LOOSE["max_history"])
    acc = _host_acc(res, W, H)
    ph, ch = _host_hits(rc, prev_hits, W, H), _host_hits(rc, got["hits"], W, H)
    want = _equals_twin(rc, got, acc, c0, ph, ch)
    src = want["src"]
    ok = src >= 0
    y, x = np.divmod(np.arange(W * H), W)
    assert np.array_equal(src[ok], (y * W + x + k)[ok]) and (x[ok] + k < W).all()
    g = gathered(acc, src[ok])
    assert same(want["sum"][:, ok], g["sum"]) and all(same(want[key][ok], g[key]) for key in KEYS[1:])
    shifted = np.full((H, W), -2, np.int32)
    shifted[:, :W - k] = ph["prim_id"][:, k:]
    eligible = ((ch["prim_id"] >= 0) & (shifted == ch["prim_id"])).reshape(-1)
    rejected = (eligible & ~ok).sum() / eligible.sum()
    print(f"G2 ortho shift {mode}: {eligible.sum()} eligible pixels, {100 * rejected:.3f} % rejected, {ok.sum()} accepted")
    assert eligible.sum() >= 0.2 * W * H and rejected <= 0.01
    gpu.close()


# ---------------------------------------------------------------- G3: the loop
TOL, MIN_SPP, MAX_SPP, BATCH, REF_SPP = 0.3, 8, 64, 8, 2048
# continued / from-scratch luminance MSE over the accepted pixels against 2048 spp, seeds 11, 12, 13, as
# measured on an MI355X (profiles/reproject/README.md); the assertion leaves 1.5 times the largest for the
# run-to-run room of a 128 x 128 estimate
MEASURED_RATIOS = (0.9712, 1.0481, 1.1784)


def _old_render_adaptive(rc, gpu, seed):
    """render_adaptive as it was before it took `history` and `sample_base`, from the library's passes."""
    import torch

    par = rc.rt_adaptive_params(TOL, 1e-3, MIN_SPP, MAX_SPP)
    W, H = gpu.width, gpu.height
    acc = {"sum": torch.zeros((3, H, W), dtype=torch.float64, device="cuda"),
           "samples": torch.zeros((H, W), dtype=torch.int32, device="cuda"),
           "misses": torch.zeros((H, W), dtype=torch.int32, device="cuda"),
           "q": torch.zeros((H, W), dtype=torch.float64, device="cuda"),
           "batches": torch.zeros((H, W), dtype=torch.int32, device="cuda")}
    d_count = torch.zeros(1, dtype=torch.int32, device="cuda")
    d_rays = torch.zeros(1, dtype=torch.int64, device="cuda")
    counts = []
    while True:
        lst = torch.empty(W * H if not counts else counts[-1], dtype=torch.int32, device="cuda")
        rc.adaptive_select_device(par, *[acc[k].data_ptr() for k in KEYS], W, H, lst.data_ptr(), lst.numel(), d_count.data_ptr())
        n = int(d_count.item()) & 0xFFFFFFFF
        if n == 0:
            break
        gpu.render_pixels_device(lst.data_ptr(), n, BATCH, seed, len(counts) * BATCH, *[acc[k].data_ptr() for k in KEYS], 0,
                                 d_rays.data_ptr(), 0)
        torch.cuda.synchronize()
        counts.append(n)
    acc.update(counts=counts, rays=int(d_rays.item()))
    return acc


def _same_result(a, b):
    return (all(same(a[k].cpu().numpy(), b[k].cpu().numpy()) for k in KEYS) and a["counts"] == b["counts"] and
            a["rays"] == b["rays"])


def _moved(rc, gpu, cam0):
    """cam0 moved 2 % of its distance to look_at along `side`."""
    st = init_render(cam0, gpu.width, gpu.height)
    step = 0.02 * np.linalg.norm(vec(cam0.look_at) - vec(cam0.position)) * st["side"]
    return change(rc, cam0, position=vec(cam0.position) + step, look_at=vec(cam0.look_at) + step)


def _frame_pair(rc, gpu, cam0, cam1, seed):
    """Render at cam0, move to cam1, reproject with the defaults, continue -- and render cam1 from scratch."""
    gpu.set_camera(cam0)
    first = gpu.render_adaptive(TOL, MIN_SPP, MAX_SPP, BATCH, seed=seed)
    prev_hits = gpu.primary_hits()
    gpu.set_camera(cam1)
    h = gpu.reproject(first, cam0, prev_hits)
    cont = gpu.render_adaptive(TOL, MIN_SPP, MAX_SPP, BATCH, seed=seed, history=h, sample_base=MAX_SPP)
    scratch = gpu.render_adaptive(TOL, MIN_SPP, MAX_SPP, BATCH, seed=seed)
    return first, prev_hits, h, cont, scratch


def _mse(res, truth, mask):
    ns = res["samples"].cpu().numpy().astype(np.float64)
    d = luminance3(res["sum"].cpu().numpy() / np.maximum(ns, 1)) - truth
    return float(np.mean(d[mask] ** 2))


def test_g3_the_loop_continues_from_the_history(rc):
    """bounce 128 x 128: render_adaptive(0.3, 8, 64, 8, seed=11) at camera 0, the camera moved 2 % of its
    distance to look_at along `side`, reproject with the defaults, render_adaptive(..., history=h,
    sample_base=64).  The reprojection equals the twin bit for bit; more than half of the pixels that can
    carry a history at all are accepted -- those with a first hit under the new camera: 59 % of this frame
    is background, which the pass leaves to start again by definition, so a share of the whole frame
    could not reach one half whatever the pass did (40.5 % of the frame has a hit, 98.5 % of it is accepted);
    the continued render traces strictly fewer rays than the same call from scratch; no pixel ends below
    min_spp; the history's tensors are untouched; render_adaptive without the new arguments returns what
    the loop it replaced returns, bit for bit; denoise with the carried hits equals denoise without.
    Luminance MSE over the accepted pixels against a 2048-spp render of the new view, continued over
    from scratch, seeds 11, 12, 13: each ratio stays below 1.5 times the largest measured one."""
    import torch

    gpu = _gpu(rc, "bounce", "AUTO", size=(128, 128))
    W, H = gpu.width, gpu.height
    cam0 = rc.rt_camera.from_buffer_copy(gpu.camera)
    cam1 = _moved(rc, gpu, cam0)
    first, prev_hits, h, cont, scratch = _frame_pair(rc, gpu, cam0, cam1, 11)
    # the device reprojection equals the twin's
    want = _equals_twin(rc, h, _host_acc(first, W, H), cam0, _host_hits(rc, prev_hits, W, H), _host_hits(rc, h["hits"], W, H),
                        **rc.REPROJECT_DEFAULTS)
    accepted = (want["src"] >= 0).reshape(H, W)
    with_hit = _host_hits(rc, h["hits"], W, H)["prim_id"] >= 0
    share = accepted.sum() / with_hit.sum()
    print(f"G3: accepted share {share:.4f} of the {with_hit.mean():.4f} of the frame with a first hit ({accepted.mean():.4f} of the "
          f"frame); rays continued {cont['rays']}, from scratch {scratch['rays']}; "
          f"lists continued {cont['counts']}, from scratch {scratch['counts']}")
    assert not (accepted & ~with_hit).any() and share > 0.5
    assert cont["rays"] < scratch["rays"]
    assert int(cont["spp"].min()) >= MIN_SPP and int(scratch["spp"].min()) >= MIN_SPP
    # the history was cloned
    assert all(same(h[k].cpu().numpy().reshape(-1), want[k].reshape(-1)) for k in KEYS)
    # without the new arguments: the loop as it was, and the defaults named
    old = _old_render_adaptive(rc, gpu, 11)
    assert _same_result(scratch, old)
    assert _same_result(gpu.render_adaptive(TOL, MIN_SPP, MAX_SPP, BATCH, seed=11, history=None, sample_base=0), old)
    # one guide pass per frame
    a, av = gpu.denoise(cont, return_var=True)
    b, bv = gpu.denoise(cont, return_var=True, hits=h["hits"])
    assert same(a.cpu().numpy(), b.cpu().numpy()) and same(av.cpu().numpy(), bv.cpu().numpy())
    # the error against a converged render of the new view
    ref = torch.zeros((3, H, W), dtype=torch.float64, device="cuda")
    ref_n = torch.zeros((H, W), dtype=torch.int32, device="cuda")
    ref_m = torch.zeros((H, W), dtype=torch.int32, device="cuda")
    rays = torch.zeros(1, dtype=torch.int64, device="cuda")
    gpu.render_device(0, 0, W, H, REF_SPP, 99, 0, ref.data_ptr(), ref_n.data_ptr(), ref_m.data_ptr(), rays.data_ptr())
    torch.cuda.synchronize()
    rn = ref_n.cpu().numpy().astype(np.float64)
    truth = luminance3(ref.cpu().numpy() / np.maximum(rn, 1))
    ratios = []
    for seed in (11, 12, 13):
        if seed != 11:
            first, prev_hits, h, cont, scratch = _frame_pair(rc, gpu, cam0, cam1, seed)
        mask = ((h["src"].cpu().numpy() >= 0) & (rn > 0) & (cont["samples"].cpu().numpy() > 0) &
                (scratch["samples"].cpu().numpy() > 0))
        assert mask.sum() > 0.25 * W * H
        mc, ms = _mse(cont, truth, mask), _mse(scratch, truth, mask)
        ratios.append(mc / ms)
        print(f"G3 seed {seed}: luminance MSE over {int(mask.sum())} accepted pixels against {REF_SPP} spp: continued {mc:.5g}, "
              f"from scratch {ms:.5g}, ratio {mc / ms:.4f}; rays {cont['rays']} / {scratch['rays']}")
    assert max(ratios) < 1.5 * max(MEASURED_RATIOS), ratios
    gpu.close()
