"""The order in which the path kernels' dispensers deal a launch's work items.

A work item is ((block << log2(n_chunks)) + chunk) * 64 + pixel of the 8x8 block; a pixel's real
chunks are the first `used` = ceil(spp / chunk) of the n_chunks (a power of two) chunk slots, the last
of them short when chunk does not divide spp.  A dispenser counts tickets; ticket_items (rt_kernels.h)
turns a ticket into its items, in the kernels' refill and, through rt_debug_item_order, here.

CPU: over a grid of small launches the tickets cover every real item once and no empty slot, each is
adjacent chunks of one block, and a range deals its short chunks last.  GPU: a render is bit for bit
what RTCORE_ITEM_ORDER=0 (every slot dealt in index order) renders, and what the brute-force kernels
render without their batched item opening (RTCORE_ITEM_BATCH=0).
"""
import numpy as np
import pytest

FRAMES = [(8, 8), (24, 24), (70, 45), (64, 64)]  # 1 block; 9 blocks, one range; ragged blocks; 64 blocks, 8 ranges
# (spp, chunks per pixel asked) -> samples per item, real chunks, samples of the last chunk
SHAPES = {
    "used1": (5, 1),             # 5, 1, 5: one slot, nothing to skip
    "used2_short": (7, 2),       # 4, 2, 3
    "used3": (9, 3),             # 3, 3, 3: 4 slots, one empty
    "used3_short": (10, 3),      # 4, 3, 2
    "used24_short": (256, 24),   # 11, 24, 3: the flagship launch's shape
    "pow2_full": (32, 8),        # 4, 8, 4: nothing to skip
    "last_of_1": (25, 8),        # 4, 7, 1
    "tuned": (130, 0),           # the tuned chunk count of a small frame: 1, 130, 1 of 256 slots
}
BANDS = (8, 2, 1)


def _launch(rc, frame, bands):
    """(w, rows of the launch, 8x8 blocks)"""
    w, h = frame
    rows = rc.band_rows_count(h, *bands) if bands else h
    return w, rows, ((w + 7) // 8) * ((rows + 7) // 8)


def _check_order(rc, frame, spp, chunks, pool, bands):
    w, rows, n_blocks = _launch(rc, frame, bands)
    t, info = rc.item_order(frame[0], frame[1], spp, chunks, pool, bands)
    if rows == 0:
        assert len(t) == 0
        return None
    n_chunks, chunk, n_split = info["n_chunks"], info["chunk"], info["n_split"]
    used = -(-spp // chunk)
    short = spp % chunk != 0
    assert n_chunks & (n_chunks - 1) == 0 and n_chunks // 2 < used <= n_chunks
    assert info["pool"] == min(pool, 64 * n_chunks)
    assert n_split == (8 if n_blocks >= 32 else 1)
    g, first, length = (t[:, k].astype(np.int64) for k in range(3))
    assert np.all(first % 64 == 0) and np.all(length % 64 == 0)
    assert np.all(length >= 64) and np.all(length <= info["pool"])
    slot0, n_slots = first // 64, length // 64
    blk, c0 = slot0 // n_chunks, slot0 % n_chunks
    # adjacent chunks of one block, none of them an empty slot
    assert np.all(c0 + n_slots <= used)
    # each ticket within its range's blocks
    lo = np.array([n_blocks * k // n_split for k in range(n_split + 1)])
    assert np.all(g < n_split) and np.all(blk >= lo[g]) and np.all(blk < lo[g + 1])
    assert np.all(np.diff(g) >= 0)  # range by range
    # every real chunk of every block exactly once, no other
    seen = np.zeros((n_blocks, n_chunks), np.int64)
    for k in range(int(n_slots.max())):
        sel = n_slots > k
        np.add.at(seen, (blk[sel], c0[sel] + k), 1)
    assert np.all(seen[:, :used] == 1) and np.all(seen[:, used:] == 0)
    # within a range the tickets that hold a short chunk come last (at 64 items per ticket: no
    # full-length chunk after a short one); a full-length ticket is a whole pool
    has_short = (c0 + n_slots == used) & short
    for k in range(n_split):
        hs = has_short[g == k]
        assert np.all(np.diff(hs.astype(np.int64)) >= 0), (k, hs)
    assert np.all(length[~has_short & (c0 + n_slots < used)] == info["pool"])
    if short:
        assert has_short.sum() == n_blocks
    return t, used, short, n_chunks


@pytest.mark.parametrize("bands", [None, BANDS], ids=["tile", "bands"])
@pytest.mark.parametrize("pool", [64, 128])
@pytest.mark.parametrize("shape", sorted(SHAPES))
@pytest.mark.parametrize("frame", FRAMES, ids=lambda f: f"{f[0]}x{f[1]}")
def test_tickets_cover_real_items_once_short_chunks_last(rc, frame, shape, pool, bands, monkeypatch):
    monkeypatch.delenv("RTCORE_ITEM_ORDER", raising=False)
    monkeypatch.delenv("RTCORE_PATH_CHUNKS", raising=False)
    monkeypatch.delenv("RTCORE_POOL_MUL", raising=False)
    monkeypatch.delenv("RTCORE_XCD_SPLIT", raising=False)
    spp, chunks = SHAPES[shape]
    got = _check_order(rc, frame, spp, chunks, pool, bands)
    if got is None:
        return
    t, used, short, n_chunks = got
    monkeypatch.setenv("RTCORE_ITEM_ORDER", "0")
    t0, info0 = rc.item_order(frame[0], frame[1], spp, chunks, pool, bands)
    # the earlier order: every slot, pool items per ticket, in index order within a range
    assert np.all(t0[:, 2] == info0["pool"])
    w, rows, n_blocks = _launch(rc, frame, bands)
    assert np.array_equal(np.sort(t0[:, 1].astype(np.int64)),
                          np.arange(0, n_blocks * n_chunks * 64, info0["pool"]))
    for k in range(info0["n_split"]):
        assert np.all(np.diff(t0[t0[:, 0] == k, 1].astype(np.int64)) == info0["pool"])
    if used == n_chunks and not short:  # nothing to skip: the same sequence
        assert np.array_equal(t, t0)
    elif used <= n_chunks - info0["pool"] // 64:  # at least a ticket's worth of empty slots per block
        assert len(t) < len(t0)


def test_flagship_launch_shape(rc, monkeypatch):
    """bench.py's step (1920 x 1080 x 256 spp as the band set (8, 1, 0)): 24 real chunks of 32 slots,
    so a quarter fewer tickets than slots, and the last 4,050 tickets of each range are the
    3-sample chunks."""
    for v in ("RTCORE_ITEM_ORDER", "RTCORE_PATH_CHUNKS", "RTCORE_POOL_MUL", "RTCORE_XCD_SPLIT"):
        monkeypatch.delenv(v, raising=False)
    t, info = rc.item_order(1920, 1080, 256, bands=(8, 1, 0))
    assert info == {"n_chunks": 32, "chunk": 11, "pool": 64, "n_split": 8}
    n_blocks = 240 * 135
    assert len(t) == n_blocks * 24
    chunk = (t[:, 1].astype(np.int64) // 64) % 32
    for k in range(8):
        c = chunk[t[:, 0] == k]
        assert len(c) == 4050 * 24 and np.all(c[-4050:] == 23) and np.all(c[:-4050] < 23)


# ---- GPU: which wave takes an item never changes what the item computes ----

def _both_orders(monkeypatch, render):
    monkeypatch.setenv("RTCORE_ITEM_ORDER", "0")
    a = render()
    monkeypatch.delenv("RTCORE_ITEM_ORDER")
    b = render()
    return a, b


def _same(a, b):
    for x, y in zip(a, b):
        assert np.array_equal(np.asarray(x), np.asarray(y))


@pytest.mark.gpu
@pytest.mark.parametrize("size,spp", [((64, 64), 201), ((70, 45), 37)])
def test_flat_renders_identically(rc, scenes, size, spp, monkeypatch):
    g = rc.GpuRaytracer(scenes["bounce.txt"], 0, size=size, traversal=rc.RT_TRAVERSAL_BRUTE)
    a, b = _both_orders(monkeypatch, lambda: g.render_tile(0, 0, *size, spp, seed=3))
    g.close()
    assert np.all(a[1] + a[2] == spp) and a[3] > 0
    _same(a, b)


@pytest.mark.gpu
def test_grouped_renders_identically(rc, scenes, monkeypatch):
    g = rc.GpuRaytracer(scenes["die.txt"], 0, size=(64, 64), traversal=rc.RT_TRAVERSAL_GROUPED)
    a, b = _both_orders(monkeypatch, lambda: g.render_tile(0, 0, 64, 64, 130, seed=3))
    g.close()
    assert np.all(a[1] + a[2] == 130) and a[3] > 0
    _same(a, b)


@pytest.mark.gpu
@pytest.mark.parametrize("name,mode,size,spp", [("bounce.txt", "BRUTE", (70, 45), 37), ("bounce.txt", "BRUTE", (64, 64), 201),
                                                ("die.txt", "GROUPED", (64, 64), 130)])
def test_batched_item_opening_renders_identically(rc, scenes, name, mode, size, spp, monkeypatch):
    """The brute-force kernels' waves draw their next ticket only when all 64 lanes wait for an item
    (RTCORE_ITEM_BATCH, default 64): bit for bit the render of waves that draw as soon as one lane
    does (0), and of a threshold in between."""
    g = rc.GpuRaytracer(scenes[name], 0, size=size, traversal=getattr(rc, "RT_TRAVERSAL_" + mode))
    got = []
    for batch in ("0", "24", None):
        if batch is None:
            monkeypatch.delenv("RTCORE_ITEM_BATCH")
        else:
            monkeypatch.setenv("RTCORE_ITEM_BATCH", batch)
        got.append(g.render_tile(0, 0, *size, spp, seed=5))
    g.close()
    assert np.all(got[0][1] + got[0][2] == spp) and got[0][3] > 0
    _same(got[0], got[1])
    _same(got[0], got[2])


@pytest.mark.gpu
def test_bvh_renders_identically(rc, scenes, monkeypatch):
    monkeypatch.setenv("RTCORE_PATH_CHUNKS", "24")  # 50 spp: 17 chunks of 3 samples, the last of 2
    g = rc.GpuRaytracer(scenes["bounce.txt"], 0, size=(64, 64), traversal=rc.RT_TRAVERSAL_BVH)
    a, b = _both_orders(monkeypatch, lambda: g.render_tile(0, 0, 64, 64, 50, seed=3))
    g.close()
    assert np.all(a[1] + a[2] == 50) and a[3] > 0
    _same(a, b)


@pytest.mark.gpu
def test_band_set_renders_identically(rc, scenes, monkeypatch):
    import torch

    W = H = 64
    band, stride = 8, 2
    g = rc.GpuRaytracer(scenes["bounce.txt"], 0, size=(W, H), traversal=rc.RT_TRAVERSAL_BRUTE)
    plane = rc.band_slot_rows(H, band, stride) * W

    def render():
        d_sum = torch.zeros(3 * plane, dtype=torch.float64, device="cuda")
        d_n = torch.zeros(plane, dtype=torch.int32, device="cuda")
        d_m = torch.zeros(plane, dtype=torch.int32, device="cuda")
        d_rays = torch.zeros(1, dtype=torch.int64, device="cuda")
        stream = torch.cuda.current_stream().cuda_stream
        g.render_bands_device(band, stride, 1, 100, 3, 0, d_sum.data_ptr(), d_n.data_ptr(), d_m.data_ptr(), plane,
                              d_rays.data_ptr(), stream)
        torch.cuda.synchronize()
        return d_sum.cpu().numpy(), d_n.cpu().numpy(), d_m.cpu().numpy(), d_rays.cpu().numpy()

    a, b = _both_orders(monkeypatch, render)
    g.close()
    rows = rc.band_rows_count(H, band, stride, 1)
    assert np.all((a[1] + a[2])[:rows * W] == 100) and a[3][0] > 0
    _same(a, b)


@pytest.mark.gpu
def test_1spp_pass_renders_identically(rc, scenes, monkeypatch):
    g = rc.GpuRaytracer(scenes["bounce.txt"], 0, size=(70, 45))
    a, b = _both_orders(monkeypatch, lambda: g.render_tile_1spp(0, 0, 70, 45, seed=3, sample_index=5))
    g.close()
    assert np.array_equal(a, b)
