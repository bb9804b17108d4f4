"""The first bounce on the host: rt_debug_block_units' masks against the oracle and the kernels' own camera rays.

In the camera-ray iteration of a rounds ticket a wave of one 8x8 block tests only the test units of the
flat order whose bit is set in the block's mask (unit_masks, block_cull.cpp; trace_units,
rt_trace.h).  That is sound only if no camera ray of a block can meet a unit whose bit is clear.
For every live block and every such unit: the fp64 oracle's primary_ids over the block's pixels names
no primitive of the unit; and the rays of all four corners of every pixel and of seeded jittered
positions, formed in numpy float32 as camera_ray forms them, miss in fp64 the unit's own box, built here
from the primitives without the pad and grown by half the pad.  Not vacuous: from bounce.txt's camera 0
at 1080p more than half of the blocks that hit anything keep the room's unit alone.  Off, with masks of
all ones: a scene with a plane, a scene with more than 64 units, a camera inside the room.
"""
import numpy as np
import pytest

from test_block_cull_host import F32, _bounce, _camera_f32, _camera_rays, _fma, _frame_rows, _oracle_ids

ROOM = {6, 8, 9, 10}  # the faces of bounce.txt's room that its cameras see from outside


def _unit_boxes(rc, scene, ids):
    """Each unit's box over the primitives it stands for, in fp64, unpadded: vertices (a parallelogram's
    fourth too), a sphere's centre +- r, an ellipsoid's exact box (object -> world is MatrixToObject)."""
    out = []
    for unit in ids:
        lo, hi = np.full(3, np.inf), np.full(3, -np.inf)
        for i in unit:
            p = scene.prims[i]
            if p.kind == rc.RT_PRIM_TRIANGLE:
                v = np.array([[q.x, q.y, q.z] for q in p.p])
                if p.flags & rc.RT_FLAG_MIRROR:
                    v = np.concatenate([v, (v[1] + v[2] - v[0])[None]])
                a, b = v.min(0), v.max(0)
            else:
                assert p.kind == rc.RT_PRIM_SPHERE
                mid, half = np.array([p.p[0].x, p.p[0].y, p.p[0].z]), np.full(3, abs(p.radius))
                if p.flags & rc.RT_FLAG_TRANSFORMED:
                    m = np.array(p.to_obj).reshape(4, 4)
                    mid, half = m[:3, :3] @ mid + m[:3, 3], abs(p.radius) * np.sqrt((m[:3, :3] ** 2).sum(1))
                a, b = mid - half, mid + half
            lo, hi = np.minimum(lo, a), np.maximum(hi, b)
        out.append((lo, hi))
    return out


def _misses(lo, hi, o, d):
    """The exact ray against box test in fp64: True where the ray (t >= 0) does not meet [lo, hi]."""
    o, d = o.astype(np.float64), d.astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        t0, t1 = (lo - o) / d, (hi - o) / d
    flat = d == 0  # parallel to the slab: inside it for every t, or never
    inside = (o >= lo) & (o <= hi)
    near = np.where(flat, np.where(inside, -np.inf, np.inf), np.minimum(t0, t1))
    far = np.where(flat, np.where(inside, np.inf, -np.inf), np.maximum(t0, t1))
    return np.maximum(near.max(1), 0.0) > far.min(1)


def _sample_points(fx, fy, px, py, w, h, rows, seed, draws):
    """Per pixel of the list: its corner (x, y); the other three corners where no neighbour pixel of the
    same block has them as its own; `draws` seeded jittered positions, drawn as the kernel draws them.
    Returns sx, sy and the index of each point's pixel."""
    k = np.arange(len(fx))
    right = (px % 8 == 7) | (px == w - 1)
    below = rows[np.minimum(py + 1, h - 1)]
    bottom = (py % 8 == 7) | (py == h - 1) | (below != fy + 1)
    sx, sy, who = [fx], [fy], [k]
    for sel, dx, dy in ((right, 1, 0), (bottom, 0, 1), (right | bottom, 1, 1)):
        sx.append(fx[sel] + dx)
        sy.append(fy[sel] + dy)
        who.append(k[sel])
    r = np.random.default_rng(seed)
    for _ in range(draws):
        sx.append(_fma(r.integers(0, 1 << 24, len(fx)).astype(F32), F32(2.0 ** -24), fx.astype(F32)))
        sy.append(_fma(r.integers(0, 1 << 24, len(fy)).astype(F32), F32(2.0 ** -24), fy.astype(F32)))
        who.append(k)
    return np.concatenate(sx).astype(F32), np.concatenate(sy).astype(F32), np.concatenate(who)


SMALL, FULL = (256, 144), (1920, 1080)
CASES = [("cam%d_%dx%d" % (k, w, h), k, (w, h), None, None) for k in range(8) for (w, h) in (SMALL, FULL)]
CASES += [
    ("cam0_window", 0, SMALL, (3, 5, 203, 77), None),
    ("cam2_window", 2, SMALL, (16, 8, 100, 121), None),
    ("cam0_band8", 0, SMALL, None, (8, 2, 1)),
    ("cam0_band5", 0, SMALL, None, (5, 2, 1)),
    ("cam3_band5_window", 3, SMALL, (8, 0, 203, 60), (5, 2, 1)),
]


@pytest.mark.parametrize("case,cam,size,window,bands", CASES, ids=[c[0] for c in CASES])
def test_clear_units_cannot_be_met(rc, case, cam, size, window, bands):
    scene, _ = _bounce(rc)
    camera = scene.cameras[cam]
    W, H = size
    u = rc.block_units(scene.prims, camera, size, window, bands)
    dead, live = rc.block_cull(scene.prims, camera, size, window, bands)
    nu = u["n_units"]
    assert 0 < nu <= 64 and len(u["ids"]) == nu and np.array_equal(u["dead"], dead) and u["live"] == live
    assert sorted(i for unit in u["ids"] for i in set(unit)) == list(range(scene.n_prims))  # every primitive, once
    assert len(u["masks"]) == live
    full = np.uint64((1 << nu) - 1)
    if cam in (1, 5):  # inside the room: no block is dead, so no cull record and no masks
        assert not u["on"] and (u["masks"] == np.uint64(2 ** 64 - 1)).all()
        return
    assert u["on"] and (u["masks"] <= full).all() and (u["masks"] != 0).all() and (u["masks"] != full).any()
    rows_n = rc.load_library().rt_band_rows(H, *bands) if bands else H
    x0, y0, w, h = window or (0, 0, W, rows_n)
    rows = _frame_rows(h, y0, bands)
    # the mask of every block (0 for a dead one), then of every real pixel of the window
    block_mask = np.zeros(dead.shape, np.uint64)
    block_mask[~dead] = u["masks"]
    py, px = np.nonzero(np.kron((~dead).astype(np.uint8), np.ones((8, 8), np.uint8))[:h, :w])
    fx, fy = x0 + px, rows[py]
    pmask = block_mask[py // 8, px // 8]
    # (a) the oracle names no primitive of a unit whose bit is clear
    unit_of = np.full(scene.n_prims, -1)
    for k, unit in enumerate(u["ids"]):
        unit_of[list(unit)] = k
    ids = _oracle_ids(rc, scene, camera, size)[fx, fy]
    hit = ids >= 0
    seen = unit_of[ids[hit]]
    assert (seen >= 0).all() and hit.any()
    assert ((pmask[hit] >> seen.astype(np.uint64)) & np.uint64(1)).all(), "the oracle sees a unit whose bit is clear"
    # (b) the kernel's camera rays miss the box of every unit whose bit is clear
    sx, sy, who = _sample_points(fx, fy, px, py, w, h, rows, len(case), 1 if size == FULL else 4)
    o, d = _camera_rays(_camera_f32(camera, W, H), sx, sy)
    half_pad = 0.5 * u["pad"]
    assert half_pad > 0
    for k, (lo, hi) in enumerate(_unit_boxes(rc, scene, u["ids"])):
        # the reporter's padded box holds the unpadded one grown by the pad
        assert (u["box"][k, 0] <= lo - u["pad"] * 0.999).all() and (u["box"][k, 1] >= hi + u["pad"] * 0.999).all()
        sel = ((pmask[who] >> np.uint64(k)) & np.uint64(1)) == 0
        if sel.any():
            miss = _misses(lo - half_pad, hi + half_pad, o[sel], d[sel])
            assert miss.all(), (k, int((~miss).sum()), int(sel.sum()))


def test_most_blocks_keep_the_room_alone(rc):
    """bounce.txt camera 0 at 1080p: by the oracle 5,648 of the 7,613 blocks that hit anything see
    nothing but the room's faces; the margins take some, and more than half must remain."""
    scene, _ = _bounce(rc)
    u = rc.block_units(scene.prims, scene.cameras[0], FULL)
    room = [k for k, unit in enumerate(u["ids"]) if ROOM <= set(unit)]
    assert len(room) == 1 and u["on"]
    ids = _oracle_ids(rc, scene, scene.cameras[0], FULL)  # [x, y]
    hits = (ids >= 0).reshape(240, 8, 135, 8).any(axis=(1, 3)).T  # [block row, block column]
    assert int(hits.sum()) == 7613 and not (hits & u["dead"]).any()
    block_mask = np.zeros(u["dead"].shape, np.uint64)
    block_mask[~u["dead"]] = u["masks"]
    alone = (block_mask == np.uint64(1 << room[0])) & hits
    assert alone.sum() > 0.5 * hits.sum(), (int(alone.sum()), int(hits.sum()))


def test_off_cases(rc):
    scene, _ = _bounce(rc)
    all_ones = np.uint64(2 ** 64 - 1)
    text = open(rc.scene_path("bounce.txt")).read()
    with_plane = rc.SceneLoader.from_text(text + "\nplane 0 0 1 -9\n")
    u = rc.block_units(with_plane.prims, with_plane.cameras[0], SMALL)
    assert not u["on"] and u["live"] == u["dead"].size and (u["masks"] == all_ones).all()
    many = rc.SceneLoader.from_text(text + "".join("\nsphere %g 0.5 -0.5 0.01" % (-0.9 + 0.02 * k) for k in range(60)) + "\n")
    u = rc.block_units(many.prims, many.cameras[0], SMALL)
    assert u["n_units"] > 64 and not u["on"] and 0 < u["live"] < u["dead"].size and (u["masks"] == all_ones).all()
    u = rc.block_units(scene.prims, scene.cameras[1], SMALL)  # inside the room
    assert not u["on"] and u["live"] == u["dead"].size and (u["masks"] == all_ones).all()
    u = rc.block_units(scene.prims, scene.cameras[0], SMALL)  # and the camera it does serve
    assert u["on"] and u["n_units"] <= 64 and (u["masks"] != all_ones).all()
