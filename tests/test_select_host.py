"""The selection pass, host side (no GPU): the layout of rt_select_item and rt_selection in C, ctypes and
numpy, and rt_debug_select_rays -- the pass's fold and per-item functions compiled for the CPU -- against
expectations that come from the reference side only:

* a primitive item's value is the distance the oracle's Scene.RayTrace gives in a scene of that one
  primitive (NaN on a miss);
* a node item's value is a NumPy fp64 restatement of AABB.IntersectAVX (written here from the reference's
  AABB.cs:107-142) on the oracle's own box of that node, near when near >= 0, else far;
* a list's answer is the fold of those values with `<=`, in list order.

The one-primitive oracle scene tests its lone leaf's box before the primitive, PrimitiveIntersector does
not: a (ray, item) pair the oracle misses and the library hits is left out only when the restated box
test reports a miss for it, and at most 1 pair in 1000 per case (the count is printed).

The cases and helpers here are shared with tests/test_select_gpu.py.
"""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

from oracle.oracle import OracleScene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRAME = (32, 24)
PRIM, NODE = 0, 1

# what bounce.txt and die.txt lack, appended to BOX_SCENE of tests/test_gpu_parity.py (one-sided,
# inverted, rotated and scaled cubes, a plane): a sphere under a non-uniform scale (RT_FLAG_TRANSFORMED)
# and a two-sided plain sphere
EXTRA_TAIL = """invert false
twosided false
pushtransform
translate 0 -2 2
scale 1 .7 1.3
sphere 0 0 0 .6
poptransform
twosided true
sphere 1.2 -2.5 .6 .5
"""
ORTHO_CAMERA = "orthographic 0 -6 1.5 0 0 0 0 0 1 4\n"


def extra_scene_text(ortho=False):
    from test_gpu_parity import BOX_SCENE

    text = BOX_SCENE + EXTRA_TAIL
    if ortho:
        lines = text.split("\n")
        assert lines[1].startswith("camera ")
        lines[1] = ORTHO_CAMERA.strip()
        text = "\n".join(lines)
    return text


@functools.lru_cache(maxsize=None)
def load_scene(name):
    import raytracercore_amd as rc

    if name in ("bounce", "die"):
        return rc.SceneLoader.from_file(rc.scene_path(name + ".txt"))
    return rc.SceneLoader.from_text(extra_scene_text(ortho=(name == "extra_ortho")))


def sized_params(scene, size):
    import raytracercore_amd as rc

    params = rc.rt_scene_params.from_buffer_copy(scene.params)
    params.width, params.height = size
    return params


def aabb_intersect_avx(box, O, D):
    """AABB.IntersectAVX (reference AABB.cs:107-142) in NumPy fp64 for the rays (O, D), each (n, 4), and
    one box (min xyzw, max xyzw): (near, far), both NaN on a miss."""
    mn, mx = np.broadcast_to(box[:4], O.shape), np.broadcast_to(box[4:], O.shape)
    with np.errstate(all="ignore"):
        inf_mask = (D == 0) & (O >= mn) & (O <= mx)
        mn = np.where(inf_mask, -np.inf, mn)
        mx = np.where(inf_mask, np.inf, mx)
        neg = np.signbit(D)  # BlendVariable takes the sign bit, -0 included
        min_m, max_m = np.where(neg, mx, mn), np.where(neg, mn, mx)
        inv = 1.0 / D
        near4, far4 = (min_m - O) * inv, (max_m - O) * inv

        def sse_max(a, b):  # maxpd: the second operand unless the first compares greater
            return np.where(a > b, a, b)

        def sse_min(a, b):
            return np.where(a < b, a, b)

        near2 = sse_max(near4[:, :2], near4[:, 2:])
        near = sse_max(near2[:, 0], near2[:, 1])
        far2 = sse_min(far4[:, :2], far4[:, 2:])
        far = sse_min(far2[:, 0], far2[:, 1])
        miss = (near > far) | (far < 0)
    return np.where(miss, np.nan, near), np.where(miss, np.nan, far)


def node_values(box, O, D):
    """BVHIntersector.Intersect (DebugRaycaster.cs:58-66)."""
    near, far = aabb_intersect_avx(box, O, D)
    with np.errstate(invalid="ignore"):
        return np.where(near >= 0, near, far)


def fold(values):
    """DebugRaycaster.GetColor, case Selection (DebugRaycaster.cs:174-192), over values[item, ray]:
    (item, distance) per ray, (-1, 0) where nothing won."""
    n = values.shape[1]
    dist, win = np.full(n, np.inf), np.full(n, -1, np.int32)
    with np.errstate(invalid="ignore"):
        for k in range(values.shape[0]):
            take = values[k] <= dist
            dist = np.where(take, values[k], dist)
            win = np.where(take, np.int32(k), win)
    return win, np.where(win < 0, 0.0, dist)


class Case:
    """A scene, the camera's rays of a FRAME-sized frame, and the reference side's per-item values."""

    def __init__(self, name):
        import raytracercore_amd as rc

        self.name = name
        self.scene = load_scene(name)
        self.prims = list(self.scene.prims)
        self.n_prims = len(self.prims)
        self.rays = rc.camera_rays(self.scene.cameras[0], FRAME).reshape(-1)
        self.O, self.D = self.rays["origin"], self.rays["direction"]
        n = self.rays.size
        params, cams = sized_params(self.scene, FRAME), list(self.scene.cameras)
        self.boxes = OracleScene.from_abi(params, self.prims, cams).bvh_boxes()  # pre-order, the oracle's own
        # E[k, i]: Hit.Distance of primitive k alone for ray i, NaN on a miss; box1[k]: its lone leaf's box
        self.E = np.full((self.n_prims, n), np.nan)
        self.box1 = np.zeros((self.n_prims, 8))
        for k in range(self.n_prims):
            orc = OracleScene.from_abi(params, [self.prims[k]], cams)
            self.box1[k] = orc.bvh_boxes()[0]
            for i in range(n):
                pid, dist = orc.raytrace(self.O[i], self.D[i])
                if pid == 0:
                    self.E[k, i] = dist
        for a in (self.rays, self.boxes, self.E, self.box1):
            a.setflags(write=False)

    def values(self, items, O=None, D=None):
        """The reference side's value of every item of the list for every ray: [item, ray].  Primitive
        items are known for the case's own rays only."""
        own = O is None
        O, D = (self.O, self.D) if own else (O, D)
        rows = []
        for kind, index in items:
            if kind == PRIM:
                assert own
                rows.append(self.E[index])
            else:
                rows.append(node_values(self.boxes[index], O, D))
        return np.array(rows).reshape(len(rows), O.shape[0])

    def structure(self):
        """(an internal node other than the root, two leaves) of the reference BVH in pre-order.  The last
        two nodes of a pre-order are leaves (an internal node is followed by at least two nodes); a node
        whose box is no single primitive's box is internal."""
        n_nodes = len(self.boxes)
        assert n_nodes == 2 * self.n_prims - 1
        leaf_boxes = {self.box1[k].tobytes() for k in range(self.n_prims)}
        internal = [j for j in range(1, n_nodes) if self.boxes[j].tobytes() not in leaf_boxes]
        assert internal and self.boxes[n_nodes - 1].tobytes() in leaf_boxes and self.boxes[n_nodes - 2].tobytes() in leaf_boxes
        return internal[len(internal) // 2], (n_nodes - 2, n_nodes - 1)


@functools.lru_cache(maxsize=None)
def case(name):
    return Case(name)


def host_select(cs):
    import raytracercore_amd as rc

    return lambda items, rays=None: rc.select_rays_host(cs.prims, items, cs.rays if rays is None else rays)


def same_bits(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def check_singles(cs, select):
    """Every primitive as a single item, through select(items) -> SELECTION_DTYPE per ray of the case.
    A hit of the oracle must be matched bit for bit; a miss of the oracle that the library hits is allowed
    only where the restated box test misses the one-primitive scene's box.  Returns excluded[item, ray]."""
    n = cs.rays.size
    excluded = np.zeros((cs.n_prims, n), bool)
    for k in range(cs.n_prims):
        got = select([(PRIM, k)])
        assert got.shape == (n,) and not got["reserved"].any()
        assert np.isin(got["item"], (-1, 0)).all()
        lib_hit, orc_hit = got["item"] == 0, ~np.isnan(cs.E[k])
        assert not got["distance"][~lib_hit].view(np.uint64).any(), k  # nothing won: distance +0
        assert lib_hit[orc_hit].all(), (k, "the oracle hits where the library misses")
        assert same_bits(got["distance"][orc_hit], cs.E[k][orc_hit]), k
        extra = lib_hit & ~orc_hit
        if extra.any():
            near, _ = aabb_intersect_avx(cs.box1[k], cs.O[extra], cs.D[extra])
            assert np.isnan(near).all(), (k, "a hit the oracle does not have, and its box is not missed")
            excluded[k] = extra
    pairs = cs.n_prims * n
    print(f"{cs.name}: {int(excluded.sum())} of {pairs} (ray, item) pairs excluded (box-face rounding)")
    assert excluded.sum() * 1000 <= pairs
    return excluded


@functools.lru_cache(maxsize=None)
def host_excluded(name):
    """check_singles through the host twin, once per case (H3's first check; the lists reuse its mask)."""
    cs = case(name)
    ex = check_singles(cs, host_select(cs))
    ex.setflags(write=False)
    return ex


def check_list(cs, items, got, excluded, O=None, D=None):
    """got against the fold of the reference side's values, over the rays no excluded pair touches."""
    win, dist = fold(cs.values(items, O, D))
    keep = np.ones(win.shape, bool)
    for kind, index in items:
        if kind == PRIM and O is None:
            keep &= ~excluded[index]
    assert (~keep).sum() * 1000 <= len(items) * keep.size
    assert not got["reserved"].any()
    assert np.array_equal(got["item"][keep], win[keep]), cs.name
    assert same_bits(got["distance"][keep], dist[keep]), cs.name
    return win, dist, keep


def h3_lists(cs):
    n = cs.n_prims
    everything = [(PRIM, k) for k in range(n)]
    win = fold(cs.E)[0]
    dup = int(np.bincount(win[win >= 0]).argmax())  # the primitive nearest on most rays
    twice = everything + [(PRIM, dup)]
    return {"all": everything, "reversed": everything[::-1], "twice": twice}


def h4_lists(cs):
    internal, (leaf_a, leaf_b) = cs.structure()
    nodes = [(NODE, 0), (NODE, internal), (NODE, leaf_a), (NODE, leaf_b)]
    prims = [(PRIM, k) for k in range(cs.n_prims)]
    lists = {f"node{j}": [it] for j, it in enumerate(nodes)}
    lists["nodes_then_prims"] = nodes + prims
    lists["prims_then_nodes"] = prims + nodes
    lists["interleaved"] = [it for pair in zip(prims, nodes * len(prims)) for it in pair]
    return lists


def h5_rays(cs):
    """Crafted rays against one internal node's box: (rays, the node's item list, notes per ray)."""
    import raytracercore_amd as rc

    internal, _ = cs.structure()
    box = cs.boxes[internal]
    lo, hi = box[:3], box[4:7]
    ctr, ext = (lo + hi) / 2, hi - lo
    assert (ext > 0).all()
    s = 1 / np.sqrt(2.0)
    o = np.array([
        ctr,                                  # 0 origin inside the box: far
        ctr + [3 * ext[0], 0, 0],             # 1 the box wholly behind the ray
        ctr - [3 * ext[0], 0, 0],             # 2 ... and in front of it, zero y and z components, inside both slabs
        ctr - [3 * ext[0], 2 * ext[1], 0],    # 3 zero y component, the origin outside the y slab
        ctr - [3 * ext[0], 0, 0],             # 4 zero z component only
        [lo[0] - 1, hi[1], ctr[2]],           # 5 on the slab's face (>= and <= are inclusive)
        ctr, ctr, ctr, ctr, ctr,              # 6-10 invalid rays
    ])
    d = np.array([[1, 0, 0], [1, 0, 0], [1, 0, 0], [1, 0, 0], [s, s * ext[1] / (8 * ext[0]), 0], [1, 0, -0.0],
                  [1, 0, 0], [1, 0, 0], [0, 0, 0], [np.nan, 0, 1], [0, -np.inf, 0]], np.float64)
    d[4] /= np.linalg.norm(d[4])
    o = o.copy()
    o[6, 1] = np.nan
    o[7, 2] = np.inf
    rays = rc._pack_rays(o, d)
    return rays, [(NODE, internal)], {"inside": 0, "behind": 1, "ahead": 2, "outside_slab": 3, "invalid": [6, 7, 8, 9, 10]}


# ------------------------------------------------------------------------------------------- H1, H2
@pytest.fixture(scope="module")
def c_layout(tmp_path_factory):
    """tests/host/select_layout.c compiled as C99 against include/rtcore.h, and what it prints."""
    exe = str(tmp_path_factory.mktemp("layout") / "select_layout")
    subprocess.run(["cc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", exe,
                    os.path.join(ROOT, "tests", "host", "select_layout.c")], check=True)
    lines = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split("\n")
    return [ln.split() for ln in lines if ln]


def test_h1_layouts_agree(rc, c_layout):
    """H1: sizes 8 / 16 and every offset agree in C, ctypes and the numpy dtypes; kinds 0 / 1; ABI 6."""
    assert c_layout[0] == ["sizeof", "8", "16"]
    assert C.sizeof(rc.rt_select_item) == 8 == rc.SELECT_ITEM_DTYPE.itemsize
    assert C.sizeof(rc.rt_selection) == 16 == rc.SELECTION_DTYPE.itemsize
    want = [("rt_select_item.kind", 0, 4), ("rt_select_item.index", 4, 4), ("rt_selection.item", 0, 4),
            ("rt_selection.reserved", 4, 4), ("rt_selection.distance", 8, 8)]
    assert [(n, int(o), int(s)) for n, o, s in c_layout[1:6]] == want
    for full, off, size in want:
        struct, field = full.split(".")
        cf = getattr(getattr(rc, struct), field)
        assert (cf.offset, cf.size) == (off, size), full
        dt, doff = (rc.SELECT_ITEM_DTYPE if struct == "rt_select_item" else rc.SELECTION_DTYPE).fields[field][:2]
        assert (doff, dt.itemsize) == (off, size), full
    assert [n for n, _ in rc.rt_select_item._fields_] == list(rc.SELECT_ITEM_DTYPE.names) == ["kind", "index"]
    assert [n for n, _ in rc.rt_selection._fields_] == list(rc.SELECTION_DTYPE.names) == ["item", "reserved", "distance"]
    assert c_layout[6] == ["kinds", "0", "1", "abi", "6", "max_tests_is_2_32", "1"]
    assert (rc.RT_SELECT_PRIM, rc.RT_SELECT_NODE) == (0, 1) == (PRIM, NODE)
    assert rc.RT_SELECT_MAX_TESTS == 2 ** 32
    assert rc.ABI_VERSION == 6 and rc.load_library().rt_abi_version() == 6


def test_h2_exported_and_bound(rc):
    lib = rc.load_library()
    out = subprocess.run(["nm", "-D", "--defined-only", rc.LIB_PATH], capture_output=True, text=True).stdout
    for name in ("rt_select_pixels", "rt_select_pixels_device", "rt_select_rays", "rt_select_rays_device",
                 "rt_debug_select_rays"):
        assert f" T {name}\n" in out
        assert getattr(lib, name).argtypes is not None
    for name in ("select_pixels", "select_pixels_device", "select_rays", "select_rays_device"):
        assert hasattr(rc.GpuRaytracer, name)
    assert callable(rc.select_rays_host)


def test_pack_items(rc):
    """The item list's input forms: an (n, 2) int array, (kind, index) pairs, the dtype itself, nothing."""
    want = np.array([(0, 5), (1, 2)], rc.SELECT_ITEM_DTYPE)
    assert same_bits(rc._pack_items([(0, 5), (1, 2)]), want)
    assert same_bits(rc._pack_items(np.array([[0, 5], [1, 2]], np.int64)), want)
    assert same_bits(rc._pack_items(want), want)
    assert rc._pack_items([]).shape == (0,) and rc._pack_items(np.zeros((0, 2), int)).dtype == rc.SELECT_ITEM_DTYPE
    for bad in ([1, 2, 3], [(0, 1, 2)], [(0, 2 ** 31)]):
        with pytest.raises(ValueError):
            rc._pack_items(bad)


# ------------------------------------------------------------------------------------------- H3
H3_CASES = ("bounce", "die", "extra")


def test_extra_scene_has_what_the_fixtures_lack(rc):
    """The text parses, and adds a transformed sphere, a two-sided plain sphere, a plane, inverted and
    one-sided triangles."""
    prims = case("extra").prims
    flags = [(p.kind, p.flags) for p in prims]
    sph = [f for k, f in flags if k == rc.RT_PRIM_SPHERE]
    assert len(sph) == 2
    assert sph[0] & rc.RT_FLAG_TRANSFORMED and not sph[0] & rc.RT_FLAG_TWOSIDED
    assert sph[1] & rc.RT_FLAG_TWOSIDED and not sph[1] & rc.RT_FLAG_TRANSFORMED
    assert any(k == rc.RT_PRIM_PLANE for k, _ in flags)
    tri = [f for k, f in flags if k == rc.RT_PRIM_TRIANGLE]
    assert any(f & rc.RT_FLAG_INVERT for f in tri) and any(not f & rc.RT_FLAG_TWOSIDED for f in tri)
    assert any(f & rc.RT_FLAG_TWOSIDED for f in tri)
    assert load_scene("extra_ortho").cameras[0].kind == rc.RT_CAMERA_ORTHO
    assert len(load_scene("extra_ortho").prims) == len(prims)


@pytest.mark.parametrize("name", H3_CASES)
def test_h3_every_primitive_alone(name):
    """H3: every primitive as a single item equals the one-primitive oracle scene bit for bit."""
    cs = case(name)
    host_excluded(name)
    hit_any = ~np.isnan(cs.E)
    assert hit_any.any(axis=1).sum() >= cs.n_prims // 2  # most primitives are on screen
    assert (~hit_any).any()


@pytest.mark.parametrize("which", ["all", "reversed", "twice"])
@pytest.mark.parametrize("name", H3_CASES)
def test_h3_lists(name, which):
    """H3: all primitives in insertion order, the same list reversed (among equal distances the other
    item wins), and a list naming one primitive twice (its later index wins wherever it is hit)."""
    cs = case(name)
    excluded = host_excluded(name)
    items = h3_lists(cs)[which]
    got = host_select(cs)(items)
    win, dist, keep = check_list(cs, items, got, excluded)
    assert (win >= 0).any()
    n = cs.n_prims
    if which == "reversed":
        fwd = host_select(cs)(h3_lists(cs)["all"])
        vals = cs.values(h3_lists(cs)["all"])
        with np.errstate(invalid="ignore"):
            ties = (vals == fold(vals)[1][None, :]).sum(axis=0) > 1
        ties &= keep & (fwd["item"] >= 0)
        print(f"{name}: {int(ties.sum())} rays with two primitives at the winning distance")
        flipped = np.where(got["item"] >= 0, n - 1 - got["item"], -1) != fwd["item"]
        assert np.array_equal(flipped[keep], ties[keep])  # the winner flips exactly at the ties
        assert same_bits(got["distance"][keep], fwd["distance"][keep])
    if which == "twice":
        first, second = items[-1][1], len(items) - 1
        assert items[second] == items[first] and second == n
        assert (got["item"] == second).any()  # the duplicate wins somewhere: a guaranteed tie
        assert not (got["item"] == first).any()  # ... and its earlier copy never does
        pair = host_select(cs)([items[first]] * 2)
        check_list(cs, [items[first]] * 2, pair, excluded)
        hit = ~np.isnan(cs.E[first])
        assert hit.any() and (pair["item"][hit] == 1).all() and (pair["item"][~hit & ~excluded[first]] == -1).all()


# ------------------------------------------------------------------------------------------- H4
def test_h4_node_items():
    """H4: the root, an internal node and two leaves of bounce.txt's reference BVH, each alone and mixed
    with the primitives in both orders."""
    cs = case("bounce")
    excluded = host_excluded("bounce")
    lists = h4_lists(cs)
    for label, items in lists.items():
        got = host_select(cs)(items)
        win, _, _ = check_list(cs, items, got, excluded)
        assert (win >= 0).any() and (label != "node0" or (win < 0).any()), label
    # a node in front of the primitives it holds wins only when it comes last among equal distances:
    # the two mixed orders differ somewhere
    a = host_select(cs)(lists["nodes_then_prims"])["item"]
    b = host_select(cs)(lists["prims_then_nodes"])["item"]
    n_nodes = 4
    assert ((a < n_nodes) & (a >= 0)).any() and (b >= cs.n_prims).any()


# ------------------------------------------------------------------------------------------- H5
def test_h5_crafted_rays():
    """H5: the origin inside the box (far), the box behind the ray (not selected), zero direction
    components inside and outside their slabs, invalid rays (-1), an empty list (-1, distance 0)."""
    cs = case("bounce")
    rays, items, note = h5_rays(cs)
    got = host_select(cs)(items, rays)
    O, D = rays["origin"], rays["direction"]
    valid = np.ones(rays.size, bool)
    valid[note["invalid"]] = False
    win, dist = fold(cs.values(items, O[valid], D[valid]))
    assert np.array_equal(got["item"][valid], win) and same_bits(got["distance"][valid], dist)
    assert (got["item"][~valid] == -1).all() and not got["distance"][~valid].view(np.uint64).any()
    near, far = aabb_intersect_avx(cs.boxes[items[0][1]], O, D)
    i = note["inside"]
    assert near[i] < 0 < far[i] and got["item"][i] == 0 and got["distance"][i] == far[i]
    assert got["item"][note["behind"]] == -1 and got["distance"][note["behind"]] == 0
    i = note["ahead"]
    assert got["item"][i] == 0 and got["distance"][i] == near[i] > 0
    assert got["item"][note["outside_slab"]] == -1
    assert got["item"][4] == 0 and got["item"][5] == 0
    # the same rays through a mixed list: the primitives' values are not known for these rays from the
    # oracle's camera set, so only the invalid ones are checked here
    mixed = host_select(cs)(items + [(PRIM, 0), (PRIM, 13)], rays)
    assert (mixed["item"][~valid] == -1).all() and not mixed["distance"][~valid].view(np.uint64).any()
    # an empty list: the reference with no intersectors
    for r in (rays, cs.rays):
        empty = host_select(cs)([], r)
        assert (empty["item"] == -1).all() and not empty["distance"].view(np.uint64).any() and not empty["reserved"].any()
    # +inf wins over "none": a ray along a slab it starts in, against a box unbounded on that axis, does
    # not occur with finite boxes; the fold's own rule is pinned instead
    w, dd = fold(np.array([[np.inf, np.nan, 1.0], [np.nan, np.nan, 1.0]]))
    assert list(w) == [0, -1, 1] and dd[0] == np.inf and dd[1] == 0 and dd[2] == 1.0


# ------------------------------------------------------------------------------------------- H6
def last_error(lib):
    buf = C.create_string_buffer(512)
    lib.rt_last_error(buf, 512)
    return buf.value.decode()


def test_h6_host_twin_arguments(rc):
    """H6: every RT_ERR_ARG case of rt_debug_select_rays; nothing is written."""
    lib = rc.load_library()
    cs = case("bounce")
    n_p = cs.n_prims
    prims = (rc.rt_prim * n_p)(*cs.prims)
    met = np.flatnonzero(fold(cs.values([(NODE, 0)]))[0] == 0)[:4]  # four rays that meet the root's box
    rays = np.ascontiguousarray(cs.rays[met])
    out = np.zeros(4, rc.SELECTION_DTYPE)
    pr, po = rays.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)

    def call(items, n_items=None, p=prims, np_=n_p, r=pr, n=4, o=po):
        it = rc._pack_items(items if items is not None else [])
        pi = it.ctypes.data_as(C.c_void_p) if items is not None else None
        code = lib.rt_debug_select_rays(p, np_, pi, it.size if n_items is None else n_items, r, n, o)
        return code, last_error(lib)

    ok = [(PRIM, 0), (NODE, 0)]
    assert call(ok)[0] == 0 and out["item"].max() >= 0
    out[:] = 0
    n_nodes = 2 * n_p - 1
    bad = {
        "null prims": dict(items=ok, p=None),
        "null items": dict(items=None, n_items=2),
        "null rays": dict(items=ok, r=None),
        "null out": dict(items=ok, o=None),
        "n_prims < 0": dict(items=ok, np_=-1),
        "n_items < 0": dict(items=ok, n_items=-1),
        "n < 0": dict(items=ok, n=-1),
        "kind 2": dict(items=[(PRIM, 0), (2, 0)]),
        "kind -1": dict(items=[(-1, 0)]),
        "prim -1": dict(items=[(PRIM, -1)]),
        "prim n_prims": dict(items=[(PRIM, 0), (PRIM, n_p)]),
        "node -1": dict(items=[(NODE, -1)]),
        "node n_nodes": dict(items=[(NODE, n_nodes - 1), (NODE, n_nodes)]),
    }
    for label, kw in bad.items():
        code, msg = call(**kw)
        assert code == -1 and "rt_debug_select_rays" in msg, label
        assert not out.view(np.uint8).any(), label
    assert call([(NODE, n_nodes - 1)])[0] == 0
    out[:] = 0
    # more than RT_SELECT_MAX_TESTS item tests: refused before a ray is read, and the message states the bound
    code, msg = call([(PRIM, 0)] * 3, n=2 ** 31)
    assert code == -1 and "RT_SELECT_MAX_TESTS" in msg and "2^32" in msg
    assert not out.view(np.uint8).any()
    # an unknown primitive kind
    broken = (rc.rt_prim * n_p)(*cs.prims)
    broken[3].kind = 7
    assert call(ok, p=broken)[0] == -1
    # n == 0 touches nothing, whatever the pointers; n_items == 0 is valid
    assert call(ok, r=None, n=0, o=None)[0] == 0
    assert call([])[0] == 0 and (out["item"] == -1).all()
    with pytest.raises(rc.RtError):
        rc.select_rays_host(cs.prims, [(PRIM, n_p)], cs.rays[:4])
