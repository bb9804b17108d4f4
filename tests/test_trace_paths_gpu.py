"""rt_trace_paths on the device: per-bounce records of the library's own samples.

Exact part (the library against itself): a sample's value depends only on seed, pixel, sample
index, scene and traversal mode, so every traced sample's colour equals the 1-spp render of that
sample bit for bit, and the record counts add up to the render's ray count.  Oracle part: the
records' (primitive, event) sequences against orc_sample_trace, and the Fresnel ratios against
orc_fresnel.  Every record set also goes through the structural rules of `_check_rules`.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIZE = (128, 128)
CONTINUES = (1, 2, 4)        # DIFFUSE, SPECULAR, TRANSMITTED: the path goes on
ENDS = (3, 5, 6, 7, 8, 9)    # SPECULAR_FAIL, EMISSION, PURE_BLACK, RECURSION_COMPLETE, MISSED, DEBUG


def _gpu(rc, scene, mode="AUTO", builder=None, size=SIZE, cam=0):
    return rc.GpuRaytracer(scene, cam, size=size, traversal=getattr(rc, "RT_TRAVERSAL_" + mode),
                           builder=None if builder is None else getattr(rc, "RT_BVH_BUILDER_" + builder))


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _check_rules(rc, rec, n_rays, recursion):
    """The rules that hold for every record of a trace, exactly."""
    per = recursion + 1
    assert rec.shape[-1] == per and rec.dtype == rc.DEBUG_RAY_DTYPE
    rec = rec.reshape(-1, per)
    n = n_rays.reshape(-1)
    assert n.min() >= 1 and n.max() <= per
    idx = np.arange(per)[None, :]
    live, last = idx < n[:, None], idx == (n[:, None] - 1)
    t = rec["type"]
    bounce = np.broadcast_to(idx, t.shape)
    assert np.array_equal(t == rc.RT_BOUNCE_MISSED, (rec["prim_id"] == -1) & live)
    assert np.isin(t[last], ENDS).all()
    assert np.isin(t[live & ~last], CONTINUES).all()
    assert (bounce[t == rc.RT_BOUNCE_RECURSION_COMPLETE] == recursion).all()
    assert np.array_equal(rec["bounce"][live], bounce[live])
    f = rec["fresnel"][live]
    assert (np.isnan(f) | ((f >= 0) & (f <= 1))).all()
    assert (rec["fresnel"][t == rc.RT_BOUNCE_TRANSMITTED] < 1).all()
    # the ray of bounce i + 1 starts where bounce i hit, bit for bit
    nxt = live[:, 1:]
    assert np.array_equal(_bits(rec["origin"][:, 1:])[nxt], _bits(rec["position"][:, :-1])[nxt])
    # past the end of a path: all zero (type Skipped)
    assert not rec[~live].view(np.uint8).any()
    return rec, n


def _colors_equal_1spp(gpu, colors, tile, seed, base, ks=None):
    spp = colors.shape[2]
    for k in range(spp) if ks is None else ks:
        one = gpu.render_tile_1spp(*tile, seed=seed, sample_index=base + k)
        assert np.array_equal(colors[:, :, k].view(np.uint64), one.view(np.uint64)), f"sample {k}"


# ---------------------------------------------------------------- the premise, on existing calls
@pytest.mark.parametrize("mode", ["BRUTE", "GROUPED", "BVH", "BVH2"])
def test_sample_value_is_tile_independent(rc, scenes, mode):
    """A 1-spp pass over a tile and over a 1x1 tile at one of its pixels return the same value."""
    gpu = _gpu(rc, scenes["bounce.txt"], mode)
    tile = gpu.render_tile_1spp(70, 60, 13, 11, seed=5, sample_index=4)
    for x, y in ((0, 0), (6, 5), (12, 10)):
        one = gpu.render_tile_1spp(70 + x, 60 + y, 1, 1, seed=5, sample_index=4)
        assert np.array_equal(one[0, 0].view(np.uint64), tile[x, y].view(np.uint64))
    gpu.close()


# ---------------------------------------------------------------- G1: every kernel, a ragged tile
G1_TILE, G1_SEED, G1_BASE, G1_SPP = (70, 60, 13, 11), 5, 3, 5


def _g1(rc, gpu):
    recursion = gpu.params.recursion
    rec, n, col = gpu.trace_paths(*G1_TILE, G1_SPP, seed=G1_SEED, sample_base=G1_BASE)
    assert rec.shape == (13, 11, G1_SPP, recursion + 1) and n.shape == (13, 11, G1_SPP) and col.shape == (13, 11, G1_SPP, 3)
    _colors_equal_1spp(gpu, col, G1_TILE, G1_SEED, G1_BASE)
    rays = gpu.render_tile(*G1_TILE, G1_SPP, seed=G1_SEED, sample_base=G1_BASE)[3]
    assert int(n.sum()) == rays
    _check_rules(rc, rec, n, recursion)
    return rec, n, col


@pytest.mark.parametrize("mode,builder", [("BRUTE", None), ("GROUPED", None), ("BVH", "HOST"), ("BVH", "GPU"),
                                          ("BVH2", None)])
def test_g1_colors_and_ray_counts(rc, scenes, mode, builder):
    gpu = _gpu(rc, scenes["bounce.txt"], mode, builder)
    assert gpu.info().traversal == getattr(rc, "RT_TRAVERSAL_" + mode)
    rec, n, _ = _g1(rc, gpu)
    # the window holds the lens and full-depth paths (checked with the oracle on the CPU)
    t = rec["type"]
    assert {1, 2, 4, 5, 7} <= set(np.unique(t).tolist())
    assert (n == gpu.params.recursion + 1).sum() > 300
    gpu.close()


def test_g1_brute_without_scene_specialised_kernels(rc, scenes):
    """The same under rt_set_jit(0): the renders it is compared with then run the generic kernels."""
    rc.set_jit(False)
    try:
        gpu = _gpu(rc, scenes["bounce.txt"], "BRUTE")
        _g1(rc, gpu)
        gpu.close()
    finally:
        rc.set_jit(True)


# ---------------------------------------------------------------- G2: one pixel, many samples
@pytest.mark.parametrize("mode,spp", [("BRUTE", 256), ("GROUPED", 256), ("BVH", 600), ("BVH2", 600)])
def test_g2_one_pixel_many_samples(rc, scenes, mode, spp):
    """The inspector's shape: more samples than chunks (192 brute force, 512 BVH), so work items of
    two samples."""
    gpu = _gpu(rc, scenes["bounce.txt"], mode)
    tile, seed = (76, 65, 1, 1), 9
    rec, n, col = gpu.trace_paths(*tile, spp, seed=seed)
    _check_rules(rc, rec, n, gpu.params.recursion)
    ks = [0, 1, 2, 3, 17, 40, 77, 100, 101, 128, 129, 200, spp // 2 + 33, spp - 3, spp - 2, spp - 1]
    assert len(set(ks)) == 16
    _colors_equal_1spp(gpu, col, tile, seed, 0, ks)
    s, ns, ms, rays = gpu.render_tile(*tile, spp, seed=seed)
    assert int(n.sum()) == rays
    c = col[0, 0]
    hit = c[:, 0] != -1.0
    assert int(hit.sum()) == int(ns[0, 0]) and int((~hit).sum()) == int(ms[0, 0])
    total = np.zeros(3)
    for k in range(spp):  # fp64, in sample order
        if hit[k]:
            total += c[k]
    bound = 1e-6 * spp * float(np.abs(c[hit]).max())  # each item adds its samples in fp32
    print(f"{mode}: |sum - render_tile| = {np.abs(total - s[0, 0]).max():.3g}, bound {bound:.3g}")
    assert np.abs(total - s[0, 0]).max() <= bound
    gpu.close()


# ---------------------------------------------------------------- G3: primary misses
def test_g3_primary_misses(rc, scenes):
    gpu = _gpu(rc, scenes["die.txt"], "AUTO")
    print("die.txt AUTO resolves to traversal", gpu.info().traversal)
    tile, spp, seed = (90, 20, 13, 11), 3, 5
    rec, n, col = gpu.trace_paths(*tile, spp, seed=seed)
    _check_rules(rc, rec, n, gpu.params.recursion)
    _colors_equal_1spp(gpu, col, tile, seed, 0)
    missed = rec["type"][..., 0] == rc.RT_BOUNCE_MISSED
    assert 0 < missed.sum() < missed.size
    assert (n[missed] == 1).all() and (col[missed] == -1.0).all() and (rec["prim_id"][..., 0][missed] == -1).all()
    for k in range(spp):
        one = gpu.render_tile_1spp(*tile, seed=seed, sample_index=k)
        assert np.array_equal(missed[:, :, k], (one == -1.0).all(axis=-1))
    gpu.close()


# ---------------------------------------------------------------- G4: vertex normals
# (the two scenes of tests/test_gpu_oracle_paths.py)
VN_SCENE = """size 64 48
camera 0 -1.2 3.2, 0 0 0, 0 0 1, 70
ambient color .3 .3 .35
emission 4 4 4
sphere 0 0 4 .8
emission 0 0 0
diffuse .6 .5 .4
specular .3 .3 .3
shininess 10 2
twosided true
vertexnormal -2 -1 0  -.3 -.3 1
vertexnormal 0 -1 .3   0 -.3 1
vertexnormal 0 1 .3   0 .3 1
vertexnormal -2 1 0 -.3 .3 1
trinormal 0 1 2
trinormal 0 2 3
vertexnormal 0 -1 .3   0 -.3 1
vertexnormal 2 -1 0  .3 -.3 1
vertexnormal 2 1 0 .3 .3 1
vertexnormal 0 1 .3   0 .3 1
trinormal 4 6 5
trinormal 4 7 6
diffuse .3 .3 .3
specular 0 0 0
shininess 4 .5
plane -1 0 0 1
"""
VN_ROOM_SCENE = VN_SCENE.replace("plane -1 0 0 1\n", "twosided false\ninvert true\ndiffuse .5 .5 .5\n"
                                 "cube 0 0 2 6 6 7 all\n")


@pytest.mark.parametrize("mode", ["BRUTE", "BVH"])
@pytest.mark.parametrize("name", ["VN_SCENE", "VN_ROOM_SCENE"])
def test_g4_vertex_normal_scenes(rc, name, mode):
    scene = rc.SceneLoader.from_text(globals()[name])
    gpu = _gpu(rc, scene, mode, size=(64, 48))
    tile, spp, seed = (0, 0, 64, 48), 2, 5
    rec, n, col = gpu.trace_paths(*tile, spp, seed=seed)
    _check_rules(rc, rec, n, gpu.params.recursion)
    _colors_equal_1spp(gpu, col, tile, seed, 0)
    assert int(n.sum()) == gpu.render_tile(*tile, spp, seed=seed)[3]
    gpu.close()


# ---------------------------------------------------------------- G5: PureBlack and Debug
BLACK_SCENE = """size 32 32
recursion 4
camera 0 -4 0, 0 0 0, 0 0 1, 50
ambient color .2 .2 .2
diffuse 0 0 0
specular 0 0 0
emission 3 3 3
sphere 0 3 0 2.5
emission 0 0 0
sphere 0 0 0 .8
diffuse .6 .6 .6
plane -1 0 0 1
"""


def test_g5_pure_black(rc):
    """A primitive of no luminance at all in front of an emitter, over a diffuse floor."""
    scene = rc.SceneLoader.from_text(BLACK_SCENE)
    gpu = _gpu(rc, scene, "BRUTE", size=(32, 32))
    tile, spp, seed = (0, 0, 32, 32), 2, 3
    rec, n, col = gpu.trace_paths(*tile, spp, seed=seed)
    recs, ns = _check_rules(rc, rec, n, gpu.params.recursion)
    _colors_equal_1spp(gpu, col, tile, seed, 0)
    black = recs["type"] == rc.RT_BOUNCE_PURE_BLACK
    assert black.any() and (recs["prim_id"][black] == 1).all()
    rows = black.any(axis=1)
    assert np.array_equal(np.argmax(black, axis=1)[rows], ns[rows] - 1)  # the last record of its path
    assert (col.reshape(-1, 3)[rows] == 0.0).all()
    assert (recs["type"] == rc.RT_BOUNCE_EMISSION).any()
    gpu.close()


def test_g5_debug_geom(rc):
    scene = rc.SceneLoader.from_text(open(rc.scene_path("bounce.txt")).read() + "\ndebug geom\n")
    gpu = _gpu(rc, scene, "AUTO", size=(48, 48))
    tile, spp, seed = (0, 0, 48, 48), 2, 3
    rec, n, col = gpu.trace_paths(*tile, spp, seed=seed)
    recs, ns = _check_rules(rc, rec, n, gpu.params.recursion)
    _colors_equal_1spp(gpu, col, tile, seed, 0)
    hit = recs["prim_id"][:, 0] >= 0
    assert hit.any() and (ns == 1).all()
    assert (recs["type"][hit, 0] == rc.RT_BOUNCE_DEBUG).all()
    assert ((recs["type"] == rc.RT_BOUNCE_DEBUG).sum(axis=1)[hit] == 1).all()
    assert np.isfinite(recs["position"][hit, 0]).all() and (recs["distance"][hit, 0] > 0).all()
    gpu.close()


# ---------------------------------------------------------------- G7: side effects
@pytest.mark.parametrize("mode", ["BRUTE", "BVH"])
def test_g7_leaves_counters_and_renders_alone(rc, scenes, mode):
    gpu = _gpu(rc, scenes["bounce.txt"], mode)
    tile = (64, 56, 24, 16)
    before = gpu.render_tile(*tile, 4, seed=2)
    gpu.set_stats(True)
    gpu.render_tile(*tile, 4, seed=2)
    alone = gpu.get_stats()
    gpu.render_tile(*tile, 4, seed=2)
    gpu.trace_paths(*G1_TILE, 2, seed=7)
    both = gpu.get_stats()
    for name in ("node_visits", "tri_tests", "sph_tests", "wave_iters"):  # counters [0..2] and [6]
        assert both[name] == alone[name], name
    assert alone["wave_iters"] > 0
    gpu.trace_paths(*G1_TILE, 2, seed=7)  # ... and on its own it adds nothing to them
    idle = gpu.get_stats()
    assert all(idle[name] == 0 for name in ("node_visits", "tri_tests", "sph_tests", "wave_iters")), idle
    gpu.set_stats(False)
    gpu.trace_paths(*G1_TILE, 2, seed=7)
    after = gpu.render_tile(*tile, 4, seed=2)
    for a, b in zip(before[:3], after[:3]):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    assert before[3] == after[3]
    gpu.close()


# ---------------------------------------------------------------- against the oracle
def test_paths_against_oracle(rc, scenes):
    """G1's window and samples in mode BRUTE against orc_sample_trace.

    Measured on an MI355X (bounce.txt 128x128, 715 samples): see DESIGN.md, "Path inspection".
    """
    # (whole paths only: the check of every bounce, diverged paths included, is tests/test_bounce_step_gpu.py)
    from oracle.oracle import OracleScene, fresnel as orc_fresnel

    scene = scenes["bounce.txt"]
    gpu = _gpu(rc, scene, "BRUTE")
    recursion = gpu.params.recursion
    params = rc.rt_scene_params.from_buffer_copy(scene.params)
    params.width, params.height = SIZE
    orc = OracleScene.from_abi(params, list(scene.prims), list(scene.cameras))
    orc.select_camera(0)
    rec, n, col = gpu.trace_paths(*G1_TILE, G1_SPP, seed=G1_SEED, sample_base=G1_BASE)
    x0, y0, w, h = G1_TILE
    total = first = whole = 0
    fres_kept = fres_skipped = 0
    fres_err = 0.0
    for x in range(w):
        for y in range(h):
            for k in range(G1_SPP):
                ocol, omiss, opath = orc.sample_trace(x0 + x, y0 + y, seed=G1_SEED, sample=G1_BASE + k,
                                                      recursion=recursion)
                r = rec[x, y, k, :n[x, y, k]]
                gpath = [(int(p), int(t) if t <= 5 else -2) for p, t in zip(r["prim_id"], r["type"])]
                total += 1
                first += gpath[0] == opath[0]
                if gpath != opath:
                    continue
                whole += 1
                o = np.array((-1.0, -1.0, -1.0) if omiss else ocol)
                assert np.all(np.abs(col[x, y, k] - o) <= 1e-3 * np.maximum(1.0, np.abs(o))), (x, y, k, col[x, y, k], o)
                for q in r[np.isfinite(r["fresnel"]) & (r["fresnel"] < 1)]:
                    ior = scene.prims[int(q["prim_id"])].refractive_index
                    ior_in, ior_out = (ior, params.air_ior) if q["inside"] else (params.air_ior, ior)
                    cs = float(q["cos_in"])
                    if (ior_in / ior_out) * np.sqrt(max(0.0, 1 - cs * cs)) > 0.995:
                        fres_skipped += 1  # sqrt(1 - sin^2) loses fp32 digits there
                        continue
                    fres_kept += 1
                    err = abs(float(q["fresnel"]) - orc_fresnel(cs, ior_in, ior_out))
                    fres_err = max(fres_err, err)
                    assert err <= 1e-3, (x, y, k, q, err)
    print(f"first bounce agrees {first}/{total} = {first / total:.4f}; whole paths {whole}/{total} = "
          f"{whole / total:.4f}; Fresnel records compared {fres_kept}, left out {fres_skipped}, "
          f"largest error {fres_err:.3g}")
    assert first / total >= 0.97
    assert whole / total >= 0.5
    assert fres_kept >= 50
    assert fres_skipped <= 0.10 * fres_kept
    gpu.close()
