"""Scenes, tiles and the record-by-record comparison of the bounce-step tests, shared by
tests/test_bounce_step_host.py (the oracle's own paths) and tests/test_bounce_step_gpu.py (the records of
rt_trace_paths).

A path is held as one row per sample of padded per-bounce arrays (`Paths`); `compare` feeds every
record's own direction, normal, inside, primitive and bounce index, with the draw cursor that the
recorded types imply, to the oracle's bounce step (orc_shade_steps) and reports the largest errors, the
excluded decisions and the per-class counts.  It asserts nothing: the two test modules do.
"""
import math
from dataclasses import dataclass

import numpy as np

from test_trace_paths_gpu import VN_ROOM_SCENE

DIFFUSE, SPECULAR, SPECULAR_FAIL, TRANSMITTED, EMISSION, PURE_BLACK, RECURSION_COMPLETE, MISSED, DEBUG = range(1, 10)
CONTINUES = (DIFFUSE, SPECULAR, TRANSMITTED)
SHADED = (DIFFUSE, SPECULAR, SPECULAR_FAIL, TRANSMITTED, EMISSION, PURE_BLACK)
MODES = ("BRUTE", "GROUPED", "BVH", "BVH2")

# The fp32 bounds of the GPU test: 4 x the largest error measured on an MI355X over all cases and modes,
# rounded up to one digit (the measured figures are in tests/test_bounce_step_gpu.py and DESIGN.md 4.1).
# cos_in, fresnel, direction, camera_*: absolute (direction: max-norm of the vector difference,
# length_*: difference of the two lengths, rays renormalised for the next bounce apart from the rays
# kept as they are); tint: relative; colour: relative to max(1, |c|).
BOUNDS = {"cos_in": 2e-6, "fresnel": 4e-5, "direction": 3e-5, "length_renormalised": 5e-7, "length_kept": 6e-6, "tint": 5e-7, "colour": 3e-7, "camera_origin": 9e-7,
          "camera_direction": 9e-7}
THRESHOLD = 8 * BOUNDS["cos_in"]  # a decision whose margin is under this is counted, not compared
EXCLUDED_CAP = 0.02        # ... and at most this share of a case's bounces may be
FRESNEL_LEFT_OUT_CAP = 0.10  # Fresnel ratios at sin_out > 0.995, as a share of the ones kept

SIZE = (64, 48)
SHININESS = (0.5, 1.0, 2.0, 50.0, 1e4, math.inf)

# ---------------------------------------------------------------- MATERIALS
# A closed room 6 x 6 x 3 (floor z = 0, ceiling z = 3: normals exactly -+z towards the inside, walls
# exactly +-x and +-y) lit by a ceiling panel, with one small object per material row of the issue.
_GRID = [(x, y) for y in (-1.6, -0.6, 0.4, 1.4) for x in (-2.2, -1.1, 0.0, 1.1, 2.2)]


def _materials_text(recursion=10, cameras=None):
    spot = iter(_GRID)
    out = ["size 64 48", f"recursion {recursion}", "ambient color .2 .3 .4"]
    out += cameras or ["camera 0 -2.9 2.2, 0 -.2 .3, 0 0 1, 75"]

    def mat(diffuse="0 0 0", specular="0 0 0", emission="0 0 0", shininess="250", refraction=None):
        out.extend([f"diffuse {diffuse}", f"specular {specular}", f"emission {emission}", f"shininess {shininess}",
                    f"refraction {refraction}" if refraction else "refraction 0 0 0, 0"])

    def sphere(r=.42):
        x, y = next(spot)
        out.append(f"sphere {x} {y} {r} {r}")

    def cube(s=.7, extra="all"):
        x, y = next(spot)
        out.append(f"cube {x} {y} {s / 2 + .001} {s} {s} {s} {extra}")

    # row 9: the room; one-sided, inverted (its faces look inwards)
    out += ["twosided false", "invert true"]
    mat(diffuse=".7 .7 .7", specular=".2 .2 .2", shininess="50")
    out.append("cube 0 0 1.5 6 6 3 all")
    out += ["invert false", "twosided true"]
    # row 5: the light, a pure emitter under the ceiling, and a small one on the floor
    mat(emission="6 6 5")
    out.append("cube 0 0 2.95 2.5 2.5 .1 all")
    sphere(.3)
    # row 1: glass 1.5 whose refraction tint is not its specular colour; glass with no specular colour
    mat(specular=".5 .5 .5", shininess="1e5", refraction=".9 .6 .3, 1.5")
    sphere()
    mat(shininess="1e5", refraction=".8 .8 .8, 1.5")
    sphere()
    # row 2: ior 2.4, a box (total internal reflection inside it)
    mat(specular=".9 .9 .9", shininess="1e5", refraction=".9 .9 .9, 2.4")
    cube()
    # row 3: thinner than air
    mat(specular=".9 .9 .9", shininess="1e5", refraction=".9 .9 .9, 0.8")
    sphere()
    # row 4: the shininess values
    for s in ("0.5", "1", "2", "50", "100 2", "inf"):
        mat(diffuse=".3 .3 .3", specular=".6 .6 .6", shininess=s)
        sphere(.5)
    # row 6: no luminance at all
    mat()
    sphere()
    # row 7: total > 1
    mat(diffuse="1 1 1", specular=".5 .5 .5")
    sphere()
    # row 8: diffuse only, specular only
    mat(diffuse=".7 .5 .3")
    sphere()
    mat(specular=".8 .8 .8")
    sphere()
    # row 9: a platform tilted 1e-4 rad off z
    mat(diffuse=".6 .6 .6", specular=".2 .2 .2", shininess="50")
    x, y = next(spot)
    t = 1e-4
    out += [f"vertex {x - .45} {y - .45} {.05 - .45 * t}", f"vertex {x + .45} {y - .45} {.05 + .45 * t}",
            f"vertex {x - .45} {y + .45} {.05 - .45 * t}", "tri 0 1 2 mirrored"]
    # row 10: a one-sided inverted glass box
    out += ["twosided false", "invert true"]
    mat(specular=".5 .5 .5", shininess="1e5", refraction=".9 .9 .9, 1.5")
    cube()
    out += ["invert false", "twosided true"]
    # row 11: a two-sided quad, standing
    mat(diffuse=".5 .6 .7", specular=".3 .3 .3", shininess="50")
    x, y = next(spot)
    out += [f"vertex {x - .4} {y} .01", f"vertex {x + .4} {y + .2} .01", f"vertex {x - .4} {y} .9", "tri 3 4 5 mirrored"]
    return "\n".join(out) + "\n"


FRUSTUM = "camera 0 -2.9 2.2, 0 -.2 .3, 0 0 1, 75"
DOF = "dof .1 1000 to 3"  # die.txt's form
ORTHO = "orthographic 0 -2.9 2.6, 0 -.2 .3, 0 0 1, .09"


@dataclass
class Case:
    name: str
    text: str = ""              # loader text, or
    shipped: str = ""           # the name of a shipped scene
    size: tuple = SIZE
    tile: tuple = (16, 20, 32, 24)
    seed: int = 1
    spp: int = 4
    air_ior: float = 0.0        # 0: the loader's default
    modes: tuple = MODES
    classes: bool = False       # the issue's per-class counts are asked of this case
    unshaded: bool = False      # no bounce of this case reaches the shading (recursion 0, debug geom)


CASES = [
    Case("MATERIALS", _materials_text(), classes=True),
    Case("MATERIALS_AIR", _materials_text(), air_ior=1.33, classes=True),
    Case("SHALLOW_2", _materials_text(recursion=2)),
    Case("SHALLOW_0", _materials_text(recursion=0), unshaded=True),
    Case("DEBUG", _materials_text() + "debug geom\n", modes=("BRUTE", "BVH"), unshaded=True),
    Case("CAMERA_DOF", _materials_text(cameras=[DOF, FRUSTUM])),
    Case("CAMERA_ORTHO", _materials_text(cameras=[ORTHO])),
    # smooth-normal triangles in a closed room: hit from behind their normal is NaN (Triangle.GetNormal)
    Case("VERTEX_NORMALS", VN_ROOM_SCENE, tile=(16, 12, 32, 24), modes=("BRUTE", "BVH")),
    Case("bounce.txt", shipped="bounce.txt", size=(128, 128), tile=(70, 60, 13, 11), seed=5, spp=5, modes=("BRUTE", "BVH")),
    Case("die.txt", shipped="die.txt", size=(1280, 960), tile=(420, 500, 32, 24), seed=5, modes=("BRUTE", "BVH")),
]
CASE = {c.name: c for c in CASES}

# what the host test asks of the oracle's own non-excluded bounces; the GPU test asks half
CLASS_MIN = {"transmit_outside": 200, "transmit_inside": 200, "tir": 50, "specular_fail": 50, "emission": 50,
             "pure_black": 20, "diffuse_off_z": 200, "out_at_3": 100, "out_at_6": 100, "out_at_9": 100,
             **{f"shininess_{s:g}": 100 for s in SHININESS}}


def parse(rc, case):
    """The case's scene in ABI form (edited where the text cannot say it)."""
    text = case.text or open(rc.scene_path(case.shipped)).read()
    scene = rc.SceneLoader.from_text(text)
    if case.air_ior:
        scene.params.air_ior = case.air_ior
    return scene


def oracle_of(rc, case, scene):
    from oracle.oracle import OracleScene

    params = rc.rt_scene_params.from_buffer_copy(scene.params)
    params.width, params.height = case.size
    orc = OracleScene.from_abi(params, list(scene.prims), list(scene.cameras))
    orc.select_camera(0)
    return orc


# ---------------------------------------------------------------- paths
@dataclass
class Paths:
    """S samples of at most `per` bounces.  Per sample: pixel index in the frame, sample index, number of
    records n, colour.  Per record [S, per]: type, prim, inside, direction, normal, position, tint (before
    the bounce), and where the source has them origin, cos_in and fresnel (else None)."""
    pixel: np.ndarray
    sample: np.ndarray
    xy: np.ndarray
    n: np.ndarray
    color: np.ndarray
    type: np.ndarray
    prim: np.ndarray
    inside: np.ndarray
    direction: np.ndarray
    normal: np.ndarray
    position: np.ndarray
    tint: np.ndarray
    origin: np.ndarray = None
    cos_in: np.ndarray = None
    fresnel: np.ndarray = None


def _keys(case):
    x0, y0, w, h = case.tile
    x, y, k = np.meshgrid(np.arange(x0, x0 + w), np.arange(y0, y0 + h), np.arange(case.spp), indexing="ij")
    x, y, k = x.reshape(-1), y.reshape(-1), k.reshape(-1)
    return np.stack([x, y], 1), (y * case.size[0] + x).astype(np.uint64), k.astype(np.uint64)


def paths_of_records(case, rec, n, col):
    """rt_trace_paths' output ([w, h, spp, per] records) as Paths, widened to fp64."""
    xy, pixel, sample = _keys(case)
    per = rec.shape[-1]
    r = rec.reshape(-1, per)
    f8 = lambda a: a.astype(np.float64)
    return Paths(pixel, sample, xy, n.reshape(-1).astype(np.int64), col.reshape(-1, 3), r["type"].astype(np.int64),
                 r["prim_id"].astype(np.int64), r["inside"].astype(np.int64), f8(r["direction"]), f8(r["normal"]),
                 f8(r["position"]), f8(r["tint"]), f8(r["origin"]), f8(r["cos_in"]), f8(r["fresnel"]))


def paths_of_oracle(case, orc, recursion):
    """The oracle's own samples of the case's tile (orc_sample_path) as Paths."""
    xy, pixel, sample = _keys(case)
    S, per = len(pixel), recursion + 1
    p = Paths(pixel, sample, xy, np.zeros(S, np.int64), np.zeros((S, 3)), np.zeros((S, per), np.int64),
              np.full((S, per), -1, np.int64), np.zeros((S, per), np.int64), np.zeros((S, per, 3)),
              np.zeros((S, per, 3)), np.zeros((S, per, 3)), np.zeros((S, per, 3)))
    for i in range(S):
        c, rows = orc.sample_path(int(xy[i, 0]), int(xy[i, 1]), seed=case.seed, sample=int(sample[i]), recursion=recursion)
        k = len(rows["prim"])
        p.n[i], p.color[i] = k, c
        p.type[i, :k], p.prim[i, :k], p.inside[i, :k] = rows["type"], rows["prim"], rows["inside"]
        p.direction[i, :k], p.normal[i, :k], p.position[i, :k], p.tint[i, :k] = (rows["direction"], rows["normal"],
                                                                                 rows["position"], rows["tint"])
    return p


def draws_of(types, shin_inf):
    """The draws a bounce of this recorded type consumed: (0 if shininess is +inf, else 1) + 1, + 1 if
    total > 0 (every shaded type but PURE_BLACK), + 2 if DIFFUSE; none for MISSED, DEBUG,
    RECURSION_COMPLETE and the empty records past a path's end."""
    shaded = np.isin(types, SHADED)
    d = np.where(shin_inf, 1, 2) + (types != PURE_BLACK) + 2 * (types == DIFFUSE)
    return np.where(shaded, d, 0)


def _materials(scene):
    lum = lambda c: np.array([c.r, c.g, c.b])
    P = scene.prims
    shin = np.array([p.shininess for p in P])
    refl = shin > 0  # Primitive.IsReflective
    emission = np.array([lum(p.emission) for p in P]).reshape(-1, 3)
    debug = np.array([lum(p.emission) + lum(p.diffuse) + (lum(p.specular) if r else 0) for p, r in zip(P, refl)])
    return shin, emission, debug.reshape(-1, 3)


def _rel(a, b):
    """|a - b| / |b| componentwise, 0 where both are 0 and inf where only b is."""
    with np.errstate(divide="ignore", invalid="ignore"):
        e = np.abs(a - b) / np.abs(b)
    return np.where(b == 0, np.where(a == 0, 0.0, np.inf), e)


def _max(a):
    a = np.asarray(a)
    return float(a.max()) if a.size else 0.0


def compare(case, scene, orc, p, threshold):
    """Every record of `p` against the oracle's bounce step on the record's own inputs.  Returns a dict:
    the largest errors (`err`), the bounces compared and excluded, type mismatches outside the
    exclusion, the Fresnel counts, the class counts over the bounces not excluded, and whether the
    draw accounting held."""
    S, per = p.type.shape
    shin, emission, debug_sum = _materials(scene)
    ambient = np.array([scene.params.ambient.r, scene.params.ambient.g, scene.params.ambient.b])
    idx = np.arange(per)[None, :]
    live = idx < p.n[:, None]
    prim0 = np.where(p.prim >= 0, p.prim, 0)
    out = {"err": {}, "samples": S}

    # 1. the camera ray of every sample, and the draws it took
    cam_o, cam_d, cam_n = np.zeros((S, 3)), np.zeros((S, 3)), np.zeros(S, np.int64)
    for i in range(S):
        cam_o[i], cam_d[i], cam_n[i] = orc.camera_sample_ray(int(p.xy[i, 0]), int(p.xy[i, 1]), seed=case.seed,
                                                            sample=int(p.sample[i]))
    out["camera_draws"] = sorted(set(cam_n.tolist()))
    out["err"]["camera_direction"] = _max(np.abs(p.direction[:, 0] - cam_d))
    if p.origin is not None:
        out["err"]["camera_origin"] = _max(np.abs(p.origin[:, 0] - cam_o))

    # 3. the draw cursor of every record, advanced by the recorded types
    d = draws_of(np.where(live, p.type, 0), np.isposinf(shin[prim0]))
    cursor = cam_n[:, None] + np.cumsum(d, axis=1) - d

    # 2. the bounce step on every shaded record
    shaded = live & np.isin(p.type, SHADED)
    si, bi = np.nonzero(shaded)
    st = orc.shade_steps(p.direction[si, bi], p.normal[si, bi], p.position[si, bi], p.inside[si, bi], p.prim[si, bi], bi,
                         case.seed, p.pixel[si], p.sample[si], cursor[si, bi])
    typ = p.type[si, bi]
    finite = np.isfinite(p.normal[si, bi]).all(axis=1)
    excluded = (st["margins"] < threshold).any(axis=1)
    same = st["type"] == typ
    keep = finite & ~excluded
    out["shaded"], out["nan_normals"] = int(finite.sum()), int((~finite).sum())
    out["excluded"] = int((finite & excluded).sum())
    out["compared"] = int(keep.sum())
    out["type_mismatch"] = int((keep & ~same).sum())
    out["type_mismatch_excluded"] = int((finite & excluded & ~same).sum())
    out["type_mismatch_nan"] = int((~finite & ~excluded & ~same).sum())
    bad = np.flatnonzero(keep & ~same)[:5]
    out["first_mismatches"] = [(int(si[j]), int(bi[j]), int(p.prim[si[j], bi[j]]), int(typ[j]), int(st["type"][j]),
                                st["margins"][j].tolist()) for j in bad]
    ok = keep & same
    out["draws_agree"] = bool((st["draws"][ok] == d[si, bi][ok]).all())
    if p.cos_in is not None:
        out["err"]["cos_in"] = _max(np.abs(p.cos_in[si, bi] - st["cos"])[finite])
        # Fresnel: NaN where the block is not reached, exactly 1 on total internal reflection; the ratio is
        # left out where sin_out > 0.995 (sqrt(1 - sin^2) loses fp32 digits there)
        f, of = p.fresnel[si, bi], st["fresnel"]
        out["fresnel_nan_mismatch"] = int((ok & (np.isnan(f) != np.isnan(of))).sum())
        out["fresnel_tir_mismatch"] = int((ok & ((f == 1) != (of == 1))).sum())
        ratio = ok & np.isfinite(of) & (of < 1) & np.isfinite(f)
        steep = ratio & (1 - st["margins"][:, 1] > 0.995)
        out["fresnel_kept"], out["fresnel_left_out"] = int((ratio & ~steep).sum()), int(steep.sum())
        out["err"]["fresnel"] = _max(np.abs(f - of)[ratio & ~steep])
    # the ray and the tint that the bounce made: record i + 1
    go = ok & np.isin(typ, CONTINUES)
    nb = np.minimum(bi + 1, per - 1)
    out["next_missing"] = int((go & (bi + 1 >= p.n[si])).sum())
    out["err"]["direction"] = _max(np.abs(p.direction[si, nb] - st["direction"])[go].max(axis=1)) if go.any() else 0.0
    # ... and its length on its own, apart for the rays that are renormalised (the next bounce index is a
    # multiple of 3: the step's vector has length 1 there, and the kernel's only the rounding of its
    # normalisation) and for the rays that are kept as they are (both carry the same drift of a few 1e-6).
    # A kernel on another cadence reaches bounces 3, 6, 9 with the drift and shows in the first figure.
    length = lambda v: np.sqrt((v * v).sum(axis=1))
    dl = np.abs(length(p.direction[si, nb]) - length(st["direction"]))
    renorm = (bi + 1) % 3 == 0
    out["err"]["length_renormalised"] = _max(dl[go & renorm])
    out["err"]["length_kept"] = _max(dl[go & ~renorm])
    if p.origin is not None:  # the next ray starts at the step's origin: the hit position, bit for bit
        out["origin_mismatch"] = int((p.origin[si, nb] != st["origin"]).any(axis=1)[go].sum())
    out["err"]["tint"] = _max(_rel(p.tint[si, nb], p.tint[si, bi] * st["factor"])[go])

    # 4. the ending, from the last record of every sample
    last = p.n - 1
    rows = np.arange(S)
    lt, lp = p.type[rows, last], prim0[rows, last]
    want = p.tint[rows, last] * emission[lp]
    want = np.where((lt == DEBUG)[:, None], debug_sum[lp], want)
    want = np.where((lt == MISSED)[:, None], ambient[None, :], want)  # untinted (GetColor returns Scene.Ambient)
    want = np.where(((lt == MISSED) & (last == 0))[:, None], -1.0, want)
    out["end_types"] = {int(t): int((lt == t).sum()) for t in np.unique(lt)}
    out["bad_end_type"] = int(np.isin(lt, CONTINUES).sum())
    out["err"]["colour"] = _max(np.abs(p.color - want) / np.maximum(1.0, np.abs(want)))

    # the classes, over the bounces that were compared
    nrm, ins = p.normal[si, bi], p.inside[si, bi]
    on_z = (nrm[:, 0] == 0) & (nrm[:, 1] == 0) & (np.abs(nrm[:, 2]) == 1)
    cls = {"transmit_outside": (typ == TRANSMITTED) & (ins == 0), "transmit_inside": (typ == TRANSMITTED) & (ins != 0),
           "tir": st["fresnel"] == 1, "specular_fail": typ == SPECULAR_FAIL, "emission": typ == EMISSION,
           "pure_black": typ == PURE_BLACK, "diffuse_off_z": (typ == DIFFUSE) & on_z}
    for b in (3, 6, 9):
        cls[f"out_at_{b}"] = np.isin(typ, CONTINUES) & (bi + 1 == b)
    ps = shin[p.prim[si, bi]]
    for s in SHININESS:
        cls[f"shininess_{s:g}"] = ps == s
    out["classes"] = {k: int((v & ok).sum()) for k, v in cls.items()}
    return out
