"""Obscurance at surfels: include/rtcore.h's "obscurance at surfels" restated in plain Python loops, one rounding
per operation and in the stated order (Python floats are IEEE doubles), and the inputs the host and the GPU tests
share.  Nothing here touches a device."""
import math

import numpy as np


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def replay_weight(prim_id, distance, radius, power):
    """(w, in) of one sample."""
    inside = prim_id >= 0 and distance < radius  # (False for a NaN distance)
    if not inside:
        return 0.0, False
    if power == 0:
        return 1.0, True
    b = 1.0 - distance / radius
    b = 0.0 if b < 0.0 else 1.0 if b > 1.0 else b
    w = b
    for _ in range(power - 1):
        w = w * b
    return w, True


def replay_fold(radius, power, rays, hits, acc):
    """The accumulation, added into acc (n,) OBSCURANCE_DTYPE in place; rays (n, spp) RAY_DTYPE, hits (n, spp)
    HIT_DTYPE."""
    for i in range(rays.shape[0]):
        o, o2 = float(acc[i]["o"]), float(acc[i]["o2"])
        bent = [float(v) for v in acc[i]["bent"]]
        samples, nhits = int(acc[i]["samples"]), int(acc[i]["hits"])
        for k in range(rays.shape[1]):
            d = [float(v) for v in rays[i, k]["direction"][:3]]
            samples += 1
            if d[0] == 0.0 and d[1] == 0.0 and d[2] == 0.0:
                continue
            w, inside = replay_weight(int(hits[i, k]["prim_id"]), float(hits[i, k]["distance"]), radius, power)
            nhits += 1 if inside else 0
            o = o + w
            o2 = o2 + w * w
            v = 1.0 - w
            for a in range(3):
                bent[a] = bent[a] + v * d[a]
        acc[i]["o"], acc[i]["o2"], acc[i]["bent"] = o, o2, bent
        acc[i]["samples"], acc[i]["hits"] = samples & 0xFFFFFFFF, nhits & 0xFFFFFFFF


def _div(a, b):
    """IEEE division of two doubles (Python raises where IEEE gives an infinity or a NaN)."""
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


def _sqrt(a):
    with np.errstate(all="ignore"):
        return float(np.sqrt(np.float64(a)))


def replay_error(o, o2, N):
    """(se, d is not a NaN) of the rule's steps 4 and 5 for N >= 2."""
    n = float(N)
    u = o2 - _div(o * o, n)
    d = _div(u, n - 1.0)
    v = d if u > (n * 2.0 ** -49) * o2 else 0.0
    return _sqrt(_div(v, n)), d == d


def replay_active(tol, min_samples, max_samples, o, o2, N):
    if N < min_samples:
        return True
    if N >= max_samples:
        return False
    if N < 2:
        return True
    se, ok = replay_error(o, o2, N)
    return ok and se > tol


def replay_select(tol, min_samples, max_samples, acc):
    return [e for e in range(len(acc))
            if replay_active(tol, min_samples, max_samples, float(acc[e]["o"]), float(acc[e]["o2"]), int(acc[e]["samples"]))]


def synthetic_samples(rc, radius=1.5, seed=31):
    """The host fold's inputs, 3 entries x 6 samples: unit fp32 directions widened, hits with distances on both
    sides of the radius; and the cases the definition names, each at a fixed place: a miss (0, 1), a distance
    exactly at the radius (0, 2), one just inside it (0, 3), a zero direction (1, 0), a NaN distance (2, 4), and a
    hit well inside at (1, 3)."""
    n, spp = 3, 6
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n, spp, 3))
    d = (d / np.linalg.norm(d, axis=-1, keepdims=True)).astype(np.float32).astype(np.float64)
    rays = np.zeros((n, spp), rc.RAY_DTYPE)
    rays["origin"][..., 3] = 1.0
    rays["direction"][..., :3] = d
    hits = np.zeros((n, spp), rc.HIT_DTYPE)
    hits["prim_id"] = rng.integers(0, 9, (n, spp))
    hits["distance"] = rng.uniform(0.1, 1.4 * radius, (n, spp))
    hits["prim_id"][0, 1] = -1
    hits["distance"][0, 1] = 0.0
    hits["distance"][0, 2] = radius
    hits["distance"][0, 3] = np.nextafter(radius, 0.0)
    rays["direction"][1, 0] = 0.0
    rays["origin"][1, 0] = 0.0
    hits["distance"][1, 3] = 0.25 * radius
    hits["distance"][2, 4] = np.nan
    return rays, hits


def start_acc(rc, n, seed=6):
    """Non-zero accumulators to add into."""
    rng = np.random.default_rng(seed)
    acc = np.zeros(n, rc.OBSCURANCE_DTYPE)
    acc["o"] = rng.uniform(0, 3, n)
    acc["o2"] = rng.uniform(0, 2, n)
    acc["bent"] = rng.uniform(-2, 2, (n, 3))
    acc["samples"] = rng.integers(3, 9, n)
    acc["hits"] = rng.integers(0, 3, n)
    return acc


def random_acc(rc, n=400, seed=3):
    """Accumulators for the rule: sums of N weights in [0, 1] with N = 0 .. 40 (0, 1 and 2 among them), then at
    fixed places a NaN in o, a NaN in o2, constant-weight entries (all 0.3, all 1, all 0) and an infinity."""
    rng = np.random.default_rng(seed)
    acc = np.zeros(n, rc.OBSCURANCE_DTYPE)
    N = rng.integers(0, 41, n)
    N[:6] = (0, 1, 2, 2, 8, 32)
    for e in range(n):
        w = rng.uniform(0, 1, N[e]) ** rng.integers(1, 4) * (rng.random(N[e]) < rng.random())
        o = o2 = 0.0
        for x in w:
            o, o2 = o + float(x), o2 + float(x) * float(x)
        acc[e] = (o, o2, (0.0, 0.0, 0.0), N[e], int((w > 0).sum()))
    acc["o"][10] = np.nan
    acc["o2"][11] = np.nan
    acc["o"][12] = np.inf
    for e, (w, cnt) in zip((13, 14, 15, 16), ((0.3, 16), (1.0, 24), (0.0, 24), (0.7, 31))):
        o = o2 = 0.0
        for _ in range(cnt):
            o, o2 = o + w, o2 + w * w
        acc[e] = (o, o2, (0.0, 0.0, 0.0), cnt, cnt if w > 0 else 0)
    return acc
