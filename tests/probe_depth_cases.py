"""Probe depth maps: include/rtcore.h's "probe depth maps" restated in plain Python loops, one rounding per
operation and in the stated order (Python floats are IEEE doubles), and the inputs the host and the GPU tests
share.  Nothing here touches a device."""
import math

import numpy as np

A_LOBE = [3.141592653589793] + [2.0943951023931953] * 3 + [0.7853981633974483] * 5
K0, K1, K2, K3, K4 = 0.28209479177387814, 0.48860251190291992, 1.0925484305920792, 0.31539156525252005, 0.54627421529603959


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def sgn(a):
    return 1.0 if a >= 0.0 else -1.0


def replay_texel_dir(t):
    tx, ty = t & 7, t >> 3
    u = float(2 * tx + 1) / 8.0 - 1.0
    v = float(2 * ty + 1) / 8.0 - 1.0
    z = (1.0 - abs(u)) - abs(v)
    x, y = u, v
    if z < 0.0:
        x = (1.0 - abs(v)) * sgn(u)
        y = (1.0 - abs(u)) * sgn(v)
    ln = math.sqrt((x * x + y * y) + z * z)
    return x / ln, y / ln, z / ln


def _coord(u):
    return min(max(int((u + 1.0) * 4.0), 0), 7)


def replay_texel(x, y, z):
    s1 = (abs(x) + abs(y)) + abs(z)
    u, v = x / s1, y / s1
    if z < 0.0:
        u, v = (1.0 - abs(v)) * sgn(x), (1.0 - abs(u)) * sgn(y)
    return _coord(v) * 8 + _coord(u)


def replay_fold(d_max, sharpness, rays, hits, depth, counts):
    """The bake's accumulation, added into depth (n, 3, 64) and counts (n, 4) in place; rays (n, spp) RAY_DTYPE,
    hits (n, spp) HIT_DTYPE."""
    T = [replay_texel_dir(t) for t in range(64)]
    for i in range(rays.shape[0]):
        s = [[float(v) for v in row] for row in depth[i]]
        c = [int(v) for v in counts[i]]
        for k in range(rays.shape[1]):
            x, y, z = (float(v) for v in rays[i, k]["direction"][:3])
            if x == 0.0 and y == 0.0 and z == 0.0:
                c[3] += 1
                continue
            hit = int(hits[i, k]["prim_id"]) >= 0
            dist = float(hits[i, k]["distance"])
            d = dist if hit and dist < d_max else d_max
            if hit:
                c[0] += 1
                c[1] += 1 if int(hits[i, k]["inside"]) != 0 else 0
            else:
                c[2] += 1
            for t in range(64):
                cs = (x * T[t][0] + y * T[t][1]) + z * T[t][2]
                if not cs > 0.0:
                    continue
                w = cs
                for _ in range(sharpness):
                    w = w * w
                wd = w * d
                s[0][t] = s[0][t] + w
                s[1][t] = s[1][t] + wd
                s[2][t] = s[2][t] + wd * d
        depth[i] = s
        counts[i] = c


def replay_close(depth):
    D = np.full((depth.shape[0], 64, 2), np.nan)
    for i in range(depth.shape[0]):
        for t in range(64):
            s0, s1, s2 = (float(depth[i, r, t]) for r in range(3))
            if s0 > 0.0:
                D[i, t] = (s1 / s0, s2 / s0)
    return D


def replay_cell(origin, step, dims, p, n):
    """rtcore.h, "probe grids": None for an invalid point, else (n^, i, t[8])."""
    vals = [float(v) for v in p] + [1.0] + [float(v) for v in n] + [0.0]
    n2 = (vals[4] * vals[4] + vals[5] * vals[5]) + vals[6] * vals[6]
    if not all(math.isfinite(v) for v in vals) or n2 == 0.0 or not math.isfinite(n2):
        return None
    ln = math.sqrt(n2)
    nh = [vals[4] / ln, vals[5] / ln, vals[6] / ln]
    i, f = [0, 0, 0], [0.0, 0.0, 0.0]
    for a in range(3):
        if dims[a] == 1:
            continue
        g = (vals[a] - origin[a]) / step[a]
        g = 0.0 if g < 0.0 else float(dims[a] - 1) if g > dims[a] - 1 else g
        i[a] = min(int(g), dims[a] - 2)
        f[a] = g - float(i[a])
    t = []
    for c in range(8):
        w = [f[a] if (c >> a) & 1 else 1.0 - f[a] for a in range(3)]
        t.append((w[0] * w[1]) * w[2])
    return nh, i, t


def replay_basis(x, y, z):
    return [K0, K1 * y, K1 * z, K1 * x, (K2 * x) * y, (K2 * y) * z, K3 * ((3.0 * z) * z + -1.0), (K2 * x) * z,
            K4 * (x * x + -(y * y))]


def replay_corner(d_max, var_floor, wrap, Dp, v, nh):
    """(c, wrap) of one visited corner: v = o - q, Dp the probe's (64, 2) moments, nh the unit normal."""
    r = math.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
    if not r > 0.0 or not math.isfinite(r):
        return 1.0, 1.0
    mu, m2 = (float(x) for x in Dp[replay_texel(v[0], v[1], v[2])])
    rc_ = r if r < d_max else d_max
    c = 1.0
    if math.isfinite(mu) and math.isfinite(m2) and rc_ > mu:
        var = m2 - mu * mu
        var = var if var > var_floor else var_floor
        delta = rc_ - mu
        q = var / (var + delta * delta)
        c = (q * q) * q
    w = 1.0
    if wrap:
        h = (1.0 - ((v[0] * nh[0] + v[1] * nh[1]) + v[2] * nh[2]) / r) * 0.5
        w = h * h + 0.2
    return c, w


def replay_shade(origin, step, dims, bias, d_max, var_floor, wrap, L, D, pos, nrm):
    """rtcore.h, "The shading": (irradiance (n, 3), weight (n,)); L (n_probes, 9, 3), D (n_probes, 64, 2)."""
    n = len(pos)
    E, Wout = np.zeros((n, 3)), np.zeros(n)
    Lp = np.asarray(L, np.float64).reshape(-1, 27)
    Dp = np.asarray(D, np.float64).reshape(-1, 64, 2)
    for k in range(n):
        cell = replay_cell(origin, step, dims, pos[k], nrm[k])
        if cell is None:
            continue
        nh, i, t = cell
        o = [float(pos[k][a]) + bias * nh[a] for a in range(3)]
        W, B = 0.0, [0.0] * 27
        for c in range(8):
            if t[c] == 0.0:
                continue
            ix, iy, iz = (i[a] + ((c >> a) & 1) for a in range(3))
            probe = (iz * dims[1] + iy) * dims[0] + ix
            row = [float(v) for v in Lp[probe]]
            if not all(math.isfinite(v) for v in row):
                continue
            q = [origin[a] + float(i[a] + ((c >> a) & 1)) * step[a] for a in range(3)]
            v = [o[a] - q[a] for a in range(3)]
            cheb, wr = replay_corner(d_max, var_floor, wrap, Dp[probe], v, nh)
            tp = (t[c] * cheb) * wr
            if not tp > 0.0:
                continue
            W = W + tp
            for j in range(27):
                B[j] = B[j] + tp * row[j]
        if not W > 0.0:
            continue
        Y = replay_basis(*nh)
        a = [A_LOBE[l] * Y[l] for l in range(9)]
        for ch in range(3):
            e = a[0] * B[ch]
            for l in range(1, 9):
                e = e + a[l] * B[3 * l + ch]
            E[k, ch] = e / W
        Wout[k] = W
    return E, Wout


def random_D(n_probes, seed=23, absent_share=0.15, lo=0.1, hi=1.7):
    """Random moments (n_probes, 64, 2): mean distances in [lo, hi), variances from a little below zero (the
    floor's case) to 0.2, and a share of absent texels (both values NaN)."""
    rng = np.random.default_rng(seed)
    mu = rng.uniform(lo, hi, (n_probes, 64))
    m2 = mu * mu + rng.uniform(-0.01, 0.2, (n_probes, 64))
    D = np.stack([mu, m2], axis=-1)
    D[rng.random((n_probes, 64)) < absent_share] = np.nan
    return D


def synthetic_samples(rc, n=3, spp=5, seed=31, d_max=1.5):
    """The host fold's inputs: unit fp32 directions widened, hits with distances on both sides of d_max; and the
    cases the issue names, each at a fixed place: a miss (0, 1), distance > d_max (0, 2), a zero direction
    (1, 0), an inside hit (1, 3), a NaN distance taken as d_max (2, 4)."""
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n, spp, 3))
    d = (d / np.linalg.norm(d, axis=-1, keepdims=True)).astype(np.float32).astype(np.float64)
    rays = np.zeros((n, spp), rc.RAY_DTYPE)
    rays["origin"][..., 3] = 1.0
    rays["direction"][..., :3] = d
    hits = np.zeros((n, spp), rc.HIT_DTYPE)
    hits["prim_id"] = rng.integers(0, 9, (n, spp))
    hits["distance"] = rng.uniform(0.1, 0.9 * d_max, (n, spp))
    hits["prim_id"][0, 1] = -1
    hits["distance"][0, 1] = 0.0
    hits["distance"][0, 2] = 2.5 * d_max
    rays["direction"][1, 0] = 0.0
    rays["origin"][1, 0] = 0.0
    hits["inside"][1, 3] = 1
    hits["distance"][2, 4] = np.nan
    return rays, hits
