"""Adaptive light probes: include/rtcore.h's "adaptive light probes" restated in numpy (every numpy operation is
one rounding, in the header's order), and the inputs the host and the GPU tests share."""
import numpy as np

from test_render_probes_host import K0, K1, basis

PI = 3.141592653589793
A1 = 2.0943951023931953


def luminance(r, g, b):
    """(0.299 r + 0.587 g) + 0.114 b, left to right, fp64."""
    r, g, b = (np.asarray(v, np.float64) for v in (r, g, b))
    return (0.299 * r + 0.587 * g) + 0.114 * b


def moments_replay(rays, rgb, miss, out=None):
    """"The moments (normative)", sample by sample: rays (n, spp) RAY_DTYPE, rgb (n, spp, 3) fp32 values, miss
    (n, spp) bool -> moments [n, 4, 2], added to `out`."""
    n, spp = rays.shape
    m = out if out is not None else np.zeros((n, 4, 2))
    d = rays["direction"][..., :3]
    Y = basis(d)[..., :4]
    col = np.asarray(rgb, np.float32).astype(np.float64)
    y = luminance(col[..., 0], col[..., 1], col[..., 2])
    dead = ~d.any(axis=2)
    miss = np.asarray(miss) != 0
    for k in range(spp):
        hit = ~dead[:, k] & ~miss[:, k]
        sky = ~dead[:, k] & miss[:, k]
        x = y[hit, k][:, None] * Y[hit, k]
        m[hit, :, 0] = m[hit, :, 0] + x * x
        m[sky, :, 1] = m[sky, :, 1] + Y[sky, k] * Y[sky, k]
    return m


def rule_replay(par, sh, samples, misses, moments, with_v=False):
    """"The rule (normative)": (active bool [n], se [n], level [n]); se and level NaN where N < 2.  with_v: the
    variances v [n, 4] instead."""
    c = np.asarray(sh, np.float64)
    m = np.asarray(moments, np.float64)
    N = np.asarray(samples, np.uint32).astype(np.uint64) + np.asarray(misses, np.uint32).astype(np.uint64)
    n = N.astype(np.float64)
    A = luminance(par.ambient.r, par.ambient.g, par.ambient.b)
    AA = A * A
    with np.errstate(all="ignore"):
        S = luminance(c[:, :4, 0], c[:, :4, 1], c[:, :4, 2]) + A * c[:, :4, 3]
        T = m[:, :, 0] + AA * m[:, :, 1]
        num = T - (S * S) / n[:, None]
        d = num / (n[:, None] - 1.0)
        v = np.where(num > (n[:, None] * 2.0 ** -49) * T, d, 0.0)
        a0, a1, p4 = PI * K0, A1 * K1, 4.0 * PI
        level = ((p4 * a0) * S[:, 0]) / n
        se = p4 * np.sqrt(((a0 * a0) * v[:, 0] + (a1 * a1) * ((v[:, 1] + v[:, 2]) + v[:, 3])) / n)
        lv = np.where(level > par.irr_floor, level, par.irr_floor)
        step4 = ~np.isnan(d).any(axis=1) & (se > par.rel_tol * lv)
    active = np.where(N < par.min_samples, True, np.where(N >= par.max_samples, False, np.where(N < 2, True, step4)))
    few = N < 2
    if with_v:
        return v
    return active, np.where(few, np.nan, se), np.where(few, np.nan, level)


def moments_case(rc, n=70, spp=37, seed=29):
    """H2's inputs: random unit fp32 directions, random fp32 colours, about 30 % misses, two probes of all-zero
    rays."""
    rng = np.random.default_rng(seed)
    rays = np.zeros((n, spp), rc.RAY_DTYPE)
    g = rng.normal(size=(n, spp, 3))
    g = (g / np.linalg.norm(g, axis=2, keepdims=True)).astype(np.float32).astype(np.float64)
    rays["direction"][..., :3] = g
    rays["origin"][..., :3] = rng.normal(size=(n, spp, 3))
    rays["origin"][..., 3] = 1.0
    rays[3] = np.zeros((), rays.dtype)
    rays[n - 2] = np.zeros((), rays.dtype)
    rgb = rng.uniform(0.0, 2.0, (n, spp, 3)).astype(np.float32)
    miss = rng.uniform(size=(n, spp)) < 0.3
    return rays, rgb, miss


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()
