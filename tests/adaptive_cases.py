"""Synthetic accumulators for the selection pass of adaptive sampling (rt_adaptive_select_device and its
host twin), shared by tests/test_adaptive_host.py and tests/test_adaptive_gpu.py, and a numpy
restatement of the rule and of the list order (include/rtcore.h, "adaptive sampling")."""
import numpy as np

REL_TOL, LUM_FLOOR, MIN_SAMPLES, MAX_SAMPLES = 0.05, 1e-2, 16, 256
FRAMES = ((8, 8), (13, 7), (128, 128))
# what a pixel was drawn to show; the last five reach the rule's fourth step
KINDS = ("below_min", "at_max", "one_batch", "noisy", "converged", "dark_noisy", "all_miss", "nan_sum", "nan_q")


def make_accumulators(width, height, seed, plane=0):
    """Accumulators in the device layout (sum: three planes `plane` doubles apart, 0 = width * height; the
    others row-major) whose pixels cover every branch of the rule, and each pixel's kind.  A pixel that
    reaches the fourth step is drawn with its standard error at 0.5, 0.9, 1.1 or 2 times the threshold,
    so that none lies at it."""
    rng = np.random.default_rng(seed)
    npix = width * height
    pl = plane or npix
    kind = rng.integers(0, len(KINDS), npix)
    kind[:len(KINDS)] = np.arange(len(KINDS))[:npix]  # every kind at least once (8 x 8 and up)
    kind = rng.permutation(kind)
    N = rng.integers(MIN_SAMPLES, MAX_SAMPLES, npix)
    N = np.where(kind == 0, rng.integers(0, MIN_SAMPLES, npix), N)
    N = np.where(kind == 1, rng.integers(MAX_SAMPLES, 4 * MAX_SAMPLES, npix), N)
    J = np.minimum(N, rng.integers(2, 40, npix))
    J = np.where(kind == 2, rng.integers(0, 2, npix), J)
    mean = rng.uniform(0.05, 2.0, npix)
    mean = np.where(kind == 5, rng.uniform(1e-4, 5e-3, npix), mean)  # below the luminance floor
    mean = np.where(kind == 6, 0.0, mean)
    misses = np.where(kind == 6, N, rng.integers(0, 3, npix).clip(max=N))
    tint = rng.uniform(0.2, 1.0, (3, npix))
    tint /= (0.299 * tint[0] + 0.587 * tint[1] + 0.114 * tint[2])  # luminance 1
    s = tint * (mean * N)
    Y = 0.299 * s[0] + 0.587 * s[1] + 0.114 * s[2]
    factor = rng.choice([0.5, 0.9, 1.1, 2.0], npix)
    factor = np.where(kind == 3, rng.choice([1.1, 2.0], npix), factor)
    factor = np.where(kind == 4, rng.choice([0.5, 0.9], npix), factor)
    factor = np.where(kind == 5, 2.0, factor)
    n = np.maximum(N, 1).astype(np.float64)
    se = factor * REL_TOL * np.maximum(Y / n, LUM_FLOOR)
    q = se * se * n * np.maximum(J - 1, 1) + Y * Y / n
    q = np.where(kind == 6, 0.0, q)
    q = np.where(kind == 8, np.nan, q)
    s[:, kind == 7] = np.nan
    sums = np.zeros(2 * pl + npix if plane else 3 * npix)
    for c in range(3):
        sums[c * pl:c * pl + npix] = s[c]
    return {"sum": sums, "samples": (N - misses).astype(np.uint32), "misses": misses.astype(np.uint32), "q": q,
            "batches": J.astype(np.uint32), "plane": plane, "kind": kind, "width": width, "height": height}


def rule(acc, rel_tol=REL_TOL, lum_floor=LUM_FLOOR, min_samples=MIN_SAMPLES, max_samples=MAX_SAMPLES):
    """active(N, Y, Q, J) per pixel in numpy, step by step as the header states it, and for the pixels
    that reach the fourth step the ratio of the standard error to the threshold."""
    npix = acc["width"] * acc["height"]
    pl = acc["plane"] or npix
    s = acc["sum"]
    N = acc["samples"].astype(np.int64) + acc["misses"].astype(np.int64)
    J = acc["batches"].astype(np.int64)
    with np.errstate(all="ignore"):
        n = N.astype(np.float64)
        Y = 0.299 * s[:npix] + 0.587 * s[pl:pl + npix] + 0.114 * s[2 * pl:2 * pl + npix]
        d = (acc["q"] - Y * Y / n) / (J - 1).astype(np.float64)
        var = np.where(d > 0.0, d, 0.0)
        mean = Y / n
        level = np.where(mean > lum_floor, mean, lum_floor)
        se = np.sqrt(var / n)
        fourth = se > rel_tol * level
        ratio = se / (rel_tol * level)
    active = np.select([N < min_samples, N >= max_samples, J < 2], [True, False, True], fourth)
    reaches = (N >= min_samples) & (N < max_samples) & (J >= 2)
    return active, reaches, ratio


def list_order(active, width, height):
    """The active pixels' frame indices in the normative order: by 8 x 8 block, blocks row-major, within
    a block by (y & 7) * 8 + (x & 7)."""
    y, x = np.divmod(np.arange(width * height), width)
    key = ((y >> 3) * ((width + 7) // 8) + (x >> 3)) * 64 + (y & 7) * 8 + (x & 7)
    idx = np.flatnonzero(active)
    return idx[np.argsort(key[idx], kind="stable")].astype(np.uint32)
