"""The moments fold of rt_render_list (rtcore.h, "indexed radiance queries") restated in numpy, for the
tests of tests/test_render_list_gpu.py; tests/test_render_list_host.py holds it to pixel_standard_error."""
import numpy as np


def lum(c):
    """DoubleColor.GetLuminance in fp64, left to right, every operation rounded on its own (numpy fuses nothing)."""
    return (0.299 * c[..., 0] + 0.587 * c[..., 1]) + 0.114 * c[..., 2]


def fold_moments(item_sums, item_counts):
    """The header's rule over one call.  item_sums [J, n, 3]: each work item's colour sums (a miss adds
    nothing); item_counts [J, n]: its finished samples t_j, misses included.  Returns (q [n], batches [n]):
    q the sum, in item order from zero, of Y_j * Y_j / t_j over the items with t_j > 0, batches their number."""
    item_sums = np.asarray(item_sums, np.float64)
    item_counts = np.asarray(item_counts)
    q = np.zeros(item_sums.shape[1])
    batches = np.zeros(item_sums.shape[1], np.uint32)
    for c, t in zip(item_sums, item_counts):
        y = lum(c)
        on = t > 0
        q = np.where(on, q + y * y / np.where(on, t, 1), q)
        batches += on.astype(np.uint32)
    return q, batches


def standard_error(sum_rgb, samples, misses, q, batches):
    """The header's estimate, entry by entry in plain Python floats: se = sqrt(s2 / N), s2 = max(0, (Q - Y Y /
    N) / (J - 1)) for J >= 2, inf below."""
    out = np.full(len(q), np.inf)
    for e in range(len(q)):
        n = float(samples[e]) + float(misses[e])
        if batches[e] >= 2:
            y = float(lum(np.asarray(sum_rgb[e], np.float64)))
            s2 = max(0.0, (float(q[e]) - y * y / n) / (float(batches[e]) - 1.0))
            out[e] = np.sqrt(s2 / n)
    return out


def per_item(single_sums, single_hits, s):
    """From per-sample results (single_sums [K, n, 3] fp64, zero on a miss; single_hits [K, n] 0 / 1) and s
    samples per item: the items' fp64 colour sums [J, n, 3], their magnitude sums, and their counts t_j
    (every sample finishes, hit or miss)."""
    K = single_sums.shape[0]
    sums = np.stack([single_sums[j:j + s].sum(axis=0) for j in range(0, K, s)])
    mags = np.stack([np.abs(single_sums[j:j + s]).sum(axis=0) for j in range(0, K, s)])
    counts = np.stack([np.full(single_sums.shape[1], min(s, K - j)) for j in range(0, K, s)])
    return sums, mags, counts
