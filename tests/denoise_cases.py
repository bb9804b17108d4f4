"""Synthetic inputs for the denoising pass (rt_denoise_device and its host twin rt_debug_denoise), shared by
tests/test_denoise_host.py and tests/test_denoise_gpu.py, and a scalar numpy restatement of the filter as
include/rtcore.h ("denoising") defines it."""
import numpy as np

FRAMES = ((8, 8), (37, 19), (130, 70))
# prim 0: a plane facing the camera; prim 1: a wall perpendicular to it; prim 2: a patch of a sphere
COLOURS = np.array([[0.8, 0.4, 0.2], [0.2, 0.5, 0.9], [0.6, 0.7, 0.3]])
PARAMS = dict(sigma_l=4.0, sigma_z=0.05, lum_eps=1e-4, normal_pow_log2=6, iterations=5, flags=0)


def luminance(rgb):
    return 0.299 * rgb[..., 0] + 0.587 * rgb[..., 1] + 0.114 * rgb[..., 2]


def bits(a):
    """An array's bytes as unsigned integers of its item size, so that NaN and -0 compare by bit pattern."""
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def make_guides(rc, width, height):
    """First hits of a synthetic frame as a HIT_DTYPE array (height, width): the plane on the left, the
    wall on the right of a vertical line, a spherical patch of varying normals in the middle, and the top
    row a background no ray hits (prim_id -1)."""
    hits = np.zeros((height, width), rc.HIT_DTYPE)
    y, x = np.mgrid[0:height, 0:width].astype(np.float64)
    u, v = (x - width / 2) * 0.02, (y - height / 2) * 0.02
    edge = (11 * width) // 20
    ue = (edge - width / 2) * 0.02
    left = x < edge
    pos = np.where(left[..., None], np.stack([u, v, np.full_like(u, 5.0)], -1), np.stack([np.full_like(u, ue), v, 5.0 - (u - ue)], -1))
    nrm = np.where(left[..., None], np.array([0.0, 0.0, -1.0]), np.array([-1.0, 0.0, 0.0]))
    prim = np.where(left, 0, 1)
    R = min(width, height) / 4
    cx, cy = width * 0.3, height * 0.55
    dx, dy = (x - cx) / R, (y - cy) / R
    r2 = dx * dx + dy * dy
    ball = r2 < 0.81
    nz = -np.sqrt(np.maximum(0.0, 1.0 - r2))
    bn = np.stack([dx, dy, nz], -1)
    bp = np.stack([(cx - width / 2) * 0.02, (cy - height / 2) * 0.02, 5.0])[None, None] + bn * (R * 0.02)
    pos = np.where(ball[..., None], bp, pos)
    nrm = np.where(ball[..., None], bn, nrm)
    prim = np.where(ball, 2, prim)
    prim[0, :] = -1
    hits["prim_id"] = prim
    hits["distance"] = np.where(prim >= 0, np.sqrt((pos * pos).sum(-1)).astype(np.float32), 0.0)
    hits["position"] = np.where((prim >= 0)[..., None], pos, 0.0)
    hits["normal"] = np.where((prim >= 0)[..., None], nrm, 0.0)
    return hits


def make_inputs(rc, width, height, seed, plane=0, spp=16):
    """A noisy render of a piecewise-constant image over make_guides: per pixel spp samples truth * m with
    m ~ Gamma(2, 1/2) (mean 1, variance 1/2) drawn with numpy, summed into accumulators in the device
    layout with one sample per batch, so q and batches are genuine moments.  The background row is all
    misses.  Three pixels of the second row are special: one has NaN in its sum, one a NaN normal (the
    quirk of rt_debug_ray.normal), one a single batch (no variance estimate).
    Returns the accumulators, the hits, the truth (height, width, 3) and which pixels are valid."""
    rng = np.random.default_rng(seed)
    npix = width * height
    pl = plane or npix
    hits = make_guides(rc, width, height)
    prim = hits["prim_id"]
    truth = COLOURS[np.maximum(prim, 0)] * (prim >= 0)[..., None]
    m = rng.gamma(2.0, 0.5, (spp, height, width))
    samples = truth[None] * m[..., None]                       # (spp, H, W, 3)
    s = samples.sum(0)
    Yj = luminance(samples)
    q = (Yj * Yj).sum(0)
    ns = np.where(prim >= 0, spp, 0).astype(np.uint32)
    nm = (spp - ns).astype(np.uint32)
    nb = np.full((height, width), spp, np.uint32)
    if height > 1 and width >= 6:
        s[1, 1, 1] = np.nan
        hits["normal"][1, 3] = np.nan
        nb[1, 5] = 1
    valid = (prim >= 0) & np.isfinite(s).all(-1)
    sums = np.zeros(2 * pl + npix)
    for c in range(3):
        sums[c * pl:c * pl + npix] = s[..., c].reshape(-1)
    acc = {"sum": sums, "samples": ns.reshape(-1), "misses": nm.reshape(-1), "q": q.reshape(-1), "batches": nb.reshape(-1),
           "plane": plane, "width": width, "height": height}
    return acc, hits, truth, valid


def run_host(rc, acc, hits, **kw):
    """denoise_host on make_inputs-style accumulators; returns (out_sum (3, H, W) view of the planes, the
    whole flat output, out_var (H, W))."""
    p = dict(PARAMS)
    p.update(kw)
    W, H = acc["width"], acc["height"]
    out, var = rc.denoise_host(rc.denoise_params(**p), acc["sum"], acc["samples"], acc["misses"], acc["q"], acc["batches"],
                               hits, W, H, plane=acc["plane"])
    return planes(out, acc), out, var


def planes(flat, acc):
    npix = acc["width"] * acc["height"]
    pl = acc["plane"] or npix
    return np.stack([flat[c * pl:c * pl + npix] for c in range(3)]).reshape(3, acc["height"], acc["width"])


def mse_luminance(sum_planes, samples, truth, mask):
    """Mean squared luminance error of sum / samples against the truth over the masked pixels."""
    n = np.maximum(samples.reshape(truth.shape[:2]), 1).astype(np.float64)
    img = np.moveaxis(sum_planes, 0, -1) / n[..., None]
    d = luminance(img) - luminance(truth)
    return float(np.mean(d[mask] ** 2))


# ---- the definition, one scalar operation at a time (np.float32 / np.float64 scalars round each result) ----

F = np.float32
H5 = [F(0.0625), F(0.25), F(0.375), F(0.25), F(0.0625)]
K3 = [F(0.25), F(0.5), F(0.25)]


def _f(t):
    return F(1) / (F(1) + t + F(0.5) * t * t) if t >= 0 else F(0)


def _wn(p, gp, gq):
    if (p["flags"] & 1) and gq["prim"] != gp["prim"]:
        return F(0)
    a, b = gp["n"], gq["n"]
    dot = a[0] * b[0] + a[1] * b[1] + a[2] * b[2]
    m = dot if dot > 0 else F(0)
    for _ in range(p["normal_pow_log2"]):
        m = m * m
    return m


def _lum(c):
    return F(0.299) * c[0] + F(0.587) * c[1] + F(0.114) * c[2]


def restate(acc, hits, **kw):
    """The filter in scalar numpy, written from the header alone: returns (out_sum (3, H, W), out_var (H, W))."""
    p = dict(PARAMS)
    p.update(kw)
    W, H = acc["width"], acc["height"]
    npix = W * H
    pl = acc["plane"] or npix
    s, hits = acc["sum"], hits.reshape(-1)
    sig_l, sig_z, eps = F(p["sigma_l"]), F(p["sigma_z"]), F(p["lum_eps"])
    guides, state = [], []
    with np.errstate(all="ignore"):
        for a in range(npix):
            ns, nm, J, Q = int(acc["samples"][a]), int(acc["misses"][a]), int(acc["batches"][a]), np.float64(acc["q"][a])
            rgb = [np.float64(s[c * pl + a]) for c in range(3)]
            prim = int(hits["prim_id"][a])
            c, v, valid = [F(0)] * 3, F(0), ns > 0 and prim >= 0
            if valid:
                n, N = np.float64(ns), np.float64(ns + nm)
                Y = np.float64(0.299) * rgb[0] + np.float64(0.587) * rgb[1] + np.float64(0.114) * rgb[2]
                if J >= 2:
                    d = (Q - Y * Y / N) / np.float64(J - 1)
                    v64 = (d if d > 0 else np.float64(0)) * N / (n * n)
                else:
                    v64 = (Y / n) * (Y / n)
                c, v = [F(ch / n) for ch in rgb], F(v64)
                valid = bool(np.isfinite(c).all() and np.isfinite(v))
                if not valid:
                    c, v = [F(0)] * 3, F(0)
            guides.append({"n": [F(t) for t in hits["normal"][a]], "x": [F(t) for t in hits["position"][a]],
                           "d": F(hits["distance"][a]), "prim": prim if valid else -1})
            state.append((c, v))
        for k in range(p["iterations"]):
            step, nxt = 1 << k, []
            for a in range(npix):
                gp, (cp, vp) = guides[a], state[a]
                if gp["prim"] < 0:
                    nxt.append(state[a])
                    continue
                y, x = divmod(a, W)
                gs, ks = F(0), F(0)
                for j in (-1, 0, 1):
                    for i in (-1, 0, 1):
                        kw_ = K3[i + 1] * K3[j + 1]
                        qx, qy = x + i, y + j
                        if (i, j) != (0, 0):
                            if not (0 <= qx < W and 0 <= qy < H):
                                continue
                            gq = guides[qy * W + qx]
                            if gq["prim"] < 0 or not _wn(p, gp, gq) > 0:
                                continue
                        gs = gs + kw_ * state[qy * W + qx][1]
                        ks = ks + kw_
                den_l = sig_l * np.sqrt(gs / ks) + eps
                den_z = sig_z * gp["d"]
                Lp = _lum(cp)
                sw, sc, sv = F(0), [F(0)] * 3, F(0)
                for j in range(-2, 3):
                    for i in range(-2, 3):
                        if (i, j) == (0, 0):
                            wc = F(0.140625)
                            sw = sw + wc
                            sv = sv + wc * wc * vp
                            continue
                        qx, qy = x + step * i, y + step * j
                        if not (0 <= qx < W and 0 <= qy < H):
                            continue
                        gq = guides[qy * W + qx]
                        if gq["prim"] < 0:
                            continue
                        wn = _wn(p, gp, gq)
                        dx = [gq["x"][t] - gp["x"][t] for t in range(3)]
                        pd = gp["n"][0] * dx[0] + gp["n"][1] * dx[1] + gp["n"][2] * dx[2]
                        wz = _f(abs(pd) / den_z)
                        cq, vq = state[qy * W + qx]
                        wl = _f(abs(_lum(cq) - Lp) / den_l)
                        w = H5[i + 2] * H5[j + 2] * wn * wz * wl
                        if not w > 0:
                            continue
                        sw = sw + w
                        sc = [sc[t] + w * (cq[t] - cp[t]) for t in range(3)]
                        sv = sv + w * w * vq
                nxt.append(([cp[t] + sc[t] / sw for t in range(3)], sv / (sw * sw)))
            state = nxt
    out = np.zeros((3, npix))
    var = np.zeros(npix, np.float32)
    for a in range(npix):
        if guides[a]["prim"] >= 0:
            for c in range(3):
                out[c, a] = np.float64(state[a][0][c]) * np.float64(acc["samples"][a])
            var[a] = state[a][1]
        else:
            for c in range(3):
                out[c, a] = s[c * pl + a]
    return out.reshape(3, H, W), var.reshape(H, W)
