"""Probe relocation: include/rtcore.h's "probe relocation" restated in plain Python, one rounding per operation and
in the stated order (Python floats are IEEE doubles), and the inputs the host and the GPU tests share.  Nothing
here touches a device."""
import math
import struct

import numpy as np

from probe_depth_cases import A_LOBE, replay_basis, replay_cell, replay_corner, same_bits  # noqa: F401 (same_bits: re-exported)

INSIDE, IDLE, CLASSIFY_ONLY = 1, 2, 1
INF = math.inf


def bits(x):
    return struct.pack("<d", float(x))


def finite3(o):
    return all(math.isfinite(float(v)) for v in o)


def grid_index(dims, p):
    return p % dims[0], (p // dims[0]) % dims[1], p // (dims[0] * dims[1])


def replay_position(origin, step, index, o):
    """q of the probe at grid index (ix, iy, iz) with offset o (three floats): the grid term, then the offset."""
    return [(origin[a] + float(index[a]) * step[a]) + float(o[a]) for a in range(3)]


def replay_positions(origin, step, dims, offsets):
    """rt_probe_positions: (n_probes, 2, 4) doubles, position and normal."""
    n = dims[0] * dims[1] * dims[2]
    out = np.zeros((n, 2, 4))
    out[:, 1, 2] = 1.0
    for p in range(n):
        o = [0.0] * 3 if offsets is None else [float(v) for v in offsets[p]]
        out[p, 0] = replay_position(origin, step, grid_index(dims, p), o) + [1.0] if finite3(o) else [math.nan] * 4
    return out


def replay_fold(rays, hits):
    """The fold of one probe: rays (spp,) RAY_DTYPE, hits (spp,) HIT_DTYPE -> a dict of the record's fields."""
    f = dict(front=0, back=0, misses=0, skipped=0, d_near=INF, d_back=INF, d_far=-INF, k_near=-1, k_back=-1, k_far=-1)
    for k in range(len(rays)):
        x, y, z = (float(v) for v in rays[k]["direction"][:3])
        if x == 0.0 and y == 0.0 and z == 0.0:
            f["skipped"] += 1
            continue
        if int(hits[k]["prim_id"]) < 0:
            f["misses"] += 1
            continue
        d = float(hits[k]["distance"])
        if int(hits[k]["inside"]) != 0:
            f["back"] += 1
            if d < f["d_back"]:
                f["d_back"], f["k_back"] = d, k
            continue
        f["front"] += 1
        if d < f["d_near"]:
            f["d_near"], f["k_near"] = d, k
        if d > f["d_far"]:
            f["d_far"], f["k_far"] = d, k
    return f


def replay_rule(step, back_share, min_front, max_offset, f, spp, o, rays):
    """The rule: (the offset it gives, state, moved, the branch taken: 'a', 'b', 'c' or 's' for all skipped, and
    whether a candidate other than o was refused)."""
    o = [float(v) for v in o]
    if f["skipped"] == spp:
        return o, INSIDE | IDLE, 0, "s", False

    def D(k):
        return [float(v) for v in rays[k]["direction"][:3]] if k >= 0 else [0.0, 0.0, 0.0]

    state = 0
    cand = list(o)
    hits = f["back"] + f["front"]
    if hits > 0 and float(f["back"]) > back_share * float(hits):
        branch = "a"
        state |= INSIDE
        m = f["d_back"] + min_front * 0.5
        Db = D(f["k_back"])
        cand = [o[a] + Db[a] * m for a in range(3)]
    elif f["front"] > 0 and f["d_near"] < min_front:
        branch = "b"
        Dn, Df = D(f["k_near"]), D(f["k_far"])
        p = (Dn[0] * Df[0] + Dn[1] * Df[1]) + Dn[2] * Df[2]
        if not p > 0.0:
            h = f["d_far"] * 0.5
            t = h if h < min_front else min_front
            cand = [o[a] + Df[a] * t for a in range(3)]
    else:
        branch = "c"
        ln = math.sqrt((o[0] * o[0] + o[1] * o[1]) + o[2] * o[2])
        if ln > 0.0:
            room = (f["d_near"] if f["front"] > 0 else INF) - min_front
            m = room if room < ln else ln
            cand = [0.0, 0.0, 0.0] if m == ln else [o[a] - (o[a] / ln) * m for a in range(3)]
    with np.errstate(all="ignore"):
        e = [float(np.float64(cand[a]) / np.float64(step[a])) for a in range(3)]
        e2 = float((np.float64(e[0]) * e[0] + np.float64(e[1]) * e[1]) + np.float64(e[2]) * e[2])
    ok = finite3(cand) and e2 < max_offset * max_offset
    c = cand if ok else o
    diag = math.sqrt((step[0] * step[0] + step[1] * step[1]) + step[2] * step[2])
    if f["front"] == 0 or f["d_near"] > diag:
        state |= IDLE
    moved = int(any(bits(c[a]) != bits(o[a]) for a in range(3)))
    refused = not ok and any(bits(cand[a]) != bits(o[a]) for a in range(3))
    return c, state, moved, branch, refused


def replay_relocate(step, back_share, min_front, max_offset, flags, rays, hits, offsets):
    """rt_debug_probe_relocate: (offsets after, a list of record dicts, the branches, the refusals)."""
    n, spp = rays.shape
    out = np.array(offsets, np.float64).reshape(n, 3).copy()
    info, branches, refusals = [], [], []
    for i in range(n):
        f = replay_fold(rays[i], hits[i])
        with np.errstate(all="ignore"):
            c, state, moved, branch, refused = replay_rule(step, back_share, min_front, max_offset, f, spp, out[i], rays[i])
        f.update(state=state, moved=moved, reserved=0)
        info.append(f)
        branches.append(branch)
        refusals.append(refused)
        if not flags & CLASSIFY_ONLY:
            out[i] = c
    return out, info, branches, refusals


def info_matches(info, want):
    """A RELOCATION_DTYPE array against replay_relocate's dicts, the doubles by their bits."""
    if len(info) != len(want):
        return False
    for rec, w in zip(info, want):
        for name in rec.dtype.names:
            if name.startswith("d_"):
                if bits(rec[name]) != bits(w[name]):
                    return False
            elif int(rec[name]) != int(w[name]):
                return False
    return True


# ---------------------------------------------------------------- forced cases
STEP = (1.0, 0.75, 1.25)
BACK_SHARE, MIN_FRONT, MAX_OFFSET = 0.25, 0.25, 0.45
SPP = 8
X, NX, Y, Z = (1.0, 0.0, 0.0), (-1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0)
DIAG = tuple(float(np.float32(v)) for v in (0.6, 0.8, 0.0))
NAN = math.nan
# name -> (offset, samples); a sample is (direction, kind, distance), kind 'f' front, 'b' back, 'm' miss, 's' skipped;
# a probe is filled up to SPP samples with misses
FORCED = {
    # (a): back 3 of 8 hits > 0.25 * 8; the nearest back face is sample 2
    "a_taken": ((0.0, 0.0, 0.0), [(Y, "b", 0.3), (Z, "f", 1.0), (X, "b", 0.2), (Z, "b", 0.4)] + [(Z, "f", 1.0)] * 4),
    # back 2 of 8 hits is exactly the share: not taken; nothing near, no offset: (c) with len == 0
    "a_exact_share": ((0.0, 0.0, 0.0), [(X, "b", 0.2), (Y, "b", 0.3)] + [(Z, "f", 1.0)] * 6),
    "b_p_positive": ((0.05, 0.0, 0.0), [(X, "f", 0.1), (DIAG, "f", 2.0), (Z, "f", 1.0)]),
    "b_p_zero_h_above": ((0.0, 0.05, 0.0), [(X, "f", 0.1), (Y, "f", 2.0), (Z, "f", 1.0)]),
    "b_p_negative_h_below": ((0.0, 0.0, 0.0), [(X, "f", 0.1), (NX, "f", 0.3), (Z, "f", 0.2)]),
    "b_p_negative_h_above": ((0.0, 0.0, 0.1), [(NX, "f", 1.0), (X, "f", 0.1), (Z, "f", 0.5)]),
    "c_len_zero": ((0.0, 0.0, 0.0), [(X, "f", 0.5), (Y, "f", 0.25), (Z, "f", 3.0)]),
    "c_home_exactly": ((0.1, -0.0, 0.05), [(X, "f", 1.0), (Y, "f", 2.0)]),
    "c_part_way": ((0.3, 0.0, 0.2), [(X, "f", 0.35), (Y, "f", 2.0)]),
    "c_no_front": ((0.2, 0.1, 0.0), [(X, "m", 0.0)]),
    # (a) with a candidate outside the ellipsoid: 0.6 + 0.125 along x at step 1
    "refused_outside": ((0.01, 0.0, 0.0), [(X, "b", 0.6), (Y, "b", 0.7), (Z, "b", 0.9), (Z, "f", 1.0)]),
    # (a) whose back distances are all NaN: no winner, m = inf, D = 0: a NaN candidate
    "refused_not_finite": ((0.0, 0.02, 0.0), [(X, "b", NAN), (Y, "b", NAN), (Z, "b", NAN), (Z, "f", 1.0)]),
    "ties_keep_lowest_k": ((0.0, 0.0, 0.0), [(X, "b", 0.5), (Y, "f", 0.1), (Z, "f", 2.0), (Y, "b", 0.5), (X, "f", 0.1), (NX, "f", 2.0),
                                            (Z, "f", 0.1), (DIAG, "f", 0.7)]),
    "zeros_of_both_signs_tie": ((0.0, 0.0, 0.0), [(X, "f", 1.0), (Y, "f", 0.0), (Z, "f", 1.0), (NX, "f", -0.0)]),
    "nan_counted_never_chosen": ((0.1, 0.0, 0.0), [(X, "f", NAN), (Y, "f", 0.5), (Z, "f", NAN), (NX, "b", NAN), (Z, "f", 0.6)]),
    "misses_and_skipped": ((0.0, 0.0, 0.1), [(X, "s", 0.0), (Y, "m", 0.0), (Z, "f", 0.2), (X, "s", 0.0), (NX, "f", 0.9)]),
    "all_skipped": ((0.1, 0.0, 0.0), [(X, "s", 0.0)] * SPP),
    "offset_not_finite": ((NAN, 0.0, 0.0), [(X, "s", 0.0)] * SPP),
}
WANT_BRANCH = {"a_taken": "a", "a_exact_share": "c", "b_p_positive": "b", "b_p_zero_h_above": "b", "b_p_negative_h_below": "b",
               "b_p_negative_h_above": "b", "c_len_zero": "c", "c_home_exactly": "c", "c_part_way": "c", "c_no_front": "c",
               "refused_outside": "a", "refused_not_finite": "a", "ties_keep_lowest_k": "b", "zeros_of_both_signs_tie": "b",
               "nan_counted_never_chosen": "c", "misses_and_skipped": "b", "all_skipped": "s", "offset_not_finite": "s"}


def forced_samples(rc):
    """(names, dims, rays (n, SPP) RAY_DTYPE, hits (n, SPP) HIT_DTYPE, offsets (n, 3)): one probe per forced case
    on an n x 1 x 1 grid."""
    names = list(FORCED)
    n = len(names)
    rays, hits, offsets = np.zeros((n, SPP), rc.RAY_DTYPE), np.zeros((n, SPP), rc.HIT_DTYPE), np.zeros((n, 3))
    hits["prim_id"] = -1
    rays["origin"][..., 3] = 1.0
    rays["direction"][..., :3] = Z
    for i, name in enumerate(names):
        offsets[i], samples = FORCED[name]
        assert len(samples) <= SPP
        for k, (d, kind, dist) in enumerate(samples):
            rays["direction"][i, k, :3] = (0.0, 0.0, 0.0) if kind == "s" else d
            if kind in "fb":
                hits["prim_id"][i, k] = 3
                hits["inside"][i, k] = int(kind == "b")
                hits["distance"][i, k] = dist
    return names, (n, 1, 1), rays, hits, offsets


# ---------------------------------------------------------------- placed shading
def random_placement(dims, step, seed=41, inside_share=0.15, max_offset=0.45, nan_probe=None):
    """Random offsets inside the ellipsoid, a share of RT_PROBE_INSIDE states (and some RT_PROBE_IDLE bits, which
    shading ignores), and one probe with a NaN offset."""
    rng = np.random.default_rng(seed)
    n = dims[0] * dims[1] * dims[2]
    u = rng.normal(size=(n, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    offsets = u * rng.uniform(0, 0.95 * max_offset, (n, 1)) * np.array(step)
    state = (rng.random(n) < inside_share).astype(np.uint32) * INSIDE | (rng.random(n) < 0.3).astype(np.uint32) * IDLE
    if nan_probe is not None:
        offsets[nan_probe, 1] = np.nan
        state[nan_probe] = 0
    return offsets, state


def probe_absent(offsets, state, p):
    return (offsets is not None and not finite3(offsets[p])) or (state is not None and int(state[p]) & INSIDE != 0)


def replay_absent_mask(origin, step, dims, offsets, state, pos, nrm):
    """(n, 8) bool: the visited corners whose probe is absent."""
    mask = np.zeros((len(pos), 8), bool)
    for k in range(len(pos)):
        cell = replay_cell(origin, step, dims, pos[k], nrm[k])
        if cell is None:
            continue
        _, i, t = cell
        for c in range(8):
            if t[c] == 0.0:
                continue
            ix, iy, iz = (i[a] + ((c >> a) & 1) for a in range(3))
            mask[k, c] = probe_absent(offsets, state, (iz * dims[1] + iy) * dims[0] + ix)
    return mask


def replay_segments_placed(origin, step, dims, bias, offsets, state, pos, nrm, visibility=True):
    """rtcore.h, "Segment" with the placed q: (rays (n, 8, 2, 4), t_max (n, 8))."""
    n = len(pos)
    rays, t_max = np.zeros((n, 8, 2, 4)), np.zeros((n, 8))
    for k in range(n):
        cell = replay_cell(origin, step, dims, pos[k], nrm[k])
        if cell is None or not visibility:
            continue
        nh, i, t = cell
        for c in range(8):
            if t[c] == 0.0:
                continue
            index = [i[a] + ((c >> a) & 1) for a in range(3)]
            probe = (index[2] * dims[1] + index[1]) * dims[0] + index[0]
            if probe_absent(offsets, state, probe):
                continue
            o = [float(pos[k][a]) + bias * nh[a] for a in range(3)]
            q = replay_position(origin, step, index, [0.0] * 3 if offsets is None else offsets[probe])
            v = [q[a] - o[a] for a in range(3)]
            dist = math.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
            if not dist > 0.0 or not math.isfinite(dist):
                continue
            rays[k, c, 0] = o + [1.0]
            rays[k, c, 1] = [v[0] / dist, v[1] / dist, v[2] / dist, 0.0]
            t_max[k, c] = dist
    return rays, t_max


def replay_shade_depth_placed(origin, step, dims, bias, d_max, var_floor, wrap, offsets, state, L, D, pos, nrm):
    """probe_depth_cases.replay_shade with the placed q and without the absent probes."""
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
            index = [i[a] + ((c >> a) & 1) for a in range(3)]
            probe = (index[2] * dims[1] + index[1]) * dims[0] + index[0]
            if probe_absent(offsets, state, probe):
                continue
            row = [float(v) for v in Lp[probe]]
            if not all(math.isfinite(v) for v in row):
                continue
            q = replay_position(origin, step, index, [0.0] * 3 if offsets is None else offsets[probe])
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
