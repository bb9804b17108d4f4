"""The surfel set the rt_occluded_surfels tests share (tests/test_occluded_surfels_host.py, _gpu.py),
computable without a GPU, and the oracle's answer for its samples.

The set of a scene: the first N = 200 generator rays of tests/test_query_rays_gpu.py (three full waves and a
short fourth) traced with the oracle; a hit gives the position o + (t - 1e-3) d, a miss the position o, both
the normal -d.  Then spoiled as tests/test_render_surfels_gpu.py spoils its set: surfel 7 gets a NaN position
component, 130 an infinite normal component, 64 a zero normal, 10 and 11 the normals (0, 0, +-1)."""
import functools

import numpy as np

from test_query_rays_gpu import _line_of_sight_rays, _oracle, _scene, _trace
from test_render_surfels_host import directions, draws

SEED = 11
N = 200
BASE = 123457
BAD = [7, 130, 64]
POLES = (10, 11)
INF = float("inf")
T_CYCLE = (0.25, 1.0, INF)  # S1's t_max by entry


@functools.lru_cache(maxsize=None)
def surfel_set(name):
    """(positions, normals), both (N, 3) f64 (read-only, shared)."""
    o, d = (a[:N] for a in _line_of_sight_rays(_scene(name).cameras[0]))
    ids, ts = _trace(_oracle(name), o, d)
    hit = ids >= 0
    pos = np.where(hit[:, None], o + (np.where(hit, ts, 0.0) - 1e-3)[:, None] * d, o)
    nrm = -d.copy()
    pos[BAD[0], 1] = np.nan
    nrm[BAD[1], 2] = np.inf
    nrm[BAD[2]] = 0.0
    nrm[POLES[0]] = (0.0, 0.0, 1.0)
    nrm[POLES[1]] = (0.0, 0.0, -1.0)
    pos.setflags(write=False)
    nrm.setflags(write=False)
    return pos, nrm


def valid_surfels():
    return np.setdiff1d(np.arange(N), BAD)


def t_cycle(n=N):
    return np.asarray(T_CYCLE)[np.arange(n) % len(T_CYCLE)]


@functools.lru_cache(maxsize=None)
def oracle_distances(name, mode, spp=5):
    """The oracle's distance along the fp64 restatement's direction of sample k of the valid surfels,
    [len(valid), spp]; +inf where it meets nothing (read-only, shared)."""
    pos, nrm = surfel_set(name)
    good = valid_surfels()
    u1, u2 = draws(SEED, BASE + good, range(spp))
    d, _ = directions(nrm[good], mode, u1, u2)
    orc = _oracle(name)
    out = np.empty((len(good), spp))
    for k in range(spp):
        ids, ts = _trace(orc, pos[good], d[:, k])
        out[:, k] = np.where(ids >= 0, ts, INF)
    out.setflags(write=False)
    return out


def shares(occluded):
    """(the occluded share of the samples, the share of surfels with both outcomes) of a bool
    [surfels, spp] array."""
    occ = np.asarray(occluded, bool)
    per = occ.sum(axis=1)
    return float(occ.mean()), float(((per > 0) & (per < occ.shape[1])).mean())


def assert_not_hollow(occluded, what):
    """The two conditions on a set's answers: the occluded share of the valid surfels' samples lies in
    [5 %, 95 %], and at least 10 % of the surfels have both outcomes among their samples."""
    share, mixed = shares(occluded)
    print(f"{what}: occluded share {100 * share:.1f} %, surfels with both outcomes {100 * mixed:.1f} %")
    assert 0.05 <= share <= 0.95, (what, share)
    assert mixed >= 0.10, (what, mixed)
