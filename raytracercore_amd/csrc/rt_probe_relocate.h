// rt_probe_relocate.h -- probe relocation (include/rtcore.h, "probe relocation"): the one copy of a placed
// probe's position, the fold of a probe's samples into its nearest front, nearest back and farthest front hit,
// the pairs' order that the device's cross-lane reduction uses, the relocation rule, and the placed forms of
// the segment, the blend and the depth-weighted blend that the kernels of api_probe_relocate.hip and the host
// twins compile.  fp64, every operation rounded on its own, as rt_probe_grid.h: sums and products through
// sh_add / sh_mul, division and square root through pg_div / pg_sqrt, no library function.
// The placed segment, corner and depth blend restate probe_segment_at, depth_corner and depth_blend with q
// handed in, rather than those being rewritten around a parameter: rt_probe_grid.h and rt_probe_depth.h, and
// with them the code of the unplaced kernels, stay as they are.
#pragma once
#include "rt_probe_depth.h"

namespace rtc {

RT_SH_HD double pr_inf()
{
    union {
        uint64_t u;
        double d;
    } q;
    q.u = 0x7ff0000000000000ull;
    return q.d;
}
RT_SH_HD uint64_t pr_bits(double a)
{
    union {
        uint64_t u;
        double d;
    } q;
    q.d = a;
    return q.u;
}

const char* const kRelocateParamsRule =
    "back_share finite in [0, 1), min_front finite and above 0, max_offset finite in (0, 0.5), flags "
    "RT_PROBE_RELOCATE_CLASSIFY_ONLY or 0, reserved 0";
inline bool relocate_params_ok(const rt_probe_relocate_params* P)
{
    return P && P->back_share >= 0.0 && P->back_share < 1.0 && pg_finite(P->min_front) && P->min_front > 0.0 && P->max_offset > 0.0 &&
           P->max_offset < 0.5 && !(P->flags & ~RT_PROBE_RELOCATE_CLASSIFY_ONLY) && !P->reserved;
}

// The offset of probe p (null: zeros) and whether it is valid.
RT_SH_HD bool placed_offset(const double* offsets, int64_t p, double o[3])
{
    o[0] = o[1] = o[2] = 0.0;
    if (offsets)
        for (int a = 0; a < 3; a++) o[a] = offsets[p * 3 + a];
    return pg_finite(o[0]) & pg_finite(o[1]) & pg_finite(o[2]);
}

// q of the probe (ix, iy, iz) with index p; false for a probe that is ABSENT by its offset or its state.
RT_SH_HD bool placed_position(const rt_probe_grid& G, const double* offsets, const uint32_t* state, int64_t ix, int64_t iy, int64_t iz,
                              int64_t p, double q[3])
{
    double o[3];
    const bool ok = placed_offset(offsets, p, o);
    q[0] = sh_add(sh_add(G.origin[0], sh_mul((double)ix, G.step[0])), o[0]);
    q[1] = sh_add(sh_add(G.origin[1], sh_mul((double)iy, G.step[1])), o[1]);
    q[2] = sh_add(sh_add(G.origin[2], sh_mul((double)iz, G.step[2])), o[2]);
    return ok && !(state && (state[p] & RT_PROBE_INSIDE));
}

// rt_probe_positions' record of probe p.
RT_SH_HD rt_surfel placed_surfel(const rt_probe_grid& G, const double* offsets, int64_t p)
{
    const int64_t nx = G.dims[0], ny = G.dims[1];
    double q[3];
    const bool ok = placed_position(G, offsets, nullptr, p % nx, (p / nx) % ny, p / (nx * ny), p, q);
    if (!ok) q[0] = q[1] = q[2] = pg_nan();
    return rt_surfel{rt_vec4d{q[0], q[1], q[2], ok ? 1.0 : pg_nan()}, rt_vec4d{0.0, 0.0, 1.0, 0.0}};
}

// ---- the fold ----
struct RelocFold {
    uint32_t front, back, misses, skipped;
    double d_near, d_back, d_far;
    int32_t k_near, k_back, k_far;
};
RT_SH_HD RelocFold reloc_fold_start()
{
    return RelocFold{0u, 0u, 0u, 0u, pr_inf(), pr_inf(), -pr_inf(), -1, -1, -1};
}
// Sample k into the fold; strict comparisons, so a later equal distance and a NaN never replace a winner.
RT_SH_HD void reloc_fold_sample(RelocFold& f, int32_t k, double x, double y, double z, int32_t prim_id, int32_t inside, double d)
{
    if (x == 0.0 && y == 0.0 && z == 0.0) {
        f.skipped++;
        return;
    }
    if (prim_id < 0) {
        f.misses++;
        return;
    }
    if (inside != 0) {
        f.back++;
        if (d < f.d_back) {
            f.d_back = d;
            f.k_back = k;
        }
        return;
    }
    f.front++;
    if (d < f.d_near) {
        f.d_near = d;
        f.k_near = k;
    }
    if (d > f.d_far) {
        f.d_far = d;
        f.k_far = k;
    }
}
// The order of (d, k) pairs across the lanes of a wave: b before a for a smaller d, then a smaller k (far: a
// larger d, then a smaller k).  A lane without a winner holds (+-inf, -1) and loses to every winner, since a
// winner's d is never that infinity.
RT_SH_HD bool reloc_less(double db, int32_t kb, double da, int32_t ka) { return db < da || (db == da && kb < ka); }
RT_SH_HD bool reloc_more(double db, int32_t kb, double da, int32_t ka) { return db > da || (db == da && kb < ka); }

// ---- the rule ----  o: the offset read; Db, Dn, Df: the directions of k_back, k_near, k_far ((0, 0, 0) for -1).
// Returns the record; c: the offset the rule gives (o where the candidate is refused).
RT_SH_HD rt_probe_relocation reloc_rule(const rt_probe_grid& G, const rt_probe_relocate_params& P, const RelocFold& f, int32_t spp,
                                        const double o[3], const double Db[3], const double Dn[3], const double Df[3], double c[3])
{
    rt_probe_relocation r;
    r.state = 0u;
    r.moved = 0u;
    r.front = f.front;
    r.back = f.back;
    r.misses = f.misses;
    r.skipped = f.skipped;
    r.k_near = f.k_near;
    r.k_back = f.k_back;
    r.k_far = f.k_far;
    r.reserved = 0;
    r.d_near = f.d_near;
    r.d_back = f.d_back;
    r.d_far = f.d_far;
    for (int a = 0; a < 3; a++) c[a] = o[a];
    if (f.skipped == (uint32_t)spp) {
        r.state = RT_PROBE_INSIDE | RT_PROBE_IDLE;
        return r;
    }
    const uint32_t hits = f.back + f.front;
    double cand[3] = {o[0], o[1], o[2]};
    if (hits > 0u && (double)f.back > sh_mul(P.back_share, (double)hits)) {
        r.state |= RT_PROBE_INSIDE;
        const double m = sh_add(f.d_back, sh_mul(P.min_front, 0.5));
        for (int a = 0; a < 3; a++) cand[a] = sh_add(o[a], sh_mul(Db[a], m));
    } else if (f.front > 0u && f.d_near < P.min_front) {
        const double p = sh_add(sh_add(sh_mul(Dn[0], Df[0]), sh_mul(Dn[1], Df[1])), sh_mul(Dn[2], Df[2]));
        if (!(p > 0.0)) {
            const double h = sh_mul(f.d_far, 0.5);
            const double t = h < P.min_front ? h : P.min_front;
            for (int a = 0; a < 3; a++) cand[a] = sh_add(o[a], sh_mul(Df[a], t));
        }
    } else {
        const double len = pg_sqrt(sh_add(sh_add(sh_mul(o[0], o[0]), sh_mul(o[1], o[1])), sh_mul(o[2], o[2])));
        if (len > 0.0) {
            const double room = sh_add(f.front > 0u ? f.d_near : pr_inf(), -P.min_front);
            const double m = room < len ? room : len;
            if (m == len)
                cand[0] = cand[1] = cand[2] = 0.0;
            else
                for (int a = 0; a < 3; a++) cand[a] = sh_add(o[a], -sh_mul(pg_div(o[a], len), m));
        }
    }
    const double ex = pg_div(cand[0], G.step[0]), ey = pg_div(cand[1], G.step[1]), ez = pg_div(cand[2], G.step[2]);
    const double e2 = sh_add(sh_add(sh_mul(ex, ex), sh_mul(ey, ey)), sh_mul(ez, ez));
    if (pg_finite(cand[0]) && pg_finite(cand[1]) && pg_finite(cand[2]) && e2 < sh_mul(P.max_offset, P.max_offset))
        for (int a = 0; a < 3; a++) c[a] = cand[a];
    const double diag = pg_sqrt(sh_add(sh_add(sh_mul(G.step[0], G.step[0]), sh_mul(G.step[1], G.step[1])), sh_mul(G.step[2], G.step[2])));
    if (f.front == 0u || f.d_near > diag) r.state |= RT_PROBE_IDLE;
    r.moved = pr_bits(c[0]) != pr_bits(o[0]) || pr_bits(c[1]) != pr_bits(o[1]) || pr_bits(c[2]) != pr_bits(o[2]) ? 1u : 0u;
    return r;
}

// ---- placed shading ----
// q of corner k of the cell; false for an absent probe.
RT_SH_HD bool placed_corner(const rt_probe_grid& G, const double* offsets, const uint32_t* state, const ProbeCell& c, int k, double q[3])
{
    return placed_position(G, offsets, state, c.i[0] + (k & 1), c.i[1] + ((k >> 1) & 1), c.i[2] + ((k >> 2) & 1), probe_index(G, c, k), q);
}

// probe_segment_at with the placed q: the empty segment also for an absent probe.
RT_SH_HD void placed_segment_at(const rt_probe_grid& G, const double* offsets, const uint32_t* state, const rt_surfel& s, const ProbeCell& c,
                                int k, double t, rt_ray& ray, double& t_max)
{
    ray = rt_ray{rt_vec4d{0.0, 0.0, 0.0, 0.0}, rt_vec4d{0.0, 0.0, 0.0, 0.0}};
    t_max = 0.0;
    if (!c.valid || !(G.flags & RT_PROBE_GRID_VISIBILITY) || t == 0.0) return;
    double q[3];
    if (!placed_corner(G, offsets, state, c, k, q)) return;
    const double ox = sh_add(s.position.x, sh_mul(G.bias, c.nx));
    const double oy = sh_add(s.position.y, sh_mul(G.bias, c.ny));
    const double oz = sh_add(s.position.z, sh_mul(G.bias, c.nz));
    const double vx = sh_add(q[0], -ox), vy = sh_add(q[1], -oy), vz = sh_add(q[2], -oz);
    const double d2 = sh_add(sh_add(sh_mul(vx, vx), sh_mul(vy, vy)), sh_mul(vz, vz));
    const double dist = pg_sqrt(d2);
    if (!(dist > 0.0) || !pg_finite(dist)) return;
    ray.origin = rt_vec4d{ox, oy, oz, 1.0};
    ray.direction = rt_vec4d{pg_div(vx, dist), pg_div(vy, dist), pg_div(vz, dist), 0.0};
    t_max = dist;
}

// The visited corners whose probe is absent, as probe_hidden's mask: probe_blend leaves them out as it leaves
// out the hidden ones.
RT_SH_HD unsigned placed_absent(const rt_probe_grid& G, const double* offsets, const uint32_t* state, const ProbeCell& c)
{
    unsigned absent = 0;
    if (!c.valid || (!offsets && !state)) return absent;
    for (int k = 0; k < kProbeCorners; k++) {
        if (c.t[k] == 0.0) continue;
        double q[3];
        absent |= placed_corner(G, offsets, state, c, k, q) ? 0u : 1u << k;
    }
    return absent;
}

// depth_corner with the placed q.
RT_SH_HD void placed_depth_corner(const rt_probe_grid& G, const rt_probe_depth_params& P, const double* D, const ProbeCell& c, int k,
                                  const double q[3], double ox, double oy, double oz, double& cheb, double& wrap)
{
    cheb = wrap = 1.0;
    const double vx = sh_add(ox, -q[0]), vy = sh_add(oy, -q[1]), vz = sh_add(oz, -q[2]);
    const double r = pg_sqrt(sh_add(sh_add(sh_mul(vx, vx), sh_mul(vy, vy)), sh_mul(vz, vz)));
    if (!(r > 0.0) || !pg_finite(r)) return;
    const double* texel = D + (probe_index(G, c, k) * kDepthTexels + oct_texel(vx, vy, vz)) * 2;
    const double mu = texel[0], m2 = texel[1];
    const double rc = r < P.d_max ? r : P.d_max;
    if (pg_finite(mu) && pg_finite(m2) && rc > mu) {
        double var = sh_add(m2, -sh_mul(mu, mu));
        var = var > P.var_floor ? var : P.var_floor;
        const double delta = sh_add(rc, -mu);
        const double qq = pg_div(var, sh_add(var, sh_mul(delta, delta)));
        cheb = sh_mul(sh_mul(qq, qq), qq);
    }
    if (P.flags & RT_PROBE_DEPTH_WRAP) {
        const double dn = sh_add(sh_add(sh_mul(vx, c.nx), sh_mul(vy, c.ny)), sh_mul(vz, c.nz));
        const double h = sh_mul(sh_add(1.0, -pg_div(dn, r)), 0.5);
        wrap = sh_add(sh_mul(h, h), 0.2);
    }
}

// depth_blend over the placed corners; an absent probe is left out like one whose L is absent.
RT_SH_HD void placed_depth_blend(const rt_probe_grid& G, const double* offsets, const uint32_t* state, const rt_probe_depth_params& P,
                                 const double* L, const double* D, const rt_surfel& s, const ProbeCell& c, double* E, double& W)
{
    E[0] = E[1] = E[2] = 0.0;
    W = 0.0;
    if (!c.valid) return;
    const double ox = sh_add(s.position.x, sh_mul(G.bias, c.nx));
    const double oy = sh_add(s.position.y, sh_mul(G.bias, c.ny));
    const double oz = sh_add(s.position.z, sh_mul(G.bias, c.nz));
    double B[kProbeL];
    for (int j = 0; j < kProbeL; j++) B[j] = 0.0;
    for (int k = 0; k < kProbeCorners; k++) {
        const double tc = c.t[k];
        if (tc == 0.0) continue;
        double q[3];
        if (!placed_corner(G, offsets, state, c, k, q)) continue;
        const double* Lc = L + probe_index(G, c, k) * kProbeL;
        double v[kProbeL];
        bool present = true;
        for (int j = 0; j < kProbeL; j++) {
            v[j] = Lc[j];
            present = present & pg_finite(v[j]);
        }
        if (!present) continue;
        double cheb, wrap;
        placed_depth_corner(G, P, D, c, k, q, ox, oy, oz, cheb, wrap);
        const double t = sh_mul(sh_mul(tc, cheb), wrap);
        if (!(t > 0.0)) continue;
        W = sh_add(W, t);
        for (int j = 0; j < kProbeL; j++) B[j] = sh_add(B[j], sh_mul(t, v[j]));
    }
    if (!(W > 0.0)) {
        W = 0.0;
        return;
    }
    const double A0 = 3.141592653589793, A1 = 2.0943951023931953, A2 = 0.7853981633974483;
    double Y[kShCoeffs];
    sh_basis(c.nx, c.ny, c.nz, Y);
    for (int l = 0; l < kShCoeffs; l++) Y[l] = sh_mul(l == 0 ? A0 : l < 4 ? A1 : A2, Y[l]);
    for (int ch = 0; ch < 3; ch++) {
        double e = sh_mul(Y[0], B[ch]);
        for (int l = 1; l < kShCoeffs; l++) e = sh_add(e, sh_mul(Y[l], B[3 * l + ch]));
        E[ch] = pg_div(e, W);
    }
}

} // namespace rtc
