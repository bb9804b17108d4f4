// rt_probe_grid.h -- a grid of L2 light probes read at shading points (include/rtcore.h, "probe grids",
// rt_probe_grid): the one copy of the radiance close, the cell, the corners, the segments and the blend that
// the three kernels of api_shade_probes.hip and the host twins rt_debug_probe_radiance,
// rt_debug_probe_segments and rt_debug_shade_probes compile.  fp64, every operation rounded on its own: the
// sums and products through sh_add / sh_mul (rt_sh.h), division and square root IEEE on both sides (the
// device's through __ddiv_rn / __dsqrt_rn), no library function.
#pragma once
#include <cstdint>

#include "../../include/rtcore.h"
#include "rt_sh.h"

namespace rtc {

constexpr int kProbeCorners = 8;          // c = dx + 2 dy + 4 dz
constexpr int kProbeL = kShCoeffs * 3;    // doubles of one probe's L: [l][ch]

RT_SH_HD double pg_div(double a, double b)
{
#ifdef __HIP_DEVICE_COMPILE__
    return __ddiv_rn(a, b);
#else
    return a / b;
#endif
}
RT_SH_HD double pg_sqrt(double a)
{
#ifdef __HIP_DEVICE_COMPILE__
    return __dsqrt_rn(a);
#else
    return __builtin_sqrt(a);
#endif
}
RT_SH_HD bool pg_finite(double x) { return x >= -1.7976931348623157e308 && x <= 1.7976931348623157e308; } // (NaN: false)
RT_SH_HD double pg_nan()
{
    union {
        uint64_t u;
        double d;
    } q;
    q.u = 0x7ff8000000000000ull;
    return q.d;
}

// L of one probe from rt_render_probes' accumulators; an absent probe (N == 0) is all quiet NaNs.
RT_SH_HD void probe_radiance(const rt_probe_sh& sh, uint32_t samples, uint32_t misses, const rt_color& ambient, double* L)
{
    const uint64_t N = (uint64_t)samples + (uint64_t)misses;
    if (N == 0) {
        for (int j = 0; j < kProbeL; j++) L[j] = pg_nan();
        return;
    }
    const double k = pg_div(4.0 * 3.141592653589793, (double)N);
    const double amb[3] = {ambient.r, ambient.g, ambient.b};
    for (int l = 0; l < kShCoeffs; l++)
        for (int ch = 0; ch < 3; ch++) L[3 * l + ch] = sh_mul(k, sh_add(sh.c[l][ch], sh_mul(sh.c[l][3], amb[ch])));
}

// A point's place in the grid: valid, its unit normal, the cell's first probe and the eight trilinear weights
// (0: a corner that is not visited).
struct ProbeCell {
    bool valid;
    double nx, ny, nz;
    int i[3];
    double t[kProbeCorners];
};

RT_SH_HD ProbeCell probe_cell(const rt_probe_grid& G, const rt_surfel& s)
{
    ProbeCell c;
    const double p[3] = {s.position.x, s.position.y, s.position.z};
    const double n2 = sh_add(sh_add(sh_mul(s.normal.x, s.normal.x), sh_mul(s.normal.y, s.normal.y)), sh_mul(s.normal.z, s.normal.z));
    c.valid = pg_finite(p[0]) && pg_finite(p[1]) && pg_finite(p[2]) && pg_finite(s.position.w) && pg_finite(s.normal.x) &&
              pg_finite(s.normal.y) && pg_finite(s.normal.z) && pg_finite(s.normal.w) && pg_finite(n2) && n2 != 0.0;
    c.nx = c.ny = c.nz = 0.0;
    c.i[0] = c.i[1] = c.i[2] = 0;
    for (int k = 0; k < kProbeCorners; k++) c.t[k] = 0.0;
    if (!c.valid) return c;
    const double len = pg_sqrt(n2);
    c.nx = pg_div(s.normal.x, len);
    c.ny = pg_div(s.normal.y, len);
    c.nz = pg_div(s.normal.z, len);
    double f[3];
    for (int a = 0; a < 3; a++) {
        if (G.dims[a] == 1) {
            c.i[a] = 0;
            f[a] = 0.0;
            continue;
        }
        double g = pg_div(sh_add(p[a], -G.origin[a]), G.step[a]);
        const double top = (double)(G.dims[a] - 1);
        g = g < 0.0 ? 0.0 : g > top ? top : g;
        int i = (int)g;
        if (i > G.dims[a] - 2) i = G.dims[a] - 2;
        c.i[a] = i;
        f[a] = sh_add(g, -(double)i);
    }
    for (int k = 0; k < kProbeCorners; k++) {
        const double wx = (k & 1) ? f[0] : sh_add(1.0, -f[0]);
        const double wy = (k & 2) ? f[1] : sh_add(1.0, -f[1]);
        const double wz = (k & 4) ? f[2] : sh_add(1.0, -f[2]);
        c.t[k] = sh_mul(sh_mul(wx, wy), wz);
    }
    return c;
}

// The probe of a visited corner (t[k] != 0: its index lies inside dims).
RT_SH_HD int64_t probe_index(const rt_probe_grid& G, const ProbeCell& c, int k)
{
    const int64_t ix = c.i[0] + (k & 1), iy = c.i[1] + ((k >> 1) & 1), iz = c.i[2] + ((k >> 2) & 1);
    return (iz * G.dims[1] + iy) * G.dims[0] + ix;
}

// The segment from the point (pushed bias along its unit normal) to corner k's probe, t = c.t[k] (its own
// argument: the segment kernel picks it without a register index); an empty segment (all zeros, t_max 0) for a
// corner that is not visited, a grid without visibility or a probe at the point itself.
RT_SH_HD void probe_segment_at(const rt_probe_grid& G, const rt_surfel& s, const ProbeCell& c, int k, double t, rt_ray& ray,
                               double& t_max)
{
    ray = rt_ray{rt_vec4d{0.0, 0.0, 0.0, 0.0}, rt_vec4d{0.0, 0.0, 0.0, 0.0}};
    t_max = 0.0;
    if (!c.valid || !(G.flags & RT_PROBE_GRID_VISIBILITY) || t == 0.0) return;
    const double ox = sh_add(s.position.x, sh_mul(G.bias, c.nx));
    const double oy = sh_add(s.position.y, sh_mul(G.bias, c.ny));
    const double oz = sh_add(s.position.z, sh_mul(G.bias, c.nz));
    const double qx = sh_add(G.origin[0], sh_mul((double)(c.i[0] + (k & 1)), G.step[0]));
    const double qy = sh_add(G.origin[1], sh_mul((double)(c.i[1] + ((k >> 1) & 1)), G.step[1]));
    const double qz = sh_add(G.origin[2], sh_mul((double)(c.i[2] + ((k >> 2) & 1)), G.step[2]));
    const double vx = sh_add(qx, -ox), vy = sh_add(qy, -oy), vz = sh_add(qz, -oz);
    const double d2 = sh_add(sh_add(sh_mul(vx, vx), sh_mul(vy, vy)), sh_mul(vz, vz));
    const double dist = pg_sqrt(d2);
    if (!(dist > 0.0) || !pg_finite(dist)) return;
    ray.origin = rt_vec4d{ox, oy, oz, 1.0};
    ray.direction = rt_vec4d{pg_div(vx, dist), pg_div(vy, dist), pg_div(vz, dist), 0.0};
    t_max = dist;
}

// The point's eight visibility answers as a mask: bit k set for a hidden corner (null: none).
RT_SH_HD unsigned probe_hidden(const uint8_t* occluded)
{
    unsigned hidden = 0;
    if (occluded)
        for (int k = 0; k < kProbeCorners; k++) hidden |= occluded[k] ? 1u << k : 0u;
    return hidden;
}

// The blend of the corners that are visited, not hidden (probe_hidden's mask) and present, in ascending
// order, and the irradiance for the point's normal.  E: three doubles.
RT_SH_HD void probe_blend(const rt_probe_grid& G, const double* L, const ProbeCell& c, unsigned hidden, double* E, double& W)
{
    E[0] = E[1] = E[2] = 0.0;
    W = 0.0;
    if (!c.valid) return;
    double B[kProbeL];
    for (int j = 0; j < kProbeL; j++) B[j] = 0.0;
    for (int k = 0; k < kProbeCorners; k++) {
        const double t = c.t[k];
        if (t == 0.0 || ((hidden >> k) & 1u)) continue;
        const double* Lc = L + probe_index(G, c, k) * kProbeL;
        double v[kProbeL];
        bool present = true;
        for (int j = 0; j < kProbeL; j++) {
            v[j] = Lc[j];
            present = present & pg_finite(v[j]);
        }
        if (!present) continue;
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
