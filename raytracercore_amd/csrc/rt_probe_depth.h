// rt_probe_depth.h -- probe depth maps (include/rtcore.h, "probe depth maps", rt_probe_depth): the one copy of
// the octahedral texel rules, the fold of a sample into a texel's distance moments, the close and the
// Chebyshev-weighted blend that the three kernels of api_probe_depth.hip and the host twins
// rt_debug_oct_texel_dirs, rt_debug_oct_texel, rt_debug_probe_depth_fold, rt_debug_probe_depth_close and
// rt_debug_shade_probes_depth compile.  fp64, every operation rounded on its own, as rt_probe_grid.h: sums and
// products through sh_add / sh_mul, division and square root through pg_div / pg_sqrt, no library function.
#pragma once
#include "rt_probe_grid.h"

namespace rtc {

constexpr int kDepthRes = 8;                          // R: texels per side of a probe's octahedral map
constexpr int kDepthTexels = kDepthRes * kDepthRes;   // 64: one per lane of a wave (the fold kernel rests on it)
constexpr int kDepthMaxSharpness = 8;

RT_SH_HD double pd_abs(double a) { return __builtin_fabs(a); } // (the sign bit cleared: exact, -0.0 -> 0.0)
RT_SH_HD double pd_sgn(double a) { return a >= 0.0 ? 1.0 : -1.0; } // (-0.0 -> 1)

// The fold of the lower half of the octahedron onto the square's corners: (u, v) of a direction with z < 0,
// signs by (sx, sy).
RT_SH_HD void oct_wrap(double u, double v, double sx, double sy, double& uo, double& vo)
{
    uo = sh_mul(sh_add(1.0, -pd_abs(v)), pd_sgn(sx));
    vo = sh_mul(sh_add(1.0, -pd_abs(u)), pd_sgn(sy));
}

// T_t: the unit direction of texel t = ty * 8 + tx's centre.
RT_SH_HD void oct_texel_dir(int t, double& Tx, double& Ty, double& Tz)
{
    const int tx = t & (kDepthRes - 1), ty = t >> 3;
    const double u = sh_add(pg_div((double)(2 * tx + 1), (double)kDepthRes), -1.0); // (both exact)
    const double v = sh_add(pg_div((double)(2 * ty + 1), (double)kDepthRes), -1.0);
    const double z = sh_add(sh_add(1.0, -pd_abs(u)), -pd_abs(v));
    double x = u, y = v;
    if (z < 0.0) oct_wrap(u, v, u, v, x, y);
    const double len = pg_sqrt(sh_add(sh_add(sh_mul(x, x), sh_mul(y, y)), sh_mul(z, z)));
    Tx = pg_div(x, len);
    Ty = pg_div(y, len);
    Tz = pg_div(z, len);
}

// A texel coordinate from u' in [-1, 1]: (int)((u' + 1) * 4) held to [0, 7] (a NaN: 0).
RT_SH_HD int oct_coord(double u)
{
    const double a = sh_mul(sh_add(u, 1.0), 4.0);
    return !(a > 0.0) ? 0 : a > (double)(kDepthRes - 1) ? kDepthRes - 1 : (int)a;
}

// The texel of a finite, non-zero vector (not necessarily unit).
RT_SH_HD int oct_texel(double x, double y, double z)
{
    const double s1 = sh_add(sh_add(pd_abs(x), pd_abs(y)), pd_abs(z));
    double u = pg_div(x, s1), v = pg_div(y, s1);
    if (z < 0.0) {
        double uo, vo;
        oct_wrap(u, v, x, y, uo, vo);
        u = uo;
        v = vo;
    }
    return oct_coord(v) * kDepthRes + oct_coord(u);
}

const char* const kDepthParamsRule = "d_max and var_floor finite and above 0, sharpness 0 .. 8, flags RT_PROBE_DEPTH_WRAP or 0, reserved 0";
inline bool depth_params_ok(const rt_probe_depth_params* P)
{
    return P && pg_finite(P->d_max) && P->d_max > 0.0 && pg_finite(P->var_floor) && P->var_floor > 0.0 && P->sharpness >= 0 &&
           P->sharpness <= kDepthMaxSharpness && !(P->flags & ~RT_PROBE_DEPTH_WRAP) && !P->reserved[0] && !P->reserved[1];
}

// A sample's distance: the hit's, held to d_max; d_max for a miss (and for a distance that is a NaN).
RT_SH_HD double depth_of(bool hit, double distance, double d_max) { return hit && distance < d_max ? distance : d_max; }

// One sample (direction x, y, z, distance d) into the three sums of the texel of direction T.
RT_SH_HD void depth_add(double Tx, double Ty, double Tz, double x, double y, double z, double d, int sharpness, double& s0, double& s1,
                        double& s2)
{
    const double c = sh_add(sh_add(sh_mul(x, Tx), sh_mul(y, Ty)), sh_mul(z, Tz));
    if (!(c > 0.0)) return;
    double w = c;
    for (int k = 0; k < sharpness; k++) w = sh_mul(w, w);
    const double wd = sh_mul(w, d);
    s0 = sh_add(s0, w);
    s1 = sh_add(s1, wd);
    s2 = sh_add(s2, sh_mul(wd, d));
}

// D of one texel: (s1 / s0, s2 / s0), or two quiet NaNs where s0 is not > 0 (the texel is ABSENT).
RT_SH_HD void depth_close(double s0, double s1, double s2, double& mu, double& m2)
{
    if (!(s0 > 0.0)) {
        mu = m2 = pg_nan();
        return;
    }
    mu = pg_div(s1, s0);
    m2 = pg_div(s2, s0);
}

// The factors of corner k of a point at o = p + bias n^ with unit normal (c.nx, c.ny, c.nz): the Chebyshev
// weight against the probe's map and the wrap weight; D: the grid's n_probes x 64 x 2 doubles.
RT_SH_HD void depth_corner(const rt_probe_grid& G, const rt_probe_depth_params& P, const double* D, const ProbeCell& c, int k, double ox,
                           double oy, double oz, double& cheb, double& wrap)
{
    cheb = wrap = 1.0;
    const double qx = sh_add(G.origin[0], sh_mul((double)(c.i[0] + (k & 1)), G.step[0]));
    const double qy = sh_add(G.origin[1], sh_mul((double)(c.i[1] + ((k >> 1) & 1)), G.step[1]));
    const double qz = sh_add(G.origin[2], sh_mul((double)(c.i[2] + ((k >> 2) & 1)), G.step[2]));
    const double vx = sh_add(ox, -qx), vy = sh_add(oy, -qy), vz = sh_add(oz, -qz);
    const double r = pg_sqrt(sh_add(sh_add(sh_mul(vx, vx), sh_mul(vy, vy)), sh_mul(vz, vz)));
    if (!(r > 0.0) || !pg_finite(r)) return;
    const double* texel = D + (probe_index(G, c, k) * kDepthTexels + oct_texel(vx, vy, vz)) * 2;
    const double mu = texel[0], m2 = texel[1];
    const double rc = r < P.d_max ? r : P.d_max;
    if (pg_finite(mu) && pg_finite(m2) && rc > mu) {
        double var = sh_add(m2, -sh_mul(mu, mu));
        var = var > P.var_floor ? var : P.var_floor; // (a NaN cannot come from finite mu and m2 short of an overflow: the floor then)
        const double delta = sh_add(rc, -mu);
        const double q = pg_div(var, sh_add(var, sh_mul(delta, delta)));
        cheb = sh_mul(sh_mul(q, q), q);
    }
    if (P.flags & RT_PROBE_DEPTH_WRAP) {
        const double dn = sh_add(sh_add(sh_mul(vx, c.nx), sh_mul(vy, c.ny)), sh_mul(vz, c.nz));
        const double h = sh_mul(sh_add(1.0, -pg_div(dn, r)), 0.5);
        wrap = sh_add(sh_mul(h, h), 0.2);
    }
}

// probe_blend with t' = (t_c * cheb) * wrap in place of t_c, over the corners that are visited, present and
// have t' > 0, ascending; the irradiance formula is probe_blend's.
RT_SH_HD void depth_blend(const rt_probe_grid& G, const rt_probe_depth_params& P, const double* L, const double* D, const rt_surfel& s,
                          const ProbeCell& c, double* E, double& W)
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
        const double* Lc = L + probe_index(G, c, k) * kProbeL;
        double v[kProbeL];
        bool present = true;
        for (int j = 0; j < kProbeL; j++) {
            v[j] = Lc[j];
            present = present & pg_finite(v[j]);
        }
        if (!present) continue;
        double cheb, wrap;
        depth_corner(G, P, D, c, k, ox, oy, oz, cheb, wrap);
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
