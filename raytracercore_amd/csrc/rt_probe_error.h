// rt_probe_error.h -- the second moments of a light probe's band-0/1 luminance coefficients and the rule
// that stops on them (include/rtcore.h, "adaptive light probes", rt_probe_moments, rt_probe_select_params):
// the one copy of the arithmetic that the probes' list fold (kernels_fold.hip, accumulate_probe_list_kernel),
// the selection pass (api_probe_list.hip) and the host twins rt_debug_probe_moments, rt_debug_probe_error and
// rt_debug_probe_select compile.  fp64, every operation rounded on its own, as rt_sh.h, whose sh_mul and
// sh_add carry every product and sum here; division and square root are IEEE on both sides.
#pragma once

#include "../../include/rtcore.h"
#include "rt_sh.h"

#ifndef __HIP_DEVICE_COMPILE__
#include <cmath>
#endif

namespace rtc {

constexpr int kProbeMomentRows = 4; // l = 0 .. 3: bands 0 and 1, in the order of Y0 .. Y3

RT_SH_HD double probe_div(double a, double b)
{
#ifdef __HIP_DEVICE_COMPILE__
    return __ddiv_rn(a, b);
#else
    return a / b;
#endif
}
RT_SH_HD double probe_sqrt(double a)
{
#ifdef __HIP_DEVICE_COMPILE__
    return __dsqrt_rn(a);
#else
    return std::sqrt(a);
#endif
}

// 0.299 r + 0.587 g + 0.114 b, left to right (rt_render_pixels' Y_j)
RT_SH_HD double probe_luminance(double r, double g, double b)
{
    return sh_add(sh_add(sh_mul(0.299, r), sh_mul(0.587, g)), sh_mul(0.114, b));
}

// One sample's update of the moments held as two columns m0 (hits) and m1 (primary misses); Y: the basis of
// the sample's direction (rt_sh.h), of which rows 0 .. 3 are read.
RT_SH_HD void probe_moments_hit(double m0[kProbeMomentRows], float r, float g, float b, const double* Y)
{
    const double y = probe_luminance((double)r, (double)g, (double)b);
#pragma unroll
    for (int l = 0; l < kProbeMomentRows; l++) {
        const double x = sh_mul(y, Y[l]);
        m0[l] = sh_add(m0[l], sh_mul(x, x));
    }
}
RT_SH_HD void probe_moments_miss(double m1[kProbeMomentRows], const double* Y)
{
#pragma unroll
    for (int l = 0; l < kProbeMomentRows; l++) m1[l] = sh_add(m1[l], sh_mul(Y[l], Y[l]));
}

// se and level of rtcore.h's rule from a probe's accumulators: c = its rt_probe_sh (rows 0 .. 3 are read),
// m = its rt_probe_moments, n = (double)(samples + misses) >= 2.  The order of operations is the header's.
// False when a d_l is NaN (a NaN in c or m, or infinities that cancel): such a probe cannot converge.
// The guard: T_l and S_l^2 / n are each n rounded additions, so their difference carries up to (3 n + 13) 2^-53 T_l
// of rounding ((n + 1) u T_l in T_l's non-negative sum; (n + 5) u sum |x| <= (n + 5) u sqrt(n T_l) in S_l, which
// S_l^2 / n turns into 2 (n + 5) u T_l, and 2 u T_l for the square and the division); n 2^-49 T_l is above that
// for every n, and a difference not above it is rounding, not variance: v_l = 0.
RT_SH_HD bool probe_error(const rt_color& ambient, const double* c, const double* m, double n, double& se, double& level)
{
    const double PI = 3.141592653589793, K0 = 0.28209479177387814, K1 = 0.48860251190291992;
    const double A = probe_luminance(ambient.r, ambient.g, ambient.b);
    const double AA = sh_mul(A, A);
    const double nm1 = sh_add(n, -1.0);
    double S0 = 0.0, v[kProbeMomentRows];
    bool ok = true;
#pragma unroll
    for (int l = 0; l < kProbeMomentRows; l++) {
        const double S = sh_add(probe_luminance(c[4 * l], c[4 * l + 1], c[4 * l + 2]), sh_mul(A, c[4 * l + 3]));
        const double T = sh_add(m[2 * l], sh_mul(AA, m[2 * l + 1]));
        const double num = sh_add(T, -probe_div(sh_mul(S, S), n));
        const double d = probe_div(num, nm1);
        v[l] = num > sh_mul(sh_mul(n, 0x1p-49), T) ? d : 0.0; // (a NaN gives 0)
        ok = ok && d == d;
        if (l == 0) S0 = S;
    }
    const double a0 = sh_mul(PI, K0), a1 = sh_mul(2.0943951023931953, K1), four_pi = sh_mul(4.0, PI);
    level = probe_div(sh_mul(sh_mul(four_pi, a0), S0), n);
    const double var = sh_add(sh_mul(sh_mul(a0, a0), v[0]), sh_mul(sh_mul(a1, a1), sh_add(sh_add(v[1], v[2]), v[3])));
    se = sh_mul(four_pi, probe_sqrt(probe_div(var, n)));
    return ok;
}

// active(probe) of rtcore.h.  A NaN in c or m makes a d_l NaN, and the probe inactive; the two conditionals
// are written so that a NaN level takes irr_floor and a NaN se is not above the threshold.
RT_SH_HD bool probe_active(const rt_probe_select_params& P, const double* c, uint32_t ns, uint32_t nm, const double* m)
{
    const uint64_t N = (uint64_t)ns + (uint64_t)nm;
    if (N < P.min_samples) return true;
    if (N >= P.max_samples) return false;
    if (N < 2) return true;
    double se, level;
    if (!probe_error(P.ambient, c, m, (double)N, se, level)) return false;
    const double lv = level > P.irr_floor ? level : P.irr_floor;
    return se > sh_mul(P.rel_tol, lv);
}

} // namespace rtc
