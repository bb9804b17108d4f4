// rt_obscurance.h -- obscurance at surfels (include/rtcore.h, "obscurance at surfels", rt_obscurance): the one
// copy of a sample's falloff weight and its five terms, the fold of a sample into an entry's accumulators and
// the rule that stops on them, which the two fold kernels and the selection pass of api_obscurance.hip and the
// host twins rt_debug_obscurance_fold, rt_debug_obscurance_select and rt_debug_obscurance_error compile.
// fp64, every operation rounded on its own, as rt_probe_grid.h: sums and products through sh_add / sh_mul,
// division and square root through pg_div / pg_sqrt, no library function.
#pragma once
#include "rt_probe_grid.h"

namespace rtc {

constexpr int kObscuranceMaxPower = 8;
constexpr int kObscuranceTerms = 5; // o, o2, bent x, y, z: the five sums of an entry, in the record's order

const char* const kObscuranceParamsRule = "radius finite and above 0, power 0 .. 8, reserved 0";
inline bool obscurance_params_ok(const rt_obscurance_params* P)
{
    return P && pg_finite(P->radius) && P->radius > 0.0 && P->power >= 0 && P->power <= kObscuranceMaxPower && !P->reserved[0] &&
           !P->reserved[1] && !P->reserved[2];
}

// A sample of an invalid surfel: the reported ray's direction is all zeros.
RT_SH_HD bool obscurance_skipped(double x, double y, double z) { return x == 0.0 && y == 0.0 && z == 0.0; }

// A sample's weight w in [0, 1] from its closest hit; within: the hit lies inside the radius (a NaN distance
// does not).
RT_SH_HD double obscurance_weight(int32_t prim_id, double distance, double radius, int power, bool& within)
{
    within = prim_id >= 0 && distance < radius;
    if (!within) return 0.0;
    if (power == 0) return 1.0;
    double b = sh_add(1.0, -pg_div(distance, radius));
    b = b < 0.0 ? 0.0 : b > 1.0 ? 1.0 : b; // (a negative distance gives b above 1: held)
    double w = b;
    for (int k = 1; k < power; k++) w = sh_mul(w, b);
    return w;
}

// The five values a sample of weight w and direction (x, y, z) adds to its entry's sums: free of order, so the
// wave-per-entry kernel computes 64 samples' at once; their sums are not.
RT_SH_HD void obscurance_terms(double w, double x, double y, double z, double t[kObscuranceTerms])
{
    const double v = sh_add(1.0, -w);
    t[0] = w;
    t[1] = sh_mul(w, w);
    t[2] = sh_mul(v, x);
    t[3] = sh_mul(v, y);
    t[4] = sh_mul(v, z);
}

// One sample into an entry's accumulators, the header's accumulation step.
RT_SH_HD void obscurance_add(double radius, int power, double x, double y, double z, int32_t prim_id, double distance, double sum[kObscuranceTerms],
                             uint32_t& samples, uint32_t& hits)
{
    samples++;
    if (obscurance_skipped(x, y, z)) return;
    bool within;
    const double w = obscurance_weight(prim_id, distance, radius, power, within);
    hits += within ? 1u : 0u;
    double t[kObscuranceTerms];
    obscurance_terms(w, x, y, z, t);
#pragma unroll
    for (int j = 0; j < kObscuranceTerms; j++) sum[j] = sh_add(sum[j], t[j]);
}

// se of rtcore.h's rule from an entry's sums, n = (double)samples >= 2.  The order of operations is the header's.
// False when d is a NaN (a NaN in o or o2, or infinities that cancel): such an entry cannot converge.
// The guard is rt_probe_error.h's: o2 and o^2 / n are each n rounded additions, so their difference carries up
// to (3 n + 13) 2^-53 o2 of rounding ((n + 1) u o2 in o2's non-negative sum; (n + 5) u sum |w| <= (n + 5) u
// sqrt(n o2) in o, which o^2 / n turns into 2 (n + 5) u o2, and 2 u o2 for the square and the division);
// n 2^-49 o2 is above that for every n, and a difference not above it is rounding, not variance: v = 0.  So an
// entry whose samples all weigh the same has se == 0 exactly.
RT_SH_HD bool obscurance_error(double o, double o2, double n, double& se)
{
    const double u = sh_add(o2, -pg_div(sh_mul(o, o), n));
    const double d = pg_div(u, sh_add(n, -1.0));
    const double v = u > sh_mul(sh_mul(n, 0x1p-49), o2) ? d : 0.0; // (a NaN gives 0)
    se = pg_sqrt(pg_div(v, n));
    return d == d;
}

// active(entry) of rtcore.h; a NaN se is not above tol.
RT_SH_HD bool obscurance_active(const rt_obscurance_select_params& P, double o, double o2, uint32_t N)
{
    if (N < P.min_samples) return true;
    if (N >= P.max_samples) return false;
    if (N < 2) return true;
    double se;
    if (!obscurance_error(o, o2, (double)N, se)) return false;
    return se > P.tol;
}

} // namespace rtc
