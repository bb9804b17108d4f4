// rt_sh.h -- the nine L2 real spherical-harmonic basis functions of a direction (include/rtcore.h, "light
// probes", rt_probe_sh): the one copy of the arithmetic that the probes' fold kernel (kernels_fold.hip,
// accumulate_probes_kernel) and the host twins rt_debug_sh_basis and rt_debug_probe_fold
// (api_render_probes.hip) compile.  fp64, every operation rounded on its own: no contraction (the pragma; the
// Makefile says so too), the device side through __dmul_rn / __dadd_rn as fold_entry's moments.
#pragma once

#define RT_SH_HD __host__ __device__ inline __attribute__((always_inline))

namespace rtc {

constexpr int kShCoeffs = 9; // l = 0 .. 8 in the order Y00, Y1-1, Y10, Y11, Y2-2, Y2-1, Y20, Y21, Y22

RT_SH_HD double sh_mul(double a, double b)
{
#pragma clang fp contract(off)
#ifdef __HIP_DEVICE_COMPILE__
    return __dmul_rn(a, b);
#else
    return a * b;
#endif
}
RT_SH_HD double sh_add(double a, double b)
{
#pragma clang fp contract(off)
#ifdef __HIP_DEVICE_COMPILE__
    return __dadd_rn(a, b);
#else
    return a + b;
#endif
}

// Y[l] of the direction (x, y, z), which is taken as given (unit: the probes' is a renormalised fp32 ray
// direction widened).  The constants are sqrt(1 / 4 pi), sqrt(3 / 4 pi), sqrt(15 / 4 pi), sqrt(5 / 16 pi) and
// sqrt(15 / 16 pi) as the decimal literals rtcore.h states.
RT_SH_HD void sh_basis(double x, double y, double z, double Y[kShCoeffs])
{
    const double K0 = 0.28209479177387814, K1 = 0.48860251190291992, K2 = 1.0925484305920792;
    const double K3 = 0.31539156525252005, K4 = 0.54627421529603959;
    Y[0] = K0;
    Y[1] = sh_mul(K1, y);
    Y[2] = sh_mul(K1, z);
    Y[3] = sh_mul(K1, x);
    Y[4] = sh_mul(sh_mul(K2, x), y);
    Y[5] = sh_mul(sh_mul(K2, y), z);
    Y[6] = sh_mul(K3, sh_add(sh_mul(sh_mul(3.0, z), z), -1.0));
    Y[7] = sh_mul(sh_mul(K2, x), z);
    Y[8] = sh_mul(K4, sh_add(sh_mul(x, x), -sh_mul(y, y)));
}

} // namespace rtc
