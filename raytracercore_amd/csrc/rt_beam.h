// rt_beam.h -- a beam's sample ray (include/rtcore.h, "radiance queries", rt_beam): the one copy of
// the arithmetic that the BEAMS instances of the path kernels (kernels_path.hip, refill) and the host
// twin rt_debug_beam_rays (api_render_beams.hip) compile.  fp32, every operation rounded on its own:
// no contraction (the pragma; the Makefile says so too), IEEE square root and division on both sides.
// Included after rt_kernels.h (double2 comes from the HIP runtime header, or from hiprtc itself).
#pragma once

#define RT_BEAM_HD __host__ __device__ inline __attribute__((always_inline))

namespace rtc {

constexpr int kBeamRows = 12; // sizeof(rt_beam) / 16

struct BeamV {
    float x, y, z;
};
enum BeamSample : int { BEAM_RAY = 0, BEAM_DEGENERATE = 1, BEAM_INVALID = 2 };

RT_BEAM_HD bool beam_finite(float x, float y, float z)
{
    const float inf = __builtin_huge_valf(); // (every compare is false for NaN)
    return (__builtin_fabsf(x) < inf) & (__builtin_fabsf(y) < inf) & (__builtin_fabsf(z) < inf);
}

// One of the beam's two vectors at (u, v): p + u * pu + v * pv per component, each of the three given
// as its two 16-B rows (xy, zw) and rounded to fp32 component by component.  false: one of the twelve
// doubles is not finite, or one of the nine used ones is not after the rounding (a double that is not
// finite is not finite as a float either, so those are tested once).
RT_BEAM_HD bool beam_vector(double2 p0, double2 p1, double2 u0, double2 u1, double2 v0, double2 v1, float u, float v, BeamV& out)
{
#pragma clang fp contract(off)
    const float px = (float)p0.x, py = (float)p0.y, pz = (float)p1.x;
    const float ux = (float)u0.x, uy = (float)u0.y, uz = (float)u1.x;
    const float vx = (float)v0.x, vy = (float)v0.y, vz = (float)v1.x;
    out.x = (px + u * ux) + v * vx;
    out.y = (py + u * uy) + v * vy;
    out.z = (pz + u * uz) + v * vz;
    const double inf = __builtin_huge_val();
    return (__builtin_fabs(p1.y) < inf) & (__builtin_fabs(u1.y) < inf) & (__builtin_fabs(v1.y) < inf) &
           beam_finite(px, py, pz) & beam_finite(ux, uy, uz) & beam_finite(vx, vy, vz);
}

RT_BEAM_HD float beam_div(float a, float b)
{
#ifdef __HIP_DEVICE_COMPILE__
    return __fdiv_rn(a, b);
#else
    return a / b;
#endif
}

// The ray of the sample at (u, v) of the footprint of the beam at rows[0 .. 11] (an rt_beam: origin,
// direction, origin_du, origin_dv, direction_du, direction_dv).  BEAM_RAY: o and d are the ray.
// BEAM_DEGENERATE: this sample is a primary miss.  BEAM_INVALID: every sample of the beam is.
// The kernel reads the origin's six rows and then the direction's, not all twelve at once: 48
// registers of rows in flight spilled every instance that calls this.
RT_BEAM_HD BeamSample beam_sample(const double2* __restrict__ rows, float u, float v, BeamV& o, BeamV& d)
{
#pragma clang fp contract(off)
    int valid = beam_vector(rows[0], rows[1], rows[4], rows[5], rows[6], rows[7], u, v, o) ? 1 : 0;
#ifdef __HIP_DEVICE_COMPILE__
    asm volatile("" : "+v"(o.x), "+v"(o.y), "+v"(o.z), "+v"(valid) : : "memory"); // (the next loads start after these)
#endif
    BeamV w;
    valid &= beam_vector(rows[2], rows[3], rows[8], rows[9], rows[10], rows[11], u, v, w) ? 1 : 0;
    if (!valid) return BEAM_INVALID;
    const float n2 = (w.x * w.x + w.y * w.y) + w.z * w.z;
    if (!((n2 > 0.0f) & (n2 < __builtin_huge_valf()) & beam_finite(o.x, o.y, o.z))) return BEAM_DEGENERATE; // (NaN fails the compares)
    const float len = __builtin_sqrtf(n2);
    d.x = beam_div(w.x, len);
    d.y = beam_div(w.y, len);
    d.z = beam_div(w.z, len);
    return BEAM_RAY;
}

} // namespace rtc
