// rt_surfel.h -- a surfel's sample ray (include/rtcore.h, "radiance queries", rt_surfel): the one copy
// of the arithmetic that the SURFELS instances of the path kernels (kernels_path.hip, refill) and the
// kernel behind rt_debug_surfel_rays_device (api_render_surfels.hip) compile.  The direction is drawn by
// the functions shade()'s diffuse bounce runs, so they live here too, with the fp32 vector they are
// written in: kernels_path.hip has no other copy.  Device code only.  surfel_sample is fp32 with every
// operation rounded on its own: no contraction (the pragma; the Makefile says so too), every fused
// multiply-add written out, IEEE square root and division for the normal; the hardware's reciprocal
// square root, square root, sine and cosine give one result per input wherever they are compiled.
// Included after rt_kernels.h (double2 comes from the HIP runtime header, or from hiprtc itself).
#pragma once
#include "rt_beam.h"

namespace rtc {

struct V3 {
    float x, y, z;
};
__device__ __forceinline__ V3 v3(float x, float y, float z) { return V3{x, y, z}; }
__device__ __forceinline__ V3 operator*(V3 a, float s) { return {a.x * s, a.y * s, a.z * s}; }
__device__ __forceinline__ float dot(V3 a, V3 b) { return fmaf(a.x, b.x, fmaf(a.y, b.y, a.z * b.z)); }
// kfma: a product with a scene or camera field, which the scene-specialised build of kernels_path.hip
// drops when the field is a literal zero (known_zero, defined in rt_trace.h before it includes this header and
// announced by RT_HAVE_KNOWN_ZERO); nothing is known anywhere else.
#ifndef RT_HAVE_KNOWN_ZERO
__device__ __forceinline__ bool known_zero(float) { return false; }
#endif
__device__ __forceinline__ float kfma(float a, float b, float c) { return (known_zero(a) || known_zero(b)) ? c : fmaf(a, b, c); }
__device__ __forceinline__ V3 cross(V3 a, V3 b)
{
    return {fmaf(a.y, b.z, -a.z * b.y), fmaf(a.z, b.x, -a.x * b.z), fmaf(a.x, b.y, -a.y * b.x)};
}
__device__ __forceinline__ V3 madd(V3 a, float s, V3 c) { return {kfma(a.x, s, c.x), kfma(a.y, s, c.y), kfma(a.z, s, c.z)}; }
__device__ __forceinline__ float fsqrt(float x) { return __builtin_amdgcn_sqrtf(x); }

// Vec4D.CreateHorizon(pole, z, theta) (Vec4D.cs:52-58) as the equivalent Rodrigues form:
// pole*z + (c*cos(theta) + (pole x c)*sin(theta)) * s, c = normalize(pole x z^) or x^.
// The frame (c, pole x c) depends on the pole only, so one bounce builds it once for both
// the rough normal and the diffuse direction (both turn about the hit normal).
struct Frame {
    V3 c, bn;
};
__device__ __forceinline__ Frame make_frame(V3 pole)
{
    V3 c = v3(pole.y, -pole.x, 0.0f);
    const float cl = fmaf(c.x, c.x, c.y * c.y);
    c = (cl == 0.0f) ? v3(1.0f, 0.0f, 0.0f) : c * __builtin_amdgcn_rsqf(cl);
    return Frame{c, cross(pole, c)};
}
__device__ __forceinline__ V3 horizon(const Frame& f, V3 pole, float z, float s, float turn)
{
    const float cs = __builtin_amdgcn_cosf(turn), sn = __builtin_amdgcn_sinf(turn); // argument in turns
    const V3 h = madd(f.c, cs, f.bn * sn);
    return madd(h, s, pole * z);
}

// 2 * acos(u) / pi for u in [0, 1): sqrt(1 - u) * P(u), the degree-7 fit of Abramowitz &
// Stegun 4.4.46 (|error| <= 2e-8 rad) scaled by 2 / pi; as accurate as fp32 acosf here.
__device__ __forceinline__ float acos_turn2(float u)
{
    float p = fmaf(u, -0.0008037268f, 0.0042463113f);
    p = fmaf(u, p, -0.0108786384f);
    p = fmaf(u, p, 0.0196663830f);
    p = fmaf(u, p, -0.0319419540f);
    p = fmaf(u, p, 0.0566457845f);
    p = fmaf(u, p, -0.1366178393f);
    p = fmaf(u, p, 1.0f);
    return fsqrt(1.0f - u) * p;
}

// The ray of a gather sample of the surfel at rows[0 .. 3] (an rt_surfel: position xy, zw, normal xy,
// zw), u1 and u2 the sample's first two draws: o the position rounded to fp32, d a direction about the
// normalised normal, its cosine z by mode (rt_gather_mode; wave-uniform in the kernels) and its turn
// about the normal u2, made as shade() makes a diffuse bounce's and renormalised by the one Newton
// step shade() applies.  false: the surfel is invalid (a double that is not finite, a component that is
// not after the rounding, a normal of squared length zero or not finite); o and d are then not set.
__device__ __forceinline__ bool surfel_sample(const double2* __restrict__ rows, int mode, float u1, float u2, V3& o, V3& d)
{
#pragma clang fp contract(off)
    const double2 r0 = rows[0], r1 = rows[1], r2 = rows[2], r3 = rows[3];
    const V3 p = v3((float)r0.x, (float)r0.y, (float)r1.x);
    const V3 n = v3((float)r2.x, (float)r2.y, (float)r3.x);
    const float n2 = (n.x * n.x + n.y * n.y) + n.z * n.z;
    const double inf = __builtin_huge_val(); // (every compare is false for NaN; a double that is not finite is not as a float either)
    if (!((__builtin_fabs(r1.y) < inf) & (__builtin_fabs(r3.y) < inf) & beam_finite(p.x, p.y, p.z) & beam_finite(n.x, n.y, n.z) &
          (n2 > 0.0f) & (n2 < __builtin_huge_valf())))
        return false;
    const float len = __builtin_sqrtf(n2);
    const V3 pole = v3(beam_div(n.x, len), beam_div(n.y, len), beam_div(n.z, len));
    float z;
    if (mode == RT_GATHER_DIFFUSE) z = acos_turn2(u1); // 2 acos(U) / pi (Raytracer.cs:215)
    else if (mode == RT_GATHER_COSINE) z = fsqrt(1.0f - u1);
    else z = fmaf(-2.0f, u1, 1.0f); // (exact: u1 is a multiple of 2^-24)
    const float s = fsqrt(fmaxf(0.0f, fmaf(-z, z, 1.0f)));
    const V3 dir = horizon(make_frame(pole), pole, z, s, u2);
    o = p;
    d = dir * fmaf(-0.5f, dot(dir, dir), 1.5f); // shade()'s renormalisation of a bounce direction
    return true;
}

} // namespace rtc
