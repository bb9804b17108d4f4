// kernels_path.hip -- the persistent fp32 path-tracing kernel for gfx950.
//
// One launch renders `spp` samples for every pixel of a tile.  Work items are
// (sample chunk, pixel) pairs dealt out by a wave-aggregated atomic; each lane owns one item
// at a time and regenerates a new camera path the iteration after its previous path ends,
// so every loop iteration issues exactly one closest-hit query (Scene.RayTrace) per live
// lane.  Per item the lane accumulates its chunk's samples in registers and writes one
// 16-byte partial; a second kernel folds the partials into fp64 accumulators in a fixed
// order, so results do not depend on scheduling.
//
// Per path this restates Raytracer.GetCameraRay + GetColor (Raytracer.cs:51-287):
//   camera jitter and depth of field, the bounce loop with RandomShine (rough normal),
//   Fresnel / total internal reflection, the luminance-weighted transmit / specular /
//   diffuse / emission choice, tint *= colour * max(totalLum, 1), and the miss rules
//   (primary miss -> Placeholder/miss, secondary miss -> AmbientRGB untinted).
//
// What is where:
//   rt_trace.h         the closest-hit / any-hit query itself (hit tests, trace_brute, the node visits,
//                      walk_step), shared with the ray-list kernels
//   this file          the path code on top of it (camera, shade, refill, bounce), path_body and the two
//                      megakernels path_kernel / path_kernel_bvh, rt_path_const for a scene-specialised
//                      build, and in the trailing host block pick, fill_launch and launch_path
//   kernels_query.hip  the ray-list kernels (trace_rays, query, occluded, occluded_surfels)
//   kernels_fold.hip   the folds of the partials this file's kernels write, tonemap, the host layouts,
//                      the pixel keys and the leaf compaction; no ray is traced there
// Only this file and rt_trace.h are sources of a scene-specialised build (rt_jit.cpp embeds them).
#include "../../include/rtcore_rng.h"
#include "rt_kernels.h"
#include "rt_beam.h"
#ifdef RT_SCENE_CONST
// rt_jit.cpp generates this header per scene (and camera, for the grouped order): the launch's
// PathScene and its brute-force records as 32-bit words (kSceneW, kGroupsW, kRectsW, kFramesW,
// kTestsW, kXfW, kCameraW) and the camera switches (RT_SCENE_CAMERA_KIND / _DOF).  Every record
// field then folds into the instructions (literal operands cost what a VGPR operand does on
// gfx950, an SGPR operand twice that), the primitive loops unroll and the per-record flag branches
// resolve at compile time.  Included first, so that every macro it defines is seen by the code.
#include "rt_scene_const.h"
#endif
#include "rt_trace.h"

namespace rtc {
namespace {

// The scene bound (PathScene::bound_lo / _hi, make_scene_bound): does the ray meet the padded box of
// every primitive but the planes, ahead of its origin?  The slab test in trace_brute's own terms (its
// 1 / d and o / d, which the compiler shares with the query where one follows).  The pad covers the
// test's fp32 error for origins up to bound_limit; an origin past it counts as meeting the box, and so
// does a ray with a NaN or an infinity in it (every compare below is written to fail for NaN).  A
// scene without bounded primitives has an empty bound, which no ray meets.
template <class SceneT>
__device__ __forceinline__ bool scene_meets(const SceneT& s, V3 o, V3 d)
{
    const V3 id = v3(slab_rcp_lean(d.x), slab_rcp_lean(d.y), slab_rcp_lean(d.z));
    const V3 oi = o * id;
    const float tx0 = fmaf(s.bound_lo[0], id.x, -oi.x), tx1 = fmaf(s.bound_hi[0], id.x, -oi.x);
    const float ty0 = fmaf(s.bound_lo[1], id.y, -oi.y), ty1 = fmaf(s.bound_hi[1], id.y, -oi.y);
    const float tz0 = fmaf(s.bound_lo[2], id.z, -oi.z), tz1 = fmaf(s.bound_hi[2], id.z, -oi.z);
    const float tmin = fmaxf(fmaxf(fminf(tx0, tx1), fminf(ty0, ty1)), fmaxf(fminf(tz0, tz1), 0.0f));
    const float tmx = fminf(fminf(fmaxf(tx0, tx1), fmaxf(ty0, ty1)), fmaxf(tz0, tz1));
    const bool near = fabsf(o.x) + fabsf(o.y) + fabsf(o.z) <= s.bound_limit; // false for a NaN origin
    const bool finite = fabsf(d.x + d.y + d.z) < __builtin_huge_valf();      // false for a NaN or infinite d
    return (!(tmin > tmx) | !near | !finite) & (s.bound_empty == 0);
}

struct Counters {
    unsigned nodes, tris, sphs;                                  // per lane
    unsigned ovf_pushes, max_sp;                                 // per lane: stack entries written past the LDS part; deepest stack
    unsigned outer;                                              // per lane: faces of the BVH order's outer group tested
    unsigned q_steps, max_steps;                                 // per lane: steps of the current / longest query
    unsigned long long cyc_start, cyc_trace, cyc_shade, iters; // per wave (uniform)
};

// q = x / d, r = x % d through the fp32 reciprocal plus one correction step (exact for the
// quotients used here, all far below 2^22).
__device__ __forceinline__ void divmod(unsigned x, unsigned d, float inv_d, unsigned& q, unsigned& r)
{
    q = (unsigned)((float)x * inv_d);
    r = x - q * d;
    if ((int)r < 0) {
        q--;
        r += d;
    } else if (r >= d) {
        q++;
        r -= d;
    }
}

struct Sample {
    V3 o, d, tint;
    int bounce;
    int prev;
    rt_rng rng;
};

__device__ __forceinline__ float next_u(rt_rng& r) { return rt_rng_next_float(&r); }

struct Ray3 {
    V3 o, d;
};
// The camera's kind and depth-of-field switch: compile-time constants in a camera-independent
// scene-specialised build (rt_jit.cpp), else read from the camera record.
template <class CamT>
__device__ __forceinline__ bool cam_frustum(const CamT& c)
{
#ifdef RT_SCENE_CAMERA_KIND
    (void)c;
    return RT_SCENE_CAMERA_KIND == RT_CAMERA_FRUSTUM;
#else
    return c.kind == RT_CAMERA_FRUSTUM;
#endif
}
template <class CamT>
__device__ __forceinline__ bool cam_dof(const CamT& c)
{
#ifdef RT_SCENE_CAMERA_DOF
    (void)c;
    return RT_SCENE_CAMERA_DOF != 0;
#else
    return c.dof != 0.0f;
#endif
}
template <class CamT> // CameraF, or CameraF in the constant address space (scalar loads)
__device__ __forceinline__ Ray3 camera_ray(const CamT& c, float x, float y)
{
    Ray3 r;
    if (cam_frustum(c)) {
        const float ox = fmaf(x, c.tan_x_per_px, -c.tan_x); // tan_x * (x - w2) / w2
        const float oy = fmaf(y, c.tan_y_per_px, -c.tan_y);
        r.d = normalize(madd(xyz(c.up), oy, madd(xyz(c.side), ox, xyz(c.look))));
        r.o = xyz(c.position);
    } else {
        r.o = madd(xyz(c.up), (y - c.h2) * c.v_mult, madd(xyz(c.side), (x - c.w2) * c.h_mult, xyz(c.position)));
        r.d = normalize(xyz(c.look));
    }
    r.o = madd(r.d, c.image_plane, r.o);
    return r;
}

// Raytracer.GetCameraRay (Raytracer.cs:262-282)
// LEAN (the brute-force kernels): x + U as one fma of the integer draw (U = h * 2^-24 exactly, so the
// single rounding is the add's: the same value); the BVH kernels keep the add (their register
// allocation moved spills into the traversal loop with it, C4 44.4 -> 55.9 ms)
// sample_point: the sample's point in its pixel, subX and subY (the start rows' loop in refill
// draws them the same way)
template <bool LEAN>
__device__ __forceinline__ void sample_point(int x, int y, Sample& S, float& sx, float& sy)
{
    sx = LEAN ? fmaf((float)rt_rng_next24(&S.rng), 0x1p-24f, (float)x) : (float)x + next_u(S.rng);
    sy = LEAN ? fmaf((float)rt_rng_next24(&S.rng), 0x1p-24f, (float)y) : (float)y + next_u(S.rng);
}
template <bool LEAN = false, class CamT>
__device__ __forceinline__ void start_sample(const CamT& cam, int x, int y, Sample& S)
{
    float sx, sy;
    sample_point<LEAN>(x, y, S, sx, sy);
    const Ray3 r = camera_ray(cam, sx, sy);
    S.o = r.o;
    S.d = r.d;
    if (cam_dof(cam)) {
        const V3 focus = madd(r.d, cam.focal_length - cam.image_plane, r.o);
        const float dist = fsqrt(next_u(S.rng)) * cam.dof;
        const float turn = next_u(S.rng);
        const float ox = __builtin_amdgcn_cosf(turn) * dist, oy = __builtin_amdgcn_sinf(turn) * dist;
        const Ray3 r2 = camera_ray(cam, sx + ox, sy + oy);
        S.o = r2.o;
        S.d = normalize(focus - r2.o);
    }
    S.tint = v3(1.0f, 1.0f, 1.0f);
    S.bounce = 0;
    S.prev = -1;
}

// 1 - z^2 for z = 2^a (a <= 0) without cancellation: 1 - 2^(2a) = -expm1(2a ln 2) by its series
// near z = 1, else directly; both forms evaluated and selected (no divergent branch).  LEAN (the
// brute-force kernels) takes the direct form as 1 - z z from the z already computed (z^2 <= 0.958
// there, so the product's rounding costs a few ulp of the difference) instead of a second exp2.
template <bool LEAN>
__device__ __forceinline__ float one_minus_exp2_2a(float a, float z)
{
    const float x = 2.0f * a * 0.69314718055994531f;
    const float series = -x * fmaf(x, fmaf(x, fmaf(x, 1.0f / 24.0f, 1.0f / 6.0f), 0.5f), 1.0f);
    const float direct = LEAN ? fmaf(-z, z, 1.0f) : 1.0f - __builtin_amdgcn_exp2f(2.0f * a);
    return x > -0.0625f ? series : direct;
}

// Triangle.RayTraceAVXFaster (Triangle.cs:77-146) in fp64, in the reference's operation order
// (FMA crosses, hadd sums), on the ray that leaves a vertex-normal triangle from its own hit
// point o = fma(e01, u, fma(e02, v, v0)) (Triangle.cs:131).  The reference's next query meets the
// same triangle at t ~ 0 whenever the rounding residual of t is >= 0; RayHitMatches then decides
// whether that is the same hit (Util.cs:179-192).  For a flat triangle it always is (the face
// normal and the geometric side agree); a smooth normal (Triangle.GetNormal, :209-224) can send the
// ray under the geometric surface, and then it is not.  The kernel evaluates the same fp64
// expression on its own hit point.
__host__ __device__ __noinline__ bool vn_rehit_test(const PrimD& P, double u, double v, V3 dir, bool& inside,
                                                   double* t_out = nullptr, double* o_out = nullptr)
{
    const Vec4d a = P.a, e1 = P.b, e2 = P.c;
    const double d[4] = {(double)dir.x, (double)dir.y, (double)dir.z, 0.0};
    const double o[4] = {__builtin_fma(e1.x, u, __builtin_fma(e2.x, v, a.x)), __builtin_fma(e1.y, u, __builtin_fma(e2.y, v, a.y)),
                         __builtin_fma(e1.z, u, __builtin_fma(e2.z, v, a.z)), __builtin_fma(e1.w, u, __builtin_fma(e2.w, v, a.w))};
    const double off[4] = {o[0] - a.x, o[1] - a.y, o[2] - a.z, o[3] - a.w};
    const double b1[4] = {e1.x, e1.y, e1.z, e1.w}, c2[4] = {e2.x, e2.y, e2.z, e2.w};
    auto crs = [](const double* l, const double* r, double* out) { // SIMDHelpers.Cross
        out[0] = __builtin_fma(l[1], r[2], -(l[2] * r[1]));
        out[1] = __builtin_fma(l[2], r[0], -(l[0] * r[2]));
        out[2] = __builtin_fma(l[0], r[1], -(l[1] * r[0]));
        out[3] = __builtin_fma(l[3], r[3], -(l[3] * r[3]));
    };
    auto hs = [](const double* x, const double* y) { return (x[0] * y[0] + x[1] * y[1]) + (x[2] * y[2] + x[3] * y[3]); };
    double s1[4], s2[4];
    crs(off, b1, s1);
    crs(d, c2, s2);
    const double uu = hs(off, s2), vv = hs(d, s1), tt = hs(c2, s1), det = hs(b1, s2);
    const double inv = 1.0 / det;
    const double invz = (inv == inv) ? inv : 0.0;
    const double u2 = uu * invz, v2 = vv * invz, t2 = tt * invz;
    bool rej = (u2 < 0) | (v2 < 0) | (t2 < 0);
    rej |= (P.flags & F_MIRROR) ? ((u2 > 1) | (v2 > 1)) : ((u2 + v2) > 1);
    inside = invz < 0;
    if (t_out) *t_out = t2;
    if (o_out) {
        o_out[0] = o[0];
        o_out[1] = o[1];
        o_out[2] = o[2];
    }
    return !rej;
}

// Raytracer.cs:74-75: `if (i % 3 == 0) ray = Ray.Directional(...)` at the start of bounce i.  Here
// i <= Recursion; for the (usual) recursion depths below 32 the brute-force kernels test one bit of a
// constant.  The BVH kernels (SLOT) take the plain remainder: the bit test's extra scene read moved
// their register spills (C4 wide kernel 17 -> 23 VGPRs spilled).
template <bool SLOT, class SceneT>
__device__ __forceinline__ bool renormalise_at(const SceneT& s, int i)
{
    if (SLOT) return (unsigned)i % 3u == 0u;
    return s.recursion < 32 ? ((0x49249249u >> (unsigned)i) & 1u) != 0 : (unsigned)i % 3u == 0u;
}

// The closest hit a query starts from: none, or the re-hit of a vertex-normal triangle that
// shade() found the reference makes (encoded in Sample.prev <= -2 as -2 - sg).
template <bool VN, class SceneT>
__device__ __forceinline__ Best query_start(const SceneT& s, int prev)
{
    if (VN && s.n_vn > 0 && prev <= -2) return Best{0.0f, -2 - prev};
    return Best{__builtin_huge_valf(), -1};
}

// What rt_trace_paths records of one bounce (rt_debug_ray, rtcore.h) beyond the ray and the tint,
// which bounce() holds: filled by shade<..., REC = true> where GetColor sets debugRay.Type and
// FresnelRatio (Raytracer.cs:79-223).
struct BounceRec {
    int prim_id, type, inside;
    float distance, fresnel, cos_in;
    V3 pos, nrm;
};
// bounce() writes the record as kRecRows float4 rows: the offsets rtcore.h documents
static_assert(sizeof(rt_debug_ray) == 16 * kRecRows && __builtin_offsetof(rt_debug_ray, distance) == 12 &&
                  __builtin_offsetof(rt_debug_ray, fresnel) == 16 && __builtin_offsetof(rt_debug_ray, bounce) == 24 &&
                  __builtin_offsetof(rt_debug_ray, position) == 32 && __builtin_offsetof(rt_debug_ray, normal) == 44 &&
                  __builtin_offsetof(rt_debug_ray, origin) == 56 && __builtin_offsetof(rt_debug_ray, direction) == 68 &&
                  __builtin_offsetof(rt_debug_ray, tint) == 80,
              "rt_debug_ray layout");

// One bounce of Raytracer.GetColor after the closest-hit query.  Returns 0 to continue the
// path, 1 if the sample ended with colour `col`, 2 if it ended as a miss (Placeholder).
// REC (the instrumented instances, for rt_trace_paths): *rec receives the bounce's record.  The
// two returns of GetColor that come before the hit's position and normal are needed (DebugGeom,
// the recursion limit) are then taken after them, so that the record holds both; nothing in
// between draws a number or changes the sample.
template <bool VN, bool PIN = false, bool SLOT = false, bool REC = false, class SceneT, class VnP, class TestP>
__device__ __forceinline__ int shade(const SceneT& s, const PrimF* __restrict__ prims, const MatF* __restrict__ mats,
                                     const XformF* __restrict__ xfs, VnP vnormals, TestP tests, const PrimD* prims_d,
                                     const Best& b, Sample& S, V3& col, [[maybe_unused]] BounceRec* rec = nullptr)
{
    if constexpr (REC) {
        const float nan = __builtin_nanf("");
        *rec = BounceRec{-1, RT_BOUNCE_MISSED, 0, 0.0f, nan, nan, v3(0.0f, 0.0f, 0.0f), v3(0.0f, 0.0f, 0.0f)};
    }
    if (b.sg < 0) {
        if (S.bounce == 0 || s.ambient_miss) return 2;
        col = v3(s.ambient_r, s.ambient_g, s.ambient_b);
        return 1;
    }
    bool gin = (b.sg & 1) != 0;
    PrimF P = prims[b.sg >> 1];
    if (PIN) { // records from global memory: every field in flight at once (see pin_rec)
        pin4(P.a);
        pin4(P.b);
        pin4(P.d);
    }
    const uint32_t fl = __float_as_uint(P.b.w);
    const int id = __float_as_int(P.a.w);
    const MatF& M = mats[__float_as_int(P.d.w)]; // the primitive's material (deduplicated table)
    const uint32_t kind = fl & KIND_MASK;
    const V3 emis = xyz(M.emission);
    if constexpr (!REC) {
        if (s.debug_geom) { // Raytracer.cs:93-98
            col = xyz(M.specular) + xyz(M.diffuse) + emis;
            return 1;
        }
        if (S.bounce >= s.recursion) {
            col = S.tint * emis;
            return 1;
        }
    }
    // hit position and normal facing the incoming ray: one straight-line form for every kind
    // (world point o + t d), with transformed spheres and vertex-normal triangles on a separate
    // (rare) path.  The rectangle tests do not track the side of their hit, so a rectangle's
    // Inside is recomputed here (Moller-Trumbore's inside = d . N > 0), and an axis-aligned one's
    // hit point is put on its plane.
    V3 pos = madd(S.d, b.t, S.o);
    const bool sph = (s.facts & FACT_SPHERE) && kind == RT_PRIM_SPHERE;
    V3 n;
    float nk; // 1 / |n| of a sphere's normal, applied with the turn toward the ray (below)
    if (SLOT) { // the BVH kernels (records in global memory: the three rows a, b, d only)
        const uint32_t axis = (fl & F_AXIS_MASK) >> F_AXIS_SHIFT; // axis-aligned rectangle: on its plane
        if (axis | (fl & F_FRAME_RECT)) gin = dot(S.d, xyz(P.d)) > 0.0f;
        pos.x = axis == 1 ? P.a.x : pos.x;
        pos.y = axis == 2 ? P.a.y : pos.y;
        pos.z = axis == 3 ? P.a.z : pos.z;
        n = sph ? (pos - xyz(P.a)) * P.b.y : xyz(P.d);
        nk = sph ? fmaf(-0.5f, dot(n, n), 1.5f) : 1.0f;
    } else { // the brute-force kernels (records in LDS): the same by arithmetic on the shading row c
        // c.xyz: one-hot plane axis of an axis-aligned rectangle (the hit point moves onto the plane
        // through v0 = P.a), c.w: 1/r of a sphere, whose P.d holds -centre/r (normal = p/r - c/r), 0
        // for the flat kinds, whose P.d is the face normal
        const float4 Pc = prims[b.sg >> 1].c;
        pos = v3(fmaf(Pc.x, P.a.x - pos.x, pos.x), fmaf(Pc.y, P.a.y - pos.y, pos.y), fmaf(Pc.z, P.a.z - pos.z, pos.z));
        n = madd(pos, Pc.w, xyz(P.d));
        // No select here, which rests on what scene_records.cpp puts into row d of a flat kind: a
        // triangle's face normal, normalised in fp64 and rounded (|n|^2 within 2e-7 of 1, so nk is 1 or 1
        // -+ an ulp; the BVH form above takes exactly 1), a plane's Normal, unit by the ABI (rtcore.h), or
        // zero (a vertex-normal triangle, a transformed sphere: nk = 1.5 on n = 0, both replaced below).
        nk = fmaf(-0.5f, dot(n, n), 1.5f);
        if (fl & (F_AXIS_MASK | F_FRAME_RECT)) gin = dot(S.d, xyz(P.d)) > 0.0f;
    }
    // The sphere test takes |d| = 1 as Sphere.cs does, and between the renormalising bounces an fp32
    // direction drifts from unit length by up to 5e-6 (most after a refraction near the critical
    // angle).  The hit point then lies off the sphere (the self-hit's far root -2 oc.d by 2 |oc.d| times
    // the drift) and p/r - c/r is off unit length by up to 2e-5, which cos_in carries and the Fresnel
    // ratio and the refracted ray magnify near the critical angle (measured 2e-4 and 3e-4 against the
    // fp64 step).  One Newton step of 1/|n| (relative error (|n|^2 - 1)^2) brings it back: nk, which
    // multiplies n together with the sign that turns it toward the ray.
    float bu = 0.0f, bv = 0.0f; // vertex-normal triangle: the barycentrics of the hit
    if ((s.facts & (FACT_XF | FACT_VN)) && (fl & (F_TRANSFORMED | F_HASNORMALS))) {
        if (sph) { // ellipsoid: the world normal is an affine map of the world hit point
            n = normalize(xf_point(xfs[__float_as_int(P.b.z)].normal, pos));
            nk = 1.0f;
        } else if (s.facts & FACT_VN) { // Triangle.GetNormal quirk: Normal is never set -> NaN when inside
            const VnP vn = vnormals + 3 * id;
            const TestRec R = tests[b.sg >> 1]; // barycentrics (u, v) = rows 0, 1 of M (p, 1)
            bu = dot4(R.r0, pos);
            bv = dot4(R.r1, pos);
            n = normalize(madd(xyz(vn[2]), bu + bv, madd(xyz(vn[1]), bv, xyz(vn[0]) * bu)));
            nk = 1.0f;
            if (gin) n = v3(__builtin_nanf(""), __builtin_nanf(""), __builtin_nanf(""));
        }
    }
    const V3 nrm = n * (gin ? -nk : nk);
    const bool inside = gin ^ ((fl & F_INVERT) != 0);
    if constexpr (REC) {
        rec->prim_id = id;
        rec->inside = inside ? 1 : 0;
        rec->distance = b.t;
        rec->pos = pos;
        rec->nrm = nrm;
        if (s.debug_geom) { // (the two returns above, see REC)
            rec->type = RT_BOUNCE_DEBUG;
            col = xyz(M.specular) + xyz(M.diffuse) + emis;
            return 1;
        }
        if (S.bounce >= s.recursion) {
            rec->type = RT_BOUNCE_RECURSION_COMPLETE;
            col = S.tint * emis;
            return 1;
        }
    }

    // RandomShine (Raytracer.cs:51-56): z = U^(1/shininess), theta = U * 2pi
    const float shin = M.shininess;
    float z = 1.0f, sz = 0.0f;
    if (!(s.facts & FACT_INF_SHININESS) || !(__builtin_isinf(shin) && shin > 0.0f)) {
        const float a = __builtin_amdgcn_logf(next_u(S.rng)) * M.inv_shininess; // log2(U) / shininess
        z = __builtin_amdgcn_exp2f(a);
        sz = fsqrt(one_minus_exp2_2a<!SLOT>(a, z));
    }
    const Frame fr = make_frame(nrm);
    const V3 rough = horizon(fr, nrm, z, sz, next_u(S.rng));

    const float diff_lum = M.diffuse.w, emis_lum = M.emission.w;
    float spec_lum = M.specular.w, refr_lum = M.refraction.w;
    const float cs = -dot(rough, S.d);
    if constexpr (REC) rec->cos_in = cs;
    float cos_out = 0.0f, ior_ratio = 0.0f;
    // (luminances are never NaN: for them x > 0 is the integer compare of the bits, which needs no
    // quieting of the LDS-loaded operands as the max the compiler made of the float form did)
    const bool some_lum = SLOT ? ((refr_lum > 0.0f) | (spec_lum > 0.0f))
                               : ((__float_as_int(refr_lum) > 0) | (__float_as_int(spec_lum) > 0));
    if ((s.facts & FACT_IOR) && some_lum && M.ior != 0.0f &&
        cs >= 0.0f) { // Raytracer.cs:120-161
        ior_ratio = inside ? M.eta_exit : M.eta_enter; // eta = iorIn / iorOut
        const float sin_out = ior_ratio * fsqrt(1.0f - cs * cs);
        if (sin_out >= 1.0f) {
            refr_lum = 0.0f;
            if constexpr (REC) rec->fresnel = 1.0f; // Raytracer.cs:144
        } else {
            cos_out = fsqrt(1.0f - sin_out * sin_out);
            // unpolarised Fresnel with numerator and denominator divided by iorOut:
            // rs = (cs - eta co) / (cs + eta co), rp = (eta cs - co) / (eta cs + co), one reciprocal
            const float ra = fmaf(-ior_ratio, cos_out, cs), rb = fmaf(ior_ratio, cos_out, cs);
            const float pa = fmaf(ior_ratio, cs, -cos_out), pb = fmaf(ior_ratio, cs, cos_out);
            const float ratio = (ra * ra * pb * pb + pa * pa * rb * rb) * rcp(rb * rb * pb * pb) * 0.5f;
            spec_lum *= ratio;
            refr_lum *= 1.0f - ratio;
            if constexpr (REC) rec->fresnel = ratio; // Raytracer.cs:155
        }
    } else {
        refr_lum = 0.0f;
    }
    const float total = diff_lum + spec_lum + refr_lum + emis_lum;
    if (total <= 0.0f) {
        if constexpr (REC) rec->type = RT_BOUNCE_PURE_BLACK;
        col = S.tint * emis;
        return 1;
    }
    // the choice (Raytracer.cs:177-229): refraction -> specular -> diffuse -> emission, by
    // subtracting luminances from U * total; then one direction formula per kind of event
    float ray_rand = next_u(S.rng) * total;
    const bool transmit = refr_lum != 0.0f && (ray_rand -= refr_lum) <= 0.0f;
    const bool specular = !transmit && spec_lum != 0.0f && (ray_rand -= spec_lum) <= 0.0f;
    const bool diffuse = !transmit && !specular && diff_lum != 0.0f && (ray_rand -= diff_lum) <= 0.0f;
    if (!(transmit | specular | diffuse)) { // emission
        if constexpr (REC) rec->type = RT_BOUNCE_EMISSION;
        col = S.tint * emis;
        return 1;
    }
    if constexpr (REC) rec->type = transmit ? RT_BOUNCE_TRANSMITTED : specular ? RT_BOUNCE_SPECULAR : RT_BOUNCE_DIFFUSE;
    V3 out_dir, new_tint;
    if (diffuse) {
        const float dz = acos_turn2(next_u(S.rng)); // 2 acos(U) / pi (Raytracer.cs:215)
        const float ds = fsqrt(fmaxf(0.0f, 1.0f - dz * dz));
        out_dir = horizon(fr, nrm, dz, ds, next_u(S.rng));
        new_tint = xyz(M.diffuse);
    } else {
        // transmission: (d + rough cs) eta - rough cos_out; reflection: d + rough 2 cs
        const float al = transmit ? ior_ratio : 1.0f;
        const float be = transmit ? cs * ior_ratio - cos_out : 2.0f * cs;
        out_dir = madd(rough, be, S.d * al);
        if (specular && !(dot(out_dir, nrm) > 0.0f)) { // a specular ray into the surface ends the path
            if constexpr (REC) rec->type = RT_BOUNCE_SPECULAR_FAIL;
            col = S.tint * emis;
            return 1;
        }
        new_tint = transmit ? (inside ? v3(1.0f, 1.0f, 1.0f) : xyz(M.refraction)) : xyz(M.specular);
    }
    S.o = pos;
    // GetColor renormalises the direction at the start of bounces i = 0, 3, 6, 9, ... only
    // (Raytracer.cs:74-75, Ray.Directional); the ray leaving this bounce is traced as bounce
    // S.bounce + 1.  The reflected, transmitted and CreateHorizon directions are unit vectors up to
    // rounding, so one Newton step of 1/|d| (1.5 - 0.5 |d|^2, relative error (|d|^2 - 1)^2) is the
    // normalisation to fp32 precision, without the reciprocal square root.
    S.d = out_dir * (renormalise_at<SLOT>(s, S.bounce + 1) ? fmaf(-0.5f, dot(out_dir, out_dir), 1.5f) : 1.0f);
    S.prev = b.sg >> 1; // the primitive the ray leaves, named by its slot (every kernel)
    if (VN && s.n_vn > 0 && kind == RT_PRIM_TRIANGLE && (fl & F_HASNORMALS)) {
        // does the reference's next query meet this triangle again (vn_rehit_test), and is that a
        // new hit?  Primitive.RayTrace culls it first when one-sided (Primitive.cs:56-64).  A NaN
        // direction (a diffuse bounce about GetNormal's NaN) never gets past the BVH root
        // (BVH.cs:301-303: far >= 0 fails), so it meets nothing.
        bool gin2;
        if (!__builtin_isnan(S.d.x + S.d.y + S.d.z) && vn_rehit_test(prims_d[id], (double)bu, (double)bv, S.d, gin2) &&
            ((fl & F_TWOSIDED) || !(gin2 ^ ((fl & F_INVERT) != 0)))) {
            const bool front = dot(out_dir, nrm) > 0.0f; // Ray.Direction . prev.Normal (false for NaN)
            if (front ? (gin2 == gin) : (gin2 != gin))  // Inside compared after Invert on both sides
                S.prev = -2 - ((b.sg & ~1) | (int)gin2);
        }
    }
    S.tint = S.tint * (new_tint * (SLOT ? fmaxf(total, 1.0f) : vmax1(total)));
    S.bounce++;
    return 0;
}

// LDS staging of the shading records (PrimF per slot, MatF per ID, XformF): the per-lane gathers
// after each closest-hit query become LDS reads instead of dependent global loads.
struct ShadeRecs {
    const PrimF* prims;
    const MatF* mats;
    const XformF* xfs;
};
template <bool LDS, class SceneT>
__device__ __forceinline__ ShadeRecs stage_scene(const SceneT& s, const PrimF* prims_g, const MatF* mats_g,
                                                 const XformF* xf, float4* lds_scene)
{
    if (!LDS) return ShadeRecs{prims_g, mats_g, xf};
    const int n_p = s.n_slots * (int)(sizeof(PrimF) / 16), n_m = s.n_mats * (int)(sizeof(MatF) / 16),
              n_x = s.n_xf * (int)(sizeof(XformF) / 16);
    const float4* gp = reinterpret_cast<const float4*>(prims_g);
    const float4* gm = reinterpret_cast<const float4*>(mats_g);
    const float4* gx = reinterpret_cast<const float4*>(xf);
    for (int i = threadIdx.x; i < n_p; i += blockDim.x) lds_scene[i] = gp[i];
    for (int i = threadIdx.x; i < n_m; i += blockDim.x) lds_scene[n_p + i] = gm[i];
    for (int i = threadIdx.x; i < n_x; i += blockDim.x) lds_scene[n_p + n_m + i] = gx[i];
    __syncthreads();
    return ShadeRecs{reinterpret_cast<const PrimF*>(lds_scene), reinterpret_cast<const MatF*>(lds_scene + n_p),
                     reinterpret_cast<const XformF*>(lds_scene + n_p + n_m)};
}

__device__ __forceinline__ int scene_lds_float4s(const PathScene& s)
{
    return s.n_slots * (int)(sizeof(PrimF) / 16) + s.n_mats * (int)(sizeof(MatF) / 16) +
           s.n_xf * (int)(sizeof(XformF) / 16);
}

// One lane's work: the open work item (a chunk of samples of one pixel), its running sums and
// the sample in flight.  The wave's item pool [pool_next, pool_end) is wave-uniform.
struct Lane {
    bool active, item_open, live;
    unsigned item;
    int fx, fy, s_next;
    rt_key2 pkey; // rt_rng_pixel_key of the open item's pixel
    float ar, ag, ab;
    unsigned cnt; // item bookkeeping: samples (bits 0-7) | misses (8-15) | samples left (16-31)
    unsigned pool_next, pool_end;
    unsigned split_j; // lane 0: item ranges (after its own) this wave found spent (PathParams::n_split)
    // sample rounds (refill, ROUNDS instances; wave-uniform): the open ticket runs in rounds, and the
    // wave's ray count, modulo 2^32, when it drew that ticket
    bool rounds;
    unsigned ticket_mark;
};

__device__ __forceinline__ void lane_init(Lane& L)
{
    L.active = true;
    L.item_open = L.live = false;
    L.item = 0;
    L.fx = L.fy = L.s_next = 0;
    L.pkey = rt_key2{0u, 0u};
    L.ar = L.ag = L.ab = 0.0f;
    L.cnt = 0;
    L.pool_next = L.pool_end = 0;
    L.split_j = 0;
    L.rounds = false;
    L.ticket_mark = 0;
}

// Lanes without a sample in flight close finished items and take new ones from the wave's
// pool (one atomic per p.pool items: chunks of one 8x8 block), then start the next camera sample
// of their item.
// NT: store the item partials non-temporally (the BVH kernels: their 16-B-per-sample partial
// stream would otherwise push the scene out of the Infinity Cache; C4 52.74-52.86 -> 52.30-52.37
// ms; the brute-force kernels keep normal stores, die.txt C3 27.5 -> 27.7-27.8 ms with them)
// The BVH (NT) kernels hold as little per lane as they can: at 7 waves per SIMD every register the
// refill and shading phases keep live spilled (round 5: 19 VGPRs, 21 GB of scratch writes per C4
// launch against 2.1 GB of partials).  Four changes, each computing the same values, took that to
// 2 (profiles/r06/c4_ab.txt, one call: C4 42.99 -> 38.52 ms, WRITE_SIZE 21.2 -> 2.7 GB per launch):
// * a lane's rank in the item dispenser by v_mbcnt (lanes_below), not a popcount of
//   m & ((1 << lane) - 1), whose 64-bit lane mask the compiler hoisted out of the loop and spilled;
// * the pixel's frame x and y in one register (L.fx = x | y << 16); since the xorshift stream (round 6),
//   in none: decoded from the item again at each sample start (item_pixel), as is the sample index
//   (item_sample; C4 scratch 24 -> 8 B per lane);
// * the pixel's RNG key derived again at each sample start instead of held per lane;
// * 1/d of every lane's query rebuilt after the shading phase instead of held through it.
// The brute-force kernels keep their layout (they read the pixel key from the scene's table).
__device__ __forceinline__ unsigned lanes_below(unsigned long long m)
{
    return __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
}
// A work item's pixel: item = ((block << log2_chunks) + chunk) * 64 + pixel of the 8x8 block, tile
// coordinates (px, py), its chunk c, and its frame coordinates (fx, fy; a band set maps tile rows to
// frame rows).  TABLE (the brute-force kernels' item open): a launch over the live blocks alone
// (PathParams::cull) reads the block's coordinates from its table, one 4-B load beside the pixel
// key's; the branch is wave-uniform.  Every other caller decodes launches that are never culled.
template <bool TABLE = false, class ParT>
__device__ __forceinline__ void item_pixel(unsigned item, const ParT& p, int& px, int& py, int& c, int& fx, int& fy)
{
    const unsigned q = item & 63u, t = item >> 6;
    c = (int)(t & (unsigned)(p.n_chunks - 1));
    unsigned by, bx;
    const unsigned blk = t >> p.log2_chunks;
    if (TABLE && p.cull != nullptr) {
        const unsigned v = p.cull[kCullTable + blk];
        bx = v & 0xFFFFu;
        by = v >> 16;
    } else if (p.magic_bx != 0) { // multiply-high division (exact here, make_params checks)
        by = __umulhi(blk, p.magic_bx);
        bx = blk - by * (unsigned)p.blocks_x;
    } else {
        divmod(blk, (unsigned)p.blocks_x, p.inv_blocks_x, by, bx);
    }
    px = (int)bx * 8 + (int)(q & 7);
    py = (int)by * 8 + (int)(q >> 3);
    fx = p.x0 + px;
    fy = p.y0 + py;
    if (p.band > 0) { // band set: tile row py -> frame row (wave-uniform branch)
        unsigned bq, br;
        if (p.band_log2 >= 0) {
            bq = (unsigned)py >> p.band_log2;
            br = (unsigned)py & (unsigned)(p.band - 1);
        } else {
            divmod((unsigned)py, (unsigned)p.band, p.inv_band, bq, br);
        }
        fy = p.y0 + ((int)bq * p.band_stride + p.band_offset) * p.band + (int)br;
    }
}

// rt_render_rays (the RAYS instances): the ray a work item names, item = ((block << log2_chunks) +
// chunk) * 64 + pixel with ray = block * 64 + pixel, so a wave's 64 items of one chunk are 64
// consecutive rays.  No division and no frame: make_params_rays plans the launch.
template <class ParT>
__device__ __forceinline__ unsigned item_ray(unsigned item, const ParT& p)
{
    return ((item >> (6 + p.log2_chunks)) << 6) | (item & 63u);
}

// rt_render_list (the RAYS, BEAMS and SURFELS instances of a launch with p.index_list): list position j
// = item_ray(item) -> the record the lane loads (rec) and the number its stream is keyed by (key), both
// j without a list.  With one the key is the entry e = index_list[j] and the record e's, or j's where the
// host entry gathered the listed records into the chunk (p.list_gathered); false for an entry at or
// past p.n_records, which opens no item.  The pointer test is wave-uniform.
template <class ParT>
__device__ __forceinline__ bool list_entry(const ParT& p, unsigned j, unsigned& rec, unsigned& key)
{
    rec = key = j;
    if (p.index_list) {
        key = p.index_list[j];
        if (key >= p.n_records) return false;
        if (!p.list_gathered) rec = key;
    }
    return true;
}

// rt_render_pixels (the PIXELS instances): a list entry pix = fy * width + fx -> (fx, fy), by the
// fp32-reciprocal divmod the item decode uses.  Exact: the estimate (float)pix * inv_frame_w carries
// three roundings of 2^-24 relative each, less than 2^-22 fy in all, so for fy < 2^20 rows
// (check_render_pixels refuses taller frames) it is within 1 of fy, which divmod's one correction
// step repairs.  A multiply-high by ceil(2^32 / width) is exact only while pix * (M * width - 2^32) <
// 2^32, which a 1080p frame already passes.
template <class ParT>
__device__ __forceinline__ void list_pixel(unsigned pix, const ParT& p, int& fx, int& fy)
{
    unsigned q, r;
    divmod(pix, (unsigned)p.scene.width, p.inv_frame_w, q, r);
    fx = (int)r;
    fy = (int)q;
}

// The next sample of the lane's item.  The BVH (NT) kernels hold no register for it: the item's
// first sample (its chunk, from the item index) plus the samples it finished (samples + misses).
template <bool NT, class ParT>
__device__ __forceinline__ int item_sample(const Lane& L, const ParT& p)
{
    if (!NT) return L.s_next;
    const int c = (int)((L.item >> 6) & (unsigned)(p.n_chunks - 1));
    return c * p.chunk + (int)(L.cnt & 0xFFu) + (int)((L.cnt >> 8) & 0xFFu);
}
// SRC, where a launch's items come from (ItemSource, rt_kernels.h).
// ITEMS_RAYS (rt_render_rays' instances): an item names a ray of p.ray_list instead of a pixel (item_ray),
// its pixel key is that of p.stream_base + ray, and a sample starts from the ray as given, with the
// two draws GetCameraRay would have spent discarded; the camera is never read.  The brute-force
// kernels keep the ray index in L.fx; every kernel loads the ray's rows again at each sample start
// (they stay in the cache between an item's samples) instead of holding six more registers.
// ITEMS_BEAMS (rt_render_beams' instances): the RAYS instances with an rt_beam of p.beam_list in the
// ray's place.  An item opens as a ray's does; a sample start loads the beam's twelve rows again and
// builds the sample's ray at the point (u, v) of the footprint that the two GetCameraRay draws name
// (beam_sample, rt_beam.h: the copy the host twin compiles too).  A degenerate sample closes as one
// primary miss without a query, an invalid beam closes all the item has left.
// ITEMS_SURFELS (rt_render_surfels' instances): the RAYS instances with an rt_surfel of p.ray_list (the
// same four rows) in the ray's place.  A sample start loads the rows again and draws the sample's
// direction about the surfel's normal from the two GetCameraRay draws, by the functions of shade()'s
// diffuse bounce (surfel_sample, rt_surfel.h: the copy rt_debug_surfel_rays_device's kernel compiles
// too); p.gather_mode, a launch constant, picks the distribution.  An invalid surfel closes as a bad ray.
// The three with an index list (rt_render_list; p.index_list, null on the three entry points' own launches):
// the item names list position j = item_ray(item), and list_entry gives the record it loads and the
// number its stream is keyed by, the entry index_list[j]; an entry at or past p.n_records opens no item.
// The pointer test is wave-uniform, and without a list both are j: the code path of the entry points is
// the one it was (profiles/render_list: the same registers and scratch in all 36 instances).
// ITEMS_PIXELS (rt_render_pixels' instances): an item names entry item_ray(item) of p.pixel_list, a
// frame pixel index fy * width + fx, and from there on the lane does what a tile launch does for that
// frame pixel: its key from the table or the hash, the rng of sample_base + sample, start_sample with
// both GetCameraRay draws used.  An entry at or past p.n_frame_px opens no item.  The brute-force
// kernels keep fx, fy in the lane; the BVH kernel reads the entry again at each sample start, as it
// decodes a tile's item again (list_pixel).
// ROWS (the brute-force tile instances that are not instrumented and have no vertex normals, whose
// instances already spill): start rows, PathParams::starts.
// A lane that starts a camera sample does so alone or with a few others: the lanes of a wave finish
// their samples at different bounces, so the start's ~60 VALU instructions were issued in most
// iterations for a tenth of the lanes.  The item open is where a wave's lanes are together (p.batch)
// and know every sample they will start: there the wave runs the start of each of the item's
// samples, the same functions on the same inputs, and stores one 16-B row per sample, direction
// and rng state; the sample start loads the lane's row and finishes camera_ray's last line.  A lane
// reads only rows it wrote itself, so no fence; lanes that open items without the rest of the wave
// run the loop under their mask.  The host sets the pointer only for a frustum camera without depth
// of field (plan_start_rows); a scene-specialised build knows the camera's kind and leaves the code out.
template <bool NT, int SRC, bool ROWS, class ParT, class CamT>
__device__ __forceinline__ bool start_rows_on(const ParT& p, [[maybe_unused]] const CamT& cam)
{
    if constexpr (NT || SRC != ITEMS_TILE || !ROWS) {
        return false;
    } else {
#ifdef RT_SCENE_CONST
        if (!cam_frustum(cam) || cam_dof(cam)) return false;
#endif
        return p.starts != nullptr;
    }
}
typedef float row_f4 __attribute__((ext_vector_type(4)));
#ifdef __HIP_DEVICE_COMPILE__
typedef __attribute__((address_space(1))) row_f4 row_g4;      // global: plain global_load / global_store
typedef __attribute__((address_space(1))) unsigned char row_g1;
#else
typedef row_f4 row_g4;
typedef unsigned char row_g1;
#endif
// byte offset of row r of this lane: the buffer stays below 4 GiB (plan_start_rows' cap)
template <class ParT>
__device__ __forceinline__ unsigned start_row_offset(const ParT& p, unsigned r, int lane)
{
    // (blocks of 256 threads: 4 waves)
    const unsigned wave = blockIdx.x * 4u + (unsigned)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    return (((wave * (unsigned)p.start_rows + r) << 6) | (unsigned)lane) * 16u;
}

// ROUNDS (the instances that have ROWS, for the same reason): sample rounds, PathParams::sample_rounds.
// A wave opens a ticket's 64 items together and closes them together (p.batch), so the lanes whose
// paths end early wait at the ticket's end in any case; and where nearly every path runs to the
// recursion limit (a closed room) some lane of the 64 is at full length in every sample.  In rounds
// that wait is taken at each sample's end instead: a lane with samples left starts the next one only
// once no lane of the wave is live, so the wave starts sample k of the ticket together.  The wave's
// iterations stay what they were (sum over samples of the longest path against the longest sum of
// paths, +0.01 % on bounce.txt, tools/round_sim.py), and every live lane is then at the same bounce
// in every iteration: the sample start below, shade's body past the recursion limit and the sample's
// end run for all lanes in one iteration of recursion + 1 and are branched over in the others.
// Where path lengths differ the wait is real (die.txt +15 %), so each ticket chooses (ticket_rounds,
// rt_kernels.h; rays_now: the wave's ray count).  The vote is taken here, outside the divergent code,
// and the mode is wave-uniform.
// Progress: a lane held back waits for live lanes only, never for a lane that waits, and a live lane
// ends within recursion + 1 iterations; once none is live every lane with samples left starts.  So
// the wait is bounded whatever p.batch is and however the items were opened.
template <bool NT, int SRC = ITEMS_TILE, bool ROWS = false, bool ROUNDS = false, class ParT, class SceneT, class CamT>
__device__ __forceinline__ void refill(Lane& L, Sample& S, const ParT& p, const SceneT& s, const CamT& cam, int lane,
                                      unsigned total, [[maybe_unused]] unsigned rays_now = 0)
{
    static_assert(!ROUNDS || (!NT && SRC == ITEMS_TILE), "sample rounds: the brute-force tile instances");
    bool go = true; // wave-uniform
    if constexpr (ROUNDS) go = !L.rounds || __ballot(L.live) == 0ull;
    const bool need = L.active && !L.live && (!L.item_open || L.cnt < 65536u);
    if (need && L.item_open) {
        const float4 part = make_float4(L.ar, L.ag, L.ab, __uint_as_float((L.cnt & 0xFFu) | ((L.cnt & 0xFF00u) << 8)));
        if (NT) {
            typedef float nt_f4 __attribute__((ext_vector_type(4)));
            const nt_f4 v = {part.x, part.y, part.z, part.w};
            __builtin_nontemporal_store(v, reinterpret_cast<nt_f4*>(&p.partial[L.item]));
        } else {
            p.partial[L.item] = part;
        }
        L.item_open = false;
        L.ar = L.ag = L.ab = 0.0f; // the next item starts from zero
    }
    const unsigned long long m = __ballot(need);
    if (m) {
        unsigned k = (unsigned)__popcll(m);
        const unsigned avail = L.pool_end - L.pool_next;
        unsigned fresh = 0, fresh_len = (unsigned)p.pool;
        // Brute-force kernels: once the pool is used up, the next ticket is drawn only when p.batch
        // lanes wait for an item (64: the whole wave), or no lane of the wave has work left; the lanes
        // that came early wait, and ask again in the next iteration.  A wave then opens a ticket's
        // items together and its lanes stay in step: in most iterations no lane closes or opens an
        // item or is alone in a shading branch, and those sections are branched over.  That saves
        // more instructions than the waiting lanes lose (make_params has the figures).
        bool draw = k > avail;
        if (!NT && draw && k < (unsigned)p.batch && __ballot(L.active && !need) != 0ull) {
            draw = false;
            k = avail; // the pool's last items are still dealt
        }
        if (draw) { // wave-uniform: one atomic refills the pool
            // lane 0 draws a ticket of a range: got = ticket | range << 28 (a launch has fewer than
            // 2^26 tickets, run_path checks), range n_split when every range is spent; the ticket's
            // items (ticket_items, rt_kernels.h) are then worked out once per wave, in scalar code.
            // p.linear (ticket t of range g is the p.pool items from split_start[g] + t * pool): lane 0
            // has the first item itself, its load of split_start[g] in flight with the atomic as before
            // tickets (C4 draws one per two samples of a lane, and ticket_items' loads wait for it)
            const bool linear = p.linear != 0;
            unsigned got = linear ? total : (unsigned)p.n_split << 28;
            if (lane == 0) {
                if (p.n_split <= 1) {
                    const unsigned f = atomicAdd(p.counter, 1u);
                    if (f < p.split_tickets[0]) got = linear ? f * (unsigned)p.pool : f;
                } else {
                    // the range of this workgroup's XCD first, then the others in turn (L.split_j: the
                    // ranges this wave found spent)
                    const unsigned g0 = blockIdx.x & (unsigned)(p.n_split - 1);
                    for (; L.split_j < (unsigned)p.n_split; L.split_j++) {
                        const unsigned g = (g0 + L.split_j) & (unsigned)(p.n_split - 1);
                        const unsigned f = atomicAdd(p.counter + kSplitStride * g, 1u);
                        if (f < p.split_tickets[g]) {
                            got = linear ? p.split_start[g] + f * (unsigned)p.pool : f | g << 28;
                            break;
                        }
                    }
                }
            }
            got = __builtin_amdgcn_readfirstlane(got);
            if constexpr (ROUNDS) { // the new ticket's mode, from the rays of the one before (pool_end 0: none)
                L.rounds = __builtin_amdgcn_readfirstlane(
                               (int)ticket_rounds(p, s.recursion, L.pool_end == 0u, rays_now - L.ticket_mark)) != 0;
                L.ticket_mark = rays_now;
            }
            fresh = linear ? got : total; // all spent -> total, which ends the lane
            if (!linear && (got >> 28) < (unsigned)p.n_split)
                ticket_items(p, got >> 28, got & 0xFFFFFFFu, fresh, fresh_len);
        }
        if (need) {
            const unsigned r = NT ? lanes_below(m) : (unsigned)__popcll(m & ((1ull << lane) - 1ull));
            L.item = r < avail ? L.pool_next + r : fresh + (r - avail);
            if (r >= k) {
                // (no ticket drawn for it yet: it asks again in the next iteration)
            } else if (L.item >= total) {
                L.active = false;
            } else if constexpr (SRC == ITEMS_PIXELS) {
                const unsigned li = item_ray(L.item, p);
                const int s0 = (int)((L.item >> 6) & (unsigned)(p.n_chunks - 1)) * p.chunk;
                if (li < p.n_rays && s0 < p.spp) {
                    const unsigned pix = p.pixel_list[li];
                    if (pix < p.n_frame_px) {
                        L.item_open = true;
                        if (!NT) L.s_next = s0;
                        L.cnt = (unsigned)(min(p.spp, s0 + p.chunk) - s0) << 16; // chunk <= 64
                        if (!NT) {
                            list_pixel(pix, p, L.fx, L.fy);
                            if (p.pkeys) L.pkey = p.pkeys[pix];
                            else L.pkey = rt_rng_pixel_key(p.seed_key, (unsigned long long)pix);
                        }
                    }
                }
            } else if constexpr (SRC == ITEMS_RAYS || SRC == ITEMS_BEAMS || SRC == ITEMS_SURFELS) {
                const unsigned ri = item_ray(L.item, p);
                const int s0 = (int)((L.item >> 6) & (unsigned)(p.n_chunks - 1)) * p.chunk;
                unsigned rec, key;
                if (ri < p.n_rays && s0 < p.spp && list_entry(p, ri, rec, key)) {
                    L.item_open = true;
                    if (!NT) L.s_next = s0;
                    L.cnt = (unsigned)(min(p.spp, s0 + p.chunk) - s0) << 16; // chunk <= 64
                    if (!NT) {
                        L.fx = (int)rec;
                        L.pkey = rt_rng_pixel_key(p.seed_key, p.stream_base + (unsigned long long)key);
                    }
                }
            } else {
                int px, py, c, fx, fy;
                item_pixel<!NT>(L.item, p, px, py, c, fx, fy);
                if (px < p.w && py < p.h && c * p.chunk < p.spp) {
                    L.item_open = true;
                    const int s0 = c * p.chunk;
                    if (!NT) L.s_next = s0; // (the BVH kernels derive it: item_sample)
                    L.cnt = (unsigned)(min(p.spp, s0 + p.chunk) - s0) << 16; // chunk <= 64
                    if (!NT) { // (the BVH kernels decode the item again at each sample start)
                        L.fx = fx;
                        L.fy = fy;
                    }
                    // the frame width from the launch record (a scene-specialised build's constant
                    // scene leaves it out, so one build serves every frame size)
                    const unsigned long long pix = (unsigned long long)fy * (unsigned long long)p.scene.width +
                                                   (unsigned long long)fx;
                    // the brute-force kernels read the key from the scene's table (the same value:
                    // two hash rounds fewer per item open, which runs in most iterations)
                    if (!NT && p.pkeys) L.pkey = p.pkeys[pix];
                    else if (!NT) L.pkey = rt_rng_pixel_key(p.seed_key, pix);
                }
            }
        }
        if (draw) {
            L.pool_next = fresh + (k - avail);
            L.pool_end = fresh + fresh_len; // (a block's last ticket may be shorter than p.pool; never < 64)
        } else {
            L.pool_next += k;
        }
        // The rows of the items just opened (k: wave-uniform; the lanes that asked had no open item).
        if (k != 0 && start_rows_on<NT, SRC, ROWS>(p, cam)) {
            const unsigned n = need && L.item_open ? L.cnt >> 16 : 0u;
            row_g1* const rows = (row_g1*)(unsigned long long)p.starts;
            for (unsigned j = 0; j < (unsigned)p.start_rows; j++) {
                if (j < n) { // start_sample's ray, built in the lane's own sample registers: it has no sample
                    S.rng = rt_rng_from_pixel_key(L.pkey, p.sample_base + (unsigned long long)(L.s_next + (int)j));
                    float sx, sy;
                    sample_point<true>(L.fx, L.fy, S, sx, sy);
                    S.d = camera_ray(cam, sx, sy).d;
                    const row_f4 v = {S.d.x, S.d.y, S.d.z, __uint_as_float(S.rng.x)};
                    *(row_g4*)(rows + start_row_offset(p, j, lane)) = v;
                }
            }
        }
    }
    if constexpr (SRC == ITEMS_RAYS) {
        if (L.active && L.item_open && !L.live && L.cnt >= 65536u) {
            unsigned ri = (unsigned)L.fx;
            if (NT) { // the record and the key again (an open item's entry is inside the records: list_entry)
                unsigned key;
                (void)list_entry(p, item_ray(L.item, p), ri, key);
                L.pkey = rt_rng_pixel_key(p.seed_key, p.stream_base + (unsigned long long)key);
            }
            const QueryRay q = load_query_ray(p.ray_list, ri);
            if (q.valid) {
                S.rng = rt_rng_from_pixel_key(L.pkey, p.sample_base + (unsigned long long)item_sample<NT>(L, p));
                (void)rt_rng_next24(&S.rng); // GetCameraRay's subX and subY (Raytracer.cs:264-265)
                (void)rt_rng_next24(&S.rng);
                S.o = q.o;
                S.d = q.d;
                S.tint = v3(1.0f, 1.0f, 1.0f);
                S.bounce = 0;
                S.prev = -1;
                L.live = true;
            } else { // every sample the item has left is a primary miss; no query, so no ray counted
                const unsigned left = L.cnt >> 16;
                L.cnt = (L.cnt & 0xFFFFu) + (left << 8);
                if (!NT) L.s_next += (int)left;
            }
        }
        return;
    }
    if constexpr (SRC == ITEMS_BEAMS) {
        if (L.active && L.item_open && !L.live && L.cnt >= 65536u) {
            unsigned bi = (unsigned)L.fx;
            if (NT) { // the record and the key again (an open item's entry is inside the records: list_entry)
                unsigned key;
                (void)list_entry(p, item_ray(L.item, p), bi, key);
                L.pkey = rt_rng_pixel_key(p.seed_key, p.stream_base + (unsigned long long)key);
            }
            S.rng = rt_rng_from_pixel_key(L.pkey, p.sample_base + (unsigned long long)item_sample<NT>(L, p));
            // GetCameraRay's subX and subY (Raytracer.cs:264-265): the sample's point in the footprint
            const float u = (float)rt_rng_next24(&S.rng) * 0x1p-24f;
            const float v = (float)rt_rng_next24(&S.rng) * 0x1p-24f;
            BeamV o, d;
            const BeamSample r = beam_sample(p.beam_list + (size_t)kBeamRows * (size_t)bi, u, v, o, d);
            if (r == BEAM_RAY) {
                S.o = v3(o.x, o.y, o.z);
                S.d = v3(d.x, d.y, d.z);
                S.tint = v3(1.0f, 1.0f, 1.0f);
                S.bounce = 0;
                S.prev = -1;
                L.live = true;
            } else { // no query, so no ray counted: one primary miss, and the lane asks again for its next
                     // sample; or, for an invalid beam, every sample the item has left (the rays' rule)
                const unsigned left = r == BEAM_INVALID ? L.cnt >> 16 : 1u;
                L.cnt += left * (256u - 65536u);
                if (!NT) L.s_next += (int)left;
            }
        }
        return;
    }
    if constexpr (SRC == ITEMS_SURFELS) {
        if (L.active && L.item_open && !L.live && L.cnt >= 65536u) {
            unsigned si = (unsigned)L.fx;
            if (NT) { // the record and the key again (an open item's entry is inside the records: list_entry)
                unsigned key;
                (void)list_entry(p, item_ray(L.item, p), si, key);
                L.pkey = rt_rng_pixel_key(p.seed_key, p.stream_base + (unsigned long long)key);
            }
            S.rng = rt_rng_from_pixel_key(L.pkey, p.sample_base + (unsigned long long)item_sample<NT>(L, p));
            // GetCameraRay's subX and subY (Raytracer.cs:264-265): the direction's cosine and turn
            const float u1 = (float)rt_rng_next24(&S.rng) * 0x1p-24f;
            const float u2 = (float)rt_rng_next24(&S.rng) * 0x1p-24f;
            if (surfel_sample(p.ray_list + 4 * (size_t)si, p.gather_mode, u1, u2, S.o, S.d)) {
                S.tint = v3(1.0f, 1.0f, 1.0f);
                S.bounce = 0;
                S.prev = -1;
                L.live = true;
            } else { // every sample the item has left is a primary miss; no query, so no ray counted
                const unsigned left = L.cnt >> 16;
                L.cnt = (L.cnt & 0xFFFFu) + (left << 8);
                if (!NT) L.s_next += (int)left;
            }
        }
        return;
    }
    if (go && L.active && L.item_open && !L.live && L.cnt >= 65536u) {
        if (start_rows_on<NT, SRC, ROWS>(p, cam)) {
            // the sample's row: the samples and misses the item has finished.  The writes to S in
            // start_sample's order: with another order the two branches' stores were merged by
            // address and four of S's fields stayed in scratch.
            const unsigned r = (L.cnt & 0xFFu) + ((L.cnt >> 8) & 0xFFu);
            const row_g1* const rows = (const row_g1*)(unsigned long long)p.starts;
            const row_f4 v = *(const row_g4*)(rows + start_row_offset(p, r, lane));
            const V3 d = v3(v.x, v.y, v.z);
            S.rng.x = __float_as_uint(v.w);
            S.o = madd(d, cam.image_plane, xyz(cam.position)); // camera_ray's last line
            S.d = d;
            S.tint = v3(1.0f, 1.0f, 1.0f);
            S.bounce = 0;
            S.prev = -1;
            L.live = true;
            return;
        }
        int fx = L.fx, fy = L.fy;
        if (NT && SRC == ITEMS_PIXELS) { // the list entry again (it stays in the cache between an item's samples)
            const unsigned pix = p.pixel_list[item_ray(L.item, p)];
            list_pixel(pix, p, fx, fy);
            L.pkey = rt_rng_pixel_key(p.seed_key, (unsigned long long)pix);
        } else if (NT) { // the pixel and its key again at every sample start: three registers fewer held
            int px, py, c;
            item_pixel(L.item, p, px, py, c, fx, fy);
            L.pkey = rt_rng_pixel_key(p.seed_key, (unsigned long long)fy * (unsigned long long)p.scene.width +
                                                      (unsigned long long)fx);
        }
        S.rng = rt_rng_from_pixel_key(L.pkey, p.sample_base + (unsigned long long)item_sample<NT>(L, p));
        start_sample<!NT>(cam, fx, fy, S);
        L.live = true;
    }
}

// After a closest-hit query: one bounce of GetColor; a finished sample goes into the item's sums.
// REC (the instrumented instances): a launch of rt_trace_paths (p.rec_rays set) also stores the
// bounce's record, and the sample's own colour and record count when it ends, at the slot the lane's
// open item names: item_pixel gives the pixel, item_sample the sample, S.bounce the bounce.
template <bool VN, bool PIN = false, bool SLOT = false, bool REC = false, class SceneT, class VnP, class TestP, class ParT>
__device__ __forceinline__ void bounce(Lane& L, Sample& S, const SceneT& s, const ShadeRecs& R, VnP vnormals, TestP tests,
                                       const PrimD* prims_d, const Best& b, [[maybe_unused]] const ParT& p)
{
    V3 col;
    [[maybe_unused]] BounceRec rec;
    [[maybe_unused]] const V3 ro = S.o, rd = S.d, rtint = S.tint; // the ray of this bounce: shade() replaces it
    [[maybe_unused]] const int rbounce = S.bounce;
    [[maybe_unused]] unsigned rsample = 0; // (py * w + px) * spp + sample, before the item's counts move on
    if constexpr (REC) {
        if (p.rec_rays) {
            int px, py, c, fx, fy;
            item_pixel(L.item, p, px, py, c, fx, fy);
            rsample = ((unsigned)py * (unsigned)p.w + (unsigned)px) * (unsigned)p.spp + (unsigned)item_sample<SLOT>(L, p);
        }
    }
    const int r = shade<VN, PIN, SLOT, REC>(s, R.prims, R.mats, R.xfs, vnormals, tests, prims_d, b, S, col, &rec);
    if constexpr (REC) {
        const unsigned slot = rsample * (unsigned)(s.recursion + 1) + (unsigned)rbounce;
        if (p.rec_rays && slot < p.rec_max && rbounce <= s.recursion) { // whole 16-byte rows (rt_debug_ray)
            float4* q = p.rec_rays + (size_t)kRecRows * slot;
            q[0] = make_float4(__int_as_float(rec.prim_id), __int_as_float(rec.type), __int_as_float(rec.inside), rec.distance);
            q[1] = make_float4(rec.fresnel, rec.cos_in, __int_as_float(rbounce), 0.0f);
            q[2] = make_float4(rec.pos.x, rec.pos.y, rec.pos.z, rec.nrm.x);
            q[3] = make_float4(rec.nrm.y, rec.nrm.z, ro.x, ro.y);
            q[4] = make_float4(ro.z, rd.x, rd.y, rd.z);
            q[5] = make_float4(rtint.x, rtint.y, rtint.z, 0.0f);
            if (r != 0) // the sample as a 1-spp pass returns it (its item's sum from zero), and its records
                p.rec_samples[rsample] = r == 1 ? make_float4(0.0f + col.x, 0.0f + col.y, 0.0f + col.z, __int_as_float(rbounce + 1))
                                                : make_float4(-1.0f, -1.0f, -1.0f, __int_as_float(rbounce + 1));
        }
    }
    if (r != 0) {
        const bool hit = r == 1;
        L.ar += hit ? col.x : 0.0f;
        L.ag += hit ? col.y : 0.0f;
        L.ab += hit ? col.z : 0.0f;
        L.cnt += hit ? 1u - 65536u : 256u - 65536u; // one more sample or miss, one fewer left
        if (!SLOT) L.s_next++; // (the BVH kernels derive it from cnt: item_sample)
        L.live = false;
        if (!SLOT) {
            // The sample is over: its ray state is dead until the next start_sample writes all of it.
            // Saying so (an empty asm that "defines" the registers) lets the register allocator give
            // these values the registers the continuing lanes' new ray state takes, instead of
            // copying the 12 sample registers out and back at this divergent join (23 moves per
            // iteration in the bounce.txt listing; measured: C2 unchanged, C3 27.31-27.40 ->
            // 27.25-27.31 ms).  The BVH kernels, whose finished lanes wait for the batched shading
            // phase, keep the plain form.
            asm volatile("" : "=v"(S.o.x), "=v"(S.o.y), "=v"(S.o.z), "=v"(S.d.x), "=v"(S.d.y), "=v"(S.d.z),
                         "=v"(S.tint.x), "=v"(S.tint.y), "=v"(S.tint.z), "=v"(S.bounce), "=v"(S.prev),
                         "=v"(S.rng.x));
        }
    }
}

template <bool STATS, class ParT>
__device__ __forceinline__ void flush_counts(unsigned long long wave_rays, const Counters& cnt, const ParT& p,
                                             int lane)
{
    // one 64-bit add per wave for the ray count (and the optional traversal counters)
    if (lane == 0) atomicAdd(p.rays, wave_rays);
    if (STATS) {
        unsigned long long a = cnt.nodes, t = cnt.tris, q = cnt.sphs;
        for (int off = 32; off > 0; off >>= 1) {
            a += __shfl_down(a, off);
            t += __shfl_down(t, off);
            q += __shfl_down(q, off);
        }
        if (lane == 0) {
            atomicAdd(p.stats + 0, a);
            atomicAdd(p.stats + 1, t);
            atomicAdd(p.stats + 2, q);
            atomicAdd(p.stats + 3, cnt.cyc_start);
            atomicAdd(p.stats + 4, cnt.cyc_trace);
            atomicAdd(p.stats + 5, cnt.cyc_shade);
            atomicAdd(p.stats + 6, cnt.iters);
        }
        unsigned long long mx = cnt.max_steps, ov = cnt.ovf_pushes, ms = cnt.max_sp, ot = cnt.outer;
        for (int off = 32; off > 0; off >>= 1) {
            mx = max(mx, (unsigned long long)__shfl_down(mx, off));
            ov += __shfl_down(ov, off);
            ms = max(ms, (unsigned long long)__shfl_down(ms, off));
            ot += __shfl_down(ot, off);
        }
        if (lane == 0) {
            atomicMax(p.stats + 7, mx);
            atomicAdd(p.stats + 8, ov);
            atomicMax(p.stats + 9, ms);
            atomicAdd(p.stats + 10, ot);
        }
    }
}

// The camera and the launch parameters in the constant address space (RT_AS_CONST, rt_trace.h): uniform
// reads become scalar loads (the kernels never write them).
typedef RT_AS_CONST const CameraF CameraC;
typedef RT_AS_CONST const PathParams ParamsC;

// Brute-force megakernel: every loop iteration issues one closest-hit query per live lane
// (the scene's records arrive through scalar loads) and shades it.
template <bool CULL, bool LDS, bool STATS, bool VN, int SRC = ITEMS_TILE>
__device__ __forceinline__ void path_body(const CameraF* __restrict__ camp, const PathParams* __restrict__ pp)
{
    // everything but the LDS staging is read from the launch record *pp (fill_launch) in the
    // constant address space, by scalar loads where it is used (the by-value arguments are the
    // BVH kernels'; held in SGPRs for the whole kernel they spilled into VGPR lanes here)
    const ParamsC& P0 = *(const ParamsC*)pp;
    extern __shared__ float4 lds_scene[];
    const ShadeRecs R = stage_scene<LDS>(P0.scene, P0.prims, P0.mats, P0.xf, lds_scene);
    const int lane = threadIdx.x & 63;
    const unsigned total = (unsigned)P0.n_chunks * (unsigned)P0.n_pad;
    // the first bounce's code: the flat order's tile instances that run sample rounds
    constexpr bool FIRST = !STATS && !VN && !CULL && SRC == ITEMS_TILE;
    Lane L;
    lane_init(L);
    Sample S;
    S.prev = -1;
    S.bounce = 0;
    Counters cnt{};
    unsigned long long wave_rays = 0; // wave-uniform
    // the scene bound's switch, read once (one SGPR pair for the whole kernel): the lanes that keep a
    // wave from the bound test, every lane when the switch is off
    // (bit 0 of the field; kFirstBounce and kFirstMasks are read where they are used)
    const unsigned long long bound_off = (P0.scene_bound & 1) != 0 ? 0ull : ~0ull;

    while (true) {
        unsigned long long t0 = 0, t1 = 0, t2 = 0;
        if (STATS) t0 = __builtin_readcyclecounter();
        // The camera and the launch record are read per iteration through scalar loads from an
        // opaque pointer: that keeps the compiler from holding ~28 camera words and the scene
        // fields in SGPRs for the whole kernel (they spilled into VGPR lanes and scratch).  The
        // pointers are in the constant address space: through a generic pointer the compiler
        // cannot rule out the kernel's own stores and emits per-lane flat loads instead.
        const CameraC* cp = (const CameraC*)camp;
        asm volatile("" : "+s"(cp));
        const ParamsC* pq = (const ParamsC*)pp;
        asm volatile("" : "+s"(pq));
#ifdef RT_SCENE_CONST
        const PathScene& sc = *(const PathScene*)kSceneW;
#else
        const auto& sc = pq->scene;
#endif
#if defined(RT_SCENE_CONST) && RT_SCENE_CONST_CAMERA
        // (the camera compiled in too)
        refill<false, ITEMS_TILE, !STATS && !VN, !STATS && !VN>(L, S, *pq, sc, *(const CameraF*)kCameraW, lane, total,
                                                         (unsigned)wave_rays);
#else
        refill<false, SRC, !STATS && !VN, !STATS && !VN && SRC == ITEMS_TILE>(L, S, *pq, sc, *cp, lane, total,
                                                                              (unsigned)wave_rays);
#endif
        if (!__any(L.active)) break;
        if (STATS) t1 = __builtin_readcyclecounter();
        wave_rays += (unsigned)__popcll(__ballot(L.live)); // one Scene.RayTrace per live lane
        if (L.live) {
#ifdef RT_SCENE_CONST // scene-specialised build (rt_jit.cpp): the records are compile-time constants
            const auto tests = (const TestRec*)kTestsW;
            const auto rects = (const RectRec*)kRectsW;
            const auto frames = (const FrameRec*)kFramesW;
            const auto boxes = (const BoxRec*)kFramesW;
            const auto groups = (const GroupRec*)kGroupsW;
            const auto xf = (const XformF*)kXfW;
#else
            const auto tests = (const RT_AS_CONST TestRec*)pq->tests;
            const auto rects = (const RT_AS_CONST RectRec*)pq->rects;
            const auto frames = (const RT_AS_CONST FrameRec*)pq->frames;
            const auto boxes = (const RT_AS_CONST BoxRec*)pq->frames;
            const auto groups = (const RT_AS_CONST GroupRec*)pq->groups;
            const auto xf = (const RT_AS_CONST XformF*)pq->xf;
#endif
            const auto vnormals = (const RT_AS_CONST float4*)pq->vnormals;
            Best b = query_start<VN>(sc, S.prev);
            // The scene bound (flat order).  A wave whose live lanes all hold camera rays (bounce 0: one
            // compare, one scalar or and a scalar branch for every other wave) tests them against the
            // box of every primitive but the planes, and skips the query when none meets it: the
            // reference's query fails such a ray at its BVH root.  bounce.txt camera 0 looks at its
            // room from outside, and 76.5 % of the frame's 8x8 blocks see none of it.
            // Secondary rays are not tested: they start on a surface inside the box.  Finished lanes
            // hold dead sample registers (bounce's asm); they are not in this branch, and the votes say
            // so again (L.live).  The planes and the NaN rule below stay outside the skip.  The
            // instrumented instances do not take it, so their counters keep their meaning: the
            // primitives a ray segment's query answers for.
            bool query = true;
            // First bounce (FIRST; every other instance has the guard as it was).  The predicate is the
            // guard's: no live lane past bounce 0, asked of the lanes.  (A scalar count of the round's
            // iterations answered the same in a rounds ticket and measured slower: DESIGN appendix A.)
            if constexpr (FIRST) {
                const bool camera_rays = __ballot(L.live && S.bounce != 0) == 0ull; // wave-uniform
                if (__builtin_expect(camera_rays, 0)) {
                    const int fb = pq->scene_bound; // (read here, once per round, not held across the loop)
                    if (fb & 1) query = __any(L.live && scene_meets(sc, S.o, S.d));
                    // The block's unit mask (block_cull.h, unit_masks): the camera rays of one 8x8 block can
                    // meet only the units whose bit is set, so the query runs those alone; a wave whose
                    // live lanes are of several blocks runs them all.  A unit left out leaves b as it was,
                    // which is what its test would have done.  The other iterations' query has no part in this.
                    if (query && (fb & kFirstMasks)) {
                        const unsigned sh = 6u + (unsigned)pq->log2_chunks;
                        const unsigned blk = (unsigned)__builtin_amdgcn_readfirstlane((int)L.item) >> sh;
                        unsigned long long mask = ~0ull;
                        if (__ballot(L.live && (L.item >> sh) != blk) == 0ull) {
                            const unsigned n_live = (unsigned)pq->n_pad >> 6;
                            const auto cw = (const RT_AS_CONST unsigned int*)pq->cull;
                            const unsigned at = cull_masks_at(n_live, cw[3]) + 2u * blk;
                            mask = (unsigned long long)cw[at] | (unsigned long long)cw[at + 1] << 32;
                        }
                        trace_units(groups, tests, rects, frames, boxes, xf, S.o, S.d, S.prev, b, mask);
                        query = false;
                    }
                }
            } else {
                if (!STATS && (!CULL || RT_BOUND_GROUPED) &&
                    __builtin_expect((__ballot(L.live && S.bounce != 0) | bound_off) == 0ull, 0))
                    query = __any(L.live && scene_meets(sc, S.o, S.d));
            }
            if (query)
                trace_brute<CULL, STATS>(sc, groups, tests, rects, frames, boxes, xf, S.o, S.d, S.prev, b, cnt.tris,
                                         cnt.sphs, cnt.nodes);
            test_planes(sc, tests, S.o, S.d, S.prev, b);
            // A NaN direction (a diffuse bounce about GetNormal's NaN normal, only in scenes with
            // vertex-normal triangles) fails the reference's BVH root test (BVH.cs:301-303: far >= 0
            // is false for NaN) and meets nothing.  The brute-force records would not all say so: a
            // box's slab reciprocals stay finite for NaN (slab_rcp_lean), so a NaN ray inside a room
            // box met its exit face.
            if (VN && __builtin_isnan(S.d.x + S.d.y + S.d.z)) b = Best{__builtin_huge_valf(), -1};
            if (STATS) t2 = __builtin_readcyclecounter();
            bounce<VN, false, false, STATS>(L, S, sc, R, vnormals, tests, pq->prims_d, b, *pq);
        } else if (STATS) {
            t2 = __builtin_readcyclecounter();
        }
        if (STATS) {
            const unsigned long long t3 = __builtin_readcyclecounter();
            cnt.cyc_start += t1 - t0;
            cnt.cyc_trace += t2 - t1;
            cnt.cyc_shade += t3 - t2;
            cnt.iters++;
        }
    }
    // a culled launch (PathParams::cull): the first wave of block 0 adds the primary rays of the dead
    // blocks' pixels, spp each, which no item stands for
    if (!STATS && SRC == ITEMS_TILE && P0.cull != nullptr && blockIdx.x == 0 && threadIdx.x < 64)
        wave_rays += ((unsigned long long)P0.cull[0] | (unsigned long long)P0.cull[1] << 32) * (unsigned long long)P0.spp;
    flush_counts<STATS>(wave_rays, cnt, *(const ParamsC*)pp, lane);
}

// SRC: ITEMS_RAYS / ITEMS_PIXELS / ITEMS_BEAMS / ITEMS_SURFELS, rt_render_rays' / rt_render_pixels' /
// rt_render_beams' / rt_render_surfels' instances (refill); the tile instances are as they were without
// the switch.
template <bool CULL, bool LDS, bool STATS, bool VN, int SRC = ITEMS_TILE>
__global__ void __launch_bounds__(256, CULL ? RT_GROUPED_WAVES : RT_PATH_WAVES)
    path_kernel(PathScene, const CameraF* __restrict__ camp, const PathParams* __restrict__ pp, const TestRec*,
                const RectRec*, const FrameRec*, const PrimF*, const NodeF*, const Node4Q*, const GroupRec*,
                const XformF*, const MatF*, const float4*)
{
    path_body<CULL, LDS, STATS, VN, SRC>(camp, pp); // the other arguments are the BVH kernels' (same launch)
}

// BVH megakernel with decoupled traversal.  A loop iteration advances the traversing lanes by one
// step of the speculative walk (walk_step): a wave-wide node step or leaf step (up to two primitives).
// Lanes whose query finished wait, and the shading / new-sample phase runs only once at least
// p.refill lanes wait (or none is still traversing).  So one long traversal no longer holds the
// other 63 lanes of its wave, and the divergent shading code is paid once per batch of finished
// queries.
template <int WIDTH, int STACK, bool LDS, bool STATS, bool VN, int SRC = ITEMS_TILE>
__global__ void __launch_bounds__(256, WIDTH == 4 ? RT_BVH_WAVES : RT_BVH2_WAVES)
    path_kernel_bvh(PathScene, const CameraF* __restrict__ camp, const PathParams* __restrict__ pp, const TestRec*,
                    const RectRec*, const FrameRec*, const PrimF*, const NodeF*, const Node4Q*, const GroupRec*,
                    const XformF*, const MatF*, const float4*)
{
    // As in the brute-force kernels, the camera and the launch record are read through opaque
    // constant-address-space pointers where they are used (held whole-kernel in SGPRs, they
    // spilled 58 SGPRs into VGPR lanes here); the other arguments are unused.
    const ParamsC& P0 = *(const ParamsC*)pp;
    __shared__ int stack_mem[STACK * 256];
    extern __shared__ float4 lds_scene[];
    const TravStack stk = make_stack(stack_mem, P0.stack_ovf);
    const ShadeRecs R = stage_scene<LDS>(P0.scene, P0.prims, P0.mats, P0.xf, lds_scene);
    // hot wide nodes after the staged shading records (dynamic LDS; see path_lds_bytes)
    Node4Q* lds_hot = reinterpret_cast<Node4Q*>(lds_scene + (LDS ? scene_lds_float4s(P0.scene) : 0));
    const LdsF4* hot_rows = (const LdsF4*)lds_hot;
    if (WIDTH == 4 && P0.scene.n_hot4 > 0) {
        const float4* src = reinterpret_cast<const float4*>(P0.scene.hot4);
        float4* dst = reinterpret_cast<float4*>(lds_hot);
        for (int i = threadIdx.x; i < P0.scene.n_hot4 * 4; i += blockDim.x) dst[i] = src[i];
        __syncthreads();
    }
    const int lane = threadIdx.x & 63;
    const unsigned total = (unsigned)P0.n_chunks * (unsigned)P0.n_pad;
    Lane L;
    lane_init(L);
    Sample S;
    S.prev = -1;
    S.bounce = 0;
    Counters cnt{};
    unsigned long long wave_rays = 0; // wave-uniform
    // traversal state of the lane's current query
    bool trav = false, done = false;
    Walk w{false, 0, 0, -1};
    // 1/d of the query; o/d is recomputed per node visit (three multiplies) instead of being held
    // across the loop (VGPR spills of the C4 kernel 13 -> 2 at 6 waves per SIMD; recomputing 1/d as
    // well, three clamped reciprocals per visit, measured slower: 45.9 -> 46.2 ms)
    V3 id{0, 0, 0};
    Best b{__builtin_huge_valf(), -1};

    while (true) {
        const ParamsC* pq = (const ParamsC*)pp;
        asm volatile("" : "+s"(pq));
        const CameraC* cp = (const CameraC*)camp;
        asm volatile("" : "+s"(cp));
        const ParamsC& p = *pq;
        const auto& s = pq->scene;
        const auto tests = (const RT_AS_CONST TestRec*)pq->tests;
        const auto rows = (const RT_AS_CONST float4*)pq->rows;
        const auto xf = (const RT_AS_CONST XformF*)pq->xf;
        const auto vnormals = (const RT_AS_CONST float4*)pq->vnormals;
        const auto nodes = (const RT_AS_CONST NodeF*)pq->nodes;
        const auto nodes4 = (const RT_AS_CONST Node4Q*)pq->nodes4;
        const unsigned long long waiting = __ballot(!trav && (L.active || L.live));
        const unsigned long long busy = __ballot(trav);
        if (!waiting && !busy) break;
        // The threshold is at most half the lanes still holding work, so that a wave whose item pool
        // ran dry does not hold its finished lanes until every query ends (C4 38.24-38.28 -> 38.10-38.15
        // ms, profiles/r06/ab_refill_adapt.log)
        const int refill_at = min(p.refill, (__popcll(waiting | busy) + 1) >> 1);
        if (!busy || __popcll(waiting) >= refill_at) {
            wave_rays += (unsigned)__popcll(__ballot(done)); // one Scene.RayTrace per finished query
            if (done) { // the query finished: the outer records and planes (outside the BVH), then one bounce
                // (a NaN direction, from a vertex-normal triangle, meets nothing: see path_body).  Here,
                // not at the query's start: there it held the query's best hit through the traversal
                // and measured 48.35 against 38.52 ms (profiles/r06/c4_ab.txt, lowreg_ostart)
                if (s.n_groups > 0 && !(VN && __builtin_isnan(S.d.x + S.d.y + S.d.z)))
                    test_outer<STATS>((const RT_AS_CONST GroupRec*)pq->groups, (const RT_AS_CONST RectRec*)pq->rects,
                                      (const RT_AS_CONST BoxRec*)pq->frames, S.o, S.d, S.prev, b, cnt.outer);
                // (test_planes' loop, written out: as a call, the render-rays instance without LDS staging
                // keeps one more register in scratch, 8 -> 12 B)
                for (int i = s.n_bvh; i < s.n_bvh + s.n_pln; i++) {
                    const TestRec tr = tests[i];
                    hit_plane<true>(tr, i, S.o, S.d, S.prev, b);
                }
                if (STATS && p.ray_log) { // rt_debug_ray_log: the query and its closest hit
                    const unsigned q = atomicAdd(p.ray_log_n, 1u);
                    if (q < p.ray_log_cap) {
                        float4* r = p.ray_log + 3 * (size_t)q;
                        r[0] = make_float4(S.o.x, S.o.y, S.o.z, __int_as_float(S.prev));
                        int px, py, c, fx, fy;
                        item_pixel(L.item, p, px, py, c, fx, fy);
                        r[1] = make_float4(S.d.x, S.d.y, S.d.z, __int_as_float(fy * p.scene.width + fx));
                        r[2] = make_float4(b.t, __int_as_float(b.sg), __int_as_float(S.bounce), 0.0f);
                    }
                }
                bounce<VN, !LDS, true, STATS>(L, S, s, R, vnormals, tests, pq->prims_d, b, p);
                done = false;
            }
            refill<true, SRC>(L, S, p, s, *cp, lane, total);
            if (L.live && !trav) { // start the next query
                walk_start(w, s.root, true); // (PathScene carries no node count; root is taken as it is)
                b = query_start<VN>(s, S.prev);
                trav = true;
            }
            // 1/d of every lane's query rebuilt after the shading phase, so that the three registers
            // are free inside it (the traversing lanes recompute the same values)
            id = v3(slab_rcp(S.d.x), slab_rcp(S.d.y), slab_rcp(S.d.z));
        }
        // One step of the walk.  The top of the wide tree comes from LDS, the rest from global memory,
        // and o / d is formed here, per visit (see id above).
        const auto fetch = [&](int ref) {
            if constexpr (WIDTH == 4) return (ref & RT_HOT_BIT) ? lds_node(hot_rows, ref & ~RT_HOT_BIT) : Node4Q(nodes4[ref]);
            else return NodeF(nodes[ref]);
        };
        [[maybe_unused]] const bool was_trav = trav, had_leaf = trav && w.pend >= 0;
        [[maybe_unused]] const int sp0 = w.sp;
        const WalkStep st = walk_step<STACK, false, STATS, WIDTH>(w, trav, p.spec, fetch, id, S.o * id, stk, tests, rows, xf,
                                                                  S.o, S.d, S.prev, b, cnt.tris, cnt.sphs);
        if (STATS) { // lane slots of this iteration (the BVH kernels reuse the brute-force cycle counters):
                     // testing a leaf | traversing but idle in this step's kind | waiting for the shading phase
            const unsigned n_trav = (unsigned)__popcll(__ballot(was_trav));
            const unsigned n_node = st.leaf_step ? 0u : (unsigned)__popcll(__ballot(st.can_node));
            const unsigned n_leaf = st.leaf_step ? (unsigned)__popcll(__ballot(had_leaf)) : 0u;
            cnt.cyc_start += n_leaf;
            cnt.cyc_trace += n_trav - n_node - n_leaf;
            cnt.cyc_shade += (unsigned)__popcll(__ballot(!was_trav && (L.active || L.live)));
            if (st.can_node && !st.leaf_step) {
                cnt.nodes++;
                if (WIDTH == 4) {
                    cnt.ovf_pushes += (unsigned)max(0, st.sp_visit - max(sp0, STACK));
                    cnt.max_sp = max(cnt.max_sp, (unsigned)st.sp_visit);
                }
            }
        }
        if (st.ended) {
            trav = false;
            done = true;
        }
        if (STATS) {
            cnt.iters++;
            if (trav) cnt.q_steps++;
            if (done) {
                cnt.max_steps = max(cnt.max_steps, cnt.q_steps);
                cnt.q_steps = 0;
            }
        }
    }
    flush_counts<STATS>(wave_rays, cnt, P0, lane);
}

} // namespace

#ifndef __HIPCC_RTC__ // the host side (not part of a hiprtc build)
namespace {
using PathKernel = void (*)(PathScene, const CameraF*, const PathParams*, const TestRec*, const RectRec*, const FrameRec*, const PrimF*,
                            const NodeF*, const Node4Q*, const GroupRec*, const XformF*, const MatF*, const float4*);

// vn: the scene has vertex-normal triangles (their re-hit test, vn_rehit_test, is fp64 code that
// costs the other scenes' kernels registers, so it is compiled only into separate instances)
// The uninstrumented pair of one item source.
template <bool CULL, bool LDS, int SRC>
PathKernel brute_src(bool vn)
{
    return vn ? path_kernel<CULL, LDS, false, true, SRC> : path_kernel<CULL, LDS, false, false, SRC>;
}
template <bool CULL, bool LDS>
PathKernel pick_brute(bool stats, bool vn, ItemSource src)
{
    switch (src) {
    case ITEMS_PIXELS: return brute_src<CULL, LDS, ITEMS_PIXELS>(vn);
    case ITEMS_RAYS: return brute_src<CULL, LDS, ITEMS_RAYS>(vn);
    case ITEMS_BEAMS: return brute_src<CULL, LDS, ITEMS_BEAMS>(vn);
    case ITEMS_SURFELS: return brute_src<CULL, LDS, ITEMS_SURFELS>(vn);
    default: break;
    }
    if (!stats) return brute_src<CULL, LDS, ITEMS_TILE>(vn);
    return vn ? path_kernel<CULL, LDS, true, true> : path_kernel<CULL, LDS, true, false>;
}
// The same for the BVH kernels: a list source has instances of the wide kernel only (rt_render_rays and
// the other list entries refuse a BVH2 scene before they get here), so none is compiled for WIDTH 2.
template <int WIDTH, int STACK, bool LDS, int SRC>
PathKernel bvh_src(bool vn)
{
    if constexpr (WIDTH == 4 || SRC == ITEMS_TILE)
        return vn ? path_kernel_bvh<WIDTH, STACK, LDS, false, true, SRC> : path_kernel_bvh<WIDTH, STACK, LDS, false, false, SRC>;
    return nullptr;
}
template <int WIDTH, int STACK, bool LDS>
PathKernel pick_bvh(bool stats, bool vn, ItemSource src)
{
    switch (src) {
    case ITEMS_PIXELS: return bvh_src<WIDTH, STACK, LDS, ITEMS_PIXELS>(vn);
    case ITEMS_RAYS: return bvh_src<WIDTH, STACK, LDS, ITEMS_RAYS>(vn);
    case ITEMS_BEAMS: return bvh_src<WIDTH, STACK, LDS, ITEMS_BEAMS>(vn);
    case ITEMS_SURFELS: return bvh_src<WIDTH, STACK, LDS, ITEMS_SURFELS>(vn);
    default: break;
    }
    if (!stats) return bvh_src<WIDTH, STACK, LDS, ITEMS_TILE>(vn);
    return vn ? path_kernel_bvh<WIDTH, STACK, LDS, true, true> : path_kernel_bvh<WIDTH, STACK, LDS, true, false>;
}

// variant = kernel * 2 + lds; kernel 0 brute force (flat), 1 brute force (grouped, culled),
// 2 BVH2 (24-entry LDS stack), 3 wide BVH (RT_WIDE_STACK-entry LDS stack); both overflow to global memory.
// src: ITEMS_RAYS / ITEMS_PIXELS / ITEMS_BEAMS / ITEMS_SURFELS, rt_render_rays' / rt_render_pixels' /
// rt_render_beams' / rt_render_surfels' instance of the variant (never instrumented; none for the BVH2 kernel)
PathKernel pick(int variant, bool stats, bool vn, ItemSource src = ITEMS_TILE)
{
    switch (variant) {
    case 1: return pick_brute<false, true>(stats, vn, src);
    case 2: return pick_brute<true, false>(stats, vn, src);
    case 3: return pick_brute<true, true>(stats, vn, src);
    case 4: return pick_bvh<2, 24, false>(stats, vn, src);
    case 5: return pick_bvh<2, 24, true>(stats, vn, src);
    case 6: return pick_bvh<4, RT_WIDE_STACK, false>(stats, vn, src);
    case 7: return pick_bvh<4, RT_WIDE_STACK, true>(stats, vn, src);
    default: return pick_brute<false, false>(stats, vn, src);
    }
}

PathScene make_path_scene(const DevScene& s)
{
    PathScene ps;
    for (int k = 0; k < 3; k++) ps.n_rect[k] = s.n_rect[k];
    ps.n_tri = s.n_tri;
    ps.n_sph = s.n_sph;
    ps.n_pln = s.n_pln;
    ps.n_bvh = s.pln0_bf; // set per order by launch_path
    ps.n_slots = ps.n_bvh + s.n_pln;
    ps.n_mats = s.n_mats;
    ps.n_xf = s.n_xf;
    ps.n_vn = s.n_vn;
    ps.facts = s.facts;
    ps.root = s.root;
    ps.width = s.width;
    ps.recursion = s.recursion;
    ps.debug_geom = s.debug_geom;
    ps.ambient_miss = s.ambient_miss;
    ps.air_ior = s.air_ior;
    ps.ambient_r = s.ambient.x;
    ps.ambient_g = s.ambient.y;
    ps.ambient_b = s.ambient.z;
    set_scene_bound(ps, s.bound);
    return ps;
}
} // namespace

int path_wide_stack() { return RT_WIDE_STACK; }

int debug_vn_rehit(const double v0[3], const double e01[3], const double e02[3], int mirror, double u, double v,
                   const float dir[3], int* inside, double* t, double o[3])
{
    PrimD P{};
    P.a = Vec4d{v0[0], v0[1], v0[2], 1.0};
    P.b = Vec4d{e01[0], e01[1], e01[2], 0.0};
    P.c = Vec4d{e02[0], e02[1], e02[2], 0.0};
    P.flags = mirror ? F_MIRROR : 0u;
    bool in = false;
    const bool hit = vn_rehit_test(P, u, v, V3{dir[0], dir[1], dir[2]}, in, t, o);
    *inside = in ? 1 : 0;
    return hit ? 1 : 0;
}

size_t path_lds_bytes(const DevScene& s)
{
    const size_t slots = (size_t)std::max(std::max(s.pln0_bf, s.pln0_gr), s.pln0_bvh) + s.n_pln;
    return slots * sizeof(PrimF) + (size_t)s.n_mats * sizeof(MatF) + (size_t)s.n_xf * sizeof(XformF);
}

int path_variant(int kernel, bool lds) { return kernel * 2 + (lds ? 1 : 0); }

bool hot_nodes_enabled()
{
    static const bool on = !(getenv("RTCORE_HOT_NODES") && getenv("RTCORE_HOT_NODES")[0] == '0'); // A/B switch
    return on;
}

size_t path_dyn_lds(const DevScene& s, int variant)
{
    size_t b = (variant & 1) ? path_lds_bytes(s) : 0;
    if ((variant >> 1) == 3 && s.n_hot4 > 0 && hot_nodes_enabled()) b += (size_t)s.n_hot4 * sizeof(Node4Q);
    return b;
}

int path_blocks_per_cu(int variant, size_t dyn_lds, bool stats, bool vn, ItemSource src)
{
    return blocks_per_cu(pick(variant, stats, vn, src), dyn_lds);
}

void fill_launch(const DevScene& s, int variant, PathParams& p)
{
    PathScene ps = make_path_scene(s);
    const int kernel = variant >> 1;
    ps.hot4 = nullptr;
    ps.n_hot4 = 0;
    if (kernel == 3) { // the wide kernel walks the collapsed tree, its top from the hot table
        ps.root = s.root4;
        if (s.n_hot4 > 0 && hot_nodes_enabled()) {
            ps.root = s.root4_hot;
            ps.hot4 = s.hot4;
            ps.n_hot4 = s.n_hot4;
        }
    }
    const bool grouped = kernel == 1, bvh = kernel >= 2;
    ps.n_groups = grouped ? s.n_groups_gr : bvh ? s.n_outer : 1;
    ps.n_bvh = bvh ? s.pln0_bvh : grouped ? s.pln0_gr : s.pln0_bf;
    ps.n_slots = ps.n_bvh + s.n_pln;
    p.scene = ps;
    p.tests = bvh ? s.tests_bvh : grouped ? s.tests_gr : s.tests_bf;
    p.rows = bvh ? s.rows_bvh : nullptr;
    p.rects = bvh ? s.rects_bvh : grouped ? s.rects_gr : s.rects_bf;
    p.frames = bvh ? s.frames_bvh : grouped ? s.frames_gr : s.frames_bf;
    p.prims = bvh ? s.prims_bvh : grouped ? s.prims_gr : s.prims_bf;
    p.groups = bvh ? s.groups_bvh : grouped ? s.groups_gr : s.groups_bf;
    p.nodes = s.nodes;
    p.nodes4 = s.nodes4;
    p.xf = s.xf;
    p.mats = s.mats;
    p.vnormals = s.vnormals;
    p.prims_d = s.prims_d;
}

hipError_t launch_path(const DevScene& s, const CameraF* d_cam, const PathParams* d_params, int variant,
                       int grid_blocks, hipStream_t stream, bool stats, ItemSource src)
{
    const PathKernel kernel = pick(variant, stats, s.n_vn > 0, src);
    if (!kernel) return hipErrorInvalidValue;
    PathParams h{}; // the same launch record as the device copy: the BVH kernels take it as arguments
    fill_launch(s, variant, h);
    PathScene ps = h.scene;
    const CameraF* ca = d_cam;
    const PathParams* pa = d_params;
    const TestRec* tests = h.tests;
    const RectRec* rects = h.rects;
    const FrameRec* frames = h.frames;
    const PrimF* prims = h.prims;
    const NodeF* nodes = s.nodes;
    const Node4Q* nodes4 = s.nodes4;
    const GroupRec* groups = h.groups;
    const XformF* xf = h.xf;
    const MatF* mats = h.mats;
    const float4* vn = h.vnormals;
    void* args[] = {&ps, &ca, &pa, &tests, &rects, &frames, &prims, &nodes, &nodes4, &groups, &xf, &mats, &vn};
    const size_t dyn = path_dyn_lds(s, variant);
    return hipLaunchKernel(reinterpret_cast<const void*>(kernel), dim3(grid_blocks), dim3(256), args, dyn, stream);
}

#endif // __HIPCC_RTC__
} // namespace rtc

#ifdef RT_SCENE_CONST
// The entry point of a scene-specialised build (rt_jit.cpp): RT_SCENE_CONST_GROUPED selects the
// grouped (culling) or the flat brute-force kernel; LDS staging of the shading records.
extern "C" __global__ void __launch_bounds__(256, RT_SCENE_CONST_GROUPED ? RT_GROUPED_WAVES : RT_PATH_WAVES)
    rt_path_const(const rtc::CameraF* __restrict__ camp, const rtc::PathParams* __restrict__ pp)
{
    rtc::path_body<RT_SCENE_CONST_GROUPED != 0, true, false, RT_SCENE_CONST_VN != 0>(camp, pp);
}
#endif
