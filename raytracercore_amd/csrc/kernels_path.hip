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
// The closest-hit query restates Scene.RayTrace semantics (Scene.cs:65-120, Primitive.cs:46-75)
// in fp32: strict-closest hit, Invert flipping Inside only, one-sided culling, and
// Util.RayHitMatches' self-hit rejection (Util.cs:179-192) restated as: a flat primitive
// is never re-hit by the ray leaving it; a sphere re-hit keeps only the far root when the
// ray heads into it (DESIGN.md §Self-hit rule).
//
// Brute-force traversal walks the primitive records with a wave-uniform index: the records
// come through the scalar data cache (s_load) into SGPRs and every lane tests every
// primitive branch-free.  BVH traversal keeps a per-lane stack in LDS.
#include "../../include/rtcore_rng.h"
#include "rt_kernels.h"
#include "rt_beam.h"
namespace rtc {
// Products with a scene or camera field.  In the scene-specialised build those fields are literals,
// and IEEE rules keep fmaf(0, x, y) as an instruction (x could be infinite, and y + 0 is not y for
// y = -0): axis-aligned cameras, rotation frames and two-sided rectangles carried ~20 such terms per
// query on bounce.txt.  A term whose literal factor is zero is dropped there; the generic kernel
// computes the same values except for the sign of an exact zero (x is always finite here).
__device__ __forceinline__ bool known_zero(float c)
{
#if defined(RT_SCENE_CONST)
    return __builtin_constant_p(c) && c == 0.0f;
#else
    (void)c;
    return false;
#endif
}
} // namespace rtc
#define RT_HAVE_KNOWN_ZERO
#include "rt_surfel.h"
#ifndef __HIPCC_RTC__ // (the probes' fold is no part of a scene-specialised build)
#include "rt_sh.h"
#include "rt_probe_error.h"
#endif
#ifdef RT_SCENE_CONST
// rt_jit.cpp generates this header per scene (and camera, for the grouped order): the launch's
// PathScene and its brute-force records as 32-bit words (kSceneW, kGroupsW, kRectsW, kFramesW,
// kTestsW, kXfW, kCameraW) and the camera switches (RT_SCENE_CAMERA_KIND / _DOF).  Every record
// field then folds into the instructions (literal operands cost what a VGPR operand does on
// gfx950, an SGPR operand twice that), the primitive loops unroll and the per-record flag branches
// resolve at compile time.  Included first, so that every macro it defines is seen by the code.
#include "rt_scene_const.h"
#endif

namespace rtc {
namespace {

// (V3 with its scaling, dot, cross, madd, kfma and fsqrt: rt_surfel.h, which shares them; known_zero: above)
__device__ __forceinline__ V3 xyz(float4 a) { return V3{a.x, a.y, a.z}; }
__device__ __forceinline__ V3 operator+(V3 a, V3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
__device__ __forceinline__ V3 operator-(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ V3 operator*(V3 a, V3 b) { return {a.x * b.x, a.y * b.y, a.z * b.z}; }
__device__ __forceinline__ V3 operator-(V3 a) { return {-a.x, -a.y, -a.z}; }
__device__ __forceinline__ float kmul(float a, float b) { return (known_zero(a) || known_zero(b)) ? -0.0f : a * b; }
__device__ __forceinline__ float dot4(float4 r, V3 p) { return kfma(r.x, p.x, kfma(r.y, p.y, kfma(r.z, p.z, r.w))); }
__device__ __forceinline__ float dot3(float4 r, V3 p) { return kfma(r.x, p.x, kfma(r.y, p.y, kmul(r.z, p.z))); }
__device__ __forceinline__ float rcp(float x) { return __builtin_amdgcn_rcpf(x); }
__device__ __forceinline__ V3 normalize(V3 a) { return a * __builtin_amdgcn_rsqf(dot(a, a)); }
__device__ __forceinline__ V3 xf_point(const float4* m, V3 p) { return {dot4(m[0], p), dot4(m[1], p), dot4(m[2], p)}; }
__device__ __forceinline__ V3 xf_dir(const float4* m, V3 p) { return {dot3(m[0], p), dot3(m[1], p), dot3(m[2], p)}; }

struct Best {
    float t; // world distance (Hit.Distance)
    int sg;  // slot << 1 | geometric inside (before Invert; selects the flipped normal); -1 = none
};
__device__ __forceinline__ int pack_sg(int slot, bool gin) { return (slot << 1) | (int)gin; }

// Triangle via the affine inverse record (TestRec): w(t) = 0 gives t, then (u, v).
// Inside (Moller-Trumbore's 1/det < 0, Triangle.cs:127) <=> d . n > 0 <=> dw > 0.
// Every kernel names the primitive a ray leaves by its slot (SLOT: id = slot, Sample.prev = slot): a
// hit-able primitive has exactly one slot in each order, the records of compact leaves carry no ID,
// and a box names its faces' slots by face index (sg0 / 2 + f) without a table.
__device__ __forceinline__ void hit_tri_rows(float4 r0, float4 r1, float4 r2, uint32_t fl, int id, int slot, V3 o, V3 d,
                                             int prev, Best& b)
{
    const float dw = dot3(r2, d);
    const float t = -dot4(r2, o) * rcp(dw);
    const float u = fmaf(t, dot3(r0, d), dot4(r0, o));
    const float v = fmaf(t, dot3(r1, d), dot4(r1, o));
    const bool gin = dw > 0.0f;
    bool ok = (t >= 0.0f) & (t < b.t) & (u >= 0.0f) & (v >= 0.0f) & (id != prev);
    ok &= (fl & F_MIRROR) ? ((u <= 1.0f) & (v <= 1.0f)) : (u + v <= 1.0f);
    if (!(fl & F_TWOSIDED)) ok &= !(gin ^ ((fl & F_INVERT) != 0)); // one-sided: cull Inside
    b.t = ok ? t : b.t;
    b.sg = ok ? pack_sg(slot, gin) : b.sg;
}
template <bool SLOT = false>
__device__ __forceinline__ void hit_tri(const TestRec& R, int slot, V3 o, V3 d, int prev, Best& b)
{
    hit_tri_rows(R.r0, R.r1, R.r2, __float_as_uint(R.meta.y), SLOT ? slot : __float_as_int(R.meta.x), slot, o, d, prev, b);
}

// Sphere (Sphere.cs:50-155).  Primitive.RayTrace returns the first surviving root: the close
// one (Inside = false) if it lies ahead and is not culled, otherwise the far one.
// WSKIP: the rest of the test is skipped, by a wave-uniform branch, when no lane's line meets the
// sphere and no lane leaves it.  The grouped brute-force order takes it (die.txt's pips, r = 0.15:
// C3 25.65 -> 23.56 ms), the flat order not (bounce.txt's large spheres: C2 18.43 -> 18.65 ms;
// the branch costs more than the waves that skip save); RT_SPH_WAVE_SKIP = 0 / 1 forces it off /
// on for both.  The box test skips its face choice the same way when no lane meets the box ahead
// (RT_BOX_WAVE_SKIP, default on: C2 18.43 -> 17.85 ms, bounce.txt's light box and rotated cube).
// Neither changes a result: the skipped part can report no hit.
#ifndef RT_SPH_WAVE_SKIP
#define RT_SPH_WAVE_SKIP -1
#endif
#ifndef RT_BOX_WAVE_SKIP
#define RT_BOX_WAVE_SKIP 1
#endif
// The scene bound's skip (path_body) in the grouped order too: off.  Its group and super-record boxes
// already reject a ray that looks past the scene after two box tests, so the skip saves nothing there
// and the guard costs (C3 20.22-20.28 -> 20.44-20.49 ms, die.txt 4K x 512 spp 39.66-39.73 -> 40.08-40.19).
#ifndef RT_BOUND_GROUPED
#define RT_BOUND_GROUPED 0
#endif
template <bool WSKIP = false, class XfP> // XfP: const XformF*, generic or in the constant address space
__device__ __forceinline__ void hit_sph_rows(float4 r0, float4 r1, uint32_t fl, int id, int slot, V3 o, V3 d, int prev,
                                             XfP xf, Best& b)
{
    V3 oo = o, dd = d;
    float k = 1.0f; // object-space ray parameter -> world distance
    if (fl & F_TRANSFORMED) {
        const XformF X = xf[__float_as_int(r1.y)];
        oo = xf_point(X.to_world, o);
        const V3 dl = xf_dir(X.to_world, d);
        k = __builtin_amdgcn_rsqf(dot(dl, dl)); // |to_obj * dd| = 1 / |to_world * d|
        dd = dl * k;
    }
    const V3 oc = oo - xyz(r0);
    const float bb = dot(oc, dd);
    const V3 l = madd(dd, -bb, oc);
    const float disc = r1.x - dot(l, l);
    const bool self = id == prev;
    if (WSKIP && !__any((disc >= 0.0f) | self)) return;
    const float sq = fsqrt(fmaxf(disc, 0.0f));
    // self-hit: the root at the bounce point is skipped; the other root is -2 (oc.dd)
    const float tn = self ? -1.0f : -bb - sq;
    const float tf = self ? -2.0f * bb : sq - bb;
    const bool any = self ? (bb < 0.0f) : ((disc >= 0.0f) & (tf >= 0.0f));
    const bool two = (fl & F_TWOSIDED) != 0, inv = (fl & F_INVERT) != 0;
    const bool use_close = any & (tn >= 0.0f) & (two | !inv);
    const bool use_far = !use_close & any & (two | inv);
    const float tc = use_close ? tn : tf;
    const float tw = tc * k;
    const bool ok = (use_close | use_far) & (tw < b.t);
    b.t = ok ? tw : b.t;
    b.sg = ok ? pack_sg(slot, use_far) : b.sg;
}
template <bool SLOT = false, bool WSKIP = false, class XfP>
__device__ __forceinline__ void hit_sph(const TestRec& R, int slot, V3 o, V3 d, int prev, XfP xf, Best& b)
{
    hit_sph_rows<WSKIP>(R.r0, R.r1, __float_as_uint(R.meta.y), SLOT ? slot : __float_as_int(R.meta.x), slot, o, d, prev,
                        xf, b);
}

// Plane (Plane.cs:36-66), including the NearlyEqual branch for rays in the plane.
template <bool SLOT = false>
__device__ __forceinline__ void hit_plane(const TestRec& R, int slot, V3 o, V3 d, int prev, Best& b)
{
    const int id = SLOT ? slot : __float_as_int(R.meta.x);
    const uint32_t fl = __float_as_uint(R.meta.y);
    const V3 n = xyz(R.r0);
    const float pd = R.r0.w;
    const float rd = dot(o, n), den = dot(d, n);
    const float t = (pd - rd) / den;
    const bool flat = den == 0.0f;
    const bool any = flat ? ((pd == rd) | (fmaxf(pd, rd) < 0.0f)) : (t >= -1e-24f);
    const float dist = flat ? 0.0f : fabsf(t);
    const bool gin = flat ? true : (den > 0.0f);
    bool ok = any & (id != prev) & (dist < b.t);
    if (!(fl & F_TWOSIDED)) ok &= !(gin ^ ((fl & F_INVERT) != 0));
    b.t = ok ? dist : b.t;
    b.sg = ok ? pack_sg(slot, gin) : b.sg;
}

// The planes of a scene: the records that follow the other primitives (n_bvh of them) in every slot order.
template <class SceneT, class TestP>
__device__ __forceinline__ void test_planes(const SceneT& s, TestP tests, V3 o, V3 d, int prev, Best& b)
{
    const int pln0 = s.n_bvh;
    for (int k = pln0; k < pln0 + s.n_pln; k++) {
        const TestRec tr = tests[k];
        hit_plane<true>(tr, k, o, d, prev, b);
    }
}

// Axis-aligned rectangle on plane `AXIS` (RectRec): the same hit as the Mirror parallelogram
// test (u, v in [0, 1]^2) with the extents in world units.  id = 1 / d, oi = o / d.  The side
// of the hit (Inside) is not tracked here: the shading step recomputes it from the normal.
// SUB: oi holds o itself and t = (c - o) / d (one fewer live vector than the fma form)
template <int AXIS, bool SUB = false>
__device__ __forceinline__ void hit_rect(const RectRec& R, int sg, V3 o, V3 d, V3 id, V3 oi, int prev, Best& b)
{
    const float ida = AXIS == 0 ? id.x : AXIS == 1 ? id.y : id.z;
    const float oia = AXIS == 0 ? oi.x : AXIS == 1 ? oi.y : oi.z;
    const float da = AXIS == 0 ? d.x : AXIS == 1 ? d.y : d.z;
    const float d1 = AXIS == 0 ? d.y : d.x, o1 = AXIS == 0 ? o.y : o.x;
    const float d2 = AXIS == 2 ? d.y : d.z, o2 = AXIS == 2 ? o.y : o.z;
    const float t = SUB ? (R.c - oia) * ida : fmaf(R.c, ida, -oia);
    // |p - mid| <= half on both in-plane axes (false for NaN)
    const bool in1 = fabsf(fmaf(t, d1, o1) - R.m1) <= R.h1;
    const bool in2 = fabsf(fmaf(t, d2, o2) - R.m2) <= R.h2;
    // 0 <= t < best as one unsigned compare of the bit patterns (b.t >= 0; NaN and -t fail)
    const bool near = __float_as_uint(t) < __float_as_uint(b.t);
    const bool ok = near & in1 & in2 & (kmul(R.cull, da) <= 0.0f) & ((R.sg >> 1) != prev); // prev: a slot
    b.t = ok ? t : b.t; // the shading step rebuilds the hit point from t
    b.sg = ok ? sg : b.sg;
}

template <int AXIS, bool SUB = false, class RectP>
__device__ __forceinline__ void rect_group(RectP r, int n, V3 o, V3 d, V3 id, V3 oi, int prev, Best& b)
{
    for (; n >= 2; n -= 2, r += 2) {
        const RectRec r0 = r[0], r1 = r[1];
        hit_rect<AXIS, SUB>(r0, r0.sg, o, d, id, oi, prev, b);
        hit_rect<AXIS, SUB>(r1, r1.sg, o, d, id, oi, prev, b);
    }
    if (n > 0) {
        const RectRec r0 = r[0];
        hit_rect<AXIS, SUB>(r0, r0.sg, o, d, id, oi, prev, b);
    }
}

// Min / max as the bare VALU instructions.  fminf / fmaxf of values the compiler cannot prove
// canonical (here: slab distances that pass through the sphere tests' divergent branches) get a
// v_max_f32 x, x, x quieting each operand first; our operands are never signalling NaNs, and a
// quiet NaN operand is ignored either way (IEEE minNum), so the bare instruction is the same min.
__device__ __forceinline__ float vmin(float a, float b)
{
    float r;
    asm("v_min_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
__device__ __forceinline__ float vmax(float a, float b)
{
    float r;
    asm("v_max_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}

__device__ __forceinline__ float vmax3(float a, float b, float c)
{
    float r;
    asm("v_max3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}
__device__ __forceinline__ float vmin3(float a, float b, float c)
{
    float r;
    asm("v_min3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}
__device__ __forceinline__ float vmax0(float a)
{
    float r;
    asm("v_max_f32 %0, 0, %1" : "=v"(r) : "v"(a));
    return r;
}
__device__ __forceinline__ float vmax1(float a)
{
    float r;
    asm("v_max_f32 %0, 1.0, %1" : "=v"(r) : "v"(a));
    return r;
}

// Closed box (BoxRec): one slab test gives the entry and exit distances and faces; each is a
// hit when it lies in [0, best), its face keeps hits from that side (culling) and it is not the
// face the ray leaves (self-hit).  The entry wins when both are hits.  Equivalent to testing the
// six faces as rectangles (a convex box is met at most twice), up to ties on its edges.
// SUB: oi holds o itself (frame-local rays), as in hit_rect.
template <bool SUB>
__device__ __forceinline__ void hit_box(const BoxRec& B, V3 o, V3 d, V3 id, V3 oi, int prev, Best& b)
{
    const float lx = SUB ? (B.lo.x - oi.x) * id.x : fmaf(B.lo.x, id.x, -oi.x);
    const float hx = SUB ? (B.hi.x - oi.x) * id.x : fmaf(B.hi.x, id.x, -oi.x);
    const float ly = SUB ? (B.lo.y - oi.y) * id.y : fmaf(B.lo.y, id.y, -oi.y);
    const float hy = SUB ? (B.hi.y - oi.y) * id.y : fmaf(B.hi.y, id.y, -oi.y);
    const float lz = SUB ? (B.lo.z - oi.z) * id.z : fmaf(B.lo.z, id.z, -oi.z);
    const float hz = SUB ? (B.hi.z - oi.z) * id.z : fmaf(B.hi.z, id.z, -oi.z);
    const float nx = vmin(lx, hx), ny = vmin(ly, hy), nz = vmin(lz, hz);
    const float fx = vmax(lx, hx), fy = vmax(ly, hy), fz = vmax(lz, hz);
    const float te = vmax3(nx, ny, nz), tx = vmin3(fx, fy, fz);
    const bool meet = te <= tx;
    if (RT_BOX_WAVE_SKIP && !__any(meet & (tx >= 0.0f))) return; // no lane meets the box ahead
    // the ray enters axis a's slab by its lower plane (side 0) when d[a] > 0
    const int sx = (int)(__float_as_uint(d.x) >> 31), sy = (int)(__float_as_uint(d.y) >> 31),
              sz = (int)(__float_as_uint(d.z) >> 31);
    const uint32_t keep = B.keep;
    const uint32_t rel_prev = (uint32_t)(prev - (B.sg0 >> 1)); // the face slot the ray leaves, relative to face 0
    bool ok_e = false, ok_x = false;
    int fe = 0, fo = 0;
    if (keep & 0x3Fu) { // some face keeps entry hits (wave-uniform)
        fe = te == nx ? sx : (te == ny ? 2 + sy : 4 + sz);
        // the keep bit is tested unconditionally: selecting on "every face keeps" cost more, and
        // folding that case in the scene-specialised build measured no change (round 3)
        ok_e = meet & (__float_as_uint(te) < __float_as_uint(b.t)) & ((uint32_t)fe != rel_prev) &
               (((keep >> fe) & 1u) != 0);
    }
    if (keep & 0x3F00u) { // some face keeps exit hits
        fo = tx == fx ? 1 - sx : (tx == fy ? 3 - sy : 5 - sz);
        ok_x = meet & (__float_as_uint(tx) < __float_as_uint(b.t)) & ((uint32_t)fo != rel_prev) &
               (((keep >> (8 + fo)) & 1u) != 0);
    }
    const bool ok = ok_e | ok_x;
    b.t = ok ? (ok_e ? te : tx) : b.t;
    b.sg = ok ? B.sg0 + 2 * (ok_e ? fe : fo) : b.sg;
}

// 1/d for the box tests, with |d| clamped to >= 2^-64 so that an axis-parallel ray (d = 0 on an
// axis, e.g. a diffuse bounce whose angle draw is exactly 0) gives large finite slab distances of
// the right sign instead of 0 * inf = NaN, which the min/max chains would ignore (a box the ray
// runs parallel to and outside of would then count as hit, and the query would visit every node).
__device__ __forceinline__ float slab_rcp(float d)
{
    return rcp(fabsf(d) >= 5.421010862e-20f ? d : __builtin_copysignf(5.421010862e-20f, d));
}
// The brute-force kernels' form: the reciprocal clamped to +-2^64 by one v_med3 instead of a
// compare, a select and a sign insert before it; the same value for every finite or zero d
// (1/(+-0) = +-inf clamps to +-2^64 = 1/(+-2^-64)).  A NaN d (a vertex-normal triangle's NaN
// normal) gets a finite +-2^64 here, so a box test could report a hit for it: path_body ends such
// a query as a miss, as the reference's BVH root test does.
__device__ __forceinline__ float slab_rcp_lean(float d)
{
    return __builtin_amdgcn_fmed3f(rcp(d), -0x1p64f, 0x1p64f);
}

// BARE (the brute-force kernels' group boxes): the per-axis min / max as bare instructions (vmin,
// vmax), which drops the compiler's NaN quieting of their operands; same values.
template <bool BARE = false>
__device__ __forceinline__ bool slab(float4 lo, float4 hi, V3 oi, V3 id, float tmax, float& tnear)
{
    // t = box * (1/d) - o * (1/d); NaN from 0*inf is ignored by fminf/fmaxf (conservative)
    const float tx0 = fmaf(lo.x, id.x, -oi.x), tx1 = fmaf(hi.x, id.x, -oi.x);
    const float ty0 = fmaf(lo.y, id.y, -oi.y), ty1 = fmaf(hi.y, id.y, -oi.y);
    const float tz0 = fmaf(lo.z, id.z, -oi.z), tz1 = fmaf(hi.z, id.z, -oi.z);
    const float nx = BARE ? vmin(tx0, tx1) : fminf(tx0, tx1), fx = BARE ? vmax(tx0, tx1) : fmaxf(tx0, tx1);
    const float ny = BARE ? vmin(ty0, ty1) : fminf(ty0, ty1), fy = BARE ? vmax(ty0, ty1) : fmaxf(ty0, ty1);
    const float nz = BARE ? vmin(tz0, tz1) : fminf(tz0, tz1), fz = BARE ? vmax(tz0, tz1) : fmaxf(tz0, tz1);
    const float tmin = BARE ? vmax3(nx, ny, vmax0(nz)) : fmaxf(fmaxf(nx, ny), fmaxf(nz, 0.0f));
    const float tmx = BARE ? vmin3(fx, fy, vmin(fz, tmax)) : fminf(fminf(fx, fy), fminf(fz, tmax));
    tnear = tmin;
    return tmin <= tmx * 1.00000024f;
}

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

// Every primitive, group by group (GroupRec: x-rects | y-rects | z-rects | triangles | spheres).
// The loop indices are wave-uniform, so the records arrive through scalar loads.  With CULL a
// group is skipped when no lane of the wave meets its box before its current closest hit, and
// with it the G.skip records that follow it (a super record: the box of a subtree of groups, no
// primitives of its own).  The skip is a wave-uniform bound (skip_to), not a jump of the loop
// index, so the scene-specialised build still unrolls the loop.
// The record pointers are in the constant address space (RT_AS_CONST) or generic.
// boxes: the frame array viewed as BoxRecs (they share it).
// ANY (rt_occluded_rays): the query is over once b.sg >= 0.  A lane with its answer no longer votes
// for a group's box, and the wave leaves as soon as no active lane is without one: between groups
// in the grouped order, between the record classes in the flat one.  The bounds stay wave-uniform.
template <bool CULL, bool STATS, bool ANY = false, class SceneT, class GroupP, class TestP, class RectP, class FrameP,
          class BoxP, class XfP>
__device__ __forceinline__ void trace_brute(const SceneT& s, GroupP groups, TestP tests, RectP rects, FrameP frames,
                                            BoxP boxes, XfP xf, V3 o, V3 d, int prev, Best& b, unsigned& n_flat,
                                            unsigned& n_sph, unsigned& n_node)
{
    const V3 id = v3(slab_rcp_lean(d.x), slab_rcp_lean(d.y), slab_rcp_lean(d.z));
    const V3 oi = o * id;
    const int n_groups = CULL ? s.n_groups : 1; // the flat order is one group (1/d and o/d die after its rects)
    int skip_to = 0;
#ifdef RT_SCENE_CONST
#pragma unroll // the scene-specialised build: every group's tests in line, their records literals
#endif
    for (int g = 0; g < n_groups; g++) {
        if (CULL && g < skip_to) continue;
        const GroupRec G = groups[g];
        if (CULL) {
            if (STATS) n_node++; // the group's box: a node of a shallow tree (SURVEY 8(d) N_node)
            float tn;
            if (!__any((!ANY || b.sg < 0) && slab<true>(G.lo, G.hi, oi, id, b.t, tn))) {
                skip_to = g + 1 + G.skip;
                continue;
            }
        }
        if (STATS) { // primitive tests actually made (groups the wave skipped are not counted)
            n_flat += G.n_rect[0] + G.n_rect[1] + G.n_rect[2] + G.n_flat_extra + (G.n_tri_sph & 0xFFFF);
            n_sph += G.n_tri_sph >> 16;
        }
        RectP r = rects + __float_as_int(G.lo.w);
        rect_group<0>(r, G.n_rect[0], o, d, id, oi, prev, b);
        r += G.n_rect[0];
        rect_group<1>(r, G.n_rect[1], o, d, id, oi, prev, b);
        r += G.n_rect[1];
        rect_group<2>(r, G.n_rect[2], o, d, id, oi, prev, b);
        for (int j = G.frame_first + G.n_frames; j < G.frame_first + G.n_frames + G.n_boxes; j++) {
            const BoxRec B = boxes[j];
            hit_box<false>(B, o, d, id, oi, prev, b);
        }
        if (ANY && !CULL && !__any(b.sg < 0)) return;
        // rectangles in a common affine frame: the ray mapped once, then the same rect tests (t is
        // invariant under the map; a local d of 0 gives an infinite or NaN t, which never hits)
        for (int f = G.frame_first; f < G.frame_first + G.n_frames; f++) {
            const FrameRec F = frames[f];
            const V3 lo = v3(dot4(F.r0, o), dot4(F.r1, o), dot4(F.r2, o));
            const V3 ld = v3(dot3(F.r0, d), dot3(F.r1, d), dot3(F.r2, d));
            const V3 lid = v3(rcp(ld.x), rcp(ld.y), rcp(ld.z));
            RectP fr = rects + F.rect_first;
            rect_group<0, true>(fr, F.n_rect[0], lo, ld, lid, lo, prev, b);
            fr += F.n_rect[0];
            rect_group<1, true>(fr, F.n_rect[1], lo, ld, lid, lo, prev, b);
            fr += F.n_rect[1];
            rect_group<2, true>(fr, F.n_rect[2], lo, ld, lid, lo, prev, b);
            if (F.box >= 0) {
                const BoxRec B = boxes[F.box];
                hit_box<true>(B, lo, ld, lid, lo, prev, b);
            }
        }
        if (ANY && !CULL && !__any(b.sg < 0)) return;
        int i = __float_as_int(G.hi.w);
        int end = i + (G.n_tri_sph & 0xFFFF);
        if (i < end) {
            TestRec cur = tests[i];
            for (; i < end; i++) {
                const TestRec nxt = tests[i + 1];
                hit_tri<true>(cur, i, o, d, prev, b);
                cur = nxt;
            }
        }
        if (ANY && !CULL && !__any(b.sg < 0)) return;
        end = i + (G.n_tri_sph >> 16);
        if (i < end) {
            TestRec cur = tests[i];
            for (; i < end; i++) {
                const TestRec nxt = tests[i + 1];
                hit_sph<true, RT_SPH_WAVE_SKIP < 0 ? CULL : RT_SPH_WAVE_SKIP != 0>(cur, i, o, d, prev, xf, b);
                cur = nxt;
            }
        }
        if (ANY && CULL && !__any(b.sg < 0)) return;
    }
}

// The flat order's query for a wave of camera rays of one 8x8 block (path_body, first bounce): trace_brute's
// one group with each test unit (rt_kernels.h, flat_unit_count) behind a scalar test of its bit in the
// block's mask.  The tests, their order and their operands are trace_brute's, so the units that run
// leave b as they do there; the units left out cannot be met by these rays (unit_masks).
#ifdef RT_SCENE_CONST
#define RT_UNROLL_UNITS _Pragma("unroll")
#else
#define RT_UNROLL_UNITS
#endif
template <class GroupP, class TestP, class RectP, class FrameP, class BoxP, class XfP>
__device__ __forceinline__ void trace_units(GroupP groups, TestP tests, RectP rects, FrameP frames, BoxP boxes, XfP xf,
                                            V3 o, V3 d, int prev, Best& b, unsigned long long mask)
{
    const V3 id = v3(slab_rcp_lean(d.x), slab_rcp_lean(d.y), slab_rcp_lean(d.z));
    const V3 oi = o * id;
    const GroupRec G = groups[0];
    auto on = [&]() { // the next unit's bit (wave-uniform): the units come in the mask's order
        const bool t = (mask & 1ull) != 0ull;
        mask >>= 1;
        return t;
    };
    RectP r = rects + __float_as_int(G.lo.w);
    RT_UNROLL_UNITS
    for (int k = 0; k < G.n_rect[0]; k++)
        if (on()) {
            const RectRec r0 = r[k];
            hit_rect<0>(r0, r0.sg, o, d, id, oi, prev, b);
        }
    r += G.n_rect[0];
    RT_UNROLL_UNITS
    for (int k = 0; k < G.n_rect[1]; k++)
        if (on()) {
            const RectRec r0 = r[k];
            hit_rect<1>(r0, r0.sg, o, d, id, oi, prev, b);
        }
    r += G.n_rect[1];
    RT_UNROLL_UNITS
    for (int k = 0; k < G.n_rect[2]; k++)
        if (on()) {
            const RectRec r0 = r[k];
            hit_rect<2>(r0, r0.sg, o, d, id, oi, prev, b);
        }
    RT_UNROLL_UNITS
    for (int j = G.frame_first + G.n_frames; j < G.frame_first + G.n_frames + G.n_boxes; j++)
        if (on()) {
            const BoxRec B = boxes[j];
            hit_box<false>(B, o, d, id, oi, prev, b);
        }
    RT_UNROLL_UNITS
    for (int f = G.frame_first; f < G.frame_first + G.n_frames; f++)
        if (on()) {
            const FrameRec F = frames[f];
            const V3 lo = v3(dot4(F.r0, o), dot4(F.r1, o), dot4(F.r2, o));
            const V3 ld = v3(dot3(F.r0, d), dot3(F.r1, d), dot3(F.r2, d));
            const V3 lid = v3(rcp(ld.x), rcp(ld.y), rcp(ld.z));
            RectP fr = rects + F.rect_first;
            rect_group<0, true>(fr, F.n_rect[0], lo, ld, lid, lo, prev, b);
            fr += F.n_rect[0];
            rect_group<1, true>(fr, F.n_rect[1], lo, ld, lid, lo, prev, b);
            fr += F.n_rect[1];
            rect_group<2, true>(fr, F.n_rect[2], lo, ld, lid, lo, prev, b);
            if (F.box >= 0) {
                const BoxRec B = boxes[F.box];
                hit_box<true>(B, lo, ld, lid, lo, prev, b);
            }
        }
    int i = __float_as_int(G.hi.w);
    const int tri_end = i + (G.n_tri_sph & 0xFFFF);
    RT_UNROLL_UNITS
    for (; i < tri_end; i++)
        if (on()) {
            const TestRec cur = tests[i];
            hit_tri<true>(cur, i, o, d, prev, b);
        }
    const int sph_end = i + (G.n_tri_sph >> 16);
    RT_UNROLL_UNITS
    for (; i < sph_end; i++)
        if (on()) {
            const TestRec cur = tests[i];
            hit_sph<true, RT_SPH_WAVE_SKIP < 0 ? false : RT_SPH_WAVE_SKIP != 0>(cur, i, o, d, prev, xf, b);
        }
}

template <bool SLOT = false, class XfP>
__device__ __forceinline__ void hit_any(const TestRec& R, int slot, V3 o, V3 d, int prev, XfP xf, Best& b)
{
    switch (__float_as_uint(R.meta.y) & KIND_MASK) {
    case RT_PRIM_TRIANGLE: hit_tri<SLOT>(R, slot, o, d, prev, b); break;
    case RT_PRIM_SPHERE: hit_sph<SLOT>(R, slot, o, d, prev, xf, b); break;
    default: hit_plane<SLOT>(R, slot, o, d, prev, b); break;
    }
}

// The pending leaf of a BVH query is one register: the leaf code (rt_internal.h) whose count field
// holds the primitives still to test, minus one; -1 when no leaf is pending.  A leaf step decodes
// its slots and, for a compact leaf, the record flags its primitives share (leaf_flags);
// kLeafGeneric for a generic leaf (flags from each record's meta row).
constexpr uint32_t kLeafGeneric = 0xFFFFFFFFu;
__device__ __forceinline__ void leaf_decode(int pend, int& k, int& kend, uint32_t& lfl)
{
    const bool compact = (pend & kLeafCompact) != 0;
    k = compact ? (pend >> 2) & (kLeafCompactMaxFirst - 1) : pend >> 3;
    kend = k + (pend & (compact ? 3 : 7)) + 1;
    lfl = compact ? leaf_flags(((uint32_t)pend >> 25) & 31u) : kLeafGeneric;
}
// after a step of n primitives: the first slot advanced by n and the count field lowered by n, or -1
__device__ __forceinline__ int leaf_advance(int pend, int n)
{
    const bool compact = (pend & kLeafCompact) != 0;
    const int left = pend & (compact ? 3 : 7);
    return left >= n ? pend + (compact ? (n << 2) - n : (n << 3) - n) : -1;
}



// One visit of a 4-wide quantised node (Node4Q): slab tests of the four children against
// dequantised planes t = q * (2^e / d) + (origin - o) / d, nearest hit child next, the other hit
// children pushed far-to-near.  pop stays true when no child is hit.
__device__ __forceinline__ float ubyte(uint32_t v, int k) { return (float)((v >> (8 * k)) & 255u); }
__device__ __forceinline__ void cswap(float& da, int& ra, float& db, int& rb)
{
    const bool sw = db < da;
    const float t = da;
    const int r = ra;
    da = sw ? db : da;
    ra = sw ? rb : ra;
    db = sw ? t : db;
    rb = sw ? r : rb;
}
// Per-lane traversal stack: the first STACK entries in LDS (stride 256 = the block's lanes), deeper
// entries in a global overflow area (stride = all lanes of the grid), reached only by rare deep
// paths; the host bounds the depth any ray can need by STACK + RT_STACK_OVF.
// The two parts are typed by address space: with plain pointers the compiler merged the LDS and the
// overflow access of push / pop into one flat access through a selected pointer (a flat store or
// load, plus the pointer arithmetic, on every push and pop, and through the texture addresser).
// The bases are wave-uniform and the lane's offset is formed at use: per-lane pointers held across
// the loop were spilled to scratch and reloaded at every push (C4 52.4 -> 66.6 ms).
#define RT_STACK_OVF 44 // = kStackOverflow (rt_kernels.h); with the 16-entry LDS stacks, 60 entries in all
typedef __attribute__((address_space(3))) int LdsInt;
typedef __attribute__((address_space(1))) int GlobalInt;
struct TravStack {
    LdsInt* lds;    // the block's stack array (entry e of thread t at e * 256 + t)
    GlobalInt* ovf; // the grid's overflow area (entry e of global thread g at e * grid threads + g)
};
__device__ __forceinline__ TravStack make_stack(int* lds_base, int* ovf_base)
{
    return TravStack{(LdsInt*)lds_base, (GlobalInt*)ovf_base};
}
__device__ __forceinline__ unsigned ovf_slot(int e)
{
    return (unsigned)e * (gridDim.x * 256u) + blockIdx.x * 256u + threadIdx.x;
}
template <int STACK>
__device__ __forceinline__ void push(const TravStack& st, int& sp, int v)
{
    if (sp < STACK) st.lds[sp * 256 + (int)threadIdx.x] = v;
    else st.ovf[ovf_slot(sp - STACK)] = v;
    sp++;
}
template <int STACK>
__device__ __forceinline__ int pop_ref(const TravStack& st, int& sp)
{
    --sp;
    return sp < STACK ? st.lds[sp * 256 + (int)threadIdx.x] : st.ovf[ovf_slot(sp - STACK)];
}

__device__ __forceinline__ void pin4(float4& f)
{
    typedef float F4 __attribute__((ext_vector_type(4)));
    F4 v = {f.x, f.y, f.z, f.w};
    asm volatile("" : "+v"(v));
    f = make_float4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ void pin_rec(TestRec& t)
{
    pin4(t.r0);
    pin4(t.r1);
    pin4(t.r2);
    pin4(t.meta);
}
template <int STACK>
__device__ __forceinline__ void wide_visit(const Node4Q& q, V3 id, V3 oi, float best, int& ref, int& sp,
                                           const TravStack& stk, bool& pop)
{
    const uint32_t ex = __float_as_uint(q.a.w);
    const float ax = __builtin_amdgcn_ldexpf(id.x, (int)(ex & 255u) - 128);
    const float ay = __builtin_amdgcn_ldexpf(id.y, (int)((ex >> 8) & 255u) - 128);
    const float az = __builtin_amdgcn_ldexpf(id.z, (int)((ex >> 16) & 255u) - 128);
    const float bx = fmaf(q.a.x, id.x, -oi.x), by = fmaf(q.a.y, id.y, -oi.y), bz = fmaf(q.a.z, id.z, -oi.z);
    const uint32_t lx = __float_as_uint(q.b.x), hx = __float_as_uint(q.b.y);
    const uint32_t ly = __float_as_uint(q.b.z), hy = __float_as_uint(q.b.w);
    const uint32_t lz = __float_as_uint(q.c.x), hz = __float_as_uint(q.c.y);
    // near / far planes by the direction's sign
    const uint32_t nx = id.x >= 0.0f ? lx : hx, fx = id.x >= 0.0f ? hx : lx;
    const uint32_t ny = id.y >= 0.0f ? ly : hy, fy = id.y >= 0.0f ? hy : ly;
    const uint32_t nz = id.z >= 0.0f ? lz : hz, fz = id.z >= 0.0f ? hz : lz;
    const int nc = __float_as_int(q.d.z);
    float d0, d1, d2, d3;
    int r0 = __float_as_int(q.c.z), r1 = __float_as_int(q.c.w), r2 = __float_as_int(q.d.x), r3 = __float_as_int(q.d.y);
    const float tmax_best = best * 1.00000024f;
#define RT_WIDE_CHILD(K, D)                                                                                       \
    {                                                                                                             \
        const float tmin = fmaxf(fmaxf(fmaxf(fmaf(ubyte(nx, K), ax, bx), fmaf(ubyte(ny, K), ay, by)),              \
                                       fmaf(ubyte(nz, K), az, bz)), 0.0f);                                         \
        const float tmax = fminf(fminf(fmaf(ubyte(fx, K), ax, bx), fmaf(ubyte(fy, K), ay, by)),                   \
                                 fmaf(ubyte(fz, K), az, bz));                                                      \
        D = ((K < nc) & (tmin <= fminf(tmax * 1.00000024f, tmax_best))) ? tmin : __builtin_huge_valf();         \
    } // (K < nc) without short-circuit: "&&" made each child a divergent branch.  The test stays although
      // an empty slot's box is inverted (quantize_node4): inverted only up to the fp32 rounding of the
      // planes, and a hit on an empty slot would push RT_NODE4_EMPTY (round 4: dropping it saved 0.6 %)
    RT_WIDE_CHILD(0, d0)
    RT_WIDE_CHILD(1, d1)
    RT_WIDE_CHILD(2, d2)
    RT_WIDE_CHILD(3, d3)
#undef RT_WIDE_CHILD
    cswap(d0, r0, d1, r1);
    cswap(d2, r2, d3, r3);
    cswap(d0, r0, d2, r2);
    cswap(d1, r1, d3, r3);
    cswap(d1, r1, d2, r2);
    const float inf = __builtin_huge_valf();
    if (d0 < inf) {
        if (d3 < inf) push<STACK>(stk, sp, r3);
        if (d2 < inf) push<STACK>(stk, sp, r2);
        if (d1 < inf) push<STACK>(stk, sp, r1);
        ref = r0;
        pop = false;
    }
}

// One visit of a 4-wide node for an any-hit query: wide_visit's four slab tests against the segment's
// end, without the sorting network (no child is nearer in any sense that matters).  The first hit
// child in slot order is entered and the other hit children are pushed, to be popped in slot order.
template <int STACK>
__device__ __forceinline__ void any_visit(const Node4Q& q, V3 id, V3 oi, float best, int& ref, int& sp,
                                          const TravStack& stk, bool& pop)
{
    const uint32_t ex = __float_as_uint(q.a.w);
    const float ax = __builtin_amdgcn_ldexpf(id.x, (int)(ex & 255u) - 128);
    const float ay = __builtin_amdgcn_ldexpf(id.y, (int)((ex >> 8) & 255u) - 128);
    const float az = __builtin_amdgcn_ldexpf(id.z, (int)((ex >> 16) & 255u) - 128);
    const float bx = fmaf(q.a.x, id.x, -oi.x), by = fmaf(q.a.y, id.y, -oi.y), bz = fmaf(q.a.z, id.z, -oi.z);
    const uint32_t lx = __float_as_uint(q.b.x), hx = __float_as_uint(q.b.y);
    const uint32_t ly = __float_as_uint(q.b.z), hy = __float_as_uint(q.b.w);
    const uint32_t lz = __float_as_uint(q.c.x), hz = __float_as_uint(q.c.y);
    const bool px = id.x >= 0.0f, py = id.y >= 0.0f, pz = id.z >= 0.0f; // near / far planes by the direction's sign
    const uint32_t nx = px ? lx : hx, fx = px ? hx : lx;
    const uint32_t ny = py ? ly : hy, fy = py ? hy : ly;
    const uint32_t nz = pz ? lz : hz, fz = pz ? hz : lz;
    const int nc = __float_as_int(q.d.z);
    const int r0 = __float_as_int(q.c.z), r1 = __float_as_int(q.c.w), r2 = __float_as_int(q.d.x), r3 = __float_as_int(q.d.y);
    const float tmax_best = best * 1.00000024f;
    bool h0, h1, h2, h3;
#define RT_ANY_CHILD(K, H)                                                                                        \
    {                                                                                                             \
        const float tmin = fmaxf(fmaxf(fmaxf(fmaf(ubyte(nx, K), ax, bx), fmaf(ubyte(ny, K), ay, by)),              \
                                       fmaf(ubyte(nz, K), az, bz)), 0.0f);                                         \
        const float tmax = fminf(fminf(fmaf(ubyte(fx, K), ax, bx), fmaf(ubyte(fy, K), ay, by)),                   \
                                 fmaf(ubyte(fz, K), az, bz));                                                      \
        H = (K < nc) & (tmin <= fminf(tmax * 1.00000024f, tmax_best));                                            \
    } // the same test as RT_WIDE_CHILD (wide_visit)
    RT_ANY_CHILD(0, h0)
    RT_ANY_CHILD(1, h1)
    RT_ANY_CHILD(2, h2)
    RT_ANY_CHILD(3, h3)
#undef RT_ANY_CHILD
    if (h0 | h1 | h2 | h3) {
        if (h3 & (h0 | h1 | h2)) push<STACK>(stk, sp, r3);
        if (h2 & (h0 | h1)) push<STACK>(stk, sp, r2);
        if (h1 & h0) push<STACK>(stk, sp, r1);
        ref = h0 ? r0 : h1 ? r1 : h2 ? r2 : r3;
        pop = false;
    }
}

// A hot node read from LDS, its rows through a pointer typed by the address space (as TravStack's):
// as a copy from a plain pointer the compiler merged this read with the read from global memory on
// the other side of the choice (walk_step's fetch) into flat loads through a selected pointer.
typedef float F4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) F4 LdsF4;
__device__ __forceinline__ Node4Q lds_node(const LdsF4* rows, int i)
{
    const F4 a = rows[4 * i], b = rows[4 * i + 1], c = rows[4 * i + 2], d = rows[4 * i + 3];
    return Node4Q{make_float4(a.x, a.y, a.z, a.w), make_float4(b.x, b.y, b.z, b.w), make_float4(c.x, c.y, c.z, c.w),
                  make_float4(d.x, d.y, d.z, d.w)};
}

// One visit of a BVH2 node, to wide_visit's contract: the nearer hit child next, the other pushed.
template <int STACK>
__device__ __forceinline__ void bvh2_visit(const NodeF& n, V3 id, V3 oi, float best, int& ref, int& sp,
                                           const TravStack& stk, bool& pop)
{
    float tl, tr;
    const bool hl = slab(n.lmin, n.lmax, oi, id, best, tl);
    const bool hr = slab(n.rmin, n.rmax, oi, id, best, tr);
    const int cl = __float_as_int(n.lmin.w), cr = __float_as_int(n.rmin.w);
    if (hl && hr) {
        const bool lf = tl <= tr;
        push<STACK>(stk, sp, lf ? cr : cl);
        ref = lf ? cl : cr;
        pop = false;
    } else if (hl | hr) {
        ref = hl ? cl : cr;
        pop = false;
    }
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

#ifndef RT_PATH_WAVES
#define RT_PATH_WAVES 7 // minimum waves per SIMD the register allocator must allow (brute force; 6 -> 7: C2 28.4 -> 27.5 ms)
#endif
#ifndef RT_GROUPED_WAVES
#define RT_GROUPED_WAVES 7 // the same for the grouped brute-force kernel
#endif
#ifndef RT_WIDE_STACK
#define RT_WIDE_STACK 16 // LDS entries of the wide BVH kernel's traversal stack (then global overflow): 7 blocks per CU
#endif
#ifndef RT_SPEC_PRIMS
#define RT_SPEC_PRIMS 2 // leaf primitives per leaf step (<= kTestSpares + 1)
#endif
#ifndef RT_BVH_WAVES
#define RT_BVH_WAVES 7 // the same for the BVH kernels (C4: 4 waves with a 40-entry LDS stack 80.7 ms, 5 waves with 24 entries
                       // 72.0 ms; with the launch record read at use, 6 waves with 20 entries (8 VGPRs spilled) 57.2-58.6
                       // against 60.7-61.3 ms at 5 / 24; 7 waves with 16 entries spilled 27 VGPRs: 70.1 ms.  Round 3,
                       // after compact leaves (one register of pending-leaf state) and o/d recomputed per node visit:
                       // 6 waves / 20 entries 45.9 ms (2 spilled), 7 waves / 16 entries 45.0 ms (17 spilled))
#endif
#ifndef RT_BVH2_WAVES
#define RT_BVH2_WAVES 6 // the BVH2 kernel (24-entry LDS stack: at most 6 blocks per CU)
#endif

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

// A caller's ray (rt_query_rays, rt_render_rays): it arrives as rt_ray (fp64, four 16-B rows) and is
// rounded to fp32 component by component.  valid: every component finite (before and after the
// rounding) and the direction not zero.  Any other ray is a miss, decided here where the ray is
// loaded and not by how a NaN would fall through the tests.
struct QueryRay {
    V3 o, d;
    bool valid;
};
__device__ __forceinline__ QueryRay load_query_ray(const double2* __restrict__ rays, unsigned i)
{
    const double2 r0 = rays[4 * (size_t)i], r1 = rays[4 * (size_t)i + 1], r2 = rays[4 * (size_t)i + 2],
                  r3 = rays[4 * (size_t)i + 3];
    QueryRay q;
    q.o = v3((float)r0.x, (float)r0.y, (float)r1.x);
    q.d = v3((float)r2.x, (float)r2.y, (float)r3.x);
    const float inf = __builtin_huge_valf();
    const bool finite = (fabsf(q.o.x) < inf) & (fabsf(q.o.y) < inf) & (fabsf(q.o.z) < inf) & (fabsf(q.d.x) < inf) &
                        (fabsf(q.d.y) < inf) & (fabsf(q.d.z) < inf) & (fabs(r1.y) < __builtin_huge_val()) &
                        (fabs(r3.y) < __builtin_huge_val()); // (every compare is false for NaN)
    q.valid = finite & ((q.d.x != 0.0f) | (q.d.y != 0.0f) | (q.d.z != 0.0f));
    return q;
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

// The camera and the launch parameters in the constant address space: uniform reads become
// scalar loads (the kernels never write them).
#ifdef __HIP_DEVICE_COMPILE__
#define RT_AS_CONST __attribute__((address_space(4)))
#else
#define RT_AS_CONST // the host pass only needs the types
#endif
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

// The BVH order's outer group (DevScene::groups_bvh): the world rects and closed boxes left out of
// the tree, tested by the lanes whose query ended, as the brute-force kernels test a group.
template <bool STATS, class GroupP, class RectP, class BoxP>
__device__ __forceinline__ void test_outer(GroupP groups, RectP rects, BoxP boxes, V3 o, V3 d, int prev, Best& b,
                                           unsigned& n_tests)
{
    const V3 id = v3(slab_rcp_lean(d.x), slab_rcp_lean(d.y), slab_rcp_lean(d.z));
    const V3 oi = o * id;
    const GroupRec G = groups[0];
    if (STATS) n_tests += G.n_rect[0] + G.n_rect[1] + G.n_rect[2] + G.n_flat_extra;
    RectP r = rects + __float_as_int(G.lo.w);
    rect_group<0>(r, G.n_rect[0], o, d, id, oi, prev, b);
    r += G.n_rect[0];
    rect_group<1>(r, G.n_rect[1], o, d, id, oi, prev, b);
    r += G.n_rect[1];
    rect_group<2>(r, G.n_rect[2], o, d, id, oi, prev, b);
    for (int j = G.frame_first + G.n_frames; j < G.frame_first + G.n_frames + G.n_boxes; j++) {
        const BoxRec B = boxes[j];
        hit_box<false>(B, o, d, id, oi, prev, b);
    }
}

// One leaf step of the BVH kernels: RT_SPEC_PRIMS primitives of the pending leaf pend, their
// loads issued together.  Every leaf reads the 48-B rows of its records (3 loads per primitive); a
// compact leaf's flags come with its reference (lfl), a generic leaf's from each record's meta row
// (one more 4-B load).  The BVH order holds triangles and spheres only (planes follow it), and both
// arrays carry kTestSpares zero records after the last slot.
template <bool STATS, class TestP, class RowP, class XfP>
__device__ __forceinline__ void test_leaf(TestP tests, RowP rows, XfP xf, int pend, V3 o, V3 d, int prev, Best& b,
                                          unsigned& n_tri, unsigned& n_sph)
{
    int k, kend;
    uint32_t lfl;
    leaf_decode(pend, k, kend, lfl);
    float4 r[RT_SPEC_PRIMS][3];
    uint32_t fl[RT_SPEC_PRIMS];
#pragma unroll
    for (int j = 0; j < RT_SPEC_PRIMS; j++) {
        r[j][0] = rows[3 * (k + j)];
        r[j][1] = rows[3 * (k + j) + 1];
        r[j][2] = rows[3 * (k + j) + 2];
    }
    if (lfl == kLeafGeneric) {
#pragma unroll
        for (int j = 0; j < RT_SPEC_PRIMS; j++) fl[j] = __float_as_uint(tests[k + j].meta.y);
    } else {
#pragma unroll
        for (int j = 0; j < RT_SPEC_PRIMS; j++) fl[j] = lfl;
    }
    // all rows in registers before the kind dispatch: otherwise the compiler sinks row loads into the
    // triangle / sphere branches, one more round trip per step (C4 49.9 -> 48.9 ms, 64-B records)
#pragma unroll
    for (int j = 0; j < RT_SPEC_PRIMS; j++) {
        pin4(r[j][0]);
        pin4(r[j][1]);
        pin4(r[j][2]);
    }
#pragma unroll
    for (int j = 0; j < RT_SPEC_PRIMS; j++) {
        if (j == 0 || k + j < kend) {
            const bool sph = (fl[j] & KIND_MASK) == RT_PRIM_SPHERE;
            if (STATS) {
                if (sph) n_sph++;
                else n_tri++;
            }
            if (sph) hit_sph_rows(r[j][0], r[j][1], fl[j], k + j, k + j, o, d, prev, xf, b);
            else hit_tri_rows(r[j][0], r[j][1], r[j][2], fl[j], k + j, k + j, o, d, prev, b);
        }
    }
}

// Speculative traversal (Aila & Laine 2009), the walk of every BVH kernel.  A lane that reaches a
// leaf keeps it pending and goes on visiting nodes.  Leaf primitives are tested in wave-wide leaf
// steps, taken once `spec` lanes are blocked (a second leaf reached, or no node left) or no lane can
// visit a node, so a step is one kind of work for the whole wave instead of both.  Node culling uses
// the best hit so far (the pending leaf not yet tested): more visits, the same closest hit.  (A lane
// with a pending leaf always runs ahead; having it wait for the leaf step measured C4 44.5 -> 48.95 ms.)
struct Walk {
    bool more; // ref still holds a reference to process (the stack is not exhausted)
    int ref;   // a node index, or ~leaf code
    int sp;
    int pend;  // the pending leaf (leaf_decode), -1 for none
};
// tree: the scene has nodes or a root leaf (without either only the planes remain, and the query
// ends at its first step)
__device__ __forceinline__ void walk_start(Walk& w, int root, bool tree)
{
    w.ref = root;
    w.sp = 0;
    w.pend = -1;
    w.more = tree;
    if (root < 0) { // the root itself is a leaf
        w.pend = ~root;
        w.more = false;
    }
}
struct WalkStep { // (can_node and sp_visit exist only for path_kernel_bvh's STATS counters)
    bool ended;               // this lane's query ended in this step
    bool leaf_step, can_node; // the step's kind (wave-uniform); the lane had a node to visit (for the callers' counters)
    int sp_visit;             // the stack pointer after the lane's visit, before the pop
};
// One step of the whole wave; trav: the lane has a query under way.  fetch(ref) loads the node: a
// Node4Q (WIDTH 4), or a NodeF (WIDTH 2).  ANY: the query wants any hit, and ends with the first one.
template <int STACK, bool ANY, bool STATS = false, int WIDTH = 4, class FetchT, class TestP, class RowP, class XfP>
__device__ __forceinline__ WalkStep walk_step(Walk& w, bool trav, int spec, FetchT fetch, V3 id, V3 oi, const TravStack& stk,
                                              TestP tests, RowP rows, XfP xf, V3 o, V3 d, int prev, Best& b,
                                              unsigned& n_tri, unsigned& n_sph)
{
    WalkStep st;
    st.can_node = trav && w.more && w.ref >= 0;
    const bool blocked = trav && w.pend >= 0 && !st.can_node;
    st.leaf_step = __ballot(st.can_node) == 0 || __popcll(__ballot(blocked)) >= spec; // wave-uniform
    st.ended = false;
    st.sp_visit = w.sp;
    if (trav) {
        if (st.leaf_step) {
            if (w.pend >= 0) { // RT_SPEC_PRIMS primitives of the pending leaf, their loads issued together
                test_leaf<STATS>(tests, rows, xf, w.pend, o, d, prev, b, n_tri, n_sph);
                w.pend = leaf_advance(w.pend, RT_SPEC_PRIMS);
                if (ANY && b.sg >= 0) { // the answer: the rest of the leaf and of the tree is not looked at
                    w.pend = -1;
                    w.more = false;
                }
            }
        } else if (st.can_node) {
            bool pop = true;
            const auto node = fetch(w.ref);
            if constexpr (WIDTH == 2) bvh2_visit<STACK>(node, id, oi, b.t, w.ref, w.sp, stk, pop);
            else if constexpr (ANY) any_visit<STACK>(node, id, oi, b.t, w.ref, w.sp, stk, pop);
            else wide_visit<STACK>(node, id, oi, b.t, w.ref, w.sp, stk, pop);
            st.sp_visit = w.sp;
            if (pop) {
                if (w.sp > 0) w.ref = pop_ref<STACK>(stk, w.sp);
                else w.more = false;
            }
        }
        // a leaf reference becomes the pending leaf once the previous one is tested, and the
        // next reference is popped so that traversal goes on past it
        if (w.more && w.ref < 0 && w.pend < 0) {
            w.pend = ~w.ref;
            if (w.sp > 0) w.ref = pop_ref<STACK>(stk, w.sp);
            else w.more = false;
        }
        // The popped reference is complete here, before the caller's stores at the end of a query.  Left
        // in flight, a register copy of it at the loop's end made the wave wait for those stores as well
        // (s_waitcnt vmcnt(0) after the hit record: rt_query_rays + 3 % at 7.6 M rays).  Seen with AMD clang
        // 22.0.0git (ROCm 7.2.0).  To re-check with another compiler: in query_bvh_kernel's ISA, no
        // s_waitcnt vmcnt(0) between the last global_store_dwordx4 and the loop's branch.
        asm volatile("" : "+v"(w.ref));
        st.ended = !w.more && w.pend < 0;
    }
    return st;
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

#ifndef __HIPCC_RTC__ // the host side and the other kernels (not part of a hiprtc build)
// The wave's pool of ray indices in the ray-list kernels (wave-uniform): one atomicAdd of 256 on
// the grid's counter whenever the lanes without a query outnumber what is left of the last grant.
struct RayPool {
    unsigned next, end;
};
// need: the lane has no query; m = __ballot(need), not 0.  Returns the ray index of a lane in need
// (which may lie past the last ray) and takes the wave's indices out of the pool.
__device__ __forceinline__ unsigned pool_take(RayPool& pool, bool need, unsigned long long m, int lane, unsigned* counter)
{
    const unsigned kk = (unsigned)__popcll(m), avail = pool.end - pool.next;
    unsigned fresh = 0;
    if (kk > avail) {
        if (lane == 0) fresh = atomicAdd(counter, 256u);
        fresh = __builtin_amdgcn_readfirstlane(fresh);
    }
    const unsigned r = (unsigned)__popcll(m & ((1ull << lane) - 1ull));
    const unsigned idx = r < avail ? pool.next + r : fresh + (r - avail);
    if (kk > avail) {
        pool.next = fresh + (kk - avail);
        pool.end = fresh + 256u;
    } else {
        pool.next += kk;
    }
    return need ? idx : 0xFFFFFFFFu;
}

// Trace-only kernel (rt_debug_trace_rays): the wide BVH kernel's speculative traversal over a
// list of logged queries, with no shading phase and no path state, so that each lane takes the
// next ray as soon as its query ends.  It measures the traversal stage of a wavefront split
// (Laine, Karras & Aila 2013) against the megakernel on the same rays.
template <int STACK, int WAVES, bool STATS>
__global__ void __launch_bounds__(256, WAVES) trace_rays_kernel(TraceRaysParams p)
{
    __shared__ int stack_mem[STACK * 256];
    const TravStack stk = make_stack(stack_mem, p.stack_ovf);
    const int lane = threadIdx.x & 63;
    const RT_AS_CONST TestRec* tests = (const RT_AS_CONST TestRec*)p.tests;
    const RT_AS_CONST float4* rows = (const RT_AS_CONST float4*)p.rows;
    const RT_AS_CONST Node4Q* nodes4 = (const RT_AS_CONST Node4Q*)p.nodes4;
    const RT_AS_CONST XformF* xf = (const RT_AS_CONST XformF*)p.xf;
    bool trav = false, exhausted = false;
    Walk w{false, 0, 0, -1};
    int prev = -1;
    unsigned n_tri = 0, n_sph = 0;
    unsigned idx = 0;
    RayPool pool{0, 0};
    V3 o{0, 0, 0}, d{0, 0, 0}, id{0, 0, 0}, oi{0, 0, 0};
    Best b{__builtin_huge_valf(), -1};
    unsigned long long n_node = 0, n_leaf = 0, n_slots = 0;
    while (true) {
        const bool need = !trav && !exhausted;
        const unsigned long long m = __ballot(need);
        if (m) { // lanes without a query take the next rays
            const unsigned take = pool_take(pool, need, m, lane, p.counter);
            if (need) {
                idx = take;
                if (idx >= p.n) {
                    exhausted = true;
                } else {
                    const float4 r0 = p.rays[3 * (size_t)idx], r1 = p.rays[3 * (size_t)idx + 1];
                    o = v3(r0.x, r0.y, r0.z);
                    d = v3(r1.x, r1.y, r1.z);
                    prev = __float_as_int(r0.w);
                    id = v3(slab_rcp(d.x), slab_rcp(d.y), slab_rcp(d.z));
                    oi = o * id;
                    walk_start(w, p.root4, true); // (rt_debug_trace_rays refuses a scene without wide nodes)
                    b = Best{__builtin_huge_valf(), -1};
                    trav = true;
                }
            }
        }
        if (!__any(trav)) break;
        // walk_step's closest-hit body, written out: this kernel measures the traversal loop, and as a call
        // its 8-wave instance (64 VGPRs) held two more values across the loop and spilled o / d (3.59 ->
        // 4.01 ms; 3.68 ms with o / d formed per visit; profiles/shared_walk).  A change to the step is made
        // in both places.
        const bool can_node = trav && w.more && w.ref >= 0;
        const bool blocked = trav && w.pend >= 0 && !can_node;
        const bool leaf_step = __ballot(can_node) == 0 || __popcll(__ballot(blocked)) >= p.spec;
        if (STATS) {
            n_slots += 64;
            if (leaf_step) n_leaf += (trav && w.pend >= 0) ? 1 : 0;
            else n_node += can_node ? 1 : 0;
        }
        if (trav) {
            if (leaf_step) {
                if (w.pend >= 0) {
                    test_leaf<false>(tests, rows, xf, w.pend, o, d, prev, b, n_tri, n_sph);
                    w.pend = leaf_advance(w.pend, RT_SPEC_PRIMS);
                }
            } else if (can_node) {
                bool pop = true;
                const Node4Q q = nodes4[w.ref];
                wide_visit<STACK>(q, id, oi, b.t, w.ref, w.sp, stk, pop);
                if (pop) {
                    if (w.sp > 0) w.ref = pop_ref<STACK>(stk, w.sp);
                    else w.more = false;
                }
            }
            if (w.more && w.ref < 0 && w.pend < 0) {
                w.pend = ~w.ref;
                if (w.sp > 0) w.ref = pop_ref<STACK>(stk, w.sp);
                else w.more = false;
            }
            if (!w.more && w.pend < 0) {
                trav = false;
                if (p.outer)
                    test_outer<false>((const RT_AS_CONST GroupRec*)p.outer, (const RT_AS_CONST RectRec*)p.outer_rects,
                                      (const RT_AS_CONST BoxRec*)p.outer_boxes, o, d, prev, b, n_tri);
                p.hits[idx] = make_float2(b.t, __int_as_float(b.sg));
            }
        }
    }
    if (STATS) {
        for (int off = 32; off > 0; off >>= 1) {
            n_node += __shfl_down(n_node, off);
            n_leaf += __shfl_down(n_leaf, off);
        }
        if (lane == 0) {
            atomicAdd(p.stats + 0, n_node);
            atomicAdd(p.stats + 1, n_leaf);
            atomicAdd(p.stats + 2, n_slots);
        }
    }
}

// ---- rt_query_rays, RT_QUERY_FAST: the closest hit of caller-supplied rays -------------------------
// Scene.RayTrace(ray, null) by the path kernels' own closest-hit code from "no previous hit" (prev
// = -1, Best = none), one rt_hit per ray, loaded by load_query_ray (above, with the path kernels'
// refill, which starts rt_render_rays' samples from the same rows).

__device__ __forceinline__ void store_query_miss(float4* __restrict__ out)
{
    out[0] = make_float4(__int_as_float(-1), 0.0f, 0.0f, 0.0f);
    out[1] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    out[2] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
}

// The Hit of a finished query as rt_hit (kHitRows 16-B rows): the geometric head of shade() -- the hit
// point (an axis-aligned rectangle's on its plane), a rectangle's side recomputed from its normal,
// sphere, ellipsoid and vertex-normal normals with Triangle.GetNormal's NaN-inside quirk, Inside after
// Invert and the normal turned toward the ray -- restated for both record forms: SLOT, the BVH
// order's records (rows a, b, d), else the brute-force orders' with the shading row c.  The same
// operations in the same order as shade(), so the values are the ones rt_trace_paths records.
template <bool SLOT, class VnP, class TestP>
__device__ __forceinline__ void query_hit(uint32_t facts, const PrimF* __restrict__ prims, const XformF* __restrict__ xfs,
                                          VnP vnormals, TestP tests, const Best& b, V3 o, V3 d, float4* __restrict__ out)
{
    if (b.sg < 0) {
        store_query_miss(out);
        return;
    }
    bool gin = (b.sg & 1) != 0;
    const PrimF& P = prims[b.sg >> 1];
    const float4 Pa = P.a, Pb = P.b, Pd = P.d;
    const uint32_t fl = __float_as_uint(Pb.w);
    const int id = __float_as_int(Pa.w);
    const uint32_t kind = fl & KIND_MASK;
    V3 pos = madd(d, b.t, o);
    const bool sph = (facts & FACT_SPHERE) && kind == RT_PRIM_SPHERE;
    V3 n;
    float nk; // (as shade(): a sphere's normal back to unit length)
    if (SLOT) {
        const uint32_t axis = (fl & F_AXIS_MASK) >> F_AXIS_SHIFT;
        if (axis | (fl & F_FRAME_RECT)) gin = dot(d, xyz(Pd)) > 0.0f;
        pos.x = axis == 1 ? Pa.x : pos.x;
        pos.y = axis == 2 ? Pa.y : pos.y;
        pos.z = axis == 3 ? Pa.z : pos.z;
        n = sph ? (pos - xyz(Pa)) * Pb.y : xyz(Pd);
        nk = sph ? fmaf(-0.5f, dot(n, n), 1.5f) : 1.0f;
    } else {
        const float4 Pc = P.c;
        pos = v3(fmaf(Pc.x, Pa.x - pos.x, pos.x), fmaf(Pc.y, Pa.y - pos.y, pos.y), fmaf(Pc.z, Pa.z - pos.z, pos.z));
        n = madd(pos, Pc.w, xyz(Pd));
        nk = fmaf(-0.5f, dot(n, n), 1.5f); // (no select: row d of a flat kind is unit or zero, see shade())
        if (fl & (F_AXIS_MASK | F_FRAME_RECT)) gin = dot(d, xyz(Pd)) > 0.0f;
    }
    if ((facts & (FACT_XF | FACT_VN)) && (fl & (F_TRANSFORMED | F_HASNORMALS))) {
        if (sph) {
            n = normalize(xf_point(xfs[__float_as_int(Pb.z)].normal, pos));
            nk = 1.0f;
        } else if (facts & FACT_VN) {
            const VnP vn = vnormals + 3 * id;
            const TestRec R = tests[b.sg >> 1];
            const float bu = dot4(R.r0, pos);
            const float bv = dot4(R.r1, pos);
            n = normalize(madd(xyz(vn[2]), bu + bv, madd(xyz(vn[1]), bv, xyz(vn[0]) * bu)));
            nk = 1.0f;
            if (gin) n = v3(__builtin_nanf(""), __builtin_nanf(""), __builtin_nanf(""));
        }
    }
    const V3 nrm = n * (gin ? -nk : nk);
    const bool inside = gin ^ ((fl & F_INVERT) != 0);
    const unsigned long long tb = (unsigned long long)__double_as_longlong((double)b.t); // fp32 widened exactly
    out[0] = make_float4(__int_as_float(id), __int_as_float(inside ? 1 : 0), __uint_as_float((unsigned)tb),
                         __uint_as_float((unsigned)(tb >> 32)));
    out[1] = make_float4(pos.x, pos.y, pos.z, nrm.x);
    out[2] = make_float4(nrm.y, nrm.z, 0.0f, 0.0f);
}

// Brute force (CULL: the grouped order): one ray per lane in a grid-stride loop whose bounds are
// wave-uniform, so the records arrive through scalar loads as in path_body; then the planes.
template <bool CULL>
__global__ void __launch_bounds__(256, CULL ? RT_GROUPED_WAVES : RT_PATH_WAVES) query_brute_kernel(QueryParams p)
{
    const auto tests = (const RT_AS_CONST TestRec*)p.tests;
    const auto rects = (const RT_AS_CONST RectRec*)p.rects;
    const auto frames = (const RT_AS_CONST FrameRec*)p.frames;
    const auto boxes = (const RT_AS_CONST BoxRec*)p.frames;
    const auto groups = (const RT_AS_CONST GroupRec*)p.groups;
    const auto xf = (const RT_AS_CONST XformF*)p.xf;
    const auto vnormals = (const RT_AS_CONST float4*)p.vnormals;
    for (unsigned base = blockIdx.x * 256u; base < p.n; base += gridDim.x * 256u) {
        const unsigned i = base + threadIdx.x;
        if (i >= p.n) continue;
        const QueryRay q = load_query_ray(p.rays, i);
        Best b{__builtin_huge_valf(), -1};
        if (q.valid) {
            unsigned n_flat = 0, n_sph = 0, n_node = 0;
            trace_brute<CULL, false>(p.scene, groups, tests, rects, frames, boxes, xf, q.o, q.d, -1, b, n_flat, n_sph,
                                     n_node);
            test_planes(p.scene, tests, q.o, q.d, -1, b);
        }
        query_hit<false>(p.scene.facts, p.prims, p.xf, vnormals, tests, b, q.o, q.d, p.hits + (size_t)kHitRows * i);
    }
}

// The wide BVH: the speculative walk over rays from the wave's pool, as in trace_rays_kernel, and
// when a query ends what path_kernel_bvh does then: the outer records, the planes that follow the
// BVH order, and the hit.
template <int STACK>
__global__ void __launch_bounds__(256, RT_BVH_WAVES) query_bvh_kernel(QueryParams p)
{
    __shared__ int stack_mem[STACK * 256];
    const TravStack stk = make_stack(stack_mem, p.stack_ovf);
    const int lane = threadIdx.x & 63;
    const RT_AS_CONST TestRec* tests = (const RT_AS_CONST TestRec*)p.tests;
    const RT_AS_CONST float4* rows = (const RT_AS_CONST float4*)p.rows;
    const RT_AS_CONST Node4Q* nodes4 = (const RT_AS_CONST Node4Q*)p.nodes4;
    const RT_AS_CONST XformF* xf = (const RT_AS_CONST XformF*)p.xf;
    const RT_AS_CONST float4* vnormals = (const RT_AS_CONST float4*)p.vnormals;
    const auto fetch = [&](int ref) { return Node4Q(nodes4[ref]); };
    bool trav = false, exhausted = false;
    Walk w{false, 0, 0, -1};
    unsigned n_tri = 0, n_sph = 0;
    unsigned idx = 0;
    RayPool pool{0, 0};
    V3 o{0, 0, 0}, d{0, 0, 0}, id{0, 0, 0}, oi{0, 0, 0};
    Best b{__builtin_huge_valf(), -1};
    while (true) {
        const bool need = !trav && !exhausted;
        const unsigned long long m = __ballot(need);
        if (m) { // lanes without a query take the next rays
            const unsigned take = pool_take(pool, need, m, lane, p.counter);
            if (need) {
                idx = take;
                if (idx >= p.n) {
                    exhausted = true;
                } else {
                    const QueryRay q = load_query_ray(p.rays, idx);
                    if (!q.valid) { // a miss; the lane takes another ray at the next refill
                        store_query_miss(p.hits + (size_t)kHitRows * idx);
                    } else {
                        o = q.o;
                        d = q.d;
                        id = v3(slab_rcp(d.x), slab_rcp(d.y), slab_rcp(d.z));
                        oi = o * id;
                        walk_start(w, p.root4, p.n_nodes4 > 0);
                        b = Best{__builtin_huge_valf(), -1};
                        trav = true;
                    }
                }
            }
        }
        if (!__any(trav)) {
            if (__any(!exhausted)) continue; // only invalid rays this round: refill again
            break;
        }
        if (walk_step<STACK, false>(w, trav, p.spec, fetch, id, oi, stk, tests, rows, xf, o, d, -1, b, n_tri, n_sph).ended) {
            trav = false; // the records outside the tree, then the query's Hit
            if (p.scene.n_groups > 0)
                test_outer<false>((const RT_AS_CONST GroupRec*)p.groups, (const RT_AS_CONST RectRec*)p.rects,
                                  (const RT_AS_CONST BoxRec*)p.frames, o, d, -1, b, n_tri);
            test_planes(p.scene, tests, o, d, -1, b);
            query_hit<true>(p.scene.facts, p.prims, p.xf, vnormals, tests, b, o, d, p.hits + (size_t)kHitRows * idx);
        }
    }
}

// ---- rt_occluded_rays, RT_QUERY_FAST: is anything on the segment [origin, origin + t_max d) ---------
// The per-primitive tests accept a hit only when t < b.t, so the closest-hit code started from
// Best{(float)t_max, -1} is the bounded query and b.sg >= 0 its answer; nothing closer is looked for.
// hit_rect and hit_box compare bit patterns and need b.t >= 0: an empty segment (t_max NaN, <= 0 or
// rounding to 0 in fp32) is decided where t_max is loaded, like an invalid ray.

// The fp32 end of ray i's segment; not above 0 (NaN included): the segment is empty.
__device__ __forceinline__ float load_t_max(const double* __restrict__ t_max, unsigned i)
{
    return t_max ? (float)t_max[i] : __builtin_huge_valf();
}

// Brute force (CULL: the grouped order): query_brute_kernel's loop around trace_brute's any-hit form.
template <bool CULL>
__global__ void __launch_bounds__(256, CULL ? RT_GROUPED_WAVES : RT_PATH_WAVES) occluded_brute_kernel(OccludedParams P)
{
    const QueryParams& p = P.q;
    const auto tests = (const RT_AS_CONST TestRec*)p.tests;
    const auto rects = (const RT_AS_CONST RectRec*)p.rects;
    const auto frames = (const RT_AS_CONST FrameRec*)p.frames;
    const auto boxes = (const RT_AS_CONST BoxRec*)p.frames;
    const auto groups = (const RT_AS_CONST GroupRec*)p.groups;
    const auto xf = (const RT_AS_CONST XformF*)p.xf;
    for (unsigned base = blockIdx.x * 256u; base < p.n; base += gridDim.x * 256u) {
        const unsigned i = base + threadIdx.x;
        if (i >= p.n) continue;
        const QueryRay q = load_query_ray(p.rays, i);
        const float tm = load_t_max(P.t_max, i);
        Best b{tm, -1};
        if (q.valid & (tm > 0.0f)) {
            unsigned n_flat = 0, n_sph = 0, n_node = 0;
            if (P.early) test_planes(p.scene, tests, q.o, q.d, -1, b);
            if (__any(b.sg < 0)) {
                trace_brute<CULL, false, true>(p.scene, groups, tests, rects, frames, boxes, xf, q.o, q.d, -1, b, n_flat,
                                               n_sph, n_node);
                if (!P.early) test_planes(p.scene, tests, q.o, q.d, -1, b);
            }
        }
        P.out[i] = b.sg >= 0 ? 1 : 0;
    }
}

// The wide BVH: query_bvh_kernel's loop around the any-hit walk.  A lane's query ends the moment a leaf
// step gives it a hit, and the lane takes its next ray at the next ballot.  The records outside the tree
// (the outer group and the planes) are tested when the ray is loaded (P.early) or when the tree gave
// no hit.  A visit pushes at most (children - 1) entries per level, as wide_visit does, so the host's
// bound on the stack depth holds for any order of descent.
template <int STACK>
__global__ void __launch_bounds__(256, RT_BVH_WAVES) occluded_bvh_kernel(OccludedParams P)
{
    __shared__ int stack_mem[STACK * 256];
    const QueryParams& p = P.q;
    const TravStack stk = make_stack(stack_mem, p.stack_ovf);
    const int lane = threadIdx.x & 63;
    const RT_AS_CONST TestRec* tests = (const RT_AS_CONST TestRec*)p.tests;
    const RT_AS_CONST float4* rows = (const RT_AS_CONST float4*)p.rows;
    const RT_AS_CONST Node4Q* nodes4 = (const RT_AS_CONST Node4Q*)p.nodes4;
    const RT_AS_CONST XformF* xf = (const RT_AS_CONST XformF*)p.xf;
    const auto fetch = [&](int ref) { return Node4Q(nodes4[ref]); };
    bool trav = false, exhausted = false;
    Walk w{false, 0, 0, -1};
    unsigned n_tri = 0, n_sph = 0;
    unsigned idx = 0;
    RayPool pool{0, 0};
    V3 o{0, 0, 0}, d{0, 0, 0}, id{0, 0, 0}, oi{0, 0, 0};
    Best b{__builtin_huge_valf(), -1};
    auto outside = [&]() { // the records outside the tree
        if (p.scene.n_groups > 0)
            test_outer<false>((const RT_AS_CONST GroupRec*)p.groups, (const RT_AS_CONST RectRec*)p.rects,
                              (const RT_AS_CONST BoxRec*)p.frames, o, d, -1, b, n_tri);
        test_planes(p.scene, tests, o, d, -1, b);
    };
    while (true) {
        const bool need = !trav && !exhausted;
        const unsigned long long m = __ballot(need);
        if (m) { // lanes without a query take the next rays
            const unsigned take = pool_take(pool, need, m, lane, p.counter);
            if (need) {
                idx = take;
                if (idx >= p.n) {
                    exhausted = true;
                } else {
                    const QueryRay q = load_query_ray(p.rays, idx);
                    const float tm = load_t_max(P.t_max, idx);
                    b = Best{tm, -1};
                    bool open = q.valid & (tm > 0.0f);
                    if (open) {
                        o = q.o;
                        d = q.d;
                        if (P.early) {
                            outside();
                            open = b.sg < 0;
                        }
                    }
                    if (!open) { // answered; the lane takes another ray at the next refill
                        P.out[idx] = b.sg >= 0 ? 1 : 0;
                    } else {
                        id = v3(slab_rcp(d.x), slab_rcp(d.y), slab_rcp(d.z));
                        oi = o * id;
                        walk_start(w, p.root4, p.n_nodes4 > 0);
                        trav = true;
                    }
                }
            }
        }
        if (!__any(trav)) {
            if (__any(!exhausted)) continue; // only answered rays this round: refill again
            break;
        }
        if (walk_step<STACK, true>(w, trav, p.spec, fetch, id, oi, stk, tests, rows, xf, o, d, -1, b, n_tri, n_sph).ended) {
            trav = false;
            if (!P.early && b.sg < 0) outside();
            P.out[idx] = b.sg >= 0 ? 1 : 0;
        }
    }
}

// ---- rt_occluded_surfels: the occluded samples of a surfel, counted ------------------------------------
// The segments of rt_occluded_rays with the ray drawn here: sample k of entry e is surfel_sample's ray
// for the draws of rt_rng_init(seed, stream_base + e, sample_base + k), the ray
// rt_debug_surfel_rays_device reports, and it is held to load_query_ray's rule as that ray would be
// when it came back through rt_occluded_rays.  The counts are integers: how the samples are split among
// lanes, waves and launches changes nothing.

// The entry of list position j; false past the list or for an entry past the records (nothing written).
__device__ __forceinline__ bool surfel_entry(const OccludedSurfelsParams& P, unsigned j, unsigned& e)
{
    if (j >= P.q.n) return false;
    e = P.index ? P.index[j] : j;
    return e < P.n_records;
}

// Sample k's ray of the surfel at rows; false: no query (an invalid surfel, or a ray rt_occluded_rays refuses).
__device__ __forceinline__ bool surfel_segment(const OccludedSurfelsParams& P, const double2* __restrict__ rows, rt_key2 pkey,
                                               unsigned k, V3& o, V3& d)
{
    rt_rng rng = rt_rng_from_pixel_key(pkey, P.sample_base + (unsigned long long)k);
    const float u1 = (float)rt_rng_next24(&rng) * 0x1p-24f;
    const float u2 = (float)rt_rng_next24(&rng) * 0x1p-24f;
    if (!surfel_sample(rows, P.gather_mode, u1, u2, o, d)) return false;
    const float inf = __builtin_huge_valf(); // (the origin is finite: surfel_sample)
    return (fabsf(d.x) < inf) & (fabsf(d.y) < inf) & (fabsf(d.z) < inf) & ((d.x != 0.0f) | (d.y != 0.0f) | (d.z != 0.0f));
}

// Brute force (CULL: the grouped order).  A unit is (64 >> P.log2_lanes) consecutive list positions x
// P.block consecutive samples, one wave per unit in a grid-stride loop.  The 1 << P.log2_lanes lanes that
// share a position keep its surfel and walk the unit's samples side by side, sample k0 + lane % lanes first,
// through occluded_brute_kernel's body: a wave then holds the samples of few neighbouring surfels, as
// a wave of rt_occluded_rays over surfel-major rays does, which is what the grouped order's wave-wide box
// culling lives on.  The sample loop is wave-uniform, so the votes of the any-hit form see the whole wave;
// a lane without an entry, past the block's end, with an invalid surfel or an empty segment is masked.
template <bool CULL>
__global__ void __launch_bounds__(256, CULL ? RT_GROUPED_WAVES : RT_PATH_WAVES) occluded_surfels_brute_kernel(OccludedSurfelsParams P)
{
    const QueryParams& p = P.q;
    const auto tests = (const RT_AS_CONST TestRec*)p.tests;
    const auto rects = (const RT_AS_CONST RectRec*)p.rects;
    const auto frames = (const RT_AS_CONST FrameRec*)p.frames;
    const auto boxes = (const RT_AS_CONST BoxRec*)p.frames;
    const auto groups = (const RT_AS_CONST GroupRec*)p.groups;
    const auto xf = (const RT_AS_CONST XformF*)p.xf;
    const unsigned lane = threadIdx.x & 63u;
    const unsigned wave = __builtin_amdgcn_readfirstlane(blockIdx.x * 4u + (threadIdx.x >> 6));
    const unsigned lanes = 1u << P.log2_lanes, per_wave = 64u >> P.log2_lanes; // lanes per position, positions per wave
    const unsigned mine = lane & (lanes - 1u);
    const unsigned n_units = ((p.n + per_wave - 1u) >> (6 - P.log2_lanes)) * P.blocks; // (the host keeps it in 32 bits)
    for (unsigned u = wave; u < n_units; u += gridDim.x * 4u) {
        const unsigned g = u / P.blocks, sb = u - g * P.blocks;
        const unsigned k0 = sb * P.block, k1 = min(P.spp, k0 + P.block);
        unsigned e = 0;
        const bool listed = surfel_entry(P, g * per_wave + (lane >> P.log2_lanes), e);
        if (!listed) e = 0; // (masked by the empty segment; its loads stay inside the records)
        const double2* const rows = p.rays + 4 * (size_t)e;
        const float tm = listed ? load_t_max(P.t_max, e) : 0.0f;
        const rt_key2 pkey = rt_rng_pixel_key(P.seed_key, P.stream_base + (unsigned long long)e);
        unsigned count = 0;
        for (unsigned k = k0; k < k1; k += lanes) {
            V3 o, d;
            Best b{tm, -1};
            if ((tm > 0.0f) && (k + mine < k1) && surfel_segment(P, rows, pkey, k + mine, o, d)) {
                unsigned n_flat = 0, n_sph = 0, n_node = 0;
                if (P.early) test_planes(p.scene, tests, o, d, -1, b);
                if (__any(b.sg < 0)) {
                    trace_brute<CULL, false, true>(p.scene, groups, tests, rects, frames, boxes, xf, o, d, -1, b, n_flat, n_sph,
                                                   n_node);
                    if (!P.early) test_planes(p.scene, tests, o, d, -1, b);
                }
            }
            count += b.sg >= 0 ? 1u : 0u;
        }
        for (unsigned off = 1; off < lanes; off <<= 1) count += (unsigned)__shfl_xor((int)count, (int)off); // the position's lanes
        if (!listed || mine != 0) continue;
        if (P.blocks == 1) { // the position's lanes own its entry for the whole launch
            P.occluded[e] += count;
        } else if (count) {
            atomicAdd(P.occluded + e, count);
        }
        if (P.samples && sb == 0) P.samples[e] += P.spp; // (one unit per entry has the first block)
    }
}

// The wide BVH: occluded_bvh_kernel's loop with the pool dealing (list position, sample) units, unit =
// position * spp + sample, so a wave's consecutive units are consecutive samples of one surfel and then
// the next surfel's: its origins stay together.  A lane that takes a unit builds the ray and walks as
// that kernel does.  The lanes whose queries ended occluded in one iteration add to the counts once per
// entry among them (a ballot of the lanes with the leader's entry, and its population count).
template <int STACK>
__global__ void __launch_bounds__(256, RT_BVH_WAVES) occluded_surfels_bvh_kernel(OccludedSurfelsParams P)
{
    __shared__ int stack_mem[STACK * 256];
    const QueryParams& p = P.q;
    const TravStack stk = make_stack(stack_mem, p.stack_ovf);
    const int lane = threadIdx.x & 63;
    const RT_AS_CONST TestRec* tests = (const RT_AS_CONST TestRec*)p.tests;
    const RT_AS_CONST float4* rows = (const RT_AS_CONST float4*)p.rows;
    const RT_AS_CONST Node4Q* nodes4 = (const RT_AS_CONST Node4Q*)p.nodes4;
    const RT_AS_CONST XformF* xf = (const RT_AS_CONST XformF*)p.xf;
    const auto fetch = [&](int ref) { return Node4Q(nodes4[ref]); };
    const unsigned n_units = p.n * P.spp; // (the host keeps it at or below 2^30)
    bool trav = false, exhausted = false;
    Walk w{false, 0, 0, -1};
    unsigned n_tri = 0, n_sph = 0;
    unsigned ent = 0;
    RayPool pool{0, 0};
    V3 o{0, 0, 0}, d{0, 0, 0}, id{0, 0, 0}, oi{0, 0, 0};
    Best b{__builtin_huge_valf(), -1};
    auto outside = [&]() { // the records outside the tree
        if (p.scene.n_groups > 0)
            test_outer<false>((const RT_AS_CONST GroupRec*)p.groups, (const RT_AS_CONST RectRec*)p.rects,
                              (const RT_AS_CONST BoxRec*)p.frames, o, d, -1, b, n_tri);
        test_planes(p.scene, tests, o, d, -1, b);
    };
    auto add_counts = [&](bool hit) { // every lane of the wave arrives
        unsigned long long left = __ballot(hit);
        while (left) {
            const int leader = __builtin_ctzll(left);
            const unsigned e0 = (unsigned)__builtin_amdgcn_readlane((int)ent, leader);
            const unsigned long long same = __ballot(hit && ent == e0);
            if (lane == leader) atomicAdd(P.occluded + e0, (unsigned)__popcll(same));
            left &= ~same;
        }
    };
    while (true) {
        const bool need = !trav && !exhausted;
        const unsigned long long m = __ballot(need);
        // lanes without a query take the next units, once there are P.refill of them (or no lane walks): a
        // unit's ray is drawn here, and that arithmetic is worth a fuller wave than a ray's four loads are
        if (m && ((unsigned)__popcll(m) >= P.refill || !__any(trav))) {
            const unsigned take = pool_take(pool, need, m, lane, p.counter);
            bool hit = false;
            if (need) {
                if (take >= n_units) {
                    exhausted = true;
                } else {
                    const unsigned j = take / P.spp, k = take - j * P.spp;
                    unsigned e = 0;
                    if (surfel_entry(P, j, e)) {
                        ent = e;
                        if (P.samples && k == 0) P.samples[e] += P.spp; // (one unit per entry has the first sample)
                        const float tm = load_t_max(P.t_max, e);
                        b = Best{tm, -1};
                        bool open = (tm > 0.0f) && surfel_segment(P, p.rays + 4 * (size_t)e,
                                                                  rt_rng_pixel_key(P.seed_key, P.stream_base + (unsigned long long)e), k, o, d);
                        if (open && P.early) {
                            outside();
                            open = b.sg < 0;
                        }
                        if (!open) { // answered; the lane takes another unit at the next refill
                            hit = b.sg >= 0;
                        } else {
                            id = v3(slab_rcp(d.x), slab_rcp(d.y), slab_rcp(d.z));
                            oi = o * id;
                            walk_start(w, p.root4, p.n_nodes4 > 0);
                            trav = true;
                        }
                    }
                }
            }
            add_counts(hit);
        }
        if (!__any(trav)) {
            if (__any(!exhausted)) continue; // only answered units this round: refill again
            break;
        }
        bool hit = false;
        if (walk_step<STACK, true>(w, trav, p.spec, fetch, id, oi, stk, tests, rows, xf, o, d, -1, b, n_tri, n_sph).ended) {
            trav = false;
            if (!P.early && b.sg < 0) outside();
            hit = b.sg >= 0;
        }
        add_counts(hit);
    }
}

// plane: element stride between the R, G and B planes of sum (>= w*h; a gather slot may be taller
// than the band set written into it)
__global__ void accumulate_kernel(PathParams p, double* sum, uint32_t* samples, uint32_t* misses, size_t plane)
{
    const int x = blockIdx.x * 16 + (threadIdx.x & 15);
    const int y = blockIdx.y * 16 + (threadIdx.x >> 4);
    if (x >= p.w || y >= p.h) return;
    size_t blk = (size_t)((y >> 3) * p.blocks_x + (x >> 3));
    const int q = (y & 7) * 8 + (x & 7);
    const size_t i = (size_t)y * p.w + x;
    if (p.cull) { // a launch over the live blocks: a dead block's pixels are spp primary misses, their sums stay
        const int live = (int)p.cull[kCullTable + (p.n_pad >> 6) + blk];
        if (live < 0) {
            misses[i] += (uint32_t)p.spp;
            return;
        }
        blk = (size_t)live;
    }
    double r = sum[i], g = sum[plane + i], bl = sum[2 * plane + i];
    uint32_t ns = 0, nm = 0;
    const int used = (p.spp + p.chunk - 1) / p.chunk; // chunks past spp hold no partial
    for (int c = 0; c < used; c++) {
        const float4 v = p.partial[(((blk << p.log2_chunks) + c) << 6) + q];
        r += v.x;
        g += v.y;
        bl += v.z;
        const uint32_t k = __float_as_uint(v.w);
        ns += k & 0xFFFFu;
        nm += k >> 16;
    }
    sum[i] = r;
    sum[plane + i] = g;
    sum[2 * plane + i] = bl;
    samples[i] += ns;
    misses[i] += nm;
}

// rt_render_rays: the same fold per ray (ray i's partials are pixel i & 63 of block i >> 6), in chunk
// order.  recs null: added to the planar accumulators (n each, planes n apart); else written, from
// zero, as one TileRec per ray for the host entry's download.
__global__ void accumulate_rays_kernel(PathParams p, double* sum, uint32_t* samples, uint32_t* misses, TileRec* recs)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t n = p.n_rays;
    if (i >= n) return;
    double r = 0.0, g = 0.0, bl = 0.0;
    if (!recs) {
        r = sum[i];
        g = sum[n + i];
        bl = sum[2 * n + i];
    }
    uint32_t ns = 0, nm = 0;
    const int used = (p.spp + p.chunk - 1) / p.chunk;
    for (int c = 0; c < used; c++) {
        const float4 v = p.partial[((((i >> 6) << p.log2_chunks) + c) << 6) + (i & 63)];
        r += v.x;
        g += v.y;
        bl += v.z;
        const uint32_t k = __float_as_uint(v.w);
        ns += k & 0xFFFFu;
        nm += k >> 16;
    }
    if (recs) {
        TileRec t;
        t.r = r;
        t.g = g;
        t.b = bl;
        t.samples = ns;
        t.misses = nm;
        recs[i] = t;
    } else {
        sum[i] = r;
        sum[n + i] = g;
        sum[2 * n + i] = bl;
        samples[i] += ns;
        misses[i] += nm;
    }
}

// rt_render_pixels: the fold per list entry.  Entry i's partials are at accumulate_rays_kernel's
// addresses; they go, in chunk order, into the frame accumulators at the entry's pixel a = pix (row-major
// y * W + x is the list's own index), exactly as accumulate_kernel adds a window's: r = sum[a], then
// r += v.x per chunk.  With q: per used chunk j of t_j = samples + misses > 0 finished samples,
// Y_j = 0.299 r + 0.587 g + 0.114 b of the chunk's fp32 sums (DoubleColor.GetLuminance, left to
// right, every operation rounded on its own), q += Y_j Y_j / t_j and batches += 1.  recs: the same
// from zero as one PixelRec per entry (the host entry's download), zero for a skipped entry.
// (fold_entry: entry i's partials into the accumulators at a; rt_render_list's fold below is the same.)
__device__ __forceinline__ void fold_entry(const PathParams& p, size_t i, size_t a, bool inside, double* sum,
                                           uint32_t* samples, uint32_t* misses, double* q, uint32_t* batches, size_t plane,
                                           PixelRec* recs)
{
    if (!inside && !recs) return;
    double r = 0.0, g = 0.0, bl = 0.0, qs = 0.0;
    if (!recs) {
        r = sum[a];
        g = sum[plane + a];
        bl = sum[2 * plane + a];
    }
    uint32_t ns = 0, nm = 0, nb = 0;
    const int used = inside ? (p.spp + p.chunk - 1) / p.chunk : 0;
    for (int c = 0; c < used; c++) {
        const float4 v = p.partial[((((i >> 6) << p.log2_chunks) + c) << 6) + (i & 63)];
        r += v.x;
        g += v.y;
        bl += v.z;
        const uint32_t k = __float_as_uint(v.w);
        ns += k & 0xFFFFu;
        nm += k >> 16;
        const uint32_t t = (k & 0xFFFFu) + (k >> 16);
        if ((q || recs) && t > 0) {
            const double y = __dadd_rn(__dadd_rn(__dmul_rn(0.299, (double)v.x), __dmul_rn(0.587, (double)v.y)),
                                       __dmul_rn(0.114, (double)v.z));
            qs = __dadd_rn(qs, __ddiv_rn(__dmul_rn(y, y), (double)t));
            nb++;
        }
    }
    if (recs) {
        PixelRec t;
        t.r = r;
        t.g = g;
        t.b = bl;
        t.q = qs;
        t.samples = ns;
        t.misses = nm;
        t.batches = nb;
        t.pad = 0;
        recs[i] = t;
    } else {
        sum[a] = r;
        sum[plane + a] = g;
        sum[2 * plane + a] = bl;
        samples[a] += ns;
        misses[a] += nm;
        if (q) {
            q[a] = __dadd_rn(q[a], qs);
            batches[a] += nb;
        }
    }
}

__global__ void accumulate_pixels_kernel(PathParams p, double* sum, uint32_t* samples, uint32_t* misses, double* q,
                                         uint32_t* batches, size_t plane, PixelRec* recs)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)p.n_rays) return;
    const size_t a = p.pixel_list[i];
    fold_entry(p, i, a, a < (size_t)p.n_frame_px, sum, samples, misses, q, batches, plane, recs);
}

// rt_render_list: accumulate_pixels_kernel for a RAYS, BEAMS or SURFELS launch.  List position i's partials
// go into the per-entry accumulators at e = index[i] (i itself without a list, where the sums are
// accumulate_rays_kernel's: r = sum[e], then r += v.x per chunk), an entry at or past n_records is
// skipped; recs: one PixelRec per list position, from zero.
__global__ void accumulate_list_kernel(PathParams p, const uint32_t* index, size_t n_records, double* sum, uint32_t* samples,
                                       uint32_t* misses, double* q, uint32_t* batches, size_t plane, PixelRec* recs)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)p.n_rays) return;
    const size_t e = index ? (size_t)index[i] : i;
    fold_entry(p, i, e, e < n_records, sum, samples, misses, q, batches, plane, recs);
}

// rt_render_probes: the fold of a SURFELS launch in RT_GATHER_SPHERE with one sample per work item
// (make_params_probes), one thread per probe as accumulate_rays_kernel, so that a wave's loads of chunk k
// are 64 consecutive float4.  Row k of probe i is sample k's fp32 colour and its hit or miss; the sample's
// direction is drawn again as the launch drew it (refill: the stream's first two draws through
// surfel_sample) and weighs the colour, or for a primary miss the count, by the nine basis functions of
// rt_sh.h: fp64, product and sum each rounded on its own, in sample order from what the accumulators hold.
// recs null: sh, samples and misses of the probe; else recs[i], which came up with the caller's sums and
// zero counts and goes down to the host entry.  The 36 sums stay in registers; no LDS, no atomics.
// (fold_probe: list position i's partials into the accumulators of entry e; the two kernels below.)
// LIST (rt_render_probe_list): the record, the stream's key and the accumulators are entry e's, the partials
// list position i's.  MOM: the entry's rt_probe_moments (rt_probe_error.h) as eight more sums in registers.
template <bool LIST, bool MOM>
__device__ __forceinline__ void fold_probe(const PathParams& p, size_t i, size_t e, rt_probe_sh* sh, uint32_t* samples,
                                           uint32_t* misses, ProbeRec* recs, rt_probe_moments* mom)
{
    double* const acc = !LIST && recs ? &recs[e].sh.c[0][0] : &sh[e].c[0][0];
    double c[kShCoeffs][4];
#pragma unroll
    for (int l = 0; l < kShCoeffs; l++)
#pragma unroll
        for (int j = 0; j < 4; j++) c[l][j] = acc[4 * l + j];
    [[maybe_unused]] double m0[kProbeMomentRows], m1[kProbeMomentRows];
    if constexpr (MOM) {
#pragma unroll
        for (int l = 0; l < kProbeMomentRows; l++) {
            m0[l] = mom[e].m[l][0];
            m1[l] = mom[e].m[l][1];
        }
    }
    uint32_t ns = 0, nm = 0;
    const double2* const rows = p.ray_list + 4 * e;
    const rt_key2 pkey = rt_rng_pixel_key(p.seed_key, p.stream_base + (unsigned long long)e);
    const float4* const row = p.partial + ((((i >> 6) << p.log2_chunks) << 6) + (i & 63));
    for (int k = 0; k < p.spp; k++) { // (chunk == 1: chunk k is sample k)
        const float4 v = row[(size_t)k << 6];
        const uint32_t w = __float_as_uint(v.w);
        rt_rng rng = rt_rng_from_pixel_key(pkey, p.sample_base + (unsigned long long)k);
        const float u1 = (float)rt_rng_next24(&rng) * 0x1p-24f;
        const float u2 = (float)rt_rng_next24(&rng) * 0x1p-24f;
        V3 o, d;
        if (!surfel_sample(rows, RT_GATHER_SPHERE, u1, u2, o, d)) { // an invalid probe: a miss in no direction
            nm++;
            continue;
        }
        double Y[kShCoeffs];
        sh_basis((double)d.x, (double)d.y, (double)d.z, Y);
        if (w >> 16) {
            nm++;
#pragma unroll
            for (int l = 0; l < kShCoeffs; l++) c[l][3] = __dadd_rn(c[l][3], Y[l]);
            if constexpr (MOM) probe_moments_miss(m1, Y);
        } else if (w & 0xFFFFu) {
            ns++;
            const double r = (double)v.x, g = (double)v.y, b = (double)v.z;
#pragma unroll
            for (int l = 0; l < kShCoeffs; l++) {
                c[l][0] = __dadd_rn(c[l][0], __dmul_rn(r, Y[l]));
                c[l][1] = __dadd_rn(c[l][1], __dmul_rn(g, Y[l]));
                c[l][2] = __dadd_rn(c[l][2], __dmul_rn(b, Y[l]));
            }
            if constexpr (MOM) probe_moments_hit(m0, v.x, v.y, v.z, Y);
        }
    }
#pragma unroll
    for (int l = 0; l < kShCoeffs; l++)
#pragma unroll
        for (int j = 0; j < 4; j++) acc[4 * l + j] = c[l][j];
    if constexpr (MOM) {
#pragma unroll
        for (int l = 0; l < kProbeMomentRows; l++) {
            mom[e].m[l][0] = m0[l];
            mom[e].m[l][1] = m1[l];
        }
    }
    if (!LIST && recs) {
        recs[e].samples += ns;
        recs[e].misses += nm;
    } else {
        samples[e] += ns;
        misses[e] += nm;
    }
}

__global__ void __launch_bounds__(256) accumulate_probes_kernel(PathParams p, rt_probe_sh* sh, uint32_t* samples,
                                                                uint32_t* misses, ProbeRec* recs)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)p.n_rays) return;
    fold_probe<false, false>(p, i, i, sh, samples, misses, recs, nullptr);
}

// rt_render_probe_list: the same fold for a launch with an index list (run_rays, records not gathered): list
// position i's rows are samples of entry e = index[i] (null: i), whose record, stream and accumulators they
// go with; an entry at or past n_records opened no item and is skipped.  mom (MOM): the entry's moments.
template <bool MOM>
__global__ void __launch_bounds__(256) accumulate_probe_list_kernel(PathParams p, const uint32_t* index, size_t n_records,
                                                                    rt_probe_sh* sh, uint32_t* samples, uint32_t* misses,
                                                                    rt_probe_moments* mom)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)p.n_rays) return;
    const size_t e = index ? (size_t)index[i] : i;
    if (e >= n_records) return;
    fold_probe<true, MOM>(p, i, e, sh, samples, misses, nullptr, mom);
}

// SampleSet.GetOutput / GetColorCode (SampleSet.cs:50-113) per pixel of planar accumulators.
__device__ __forceinline__ uint32_t color_code(double r, double g, double b, double a)
{
    auto q = [](double v) { // Util.Clamp to [0, 1], then (int)(v * 255)
        v = v > 0.0 ? v : 0.0;
        v = v < 1.0 ? v : 1.0;
        return (uint32_t)(int32_t)(v * 255);
    };
    return (q(a) << 24) | (q(r) << 16) | (q(g) << 8) | q(b);
}

__global__ void tonemap_kernel(int w, int h, const double* __restrict__ sum, const uint32_t* __restrict__ samples,
                               const uint32_t* __restrict__ misses, double br, double bg, double bb, double back_alpha,
                               double exposure, int32_t* __restrict__ argb)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int n = w * h;
    if (i >= n) return;
    const uint32_t ns = samples[i], nm = misses[i];
    if (ns == 0) {
        argb[i] = (int32_t)color_code(br * exposure, bg * exposure, bb * exposure, back_alpha);
        return;
    }
    const double total = (double)ns + (double)nm;
    const double mult = exposure / ns;
    double r = sum[i] * mult, g = sum[n + i] * mult, b = sum[2 * (size_t)n + i] * mult, a = 1;
    const double bam = nm / total, bk = bam * back_alpha;
    r += (br - r) * bk;
    g += (bg - g) * bk;
    b += (bb - b) * bk;
    a += (back_alpha - a) * bam;
    const double gamma = 1 / 2.2;
    argb[i] = (int32_t)color_code(pow(r, gamma), pow(g, gamma), pow(b, gamma), a);
}

// One pass of Raytracer.Render (1 spp): DoubleColor[w, h] with Placeholder (-1) on a primary miss,
// in the caller's order x * h + y, as fp32 -- a sample's colour is fp32 in the kernel, so the host
// widens it to double exactly, and the PCIe copy is 12 B per pixel instead of 24.
__global__ void colors_1spp_kernel(PathParams p, float* __restrict__ out)
{
    const size_t npix = (size_t)p.w * p.h;
    const size_t o = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (o >= npix) return;
    const int x = (int)(o / (size_t)p.h), y = (int)(o - (size_t)x * p.h);
    int blk = (y >> 3) * p.blocks_x + (x >> 3);
    if (p.cull) blk = (int)p.cull[kCullTable + (p.n_pad >> 6) + blk]; // live number, or -1: a dead block, a miss
    const int q = (blk < 0 ? 0 : blk) * 64 + (y & 7) * 8 + (x & 7); // 1 spp: one chunk
    const float4 v = blk < 0 ? make_float4(0.0f, 0.0f, 0.0f, 0.0f) : p.partial[q];
    const bool miss = (__float_as_uint(v.w) & 0xFFFFu) == 0;
    out[3 * o + 0] = miss ? -1.0f : v.x;
    out[3 * o + 1] = miss ? -1.0f : v.y;
    out[3 * o + 2] = miss ? -1.0f : v.z;
}

// rt_trace_paths: the records and per-sample rows of a launch, which the path kernel wrote row-major
// over the tile (sample (py * w + px) * spp + k), into the caller's order (x * h + y) * spp + k.
// One thread per 16-byte row: rows = kRecRows * (recursion + 1) per sample of `rays`, 1 of `samples`.
__global__ void trace_host_layout_kernel(int w, int h, int spp, int rows, const float4* __restrict__ rays,
                                         const float4* __restrict__ samples, float4* __restrict__ rays_out,
                                         float4* __restrict__ samples_out)
{
    const size_t n = (size_t)w * h * spp;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n * (size_t)(rows + 1)) return;
    const size_t so = i / (size_t)(rows + 1), row = i - so * (size_t)(rows + 1); // the caller's sample, its row
    const size_t pix = so / (size_t)spp, k = so - pix * (size_t)spp;
    const size_t x = pix / (size_t)h, y = pix - x * (size_t)h;
    const size_t si = (y * (size_t)w + x) * (size_t)spp + k;
    if (row < (size_t)rows) rays_out[so * rows + row] = rays[si * rows + row];
    else samples_out[so] = samples[si];
}

// Planar row-major tile accumulators -> the caller's SampleSet order (C# [x, y]: x * h + y), one
// 32-B record per pixel (DoubleColor, samples, misses), so that the host-buffer entry point copies
// one contiguous image in chunks and adds each chunk sequentially as it lands.
__global__ void tile_host_layout_kernel(int w, int h, const double* __restrict__ sum, const uint32_t* __restrict__ ns,
                                        const uint32_t* __restrict__ ms, TileRec* __restrict__ out)
{
    const size_t npix = (size_t)w * h;
    const size_t o = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (o >= npix) return;
    const size_t x = o / (size_t)h, y = o - x * (size_t)h;
    const size_t i = y * (size_t)w + x;
    TileRec r;
    r.r = sum[i];
    r.g = sum[npix + i];
    r.b = sum[2 * npix + i];
    r.samples = ns[i];
    r.misses = ms[i];
    out[o] = r;
}

// ---- compact leaves (rt_internal.h): 48-B rows and homogeneous leaf references --------------
__global__ void rows_kernel(const TestRec* __restrict__ tests, int n, float4* __restrict__ rows)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const TestRec t = tests[i];
    rows[3 * (size_t)i] = t.r0;
    rows[3 * (size_t)i + 1] = t.r1;
    rows[3 * (size_t)i + 2] = t.r2;
}

// A generic leaf whose primitives (at most 4, all of them at slots below 2^23) share their kind
// (triangle or sphere) and test flags becomes a compact leaf; any other reference is returned
// unchanged.  (A leaf reaching past slot 2^23 stays generic: leaf_advance adds to the first-slot
// field, whose carry would run into the flag bits.)
__device__ int compact_ref(int ref, const TestRec* __restrict__ tests)
{
    if (ref >= 0 || ref == RT_NODE4_EMPTY) return ref;
    const int code = ~ref;
    if (code & kLeafCompact) return ref;
    const int first = code >> 3, count = (code & 7) + 1;
    if (count > 4 || first + count > kLeafCompactMaxFirst) return ref;
    uint32_t key = 0;
    for (int j = 0; j < count; j++) {
        const uint32_t fl = __float_as_uint(tests[first + j].meta.y), kind = fl & KIND_MASK;
        if (kind != RT_PRIM_TRIANGLE && kind != RT_PRIM_SPHERE) return ref;
        const uint32_t lf = (kind == RT_PRIM_SPHERE ? 1u : 0u) | ((fl >> 1) & 0xEu) | ((fl >> 2) & 0x10u);
        if (j > 0 && lf != key) return ref;
        key = lf;
    }
    return ~(kLeafCompact | (int)(key << 25) | (first << 2) | (count - 1));
}

__global__ void compact_nodes_kernel(NodeF* __restrict__ n2, int n_n2, Node4Q* __restrict__ n4, int n_n4,
                                     const TestRec* __restrict__ tests)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_n2) {
        NodeF& n = n2[i];
        n.lmin.w = __int_as_float(compact_ref(__float_as_int(n.lmin.w), tests));
        n.rmin.w = __int_as_float(compact_ref(__float_as_int(n.rmin.w), tests));
    }
    if (i < n_n4) {
        Node4Q& q = n4[i];
        q.c.z = __int_as_float(compact_ref(__float_as_int(q.c.z), tests));
        q.c.w = __int_as_float(compact_ref(__float_as_int(q.c.w), tests));
        q.d.x = __int_as_float(compact_ref(__float_as_int(q.d.x), tests));
        q.d.y = __int_as_float(compact_ref(__float_as_int(q.d.y), tests));
    }
}

using PathKernel = void (*)(PathScene, const CameraF*, const PathParams*, const TestRec*, const RectRec*, const FrameRec*, const PrimF*,
                            const NodeF*, const Node4Q*, const GroupRec*, const XformF*, const MatF*, const float4*);

// vn: the scene has vertex-normal triangles (their re-hit test, vn_rehit_test, is fp64 code that
// costs the other scenes' kernels registers, so it is compiled only into separate instances)
template <bool CULL, bool LDS>
PathKernel pick_brute(bool stats, bool vn, ItemSource src)
{
    if (src == ITEMS_PIXELS)
        return vn ? path_kernel<CULL, LDS, false, true, ITEMS_PIXELS> : path_kernel<CULL, LDS, false, false, ITEMS_PIXELS>;
    if (src == ITEMS_RAYS)
        return vn ? path_kernel<CULL, LDS, false, true, ITEMS_RAYS> : path_kernel<CULL, LDS, false, false, ITEMS_RAYS>;
    if (src == ITEMS_BEAMS)
        return vn ? path_kernel<CULL, LDS, false, true, ITEMS_BEAMS> : path_kernel<CULL, LDS, false, false, ITEMS_BEAMS>;
    if (src == ITEMS_SURFELS)
        return vn ? path_kernel<CULL, LDS, false, true, ITEMS_SURFELS> : path_kernel<CULL, LDS, false, false, ITEMS_SURFELS>;
    if (vn) return stats ? path_kernel<CULL, LDS, true, true> : path_kernel<CULL, LDS, false, true>;
    return stats ? path_kernel<CULL, LDS, true, false> : path_kernel<CULL, LDS, false, false>;
}
template <int WIDTH, int STACK, bool LDS>
PathKernel pick_bvh(bool stats, bool vn, ItemSource src)
{
    if (src == ITEMS_PIXELS) { // (the wide kernel only, as for the rays)
        if constexpr (WIDTH == 4)
            return vn ? path_kernel_bvh<WIDTH, STACK, LDS, false, true, ITEMS_PIXELS>
                      : path_kernel_bvh<WIDTH, STACK, LDS, false, false, ITEMS_PIXELS>;
        return nullptr;
    }
    if (src == ITEMS_RAYS) { // (the wide kernel only; rt_render_rays refuses a BVH2 scene before it gets here)
        if constexpr (WIDTH == 4)
            return vn ? path_kernel_bvh<WIDTH, STACK, LDS, false, true, ITEMS_RAYS>
                      : path_kernel_bvh<WIDTH, STACK, LDS, false, false, ITEMS_RAYS>;
        return nullptr;
    }
    if (src == ITEMS_BEAMS) { // (the wide kernel only, as for the rays)
        if constexpr (WIDTH == 4)
            return vn ? path_kernel_bvh<WIDTH, STACK, LDS, false, true, ITEMS_BEAMS>
                      : path_kernel_bvh<WIDTH, STACK, LDS, false, false, ITEMS_BEAMS>;
        return nullptr;
    }
    if (src == ITEMS_SURFELS) {
        if constexpr (WIDTH == 4)
            return vn ? path_kernel_bvh<WIDTH, STACK, LDS, false, true, ITEMS_SURFELS>
                      : path_kernel_bvh<WIDTH, STACK, LDS, false, false, ITEMS_SURFELS>;
        return nullptr;
    }
    if (vn) return stats ? path_kernel_bvh<WIDTH, STACK, LDS, true, true> : path_kernel_bvh<WIDTH, STACK, LDS, false, true>;
    return stats ? path_kernel_bvh<WIDTH, STACK, LDS, true, false> : path_kernel_bvh<WIDTH, STACK, LDS, false, false>;
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

#endif // __HIPCC_RTC__
} // namespace

#ifndef __HIPCC_RTC__
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

// Blocks of 256 threads a CU can hold of a kernel, at least 1 (also when the runtime cannot say).
template <class KernelT>
int blocks_per_cu(KernelT kernel, size_t dyn_lds = 0)
{
    int n = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, reinterpret_cast<const void*>(kernel), 256, dyn_lds) != hipSuccess ||
        n < 1)
        n = 1;
    return n;
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

hipError_t launch_accumulate(const PathParams& p, double* d_sum, uint32_t* d_samples, uint32_t* d_misses, hipStream_t stream,
                             size_t plane)
{
    if (plane == 0) plane = (size_t)p.w * p.h;
    dim3 grid((p.w + 15) / 16, (p.h + 15) / 16);
    hipLaunchKernelGGL(accumulate_kernel, grid, dim3(256), 0, stream, p, d_sum, d_samples, d_misses, plane);
    return hipGetLastError();
}

hipError_t launch_accumulate_rays(const PathParams& p, double* d_sum, uint32_t* d_samples, uint32_t* d_misses,
                                  TileRec* d_recs, hipStream_t stream)
{
    if (p.n_rays == 0) return hipSuccess;
    hipLaunchKernelGGL(accumulate_rays_kernel, dim3((p.n_rays + 255u) / 256u), dim3(256), 0, stream, p, d_sum, d_samples,
                       d_misses, d_recs);
    return hipGetLastError();
}

hipError_t launch_accumulate_pixels(const PathParams& p, double* d_sum, uint32_t* d_samples, uint32_t* d_misses,
                                    double* d_q, uint32_t* d_batches, size_t plane, hipStream_t stream)
{
    if (p.n_rays == 0) return hipSuccess;
    if (plane == 0) plane = (size_t)p.n_frame_px;
    hipLaunchKernelGGL(accumulate_pixels_kernel, dim3((p.n_rays + 255u) / 256u), dim3(256), 0, stream, p, d_sum, d_samples,
                       d_misses, d_q, d_batches, plane, (PixelRec*)nullptr);
    return hipGetLastError();
}

hipError_t launch_accumulate_list(const PathParams& p, const uint32_t* d_index, size_t n_records, double* d_sum,
                                  uint32_t* d_samples, uint32_t* d_misses, double* d_q, uint32_t* d_batches, size_t plane,
                                  PixelRec* d_recs, hipStream_t stream)
{
    if (p.n_rays == 0) return hipSuccess;
    if (plane == 0) plane = n_records;
    hipLaunchKernelGGL(accumulate_list_kernel, dim3((p.n_rays + 255u) / 256u), dim3(256), 0, stream, p, d_index, n_records,
                       d_sum, d_samples, d_misses, d_q, d_batches, plane, d_recs);
    return hipGetLastError();
}

hipError_t launch_accumulate_probes(const PathParams& p, rt_probe_sh* d_sh, uint32_t* d_samples, uint32_t* d_misses,
                                    ProbeRec* d_recs, hipStream_t stream)
{
    if (p.n_rays == 0) return hipSuccess;
    hipLaunchKernelGGL(accumulate_probes_kernel, dim3((p.n_rays + 255u) / 256u), dim3(256), 0, stream, p, d_sh, d_samples,
                       d_misses, d_recs);
    return hipGetLastError();
}

hipError_t launch_accumulate_probe_list(const PathParams& p, const uint32_t* d_index, size_t n_records, rt_probe_sh* d_sh,
                                        uint32_t* d_samples, uint32_t* d_misses, rt_probe_moments* d_moments,
                                        hipStream_t stream)
{
    if (p.n_rays == 0) return hipSuccess;
    const dim3 grid((p.n_rays + 255u) / 256u);
    if (d_moments)
        hipLaunchKernelGGL(accumulate_probe_list_kernel<true>, grid, dim3(256), 0, stream, p, d_index, n_records, d_sh,
                           d_samples, d_misses, d_moments);
    else
        hipLaunchKernelGGL(accumulate_probe_list_kernel<false>, grid, dim3(256), 0, stream, p, d_index, n_records, d_sh,
                           d_samples, d_misses, d_moments);
    return hipGetLastError();
}

hipError_t launch_accumulate_pixels_recs(const PathParams& p, PixelRec* d_recs, hipStream_t stream)
{
    if (p.n_rays == 0) return hipSuccess;
    hipLaunchKernelGGL(accumulate_pixels_kernel, dim3((p.n_rays + 255u) / 256u), dim3(256), 0, stream, p, (double*)nullptr,
                       (uint32_t*)nullptr, (uint32_t*)nullptr, (double*)nullptr, (uint32_t*)nullptr, (size_t)0, d_recs);
    return hipGetLastError();
}

hipError_t launch_tonemap(int w, int h, const double* d_sum, const uint32_t* d_samples, const uint32_t* d_misses,
                          rt_color back, double back_alpha, double exposure, int32_t* d_argb, hipStream_t stream)
{
    const int n = w * h;
    hipLaunchKernelGGL(tonemap_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, w, h, d_sum, d_samples, d_misses,
                       back.r, back.g, back.b, back_alpha, exposure, d_argb);
    return hipGetLastError();
}

hipError_t launch_tile_host_layout(int w, int h, const double* d_sum, const uint32_t* d_samples,
                                  const uint32_t* d_misses, TileRec* d_out, hipStream_t stream)
{
    const size_t npix = (size_t)w * h;
    if (npix == 0) return hipSuccess;
    hipLaunchKernelGGL(tile_host_layout_kernel, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, stream, w, h, d_sum,
                       d_samples, d_misses, d_out);
    return hipGetLastError();
}

hipError_t launch_trace_host_layout(int w, int h, int spp, int recursion, const float4* d_rays, const float4* d_samples,
                                    float4* d_rays_out, float4* d_samples_out, hipStream_t stream)
{
    const int rows = kRecRows * (recursion + 1);
    const size_t n = (size_t)w * h * spp * (size_t)(rows + 1);
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(trace_host_layout_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, w, h, spp, rows,
                       d_rays, d_samples, d_rays_out, d_samples_out);
    return hipGetLastError();
}

using TraceKernel = void (*)(TraceRaysParams);
TraceKernel pick_trace(int waves, bool stats)
{
    if (waves >= 8) return stats ? trace_rays_kernel<16, 8, true> : trace_rays_kernel<16, 8, false>;
    if (waves == 7) return stats ? trace_rays_kernel<16, 7, true> : trace_rays_kernel<16, 7, false>;
    return stats ? trace_rays_kernel<20, 6, true> : trace_rays_kernel<20, 6, false>;
}

int trace_rays_blocks_per_cu(int waves) { return blocks_per_cu(pick_trace(waves, false)); }

hipError_t launch_trace_rays(const TraceRaysParams& p, int waves, int grid_blocks, hipStream_t stream)
{
    hipLaunchKernelGGL(pick_trace(waves, p.stats != nullptr), dim3(grid_blocks), dim3(256), 0, stream, p);
    return hipGetLastError();
}

using QueryKernel = void (*)(QueryParams);
QueryKernel pick_query(int kernel)
{
    if (kernel == 3) return query_bvh_kernel<RT_WIDE_STACK>;
    return kernel == 1 ? query_brute_kernel<true> : query_brute_kernel<false>;
}

int query_blocks_per_cu(int kernel) { return blocks_per_cu(pick_query(kernel)); }

hipError_t launch_query(const QueryParams& p, int kernel, int grid_blocks, hipStream_t stream)
{
    hipLaunchKernelGGL(pick_query(kernel), dim3(grid_blocks), dim3(256), 0, stream, p);
    return hipGetLastError();
}

using OccludedKernel = void (*)(OccludedParams);
OccludedKernel pick_occluded(int kernel)
{
    if (kernel == 3) return occluded_bvh_kernel<RT_WIDE_STACK>;
    return kernel == 1 ? occluded_brute_kernel<true> : occluded_brute_kernel<false>;
}

int occluded_blocks_per_cu(int kernel) { return blocks_per_cu(pick_occluded(kernel)); }

hipError_t launch_occluded(const OccludedParams& p, int kernel, int grid_blocks, hipStream_t stream)
{
    hipLaunchKernelGGL(pick_occluded(kernel), dim3(grid_blocks), dim3(256), 0, stream, p);
    return hipGetLastError();
}

using OccludedSurfelsKernel = void (*)(OccludedSurfelsParams);
OccludedSurfelsKernel pick_occluded_surfels(int kernel)
{
    if (kernel == 3) return occluded_surfels_bvh_kernel<RT_WIDE_STACK>;
    return kernel == 1 ? occluded_surfels_brute_kernel<true> : occluded_surfels_brute_kernel<false>;
}

int occluded_surfels_blocks_per_cu(int kernel) { return blocks_per_cu(pick_occluded_surfels(kernel)); }

hipError_t launch_occluded_surfels(const OccludedSurfelsParams& p, int kernel, int grid_blocks, hipStream_t stream)
{
    hipLaunchKernelGGL(pick_occluded_surfels(kernel), dim3(grid_blocks), dim3(256), 0, stream, p);
    return hipGetLastError();
}

hipError_t compact_leaves(const TestRec* d_tests, int n_records, float4* d_rows, NodeF* d_nodes, int n_nodes,
                          Node4Q* d_nodes4, int n_nodes4, bool rewrite, hipStream_t stream)
{
    if (n_records > 0)
        hipLaunchKernelGGL(rows_kernel, dim3((n_records + 255) / 256), dim3(256), 0, stream, d_tests, n_records, d_rows);
    const int n = std::max(n_nodes, n_nodes4);
    if (rewrite && n > 0)
        hipLaunchKernelGGL(compact_nodes_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, d_nodes, n_nodes, d_nodes4,
                           n_nodes4, d_tests);
    return hipGetLastError();
}

__global__ void pixel_keys_kernel(rt_key2 seed_key, int w, int h, rt_key2* __restrict__ out)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)w * (size_t)h) return;
    out[i] = rt_rng_pixel_key(seed_key, (unsigned long long)i);
}

hipError_t launch_pixel_keys(rt_key2 seed_key, int w, int h, rt_key2* out, hipStream_t stream)
{
    const size_t n = (size_t)w * (size_t)h;
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(pixel_keys_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, seed_key, w, h, out);
    return hipGetLastError();
}

hipError_t launch_colors_1spp(const PathParams& p, float* d_out, hipStream_t stream)
{
    const size_t npix = (size_t)p.w * p.h;
    if (npix == 0) return hipSuccess;
    hipLaunchKernelGGL(colors_1spp_kernel, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, stream, p, d_out);
    return hipGetLastError();
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
