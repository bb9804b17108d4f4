// rt_trace.h -- the fp32 closest-hit and any-hit query: the device code every tracing kernel is built
// from.  kernels_path.hip (the path megakernels, and through it every scene-specialised build: the
// header is one of the embedded JIT sources) and kernels_query.hip (the ray-list kernels) include it;
// nothing here is a kernel.  In order: the hit tests, the brute-force query (trace_brute, trace_units),
// the traversal stack and the node visits, the launch-bound defaults, a caller's ray, and the
// speculative walk of the BVH kernels (test_outer, test_leaf, walk_step).
//
// The closest-hit query restates Scene.RayTrace semantics (Scene.cs:65-120, Primitive.cs:46-75)
// in fp32: strict-closest hit, Invert flipping Inside only, one-sided culling, and
// Util.RayHitMatches' self-hit rejection (Util.cs:179-192) restated as: a flat primitive
// is never re-hit by the ray leaving it; a sphere re-hit keeps only the far root when the
// ray heads into it (DESIGN.md §Self-hit rule).
//
// Brute-force traversal walks the primitive records with a wave-uniform index: the records
// come through the scalar data cache (s_load) into SGPRs and every lane tests every
// primitive branch-free.  BVH traversal keeps a per-lane stack in LDS.
//
// A scene-specialised build includes its generated rt_scene_const.h before this header, so that every
// macro it defines is seen by the code below.
#pragma once
#include "../../include/rtcore_rng.h"
#include "rt_kernels.h"
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
#define RT_STACK_OVF 44 // with the 16-entry LDS stacks, 60 entries in all
#ifndef __HIPCC_RTC__   // (the host's constant is no part of a hiprtc build)
static_assert(RT_STACK_OVF == kStackOverflow, "the kernels' overflow depth is the one the host allocates (rt_kernels.h)");
#endif
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

// The constant address space, for the scene's records, the camera and the launch parameters: uniform
// reads become scalar loads (the kernels never write them).
#ifdef __HIP_DEVICE_COMPILE__
#define RT_AS_CONST __attribute__((address_space(4)))
#else
#define RT_AS_CONST // the host pass only needs the types
#endif

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

} // namespace
} // namespace rtc
