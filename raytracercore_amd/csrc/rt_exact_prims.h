// rt_exact_prims.h -- the exact fp64 primitive tests and the Selection fold, shared by the exact
// device kernels (kernels_exact.hip) and the host twin of the selection pass (api_select.hip).
//
// Primitive.RayTrace (Primitive.cs:46-75) over Triangle.RayTraceAVXFaster (Triangle.cs:77-146),
// Sphere.RayTraceAVX (Sphere.cs:50-155) and Plane.DoRayTrace (Plane.cs:36-66), and
// DebugRaycaster.GetColor's Selection case (DebugRaycaster.cs:174-192) with its two intersectors
// (:27-78).  Every operation keeps the reference's order and FMA use; compile with
// -ffp-contract=off, on the host as on the device, so both give the same bits.
#pragma once
#include "rt_refmath.h"

namespace rtc {

struct HitD {
    int prim;
    double dist;
    bool inside;
};

RT_HDI int tri_trace_d(const PrimD& p, Vec4d o, Vec4d d, HitD* out)
{
    Vec4d off = sub(o, p.a);
    Vec4d s1 = cross_fma(off, p.b);
    Vec4d s2 = cross_fma(d, p.c);
    double uu = hsum(mul(off, s2)), vv = hsum(mul(d, s1)), tt = hsum(mul(p.c, s1)), det = hsum(mul(p.b, s2));
    double inv = 1.0 / det;
    double invz = (inv == inv) ? inv : 0.0;
    double u = uu * invz, v = vv * invz, t = tt * invz;
    bool rej = (u < 0) | (v < 0);
    if (p.flags & F_MIRROR)
        rej |= (u > 1) | (v > 1);
    else
        rej |= ((u + v) > 1);
    rej |= (t < 0);
    if (rej) return 0;
    out[0].dist = t;
    out[0].inside = invz < 0;
    return 1;
}

RT_HDI int sphere_trace_d(const PrimD& p, const XformD* xf, Vec4d o, Vec4d d, HitD* out)
{
    Vec4d oo = o, od = d;
    const bool tr = (p.flags & F_TRANSFORMED) != 0;
    if (tr) {
        oo = mat_vec(xf[p.xf].to_world, o);
        od = normalize_v(mat_vec(xf[p.xf].to_world, d));
    }
    Vec4d off = sub(oo, p.a);
    double b = -2 * dot_v(off, od);
    double c = dot_v(off, off) - p.b.y;
    double radix = sqrt((b * b) - (4 * c));
    double dfar = (b + radix) / 2, dclose = (b - radix) / 2;
    if (tr) {
        Vec4d pfar = mat_vec(xf[p.xf].to_obj, fma4(dfar, od, oo));
        Vec4d pclose = mat_vec(xf[p.xf].to_obj, fma4(dclose, od, oo));
        dfar = dot_v(d, sub(pfar, o));
        dclose = dot_v(d, sub(pclose, o));
    }
    if (!(dfar >= 0)) return 0;
    if (!(dclose >= 0)) {
        out[0] = HitD{0, dfar, true};
        return 1;
    }
    out[0] = HitD{0, dclose, false};
    out[1] = HitD{0, dfar, true};
    return 2;
}

RT_HDI bool nearly_equal_d(double a, double b, double delta) // Util.cs:41-51
{
    const double min_normal = 4.9406564584124654e-324 * 1e7;
    if (delta == 0) return true;
    delta = fabs(delta);
    return delta <= min_normal || delta / net_max(a, b) < 1e-24;
}

RT_HDI int plane_trace_d(const PrimD& p, Vec4d o, Vec4d d, HitD* out)
{
    double ray_dist = dot_s(o, p.a);
    double denom = dot_s(d, p.a);
    const double od = p.b.x;
    if (nearly_equal_d(denom, 0, denom - 0) && nearly_equal_d(od, ray_dist, od - ray_dist)) {
        out[0] = HitD{0, 0.0, true};
        return 1;
    }
    if (denom == 0) return 0;
    double dist = (od - ray_dist) / denom;
    if (dist >= -1e-24) {
        Vec4d hp = add(o, scale(d, dist));
        out[0] = HitD{0, length_s(sub(hp, o)), dot_s(p.a, d) > 0};
        return 1;
    }
    return 0;
}

// Primitive.RayTrace with a null skip hit (primary rays): first hit that survives culling.
RT_HDI bool prim_raytrace_d(const DevScene& s, int pi, Vec4d o, Vec4d d, HitD& h)
{
    const PrimD& p = s.prims_d[pi];
    HitD hits[2];
    int n;
    switch (p.flags & KIND_MASK) {
    case RT_PRIM_TRIANGLE: n = tri_trace_d(p, o, d, hits); break;
    case RT_PRIM_SPHERE: n = sphere_trace_d(p, s.xf_d, o, d, hits); break;
    default: n = plane_trace_d(p, o, d, hits); break;
    }
    for (int i = 0; i < n; i++) {
        bool inside = hits[i].inside;
        if (p.flags & F_INVERT) inside = !inside;
        if (inside && !(p.flags & F_TWOSIDED)) continue;
        h = HitD{pi, hits[i].dist, inside};
        return true;
    }
    return false;
}

// The ray rule of the caller-supplied-ray passes: a non-finite component or a zero direction
// answers nothing.
RT_HDI bool ray_valid_d(Vec4d o, Vec4d d)
{
    const double inf = __builtin_huge_val();
    const bool finite = (fabs(o.x) < inf) & (fabs(o.y) < inf) & (fabs(o.z) < inf) & (fabs(o.w) < inf) & (fabs(d.x) < inf) &
                        (fabs(d.y) < inf) & (fabs(d.z) < inf) & (fabs(d.w) < inf); // false for NaN
    return finite & ((d.x != 0.0) | (d.y != 0.0) | (d.z != 0.0));
}

// DebugRaycaster Selection mode for one ray: the fold of GetColor (DebugRaycaster.cs:174-192) over the
// caller's list, in list order, with `<=` (the later of two equal distances wins, +inf beats "none",
// NaN never wins).  A primitive item is PrimitiveIntersector (Hit.Distance, NaN on a miss; no box is
// tested), a node item BVHIntersector over the node's own box (near when near >= 0, else far; both
// NaN on a miss), SkipVolume nodes included.  The items and the records they name are read through
// the loop index alone, the same for every lane of a wave.  Returns (-1, 0) when nothing won.
RT_HDI rt_selection select_items(const DevScene& s, const rt_select_item* items, int n_items, Vec4d o, Vec4d d)
{
    double dist = __builtin_huge_val();
    int winner = -1;
    for (int k = 0; k < n_items; k++) {
        const rt_select_item it = items[k];
        double cur;
        if (it.kind == RT_SELECT_PRIM) {
            HitD h;
            cur = prim_raytrace_d(s, it.index, o, d, h) ? h.dist : __builtin_nan("");
        } else {
            const RefNode& n = s.ref_nodes[it.index];
            double nr, fr;
            aabb_hit_ref(n.mn, n.mx, o, d, nr, fr);
            cur = nr >= 0 ? nr : fr;
        }
        if (cur <= dist) {
            dist = cur;
            winner = k;
        }
    }
    return rt_selection{winner, 0, winner < 0 ? 0.0 : dist};
}

} // namespace rtc
