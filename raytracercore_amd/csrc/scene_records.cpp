// scene_records.cpp -- the host-built fp32 records of a scene (scene_records.h).  No HIP calls: it
// fills the PODs of rt_internal.h, and links into the host-only checks as well as the library.
#include "scene_records.h"

#include "rt_kernels.h"

#include <algorithm>
#include <array>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <string>
#include <unordered_map>

namespace rtc {

float4 f4(Vec4d v, float w) { return make_float4((float)v.x, (float)v.y, (float)v.z, w); }
float as_f(int v)
{
    float f;
    std::memcpy(&f, &v, 4);
    return f;
}
float as_f(uint32_t v)
{
    float f;
    std::memcpy(&f, &v, 4);
    return f;
}

void make_exact_records(const std::vector<HostPrim>& H, std::vector<PrimD>& pd, std::vector<XformD>& xd)
{
    const int n = (int)H.size();
    pd.resize(n);
    xd.clear();
    for (int i = 0; i < n; i++) {
        const HostPrim& p = H[i];
        PrimD& d = pd[i];
        std::memset(&d, 0, sizeof d);
        d.flags = p.flags;
        d.xf = -1;
        if (p.kind == RT_PRIM_TRIANGLE) {
            d.a = p.v[0];
            d.b = p.e01;
            d.c = p.e02;
            d.d = p.n;
            for (int k = 0; k < 3; k++) d.vn[k] = p.vn[k];
        } else if (p.kind == RT_PRIM_SPHERE) {
            d.a = p.center;
            d.b = v4d(p.radius, p.radius_sqr, 0, 0);
            if (p.flags & F_TRANSFORMED) {
                d.xf = (int)xd.size(); // = xf_index[i]: both sets list the transformed spheres in ID order
                XformD X;
                std::memcpy(X.to_world, p.to_world, sizeof X.to_world);
                std::memcpy(X.to_obj, p.to_obj, sizeof X.to_obj);
                std::memcpy(X.to_normal, p.to_normal, sizeof X.to_normal);
                xd.push_back(X);
            }
        } else {
            d.a = p.pn;
            d.b = v4d(p.pd, 0, 0, 0);
        }
    }
}

namespace {

double luminance(rt_color c) { return 0.299 * c.r + 0.587 * c.g + 0.114 * c.b; } // DoubleColor.cs:76-79
uint32_t p_flags_with_axis(uint32_t flags, int axis) { return flags | ((uint32_t)(axis + 1) << F_AXIS_SHIFT); }
// A slot tested as an axis-aligned rectangle on plane `axis`: its flags name the axis, and its
// shading row c (brute-force kernels) the one-hot axis whose hit coordinate is the plane's.
void set_rect_axis(PrimF& f, uint32_t flags, int axis)
{
    const uint32_t fl = p_flags_with_axis(flags, axis);
    std::memcpy(&f.b.w, &fl, 4);
    f.c = make_float4(axis == 0 ? 1.0f : 0.0f, axis == 1 ? 1.0f : 0.0f, axis == 2 ? 1.0f : 0.0f, 0.0f);
}

} // namespace

PrimF make_primf(const std::vector<HostPrim>& H, const std::vector<int>& xf_index, int i)
{
    {
        const HostPrim& p = H[i];
        PrimF f;
        std::memset(&f, 0, sizeof f);
        if (p.kind == RT_PRIM_TRIANGLE) {
            f.a = f4(p.v[0], as_f(i));
            f.b = f4(p.e01, as_f(p.flags));
            f.c = make_float4(0.0f, 0.0f, 0.0f, 0.0f); // the shading row (see set_rect_axis)
            f.d = f4(p.n, 0.0f);
        } else if (p.kind == RT_PRIM_SPHERE) {
            f.a = f4(p.center, as_f(i));
            f.b = make_float4((float)p.radius, (float)(1.0 / p.radius), as_f(xf_index[i]), as_f(p.flags));
            if (!(p.flags & F_TRANSFORMED)) { // brute-force shading: normal = p / r - centre / r
                const double ir = 1.0 / p.radius;
                f.c = make_float4(0.0f, 0.0f, 0.0f, (float)ir);
                f.d = make_float4((float)(-p.center.x * ir), (float)(-p.center.y * ir), (float)(-p.center.z * ir), 0.0f);
            }
        } else {
            f.a = f4(p.pn, as_f(i));
            f.b = make_float4((float)p.pd, 0.0f, 0.0f, as_f(p.flags));
            f.d = f4(p.pn, 0.0f); // face normal where the shading step reads it for every flat kind
        }
        return f;
    }
}
TestRec make_testrec(const std::vector<HostPrim>& H, const std::vector<int>& xf_index, int i)
{
    {
        const HostPrim& p = H[i];
        TestRec t;
        std::memset(&t, 0, sizeof t);
        t.meta = make_float4(as_f(i), as_f(p.flags), 0.0f, 0.0f);
        if (p.kind == RT_PRIM_TRIANGLE) {
            // inverse of A = [e01 e02 n] (columns) with n = e01 x e02: rows (e02 x n, n x e01, n) / |n|^2
            const Vec4d e1 = p.e01, e2 = p.e02, nn = cross_s(p.e01, p.e02);
            const double D = dot_s(e1, cross_s(e2, nn));
            const Vec4d rows[3] = {cross_s(e2, nn), cross_s(nn, e1), nn};
            float4* out[3] = {&t.r0, &t.r1, &t.r2};
            for (int k = 0; k < 3; k++) {
                const Vec4d r = divs(rows[k], D);
                *out[k] = make_float4((float)r.x, (float)r.y, (float)r.z,
                                      (float)(-(r.x * p.v[0].x + r.y * p.v[0].y + r.z * p.v[0].z)));
            }
        } else if (p.kind == RT_PRIM_SPHERE) {
            t.r0 = f4(p.center, (float)p.radius);
            t.r1 = make_float4((float)p.radius_sqr, as_f(xf_index[i]), 0.0f, 0.0f);
        } else {
            t.r0 = f4(p.pn, (float)p.pd);
        }
        return t;
    }
}

// An axis-aligned rectangle: a Mirror parallelogram with both edges on coordinate axes; returns
// the axis of its plane, or -1.
int rect_axis_of(const HostPrim& p)
{
    if (p.kind != RT_PRIM_TRIANGLE || !(p.flags & F_MIRROR) || (p.flags & F_HASNORMALS)) return -1;
    const double e1[3] = {p.e01.x, p.e01.y, p.e01.z}, e2[3] = {p.e02.x, p.e02.y, p.e02.z};
    for (int k = 0; k < 3; k++) {
        const int a = (k + 1) % 3, b = (k + 2) % 3;
        if (e1[k] != 0 || e2[k] != 0) continue;
        const bool e1a = e1[a] != 0 && e1[b] == 0, e1b = e1[b] != 0 && e1[a] == 0;
        const bool e2a = e2[a] != 0 && e2[b] == 0, e2b = e2[b] != 0 && e2[a] == 0;
        if ((e1a && e2b) || (e1b && e2a)) return k;
    }
    return -1;
}

namespace {

// Builds one brute-force slot order (build_order) from groups of primitive IDs: the frame finder
// and its rows, the rectangle geometry, the box finder and its record, the per-group slot emission.
struct OrderBuilder {
    const std::vector<HostPrim>& H;
    const std::vector<int>& xf_index;
    const int n;
    std::vector<int> kind_of; // per primitive: 0-2 world rect on that axis, 3 triangle, 4 sphere, 5 plane
    const bool use_boxes = !getenv("RTCORE_NO_BOXES"); // A/B switch for measurements

    OrderBuilder(const std::vector<HostPrim>& H_, const std::vector<int>& xf_index_)
        : H(H_), xf_index(xf_index_), n((int)H_.size()), kind_of(H_.size())
    {
        for (int i = 0; i < n; i++) {
            const int ax = rect_axis_of(H[i]);
            kind_of[i] = ax >= 0 ? ax : (H[i].kind == RT_PRIM_TRIANGLE ? 3 : H[i].kind == RT_PRIM_SPHERE ? 4 : 5);
        }
    }
    PrimF primf(int i) const { return make_primf(H, xf_index, i); }
    TestRec testrec(int i) const { return make_testrec(H, xf_index, i); }
    RectRec rectrec(int i, int k) const
    {
        const HostPrim& p = H[i];
        const double v0[3] = {p.v[0].x, p.v[0].y, p.v[0].z}, e1[3] = {p.e01.x, p.e01.y, p.e01.z},
                     e2[3] = {p.e02.x, p.e02.y, p.e02.z}, nn[3] = {p.n.x, p.n.y, p.n.z};
        const int a1 = k == 0 ? 1 : 0, a2 = k == 2 ? 1 : 2; // the other two axes in x, y, z order
        RectRec r;
        r.c = (float)v0[k];
        const double c1[4] = {v0[a1], v0[a1] + e1[a1], v0[a1] + e2[a1], v0[a1] + e1[a1] + e2[a1]};
        const double c2[4] = {v0[a2], v0[a2] + e1[a2], v0[a2] + e2[a2], v0[a2] + e1[a2] + e2[a2]};
        // fp32 extents rounded outward, stored as mid-point +- half-width
        const double lo1 = std::min(std::min(c1[0], c1[1]), std::min(c1[2], c1[3]));
        const double hi1 = std::max(std::max(c1[0], c1[1]), std::max(c1[2], c1[3]));
        const double lo2 = std::min(std::min(c2[0], c2[1]), std::min(c2[2], c2[3]));
        const double hi2 = std::max(std::max(c2[0], c2[1]), std::max(c2[2], c2[3]));
        r.m1 = (float)(0.5 * (lo1 + hi1));
        r.h1 = (float)(0.5 * (hi1 - lo1));
        r.m2 = (float)(0.5 * (lo2 + hi2));
        r.h2 = (float)(0.5 * (hi2 - lo2));
        // gin = N[k] * d[k] > 0; one-sided keeps gin == Invert (Primitive.cs:56-61): with
        // q = +-sign(N[k]) that is q * d[k] <= 0 (d[k] = 0 never hits: t is inf or NaN)
        const float ns = nn[k] > 0 ? 1.0f : -1.0f;
        r.cull = (p.flags & F_TWOSIDED) ? 0.0f : ((p.flags & F_INVERT) ? -ns : ns);
        r.id = i;
        r.sg = 0; // set once the slot is known
        return r;
    }
    // Frames: the general Mirror parallelograms of a group whose edges run along the three edge
    // directions of one affine frame (a transformed cube's faces) become rectangles in that frame
    // (FrameRec); a frame is used when it collects at least two faces.
    struct FrameB {
        Vec4d b[3];
        bool b2_set = false; // b[2] came from an edge (else it is the first face's normal)
        Vec4d org;
        std::vector<int> face[3]; // faces on local plane k (edges along the other two axes)
    };
    static bool parallel(const Vec4d& a, const Vec4d& b)
    {
        const Vec4d c = cross_s(a, b);
        const double aa = dot_s(a, a), bb = dot_s(b, b);
        return aa > 0 && bb > 0 && dot_s(c, c) <= 1e-18 * aa * bb;
    }
    // The box and frame finders pair rectangles by search (quadratic in the group's rectangles).
    // They only make the brute-force orders cheaper to test, and a group with more than
    // kFindMax candidates belongs to a scene the BVH kernels render (AUTO takes brute force up to 48
    // primitives), so such a group keeps its rectangles as they are: scene creation stays linear
    // (8,000 single axis-aligned rectangles took 0.7 s, 100,000 would take minutes).
    static constexpr size_t kFindMax = 4096;
    std::vector<FrameB> find_frames(const std::vector<int>& ids) const
    {
        std::vector<FrameB> fr;
        size_t cand = 0;
        for (int i : ids) cand += kind_of[i] == 3 && (H[i].flags & F_MIRROR) && !(H[i].flags & F_HASNORMALS);
        if (cand > kFindMax) return fr;
        for (int i : ids) {
            const HostPrim& p = H[i];
            if (kind_of[i] != 3 || !(p.flags & F_MIRROR) || (p.flags & F_HASNORMALS)) continue;
            bool placed = false;
            for (auto& F : fr) {
                int k1 = -1, k2 = -1;
                for (int k = 0; k < 3; k++) {
                    if (k1 < 0 && parallel(p.e01, F.b[k])) k1 = k;
                    if (k2 < 0 && parallel(p.e02, F.b[k])) k2 = k;
                }
                if (!F.b2_set && F.face[0].empty() && F.face[1].empty()) { // third axis still open
                    if (k1 >= 0 && k1 != 2 && k2 < 0) {
                        F.b[2] = p.e02;
                        k2 = 2;
                    } else if (k2 >= 0 && k2 != 2 && k1 < 0) {
                        F.b[2] = p.e01;
                        k1 = 2;
                    }
                    if (k1 == 2 || k2 == 2) F.b2_set = true;
                }
                if (k1 >= 0 && k2 >= 0 && k1 != k2) {
                    F.face[3 - k1 - k2].push_back(i);
                    placed = true;
                    break;
                }
            }
            if (!placed) {
                FrameB F;
                F.b[0] = p.e01;
                F.b[1] = p.e02;
                F.b[2] = cross_s(p.e01, p.e02);
                F.org = p.v[0];
                F.face[2].push_back(i);
                fr.push_back(F);
            }
        }
        std::vector<FrameB> keep;
        for (auto& F : fr)
            if (F.face[0].size() + F.face[1].size() + F.face[2].size() >= 2) keep.push_back(F);
        return keep;
    }
    // local rows (world -> frame) of F: the inverse of [b0 b1 b2] applied to p - org
    static void frame_rows(const FrameB& F, double M[3][4])
    {
        const Vec4d c0 = cross_s(F.b[1], F.b[2]), c1 = cross_s(F.b[2], F.b[0]), c2 = cross_s(F.b[0], F.b[1]);
        const double det = dot_s(F.b[0], c0);
        const Vec4d rows[3] = {c0, c1, c2};
        for (int k = 0; k < 3; k++) {
            M[k][0] = rows[k].x / det;
            M[k][1] = rows[k].y / det;
            M[k][2] = rows[k].z / det;
            M[k][3] = -(M[k][0] * F.org.x + M[k][1] * F.org.y + M[k][2] * F.org.z);
        }
    }
    // Rectangle geometry in double (world axes, or a frame's local axes): plane coordinate c on
    // axis k, extents on the other two axes in increasing axis order, and sign(N . axis k).
    struct RectG {
        int i, k;
        double c, lo1, hi1, lo2, hi2;
        double ns;
    };
    RectG rect_geom(int i, int k, const double (*M)[4], const FrameB* F) const
    {
        const HostPrim& p = H[i];
        auto loc = [&](double x, double y, double z, int a) {
            if (!M) return a == 0 ? x : a == 1 ? y : z;
            return M[a][0] * x + M[a][1] * y + M[a][2] * z + M[a][3];
        };
        const Vec4d v0 = p.v[0], e1 = p.e01, e2 = p.e02;
        const double cx[4] = {v0.x, v0.x + e1.x, v0.x + e2.x, v0.x + e1.x + e2.x};
        const double cy[4] = {v0.y, v0.y + e1.y, v0.y + e2.y, v0.y + e1.y + e2.y};
        const double cz[4] = {v0.z, v0.z + e1.z, v0.z + e2.z, v0.z + e1.z + e2.z};
        const int a1 = k == 0 ? 1 : 0, a2 = k == 2 ? 1 : 2;
        RectG g{i, k, 0, 1e300, -1e300, 1e300, -1e300, 0};
        for (int j = 0; j < 4; j++) {
            g.c += 0.25 * loc(cx[j], cy[j], cz[j], k);
            const double q1 = loc(cx[j], cy[j], cz[j], a1), q2 = loc(cx[j], cy[j], cz[j], a2);
            g.lo1 = std::min(g.lo1, q1);
            g.hi1 = std::max(g.hi1, q1);
            g.lo2 = std::min(g.lo2, q2);
            g.hi2 = std::max(g.hi2, q2);
        }
        if (!M) g.c = k == 0 ? v0.x : k == 1 ? v0.y : v0.z; // world rects sit exactly on v0's plane
        const double nk = F ? dot_s(p.n, F->b[k]) : (k == 0 ? p.n.x : k == 1 ? p.n.y : p.n.z);
        g.ns = nk > 0 ? 1.0 : -1.0;
        return g;
    }
    RectRec frame_rect(const RectG& g) const
    {
        const HostPrim& p = H[g.i];
        RectRec r;
        r.c = (float)g.c;
        r.m1 = (float)(0.5 * (g.lo1 + g.hi1));
        r.m2 = (float)(0.5 * (g.lo2 + g.hi2));
        // half-widths padded by 2^-21 relative: the fp32 frame rows move the shared edges of
        // neighbouring faces by about an ulp, and a padded edge is met by both faces (closest wins)
        r.h1 = (float)(0.5 * (g.hi1 - g.lo1) + (std::fabs(0.5 * (g.lo1 + g.hi1)) + 0.5 * (g.hi1 - g.lo1)) * 4.76837158203125e-07);
        r.h2 = (float)(0.5 * (g.hi2 - g.lo2) + (std::fabs(0.5 * (g.lo2 + g.hi2)) + 0.5 * (g.hi2 - g.lo2)) * 4.76837158203125e-07);
        // gin = N . d > 0 = sign(N . b_k) * d_local[k] > 0; the culling factor as for world rects
        r.cull = (p.flags & F_TWOSIDED) ? 0.0f : ((p.flags & F_INVERT) ? -(float)g.ns : (float)g.ns);
        r.id = g.i;
        r.sg = 0;
        return r;
    }
    // Boxes: rectangles on the faces of one axis-aligned box -- a pair on some axis with equal
    // extents, and the other faces on the planes and extents of the box they span (within 1e-9
    // relative), at least five of the six, with primitive IDs within 16 of each other.  Face
    // lists are in face order f = 2 axis + side, -1 for a missing face (an open box: the ray may
    // enter through the opening, and its exit face is still the other candidate).
    struct BoxFit {
        std::array<int, 6> f;
        double lo[3], hi[3];
    };
    static std::vector<BoxFit> find_boxes(const std::vector<RectG>& rg, std::vector<char>& used)
    {
        std::vector<BoxFit> boxes;
        auto eq = [](double a, double b, double sc) { return std::fabs(a - b) <= 1e-9 * sc; };
        for (int pa = 0; pa < 3; pa++)
            for (size_t A = 0; A < rg.size(); A++) {
                if (used[A] || rg[A].k != pa) continue;
                for (size_t B = 0; B < rg.size(); B++) {
                    if (B == A || used[B] || used[A] || rg[B].k != pa) continue;
                    const RectG &ga = rg[A], &gb = rg[B];
                    // the pair's axis pa and its two in-plane axes (increasing order)
                    const int q1 = pa == 0 ? 1 : 0, q2 = pa == 2 ? 1 : 2;
                    double lo[3], hi[3];
                    lo[pa] = std::min(ga.c, gb.c);
                    hi[pa] = std::max(ga.c, gb.c);
                    lo[q1] = ga.lo1;
                    hi[q1] = ga.hi1;
                    lo[q2] = ga.lo2;
                    hi[q2] = ga.hi2;
                    double sc = 0;
                    for (int k = 0; k < 3; k++) sc = std::max({sc, std::fabs(lo[k]), std::fabs(hi[k]), hi[k] - lo[k]});
                    bool flat = false;
                    for (int k = 0; k < 3; k++) flat |= !(hi[k] - lo[k] > 1e-9 * sc);
                    if (flat || !eq(gb.lo1, ga.lo1, sc) || !eq(gb.hi1, ga.hi1, sc) || !eq(gb.lo2, ga.lo2, sc) ||
                        !eq(gb.hi2, ga.hi2, sc))
                        continue;
                    BoxFit fit;
                    fit.f.fill(-1);
                    fit.f[2 * pa] = ga.c < gb.c ? (int)A : (int)B;
                    fit.f[2 * pa + 1] = ga.c < gb.c ? (int)B : (int)A;
                    int found = 2;
                    for (int k = 0; k < 3; k++) {
                        fit.lo[k] = lo[k];
                        fit.hi[k] = hi[k];
                        if (k == pa) continue;
                        const int a1 = k == 0 ? 1 : 0, a2 = k == 2 ? 1 : 2;
                        for (int side = 0; side < 2; side++) {
                            const double c = side ? hi[k] : lo[k];
                            for (size_t j = 0; j < rg.size(); j++)
                                if (!used[j] && rg[j].k == k && eq(rg[j].c, c, sc) && eq(rg[j].lo1, lo[a1], sc) &&
                                    eq(rg[j].hi1, hi[a1], sc) && eq(rg[j].lo2, lo[a2], sc) && eq(rg[j].hi2, hi[a2], sc)) {
                                    fit.f[2 * k + side] = (int)j;
                                    found++;
                                    break;
                                }
                        }
                    }
                    if (found < 5) continue;
                    int idmin = 1 << 30, idmax = -1;
                    for (int j : fit.f)
                        if (j >= 0) {
                            idmin = std::min(idmin, rg[j].i);
                            idmax = std::max(idmax, rg[j].i);
                        }
                    if (idmax - idmin >= 16) continue;
                    for (int j : fit.f)
                        if (j >= 0) used[j] = 1;
                    boxes.push_back(fit);
                }
            }
        return boxes;
    }
    BoxRec box_rec(const std::vector<RectG>& rg, const BoxFit& fit, int slot0) const
    {
        BoxRec B;
        std::memset(&B, 0, sizeof B);
        int id0 = 1 << 30;
        for (int j : fit.f)
            if (j >= 0) id0 = std::min(id0, rg[j].i);
        uint32_t perm = 0, keep = 0;
        for (int fi = 0; fi < 6; fi++) {
            if (fit.f[fi] < 0) continue; // missing face: keeps nothing
            const RectG& g = rg[fit.f[fi]];
            const uint32_t fl = H[g.i].flags;
            perm |= (uint32_t)(g.i - id0) << (4 * fi);
            // entering through the lower plane moves along +axis: Inside (N . d > 0) iff sign(N_k) > 0
            const bool gin_entry = (fi & 1) == 0 ? g.ns > 0 : g.ns < 0;
            const bool two = (fl & F_TWOSIDED) != 0, inv = (fl & F_INVERT) != 0;
            if (two || gin_entry == inv) keep |= 1u << fi;
            if (two || !gin_entry == inv) keep |= 1u << (8 + fi);
        }
        // the planes: a face's own (fp32) coordinate where it exists (hit points are snapped to it)
        float pl[6];
        for (int fi = 0; fi < 6; fi++)
            pl[fi] = (float)(fit.f[fi] >= 0 ? rg[fit.f[fi]].c : ((fi & 1) ? fit.hi[fi >> 1] : fit.lo[fi >> 1]));
        B.lo = make_float4(pl[0], pl[2], pl[4], as_f(id0));
        B.hi = make_float4(pl[1], pl[3], pl[5], as_f(perm));
        B.keep = keep;
        B.sg0 = slot0 << 1;
        return B;
    }
    // the six slots of a box, face order; a missing face gets a placeholder slot (never hit)
    static int box_face_prim(const std::vector<RectG>& rg, const BoxFit& fit, int fi)
    {
        const int j = fit.f[fi] >= 0 ? fit.f[fi] : fit.f[fi ^ 1] >= 0 ? fit.f[fi ^ 1] : fit.f[(fi + 2) % 6];
        return rg[j].i;
    }
    // the fp32 box of a group's primitives, padded by 2^-20 relative and rounded outward
    void fbox(const std::vector<int>& ids, float lo[3], float hi[3]) const
    {
        for (int k = 0; k < 3; k++) {
            lo[k] = __builtin_huge_valf();
            hi[k] = -__builtin_huge_valf();
        }
        for (int i : ids) {
            const double l[3] = {H[i].box.mn.x, H[i].box.mn.y, H[i].box.mn.z};
            const double u[3] = {H[i].box.mx.x, H[i].box.mx.y, H[i].box.mx.z};
            for (int k = 0; k < 3; k++) {
                const double pad = (std::fabs(l[k]) + std::fabs(u[k])) * 9.5367431640625e-07 + 1e-30;
                lo[k] = std::min(lo[k], std::nextafter((float)(l[k] - pad), -__builtin_huge_valf()));
                hi[k] = std::max(hi[k], std::nextafter((float)(u[k] + pad), __builtin_huge_valf()));
            }
        }
    }
    // Brute-force slot orders: groups of primitives, each [x-rects | y-rects | z-rects | world
    // box faces | frame rects and frame box faces | triangles | spheres], then the planes.  The
    // flat order is one group of everything; the grouped order cuts the SAH BVH into subtrees of
    // at most kGroupMax primitives.
    // skips[k] > 0: groups[k] lists a subtree's primitives for a super record (its box only) that
    // holds the skips[k] records after it
    BruteOrder build_order(const std::vector<std::vector<int>>& groups, const std::vector<int>& skips) const
    {
        BruteOrder o;
        for (size_t gi = 0; gi < groups.size(); gi++) {
            const auto& g = groups[gi];
            GroupRec G;
            std::memset(&G, 0, sizeof G);
            float lo[3], hi[3];
            fbox(g, lo, hi);
            if (skips[gi] > 0) {
                G.lo = make_float4(lo[0], lo[1], lo[2], as_f((int)o.rects.size()));
                G.hi = make_float4(hi[0], hi[1], hi[2], as_f((int)o.prims.size()));
                G.frame_first = (int)o.frames.size();
                G.skip = skips[gi];
                o.groups.push_back(G);
                continue;
            }
            emit_group(o, G, g, lo, hi);
            o.groups.push_back(G);
        }
        for (int i = 0; i < n; i++) // planes follow
            if (kind_of[i] == 5) push_slot(o, i, primf(i));
        o.tests.push_back(TestRec{}); // spare records: loops may load one past a range
        o.rects.push_back(RectRec{});
        o.frames.push_back(FrameRec{});
        return o;
    }
    void push_slot(BruteOrder& o, int i, PrimF f) const
    {
        o.prims.push_back(f);
        o.tests.push_back(testrec(i));
    }
    // The slots and records of one group (G: its record, filled here; lo, hi: its box).
    void emit_group(BruteOrder& o, GroupRec& G, const std::vector<int>& g, const float lo[3], const float hi[3]) const
    {
        const bool first = o.groups.empty();
        const int rect_first = (int)o.rects.size();
        int cnt[5] = {0, 0, 0, 0, 0};
        // world rects: closed boxes first, the rest as single rects
        std::vector<RectG> wr;
        for (int i : g)
            if (kind_of[i] < 3) wr.push_back(rect_geom(i, kind_of[i], nullptr, nullptr));
        std::vector<char> wused(wr.size(), 0);
        const auto wboxes = use_boxes && wr.size() <= kFindMax ? find_boxes(wr, wused) : std::vector<BoxFit>{};
        for (int kind = 0; kind < 3; kind++)
            for (size_t j = 0; j < wr.size(); j++) {
                if (wused[j] || wr[j].k != kind) continue;
                const int i = wr[j].i;
                PrimF f = primf(i);
                set_rect_axis(f, H[i].flags, kind);
                o.rects.push_back(rectrec(i, kind));
                o.rects.back().sg = (int)o.prims.size() << 1;
                o.nr[kind]++;
                cnt[kind]++;
                push_slot(o, i, f);
            }
        // frames (their rects after the world rects), then the world boxes, in one array
        const std::vector<FrameB> frames = find_frames(g);
        std::vector<char> in_frame(n, 0);
        for (const auto& F : frames)
            for (int k = 0; k < 3; k++)
                for (int i : F.face[k]) in_frame[i] = 1;
        G.frame_first = (int)o.frames.size();
        G.n_frames = (int16_t)frames.size();
        G.n_boxes = (int16_t)wboxes.size();
        // the counts are int16 in the record: more would wrap and drop geometry silently
        if (frames.size() > INT16_MAX || wboxes.size() > INT16_MAX ||
            frames.size() + wboxes.size() > INT16_MAX)
            o.overflow = true;
        std::vector<BoxRec> frame_boxes;
        const int frame_box_first = G.frame_first + (int)frames.size() + (int)wboxes.size();
        for (const auto& F : frames) emit_frame(o, G, F, frame_box_first, frame_boxes);
        for (const auto& f6 : wboxes) {
            BoxRec B = box_rec(wr, f6, (int)o.prims.size());
            for (int fi = 0; fi < 6; fi++) {
                const int i = box_face_prim(wr, f6, fi), kind = fi >> 1;
                PrimF f = primf(i);
                set_rect_axis(f, H[i].flags, kind);
                push_slot(o, i, f);
                G.n_flat_extra += f6.f[fi] >= 0;
                o.nr[kind]++;
            }
            FrameRec R;
            std::memcpy(&R, &B, sizeof R);
            o.frames.push_back(R);
        }
        for (const auto& B : frame_boxes) {
            FrameRec R;
            std::memcpy(&R, &B, sizeof R);
            o.frames.push_back(R);
        }
        const int tri_slot = (int)o.prims.size();
        for (int kind = 3; kind < 5; kind++)
            for (int i : g) {
                if (kind_of[i] != kind || (kind == 3 && in_frame[i])) continue;
                (kind == 3 ? o.nt : o.ns)++;
                cnt[kind]++;
                push_slot(o, i, primf(i));
            }
        G.lo = make_float4(lo[0], lo[1], lo[2], as_f(rect_first));
        G.hi = make_float4(hi[0], hi[1], hi[2], as_f(tri_slot));
        for (int k = 0; k < 3; k++) G.n_rect[k] = cnt[k];
        G.n_tri_sph = cnt[3] | (cnt[4] << 16);
        if (cnt[3] > 0xFFFF || cnt[4] > 0x7FFF) o.overflow = true;
        if (first) {
            o.tris0 = cnt[3];
            o.sphs0 = cnt[4];
        }
    }
    // One frame of a group: its FrameRec, the rects of its faces and at most one closed box of them
    // (appended to frame_boxes, whose records follow the group's frames and world boxes).
    void emit_frame(BruteOrder& o, GroupRec& G, const FrameB& F, int frame_box_first,
                    std::vector<BoxRec>& frame_boxes) const
    {
        double M[3][4];
        frame_rows(F, M);
        FrameRec R;
        std::memset(&R, 0, sizeof R);
        float4* rows[3] = {&R.r0, &R.r1, &R.r2};
        for (int k = 0; k < 3; k++)
            *rows[k] = make_float4((float)M[k][0], (float)M[k][1], (float)M[k][2], (float)M[k][3]);
        std::vector<RectG> fr;
        for (int k = 0; k < 3; k++)
            for (int i : F.face[k]) fr.push_back(rect_geom(i, k, M, &F));
        std::vector<char> fused(fr.size(), 0);
        auto fb = use_boxes ? find_boxes(fr, fused) : std::vector<BoxFit>{};
        for (size_t bi = 1; bi < fb.size(); bi++) // one box per frame; further ones stay rects
            for (int fi = 0; fi < 6; fi++)
                if (fb[bi].f[fi] >= 0) fused[fb[bi].f[fi]] = 0;
        fb.resize(std::min<size_t>(fb.size(), 1));
        R.rect_first = (int)o.rects.size();
        for (int k = 0; k < 3; k++) {
            R.n_rect[k] = 0;
            for (size_t j = 0; j < fr.size(); j++) {
                if (fused[j] || fr[j].k != k) continue;
                const int i = fr[j].i;
                o.rects.push_back(frame_rect(fr[j]));
                o.rects.back().sg = (int)o.prims.size() << 1;
                PrimF f = primf(i);
                const uint32_t fl = H[i].flags | F_FRAME_RECT;
                std::memcpy(&f.b.w, &fl, 4);
                push_slot(o, i, f);
                R.n_rect[k]++;
                G.n_flat_extra++;
                o.nt++;
            }
        }
        R.box = -1;
        if (!fb.empty()) { // at most one closed box per frame is tested as a box
            R.box = (int16_t)(frame_box_first + (int)frame_boxes.size());
            frame_boxes.push_back(box_rec(fr, fb[0], (int)o.prims.size()));
            for (int fi = 0; fi < 6; fi++) {
                const int i = box_face_prim(fr, fb[0], fi);
                PrimF f = primf(i);
                const uint32_t fl = H[i].flags | F_FRAME_RECT;
                std::memcpy(&f.b.w, &fl, 4);
                push_slot(o, i, f);
                G.n_flat_extra += fb[0].f[fi] >= 0;
                o.nt++;
            }
        }
        o.frames.push_back(R);
    }
};

// The flat order's decomposition (build statistics): the counts of its only group.
BruteLayout layout_of(const BruteOrder& flat)
{
    BruteLayout L;
    if (flat.groups.empty()) return L;
    const GroupRec& G = flat.groups[0];
    L.rects = G.n_rect[0] + G.n_rect[1] + G.n_rect[2];
    L.boxes = G.n_boxes;
    L.frames = G.n_frames;
    for (int f = 0; f < G.n_frames; f++) {
        const FrameRec& F = flat.frames[G.frame_first + f];
        L.frame_boxes += F.box >= 0;
        L.frame_rects += F.n_rect[0] + F.n_rect[1] + F.n_rect[2];
    }
    L.tris = flat.tris0;
    L.sphs = flat.sphs0;
    return L;
}

// The grouped order's groups: the SAH BVH cut into subtrees of at most group_max primitives
// (build_order's groups and skips).
struct GroupCut {
    const SahBvh& sah;
    const int group_max, super_min;
    std::vector<int> box_of; // box-aware cut: per primitive, the closed box it is a face of, or -1
    std::vector<std::vector<int>> box_faces;
    std::vector<char> box_done;
    std::vector<std::vector<int>> cut;
    std::vector<int> skips;

    // the world rectangles that make closed boxes, by the box finder on the whole scene
    void find_scene_boxes(const OrderBuilder& b, const std::vector<int>& all)
    {
        std::vector<OrderBuilder::RectG> wr;
        for (int i : all)
            if (b.kind_of[i] < 3) wr.push_back(b.rect_geom(i, b.kind_of[i], nullptr, nullptr));
        std::vector<char> used(wr.size(), 0);
        for (const OrderBuilder::BoxFit& f6 : OrderBuilder::find_boxes(wr, used)) {
            box_faces.emplace_back();
            for (int j : f6.f)
                if (j >= 0) {
                    box_of[wr[j].i] = (int)box_faces.size() - 1;
                    box_faces.back().push_back(wr[j].i);
                }
        }
        box_done.assign(box_faces.size(), 0);
    }
    std::vector<int> take_boxes(const std::vector<int>& sub) // a group's primitives, boxes whole
    {
        std::vector<int> g;
        for (int i : sub) {
            const int b = box_of[i];
            if (b < 0) {
                g.push_back(i);
            } else if (!box_done[b]) {
                box_done[b] = 1;
                g.insert(g.end(), box_faces[b].begin(), box_faces[b].end());
            }
        }
        return g;
    }
    void children(int ref, int& l, int& r) const // the child references of a BVH2 node
    {
        std::memcpy(&l, &sah.nodes[ref].lmin.w, 4);
        std::memcpy(&r, &sah.nodes[ref].rmin.w, 4);
    }
    void leaves(int ref, std::vector<int>& out) const
    {
        if (ref < 0) {
            const int code = ~ref, first = code >> 3, c = (code & 7) + 1;
            for (int k = first; k < first + c; k++) out.push_back(sah.order[k]);
            return;
        }
        int l, r;
        children(ref, l, r);
        leaves(l, out);
        leaves(r, out);
    }
    int n_cut(int ref) const // groups the cut makes of a subtree
    {
        std::vector<int> sub;
        leaves(ref, sub);
        if ((int)sub.size() <= group_max || ref < 0) return 1;
        int l, r;
        children(ref, l, r);
        return n_cut(l) + n_cut(r);
    }
    void split(int ref, bool in_super)
    {
        std::vector<int> sub;
        leaves(ref, sub);
        if ((int)sub.size() <= group_max || ref < 0) {
            std::vector<int> g = take_boxes(sub);
            if (!g.empty()) {
                cut.push_back(std::move(g));
                skips.push_back(0);
            }
            return;
        }
        int l, r;
        children(ref, l, r);
        const size_t at = cut.size();
        // one level: a super record inside another mostly repeats its box (die.txt: the die
        // and the die minus a face's pips)
        const bool super = super_min > 0 && !in_super && ref != sah.root && n_cut(ref) >= super_min;
        if (super) {
            cut.push_back(sub);
            skips.push_back(0);
        }
        split(l, in_super || super);
        split(r, in_super || super);
        if (super) {
            skips[at] = (int)(cut.size() - at - 1);
            // its box: the primitives of the groups it holds (a box taken whole may reach
            // outside the subtree); a super record holding fewer than two groups is dropped
            cut[at].clear();
            for (size_t k = at + 1; k < cut.size(); k++) cut[at].insert(cut[at].end(), cut[k].begin(), cut[k].end());
            if (skips[at] < 2) {
                cut.erase(cut.begin() + (long)at);
                skips.erase(skips.begin() + (long)at);
            }
        }
    }
};

} // namespace

BruteOrders make_brute_orders(const std::vector<HostPrim>& H, const std::vector<int>& xf_index, const SahBvh& sah,
                              int group_max, const std::vector<char>& outer)
{
    BruteOrders out;
    const OrderBuilder b(H, xf_index);
    const int n = b.n;
    std::vector<int> all;
    for (int i = 0; i < n; i++)
        if (b.kind_of[i] != 5) all.push_back(i);
    out.flat = b.build_order({all}, {0});
    if (!outer.empty()) {
        std::vector<int> ids;
        for (int i = 0; i < n; i++)
            if (outer[i]) ids.push_back(i);
        out.outer = b.build_order({ids}, {0});
    }
    for (int k = 0; k < 3; k++) out.nr[k] = out.flat.nr[k];
    out.nt = out.flat.nt;
    out.ns = out.flat.ns;
    out.layout = layout_of(out.flat);
    for (int i = 0; i < n; i++) out.np += b.kind_of[i] == 5;
    // groups: subtrees of the SAH BVH with at most kGroupMax primitives (small scenes only); the
    // caller chooses the size (group_max_default, scene_upload.hip, has the sweeps)
    int kGroupMax = group_max;
    if (const char* e = getenv("RTCORE_GROUP_MAX")) kGroupMax = std::max(1, atoi(e)); // tuning
    out.group_max = kGroupMax;
    // Super records: a subtree (below the root) that the cut makes into at least kSuperMin groups
    // also gets a record of its own box in front of them, so that a wave that misses it skips them
    // all (die.txt: the die's five groups behind one box; background rays then test two boxes
    // instead of six: 6.0 -> 4.69 box tests per ray, C3 26.81 -> 25.64 ms in the same call,
    // profiles/r04/ab_group_super_boxes.log).  RTCORE_GROUP_SUPER sets kSuperMin (0: none).
    int kSuperMin = 3;
    if (const char* e = getenv("RTCORE_GROUP_SUPER")) kSuperMin = std::max(0, atoi(e));
    // Box-aware cut (RTCORE_GROUP_BOXES=1, off): the world rectangles that make closed boxes (the
    // box finder on the whole scene) go to the first group that holds any of them, all together,
    // so that the group's box finder makes them one slab test instead of rectangles spread over
    // several groups (die.txt's cube: 4 + 1 + 1 faces in three groups).  Measured slower on
    // die.txt (C3 26.81 -> 28.73 ms; with super records 25.64 -> 27.56): the group that takes
    // the cube spans the whole die, so nearly every ray that meets the die tests its pips too
    // (sphere tests per ray 4.61 -> 6.18).
    bool group_boxes = false;
    if (const char* e = getenv("RTCORE_GROUP_BOXES")) group_boxes = atoi(e) != 0;
    GroupCut c{sah, kGroupMax, kSuperMin, std::vector<int>(n, -1), {}, {}, {}, {}};
    if (group_boxes && b.use_boxes) c.find_scene_boxes(b, all);
    if ((int)all.size() <= 4096 && !sah.order.empty()) c.split(sah.root, false);
    if (!c.cut.empty()) out.grouped = b.build_order(c.cut, c.skips);
    return out;
}

int grouping_max_leaf(GroupingTree who, int n_prims, bool has_outer)
{
    // The reporters' comments said "as rt_scene_create does"; none of the three is.  Settling it
    // changes the grouped records the reporters and the header generator make for n > 256.
    switch (who) {
    case GroupingTree::Scene: return n_prims > 256 && !has_outer ? 3 : 2;
    case GroupingTree::LayoutReport: return n_prims > 256 ? 4 : 2;
    case GroupingTree::JitHeader: return n_prims > 256 ? 3 : 2;
    }
    return 2;
}

HostRecords make_host_records(const std::vector<HostPrim>& H, int max_leaf, int group_max, const SahBvh* sah,
                              const std::vector<char>* outer)
{
    HostRecords r;
    const int n = (int)H.size();
    r.xf_index.assign(n, -1);
    for (int i = 0; i < n; i++) {
        const HostPrim& p = H[i];
        r.n_bvh += p.kind != RT_PRIM_PLANE;
        r.n_planes += p.kind == RT_PRIM_PLANE;
        r.n_vn += (p.kind == RT_PRIM_TRIANGLE && (p.flags & F_HASNORMALS)) ? 1 : 0;
        if (p.kind == RT_PRIM_SPHERE && (p.flags & F_TRANSFORMED)) {
            r.xf_index[i] = (int)r.xf.size();
            r.xf.push_back(make_xformf(p));
        }
    }
    SahBvh own;
    if (!sah && max_leaf > 0 && r.n_bvh > 0) own = build_sah_bvh(H, max_leaf);
    const SahBvh& tree = sah ? *sah : own;
    r.sah_root = tree.root;
    r.orders = make_brute_orders(H, r.xf_index, tree, group_max, outer ? *outer : std::vector<char>{});
    return r;
}

MatTable make_materials(const std::vector<HostPrim>& H, double air_ior)
{
    MatTable t;
    const int n = (int)H.size();
    t.mat_of.resize(n);
    std::unordered_map<std::string, int32_t> mat_index;
    for (int i = 0; i < n; i++) {
        const HostPrim& p = H[i];
        const bool refl = p.shininess > 0; // Primitive.IsReflective (Primitive.cs:107-129)
        rt_color spec = refl ? p.specular : rt_color{0, 0, 0};
        rt_color refr = refl ? p.refraction : rt_color{0, 0, 0};
        MatF m;
        std::memset(&m, 0, sizeof m);
        m.emission = make_float4((float)p.emission.r, (float)p.emission.g, (float)p.emission.b, (float)luminance(p.emission));
        m.diffuse = make_float4((float)p.diffuse.r, (float)p.diffuse.g, (float)p.diffuse.b, (float)luminance(p.diffuse));
        m.specular = make_float4((float)spec.r, (float)spec.g, (float)spec.b, (float)luminance(spec));
        m.refraction = make_float4((float)refr.r, (float)refr.g, (float)refr.b, (float)luminance(refr));
        m.shininess = (float)p.shininess;
        m.ior = (float)p.ior;
        m.flags = p.flags;
        m.inv_shininess = (float)(1.0 / p.shininess);
        // Raytracer.cs:127-133: ratio = iorIn / iorOut, air outside, swapped when the hit is Inside
        m.eta_enter = p.ior != 0 ? (float)(air_ior / p.ior) : 0.0f;
        m.eta_exit = p.ior != 0 ? (float)(p.ior / air_ior) : 0.0f;
        m.pad[0] = m.pad[1] = 0.0f;
        const std::string key(reinterpret_cast<const char*>(&m), sizeof m);
        auto it = mat_index.find(key);
        if (it == mat_index.end()) {
            it = mat_index.emplace(key, (int32_t)t.mats.size()).first;
            t.mats.push_back(m);
        }
        t.mat_of[i] = it->second;
    }
    return t;
}

// The grouped order's records sorted by the distance from the camera to their boxes (stable), as
// a tree: a super record keeps the records it holds (its skip) right behind it, sorted among
// themselves the same way.
std::vector<GroupRec> groups_nearest_first(const std::vector<GroupRec>& g, const CameraD& cam)
{
    const double px = cam.position.x, py = cam.position.y, pz = cam.position.z;
    auto dist2 = [&](const GroupRec& G) {
        // distance from the camera to the group's box (0 inside)
        const double dx = std::max({0.0, (double)G.lo.x - px, px - (double)G.hi.x});
        const double dy = std::max({0.0, (double)G.lo.y - py, py - (double)G.hi.y});
        const double dz = std::max({0.0, (double)G.lo.z - pz, pz - (double)G.hi.z});
        return dx * dx + dy * dy + dz * dz;
    };
    std::vector<GroupRec> out;
    std::function<void(size_t, size_t)> emit = [&](size_t a, size_t b) { // the sibling subtrees in [a, b)
        std::vector<std::pair<size_t, size_t>> sib;
        for (size_t i = a; i < b; i += 1 + (size_t)std::max(0, g[i].skip))
            sib.push_back({i, std::min(b, i + 1 + (size_t)std::max(0, g[i].skip))});
        std::stable_sort(sib.begin(), sib.end(), [&](const auto& x, const auto& y) { return dist2(g[x.first]) < dist2(g[y.first]); });
        for (const auto& [i, e] : sib) {
            out.push_back(g[i]);
            emit(i + 1, e);
        }
    };
    emit(0, g.size());
    return out;
}

// The fp32 transform rows of a transformed sphere (XformF).
XformF make_xformf(const HostPrim& p)
{
    XformF F;
    const double c[3] = {p.center.x, p.center.y, p.center.z};
    for (int r = 0; r < 3; r++) {
        F.to_world[r] = make_float4((float)p.to_world[4 * r], (float)p.to_world[4 * r + 1], (float)p.to_world[4 * r + 2],
                                    (float)p.to_world[4 * r + 3]);
        // normal(p) = N3 * (W * p + w - c) / r: one affine map of the world hit point
        double row[4] = {0, 0, 0, 0};
        for (int k = 0; k < 3; k++) {
            const double nk = p.to_normal[4 * r + k] / p.radius;
            for (int j = 0; j < 3; j++) row[j] += nk * p.to_world[4 * k + j];
            row[3] += nk * (p.to_world[4 * k + 3] - c[k]);
        }
        F.normal[r] = make_float4((float)row[0], (float)row[1], (float)row[2], (float)row[3]);
    }
    return F;
}

// What the scene's primitives and materials use at all (FACT_*, rt_internal.h).
uint32_t scene_facts(const std::vector<HostPrim>& H)
{
    uint32_t facts = 0;
    for (const HostPrim& p : H) {
        if (std::isinf(p.shininess) && p.shininess > 0) facts |= FACT_INF_SHININESS;
        if ((float)p.ior != 0.0f) facts |= FACT_IOR;
        if (p.flags & F_TRANSFORMED) facts |= FACT_XF;
        if (p.flags & F_HASNORMALS) facts |= FACT_VN;
        if (p.kind == RT_PRIM_SPHERE) facts |= FACT_SPHERE;
    }
    return facts;
}

// The scene bound: one world-space box over every primitive of the brute-force orders but the planes,
// which path_body tests once per wave of camera rays (scene_meets, kernels_path.hip) to skip the whole
// query of a wave that looks past the scene.  Triangles and parallelograms (frame rectangles and
// boxes among them: the loader bakes their vertices into world space) from their vertices, a sphere
// from centre +- r, a transformed sphere from the exact box of its ellipsoid: the world point of the
// object-space point q is MatrixToObject * q, so on world axis k the ellipsoid spans
// (MatrixToObject * centre)_k +- r |row k of its 3x3 part|.  All in fp64, rounded outward to fp32.
//
// The pad.  The kernel's predicate is the fp32 slab test t = fma(plane, id, -(o * id)) with id =
// slab_rcp_lean(d): id is 1 / d within one ulp (2^-23 relative, a scale of that axis's distances), the
// product o * id and the fma round once each (2^-24 relative).  Set against the exact distance of the
// plane along the ray, and brought back to position space (times |d|), a slab end is off by at most
//   2^-23 |plane - o| + 2^-24 (|o| + |plane - o|) <= 2^-22 (2 |o| + M),  M = the largest |coordinate| of the box,
// so it grows with the origin's distance from zero, not only with the box's extent.  The primitive
// tests are fp32 too and accept points as far outside their primitive as a few 2^-24 |o| (the
// triangle's (u, v), the sphere's perpendicular l = oc - (oc . d) d).  The predicate serves origins
// with |o.x| + |o.y| + |o.z| <= limit = 1024 M, and the box is padded on every side by
//   pad = 2^-18 (limit + M):
// 8 times the slab's own bound at the limit (2^-21 (limit + M)), the rest for the primitive tests'
// error.  For bounce.txt (M = 2) that is 0.0078 on a 4 x 4 x 2 room.  An origin past the limit
// counts as meeting the box, as does a ray with a NaN or an infinity in it.
// No bounded primitive: an empty bound, which no ray meets.  A NaN or infinite extent: limit = -1,
// so every origin is past it and the skip is off for the scene.
// One primitive's extent on the three axes (fp64), as the bounds take it; false for a plane.
static bool prim_extent(const HostPrim& p, double lo[3], double hi[3])
{
    for (int k = 0; k < 3; k++) {
        lo[k] = INFINITY;
        hi[k] = -INFINITY;
    }
    if (p.kind == RT_PRIM_TRIANGLE) {
        const Vec4d v3 = add(add(p.v[0], p.e01), p.e02); // a parallelogram's fourth vertex
        const int nv = (p.flags & F_MIRROR) ? 4 : 3;
        bool bad = false; // (min and max drop a NaN)
        for (int j = 0; j < nv; j++) {
            const Vec4d& v = j < 3 ? p.v[j] : v3;
            const double c[3] = {v.x, v.y, v.z};
            for (int k = 0; k < 3; k++) {
                bad |= !std::isfinite(c[k]);
                lo[k] = std::min(lo[k], c[k]);
                hi[k] = std::max(hi[k], c[k]);
            }
        }
        if (bad) lo[0] = hi[0] = NAN;
        return true;
    }
    if (p.kind == RT_PRIM_SPHERE) {
        const double c[3] = {p.center.x, p.center.y, p.center.z};
        for (int k = 0; k < 3; k++) {
            double mid = c[k], half = std::fabs(p.radius);
            if (p.flags & F_TRANSFORMED) {
                const double* m = p.to_obj + 4 * k;
                mid = m[0] * c[0] + m[1] * c[1] + m[2] * c[2] + m[3];
                half = std::fabs(p.radius) * std::sqrt(m[0] * m[0] + m[1] * m[1] + m[2] * m[2]);
            }
            // (the fp64 rounding of mid and half is 2^-52 relative: far inside the pad)
            lo[k] = mid - half;
            hi[k] = mid + half;
        }
        return true;
    }
    return false;
}
// [a - pad, c + pad] in fp32, rounded outward
static void pad_outward(double a, double c, double pad, float& lo, float& hi)
{
    a -= pad;
    c += pad;
    lo = (float)a;
    if ((double)lo > a) lo = std::nextafterf(lo, -INFINITY);
    hi = (float)c;
    if ((double)hi < c) hi = std::nextafterf(hi, INFINITY);
}

SceneBound make_scene_bound(const std::vector<HostPrim>& H)
{
    double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    bool any = false, bad = false;
    for (const HostPrim& p : H) {
        double a[3], c[3];
        if (!prim_extent(p, a, c)) continue;
        for (int k = 0; k < 3; k++) {
            if (!(std::isfinite(a[k]) && std::isfinite(c[k]))) bad = true;
            lo[k] = std::min(lo[k], a[k]);
            hi[k] = std::max(hi[k], c[k]);
        }
        any = true;
    }
    SceneBound b{};
    if (!any) {
        b.empty = 1;
        b.limit = INFINITY;
        return b;
    }
    double M = 0.0;
    for (int k = 0; k < 3; k++) M = std::max(M, std::max(std::fabs(lo[k]), std::fabs(hi[k])));
    const double limit = 1024.0 * M, pad = std::ldexp(limit + M, -18);
    if (bad || !std::isfinite(M) || !((float)(limit + M + pad) < INFINITY)) {
        b.limit = -1.0f; // the skip is off
        return b;
    }
    for (int k = 0; k < 3; k++) pad_outward(lo[k], hi[k], pad, b.lo[k], b.hi[k]);
    b.limit = (float)limit;
    if ((double)b.limit > limit) b.limit = std::nextafterf(b.limit, 0.0f); // never above what the pad covers
    b.pad = (float)pad;
    return b;
}

// The flat order's test units and their boxes (scene_records.h).  A unit's slots name its primitives
// (PrimF::a.w; a box's missing face has the slot of one of its other faces), and its box is the scene
// bound's construction over those primitives alone: the same extents, the same pad, so the argument
// that a ray past the padded box fails the fp32 tests of what is inside it holds unit by unit, for the
// origins the scene bound serves (its limit).
FlatUnits make_flat_units(const std::vector<HostPrim>& H, const BruteOrder& flat, const SceneBound& bound, int n_planes,
                          int n_vn)
{
    FlatUnits U;
    if (flat.groups.empty() || flat.overflow) return U;
    const GroupRec& G = flat.groups[0];
    auto slot_id = [&](int slot) {
        int id;
        std::memcpy(&id, &flat.prims[(size_t)slot].a.w, 4);
        return id;
    };
    auto box_ids = [&](const FrameRec& R, std::vector<int>& out) {
        BoxRec B;
        std::memcpy(&B, &R, sizeof B);
        for (int f = 0; f < 6; f++) out.push_back(slot_id((B.sg0 >> 1) + f));
    };
    int rect_first, tri_slot;
    std::memcpy(&rect_first, &G.lo.w, 4);
    std::memcpy(&tri_slot, &G.hi.w, 4);
    const int n_rects = G.n_rect[0] + G.n_rect[1] + G.n_rect[2];
    for (int k = 0; k < n_rects; k++) U.ids.push_back({slot_id(flat.rects[(size_t)(rect_first + k)].sg >> 1)});
    for (int j = 0; j < G.n_boxes; j++) {
        U.ids.emplace_back();
        box_ids(flat.frames[(size_t)(G.frame_first + G.n_frames + j)], U.ids.back());
    }
    for (int f = 0; f < G.n_frames; f++) {
        const FrameRec& F = flat.frames[(size_t)(G.frame_first + f)];
        U.ids.emplace_back();
        for (int k = 0; k < F.n_rect[0] + F.n_rect[1] + F.n_rect[2]; k++)
            U.ids.back().push_back(slot_id(flat.rects[(size_t)(F.rect_first + k)].sg >> 1));
        if (F.box >= 0) box_ids(flat.frames[(size_t)F.box], U.ids.back());
    }
    const int n_ts = (G.n_tri_sph & 0xFFFF) + (G.n_tri_sph >> 16);
    for (int i = 0; i < n_ts; i++) U.ids.push_back({slot_id(tri_slot + i)});
    U.n = (int)U.ids.size();
    bool ok = U.n == flat_unit_count(G) && U.n <= kMaxUnits && n_planes == 0 && n_vn == 0 && !bound.empty &&
              bound.limit >= 0.0f;
    U.lo.assign((size_t)U.n * 3, -INFINITY);
    U.hi.assign((size_t)U.n * 3, INFINITY);
    for (int u = 0; u < U.n && ok; u++) {
        double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
        for (int id : U.ids[(size_t)u]) {
            double a[3], c[3];
            if (id < 0 || id >= (int)H.size() || !prim_extent(H[(size_t)id], a, c)) {
                ok = false;
                break;
            }
            for (int k = 0; k < 3; k++) {
                lo[k] = std::min(lo[k], a[k]);
                hi[k] = std::max(hi[k], c[k]);
            }
        }
        for (int k = 0; k < 3 && ok; k++) {
            if (!(std::isfinite(lo[k]) && std::isfinite(hi[k]))) ok = false;
            else pad_outward(lo[k], hi[k], (double)bound.pad, U.lo[(size_t)u * 3 + k], U.hi[(size_t)u * 3 + k]);
        }
    }
    U.on = ok;
    return U;
}

// Which axis-aligned rectangles become outer records.  Only large ones pay: a wall whose box
// overlaps the whole scene sits near the root of any tree, while a small cube face is cheap inside
// it and would cost every query a test outside it (test_outer is linear in the group).  So a
// rectangle qualifies when its area is at least 1/kOuterAreaDiv of the scene box's largest face,
// and at most kOuterMax of them (largest first) are taken.  C4: the room's six walls and the
// light box's five faces (the smallest, 0.75 x 0.1, is 1/213 of the 4 x 4 face).  None, or all
// of the BVH primitives, leaves the tree as it is.
static constexpr int kOuterMax = 64;
static constexpr double kOuterAreaDiv = 1024.0;

void select_outer(const std::vector<HostPrim>& H, std::vector<char>& out)
{
    out.clear();
    const int n = (int)H.size();
    float slo[3] = {INFINITY, INFINITY, INFINITY}, shi[3] = {-INFINITY, -INFINITY, -INFINITY};
    int nb = 0;
    std::vector<std::pair<double, int>> cand;
    for (int i = 0; i < n; i++) {
        if (H[i].kind == RT_PRIM_PLANE) continue;
        nb++;
        float lo[3], hi[3];
        sah_prim_box(H[i], lo, hi);
        for (int k = 0; k < 3; k++) {
            slo[k] = std::min(slo[k], lo[k]);
            shi[k] = std::max(shi[k], hi[k]);
        }
        const int k = rect_axis_of(H[i]);
        if (k < 0) continue;
        const double a = (double)(hi[(k + 1) % 3] - lo[(k + 1) % 3]) * (double)(hi[(k + 2) % 3] - lo[(k + 2) % 3]);
        cand.push_back({a, i});
    }
    double face = 0.0;
    for (int k = 0; k < 3; k++)
        face = std::max(face, (double)(shi[(k + 1) % 3] - slo[(k + 1) % 3]) * (double)(shi[(k + 2) % 3] - slo[(k + 2) % 3]));
    // largest first, then by ID (a stable choice at the cap)
    std::sort(cand.begin(), cand.end(), [](const auto& a, const auto& b) { return a.first != b.first ? a.first > b.first : a.second < b.second; });
    std::vector<char> m(n, 0);
    int k = 0;
    for (const auto& c : cand) {
        if (k == kOuterMax || !(c.first * kOuterAreaDiv >= face)) break;
        m[c.second] = 1;
        k++;
    }
    if (k > 0 && k < nb) out = std::move(m);
}

} // namespace rtc
