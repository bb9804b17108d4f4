// block_cull.cpp -- a conservative cull of the 8x8 pixel blocks of a path-tracing launch (block_cull.h).
//
// A block is dead when no sample of any of its pixels can give a camera ray that meets the scene
// bound (make_scene_bound).  What holds that up is the argument of the wave-level skip (path_body,
// DESIGN 3.2e): the bound's pad covers the fp32 error of the kernel's slab predicate and of the
// primitive tests, so a ray that misses the padded box is answered "miss" by the kernel's own query,
// whether the wave skips it or runs it.  A dead pixel's result is therefore known before the launch:
// misses += spp, rays += spp, nothing added to the sums.  The pad is the bound's business; the
// margins below are this file's, and cover only how the kernel forms a camera ray.
//
// The ray set.  The kernel's camera ray for the sample position (sx, sy) (camera_ray, kernels_path.hip)
// is, for the frustum camera, the ray from `position` along look + ox side + oy up with
// ox = fma(sx, tan_x_per_px, -tan_x), oy likewise; for the orthographic camera the ray along look
// from position + (sx - w2) h_mult side + (sy - h2) v_mult up.  Written in the basis dual to
// (side, up, look), a point P = position + a side + b up + c look with c > 0 lies on the ray of
// exactly one sample position: (a / c, b / c) mapped affinely to (sx, sy) for the frustum camera,
// (a, b) mapped affinely for the orthographic one.  No orthonormality is assumed, so the fp32
// rounding of the basis is part of the exact model.  Both maps take the box, a convex set wholly in
// c > 0, to a convex set of the sample plane: the convex hull of its eight corners' images.  A ray
// meets the box exactly when its sample position lies in that hull, so a rectangle of sample
// positions is dead exactly when it is disjoint from the hull.  Rectangle against convex polygon has
// an exact separating-axis test in 2D: the rectangle's two axes and the hull's edge normals.  The
// hull of bounce.txt's room from camera 0 is a hexagon; its bounding rectangle alone would cull 62.8 %
// of the 1080p frame's blocks, the hull culls 76 %.
// The image_plane offset moves a ray's origin along the ray: forward it only shortens the ray, and
// backward it adds a stretch behind the camera plane, where no part of the box is (every corner is
// required to be ahead of it).
//
// The sample rectangle of a run of pixels [xa, xb] x [ya, yb] is [xa, xb + 1] x [ya, yb + 1]: the
// jitter is x + U, U in [0, 1), rounded to fp32, which can give x + 1 exactly and nothing beyond.
// It is widened on every side by kMargin = 1/4 pixel for the fp32 arithmetic between the sample
// position and the ray.  In pixel units that error is bounded as follows (u = 2^-24):
//   frustum: ox and oy round once (<= u |tan|); the two fmas of each direction component round once
//     each, on values no larger than L = 1 + |tan_x| + |tan_y| (<= 2 u L per component, with the
//     carried error of ox, oy under 2^-21 L for the vector); the normalise changes each component by
//     a few u relative (<= 2^-21 L).  The direction is off by less than 2^-20 L, its slopes a / c,
//     b / c (each below L) by less than 1.01 * 2^-20 L^2, that is 2^-20 L^2 / min |tan_per_px| pixels
//     -- and the origin's fma with image_plane moves it sideways by at most 2^-22 (|position| +
//     |image_plane|), seen from the nearest corner at depth c_min.  bounce.txt camera 0 at 1080p:
//     L = 3.8, 0.007 pixels.
//   orthographic: sx - w2 and its product round once each (<= 2 u w pixels); the origin's three fmas
//     round on values up to R = |position| + reach + |image_plane| (<= 2^-22 R in position); the
//     normalised look is off by 2^-22 relative, which at the box's far depth c_max moves the ray by
//     2^-22 c_max.  Together 2^-22 (R + c_max) / min(|h_mult|, |v_mult|) + 2^-22 w pixels.
// The proof is given up (every block live) when that bound exceeds kMargin / 8, so the margin is
// always at least eight times the error.  The box is also grown by the bound's own pad once more
// before it is projected: the kernel's fp32 predicate may answer "meets" for a ray that passes the
// padded box within the predicate's error (an eighth of the pad), and a dead block's rays should
// fail that predicate too, not only the exact test.
//
// Nothing is culled when: the scene has planes (they lie outside the bound, and test_planes runs
// outside the skip); the bound's state is "no skip"; the camera has depth of field (its ray set is
// no pyramid); a camera value is NaN or infinite, or its basis is degenerate; the camera origin is
// past the bound's limit (the kernel counts such an origin as meeting the box); a corner of the box
// is not ahead of the camera plane by kAhead of its distance (a camera inside or beside the box).
// An empty bound with no planes makes every block dead: there is nothing to meet.
#include "block_cull.h"

#include <algorithm>
#include <cmath>

namespace rtc {

namespace {

constexpr double kMargin = 0.25;  // pixels added on every side of a sample rectangle
constexpr double kAhead = 1e-3;   // a corner's depth along look, relative to its distance, at the least

struct P2 {
    double x, y;
};

// The bound's image in the sample plane: a convex polygon, counter-clockwise, and its bounding rectangle.
struct Hull {
    std::vector<P2> v;
    double xmin, xmax, ymin, ymax;
};

double cross2(P2 o, P2 a, P2 b) { return (a.x - o.x) * (b.y - o.y) - (a.y - o.y) * (b.x - o.x); }

void convex_hull(std::vector<P2> pts, Hull& h)
{
    std::sort(pts.begin(), pts.end(), [](P2 a, P2 b) { return a.x < b.x || (a.x == b.x && a.y < b.y); });
    std::vector<P2> v(2 * pts.size());
    size_t k = 0;
    for (size_t i = 0; i < pts.size(); i++) { // lower chain
        while (k >= 2 && cross2(v[k - 2], v[k - 1], pts[i]) <= 0.0) k--;
        v[k++] = pts[i];
    }
    for (size_t i = pts.size() - 1, t = k + 1; i > 0; i--) { // upper chain
        while (k >= t && cross2(v[k - 2], v[k - 1], pts[i - 1]) <= 0.0) k--;
        v[k++] = pts[i - 1];
    }
    v.resize(k > 1 ? k - 1 : k);
    h.v = v;
    h.xmin = h.ymin = INFINITY;
    h.xmax = h.ymax = -INFINITY;
    for (P2 p : pts) {
        h.xmin = std::min(h.xmin, p.x);
        h.xmax = std::max(h.xmax, p.x);
        h.ymin = std::min(h.ymin, p.y);
        h.ymax = std::max(h.ymax, p.y);
    }
}

// Is the rectangle [xa, xb] x [ya, yb] disjoint from the hull?  The rectangle's axes, then the hull's
// edge normals: the corner of the rectangle deepest inside an edge decides that edge.  (A hull
// without area has only the first test, which errs on the live side.)
bool separated(const Hull& h, double xa, double xb, double ya, double yb)
{
    if (xb < h.xmin || xa > h.xmax || yb < h.ymin || ya > h.ymax) return true;
    const size_t n = h.v.size();
    if (n < 3) return false;
    for (size_t i = 0; i < n; i++) {
        const P2 p = h.v[i], q = h.v[i + 1 == n ? 0 : i + 1];
        const double nx = q.y - p.y, ny = -(q.x - p.x); // outward for a counter-clockwise polygon
        const double cx = nx > 0.0 ? xa : xb, cy = ny > 0.0 ? ya : yb;
        if (nx * (cx - p.x) + ny * (cy - p.y) > 0.0) return true;
    }
    return false;
}

struct V3d {
    double x, y, z;
};
V3d crs(V3d a, V3d b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
double dot(V3d a, V3d b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
V3d v3d(const float4& f) { return {(double)f.x, (double)f.y, (double)f.z}; }

// The hull of the bound for this camera, or false when the proof is not available.
bool project_bound(const CameraF& c, const SceneBound& b, int frame_w, Hull& hull)
{
    const bool frustum = c.kind == RT_CAMERA_FRUSTUM;
    const double vals[] = {c.position.x, c.position.y, c.position.z, c.look.x, c.look.y, c.look.z, c.side.x,
                           c.side.y, c.side.z, c.up.x, c.up.y, c.up.z, c.w2, c.h2, c.tan_x, c.tan_y,
                           c.h_mult, c.v_mult, c.image_plane, c.dof, c.focal_length, c.tan_x_per_px, c.tan_y_per_px};
    for (double v : vals)
        if (!std::isfinite(v)) return false;
    if (c.dof != 0.0f) return false;
    const V3d pos = v3d(c.position), look = v3d(c.look), side = v3d(c.side), up = v3d(c.up);
    const double apos = std::fabs(pos.x) + std::fabs(pos.y) + std::fabs(pos.z);
    // the dual basis of (side, up, look): P - position = a side + b up + c look
    const V3d da = crs(up, look), db = crs(look, side), dc = crs(side, up);
    const double det = dot(side, da);
    if (!(std::fabs(det) > 0.5 && std::fabs(det) < 2.0)) return false; // InitRender's basis is orthonormal
    const double sxa = frustum ? c.tan_x_per_px : c.h_mult, sya = frustum ? c.tan_y_per_px : c.v_mult;
    if (sxa == 0.0 || sya == 0.0) return false;
    const double scale = std::min(std::fabs(sxa), std::fabs(sya));
    if (frustum) {
        if (!(apos <= (double)b.limit)) return false;
    } else { // the origins of the frame's rays: position + the reach of the image
        const double reach = std::fabs((double)c.w2 * c.h_mult) * (std::fabs(side.x) + std::fabs(side.y) + std::fabs(side.z)) +
                             std::fabs((double)c.h2 * c.v_mult) * (std::fabs(up.x) + std::fabs(up.y) + std::fabs(up.z));
        if (!(apos + 2.0 * reach + std::fabs((double)c.image_plane) <= (double)b.limit)) return false;
    }
    std::vector<P2> pts;
    double c_min = INFINITY, c_max = 0.0;
    for (int k = 0; k < 8; k++) {
        const V3d P = {(k & 1) ? (double)b.hi[0] + b.pad : (double)b.lo[0] - b.pad,
                       (k & 2) ? (double)b.hi[1] + b.pad : (double)b.lo[1] - b.pad,
                       (k & 4) ? (double)b.hi[2] + b.pad : (double)b.lo[2] - b.pad};
        const V3d v = {P.x - pos.x, P.y - pos.y, P.z - pos.z};
        const double a = dot(v, da) / det, bb = dot(v, db) / det, cc = dot(v, dc) / det;
        if (!(cc > kAhead * std::sqrt(dot(v, v))) || !(cc > 0.0)) return false;
        c_min = std::min(c_min, cc);
        c_max = std::max(c_max, cc);
        if (frustum) pts.push_back({(a / cc + (double)c.tan_x) / sxa, (bb / cc + (double)c.tan_y) / sya});
        else pts.push_back({a / sxa + (double)c.w2, bb / sya + (double)c.h2});
    }
    // the fp32 error of the kernel's ray in pixels (the bound derived at the top of this file)
    double err;
    if (frustum) {
        const double L = 1.0 + std::fabs((double)c.tan_x) + std::fabs((double)c.tan_y);
        err = std::ldexp(L * L, -20) / scale +
              std::ldexp(apos + std::fabs((double)c.image_plane), -22) / (c_min * scale);
    } else {
        const double R = apos + std::fabs((double)c.w2 * c.h_mult) + std::fabs((double)c.h2 * c.v_mult) +
                         std::fabs((double)c.image_plane);
        err = std::ldexp(R + c_max, -22) / scale + std::ldexp((double)std::max(frame_w, 1), -22);
    }
    if (!(err <= kMargin / 8.0)) return false;
    for (P2 p : pts)
        if (!(std::isfinite(p.x) && std::isfinite(p.y))) return false;
    convex_hull(pts, hull);
    return true;
}

// Block row by's runs of consecutive frame rows (one run without a band set, or when the band length
// is a multiple of 8).
int block_runs(const CullWindow& win, int by, int run_a[8], int run_b[8])
{
    int runs = 0;
    for (int py = by * 8; py < std::min(win.h, by * 8 + 8); py++) {
        int fy = win.y0 + py;
        if (win.band > 0) fy = win.y0 + ((py / win.band) * win.band_stride + win.band_offset) * win.band + py % win.band;
        if (runs > 0 && fy == run_b[runs - 1] + 1) run_b[runs - 1] = fy;
        else {
            run_a[runs] = run_b[runs] = fy;
            runs++;
        }
    }
    return runs;
}

// Is block (bx, by)'s sample rectangle, widened by kMargin, disjoint from the hull?
bool block_misses(const Hull& hull, const CullWindow& win, int bx, int runs, const int run_a[8], const int run_b[8])
{
    const double xa = (double)(win.x0 + bx * 8) - kMargin;
    const double xb = (double)(win.x0 + std::min(win.w, bx * 8 + 8)) + kMargin; // last pixel + 1
    bool miss = true;
    for (int r = 0; r < runs && miss; r++)
        miss = separated(hull, xa, xb, (double)run_a[r] - kMargin, (double)(run_b[r] + 1) + kMargin);
    return miss;
}

} // namespace

// The unit masks (block_cull.h).  Each unit's box goes through the cull's own projection: grown by the
// bound's pad once more, every corner ahead of the camera plane by kAhead, the fp32 error of the
// kernel's ray below kMargin / 8 at the unit's own nearest corner.  What the cull's argument says of the
// scene bound it then says of the unit: a camera ray of a block whose widened sample rectangle is
// disjoint from that hull passes the unit's padded box, and the pad covers the fp32 tests of the
// unit's primitives (make_flat_units), so each of them answers "miss" for it, run or not.
bool unit_masks(const CameraF& cam, const SceneBound& bound, int n_units, const float* unit_lo, const float* unit_hi,
                const CullWindow& win, const std::vector<unsigned char>& dead, std::vector<uint64_t>& masks)
{
    const int bxn = (win.w + 7) / 8, byn = (win.h + 7) / 8;
    size_t n_live = 0;
    for (unsigned char d : dead) n_live += d ? 0 : 1;
    masks.assign(n_live, ~0ull);
    Hull scene_hull;
    if (n_units < 0 || n_units > 64 || bound.empty || !(bound.limit >= 0.0f) || dead.size() != (size_t)bxn * byn ||
        !project_bound(cam, bound, (int)(2.0f * cam.w2), scene_hull))
        return false;
    std::vector<Hull> hulls((size_t)n_units);
    uint64_t proven = 0; // units with a hull
    for (int u = 0; u < n_units; u++) {
        SceneBound ub = bound; // the scene's limit and pad
        for (int k = 0; k < 3; k++) {
            ub.lo[k] = unit_lo[3 * u + k];
            ub.hi[k] = unit_hi[3 * u + k];
        }
        if (project_bound(cam, ub, (int)(2.0f * cam.w2), hulls[(size_t)u])) proven |= 1ull << u;
    }
    const uint64_t all = n_units == 64 ? ~0ull : (1ull << n_units) - 1ull;
    size_t live = 0;
    for (int by = 0; by < byn; by++) {
        int run_a[8], run_b[8];
        const int runs = block_runs(win, by, run_a, run_b);
        for (int bx = 0; bx < bxn; bx++) {
            if (dead[(size_t)by * bxn + bx]) continue;
            uint64_t m = all;
            for (int u = 0; u < n_units; u++)
                if (((proven >> u) & 1ull) && block_misses(hulls[(size_t)u], win, bx, runs, run_a, run_b)) m &= ~(1ull << u);
            masks[live++] = m;
        }
    }
    return true;
}

int cull_blocks(const CameraF& cam, const SceneBound& bound, int n_planes, const CullWindow& win,
                std::vector<unsigned char>& dead)
{
    const int bxn = (win.w + 7) / 8, byn = (win.h + 7) / 8;
    const int n = bxn * byn;
    dead.assign((size_t)n, 0);
    if (n_planes > 0) return n;
    if (bound.empty) {
        dead.assign((size_t)n, 1);
        return 0;
    }
    if (!(bound.limit >= 0.0f)) return n;
    Hull hull;
    if (!project_bound(cam, bound, (int)(2.0f * cam.w2), hull)) return n;
    int live = 0;
    for (int by = 0; by < byn; by++) {
        int run_a[8], run_b[8];
        const int runs = block_runs(win, by, run_a, run_b);
        for (int bx = 0; bx < bxn; bx++) {
            const bool is_dead = block_misses(hull, win, bx, runs, run_a, run_b);
            dead[(size_t)by * bxn + bx] = is_dead ? 1 : 0;
            live += is_dead ? 0 : 1;
        }
    }
    return live;
}

uint64_t dead_pixels(const CullWindow& win, const std::vector<unsigned char>& dead)
{
    const int bxn = (win.w + 7) / 8, byn = (win.h + 7) / 8;
    uint64_t n = 0;
    for (int by = 0; by < byn; by++)
        for (int bx = 0; bx < bxn; bx++)
            if (dead[(size_t)by * bxn + bx])
                n += (uint64_t)(std::min(win.w, bx * 8 + 8) - bx * 8) * (uint64_t)(std::min(win.h, by * 8 + 8) - by * 8);
    return n;
}

} // namespace rtc
