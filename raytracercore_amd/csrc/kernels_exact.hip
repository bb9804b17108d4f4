// kernels_exact.hip -- the exact fp64 primary-ray pass (DebugRaycaster Primitives mode).
//
// Restates, per pixel, camera.GetRay(x, y).Offset(camera.imagePlane)
// (DebugRaycaster.cs:241; FrustumCamera.cs:33-41; OrthoCamera.cs:33-38) followed by
// Scene.RayTrace(ray, null) (Scene.cs:65-111): the reference BVH's IntersectLeaves
// (BVH.cs:295-331: every pierced leaf in depth-first order, AABB.IntersectAVX,
// SkipVolume reuse), the stable insertion sort by Near (Util.cs:262-280), the
// `Near > previous.Far` early break and the strict `<` replacement, with
// Primitive.RayTrace (Primitive.cs:46-75) over Triangle.RayTraceAVXFaster
// (Triangle.cs:77-146), Sphere.RayTraceAVX (Sphere.cs:50-155) and Plane.DoRayTrace
// (Plane.cs:36-66), which rt_exact_prims.h holds together with the Selection mode's fold
// (the selection kernels below).  Every operation keeps the reference's order and FMA use, and the file
// is compiled with -ffp-contract=off, so the result is bit-identical to an fp64 host
// restatement on the same inputs.
#include "rt_kernels.h"
#include "rt_exact_prims.h"

namespace rtc {

constexpr int kLeafCap = 64;
constexpr int kStackCap = 96;

__device__ static int cmp_near(double a, double b) // double.CompareTo
{
    if (a < b) return -1;
    if (a > b) return 1;
    if (a == b) return 0;
    return (a != a) ? ((b != b) ? 0 : -1) : 1;
}

struct LeafItem {
    int node;
    double nr, fr;
};

// The leaf scan of Scene.RayTracePrimitives (Scene.cs:74-91) over leaves given in sorted order.
struct LeafScan {
    int best = -1;
    double best_d = 0, prev_far = 0;
    bool best_in = false; // Hit.Inside of the best hit (after Invert)
    bool have_prev = false;
    // returns false once the `Near > previous.Far` break is reached
    __device__ bool visit(const DevScene& s, const LeafItem& it, Vec4d o, Vec4d d)
    {
        if (have_prev && it.nr > prev_far) return false;
        HitD h;
        if (prim_raytrace_d(s, s.ref_nodes[it.node].prim, o, d, h) && (best < 0 || h.dist < best_d)) {
            best = h.prim;
            best_d = h.dist;
            best_in = h.inside;
            prev_far = it.fr;
            have_prev = true;
        }
        return true;
    }
};

// (near, DFS ordinal) in the order of the stable insertion sort with double.CompareTo
__device__ static bool key_less(double an, int ao, double bn, int bo)
{
    const int c = cmp_near(an, bn);
    return c < 0 || (c == 0 && ao < bo);
}

// BVH<T>.IntersectLeaves (BVH.cs:295-331) as an explicit depth-first walk: calls f(item, ordinal)
// for every pierced leaf in the order the reference appends them.
template <class F>
__device__ static bool walk_leaves(const DevScene& s, Vec4d o, Vec4d d, F&& f)
{
    LeafItem stack[kStackCap];
    int sp = 0, ord = 0;
    stack[sp++] = LeafItem{0, 0.0, 0.0};
    while (sp > 0) {
        LeafItem it = stack[--sp];
        const RefNode& n = s.ref_nodes[it.node];
        if (!n.skip) {
            aabb_hit_ref(n.mn, n.mx, o, d, it.nr, it.fr);
            if (!(it.fr >= 0)) continue;
        }
        if (n.prim >= 0) {
            f(it, ord++);
            continue;
        }
        if (sp + 2 > kStackCap) return false;
        stack[sp++] = LeafItem{n.right, it.nr, it.fr};
        stack[sp++] = LeafItem{it.node + 1, it.nr, it.fr};
    }
    return true;
}

// Same result when more than kLeafCap leaves are pierced (large meshes): the leaves are taken in
// sorted order by repeated selection, one depth-first walk per leaf the scan consumes (the scan
// usually stops after a few leaves), so no list is stored.
__device__ static int ref_raytrace_select(const DevScene& s, Vec4d o, Vec4d d, LeafScan& scan)
{
    double cur_n = 0;
    int cur_o = -1;
    bool first = true;
    while (true) {
        LeafItem next{-1, 0.0, 0.0};
        int next_o = -1;
        const bool ok = walk_leaves(s, o, d, [&](const LeafItem& it, int ord) {
            if (!first && !key_less(cur_n, cur_o, it.nr, ord)) return; // already consumed
            if (next_o < 0 || key_less(it.nr, ord, next.nr, next_o)) {
                next = it;
                next_o = ord;
            }
        });
        if (!ok) return -2;
        if (next_o < 0 || !scan.visit(s, next, o, d)) break;
        cur_n = next.nr;
        cur_o = next_o;
        first = false;
    }
    return 0;
}

// Scene.RayTrace(ray, null) into scan (a fresh LeafScan; s.n_ref_nodes > 0): 0, or -2 if the
// traversal stack overflowed.
__device__ static int ref_raytrace_scan(const DevScene& s, Vec4d o, Vec4d d, LeafScan& scan)
{
    LeafItem leaves[kLeafCap];
    int nl = 0;
    bool overflow = false;
    const bool ok = walk_leaves(s, o, d, [&](const LeafItem& it, int) {
        if (nl < kLeafCap) leaves[nl++] = it;
        else overflow = true;
    });
    if (!ok) return -2;
    if (overflow) return ref_raytrace_select(s, o, d, scan);
    for (int i = 1; i < nl; i++) { // Util.InsertSort, stable
        LeafItem a = leaves[i];
        int j = i - 1;
        while (j >= 0 && cmp_near(a.nr, leaves[j].nr) < 0) {
            leaves[j + 1] = leaves[j];
            j--;
        }
        leaves[j + 1] = a;
    }
    for (int i = 0; i < nl; i++)
        if (!scan.visit(s, leaves[i], o, d)) break;
    return 0;
}

// Returns the primitive ID, -1 on a miss, -2 if the traversal stack overflowed.
__device__ int ref_raytrace(const DevScene& s, Vec4d o, Vec4d d)
{
    if (s.n_ref_nodes == 0) return -1;
    LeafScan scan;
    if (ref_raytrace_scan(s, o, d, scan) < 0) return -2;
    return scan.best;
}

// The same query with the winning hit: h = (ID, Hit.Distance, Hit.Inside), (-1, 0, false) on a miss.
// Returns the primitive ID, -1 or -2 as ref_raytrace.
__device__ int ref_raytrace_hit(const DevScene& s, Vec4d o, Vec4d d, HitD& h)
{
    h = HitD{-1, 0.0, false};
    if (s.n_ref_nodes == 0) return -1;
    LeafScan scan;
    if (ref_raytrace_scan(s, o, d, scan) < 0) return -2;
    if (scan.best >= 0) h = HitD{scan.best, scan.best_d, scan.best_in};
    return scan.best;
}

// BVH<T>.GetIntersectionCount (BVH.cs:352-363), DebugRaycaster BoundingVolumes mode: the nodes
// whose own box the ray meets (Volume.Intersect(ray).far >= 0), descending only through them.
__device__ int ref_bvh_count(const DevScene& s, Vec4d o, Vec4d d)
{
    if (s.n_ref_nodes == 0) return 0;
    int stack[kStackCap];
    int sp = 0, count = 0;
    stack[sp++] = 0;
    while (sp > 0) {
        const int i = stack[--sp];
        const RefNode& n = s.ref_nodes[i];
        double nr, fr;
        aabb_hit_ref(n.mn, n.mx, o, d, nr, fr);
        if (!(fr >= 0)) continue;
        count++;
        if (n.prim >= 0) continue;
        if (sp + 2 > kStackCap) return -2;
        stack[sp++] = n.right;
        stack[sp++] = i + 1;
    }
    return count;
}

// mode 0: primary hit IDs (Primitives mode), mode 1: BVH node counts (BoundingVolumes mode)
__global__ void __launch_bounds__(64) primary_ids_kernel(DevScene s, CameraD cam, int x0, int y0, int w, int h, int mode,
                                                         int32_t* ids)
{
    int x = blockIdx.x * 8 + (threadIdx.x & 7);
    int y = blockIdx.y * 8 + (threadIdx.x >> 3);
    if (x >= w || y >= h) return;
    Vec4d o, d;
    camera_ray_d(cam, (double)(x0 + x), (double)(y0 + y), o, d);
    ids[(size_t)y * w + x] = mode == 0 ? ref_raytrace(s, o, d) : ref_bvh_count(s, o, d);
}

// rt_query_rays, RT_QUERY_EXACT: the reference query on caller-supplied rays, one ray per lane.  A
// ray is four 16-B rows (origin, direction as Vec4D), a hit three: (ID, inside, distance) and two
// rows of zeros (rt_hit, rtcore.h).  A ray with a non-finite component or a zero direction is a miss
// (decided here, where the ray is loaded); prim_id -2 reports a traversal-stack overflow.
__global__ void __launch_bounds__(64) query_exact_kernel(DevScene s, const double2* __restrict__ rays, unsigned n,
                                                         uint4* __restrict__ hits)
{
    const unsigned i = blockIdx.x * 64u + threadIdx.x;
    if (i >= n) return;
    const double2 r0 = rays[4 * (size_t)i], r1 = rays[4 * (size_t)i + 1], r2 = rays[4 * (size_t)i + 2],
                  r3 = rays[4 * (size_t)i + 3];
    const Vec4d o{r0.x, r0.y, r1.x, r1.y}, d{r2.x, r2.y, r3.x, r3.y};
    const double inf = __builtin_huge_val();
    const bool finite = (fabs(o.x) < inf) & (fabs(o.y) < inf) & (fabs(o.z) < inf) & (fabs(o.w) < inf) & (fabs(d.x) < inf) &
                        (fabs(d.y) < inf) & (fabs(d.z) < inf) & (fabs(d.w) < inf); // false for NaN
    const bool valid = finite & ((d.x != 0.0) | (d.y != 0.0) | (d.z != 0.0));
    HitD h{-1, 0.0, false};
    int id = -1;
    if (valid) id = ref_raytrace_hit(s, o, d, h);
    const unsigned long long db = (unsigned long long)__double_as_longlong(h.dist);
    hits[3 * (size_t)i] = make_uint4((unsigned)id, h.inside ? 1u : 0u, (unsigned)db, (unsigned)(db >> 32));
    hits[3 * (size_t)i + 1] = make_uint4(0u, 0u, 0u, 0u);
    hits[3 * (size_t)i + 2] = make_uint4(0u, 0u, 0u, 0u);
}

// rt_occluded_rays, RT_QUERY_EXACT: the same query with its Hit.Distance held against t_max in fp64
// (strictly below: RayTracePrimitives' own comparison), one answer byte per ray.  No early exit: this
// is the reference's answer.  An invalid ray (ray_valid_d) or an empty segment (t_max NaN or <= 0)
// gives 0 without a query; 255 reports a traversal-stack overflow.
__global__ void __launch_bounds__(64) occluded_exact_kernel(DevScene s, const double2* __restrict__ rays,
                                                            const double* __restrict__ t_max, unsigned n,
                                                            unsigned char* __restrict__ out)
{
    const unsigned i = blockIdx.x * 64u + threadIdx.x;
    if (i >= n) return;
    const double2 r0 = rays[4 * (size_t)i], r1 = rays[4 * (size_t)i + 1], r2 = rays[4 * (size_t)i + 2],
                  r3 = rays[4 * (size_t)i + 3];
    const Vec4d o{r0.x, r0.y, r1.x, r1.y}, d{r2.x, r2.y, r3.x, r3.y};
    const double tm = t_max ? t_max[i] : __builtin_huge_val();
    unsigned char r = 0;
    if (ray_valid_d(o, d) && tm > 0.0) {
        HitD h;
        const int id = ref_raytrace_hit(s, o, d, h);
        r = id == -2 ? 255 : (id >= 0 && h.dist < tm) ? 1 : 0;
    }
    out[i] = r;
}

// DebugRaycaster Selection mode (rt_select_pixels, rt_select_rays): select_items (rt_exact_prims.h)
// for one ray per lane.  The item loop is the same for every lane of the wave (no early exit, no
// LDS); a result is one 16-B row (rt_selection: item, 0, distance), written with one store.
__device__ static void store_selection(uint4* out, size_t i, const rt_selection& r)
{
    const unsigned long long db = (unsigned long long)__double_as_longlong(r.distance);
    out[i] = make_uint4((unsigned)r.item, 0u, (unsigned)db, (unsigned)(db >> 32));
}

__global__ void __launch_bounds__(64) select_pixels_kernel(DevScene s, CameraD cam, const rt_select_item* __restrict__ items,
                                                           int n_items, int x0, int y0, int w, int h, uint4* __restrict__ out)
{
    int x = blockIdx.x * 8 + (threadIdx.x & 7);
    int y = blockIdx.y * 8 + (threadIdx.x >> 3);
    if (x >= w || y >= h) return;
    Vec4d o, d;
    camera_ray_d(cam, (double)(x0 + x), (double)(y0 + y), o, d);
    store_selection(out, (size_t)y * w + x, select_items(s, items, n_items, o, d));
}

__global__ void __launch_bounds__(64) select_rays_kernel(DevScene s, const rt_select_item* __restrict__ items, int n_items,
                                                         const double2* __restrict__ rays, unsigned n, uint4* __restrict__ out)
{
    const unsigned i = blockIdx.x * 64u + threadIdx.x;
    if (i >= n) return;
    const double2 r0 = rays[4 * (size_t)i], r1 = rays[4 * (size_t)i + 1], r2 = rays[4 * (size_t)i + 2],
                  r3 = rays[4 * (size_t)i + 3];
    const Vec4d o{r0.x, r0.y, r1.x, r1.y}, d{r2.x, r2.y, r3.x, r3.y};
    rt_selection r{-1, 0, 0.0};
    if (ray_valid_d(o, d)) r = select_items(s, items, n_items, o, d);
    store_selection(out, i, r);
}

hipError_t launch_select_pixels(const DevScene& s, const CameraD& cam, const rt_select_item* d_items, int n_items, int x0,
                                int y0, int w, int h, rt_selection* d_out, hipStream_t stream)
{
    static_assert(sizeof(rt_selection) == 16 && sizeof(rt_select_item) == 8, "rt_selection is one 16-B row");
    dim3 grid((w + 7) / 8, (h + 7) / 8);
    hipLaunchKernelGGL(select_pixels_kernel, grid, dim3(64), 0, stream, s, cam, d_items, n_items, x0, y0, w, h,
                       reinterpret_cast<uint4*>(d_out));
    return hipGetLastError();
}

hipError_t launch_select_rays(const DevScene& s, const rt_select_item* d_items, int n_items, const rt_ray* d_rays,
                              unsigned n, rt_selection* d_out, hipStream_t stream)
{
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(select_rays_kernel, dim3((n + 63u) / 64u), dim3(64), 0, stream, s, d_items, n_items,
                       reinterpret_cast<const double2*>(d_rays), n, reinterpret_cast<uint4*>(d_out));
    return hipGetLastError();
}

hipError_t launch_query_exact(const DevScene& s, const rt_ray* d_rays, unsigned n, rt_hit* d_hits, hipStream_t stream)
{
    static_assert(sizeof(rt_ray) == 64 && sizeof(rt_hit) == 48, "rt_ray is four 16-B rows, rt_hit three");
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(query_exact_kernel, dim3((n + 63u) / 64u), dim3(64), 0, stream, s,
                       reinterpret_cast<const double2*>(d_rays), n, reinterpret_cast<uint4*>(d_hits));
    return hipGetLastError();
}

hipError_t launch_occluded_exact(const DevScene& s, const rt_ray* d_rays, const double* d_t_max, unsigned n,
                                 unsigned char* d_out, hipStream_t stream)
{
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(occluded_exact_kernel, dim3((n + 63u) / 64u), dim3(64), 0, stream, s,
                       reinterpret_cast<const double2*>(d_rays), d_t_max, n, d_out);
    return hipGetLastError();
}

hipError_t launch_primary_ids(const DevScene& s, const CameraD& cam, int x0, int y0, int w, int h, int mode,
                              int32_t* d_ids, hipStream_t stream)
{
    dim3 grid((w + 7) / 8, (h + 7) / 8);
    hipLaunchKernelGGL(primary_ids_kernel, grid, dim3(64), 0, stream, s, cam, x0, y0, w, h, mode, d_ids);
    return hipGetLastError();
}

} // namespace rtc
