// kernels_query.hip -- the ray-list kernels: queries over a caller's rays, segments or surfels, built from
// rt_trace.h's closest-hit / any-hit query without a path on top.  trace_rays_kernel (rt_debug_trace_rays),
// query_* (rt_query_rays), occluded_* (rt_occluded_rays) and occluded_surfels_* (rt_occluded_surfels), each
// with its launcher.  Not a source of a scene-specialised build: nothing here changes a cached JIT kernel.
#include "rt_trace.h"

namespace rtc {
namespace {

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
} // namespace

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

} // namespace rtc
