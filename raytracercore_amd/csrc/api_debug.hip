// api_debug.hip -- the C ABI's host-only, checking and experiment entry points.
#include <cstdlib>
#include <cstring>

#include "rt_scene.h"

namespace {

int n_bvh_prims(const std::vector<HostPrim>& H)
{
    int nb = 0;
    for (const HostPrim& p : H) nb += p.kind != RT_PRIM_PLANE;
    return nb;
}

// The records of the two layout reporters: the grouping cuts a host SAH tree where rt_scene_create
// would build one on the host.
HostRecords report_records(const std::vector<HostPrim>& H)
{
    const bool host_tree = builder_for(n_bvh_prims(H)) == RT_BVH_BUILDER_HOST;
    return make_host_records(H, host_tree ? grouping_max_leaf(GroupingTree::LayoutReport, (int)H.size(), false) : 0,
                             group_max_default());
}

} // namespace

extern "C" {

int rt_debug_brute_layout(const rt_prim* prims, int32_t n_prims, int32_t* out, int32_t n_out)
{
    if (n_prims < 0 || (n_prims > 0 && !prims) || !out || n_out < 0) {
        set_error("rt_debug_brute_layout: bad argument");
        return RT_ERR_ARG;
    }
    for (int i = 0; i < n_prims; i++)
        if (prims[i].kind < 0 || prims[i].kind > 2) {
            set_error("rt_debug_brute_layout: unknown primitive kind at index " + std::to_string(i));
            return RT_ERR_ARG;
        }
    const HostRecords rec = report_records(prepare_prims(prims, n_prims));
    const BruteOrders& o = rec.orders;
    const BruteLayout& L = o.layout;
    const int32_t v[RT_LAYOUT_COUNT] = {L.rects, L.boxes, L.frames, L.frame_boxes, L.frame_rects, L.tris, L.sphs,
                                        o.np, o.grouped.groups.empty() ? 0 : (int32_t)o.grouped.groups.size(),
                                        (int32_t)o.grouped.prims.size() - o.np};
    for (int i = 0; i < n_out && i < RT_LAYOUT_COUNT; i++) out[i] = v[i];
    return RT_OK;
}

// Experiment support: the flat brute-force order's records as 32-bit words (groups | rects |
// frames | tests); counts = {groups, rects, frames, tests}.  Host code only.
int rt_debug_flat_records(const rt_prim* prims, int32_t n_prims, uint32_t* out, int64_t cap_words, int32_t* counts)
{
    if (n_prims < 0 || (n_prims > 0 && !prims) || !out || !counts) {
        set_error("rt_debug_flat_records: bad argument");
        return RT_ERR_ARG;
    }
    const HostRecords rec = report_records(prepare_prims(prims, n_prims));
    const BruteOrder& f = rec.orders.flat;
    size_t w = 0;
    auto put = [&](const void* p, size_t bytes) {
        const size_t k = bytes / 4;
        if ((int64_t)(w + k) <= cap_words) memcpy(out + w, p, bytes);
        w += k;
    };
    put(f.groups.data(), f.groups.size() * sizeof(GroupRec));
    put(f.rects.data(), f.rects.size() * sizeof(RectRec));
    put(f.frames.data(), f.frames.size() * sizeof(FrameRec));
    put(f.tests.data(), f.tests.size() * sizeof(TestRec));
    counts[0] = (int32_t)f.groups.size();
    counts[1] = (int32_t)f.rects.size();
    counts[2] = (int32_t)f.frames.size();
    counts[3] = (int32_t)f.tests.size();
    if ((int64_t)w > cap_words) {
        set_error("rt_debug_flat_records: buffer too small");
        return RT_ERR_ARG;
    }
    return RT_OK;
}

// Experiment support (host only, no device): the generated header of the scene-specialised build
// that rt_scene_create + rt_scene_set_camera would make for these primitives and this camera, so
// that its code can be compiled and read on a machine without a GPU (tools/jit_isa.py).  Returns
// the header's length (copied into buf, NUL-terminated, when it fits in cap).
int rt_debug_jit_header(const rt_scene_params* params, const rt_prim* prims, int32_t n_prims, const rt_camera* camera,
                        int32_t grouped, char* buf, int64_t cap)
{
    if (!params || !camera || n_prims < 0 || (n_prims > 0 && !prims) || (grouped != 0 && grouped != 1)) {
        set_error("rt_debug_jit_header: bad argument");
        return RT_ERR_ARG;
    }
    const std::vector<HostPrim> H = prepare_prims(prims, n_prims);
    if (n_bvh_prims(H) > 48) {
        set_error("rt_debug_jit_header: the scene-specialised build serves brute-force scenes (<= 48 primitives)");
        return RT_ERR_ARG;
    }
    const HostRecords rec =
        make_host_records(H, grouping_max_leaf(GroupingTree::JitHeader, (int)H.size(), false), group_max_default());
    const BruteOrders& o = rec.orders;
    const std::vector<XformF>& xf = rec.xf;
    const int np = rec.n_planes;
    const BruteOrder& B = grouped ? o.grouped : o.flat;
    if (grouped && B.groups.empty()) {
        set_error("rt_debug_jit_header: no grouped order for this scene");
        return RT_ERR_ARG;
    }
    PathScene ps; // make_path_scene + fill_launch, from the host records
    std::memset(&ps, 0, sizeof ps);
    for (int k = 0; k < 3; k++) ps.n_rect[k] = o.nr[k];
    ps.n_tri = o.nt;
    ps.n_sph = o.ns;
    ps.n_pln = np;
    ps.n_bvh = (int)B.prims.size() - np;
    ps.n_slots = ps.n_bvh + np;
    ps.n_mats = (int)make_materials(H, params->air_ior).mats.size();
    ps.n_xf = (int)xf.size();
    ps.n_vn = rec.n_vn;
    ps.facts = getenv("RTCORE_NO_FACTS") ? (uint32_t)FACT_ALL : scene_facts(H);
    ps.n_groups = grouped ? (int)B.groups.size() : 1;
    ps.root = rec.sah_root;
    ps.width = params->width;
    ps.recursion = params->recursion;
    ps.debug_geom = params->debug_geom;
    const rt_color& a = params->ambient;
    ps.ambient_miss = (a.r == -1 && a.g == -1 && a.b == -1) ? 1 : 0;
    ps.air_ior = (float)params->air_ior;
    ps.ambient_r = (float)a.r;
    ps.ambient_g = (float)a.g;
    ps.ambient_b = (float)a.b;
    set_scene_bound(ps, make_scene_bound(H));
    CameraD camd;
    CameraF camf;
    camera_init(*camera, params->width, params->height, camd, camf);
    const std::vector<GroupRec> groups =
        (grouped && B.groups.size() > 1 && !getenv("RTCORE_NO_GROUP_SORT")) ? groups_nearest_first(B.groups, camd) : B.groups;
    const std::string h = jit_scene_header(ps, camf, grouped == 1, groups, B.rects, B.frames, B.tests, xf);
    if (buf && cap > (int64_t)h.size()) std::memcpy(buf, h.c_str(), h.size() + 1);
    return (int)h.size();
}

int rt_debug_vn_rehit(const double* v0, const double* e01, const double* e02, int32_t mirror, double u, double v,
                      const float* dir, int32_t* inside, double* t, double* origin)
{
    if (!v0 || !e01 || !e02 || !dir || !inside || !t || !origin) {
        set_error("rt_debug_vn_rehit: bad argument");
        return RT_ERR_ARG;
    }
    int in = 0;
    const int hit = debug_vn_rehit(v0, e01, e02, mirror, u, v, dir, &in, t, origin);
    *inside = in;
    return hit;
}

int rt_debug_ray_log(rt_scene* s, void* d_log, uint32_t cap, void* d_count)
{
    if (!s || (d_log && !d_count)) {
        set_error("rt_debug_ray_log: bad argument");
        return RT_ERR_ARG;
    }
    s->ray_log = static_cast<float4*>(d_log);
    s->ray_log_n = static_cast<unsigned int*>(d_count);
    s->ray_log_cap = d_log ? cap : 0;
    return RT_OK;
}

int rt_debug_trace_rays(rt_scene* s, const void* d_rays, uint32_t n, void* d_hits, int32_t waves, void* d_stats,
                        void* stream, float* ms)
{
    if (!s || !d_rays || !d_hits || !ms || waves < 6 || waves > 8) {
        set_error("rt_debug_trace_rays: bad argument");
        return RT_ERR_ARG;
    }
    if (s->dev.n_pln > 0 || s->bvh.n_nodes4 == 0) {
        set_error("rt_debug_trace_rays: needs a wide BVH and a scene without planes");
        return RT_ERR_STATE;
    }
    // the trace-only kernel starts every query from no hit: the vertex-normal re-hit start of a
    // logged query (Sample.prev <= -2, query_start) is not restated there
    if (s->dev.n_vn > 0) {
        set_error("rt_debug_trace_rays: scenes with vertex-normal triangles are not supported");
        return RT_ERR_STATE;
    }
    HIP_TRY(hipSetDevice(s->device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    // the work counter and the stack overflow area are the scene's: order after its last render
    if (s->any_op && st != s->last_stream) HIP_TRY(hipStreamWaitEvent(st, s->done_ev, 0));
    const int grid = s->n_cu * trace_rays_blocks_per_cu(waves);
    HIP_TRY(s->stack_ovf.reserve((size_t)grid * 256 * kStackOverflow));
    HIP_TRY(s->counter.reserve(1));
    HIP_TRY(hipMemsetAsync(s->counter.p, 0, sizeof(unsigned int), st));
    TraceRaysParams p{};
    p.rays = static_cast<const float4*>(d_rays);
    p.hits = static_cast<float2*>(d_hits);
    p.n = n;
    p.counter = s->counter.p;
    p.stack_ovf = s->stack_ovf.p;
    p.tests = s->dev.tests_bvh;
    p.rows = s->dev.rows_bvh;
    p.nodes4 = s->dev.nodes4;
    p.xf = s->dev.xf;
    p.root4 = s->dev.root4;
    if (s->dev.n_outer > 0) {
        p.outer = s->dev.groups_bvh;
        p.outer_rects = s->dev.rects_bvh;
        p.outer_boxes = s->dev.frames_bvh;
    }
    p.spec = 16;
    if (const char* e = getenv("RTCORE_BVH_SPEC")) p.spec = std::max(1, std::min(64, atoi(e)));
    p.stats = static_cast<unsigned long long*>(d_stats);
    struct Events { // destroyed on every exit path
        hipEvent_t e0 = nullptr, e1 = nullptr;
        ~Events()
        {
            if (e0) (void)hipEventDestroy(e0);
            if (e1) (void)hipEventDestroy(e1);
        }
    } ev;
    HIP_TRY(hipEventCreate(&ev.e0));
    HIP_TRY(hipEventCreate(&ev.e1));
    HIP_TRY(hipEventRecord(ev.e0, st));
    HIP_TRY(launch_trace_rays(p, waves, grid, st));
    HIP_TRY(hipEventRecord(ev.e1, st));
    const int rc = end_op(s, st);
    if (rc != RT_OK) return rc;
    HIP_TRY(hipEventSynchronize(ev.e1));
    HIP_TRY(hipEventElapsedTime(ms, ev.e0, ev.e1));
    return RT_OK;
}

int rt_debug_jit_compile(const char* arch, int32_t grouped, char* log, int32_t cap)
{
    if (!arch || (grouped != 0 && grouped != 1)) {
        set_error("rt_debug_jit_compile: bad argument");
        return RT_ERR_ARG;
    }
    std::string err;
    const size_t n = jit_compile_check(arch, grouped == 1, err);
    if (log && cap > 0) {
        const size_t k = std::min((size_t)cap - 1, err.size());
        memcpy(log, err.data(), k);
        log[k] = '\0';
    }
    if (n == 0) {
        set_error("rt_debug_jit_compile: " + err);
        return RT_ERR_STATE;
    }
    return (int)std::min(n, (size_t)0x7fffffff);
}

// Structural check of the device-resident fast-path BVHs (either builder): every child box of
// the BVH2 and every dequantised child box of the wide tree contains the boxes of all primitives
// below it, every non-plane primitive sits in exactly one leaf of each tree, and the depth and
// stack figures the kernels were sized by are not exceeded.
int rt_scene_check_bvh(rt_scene* s)
{
    if (!s) {
        set_error("rt_scene_check_bvh: bad argument");
        return RT_ERR_ARG;
    }
    HIP_TRY(hipSetDevice(s->device));
    const auto& H = s->host;
    const int n = (int)H.size();
    // nb: the slots the tree's leaves address (outer records, when present, follow them)
    auto outside = [&](int i) { return H[i].kind == RT_PRIM_PLANE || (!s->bvh_outer.empty() && s->bvh_outer[i]); };
    int nb = 0;
    for (int i = 0; i < n; i++) nb += !outside(i);
    std::vector<NodeF> n2(s->bvh.n_nodes2);
    std::vector<Node4Q> n4(s->bvh.n_nodes4);
    std::vector<PrimF> recs(nb);
    if (!n2.empty()) HIP_TRY(hipMemcpy(n2.data(), s->nodes.p, n2.size() * sizeof(NodeF), hipMemcpyDeviceToHost));
    if (!n4.empty()) HIP_TRY(hipMemcpy(n4.data(), s->nodes4.p, n4.size() * sizeof(Node4Q), hipMemcpyDeviceToHost));
    if (nb > 0) HIP_TRY(hipMemcpy(recs.data(), s->bvh_d.prims.p, nb * sizeof(PrimF), hipMemcpyDeviceToHost));
    std::vector<int> id(nb);
    for (int k = 0; k < nb; k++) std::memcpy(&id[k], &recs[k].a.w, 4);
    struct B {
        double lo[3], hi[3];
    };
    auto empty = [] {
        B b;
        for (int a = 0; a < 3; a++) {
            b.lo[a] = __builtin_huge_val();
            b.hi[a] = -__builtin_huge_val();
        }
        return b;
    };
    auto grow = [](B& b, const B& c) {
        for (int a = 0; a < 3; a++) {
            b.lo[a] = std::min(b.lo[a], c.lo[a]);
            b.hi[a] = std::max(b.hi[a], c.hi[a]);
        }
    };
    std::vector<B> pbox(n);
    for (int i = 0; i < n; i++)
        if (H[i].kind != RT_PRIM_PLANE) {
            float l[3], h[3];
            sah_prim_box(H[i], l, h);
            for (int a = 0; a < 3; a++) {
                pbox[i].lo[a] = l[a];
                pbox[i].hi[a] = h[a];
            }
        }
    std::string err;
    std::vector<int> seen(n, 0);
    const uint32_t test_mask = KIND_MASK | F_MIRROR | F_TWOSIDED | F_INVERT | F_TRANSFORMED;
    auto leaf = [&](int ref, B& u) {
        int first, cnt;
        leaf_range(ref, first, cnt);
        const bool compact = ((~ref) & kLeafCompact) != 0;
        const uint32_t lfl = leaf_flags(((uint32_t)(~ref) >> 25) & 31u);
        if (first < 0 || first + cnt > nb) {
            err = "leaf range out of bounds";
            return;
        }
        if (compact && first + cnt > kLeafCompactMaxFirst) {
            err = "compact leaf beyond the slots its code can address";
            return;
        }
        for (int k = first; k < first + cnt; k++) {
            const int p = id[k];
            if (p < 0 || p >= n || outside(p)) {
                err = "leaf record with a bad primitive ID";
                return;
            }
            // a compact leaf's flags are what its primitives' own records say
            if (compact && (H[p].flags & test_mask) != lfl) {
                err = "compact leaf flags differ from primitive " + std::to_string(p);
                return;
            }
            seen[p]++;
            grow(u, pbox[p]);
        }
    };
    auto contains = [](const B& outer, const B& inner) {
        for (int a = 0; a < 3; a++)
            if (!(outer.lo[a] <= inner.lo[a] && outer.hi[a] >= inner.hi[a])) return false;
        return true;
    };
    // BVH2
    int max_depth = 0;
    std::function<B(int, int)> walk2 = [&](int ref, int depth) -> B {
        B u = empty();
        max_depth = std::max(max_depth, depth);
        if (!err.empty()) return u;
        if (ref < 0) {
            leaf(ref, u);
            return u;
        }
        if (ref >= (int)n2.size()) {
            err = "BVH2 child index out of range";
            return u;
        }
        const NodeF& q = n2[ref];
        for (int side = 0; side < 2; side++) {
            const float4 lo = side ? q.rmin : q.lmin, hi = side ? q.rmax : q.lmax;
            int c;
            std::memcpy(&c, &lo.w, 4);
            const B sub = walk2(c, depth + 1);
            const B box{{lo.x, lo.y, lo.z}, {hi.x, hi.y, hi.z}};
            if (err.empty() && !contains(box, sub)) err = "BVH2 child box misses a primitive below it";
            grow(u, sub);
        }
        return u;
    };
    if (nb > 0) walk2(s->bvh.root2, 0);
    for (int i = 0; i < n && err.empty(); i++)
        if (seen[i] != (outside(i) ? 0 : 1))
            err = "BVH2: primitive " + std::to_string(i) + " referenced " + std::to_string(seen[i]) + " times";
    if (err.empty() && max_depth > s->bvh.depth2) err = "BVH2 deeper than its recorded depth";
    // wide tree
    std::fill(seen.begin(), seen.end(), 0);
    int max_stack = 0;
    std::function<B(int, int)> walk4 = [&](int ref, int pushes) -> B {
        B u = empty();
        if (!err.empty()) return u;
        if (ref < 0) {
            leaf(ref, u);
            return u;
        }
        if (ref >= (int)n4.size()) {
            err = "wide child index out of range";
            return u;
        }
        const Node4Q& q = n4[ref];
        uint32_t ex, ql[3], qh[3];
        int refs[4], nc;
        std::memcpy(&ex, &q.a.w, 4);
        std::memcpy(&ql[0], &q.b.x, 4);
        std::memcpy(&qh[0], &q.b.y, 4);
        std::memcpy(&ql[1], &q.b.z, 4);
        std::memcpy(&qh[1], &q.b.w, 4);
        std::memcpy(&ql[2], &q.c.x, 4);
        std::memcpy(&qh[2], &q.c.y, 4);
        std::memcpy(&refs[0], &q.c.z, 4);
        std::memcpy(&refs[1], &q.c.w, 4);
        std::memcpy(&refs[2], &q.d.x, 4);
        std::memcpy(&refs[3], &q.d.y, 4);
        std::memcpy(&nc, &q.d.z, 4);
        if (nc < 1 || nc > 4) {
            err = "wide node with a bad child count";
            return u;
        }
        max_stack = std::max(max_stack, pushes + nc - 1);
        const double org[3] = {q.a.x, q.a.y, q.a.z};
        for (int k = 0; k < nc; k++) {
            const B sub = walk4(refs[k], pushes + nc - 1);
            B box;
            for (int a = 0; a < 3; a++) {
                const double sc = std::ldexp(1.0, (int)((ex >> (8 * a)) & 255u) - 128);
                box.lo[a] = org[a] + ((ql[a] >> (8 * k)) & 255u) * sc;
                box.hi[a] = org[a] + ((qh[a] >> (8 * k)) & 255u) * sc;
            }
            if (err.empty() && !contains(box, sub)) err = "wide child box misses a primitive below it";
            grow(u, sub);
        }
        return u;
    };
    if (err.empty() && nb > 0) walk4(s->bvh.root4, 0);
    for (int i = 0; i < n && err.empty(); i++)
        if (seen[i] != (outside(i) ? 0 : 1))
            err = "wide tree: primitive " + std::to_string(i) + " referenced " + std::to_string(seen[i]) + " times";
    if (err.empty() && max_stack > s->bvh.stack4) err = "wide tree needs more stack than recorded";
    if (!err.empty()) {
        set_error("rt_scene_check_bvh: " + err);
        return RT_ERR_STATE;
    }
    return RT_OK;
}

// Host only: the launch record of such a render (make_params_for, set_band) and every ticket of its
// dispensers through ticket_items, the function the kernels' refill calls.
int rt_debug_item_order(int32_t w, int32_t h, int32_t spp, int32_t chunks, int32_t pool, int32_t band,
                        int32_t band_stride, int32_t band_offset, uint32_t* out, int64_t cap_words, int32_t* info)
{
    const bool banded = band > 0;
    if (w <= 0 || h <= 0 || spp <= 0 || chunks < 0 || pool < 0 || pool % 64 != 0 || cap_words < 0 ||
        (cap_words > 0 && !out) || (banded && (band_stride <= 0 || band_offset < 0 || band_offset >= band_stride))) {
        set_error("rt_debug_item_order: bad argument");
        return RT_ERR_ARG;
    }
    const int rows = banded ? band_set_rows(h, band, band_stride, band_offset) : h;
    if (rows <= 0) return 0;
    PathParams p = make_params_for(pool > 64 ? 1 : 0, chunks, pool, 0, 0, w, rows, spp, 0, 0, 0.0);
    if (banded) set_band(p, band, band_stride, band_offset);
    if ((uint64_t)p.n_chunks * (uint64_t)p.n_pad > 0xF0000000ull) {
        set_error("rt_debug_item_order: tile x spp too large for one launch");
        return RT_ERR_ARG;
    }
    if (info) {
        info[0] = p.n_chunks;
        info[1] = p.chunk;
        info[2] = p.pool;
        info[3] = p.n_split;
    }
    const int64_t n = list_tickets(p, out, cap_words);
    if (n > INT32_MAX) {
        set_error("rt_debug_item_order: too many tickets");
        return RT_ERR_ARG;
    }
    return (int)n;
}

// Host only: the launch record of rt_render_pixels for a list of n entries (make_params_pixels).
int rt_debug_pixels_plan(int32_t kernel, int64_t n, int32_t spp, int32_t* info)
{
    if (kernel < 0 || kernel > 3 || kernel == 2 || n <= 0 || n > ((int64_t)1 << 30) || spp <= 0 || !info) {
        set_error("rt_debug_pixels_plan: bad argument");
        return RT_ERR_ARG;
    }
    const PathParams p = make_params_pixels(kernel, n, spp, 0, 0, 1920, 1080);
    info[0] = p.n_chunks;
    info[1] = p.chunk;
    info[2] = (p.spp + p.chunk - 1) / p.chunk;
    info[3] = p.n_pad / 64;
    return RT_OK;
}

// Host only: the scene bound rt_scene_create would give the brute-force path kernels for these primitives.
int rt_debug_scene_bound(const rt_prim* prims, int32_t n_prims, float* lo, float* hi, float* info)
{
    if (n_prims < 0 || (n_prims > 0 && !prims) || !lo || !hi) {
        set_error("rt_debug_scene_bound: bad argument");
        return RT_ERR_ARG;
    }
    for (int i = 0; i < n_prims; i++)
        if (prims[i].kind < 0 || prims[i].kind > 2) {
            set_error("rt_debug_scene_bound: unknown primitive kind at index " + std::to_string(i));
            return RT_ERR_ARG;
        }
    const SceneBound b = make_scene_bound(prepare_prims(prims, n_prims));
    for (int k = 0; k < 3; k++) {
        lo[k] = b.lo[k];
        hi[k] = b.hi[k];
    }
    if (info) {
        info[0] = b.limit;
        info[1] = b.pad;
    }
    return b.empty ? 1 : (b.limit < 0.0f ? 2 : 0);
}

// Host only: the block cull run_path would plan a brute-force launch of this window with (block_cull.h).
int rt_debug_block_cull(const rt_prim* prims, int32_t n_prims, const rt_camera* camera, int32_t width, int32_t height,
                        int32_t x0, int32_t y0, int32_t w, int32_t h, int32_t band, int32_t band_stride,
                        int32_t band_offset, uint8_t* dead, int64_t cap, int32_t* info)
{
    const bool banded = band > 0;
    if (n_prims < 0 || (n_prims > 0 && !prims) || !camera || width <= 0 || height <= 0 || w <= 0 || h <= 0 || x0 < 0 ||
        y0 < 0 || x0 + w > width || cap < 0 || (cap > 0 && !dead) || band < 0 ||
        (camera->kind != RT_CAMERA_FRUSTUM && camera->kind != RT_CAMERA_ORTHO) ||
        (banded && (band_stride <= 0 || band_offset < 0 || band_offset >= band_stride)) || (!banded && y0 + h > height)) {
        set_error("rt_debug_block_cull: bad argument");
        return RT_ERR_ARG;
    }
    int n_planes = 0;
    for (int i = 0; i < n_prims; i++) {
        if (prims[i].kind < 0 || prims[i].kind > 2) {
            set_error("rt_debug_block_cull: unknown primitive kind at index " + std::to_string(i));
            return RT_ERR_ARG;
        }
        n_planes += prims[i].kind == RT_PRIM_PLANE ? 1 : 0;
    }
    const SceneBound b = make_scene_bound(prepare_prims(prims, n_prims));
    CameraD camd;
    CameraF camf;
    camera_init(*camera, width, height, camd, camf);
    const CullWindow win{x0, y0, w, h, banded ? band : 0, banded ? band_stride : 0, banded ? band_offset : 0};
    std::vector<unsigned char> flags;
    const int live = cull_blocks(camf, b, n_planes, win, flags);
    for (size_t i = 0; i < flags.size() && (int64_t)i < cap; i++) dead[i] = flags[i];
    if (info) {
        info[0] = (w + 7) / 8;
        info[1] = (h + 7) / 8;
    }
    return live;
}

// Host only: the first bounce's test units and the unit masks run_path would add to the cull record of such a
// launch (make_flat_units, unit_masks).
int rt_debug_block_units(const rt_prim* prims, int32_t n_prims, const rt_camera* camera, int32_t width, int32_t height,
                         int32_t x0, int32_t y0, int32_t w, int32_t h, int32_t band, int32_t band_stride,
                         int32_t band_offset, int32_t* unit_first, int32_t* unit_ids, int64_t cap_ids, float* unit_box,
                         uint8_t* dead, uint64_t* masks, int64_t cap_blocks, int32_t* info)
{
    const bool banded = band > 0;
    if (n_prims < 0 || (n_prims > 0 && !prims) || !camera || width <= 0 || height <= 0 || w <= 0 || h <= 0 || x0 < 0 ||
        y0 < 0 || x0 + w > width || cap_ids < 0 || (cap_ids > 0 && !unit_ids) || cap_blocks < 0 ||
        (cap_blocks > 0 && (!dead || !masks)) || band < 0 ||
        (camera->kind != RT_CAMERA_FRUSTUM && camera->kind != RT_CAMERA_ORTHO) ||
        (banded && (band_stride <= 0 || band_offset < 0 || band_offset >= band_stride)) || (!banded && y0 + h > height)) {
        set_error("rt_debug_block_units: bad argument");
        return RT_ERR_ARG;
    }
    for (int i = 0; i < n_prims; i++)
        if (prims[i].kind < 0 || prims[i].kind > 2) {
            set_error("rt_debug_block_units: unknown primitive kind at index " + std::to_string(i));
            return RT_ERR_ARG;
        }
    const std::vector<HostPrim> H = prepare_prims(prims, n_prims);
    const HostRecords rec = report_records(H);
    const SceneBound b = make_scene_bound(H);
    const FlatUnits U = make_flat_units(H, rec.orders.flat, b, rec.n_planes, rec.n_vn);
    CameraD camd;
    CameraF camf;
    camera_init(*camera, width, height, camd, camf);
    const CullWindow win{x0, y0, w, h, banded ? band : 0, banded ? band_stride : 0, banded ? band_offset : 0};
    std::vector<unsigned char> flags;
    const int live = cull_blocks(camf, b, rec.n_planes, win, flags);
    // run_path keeps a cull record, and with it the masks, only when some block is dead
    std::vector<uint64_t> m((size_t)live, ~0ull);
    const bool on = U.on && live > 0 && live < (int)flags.size() &&
                    unit_masks(camf, b, U.n, U.lo.data(), U.hi.data(), win, flags, m);
    int64_t n_ids = 0;
    for (int u = 0; u < U.n; u++) {
        if (unit_first && u < kMaxUnits) unit_first[u] = (int32_t)n_ids;
        for (int id : U.ids[(size_t)u]) {
            if (n_ids < cap_ids) unit_ids[n_ids] = id;
            n_ids++;
        }
        if (unit_box && u < kMaxUnits)
            for (int k = 0; k < 3; k++) {
                unit_box[6 * u + k] = U.lo[(size_t)u * 3 + k];
                unit_box[6 * u + 3 + k] = U.hi[(size_t)u * 3 + k];
            }
    }
    if (unit_first && U.n <= kMaxUnits) unit_first[U.n] = (int32_t)n_ids;
    for (size_t i = 0; i < flags.size() && (int64_t)i < cap_blocks; i++) dead[i] = flags[i];
    for (size_t i = 0; i < m.size() && (int64_t)i < cap_blocks; i++) masks[i] = m[i];
    if (info) {
        info[0] = (w + 7) / 8;
        info[1] = (h + 7) / 8;
        info[2] = live;
        info[3] = on ? 1 : 0;
        info[4] = (int32_t)std::min<int64_t>(n_ids, INT32_MAX);
        std::memcpy(&info[5], &b.pad, 4);
    }
    return U.n;
}

// Host only: the start rows run_path would plan for such a launch (make_params_for, plan_start_rows).
int rt_debug_start_rows(int32_t kernel, const rt_camera* camera, int32_t w, int32_t h, int32_t spp, int32_t chunks,
                        int32_t grid_blocks, int32_t flags, int64_t* info)
{
    if (kernel < 0 || kernel > 3 || !camera || w <= 0 || h <= 0 || spp <= 0 || chunks < 0 || grid_blocks <= 0 || !info ||
        (camera->kind != RT_CAMERA_FRUSTUM && camera->kind != RT_CAMERA_ORTHO)) {
        set_error("rt_debug_start_rows: bad argument");
        return RT_ERR_ARG;
    }
    CameraD camd;
    CameraF camf;
    camera_init(*camera, w, h, camd, camf);
    const PathParams p = make_params_for(kernel, chunks, 0, 0, 0, w, h, spp, 0, 0, 0.0);
    const StartRowsPlan sr = plan_start_rows(kernel, (flags & 1) != 0, (flags & 2) != 0, camf.kind, camf.dof != 0.0f, p.chunk, grid_blocks);
    info[0] = sr.rows;
    info[1] = (int64_t)sr.bytes;
    info[2] = p.chunk;
    return sr.on ? 1 : 0;
}

// Host only: run_path's two decisions about launch overlap (launch_overlaps, overlap_wait).
int rt_debug_launch_overlap(int32_t launch_flags, uint64_t partial_bytes, int32_t change_flags, int32_t* wait)
{
    if (launch_flags < 0 || launch_flags > 31 || change_flags < 0 || change_flags > 31 || !wait) {
        set_error("rt_debug_launch_overlap: bad argument");
        return RT_ERR_ARG;
    }
    const OverlapChange c{(change_flags & 1) != 0, (change_flags & 2) != 0, (change_flags & 4) != 0,
                          (change_flags & 8) != 0, (change_flags & 16) != 0};
    *wait = (int32_t)overlap_wait(c);
    return launch_overlaps((launch_flags & 1) != 0, (launch_flags & 8) != 0, (launch_flags & 16) != 0, (launch_flags & 2) != 0, (launch_flags & 4) != 0,
                           (size_t)partial_bytes) ? 1 : 0;
}

int rt_parse_scene(const char* text, rt_scene_params* params, rt_prim* prims, int32_t* n_prims, rt_camera* cameras,
                   int32_t* n_cameras)
{
    if (!text || !n_prims || !n_cameras) {
        set_error("rt_parse_scene: bad argument");
        return RT_ERR_ARG;
    }
    ParsedScene ps;
    std::string err;
    if (!parse_scene_text(text, ps, err)) {
        set_error(err);
        return RT_ERR_PARSE;
    }
    const int cap_p = *n_prims, cap_c = *n_cameras;
    *n_prims = (int32_t)ps.prims.size();
    *n_cameras = (int32_t)ps.cameras.size();
    if (params) *params = ps.params;
    if (prims) {
        if (cap_p < (int)ps.prims.size()) {
            set_error("rt_parse_scene: primitive array too small");
            return RT_ERR_ARG;
        }
        std::copy(ps.prims.begin(), ps.prims.end(), prims);
    }
    if (cameras) {
        if (cap_c < (int)ps.cameras.size()) {
            set_error("rt_parse_scene: camera array too small");
            return RT_ERR_ARG;
        }
        std::copy(ps.cameras.begin(), ps.cameras.end(), cameras);
    }
    return RT_OK;
}

int rt_ref_bvh_export(const rt_prim* prims, int32_t n, int32_t* leaf_order, double* boxes, int32_t* n_nodes,
                      int32_t* depth)
{
    if (n < 0 || (n > 0 && !prims)) {
        set_error("rt_ref_bvh_export: bad argument");
        return RT_ERR_ARG;
    }
    std::vector<HostPrim> host = prepare_prims(prims, n);
    RefBvh ref = build_ref_bvh(host);
    int k = 0;
    for (size_t i = 0; i < ref.nodes.size(); i++) {
        const RefNode& r = ref.nodes[i];
        if (r.prim >= 0 && leaf_order) leaf_order[k++] = r.prim;
        if (boxes) {
            double* b = boxes + 8 * i;
            b[0] = r.mn.x; b[1] = r.mn.y; b[2] = r.mn.z; b[3] = r.mn.w;
            b[4] = r.mx.x; b[5] = r.mx.y; b[6] = r.mx.z; b[7] = r.mx.w;
        }
    }
    if (n_nodes) *n_nodes = (int32_t)ref.nodes.size();
    if (depth) *depth = ref.depth;
    return RT_OK;
}

} // extern "C"
