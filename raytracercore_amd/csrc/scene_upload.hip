// scene_upload.hip -- from prepared primitives to a scene the kernels can run: the BVHs, the upload
// of every record, the choice of kernel variant, and the launch of the path kernel (rt_scene.h).
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <unordered_map>

#include "bvh_gpu.h"
#include "rt_scene.h"

namespace rtc {

static std::atomic<int> g_builder{RT_BVH_BUILDER_AUTO};
// AUTO builds on the GPU from this many BVH primitives.  Below it the host's binned-SAH tree is
// worth its build time: on the 1 M-triangle mesh (C4) the PLOC tree costs 15 % more node visits
// and 8 % of the render rate, against 0.4 s of build time saved.
constexpr int kGpuBuildMin = 1 << 22;

int builder_for(int n_bvh)
{
    int b = g_builder.load();
    if (b == RT_BVH_BUILDER_AUTO)
        if (const char* e = getenv("RTCORE_BVH_BUILDER")) // for A/B measurements
            b = std::strcmp(e, "gpu") == 0 ? RT_BVH_BUILDER_GPU : std::strcmp(e, "host") == 0 ? RT_BVH_BUILDER_HOST : b;
    if (b == RT_BVH_BUILDER_AUTO) b = n_bvh >= kGpuBuildMin ? RT_BVH_BUILDER_GPU : RT_BVH_BUILDER_HOST;
    return n_bvh > 0 ? b : RT_BVH_BUILDER_HOST;
}

// Primitives per group of the grouped order.
// generic kernel, die.txt 1080p grouped: 2 -> 50.1 ms, 3 -> 47.6, 4 -> 46.4, 6 -> 48.4, 8 -> 48.4, 16 -> 50.7;
// scene-specialised build (literal operands make primitive tests cheaper than group tests):
// 2 -> 32.8, 3 -> 30.6, 4 -> 30.2-30.4, 5 -> 28.9, 6 -> 29.1, 7 -> 28.3, 8 -> 28.3, 10 -> 30.2, 16 -> 30.9
// The size is fixed at scene creation, by the process-wide rt_set_jit state then: a later
// rt_set_jit(0) leaves the generic grouped kernel on groups of 8 (correct, tuned for the
// specialised build); build statistic 18 (group_max) records the size chosen.
int group_max_default() { return jit_enabled() ? 8 : 4; }

// The fast-path BVH2 and its wide collapse, by the host (binned SAH, bvh_sah.cpp) or the GPU
// (PLOC, bvh_gpu.hip).  Planes are never in the BVH.
int build_bvhs(rt_scene* s)
{
    const auto& H = s->host;
    const int n = (int)H.size();
    std::vector<int32_t> ids;
    for (int i = 0; i < n; i++)
        if (H[i].kind != RT_PRIM_PLANE) ids.push_back(i);
    const int nb = (int)ids.size();
    if (nb + kTestSpares >= kLeafGenericMaxSlots) { // leaf codes (rt_internal.h) address 2^27 slots
        set_error("rt_scene_create: more than 2^27 - " + std::to_string(kTestSpares) + " BVH primitives");
        return RT_ERR_ARG;
    }
    s->bvh.builder = builder_for(nb);
    // Outer records: in a large scene (nb > 4096: no grouped brute-force order, which would cut
    // this tree) the axis-aligned rectangles -- a room's walls, a light box -- stay out of the
    // tree and are tested as one group of rects and closed boxes when a query ends.  Their
    // large boxes overlap the whole scene near the root (tools/bvh_sim.cpp on C4's mesh: node
    // visits per query 8.75 -> 7.88, primitive tests 5.33 -> 2.46; measured: C4 46.5 -> 44.0 ms,
    // nodes 9.16 -> 8.34 and leaf tests 5.75 -> 2.88 per ray segment).  RTCORE_BVH_OUTER=0: off.
    bool outer_on = nb > 4096;
    if (const char* e = getenv("RTCORE_BVH_OUTER")) outer_on = outer_on && atoi(e) != 0;
    s->bvh_outer.clear();
    if (outer_on) select_outer(H, s->bvh_outer);
    // leaves of <= 3 primitives, <= 2 with outer records (C4, round 2: leaves of <= 2, 3, 4, 6, 8 ->
    // 70.6, 70.5, 72.2, 76.1, 80.2 ms; round 5 with outer records: 2 / 3 / 4 -> 43.8 / 44.0 / 47.2)
    int max_leaf = grouping_max_leaf(GroupingTree::Scene, n, !s->bvh_outer.empty());
    if (const char* e = getenv("RTCORE_MAX_LEAF")) max_leaf = std::max(1, std::min(8, atoi(e))); // tuning
    if (s->bvh.builder == RT_BVH_BUILDER_HOST) {
        // the wide tree: greedy collapse of the BVH2 (default), or the SAH-optimal collapse of the
        // whole SAH tree (RTCORE_WIDE_COLLAPSE=1; RTCORE_WIDE_CNODE / _CPRIM / _LEAF set its costs)
        WideCosts wc;
        bool sah_collapse = false; // measured slower on C4
        if (const char* e = getenv("RTCORE_WIDE_COLLAPSE")) sah_collapse = atoi(e) != 0;
        if (const char* e = getenv("RTCORE_WIDE_CNODE")) wc.c_node = (float)atof(e);
        if (const char* e = getenv("RTCORE_WIDE_CPRIM")) wc.c_prim = (float)atof(e);
        if (const char* e = getenv("RTCORE_WIDE_LEAF")) wc.max_leaf = std::max(1, std::min(8, atoi(e)));
        s->sah = build_sah_bvh(H, max_leaf, sah_collapse, s->bvh_outer.empty() ? nullptr : &s->bvh_outer);
        s->bvh4 = build_bvh4(s->sah, sah_collapse ? &wc : nullptr);
        s->sah.full.clear(); // only the collapse reads the whole tree
        s->sah.full.shrink_to_fit();
        s->bvh.n_nodes2 = (int)s->sah.nodes.size();
        s->bvh.root2 = s->sah.root;
        s->bvh.depth2 = s->sah.depth;
        s->bvh.n_nodes4 = (int)s->bvh4.nodes.size();
        s->bvh.root4 = s->bvh4.root;
        s->bvh.stack4 = s->bvh4.stack_need;
        return RT_OK;
    }
    const int n_planes = n - nb;
    if (!s->bvh_outer.empty()) // the outer records stay out of the GPU builder's tree too
        ids.erase(std::remove_if(ids.begin(), ids.end(), [&](int32_t i) { return s->bvh_outer[i] != 0; }), ids.end());
    const int n_tree = (int)ids.size();
    std::vector<float4> lo(n_tree), hi(n_tree);
    parallel_for(n_tree, [&](int k) {
        float l[3], h[3];
        sah_prim_box(H[ids[k]], l, h);
        lo[k] = make_float4(l[0], l[1], l[2], 0.0f);
        hi[k] = make_float4(h[0], h[1], h[2], 0.0f);
    });
    GpuBvh g;
    HIP_TRY(build_bvh_gpu(lo.data(), hi.data(), ids.data(), n_tree, max_leaf, n_planes + 1, s->stream, g));
    s->nodes.adopt(g.nodes, g.n_nodes);
    s->nodes4.adopt(g.nodes4, g.n_nodes4);
    s->order_d.adopt(g.order, (size_t)n_tree + n_planes + 1);
    s->bvh.n_nodes2 = g.n_nodes;
    s->bvh.root2 = g.root;
    s->bvh.depth2 = g.depth;
    s->bvh.n_nodes4 = g.n_nodes4;
    s->bvh.root4 = g.root4;
    s->bvh.stack4 = g.stack_need;
    s->bvh.rounds = g.rounds;
    s->bvh.gpu_ms = g.ms;
    return RT_OK;
}

int upload_scene(rt_scene* s)
{
    const auto& H = s->host;
    const int n = (int)H.size();
    // --- fast fp32 set: the brute-force orders (the grouped one cuts the scene's own tree)
    HostRecords rec = make_host_records(H, 0, group_max_default(), &s->sah, &s->bvh_outer);
    const std::vector<int>& xf_index = rec.xf_index;
    const std::vector<XformF>& xf = rec.xf;
    // --- exact fp64 set
    std::vector<PrimD> pd;
    std::vector<XformD> xd;
    make_exact_records(H, pd, xd);
    std::vector<float4> vn((size_t)std::max(1, n) * 3, make_float4(0, 0, 0, 0));
    for (int i = 0; i < n; i++)
        if (H[i].kind == RT_PRIM_TRIANGLE)
            for (int k = 0; k < 3; k++) vn[3 * i + k] = f4(H[i].vn[k], 0.0f);
    auto primf = [&](int i) { return make_primf(H, xf_index, i); };
    auto testrec = [&](int i) { return make_testrec(H, xf_index, i); };
    BruteOrders& orders = rec.orders;
    BruteOrder& flat = orders.flat;
    BruteOrder& grouped = orders.grouped;
    s->flat_overflow = flat.overflow;
    const int np = orders.np;
    s->layout = orders.layout;
    s->group_max = orders.group_max;
    // Materials, deduplicated (make_materials), and the scene facts
    const MatTable mt = make_materials(H, s->params.air_ior);
    const std::vector<MatF>& mats = mt.mats;
    const std::vector<int32_t>& mat_of = mt.mat_of;
    uint32_t facts = scene_facts(H);
    if (getenv("RTCORE_NO_FACTS")) facts = FACT_ALL; // A/B: every shading feature compiled in
    auto set_mats = [&](std::vector<PrimF>& v) { // PrimF.d.w = the material of the record's ID
        for (PrimF& f : v) {
            int32_t id;
            std::memcpy(&id, &f.a.w, 4);
            f.d.w = as_f(mat_of[id]);
        }
    };
    set_mats(flat.prims);
    set_mats(grouped.prims);
    // The BVH order: the tree's slots (host: s->sah.order; GPU: gathered on the device), then the
    // outer records' slots (their records renumbered past the tree), then the planes -- the tail,
    // built here for both builders.
    std::vector<PrimF> bv;
    std::vector<TestRec> tbv;
    const int n_tree = s->bvh.builder == RT_BVH_BUILDER_GPU
                           ? (s->order_d.n > 0 ? (int)s->order_d.n - np - 1 : 0)
                           : (int)s->sah.order.size();
    {
        BruteOrder& ob = orders.outer;
        if (!ob.groups.empty()) {
            const int n_slots = (int)ob.prims.size() - np;
            bv.insert(bv.end(), ob.prims.begin(), ob.prims.begin() + n_slots);
            tbv.insert(tbv.end(), ob.tests.begin(), ob.tests.begin() + n_slots);
            for (RectRec& r : ob.rects) r.sg += n_tree << 1;
            const GroupRec& G = ob.groups[0];
            for (int j = G.frame_first + G.n_frames; j < G.frame_first + G.n_frames + G.n_boxes; j++) {
                BoxRec B;
                std::memcpy(&B, &ob.frames[j], sizeof B);
                B.sg0 += n_tree << 1;
                std::memcpy(&ob.frames[j], &B, sizeof B);
            }
        }
        for (int i = 0; i < n; i++) // planes follow the BVH's primitives in both orders
            if (H[i].kind == RT_PRIM_PLANE) {
                bv.push_back(primf(i));
                tbv.push_back(testrec(i));
            }
    }
    const size_t n_bvh_records = (size_t)n_tree + bv.size();
    set_mats(bv);
    if (s->bvh.builder == RT_BVH_BUILDER_GPU) {
        // the tree's records in ID order, gathered on the device into the GPU builder's leaf order
        std::vector<PrimF> pid(n);
        std::vector<TestRec> tid(n);
        parallel_for(n, [&](int i) {
            pid[i] = primf(i);
            tid[i] = testrec(i);
        });
        DevBuf<PrimF> pid_d;
        DevBuf<TestRec> tid_d;
        set_mats(pid);
        HIP_TRY(pid_d.upload(pid));
        HIP_TRY(tid_d.upload(tid));
        HIP_TRY(s->bvh_d.prims.reserve(n_bvh_records));
        HIP_TRY(s->bvh_d.tests.reserve(n_bvh_records + kTestSpares));
        HIP_TRY(gather_bvh_records(s->order_d.p, n_tree, pid_d.p, tid_d.p, s->bvh_d.prims.p, s->bvh_d.tests.p, s->stream));
        if (!bv.empty()) {
            HIP_TRY(hipMemcpyAsync(s->bvh_d.prims.p + n_tree, bv.data(), bv.size() * sizeof(PrimF), hipMemcpyHostToDevice,
                                   s->stream));
            HIP_TRY(hipMemcpyAsync(s->bvh_d.tests.p + n_tree, tbv.data(), tbv.size() * sizeof(TestRec),
                                   hipMemcpyHostToDevice, s->stream));
        }
        // spare records: the BVH leaf step loads up to kTestSpares past a leaf
        HIP_TRY(hipMemsetAsync(s->bvh_d.tests.p + n_bvh_records, 0, kTestSpares * sizeof(TestRec), s->stream));
        HIP_TRY(hipStreamSynchronize(s->stream));
        s->order_d.release();
    } else {
        std::vector<PrimF> tree(n_tree);
        std::vector<TestRec> ttree(n_tree);
        parallel_for(n_tree, [&](int k) {
            tree[k] = primf(s->sah.order[k]);
            ttree[k] = testrec(s->sah.order[k]);
        });
        set_mats(tree);
        bv.insert(bv.begin(), tree.begin(), tree.end());
        tbv.insert(tbv.begin(), ttree.begin(), ttree.end());
    }
    HIP_TRY(s->prims_d.upload(pd));
    HIP_TRY(s->xf_d.upload(xd));
    HIP_TRY(s->flat_d.upload(flat));
    HIP_TRY(s->grouped_d.upload(grouped));
    s->groups_gr_host = grouped.groups;
    s->flat_h = {flat.groups, flat.rects, flat.frames, flat.tests};
    s->grouped_h = {grouped.groups, grouped.rects, grouped.frames, grouped.tests};
    s->xf_h = xf;
    if (s->bvh.builder != RT_BVH_BUILDER_GPU) {
        HIP_TRY(s->bvh_d.prims.upload(bv));
        tbv.resize(tbv.size() + kTestSpares, TestRec{}); // spare records: the BVH leaf step loads past a leaf
        HIP_TRY(s->bvh_d.tests.upload(tbv));
        HIP_TRY(s->nodes.upload(s->sah.nodes));
        HIP_TRY(s->nodes4.upload(s->bvh4.nodes));
    }
    if (!orders.outer.groups.empty()) {
        HIP_TRY(s->bvh_d.rects.upload(orders.outer.rects));
        HIP_TRY(s->bvh_d.frames.upload(orders.outer.frames));
        HIP_TRY(s->bvh_d.groups.upload(orders.outer.groups));
    }
    HIP_TRY(s->xf.upload(xf));
    HIP_TRY(s->mats.upload(mats));
    HIP_TRY(s->vnormals.upload(vn));
    s->device_bytes = pd.size() * sizeof(PrimD) + xd.size() * sizeof(XformD) +
                      (flat.prims.size() + grouped.prims.size() + n_bvh_records) * sizeof(PrimF) +
                      (flat.tests.size() + grouped.tests.size() + n_bvh_records + 1) * sizeof(TestRec) +
                      (size_t)s->bvh.n_nodes2 * sizeof(NodeF) + (size_t)s->bvh.n_nodes4 * sizeof(Node4Q) +
                      xf.size() * sizeof(XformF) + mats.size() * sizeof(MatF) + vn.size() * sizeof(float4);

    // Compact leaves: the BVH order's 48-B rows, and every leaf whose primitives share their kind and
    // test flags referenced as a compact leaf (RTCORE_COMPACT_LEAVES=0 keeps them generic, for A/B)
    {
        const char* e = getenv("RTCORE_COMPACT_LEAVES");
        const bool rewrite = !(e && e[0] == '0');
        const size_t n_rec = n_bvh_records + kTestSpares;
        HIP_TRY(s->rows_bvh.reserve(3 * n_rec));
        HIP_TRY(compact_leaves(s->bvh_d.tests.p, (int)n_rec, s->rows_bvh.p, s->nodes.p, s->bvh.n_nodes2, s->nodes4.p,
                               s->bvh.n_nodes4, rewrite, s->stream));
        HIP_TRY(hipStreamSynchronize(s->stream));
    }
    // Hot table: the first kHot wide nodes in breadth-first order from the root, their references
    // to each other rewritten to RT_HOT_BIT | hot index (the global tree is unchanged).
    std::vector<Node4Q> hot;
    int root4_hot = s->bvh.root4;
    {
        std::vector<Node4Q> all4((size_t)s->bvh.n_nodes4);
        if (!all4.empty())
            HIP_TRY(hipMemcpy(all4.data(), s->nodes4.p, all4.size() * sizeof(Node4Q), hipMemcpyDeviceToHost));
        s->bvh.leaves4 = s->bvh.compact4 = 0; // build statistics: the wide tree's leaves, compact ones
        for (const Node4Q& nd : all4)
            for (float f : {nd.c.z, nd.c.w, nd.d.x, nd.d.y}) {
                int32_t c;
                std::memcpy(&c, &f, 4);
                if (c < 0 && c != RT_NODE4_EMPTY) {
                    s->bvh.leaves4++;
                    s->bvh.compact4 += ((~c) & kLeafCompact) != 0;
                }
            }
        int k_hot = 64; // with the 16-entry LDS stack: 7 blocks x (16 + 4) KB per CU
        if (const char* e = getenv("RTCORE_HOT_NODES")) k_hot = std::max(0, std::min(1024, atoi(e)));
        if (k_hot > 0 && s->bvh.root4 >= 0 && s->bvh.n_nodes4 > 0) {
            std::vector<int> order{s->bvh.root4};
            std::unordered_map<int, int> slot_of{{s->bvh.root4, 0}};
            for (size_t q = 0; q < order.size() && (int)order.size() < k_hot; q++) {
                const Node4Q& nd = all4[order[q]];
                int32_t ch[4];
                std::memcpy(&ch[0], &nd.c.z, 4);
                std::memcpy(&ch[1], &nd.c.w, 4);
                std::memcpy(&ch[2], &nd.d.x, 4);
                std::memcpy(&ch[3], &nd.d.y, 4);
                for (int c : ch)
                    if (c >= 0 && (int)order.size() < k_hot && !slot_of.count(c)) {
                        slot_of[c] = (int)order.size();
                        order.push_back(c);
                    }
            }
            for (int g : order) {
                Node4Q nd = all4[g];
                float* refs[4] = {&nd.c.z, &nd.c.w, &nd.d.x, &nd.d.y};
                for (float* r : refs) {
                    int32_t c;
                    std::memcpy(&c, r, 4);
                    auto it = c >= 0 ? slot_of.find(c) : slot_of.end();
                    if (it != slot_of.end()) {
                        c = RT_HOT_BIT | it->second;
                        std::memcpy(r, &c, 4);
                    }
                }
                hot.push_back(nd);
            }
            root4_hot = RT_HOT_BIT | 0;
        }
    }
    HIP_TRY(s->hot4.upload(hot));

    DevScene& d = s->dev;
    d.hot4 = s->hot4.p;
    d.n_hot4 = (int)hot.size();
    d.root4_hot = root4_hot;
    d.tests_bf = s->flat_d.tests.p;
    d.tests_bvh = s->bvh_d.tests.p;
    d.rows_bvh = s->rows_bvh.p;
    d.rects_bf = s->flat_d.rects.p;
    d.frames_bf = s->flat_d.frames.p;
    d.prims_bf = s->flat_d.prims.p;
    d.groups_bf = s->flat_d.groups.p;
    d.tests_gr = s->grouped_d.tests.p;
    d.rects_gr = s->grouped_d.rects.p;
    d.frames_gr = s->grouped_d.frames.p;
    d.prims_gr = s->grouped_d.prims.p;
    d.groups_gr = s->grouped_d.groups.p;
    d.n_groups_gr = (int)grouped.groups.size();
    // slots before the planes, per order (open boxes add placeholder slots to the brute orders)
    d.pln0_bf = (int)flat.prims.size() - np;
    d.pln0_gr = grouped.prims.empty() ? 0 : (int)grouped.prims.size() - np;
    d.pln0_bvh = (int)n_bvh_records - np;
    d.rects_bvh = s->bvh_d.rects.p;
    d.frames_bvh = s->bvh_d.frames.p;
    d.groups_bvh = s->bvh_d.groups.p;
    d.n_outer = orders.outer.groups.empty() ? 0 : 1;
    for (int k = 0; k < 3; k++) d.n_rect[k] = orders.nr[k];
    d.n_tri = orders.nt;
    d.n_sph = orders.ns;
    d.n_pln = np;
    d.prims_bvh = s->bvh_d.prims.p;
    d.nodes = s->nodes.p;
    d.n_nodes = s->bvh.n_nodes2;
    d.root = s->bvh.root2;
    d.nodes4 = s->nodes4.p;
    d.n_nodes4 = s->bvh.n_nodes4;
    d.root4 = s->bvh.root4;
    d.xf = s->xf.p;
    d.mats = s->mats.p;
    d.vnormals = s->vnormals.p;
    d.n_mats = (int)mats.size();
    d.n_xf = (int)xf.size();
    d.facts = facts;
    d.n_vn = rec.n_vn;
    d.prims_d = s->prims_d.p;
    d.xf_d = s->xf_d.p;
    d.ref_nodes = nullptr; // built on first use (ensure_ref_bvh)
    d.n_ref_nodes = 0;
    d.width = s->params.width;
    d.height = s->params.height;
    d.recursion = s->params.recursion;
    d.debug_geom = s->params.debug_geom;
    d.air_ior = (float)s->params.air_ior;
    const rt_color& a = s->params.ambient;
    d.ambient = make_float3((float)a.r, (float)a.g, (float)a.b);
    d.ambient_miss = (a.r == -1 && a.g == -1 && a.b == -1) ? 1 : 0; // AmbientRGB == Placeholder
    d.bound = make_scene_bound(H);
    s->units = make_flat_units(H, orders.flat, d.bound, np, rec.n_vn);
    return RT_OK;
}

// The reference agglomerative BVH (BVH.cs:12-236) serves only the exact debug passes; it is built
// and uploaded on first use, so a render-only scene does not pay for it (5.8 s for 1 M triangles).
int ensure_ref_bvh(rt_scene* s)
{
    if (s->ref_built) return RT_OK;
    s->ref = build_ref_bvh(s->host);
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(s->ref_nodes.upload(s->ref.nodes));
    s->dev.ref_nodes = s->ref_nodes.p;
    s->dev.n_ref_nodes = (int)s->ref.nodes.size();
    s->device_bytes += s->ref.nodes.size() * sizeof(RefNode);
    s->ref_built = true;
    return RT_OK;
}

int resolve_traversal(rt_scene* s)
{
    int t = s->traversal;
    if (t == RT_TRAVERSAL_AUTO) {
        const int n_bvh = s->dev.pln0_bvh; // primitives other than planes
        t = n_bvh <= 48 ? RT_TRAVERSAL_BRUTE : RT_TRAVERSAL_BVH;
    }
    if (s->traversal == RT_TRAVERSAL_AUTO && t == RT_TRAVERSAL_BRUTE && s->grouped_measured > 1.25)
        t = RT_TRAVERSAL_GROUPED;
    if (t == RT_TRAVERSAL_GROUPED && s->dev.n_groups_gr == 0) t = RT_TRAVERSAL_BRUTE; // too big to group
    if (t == RT_TRAVERSAL_BRUTE && s->flat_overflow) {
        set_error("brute-force traversal: more than 65535 triangles or 32767 spheres in the flat order");
        return RT_ERR_ARG;
    }
    // kernel: 0 brute force, 1 grouped brute force, 2 BVH2 (24 + kStackOverflow stack entries),
    // 3 wide BVH (RT_WIDE_STACK + kStackOverflow)
    int kernel = t == RT_TRAVERSAL_GROUPED ? 1 : 0;
    if (t == RT_TRAVERSAL_BVH2) {
        if (s->bvh.depth2 >= 24 + kStackOverflow) {
            set_error("BVH2 deeper than the kernel's traversal stack");
            return RT_ERR_ARG;
        }
        kernel = 2;
    } else if (t == RT_TRAVERSAL_BVH) {
        if (s->bvh.stack4 > path_wide_stack() + kStackOverflow) {
            set_error("wide BVH needs a deeper traversal stack than the kernel's");
            return RT_ERR_ARG;
        }
        kernel = 3;
    }
    s->resolved = t;
    // Stage the shading records in LDS when that costs no occupancy (RTCORE_PATH_LDS=0/1 forces
    // the choice for A/B measurements).
    const size_t lds = path_lds_bytes(s->dev);
    const int plain = path_variant(kernel, false), staged = path_variant(kernel, true);
    const int occ_plain = path_blocks_per_cu(plain, path_dyn_lds(s->dev, plain), false, s->dev.n_vn > 0);
    const int occ_staged = lds <= 64 * 1024 ? path_blocks_per_cu(staged, path_dyn_lds(s->dev, staged), false, s->dev.n_vn > 0) : 0;
    // The scene-specialised build (rt_set_jit) is a build of the staged brute-force variant, and its
    // occupancy is its own: with it on, a brute-force order stays staged whenever the records fit.
    bool use_lds = occ_staged >= occ_plain || (kernel <= 1 && occ_staged > 0 && jit_enabled());
    if (const char* e = getenv("RTCORE_PATH_LDS")) use_lds = e[0] == '1' && occ_staged > 0;
    s->variant = use_lds ? staged : plain;
    s->blocks_per_cu = use_lds ? occ_staged : occ_plain;
    if (s->stats_on) s->stats_blocks_per_cu = path_blocks_per_cu(s->variant, path_dyn_lds(s->dev, s->variant), true, s->dev.n_vn > 0);
    return RT_OK;
}

// AUTO on a small scene: flat or grouped brute force?  Whether a group can be skipped depends on
// how coherent a wave's rays are, which the camera decides, so each camera is calibrated once:
// the grouped kernel's instrumented variant renders a fixed 64x64 tile at 2 spp and counts the
// primitive tests it actually made.  The choice is a function of scene, camera and that fixed
// sample only (no timing), so it is the same on every run.
int calibrate_grouping(rt_scene* s)
{
    s->grouped_measured = 0;
    if (s->traversal != RT_TRAVERSAL_AUTO || s->dev.n_groups_gr < 2) return RT_OK;
    const int n_bvh = s->dev.pln0_bvh; // primitives other than planes
    if (n_bvh > 48) return RT_OK;
    const int w = std::min(64, s->params.width), h = std::min(64, s->params.height);
    const int x0 = (s->params.width - w) / 2, y0 = (s->params.height - h) / 2;
    const int saved_variant = s->variant, saved_blocks = s->blocks_per_cu;
    const int variant = path_variant(1, false);
    s->variant = variant;
    s->blocks_per_cu = path_blocks_per_cu(variant, 0, true, s->dev.n_vn > 0);
    HIP_TRY(s->stats_buf.reserve(RT_STATS_COUNT));
    HIP_TRY(s->sum.reserve((size_t)3 * w * h));
    HIP_TRY(s->samples.reserve((size_t)w * h));
    HIP_TRY(s->misses.reserve((size_t)w * h));
    HIP_TRY(hipMemsetAsync(s->stats_buf.p, 0, RT_STATS_COUNT * sizeof(unsigned long long), s->stream));
    HIP_TRY(hipMemsetAsync(s->rays.p, 0, sizeof(unsigned long long), s->stream));
    const bool was_on = s->stats_on;
    const int was_blocks = s->stats_blocks_per_cu;
    s->stats_on = true;
    s->stats_blocks_per_cu = s->blocks_per_cu;
    PathParams p = make_params(s, x0, y0, w, h, 2, 0x5EEDull, 0);
    p.pool = 64; // one chunk per pool: the counts must not depend on the pool size
    set_item_order(p);
    p.batch = 0; // nor on which lanes share a wave: the probe deals its items as it always has
    int rc = run_path(s, p, s->rays.p, s->stream, false); // an internal probe: not in rt_kernel_times
    if (rc == RT_OK) rc = end_op(s, s->stream);
    s->stats_on = was_on;
    s->stats_blocks_per_cu = was_blocks;
    s->variant = saved_variant;
    s->blocks_per_cu = saved_blocks;
    if (rc != RT_OK) return rc;
    unsigned long long st[RT_STATS_COUNT], rays = 0;
    HIP_TRY(hipMemcpyAsync(st, s->stats_buf.p, sizeof st, hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipMemcpyAsync(&rays, s->rays.p, sizeof rays, hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    HIP_TRY(hipMemsetAsync(s->stats_buf.p, 0, RT_STATS_COUNT * sizeof(unsigned long long), s->stream));
    if (rays == 0) return RT_OK;
    // relative costs of a rect/triangle test, a sphere test and a group box test (instruction counts)
    const double flat = 20.0 * (n_bvh - s->dev.n_sph) + 30.0 * s->dev.n_sph;
    const double grouped = (15.0 * st[0] + 20.0 * st[1] + 30.0 * st[2]) / (double)rays; // st[0]: box tests made
    s->grouped_measured = flat / std::max(grouped, 1e-9);
    return resolve_traversal(s);
}

PathParams make_params(rt_scene* s, int x0, int y0, int w, int h, int spp, uint64_t seed, uint64_t base,
                       double chunk_npix)
{
    return make_params_for(s->variant >> 1, 0, 0, x0, y0, w, h, spp, seed, base, chunk_npix);
}

int check_tile(rt_scene* s, int x0, int y0, int w, int h)
{
    if (!s) {
        set_error("null scene");
        return RT_ERR_ARG;
    }
    if (!s->has_camera) {
        set_error("no camera set (rt_scene_set_camera)");
        return RT_ERR_STATE;
    }
    if (w <= 0 || h <= 0 || x0 < 0 || y0 < 0 || x0 + w > s->params.width || y0 + h > s->params.height) {
        set_error("tile outside the frame");
        return RT_ERR_ARG;
    }
    return RT_OK;
}

// The scene-specialised kernel (rt_jit.h) of the current brute-force variant, built on first use
// and again after a group-order change.  Returns 1 when it is to be launched, 0 to launch the
// generic kernel: JIT off, the instrumented kernel, a BVH or unstaged variant, or a failed build
// (the generic kernel computes the same; the failure is kept in s->jit.error).
static bool jit_eligible(const rt_scene* s)
{
    // Both brute-force orders (RTCORE_JIT_GROUPED=0 leaves the grouped one generic).  The grouped
    // order's group loop is unrolled by pragma: left to the compiler's heuristics it stayed a loop
    // over constant memory and ran slower than the generic kernel (die.txt 36.6 -> 37.9 ms);
    // unrolled, die.txt C3 36.6 -> 30.9 ms.
    const char* eg = getenv("RTCORE_JIT_GROUPED");
    const bool grouped_ok = !(eg && eg[0] == '0');
    return jit_enabled() && !s->stats_on &&
           (s->variant == path_variant(0, true) || (grouped_ok && s->variant == path_variant(1, true)));
}

int prepare_jit(rt_scene* s)
{
    const bool eligible = jit_eligible(s);
    if (!eligible) {
        s->jit.status = 0;
        return 0;
    }
    const bool grouped = s->variant == path_variant(1, true);
    const unsigned gen = s->jit_gen;
    if (s->jit.variant == s->variant && s->jit.gen == gen) { // built (or failed) already
        s->jit.status = s->jit.fn ? 1 : (s->jit.error.empty() ? 0 : -1);
        return s->jit.fn ? 1 : 0;
    }
    PathParams lp{};
    fill_launch(s->dev, s->variant, lp);
    const auto& B = grouped ? s->grouped_h : s->flat_h;
    // The grouped order's build carries the camera (its group order is per camera anyway); the flat
    // order's only the camera's kind and depth-of-field switch, so moving the camera among cameras
    // of one kind (MainWindow.cs:262-269 restarts the render with another scene camera) reuses the
    // build: the same header, no hiprtc build and no cache lookup.
    static const bool cam_in = getenv("RTCORE_JIT_CAMERA") && getenv("RTCORE_JIT_CAMERA")[0] == '1'; // A/B: round 3's form
    const std::string header =
        jit_scene_header(lp.scene, s->camf, grouped || cam_in, B.groups, B.rects, B.frames, B.tests, s->xf_h);
    if (s->jit.variant == s->variant && s->jit.fn && header == s->jit.header) {
        s->jit.gen = gen;
        s->jit.status = 1;
        s->jit.compile_ms = 0;
        s->jit.from_cache = true;
        return 1;
    }
    s->jit.error.clear();
    s->jit.variant = s->variant;
    s->jit.gen = gen;
    s->jit.header = header;
    if (s->jit.fn) jit_release(s->device, s->jit.fn); // launches still queued keep it: eviction syncs the device
    s->jit.fn = nullptr;
    if (const char* dump = getenv("RTCORE_JIT_DUMP")) { // inspection: the generated header of the last build
        if (FILE* f = fopen(dump, "w")) {
            fwrite(header.data(), 1, header.size(), f);
            fclose(f);
        }
    }
    JitKernel k;
    std::string err;
    if (!jit_kernel(s->device, header, grouped, k, err)) {
        s->jit.status = -1;
        s->jit.error = err;
        return 0;
    }
    int n = 0;
    if (hipModuleOccupancyMaxActiveBlocksPerMultiprocessor(&n, k.fn, 256, path_dyn_lds(s->dev, s->variant)) !=
            hipSuccess ||
        n < 1) {
        jit_release(s->device, k.fn); // the reference jit_kernel took: the module stays evictable
        (void)hipGetLastError();
        s->jit.status = -1;
        s->jit.error = "occupancy query of the scene-specialised kernel failed";
        return 0;
    }
    s->jit.fn = k.fn;
    s->jit.blocks_per_cu = n;
    s->jit.status = 1;
    s->jit.compile_ms = k.compile_ms;
    s->jit.from_cache = k.from_cache;
    return 1;
}

// A launch record into the next slot of the scene's ring (rt_scene::params_d), queued on `stream`.
int upload_params(rt_scene* s, const PathParams& p, hipStream_t stream, const PathParams** d_out)
{
    if (!s->params_h) {
        HIP_TRY(hipHostMalloc(&s->params_h, sizeof(PathParams) * rt_scene::kParamRing, hipHostMallocDefault));
        HIP_TRY(s->params_d.reserve(rt_scene::kParamRing));
    }
    const unsigned slot = s->params_next++ % rt_scene::kParamRing;
    hipEvent_t& sev = s->slot_ev[slot];
    if (sev) HIP_TRY(hipEventSynchronize(sev)); // the slot's previous upload has been read
    else HIP_TRY(hipEventCreateWithFlags(&sev, hipEventDisableTiming));
    s->params_h[slot] = p;
    HIP_TRY(hipMemcpyAsync(s->params_d.p + slot, s->params_h + slot, sizeof(PathParams), hipMemcpyHostToDevice, stream));
    HIP_TRY(hipEventRecord(sev, stream));
    *d_out = s->params_d.p + slot;
    return RT_OK;
}

// The block cull of a brute-force launch (block_cull.h): the record of p's window for the current
// camera from the scene's cache, built on a miss.  ent: the record to launch with, or null when the
// launch runs whole (the cull is off, or no block is dead); fresh: its words are new and still to be
// uploaded (run_path does that on the launch stream).  Camera and bound stay the same from launch to
// launch in real use -- a progressive render repeats one camera until the user moves it -- so the
// proof is done once per camera and window and a steady launch pays a cache lookup.
// Off for the instrumented and tracing instances, whose counters and records keep their meaning
// (rt_render_rays has a launcher of its own and never comes here), and below kCullMinBlocks blocks,
// so that a host which renders many small tiles (rt_render_tile per 64 x 64 tile) does not build a
// table per call: the build takes 12 ns per block on the host (0.39 ms for a 1080p frame, 0.09 ms for
// 4096 blocks, profiles/block_cull/README.md), once per camera and window; 4096 blocks (512 x 512
// pixels) is the size from which one of rt_render_tile's four column bands of a 1080p frame (8100
// blocks) and every larger launch is culled.  Read per launch, like RTCORE_SCENE_BOUND:
// RTCORE_BLOCK_CULL=0 turns it off, RTCORE_BLOCK_CULL_MIN=<blocks> sets the threshold.
constexpr int kCullMinBlocks = 4096;
// Both launch sets' path kernels have ended (host wait): before memory they may read is freed.
static int wait_sets_host(rt_scene* s)
{
    for (rt_scene::LaunchSet& l : s->sets)
        if (l.path_recorded) HIP_TRY(hipEventSynchronize(l.path_done));
    return RT_OK;
}

static int plan_block_cull(rt_scene* s, const PathParams& p, rt_scene::CullEntry*& ent, bool& fresh)
{
    ent = nullptr;
    fresh = false;
    if ((s->variant >> 1) >= 2 || s->stats_on || s->tracing) return RT_OK;
    if (const char* e = getenv("RTCORE_BLOCK_CULL"))
        if (atoi(e) == 0) return RT_OK;
    int min_blocks = kCullMinBlocks;
    if (const char* e = getenv("RTCORE_BLOCK_CULL_MIN")) min_blocks = std::max(1, atoi(e));
    const int n_blocks = p.n_pad / 64;
    if (n_blocks < min_blocks || p.blocks_x > 0xFFFF || n_blocks / p.blocks_x > 0xFFFF) return RT_OK; // (16-bit bx, by)
    const CullWindow win{p.x0, p.y0, p.w, p.h, p.band > 0 ? p.band : 0, p.band > 0 ? p.band_stride : 0,
                         p.band > 0 ? p.band_offset : 0};
    auto same = [](const CullWindow& a, const CullWindow& b) {
        return a.x0 == b.x0 && a.y0 == b.y0 && a.w == b.w && a.h == b.h && a.band == b.band &&
               a.band_stride == b.band_stride && a.band_offset == b.band_offset;
    };
    rt_scene::CullEntry* c = nullptr;
    for (rt_scene::CullEntry& e : s->cull_cache)
        if (e.valid && e.cam_gen == s->cam_gen && same(e.win, win)) c = &e;
    if (!c) {
        // replaced: an unused entry or one of an earlier camera first, else the least recently used
        auto age = [&](const rt_scene::CullEntry& e) { return e.valid && e.cam_gen == s->cam_gen ? e.used : 0; };
        c = &s->cull_cache[0];
        for (rt_scene::CullEntry& e : s->cull_cache)
            if (age(e) < age(*c)) c = &e;
        c->valid = false;
        // an entry is replaced and its record may be reallocated: a path kernel of either launch set,
        // queued on the set's own stream, may still read it (overlap_wait's cull_replaced case, waited
        // for here where the entry is chosen; a miss is rare, once per camera and window)
        const int wrc = wait_sets_host(s);
        if (wrc != RT_OK) return wrc;
        if (c->up) HIP_TRY(hipEventSynchronize(c->up)); // the previous upload has read the pinned words
        else HIP_TRY(hipEventCreateWithFlags(&c->up, hipEventDisableTiming));
        std::vector<unsigned char> dead;
        c->n_live = cull_blocks(s->camf, s->dev.bound, s->dev.n_pln, win, dead);
        c->n_blocks = n_blocks;
        c->dead_px = dead_pixels(win, dead);
        c->cam_gen = s->cam_gen;
        c->win = win;
        c->masks = false;
        if (c->n_live < n_blocks) {
            // the first bounce's unit masks (unit_masks, block_cull.h) after the two tables: they depend
            // on what the record depends on, and are cached with it
            std::vector<uint64_t> masks;
            c->masks = s->units.on && c->n_live > 0 &&
                       unit_masks(s->camf, s->dev.bound, s->units.n, s->units.lo.data(), s->units.hi.data(), win, dead, masks);
            const size_t masks_at = cull_masks_at((unsigned)c->n_live, (unsigned)n_blocks);
            const size_t words = c->masks ? masks_at + 2 * (size_t)c->n_live
                                          : (size_t)kCullTable + (size_t)c->n_live + (size_t)n_blocks;
            HIP_TRY(c->host.reserve(words));
            HIP_TRY(c->dev.reserve(words));
            unsigned int* h = c->host.p;
            h[0] = (unsigned)(c->dead_px & 0xFFFFFFFFull);
            h[1] = (unsigned)(c->dead_px >> 32);
            h[2] = (unsigned)c->n_live;
            h[3] = (unsigned)n_blocks;
            unsigned live = 0;
            for (int b = 0; b < n_blocks; b++) {
                if (!dead[(size_t)b]) h[kCullTable + live] = (unsigned)(b % p.blocks_x) | (unsigned)(b / p.blocks_x) << 16;
                h[kCullTable + c->n_live + b] = dead[(size_t)b] ? 0xFFFFFFFFu : live;
                live += dead[(size_t)b] ? 0u : 1u;
            }
            if (c->masks) {
                // (the word that aligns them, when there is one: otherwise that is the table's last entry)
                if (masks_at > (size_t)kCullTable + (size_t)c->n_live + (size_t)n_blocks) h[masks_at - 1] = 0;
                for (size_t i = 0; i < (size_t)c->n_live; i++) {
                    h[masks_at + 2 * i] = (unsigned)(masks[i] & 0xFFFFFFFFull);
                    h[masks_at + 2 * i + 1] = (unsigned)(masks[i] >> 32);
                }
            }
            fresh = true; // valid once the upload is queued (run_path)
        } else {
            c->valid = true; // nothing to cull for this camera and window: remembered, never launched with
        }
    }
    c->used = ++s->cull_clock;
    if (c->n_live < c->n_blocks) ent = c;
    return RT_OK;
}

// Launch the path kernel for p (work buffers sized here), timing it with the scene's events.
// may_overlap (rt_render_device, rt_render_bands_device): the launch runs on a launch set's own stream
// when launch_overlaps allows it (rt_scene::LaunchSet, launch_params.h: a launch that repeats the one
// before it in width, height and samples).  Launch k of these uses set k & 1.
// Its stream waits for the fold of the set's previous launch (fold_done, two launches ago), then runs what
// the caller's stream runs for a serial launch -- a fresh cull record's upload, the dispenser memset, a
// pixel-key rebuild, the parameter upload, the path kernel -- and records path_done; the caller's stream
// waits for path_done, and the caller queues the fold there.  The path kernel does not wait for the
// caller's stream: it reads and writes library-owned memory only (its rays go to the set's counter, which
// the fold moves into d_rays), so it starts as soon as the previous launch's last waves leave room.
// What both sets read -- pixel keys, cull records, the scene-specialised kernel -- is not rewritten
// while the other set's kernel can be in flight (overlap_wait), and a rewrite on one set's stream is
// waited for by the other's next launch (shared_ev).  Every other launch runs on `stream` with set 0's
// buffers: `stream` is behind both sets' folds (its own order, or done_ev), hence behind both path kernels.
int run_path(rt_scene* s, PathParams& p, unsigned long long* d_rays, hipStream_t stream, bool timed, bool may_overlap)
{
    s->open_set = -1;
    // A brute-force launch is planned over the blocks that can see the scene (block_cull.h): tickets,
    // item ranges, n_pad, the item total and the partial buffer over the n_live live blocks in their
    // original order.  Chunks, samples per item and pool stay the window's, so an item holds the same
    // samples, its fp32 partial has the same bits and the fixed-order fold gives the same fp64 sums;
    // the kernels that fold the partials (accumulate_kernel, colors_1spp_kernel) count a dead block's
    // pixels as spp primary misses, and the path kernel adds their rays (path_body).  The kernel is
    // launched even when no block is live, so rt_kernel_times keeps one event pair per launch.
    rt_scene::CullEntry* cull = nullptr;
    bool cull_fresh = false;
    p.cull = nullptr;
    const int crc = plan_block_cull(s, p, cull, cull_fresh);
    if (crc != RT_OK) return crc;
    if (cull) {
        set_blocks(p, cull->n_live);
        p.cull = cull->dev.p;
        if ((p.scene_bound & kFirstBounce) && cull->masks) p.scene_bound |= kFirstMasks;
    }
    const size_t need = (size_t)p.n_chunks * (size_t)p.n_pad;
    // 32-bit item indices: the end-of-work sentinel is `need` itself and a pool's end is at most
    // p.pool past it.  The dispensers count tickets, one per >= 64 items, and every wave draws once
    // more from each range it finds spent: with `need` in range a dispenser stays below 2^26 + waves.
    uint64_t tickets = 0;
    for (int g = 0; g < p.n_split; g++) tickets += p.split_tickets[g];
    if (need > 0xF0000000ull || tickets > need / 64) {
        set_error("tile x spp too large for one launch; split the tile");
        return RT_ERR_ARG;
    }
    const bool repeats = may_overlap && p.w == s->prev_w && p.h == s->prev_h && p.spp == s->prev_spp;
    if (may_overlap) s->prev_w = p.w, s->prev_h = p.h, s->prev_spp = p.spp;
    const bool overlap = may_overlap && timed && launch_overlaps(true, repeats, (s->variant >> 1) >= 2, s->stats_on, s->tracing, need * sizeof(float4));
    const int set = overlap ? (int)(s->overlapped & 1) : 0;
    rt_scene::LaunchSet& ls = s->sets[set];
    const hipStream_t st = overlap ? ls.stream : stream; // the path kernel's stream
    DevBuf<float4>& partial = set ? s->alt.partial : s->partial;
    DevBuf<unsigned int>& counter = set ? s->alt.counter : s->counter;
    DevBuf<float4>& starts = set ? s->alt.starts : s->starts;
    DevBuf<int>& stack_ovf = set ? s->alt.stack_ovf : s->stack_ovf;
    int grid = s->n_cu * (s->stats_on ? s->stats_blocks_per_cu : s->blocks_per_cu);
    const size_t stack_need = s->variant >= 4 ? (size_t)grid * 256 * kStackOverflow : 0;
    static const bool pkeys_on = !(getenv("RTCORE_PIXEL_KEYS") && getenv("RTCORE_PIXEL_KEYS")[0] == '0');
    const bool pkeys_use = (s->variant >> 1) < 2 && !s->stats_on && pkeys_on;
    const bool pkeys_rebuild = pkeys_use && (!s->pkeys_valid || s->pkeys_seed != p.seed);
    if (overlap) {
        // (a grown start-row buffer is seen below, once the grid is known: its reserve waits there)
        // (prepare_jit would look at the build again: a new variant or group order)
        const bool jit_stale = jit_eligible(s) && (s->jit.variant != s->variant || s->jit.gen != s->jit_gen);
        const OverlapChange change{pkeys_rebuild, cull && cull_fresh, false /* waited for in plan_block_cull */, jit_stale,
                                   need > partial.n || (size_t)(kMaxSplit * kSplitStride) > counter.n || stack_need > stack_ovf.n};
        // (The host waits are belt and braces: hipFree synchronises the device and a module's eviction
        // does too, which the serial path has always relied on; here the order is also written down.)
        const OverlapWait w = overlap_wait(change);
        rt_scene::LaunchSet& other = s->sets[set ^ 1];
        if (w == kOverlapHostWait) {
            const int wrc = wait_sets_host(s);
            if (wrc != RT_OK) return wrc;
            if (ls.fold_recorded) HIP_TRY(hipEventSynchronize(ls.fold_done)); // the fold reads the buffer that grows
        } else if (w == kOverlapStreamWait && other.path_recorded) {
            HIP_TRY(hipStreamWaitEvent(st, other.path_done, 0));
        }
        if (ls.fold_recorded) HIP_TRY(hipStreamWaitEvent(st, ls.fold_done, 0));
        if (ls.after_serial && s->any_op) HIP_TRY(hipStreamWaitEvent(st, s->done_ev, 0));
        if (ls.after_shared) HIP_TRY(hipStreamWaitEvent(st, s->shared_ev, 0));
        ls.after_serial = ls.after_shared = false;
    }
    HIP_TRY(partial.reserve(need));
    HIP_TRY(counter.reserve(kMaxSplit * kSplitStride));
    p.partial = partial.p;
    p.counter = counter.p;
    p.rays = overlap ? s->set_rays.p + set : d_rays;
    p.stats = s->stats_on ? (s->tracing ? s->trace_stats.p : s->stats_buf.p) : nullptr;
    // rt_debug_ray_log arms the next instrumented BVH launch only, so a buffer the caller frees
    // afterwards is never written (rt_trace_paths' launch is not one of them)
    p.ray_log = (s->stats_on && !s->tracing && s->variant >= 4) ? s->ray_log : nullptr;
    p.ray_log_n = s->ray_log_n;
    p.ray_log_cap = s->ray_log_cap;
    if (p.ray_log) s->ray_log = nullptr;
    // order after the previous operation when it ran on another stream (shared scratch; an overlapped
    // launch: the fold's order among the caller's streams)
    if (s->any_op && stream != s->last_stream) HIP_TRY(hipStreamWaitEvent(stream, s->done_ev, 0));
    bool shared_written = false;
    if (cull && cull_fresh) { // a new record: after the operations that read the entry's previous one
        const size_t words = cull->masks ? cull_masks_at((unsigned)cull->n_live, (unsigned)cull->n_blocks) + 2 * (size_t)cull->n_live
                                         : (size_t)kCullTable + (size_t)cull->n_live + (size_t)cull->n_blocks;
        HIP_TRY(hipMemcpyAsync(cull->dev.p, cull->host.p, words * sizeof(unsigned int), hipMemcpyHostToDevice, st));
        HIP_TRY(hipEventRecord(cull->up, st));
        cull->valid = true;
        shared_written = true;
    }
    HIP_TRY(hipMemsetAsync(p.counter, 0, sizeof(unsigned int) * kSplitStride * p.n_split, st));
    p.stack_ovf = nullptr;
    if (s->variant >= 4) { // BVH kernels: the stacks' global overflow area
        HIP_TRY(stack_ovf.reserve(stack_need));
        p.stack_ovf = stack_ovf.p;
    }
    const int jit = s->tracing ? 0 : prepare_jit(s); // (rt_trace_paths: the generic kernel, the build's state untouched)
    int jit_grid = jit ? s->n_cu * s->jit.blocks_per_cu : 0;
    // A small brute-force launch runs fewer blocks per CU.  Its time is a lane's serial chain of
    // samples (each a few dependent iterations), and an iteration takes as long as the waves sharing
    // a SIMD make it: with ~2 samples per lane (bounce.txt 256x256 x 16 spp on 8 blocks per CU) the
    // launch is all tail.  So the grid gives each lane at least kSamplesPerLane samples, up to the
    // occupancy the kernel allows.  Measured on that launch (profiles/r06/probe_grid.log, kernel ms):
    // 8 / 6 / 4 / 3 / 2 blocks per CU 0.205 / 0.191 / 0.165 / 0.156-0.161 / 0.163-0.164; the 1080p x 256
    // spp launch (1,157 samples per lane) stays at the full 8 (16.72-16.75 ms; 6: 17.11).  Which lane
    // renders an item never changes what it computes.  RTCORE_GRID_BPC caps it (tuning).
    if ((s->variant >> 1) < 2 && !s->stats_on) {
        constexpr double kSamplesPerLane = 6.0;
        // (a culled launch: the samples of the live blocks' pixels)
        const double samples = ((double)p.w * (double)p.h - (cull ? (double)cull->dead_px : 0.0)) * (double)p.spp;
        int cap = (int)std::ceil(samples / ((double)s->n_cu * 256.0 * kSamplesPerLane));
        if (const char* e = getenv("RTCORE_GRID_BPC")) cap = atoi(e);
        cap = std::max(1, cap);
        if (jit) jit_grid = s->n_cu * std::min(s->jit.blocks_per_cu, cap);
        else grid = s->n_cu * std::min(s->blocks_per_cu, cap);
    }
    const int tslot = (int)(s->launches % rt_scene::kTimeSlots);
    if (timed) HIP_TRY(hipEventRecord(s->t_start[tslot], st));
    fill_launch(s->dev, s->variant, p);
    // The brute-force kernels read each item's pixel key (two lowbias32 rounds of the seed key and
    // the frame pixel index, rtcore_rng.h) from a per-scene table, built here once per seed (a
    // ~10-us kernel on the launch stream): the same keys, without hashing in the loop.
    // RTCORE_PIXEL_KEYS=0 hashes per item (A/B).
    p.pkeys = nullptr;
    if (pkeys_use) {
        if (pkeys_rebuild) {
            HIP_TRY(s->pkeys.reserve((size_t)s->params.width * (size_t)s->params.height));
            HIP_TRY(launch_pixel_keys(p.seed_key, s->params.width, s->params.height, s->pkeys.p, st));
            s->pkeys_valid = true;
            s->pkeys_seed = p.seed;
            shared_written = true;
        }
        p.pkeys = s->pkeys.p;
    }
    // Start rows (plan_start_rows, launch_params.cpp): one row set per wave of the grid launched.
    p.starts = nullptr;
    p.start_rows = 0;
    const StartRowsPlan sr = plan_start_rows(s->variant >> 1, s->stats_on || s->tracing, s->dev.n_vn > 0, s->camf.kind,
                                             s->camf.dof != 0.0f, p.chunk, jit ? jit_grid : grid);
    if (sr.on) {
        if (overlap && sr.bytes / sizeof(float4) > starts.n && starts.n > 0) { // overlap_wait's buffer_grown case
            const int wrc = wait_sets_host(s); // (the set's previous kernel read the buffer that grows)
            if (wrc != RT_OK) return wrc;
        }
        HIP_TRY(starts.reserve(sr.bytes / sizeof(float4)));
        p.starts = starts.p;
        p.start_rows = sr.rows;
    }
    if (overlap && shared_written) { // the other set's next launch reads what this stream has just queued
        HIP_TRY(hipEventRecord(s->shared_ev, st));
        s->sets[set ^ 1].after_shared = true;
    }
    const PathParams* pa = nullptr;
    const int urc = upload_params(s, p, st, &pa);
    if (urc != RT_OK) return urc;
    if (jit) {
        const CameraF* ca = s->camf_d.p;
        void* args[] = {&ca, &pa};
        HIP_TRY(hipModuleLaunchKernel(s->jit.fn, jit_grid, 1, 1, 256, 1, 1,
                                      (unsigned)path_dyn_lds(s->dev, s->variant), st, args, nullptr));
    } else {
        HIP_TRY(launch_path(s->dev, s->camf_d.p, pa, s->variant, grid, st, s->stats_on));
    }
    if (timed) {
        HIP_TRY(hipEventRecord(s->t_end[tslot], st));
        s->launches++;
    }
    if (overlap) {
        HIP_TRY(hipEventRecord(ls.path_done, st));
        ls.path_recorded = true;
        HIP_TRY(hipStreamWaitEvent(stream, ls.path_done, 0));
        s->overlapped++;
        s->open_set = set;
    }
    return RT_OK;
}

// Marks the end of a render operation (path kernel + the kernel that consumed its partials).
int end_op(rt_scene* s, hipStream_t stream)
{
    HIP_TRY(hipEventRecord(s->done_ev, stream));
    s->last_stream = stream;
    s->any_op = true;
    if (s->open_set >= 0) { // an overlapped launch's fold: the set's next launch waits for it
        rt_scene::LaunchSet& ls = s->sets[s->open_set];
        HIP_TRY(hipEventRecord(ls.fold_done, stream));
        ls.fold_recorded = true;
        s->open_set = -1;
    } else { // a serial operation used set 0's buffers or rewrote shared state: both sets' next launches follow it
        for (rt_scene::LaunchSet& l : s->sets) l.after_serial = true;
    }
    return RT_OK;
}

int queue_copy(rt_scene* s, CopyPlan& plan, const void* d_src, size_t a, size_t b, size_t rec_bytes, int k,
               hipStream_t stream)
{
    k = std::max(1, std::min(k, rt_scene::kCopyChunks - plan.n));
    const size_t per = (b - a + k - 1) / k;
    for (int c = 0; c < k; c++) {
        const size_t ca = std::min(b, a + c * per), cb = std::min(b, a + (c + 1) * per);
        hipEvent_t& ev = s->copy_ev[plan.n];
        if (!ev) HIP_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        if (cb > ca)
            HIP_TRY(hipMemcpyAsync(s->stage.p + ca * rec_bytes, static_cast<const unsigned char*>(d_src) + ca * rec_bytes,
                                   (cb - ca) * rec_bytes, hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipEventRecord(ev, stream));
        plan.a[plan.n] = ca;
        plan.b[plan.n] = cb;
        plan.n++;
    }
    return RT_OK;
}

int consume_copies(rt_scene* s, const CopyPlan& plan, const std::function<void(const unsigned char*, size_t, size_t)>& consume)
{
    // chunks x S slices, handed out in order: the first tasks wait for the first chunk.  A slice
    // holds at least kMinItems records, so a small tile (a few thousand pixels) is consumed on the
    // calling thread instead of waking the pool for a few hundred records per thread.
    constexpr size_t kMinItems = 65536;
    size_t longest = 0;
    for (int k = 0; k < plan.n; k++) longest = std::max(longest, plan.b[k] - plan.a[k]);
    const size_t S = std::max<size_t>(1, std::min<size_t>((size_t)host_threads(), longest / kMinItems));
    std::atomic<int> failed{0};
    host_run((size_t)plan.n * S, [&](size_t t) {
        const size_t k = t / S, j = t % S;
        const size_t a0 = plan.a[k], b0 = plan.b[k];
        const size_t sl = (b0 - a0 + S - 1) / S;
        const size_t a = std::min(b0, a0 + j * sl), b = std::min(b0, a + sl);
        if (hipEventSynchronize(s->copy_ev[k]) != hipSuccess) {
            failed = 1;
            return;
        }
        if (b > a) consume(s->stage.p, a, b);
    });
    if (failed) {
        set_error("device -> host copy failed");
        return RT_ERR_HIP;
    }
    return RT_OK;
}

// n_items records of rec_bytes from d_src in up to kCopyChunks chunks of at least 1 MB.
int copy_consume(rt_scene* s, const void* d_src, size_t n_items, size_t rec_bytes,
                 const std::function<void(const unsigned char*, size_t, size_t)>& consume)
{
    const size_t bytes = n_items * rec_bytes;
    HIP_TRY(s->stage.reserve(bytes));
    CopyPlan plan;
    const int K = (int)std::max<size_t>(1, std::min<size_t>(rt_scene::kCopyChunks, bytes >> 20));
    int rc = queue_copy(s, plan, d_src, 0, n_items, rec_bytes, K, s->stream);
    if (rc != RT_OK) return rc;
    return consume_copies(s, plan, consume);
}

} // namespace rtc

extern "C" int rt_set_bvh_builder(int32_t builder)
{
    if (builder < RT_BVH_BUILDER_AUTO || builder > RT_BVH_BUILDER_GPU) {
        set_error("rt_set_bvh_builder: bad argument");
        return RT_ERR_ARG;
    }
    g_builder.store(builder);
    return RT_OK;
}
